"""The LF_InterNet graph in stock torch ops (F.conv2d on the MacPI, F.pixel_shuffle), with an optional rounding hook on the operands that
lfsr_set_wide_arithmetic(LFSR_WIDE_ARITH_BF16) rounds: what the tests of the mode emulate the HIP path with, and, under torch.autocast, their reduced-precision
yardstick.

oracle/lfsr_torch_port.py::internet_forward states the same graph; tests/test_wide_arith_cpu.py holds the two equal to 1e-12 in fp64.  The hook sees the
activations (the concatenated 128 or 320 channels) and the weight of the sixteen SpaConvSq and of BottleNeck.SpaBottle, and nothing else: not the residual, not
the angular branch, not SpaFE or the reconstruction."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.lfsr_torch_port import macpi2sai, sai2macpi


def r_bf16(t):
    """round to bf16, nearest even, once; the value back in t's dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def wide_conv(t, w, A, r_wide=None):
    """relu(per-view 3x3 conv, zero pad 1) of a MacPI t (B, cin, h A, w A): dilation A; r_wide rounds both operands"""
    rnd = r_wide or (lambda v: v)
    return F.relu(F.conv2d(rnd(t), rnd(w), dilation=A, padding=A))


def internet_stock(x, sd, A, s, dtype=torch.float64, n_groups=4, n_layers=4, r_wide=None):
    """SAI mosaic x (B, 1, A h, A w), state_dict of numpy arrays -> the SR mosaic (B, 1, A s h, A s w) in `dtype` (or what autocast makes of it)"""
    p = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}
    m = sai2macpi(torch.from_numpy(np.asarray(x)).to(dtype), A)
    xa = F.conv2d(m, p["AngFE.0.weight"], stride=A)
    xs = F.conv2d(m, p["SpaFE.0.weight"], dilation=A, padding=A)
    ba, bs = xa, xs
    outs_a, outs_s = [], []
    for g in range(n_groups):
        for l in range(n_layers):
            k = f"CascadeInterBlock.body.{g}.chained_layers.{l}."
            ang2 = F.relu(F.conv2d(bs, p[k + "Spa2Ang.weight"], stride=A))
            spa2 = F.pixel_shuffle(F.conv2d(ba, p[k + "Ang2Spa.0.weight"]), A)
            na = F.relu(F.conv2d(torch.cat((ba, ang2), 1), p[k + "AngConvSq.weight"])) + ba
            ns = wide_conv(torch.cat((bs, spa2), 1), p[k + "SpaConvSq.weight"], A, r_wide) + bs
            ba, bs = na, ns
        outs_a.append(ba)
        outs_s.append(bs)
    a = F.relu(F.conv2d(torch.cat(outs_a, 1), p["BottleNeck.AngBottle.weight"]))
    cs = torch.cat(outs_s + [F.pixel_shuffle(F.conv2d(a, p["BottleNeck.Ang2Spa.0.weight"]), A)], 1)
    out = wide_conv(cs, p["BottleNeck.SpaBottle.weight"], A, r_wide) + xs
    pre = F.conv2d(out, p["ReconBlock.PreConv.weight"], dilation=A, padding=A)
    return F.conv2d(F.pixel_shuffle(macpi2sai(pre, A), s), p["ReconBlock.FinalConv.weight"])
