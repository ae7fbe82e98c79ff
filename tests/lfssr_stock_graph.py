"""The LFSSR graph in stock torch ops (F.conv2d, F.pixel_shuffle), with optional rounding hooks on the operands the reduced-precision modes round: what the tests
of lfsr_set_ang_arithmetic emulate the HIP path with, and, under torch.autocast, their reduced-precision yardstick.

tests/lfssr_helpers.py::lfssr_layers states the same graph as shifted einsum products (the formula); tests/test_ang_arith_cpu.py holds the two equal to 1e-12 in
fp64.  Here the angular conv is a conv2d with padding 1 on (B h w, 64, A, A): the zero padding of the A x A grid is the skipped off-grid tap."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.lfssr_helpers import mosaic_to_views, views_to_mosaic


def r_bf16(t):
    """round to bf16, nearest even, once; the value back in t's dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def ang_conv2d(a, w, b, B, A, r_ang=None):
    """relu(angular 3x3 conv + bias) of per-view images a (B A^2, C, H, W), image (b A + u) A + v: a conv2d over (u, v) at every pixel, the first kernel axis on u;
    r_ang rounds both operands"""
    rnd = r_ang or (lambda t: t)
    n, c, H, W = a.shape
    g = a.reshape(B, A, A, c, H, W).permute(0, 4, 5, 3, 1, 2).reshape(B * H * W, c, A, A)
    o = torch.relu(F.conv2d(rnd(g), rnd(w), b, padding=1))
    return o.reshape(B, H, W, w.shape[0], A, A).permute(0, 4, 5, 3, 1, 2).reshape(n, w.shape[0], H, W)


def lfssr_stock(x, sd, A, s, dtype=torch.float64, n_layer=10, r_ang=None, r_conv=None):
    """SAI mosaic x (B, 1, A h, A w), state_dict of numpy arrays -> the SR mosaic (B, 1, A s h, A s w) in `dtype` (or what autocast makes of it).
    r_ang: applied to the activations (after the spatial conv's bias + ReLU) and the weight of every angular conv (LFSR_ANG_ARITH_BF16);
    r_conv: applied to the activations and the weight of every per-view 64 -> 64 and 64 -> 256 conv (LFSR_ARITH_BF16).
    conv0 (1 -> 64), res (64 -> 1) and iup (1 -> 4) take no hook."""
    rc = r_conv or (lambda t: t)
    p = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}
    x = torch.from_numpy(np.asarray(x)).to(dtype)
    B = x.shape[0]
    lo = mosaic_to_views(x, A)
    f = torch.relu(F.conv2d(lo, p["net.conv0.weight"], p["net.conv0.bias"], padding=1))
    for level in ("1", "2")[:1 if s == 2 else 2]:
        for i in range(n_layer):
            k = f"net.altblock{level}.{i}."
            a = torch.relu(F.conv2d(rc(f), rc(p[k + "spaconv.weight"]), p[k + "spaconv.bias"], padding=1))
            f = ang_conv2d(a, p[k + "angconv.weight"], p[k + "angconv.bias"], B, A, r_ang)
        f = torch.relu(F.pixel_shuffle(F.conv2d(rc(f), rc(p[f"net.fup{level}.0.weight"]), p[f"net.fup{level}.0.bias"], padding=1), 2))
        res = F.conv2d(f, p[f"net.res{level}.weight"], p[f"net.res{level}.bias"], padding=1)
        lo = res + F.pixel_shuffle(F.conv2d(lo, p[f"net.iup{level}.0.weight"], p[f"net.iup{level}.0.bias"], padding=1), 2)
    return views_to_mosaic(lo, B, A)
