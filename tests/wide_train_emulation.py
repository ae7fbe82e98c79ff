"""The LF_InterNet graph of tests/internet_stock_graph.py on leaf parameters the caller supplies, with the wide per-view 3x3 convs (the sixteen SpaConvSq and
BottleNeck.SpaBottle) replaced by an autograd function that rounds what lfsr_set_wide_train_arithmetic rounds: the CPU emulation the tests of that switch print
their forecast from, and, with no rounding and under torch.autocast, their fp64 reference and reduced-precision yardstick.

WideConv(t, w, A, r, fwd, wgrad, dgrad): relu(conv(t, w)) is formed outside; the function is the conv alone.
  fwd    the forward multiplies r(t) by r(w)                       (LFSR_WIDE_TRAIN_ARITH_BF16: csrc/conv3x3_wide_bf16.hip)
  wgrad  the weight gradient is conv2d_weight(r(t), r(dy))         (modes 1 and 2: csrc/wgrad_wide_bf16.hip)
  dgrad  the data gradient is conv2d_input(r(dy), r(w))            (not this switch: LFSR_GRAD_ARITH_BF16 on the 64 -> 64 slices)
Whatever a flag leaves out is exact in the graph's dtype: the data gradient of modes 1 and 2 uses the unrounded dy and w."""
import torch
import torch.nn.functional as F

from oracle.lfsr_torch_port import macpi2sai, sai2macpi

WIDE_KEYS = tuple(f"CascadeInterBlock.body.{g}.chained_layers.{l}.SpaConvSq.weight" for g in range(4) for l in range(4)) + ("BottleNeck.SpaBottle.weight",)
MODES = {0: (False, False, False), 1: (False, True, False), 2: (True, True, False)}      # lfsr_set_wide_train_arithmetic -> (fwd, wgrad, dgrad)


def r_bf16(t):
    """round to bf16, nearest even, once; the value back in t's dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


class WideConv(torch.autograd.Function):
    """per-view 3x3 conv, zero pad 1, of a MacPI t (B, cin, h A, w A) with w (64, cin, 3, 3): dilation A"""

    @staticmethod
    def forward(ctx, t, w, A, r, fwd, wgrad, dgrad):
        ctx.save_for_backward(t, w)
        ctx.cfg = (A, r, wgrad, dgrad)
        return F.conv2d(r(t), r(w), dilation=A, padding=A) if fwd else F.conv2d(t, w, dilation=A, padding=A)

    @staticmethod
    def backward(ctx, dy):
        t, w = ctx.saved_tensors
        A, r, wgrad, dgrad = ctx.cfg
        dw = torch.nn.grad.conv2d_weight(r(t), w.shape, r(dy), dilation=A, padding=A) if wgrad else torch.nn.grad.conv2d_weight(t, w.shape, dy, dilation=A, padding=A)
        dt = torch.nn.grad.conv2d_input(t.shape, r(w), r(dy), dilation=A, padding=A) if dgrad else torch.nn.grad.conv2d_input(t.shape, w, dy, dilation=A, padding=A)
        return dt, dw, None, None, None, None, None


def internet_graph(x, p, A, s, r=None, flags=(False, False, False), seen=None, n_groups=4, n_layers=4):
    """SAI mosaic x (B, 1, A h, A w) tensor, p: key -> leaf tensor -> the SR mosaic.  r is None: stock F.conv2d everywhere (what autocast sees);
    otherwise every wide conv is WideConv with r and the three flags.  seen: a list that receives the keys of the weights that went through WideConv"""
    def wide(t, key):
        if r is None:
            return F.relu(F.conv2d(t, p[key], dilation=A, padding=A))
        if seen is not None:
            seen.append(key)
        return F.relu(WideConv.apply(t, p[key], A, r, *flags))

    m = sai2macpi(x, A)
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
            ns = wide(torch.cat((bs, spa2), 1), k + "SpaConvSq.weight") + bs
            ba, bs = na, ns
        outs_a.append(ba)
        outs_s.append(bs)
    a = F.relu(F.conv2d(torch.cat(outs_a, 1), p["BottleNeck.AngBottle.weight"]))
    cs = torch.cat(outs_s + [F.pixel_shuffle(F.conv2d(a, p["BottleNeck.Ang2Spa.0.weight"]), A)], 1)
    out = wide(cs, "BottleNeck.SpaBottle.weight") + xs
    pre = F.conv2d(out, p["ReconBlock.PreConv.weight"], dilation=A, padding=A)
    return F.conv2d(F.pixel_shuffle(macpi2sai(pre, A), s), p["ReconBlock.FinalConv.weight"])


def step_grads(sd, x, label, A, s, dtype=torch.float64, r=None, flags=(False, False, False), seen=None, autocast=False):
    """one forward + L1 + backward on fresh leaves made from the numpy state_dict -> (output, {key: gradient as an fp64 numpy array})"""
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        y = internet_graph(torch.from_numpy(x).to(dtype), p, A, s, r, flags, seen)
        loss = F.l1_loss(y.to(dtype), torch.from_numpy(label).to(dtype))
    loss.backward()
    return y.detach(), {k: v.grad.double().numpy() for k, v in p.items()}
