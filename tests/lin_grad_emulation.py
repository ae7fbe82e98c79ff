"""Stock-torch emulation of lfsr_set_lin_grad_arithmetic(LFSR_LIN_GRAD_ARITH_BF16) on the CPU: the graphs of EPIT and LFT as tests/helpers.py states them (op for op
oracle/lfsr_torch_port.py), with every linear the mode computes replaced by a torch.autograd.Function whose forward is the plain product and whose backward rounds
dy, W and x (`rounding`, r_bf16 = .bfloat16()) before the two gradient products -- what csrc/lin_dgrad_bf16.hip and csrc/lin_wgrad_bf16.hip do, up to fp32
accumulation.  The linears are found by their weight: F.linear, and F.conv2d / F.conv3d with a 1 x 1 kernel, on (a slice of) one of the parameters is_mode_linear
names.  Everything else -- LFT's 576 -> 128 token embedding (MLP.weight: a 3x3 conv in the HIP path), the 3x3 convs, LayerNorm, attention -- is untouched.
tests/test_gpu_lin_grad_bf16.py records what this forecasts; tests/test_lin_grad_arith_cpu.py checks the patch itself."""
import contextlib

import torch
import torch.nn.functional as F

from lfsr_amd.synth import synth_input
from tests import helpers as TH

MODE_LINEARS = ("linear_in.weight", "linear_out.weight", "linear.0.weight", "in_proj_weight", "out_proj.weight", "feed_forward.1.weight", "feed_forward.4.weight",
                "upsampling.0.weight")


def is_mode_linear(key):
    return key.endswith(MODE_LINEARS)


def r_bf16(t):
    """the same values rounded to bf16 (nearest even), in t's dtype"""
    return t.float().bfloat16().to(t.dtype)


class RoundedGradLinear(torch.autograd.Function):
    """y = x W^T over the last axis of x; backward: dx = r(dy) r(W), dW = r(dy)^T r(x)"""

    @staticmethod
    def forward(ctx, x, w, r):
        ctx.save_for_backward(x, w)
        ctx.r = r
        return x @ w.t()

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        r = ctx.r
        dyr = r(dy)
        return dyr @ r(w), dyr.reshape(-1, dyr.shape[-1]).t() @ r(x).reshape(-1, x.shape[-1]), None


@contextlib.contextmanager
def emulate(params, rounding, seen=None):
    """inside the block the linears of `params` (name -> leaf tensor) that is_mode_linear names run through RoundedGradLinear; seen: receives their names"""
    names = {id(v): k for k, v in params.items() if is_mode_linear(k)}
    lin0, c20, c30 = F.linear, F.conv2d, F.conv3d

    def name_of(w):
        return names.get(id(w if w._base is None else w._base))

    def note(k):
        if seen is not None:
            seen.append(k)

    def linear(x, w, bias=None):
        k = name_of(w)
        if k is None or bias is not None:
            return lin0(x, w, bias)
        note(k)
        return RoundedGradLinear.apply(x, w, rounding)

    def conv(orig, nd):
        def f(x, w, *a, **kw):
            k = name_of(w)
            if k is None or a or kw or any(d != 1 for d in w.shape[2:]):
                return orig(x, w, *a, **kw)
            note(k)
            y = RoundedGradLinear.apply(x.movedim(1, -1), w.reshape(w.shape[0], w.shape[1]), rounding)
            return y.movedim(-1, 1)
        return f

    F.linear, F.conv2d, F.conv3d = linear, conv(c20, 2), conv(c30, 3)
    try:
        yield
    finally:
        F.linear, F.conv2d, F.conv3d = lin0, c20, c30


def port_grads(name, case, sd, x, dtype, rounding=None, seen=None, autocast=False):
    """-> {key: gradient (fp64 tensor)} of the L1 loss against synth_input(seed = 2) through the stock graph of `name` ("EPIT" | "LFT") with its own activation
    decisions: plain autograd in `dtype`; rounding: the mode's emulation; autocast: under torch.autocast("cpu", bfloat16) (the reference's reduced-precision path)"""
    A, s, B, h, w = case["A"], case["s"], case["B"], case["h"], case["w"]
    layers = {"EPIT": TH.epit_layers_fp64, "LFT": TH.lft_layers_fp64}[name]
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).to(dtype)
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
    ctx = emulate(p, rounding, seen) if rounding is not None else contextlib.nullcontext()
    with ctx, torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        y = layers(x, p, A, s, dtype=dtype)[0]
        loss = F.l1_loss(y.to(dtype), label)
    loss.backward()
    return {k: v.grad.double() for k, v in p.items()}
