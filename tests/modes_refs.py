"""The CPU reference legs of tests/test_gpu_modes_geometries.py: for each of the four trainable models at an arbitrary (A, s, B, h, w), the stock graph's output and
the gradients of one L1 step in fp64, the same under torch.autocast("cpu", bfloat16) (the reference's own reduced-precision path: the yardstick of every gate), and a
CPU emulation of the gradient switches inside the same graph.

The graphs are the ones the per-switch tests already differentiate at the golden tags -- tests/helpers.py:epit_layers_fp64 / lft_layers_fp64 (what
tests/lin_grad_emulation.py:port_grads runs), tests/wide_train_emulation.py:internet_graph (step_grads) and oracle/lfsr_torch_port.py:distgssr_forward_graph
(tests/test_gpu_grad_bf16.py:_distg_refs) -- on fresh leaves made the same way, so that at a tag the numbers are theirs bit for bit
(tests/test_modes_refs_cpu.py asserts it).

Emulation of leg G (LFSR_GRAD_ARITH_BF16 + LFSR_LIN_GRAD_ARITH_BF16 + LFSR_BRANCH_GRAD_ARITH_BF16 + LFSR_WIDE_TRAIN_ARITH_BF16_WGRAD): the forward is the stock
one in fp64, so every activation decision is fp64's own; in the backward
  the 64 -> 64 3x3 convs (weights (64, 64, 3, 3) and (64, 64, 1, 3, 3))      dx = conv_input(r(w), r(dy)), dw = conv_weight(r(x), r(dy))       Conv64, here
  the linears of EPIT and LFT                                                lin_grad_emulation.emulate
  EPIConv.0 of DistgSSR where the EPI-line kernels cover the pass            branch_grad_emulation.distg_graph
  LF_InterNet's wide convs                                                   wide_train_emulation.WideConv, weight and data gradient rounded (the data
                                                                             gradient is LFSR_GRAD_ARITH_BF16 on the 64 -> 64 slices)
round their operands to bf16 (r) and sum in fp64.  It shares no code with the HIP library.  `fault=` plants a lost LeakyReLU' mask in one conv's data gradient
(tests/test_modes_refs_cpu.py: what the per-parameter gate is there to catch)."""
import contextlib
import functools
import time

import numpy as np
import torch
import torch.nn.functional as F

from lfsr_amd.synth import synth_input
from oracle import lfsr_torch_port as TP
from tests import branch_grad_emulation as BG
from tests import helpers as TH
from tests import lin_grad_emulation as LG
from tests import wide_train_emulation as WT

MODELS = ("EPIT", "LFT", "LF_InterNet", "DistgSSR")
EMULATION_MAX_VIEW_PIXELS = 3000        # tests/test_modes_refs_cpu.py runs the emulation on the rows below this many view pixels

# (A, s, B, h, w) per model.  EPIT and LFT: their fp32 matrices (tests/helpers.py states each row's reason) without the published B = 8 geometry.
ROWS = {
    "EPIT": TH.EPIT_MATRIX[:-1],
    "LFT": TH.LFT_MATRIX[:-1],
    "LF_InterNet": (
        (7, 2, 1, 5, 6),        # 49 gather taps; 30 LR pixels: the angular squeeze far below the 2048 rows of lfsr_linear_run, nothing reads LFSR_GEMM_ARITH_BF16
        (2, 3, 2, 9, 7),        # even A, scale 3, odd ragged views, a batch boundary in the wide convs' tiles
        (4, 4, 1, 6, 5),        # even A, scale 4
        (5, 3, 2, 13, 16),      # the benchmark's angRes at scale 3; 416 LR pixels
        (9, 2, 1, 4, 4),        # largest accepted angRes; views of one 4x4 tile
        (1, 2, 2, 8, 8),        # one view: the wide convs and their 64 -> 64 data-gradient slices on B images only
        (2, 2, 2, 32, 33)),     # 2112 LR pixels, 8448 view pixels: the smallest row whose 128 -> 64 angular squeeze passes the 2048-row threshold, ragged against
    #                             2048 and against the batch boundary at 1056; w = 33 is past the 32-pixel tile of the wide convs
    "DistgSSR": (
        (5, 3, 2, 13, 16),      # every mode covers it: scale 3, ragged lines, a batch boundary
        (5, 2, 1, 33, 6),       # vertical lines of 33: the fused block tail (and with it the branch mode) is not taken, the EPIConv.0 bf16 gradients cover the
        #                         horizontal pass only (data gradient; the merged weight gradient declines)
        (5, 4, 1, 6, 33),       # the transpose of the row above, at scale 4
        (7, 2, 1, 5, 6),        # A != 5: only the conv modes are live, the branch modes change no bit
        (3, 3, 1, 13, 16),      # A = 3 at scale 3, odd h
        (1, 3, 2, 9, 7),        # one view
        (2, 3, 2, 9, 7)),       # even A: forward only, the backward refuses
}
_CASE = {"EPIT": TH.epit_case, "LFT": TH.lft_case, "LF_InterNet": TH.internet_case, "DistgSSR": TH.distg_case}


def has_backward(model, geom):
    return not (model == "DistgSSR" and geom[0] % 2 == 0)


def view_pixels(geom):
    A, s, B, h, w = geom
    return B * A * A * h * w


def case(model, geom):
    """-> state_dict, input, training label (numpy fp32): synth seeds 0 / 1 / 2, as the golden cases and every per-switch whole-model test"""
    A, s, B, h, w = geom
    sd, x = _CASE[model](*geom)
    return sd, x, synth_input((B, 1, A * h * s, A * w * s), seed=2)


def r_bf16(t):
    """the same values rounded to bf16 (nearest even) as the library rounds fp32 operands, in t's dtype"""
    return t.float().bfloat16().to(t.dtype)


class Conv64(torch.autograd.Function):
    """a stride-1 conv (2-D or 3-D) whose forward is the stock one and whose backward rounds dy, w and x before the two gradient products"""

    @staticmethod
    def forward(ctx, x, w, orig, nd, r, kw, unmask=None):
        ctx.save_for_backward(x, w)
        ctx.cfg = (nd, r, kw, unmask)
        return orig(x, w, **kw)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        nd, r, kw, unmask = ctx.cfg
        g = torch.nn.grad
        d_in, d_w = (g.conv2d_input, g.conv2d_weight) if nd == 2 else (g.conv3d_input, g.conv3d_weight)
        dyr = r(dy)
        dx = d_in(x.shape, r(w), dyr, **kw)
        if unmask is not None:      # a planted fault (tests/test_modes_refs_cpu.py): the LeakyReLU' mask in front of this conv is lost in every fourth channel --
            dx = dx.clone()         # x is that LeakyReLU's output, autograd multiplies dx by (x > 0 ? 1 : slope) next, so the factor is undone here
            dx[:, 3::4] = torch.where(x[:, 3::4] > 0, dx[:, 3::4], dx[:, 3::4] / unmask)
        return dx, d_w(r(x), w.shape, dyr, **kw), None, None, None, None, None


def is_conv64(shape):
    return tuple(shape) in ((64, 64, 3, 3), (64, 64, 1, 3, 3))


@contextlib.contextmanager
def emulate_conv64(params, r, seen=None, fault=None):
    """inside the block every F.conv2d / F.conv3d on one of the 64 -> 64 3x3 leaves of `params` runs through Conv64; seen: receives their names.  Wraps whatever
    F.conv2d / F.conv3d are at entry (lin_grad_emulation.emulate's patch, entered first, stays in the chain).  fault: (name, slope, call) -- the call-th use of that
    conv, which reads a LeakyReLU(slope) output, loses the mask in every fourth channel of its data gradient (Conv64.backward)"""
    names = {id(v): k for k, v in params.items() if is_conv64(v.shape)}
    c20, c30 = F.conv2d, F.conv3d
    calls = {}

    def conv(orig, nd):
        def f(x, w, *a, **kw):
            k = names.get(id(w))
            if k is None or a or set(kw) - {"padding", "dilation"}:
                return orig(x, w, *a, **kw)
            if seen is not None:
                seen.append(k)
            calls[k] = calls.get(k, 0) + 1
            hit = fault is not None and fault[0] == k and fault[2] == calls[k] - 1
            return Conv64.apply(x, w, orig, nd, r, kw, fault[1] if hit else None)
        return f

    F.conv2d, F.conv3d = conv(c20, 2), conv(c30, 3)
    try:
        yield
    finally:
        F.conv2d, F.conv3d = c20, c30


def graph(model, xt, p, A, s, dtype, r=None, seen=None):
    """the stock graph of `model` on the leaves p -> the SR mosaic; r: with leg G's emulation (call inside emulated(), which patches what the graph cannot be told)"""
    if model == "EPIT":
        return TH.epit_layers_fp64(xt, p, A, s, dtype=dtype)[0]
    if model == "LFT":
        return TH.lft_layers_fp64(xt, p, A, s, dtype=dtype)[0]
    if model == "LF_InterNet":
        return WT.internet_graph(xt, p, A, s) if r is None else WT.internet_graph(xt, p, A, s, r, (False, True, True), seen)
    if model == "DistgSSR":
        return TP.distgssr_forward_graph(xt, p, A, s) if r is None else BG.distg_graph(xt, p, A, s, r=r, seen=seen)
    raise KeyError(model)


@contextlib.contextmanager
def emulated(model, p, r, seen=None, fault=None):
    with contextlib.ExitStack() as st:
        if r is not None:
            if model in ("EPIT", "LFT"):
                st.enter_context(LG.emulate(p, r, seen))
            st.enter_context(emulate_conv64(p, r, seen, fault))
        yield


def step_grads(model, geom, sd, x, label, dtype=torch.float64, autocast=False, r=None, seen=None, fault=None):
    """one forward + L1 + backward of the stock graph on fresh leaves made from the numpy state_dict -> (output, {key: gradient}), fp64 numpy arrays"""
    A, s = geom[0], geom[1]
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
    with emulated(model, p, r, seen, fault), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        y = graph(model, torch.from_numpy(x).to(dtype), p, A, s, dtype, r, seen)
        loss = F.l1_loss(y.to(dtype), torch.from_numpy(label).to(dtype))
    loss.backward()
    return y.detach().double().numpy(), {k: v.grad.double().numpy() for k, v in p.items()}


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def flat(g, names):
    return np.concatenate([np.asarray(g[k], np.float64).reshape(-1) for k in names])


@functools.lru_cache(maxsize=None)
def refs(model, geom):
    """-> dict: sd, x, label, names (state_dict order), y64 / y_amp (outputs), g64 / g_amp (gradients), e_amp_out (rms), e_amp (per parameter rel-L2), e_amp_bucket,
    seconds (host time of the two legs).  Computed once per row, shared between tests, never written to; at most 16 torch threads"""
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    sd, x, label = case(model, geom)
    names = list(sd)
    t0 = time.time()
    y64, g64 = step_grads(model, geom, sd, x, label)
    y_amp, g_amp = step_grads(model, geom, sd, x, label, dtype=torch.float32, autocast=True)
    return {"sd": sd, "x": x, "label": label, "names": names, "y64": y64, "y_amp": y_amp, "g64": g64, "g_amp": g_amp, "e_amp_out": rms(y_amp, y64),
            "e_amp": {k: rel_l2(g_amp[k], g64[k]) for k in names}, "e_amp_bucket": rel_l2(flat(g_amp, names), flat(g64, names)), "seconds": time.time() - t0}


@functools.lru_cache(maxsize=None)
def emulation(model, geom):
    """-> ({parameter: rel-L2 of leg G's emulation against fp64 autograd}, the names that went through an emulated operator, the flat bucket's rel-L2)"""
    ref = refs(model, geom)
    seen = []
    _, g = step_grads(model, geom, ref["sd"], ref["x"], ref["label"], r=r_bf16, seen=seen)
    return {k: rel_l2(g[k], ref["g64"][k]) for k in ref["names"]}, sorted(set(seen)), rel_l2(flat(g, ref["names"]), flat(ref["g64"], ref["names"]))
