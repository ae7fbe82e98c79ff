"""GPU: lfsr_set_grad_arithmetic(LFSR_GRAD_ARITH_BF16) -- the data gradient (csrc/conv3x3_bf16_dgrad.hip) and the weight gradient (csrc/wgrad_bf16.hip) of the
64 -> 64 per-view 3x3 conv on bf16-rounded operands, fp32 accumulation; everything else, the forward included, as it was.

Operator gates: against the fp64 gradient of the SAME rounded operands (torch.Tensor.bfloat16()) a kernel differs by fp32 accumulation only: max|err| < 1e-4
(the suite's ATOL) for the data gradient, rel-L2 <= 1e-4 for the weight gradient (CPU emulation of fp32 accumulation over rounded operands: <= 1.1e-6).
Whole-model gates (DistgSSR): every parameter's rel-L2 error against fp64 autograd not above that of the reference's own reduced-precision path, the torch port
under torch.autocast("cpu", bfloat16), margin 1.0x (CPU emulation of the mode: >= 3.2x inside on all 137 tensors); with the bf16 forward as well only the flat
bucket is gated (emulation: 1.44x / 1.67x inside, single tensors within 1.05x).  The other three drivers share the data-gradient dispatcher: their gradients
move, stay finite, and stay within 5e-2 rel-L2 of the default's bucket (rounding alone: 2.35e-3 sqrt(depth) <= 1.4e-2; a wrong mask or tap order gives O(1)).
That distance cannot see a fault in a single layer (a mask lost in one conv moves the bucket by ~6e-3: tests/test_modes_refs_cpu.py); the fp64 gate per parameter
for those three drivers, across geometry rows, is tests/test_gpu_modes_geometries.py::test_training_step (leg G)."""
import contextlib
import functools
import importlib
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lfsr_amd import capi
from lfsr_amd.synth import synth_input
from oracle import lfsr_torch_port as TP
from tests import helpers as TH

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)   # the CPU reference legs run tiny convs
ATOL = 1e-4
SENTINEL = -2.0 ** 100
BAND = 1 << 16
E_ARG = -1


@contextlib.contextmanager
def grad_arithmetic(mode):
    """lfsr_set_grad_arithmetic(mode) for the block, the default again after it (the setting is process-wide)"""
    capi.set_grad_arithmetic(mode)
    try:
        yield
    finally:
        capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT)


def P(t):
    return capi.dev_ptr(t)


def rows(t):
    """(n, C, h, w) -> VCL rows (n h w, C) at A = 1, on the CPU"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def r16(t):
    """the same values rounded to bf16 (nearest even), as fp64"""
    return t.float().bfloat16().double()


GEOMS = [(1, 5, 8, 8),        # one ragged tile per view
         (2, 3, 6, 8),
         (3, 2, 5, 7),        # smaller than a tile both ways
         (2, 1, 37, 70),      # several ragged tile rows and columns
         (5, 4, 32, 32)]      # 320 tiles: more than one persistent round, the weight gradient's accumulators carry over tiles


@functools.lru_cache(maxsize=None)
def case(B, A, h, w):
    """operands (randn seeds 1 / 2 / 3, weights x 0.05) and the fp64 gradients of the bf16-ROUNDED and of the exact operands, computed once per geometry"""
    n = B * A * A
    dy = torch.randn(n, 64, h, w, generator=torch.Generator().manual_seed(1))
    wt = torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(2)) * 0.05
    x = torch.randn(n, 64, h, w, generator=torch.Generator().manual_seed(3))      # the conv's input (weight gradient); also the skip gradient / saved activation
    out = {"n": n, "dy": dy, "wt": wt, "x": x}
    for tag, f in (("r", r16), ("e", lambda t: t.double())):
        out["dx_" + tag] = torch.nn.grad.conv2d_input((n, 64, h, w), f(wt), f(dy), padding=1)
        out["dw_" + tag] = torch.nn.grad.conv2d_weight(f(x), (64, 64, 3, 3), f(dy), padding=1)
    return out


@pytest.mark.parametrize("B,A,h,w", GEOMS)
def test_data_gradient_is_the_exact_form_on_rounded_operands(B, A, h, w):
    c = case(B, A, h, w)
    n, dyv, xv = c["n"], rows(c["dy"]).cuda(), rows(c["x"]).cuda()
    wT = capi.pack_conv_weight_T(c["wt"].cuda())
    with grad_arithmetic(capi.GRAD_ARITH_BF16):
        d1 = capi.conv3x3_dgrad(dyv, wT, n, h, w)
        d2 = capi.conv3x3_dgrad(dyv, wT, n, h, w, res1=xv, act=xv, act_slope=0.1)
        torch.cuda.synchronize()
    ref1 = rows(c["dx_r"])
    ref2 = rows(c["dx_r"] * torch.where(c["x"] > 0, 1.0, 0.1).double() + c["x"].double())
    errs = [float((d1.cpu().double() - ref1).abs().max()), float((d2.cpu().double() - ref2).abs().max())]
    print(f"bf16 dgrad {(B, A, h, w)}: max|hip - fp64(rounded operands)| plain {errs[0]:.2e}, mask + residual {errs[1]:.2e}")
    assert max(errs) < ATOL, errs
    # (the two-residual row of the dispatcher has no operator entry point: DistgSSR's backward runs it, test_distgssr_whole_model)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("B,A,h,w", GEOMS)
def test_weight_gradient_is_the_exact_form_on_rounded_operands(B, A, h, w, accumulate):
    c = case(B, A, h, w)
    n, dyv, xv = c["n"], rows(c["dy"]).cuda(), rows(c["x"]).cuda()
    lib, st = capi.load(), capi.stream_ptr()
    n_ws = lib.lfsr_conv3x3_wgrad_workspace_floats(n, h, w)
    with grad_arithmetic(capi.GRAD_ARITH_BF16):
        assert lib.lfsr_conv3x3_wgrad_workspace_floats(n, h, w) == n_ws       # the workspace does not depend on the mode
        ws = torch.full((n_ws + BAND,), SENTINEL, device="cuda")
        dw0 = torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(5)) if accumulate else torch.full((64, 64, 3, 3), SENTINEL)
        dw = dw0.cuda()
        rc = lib.lfsr_conv3x3_wgrad(P(dyv), 64, 0, P(xv), 64, 0, P(dw), P(ws), n_ws, n, h, w, accumulate, st)
        torch.cuda.synchronize()
    assert rc == 0 and bool((ws[n_ws:] == SENTINEL).all())
    ref = c["dw_r"] + (dw0.double() if accumulate else 0.0)
    e = rel(dw, ref)
    print(f"bf16 wgrad {(B, A, h, w)} accumulate {accumulate}: rel-L2 vs fp64(rounded operands) {e:.2e}")
    assert bool(torch.isfinite(dw).all()) and e <= 1e-4


def test_it_really_is_bf16_and_the_default_is_untouched():
    B, A, h, w = GEOMS[0]
    c = case(B, A, h, w)
    n, dyv, xv = c["n"], rows(c["dy"]).cuda(), rows(c["x"]).cuda()
    wT = capi.pack_conv_weight_T(c["wt"].cuda())
    ops = {"dgrad": (lambda: capi.conv3x3_dgrad(dyv, wT, n, h, w), rows(c["dx_r"]), rows(c["dx_e"])),
           "wgrad": (lambda: capi.conv3x3_wgrad(dyv, xv, n, h, w), c["dw_r"], c["dw_e"])}
    for name, (f, ref_r, ref_e) in ops.items():
        before = f().clone()
        with grad_arithmetic(capi.GRAD_ARITH_BF16):
            got = f().clone()
        assert capi.get_grad_arithmetic() == capi.GRAD_ARITH_DEFAULT
        after = f().clone()
        torch.cuda.synchronize()
        d_def, d_r, d_e = rel(got, before), rel(got, ref_r), rel(got, ref_e)
        print(f"bf16 {name}: rel-L2 to the default {d_def:.2e}, to fp64 of rounded operands {d_r:.2e}, to fp64 of the operands {d_e:.2e}")
        assert d_def > 1e-3, name                       # the rounding alone is 2.35e-3
        assert d_r < d_e, name
        assert torch.equal(before, after), name         # the default's bits, before and after a round trip through the mode
        assert rel(before, ref_e) <= 1e-4, name


@functools.lru_cache(maxsize=None)
def ragged_case():
    n, h, w = 3, 30, 29
    g = torch.Generator().manual_seed(41)
    return n, h, w, torch.randn(n, 64, h, w, generator=g), torch.randn(64, 64, 3, 3, generator=g) * 0.05, torch.randn(n, 64, h, w, generator=g)


def _embed(r, stride, choff, seed):
    buf = torch.randn(r.shape[0] + 1, stride, generator=torch.Generator().manual_seed(seed))      # (one sentinel row behind the last pixel)
    buf[:r.shape[0], choff:choff + 64] = r
    return buf.cuda()


def _dgrad(lib, dyb, dys, dyo, wT, out, os_, oo, r1, r1s, r1o, act, as_, ao, n, h, w):
    return lib.lfsr_conv3x3_dgrad(P(dyb), dys, dyo, P(wT), P(out), os_, oo, P(r1), r1s, r1o, P(act), as_, ao, 0.1, n, h, w, capi.stream_ptr())


def test_strided_data_gradient_and_untouched_memory():
    """dx in channels [64, 128) of a 144-float row, dy at channel offset 16 of an 80-float row, r1 / act at offsets 8 / 4 of 72-float rows, ragged 30 x 29 views:
    every float outside the 64 output channels and a sentinel row behind the last pixel keep their bits"""
    n, h, w, dy, wt, x = ragged_case()
    M = n * h * w
    lib = capi.load()
    wT = capi.pack_conv_weight_T(wt.cuda())
    dx64 = torch.nn.grad.conv2d_input((n, 64, h, w), r16(wt), r16(dy), padding=1)
    ref = rows(dx64 * torch.where(x > 0, 1.0, 0.1).double() + x.double())
    dyb, r1b, actb = _embed(rows(dy), 80, 16, 44), _embed(rows(x), 72, 8, 45), _embed(rows(x), 72, 4, 46)
    fill = torch.randn(M + 1, 144, generator=torch.Generator().manual_seed(47)).cuda()
    buf = fill.clone()
    with grad_arithmetic(capi.GRAD_ARITH_BF16):
        assert _dgrad(lib, dyb, 80, 16, wT, buf, 144, 64, r1b, 72, 8, actb, 72, 4, n, h, w) == 0
        torch.cuda.synchronize()
    assert float((buf[:M, 64:128].cpu().double() - ref).abs().max()) < ATOL
    assert torch.equal(buf[:M, :64], fill[:M, :64]) and torch.equal(buf[:M, 128:], fill[:M, 128:]) and torch.equal(buf[M], fill[M])


@pytest.mark.parametrize("which", ["dx", "r1", "act"])
def test_unaligned_data_gradient_operands_give_the_defaults_bits(which):
    """a channel offset that is no multiple of 4 floats on dx, r1 or act: the tile kernels do not take it, the call runs the fp32 gather-GEMM in either mode"""
    n, h, w, dy, wt, x = ragged_case()
    M = n * h * w
    lib = capi.load()
    wT = capi.pack_conv_weight_T(wt.cuda())
    off = {"dx": 0, "r1": 0, "act": 0}
    off[which] = 6
    dyb, r1b, actb = rows(dy).cuda(), _embed(rows(x), 72, off["r1"], 45), _embed(rows(x), 72, off["act"], 46)
    fill = torch.randn(M + 1, 72, generator=torch.Generator().manual_seed(48)).cuda()
    got = []
    for mode in (capi.GRAD_ARITH_DEFAULT, capi.GRAD_ARITH_BF16):
        buf = fill.clone()
        with grad_arithmetic(mode):
            assert _dgrad(lib, dyb, 64, 0, wT, buf, 72, off["dx"], r1b, 72, off["r1"], actb, 72, off["act"], n, h, w) == 0
            torch.cuda.synchronize()
        got.append(buf)
    o = off["dx"]
    assert torch.equal(got[0], got[1])
    assert torch.equal(got[1][:M, :o], fill[:M, :o]) and torch.equal(got[1][:M, o + 64:], fill[:M, o + 64:]) and torch.equal(got[1][M], fill[M])
    dx64 = torch.nn.grad.conv2d_input((n, 64, h, w), wt.double(), dy.double(), padding=1)
    ref = rows(dx64 * torch.where(x > 0, 1.0, 0.1).double() + x.double())
    assert float((got[1][:M, o:o + 64].cpu().double() - ref).abs().max()) < ATOL      # fp32, of the UNROUNDED operands


def test_strided_weight_gradient_and_strides_it_does_not_cover():
    """dy at channel offset 64 of a 144-float row, x at offset 16 of an 80-float row: the bf16 kernel takes every stride the fp32 tile kernels take (16-B aligned
    channel vectors), so those run in the mode; a stride neither covers (65 floats) is answered in the mode exactly as without it -- the call goes down to the
    fp32 kernel's own answer instead of failing on its own."""
    n, h, w, dy, wt, x = ragged_case()
    lib, st = capi.load(), capi.stream_ptr()
    ref = torch.nn.grad.conv2d_weight(r16(x), (64, 64, 3, 3), r16(dy), padding=1)
    dyb, xb = _embed(rows(dy), 144, 64, 51), _embed(rows(x), 80, 16, 52)
    n_ws = lib.lfsr_conv3x3_wgrad_workspace_floats(n, h, w)
    ws = torch.full((n_ws + BAND,), SENTINEL, device="cuda")
    dw = torch.full((64, 64, 3, 3), SENTINEL, device="cuda")
    with grad_arithmetic(capi.GRAD_ARITH_BF16):
        assert lib.lfsr_conv3x3_wgrad(P(dyb), 144, 64, P(xb), 80, 16, P(dw), P(ws), n_ws, n, h, w, 0, st) == 0
        torch.cuda.synchronize()
    assert rel(dw, ref) <= 1e-4 and bool((ws[n_ws:] == SENTINEL).all())
    odd = torch.zeros(n * h * w + 1, 65, device="cuda")
    rcs = []
    for mode in (capi.GRAD_ARITH_DEFAULT, capi.GRAD_ARITH_BF16):
        dw1 = torch.full((64, 64, 3, 3), SENTINEL, device="cuda")
        with grad_arithmetic(mode):
            rcs.append(lib.lfsr_conv3x3_wgrad(P(odd), 65, 0, P(xb), 80, 16, P(dw1), P(ws), n_ws, n, h, w, 0, st))
            torch.cuda.synchronize()
        assert bool((dw1 == SENTINEL).all())
    assert rcs[0] == rcs[1] == E_ARG


def test_launch_size_invariance_and_determinism():
    B, A, h, w = GEOMS[4]
    c = case(B, A, h, w)
    n, dyv, xv = c["n"], rows(c["dy"]).cuda(), rows(c["x"]).cuda()
    wT = capi.pack_conv_weight_T(c["wt"].cuda())
    with grad_arithmetic(capi.GRAD_ARITH_BF16):
        for kw in ({}, {"res1": xv, "act": xv, "act_slope": 0.1}):
            k1 = {k: (v[:h * w] if torch.is_tensor(v) else v) for k, v in kw.items()}
            big, big2 = capi.conv3x3_dgrad(dyv, wT, n, h, w, **kw).clone(), capi.conv3x3_dgrad(dyv, wT, n, h, w, **kw).clone()
            one = capi.conv3x3_dgrad(dyv[:h * w], wT, 1, h, w, **k1).clone()
            torch.cuda.synchronize()
            assert torch.equal(big, big2)
            assert torch.equal(big[:h * w], one)
        w1, w2 = capi.conv3x3_wgrad(dyv, xv, n, h, w).clone(), capi.conv3x3_wgrad(dyv, xv, n, h, w).clone()
        torch.cuda.synchronize()
        assert torch.equal(w1, w2)


# ---------------------------------------------------------------------------------------------------------------------
# whole models
# ---------------------------------------------------------------------------------------------------------------------
def _distg_plugin():
    sys.path.insert(0, capi._HERE)
    try:
        return importlib.import_module("model.SR.DistgSSR")
    finally:
        sys.path.remove(capi._HERE)


def _step(net, xg, label):
    for p in net.parameters():
        p.grad = None
    out = net(xg, None)
    loss = F.l1_loss(out, label)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), float(loss.detach()), {k: p.grad.detach().cpu().double().numpy() for k, p in net.named_parameters()}, net.grad_bucket.clone()


def _flat(g, names):
    return np.concatenate([np.asarray(g[k], np.float64).reshape(-1) for k in names])


def _rel_np(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@functools.lru_cache(maxsize=None)
def _distg_refs(A, s, B, h, w):
    """plain fp64 autograd of the port, and the port's gradient under torch.autocast("cpu", bfloat16) (the reference's own reduced-precision path)"""
    sd, x = TH.distg_case(A, s, B, h, w)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    out = []
    for dt, amp in ((torch.float64, False), (torch.float32, True)):
        p = {k: torch.from_numpy(v).to(dt).requires_grad_(True) for k, v in sd.items()}
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=amp):
            y = TP.distgssr_forward_graph(torch.from_numpy(x).to(dt), p, A, s)
            loss = F.l1_loss(y.to(dt), torch.from_numpy(label).to(dt))
        loss.backward()
        out.append({k: v.grad.double().numpy() for k, v in p.items()})
    return sd, x, label, out[0], out[1]


@pytest.mark.parametrize("A,s,B,h,w", [(5, 2, 1, 8, 8), (3, 2, 2, 6, 8)])
def test_distgssr_whole_model(A, s, B, h, w):
    sd, x, label_np, g64, gamp = _distg_refs(A, s, B, h, w)
    names = [k for k, _ in TH.distg_spec(A, s)]
    M = _distg_plugin()
    net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to("cuda:0").train()
    assert [k for k, _ in net.named_parameters()] == names and len(names) == 137
    xg, label = torch.from_numpy(x).cuda(), torch.from_numpy(label_np).cuda()
    y_def, l_def, g_def, b_def = _step(net, xg, label)
    masks = TH.distg_hip_masks_flat(net._rt, xg)          # the default forward's LeakyReLU decisions (the forward does not read the switch)
    with grad_arithmetic(capi.GRAD_ARITH_BF16):
        y, l, g, b = _step(net, xg, label)
        # (d) the bucket holds the .grads
        assert torch.equal(torch.cat([p.grad.reshape(-1) for p in net.parameters()]), net.grad_bucket)
    # (a) the forward does not read the switch
    assert torch.equal(y, y_def) and l == l_def
    # (d) the mode is live
    assert not torch.equal(b, b_def)
    # (b) default forward, bf16 gradients: every parameter against fp64 autograd under the HIP forward's decisions, not above autocast's error for that parameter
    forced, flips = TH.distg_forced_fp64_grads(net._rt, xg, sd, x, label_np, A, s, masks=masks)
    e = {k: _rel_np(g[k], forced[k]) for k in names}
    e_amp = {k: _rel_np(gamp[k], g64[k]) for k in names}
    ratio = {k: e_amp[k] / max(e[k], 1e-30) for k in names}
    eb, eb_amp = _rel_np(_flat(g, names), _flat(forced, names)), _rel_np(_flat(gamp, names), _flat(g64, names))
    v = np.array(list(e.values()))
    kmin = min(ratio, key=ratio.get)
    print(f"distgssr {(A, s, B, h, w)} fp32 forward + bf16 gradients: per-parameter rel-L2 median {np.median(v):.2e} max {v.max():.2e}, bucket {eb:.2e}; "
          f"autocast median {np.median(list(e_amp.values())):.2e} max {max(e_amp.values()):.2e}, bucket {eb_amp:.2e}; "
          f"smallest autocast / hip ratio {ratio[kmin]:.2f} ({kmin}); decisions differing from fp64's own {flips}")
    bad = {k: (e[k], e_amp[k]) for k in names if not e[k] <= e_amp[k]}
    assert not bad, bad
    assert eb <= eb_amp
    # (c) bf16 forward + bf16 gradients: the bucket against plain fp64 autograd, not above autocast's
    with TH.arithmetic(capi.ARITH_BF16), grad_arithmetic(capi.GRAD_ARITH_BF16):
        _, _, g2, _ = _step(net, xg, label)
    eb2 = _rel_np(_flat(g2, names), _flat(g64, names))
    print(f"distgssr {(A, s, B, h, w)} bf16 forward + bf16 gradients: bucket rel-L2 {eb2:.2e}, autocast {eb_amp:.2e} (ratio {eb_amp / eb2:.2f})")
    assert eb2 <= eb_amp
    # the default is what it was
    _, _, _, b_again = _step(net, xg, label)
    assert torch.equal(b_again, b_def)


@pytest.mark.parametrize("name,tag", [("EPIT", "a5h8s4"), ("LFT", "a5h8s4"), ("LF_InterNet", "a5h8s2")])
def test_the_other_drivers_follow_the_data_gradient(name, tag):
    c, sd, x, _ = TH.model_case(name, tag)
    A, h, w, s, B = c["A"], c["h"], c["w"], c["s"], c["B"]
    M = importlib.import_module("lfsr_amd.model.SR." + name)
    net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.cuda().train()
    xg = torch.from_numpy(x).cuda()
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).cuda()

    def step():
        for p in net.parameters():
            p.grad = None
        F.l1_loss(net(xg), label).backward()
        torch.cuda.synchronize()
        return net.grad_bucket.clone()

    b_def = step()
    with grad_arithmetic(capi.GRAD_ARITH_BF16):
        b = step()
    d = rel(b, b_def)
    print(f"{name} {tag}: bucket rel-L2 distance of the bf16-gradient mode to the default {d:.2e}")
    assert bool(torch.isfinite(b).all()) and not torch.equal(b, b_def)
    assert d <= 5e-2
    assert torch.equal(step(), b_def)
