"""GPU: lfsr_set_wide_train_arithmetic -- LF_InterNet's wide per-view 3x3 convs (SpaConvSq 128 -> 64, SpaBottle 320 -> 64) in training: their weight gradient,
lfsr_conv3x3_wide_wgrad, on bf16 operands (csrc/wgrad_wide_bf16.hip: k_wgrad_wide_bf16) in modes 1 and 2, and forward_train's wide convs on
csrc/conv3x3_wide_bf16.hip in mode 2.

Operator: against the fp64 weight gradient of the same bf16-rounded operands, rel-L2 <= 1e-4 -- the gate tests/test_gpu_grad_bf16.py puts on the 64 -> 64 kernel,
which differs from its emulation by fp32 accumulation only, as this one does.  The kernel's tile is 4 rows x 32 columns of one view.
Whole model (tests/wide_train_emulation.py), rel-L2 against fp64 autograd of the stock graph, the yardstick being the stock graph under
torch.autocast("cpu", bfloat16), margin 1.0x.  CPU emulation of the modes:
  a5h8s2    bucket mode 1 1.14e-4, mode 2 4.06e-3, autocast 8.73e-3; every wide tensor of mode 1 inside autocast's by >= 57x
  a3h6w8s4  bucket mode 1 1.20e-4, mode 2 3.21e-3, autocast 5.84e-3; every wide tensor of mode 1 inside autocast's by >= 42x
Single tensors are not gated in mode 2 (ReLU decisions flipped by the bf16 forward: the emulation's smallest ratio is 0.97, at a Spa2Ang weight).
Every test restores all eight arithmetic selections."""
import contextlib
import ctypes as C
import functools
import importlib
from argparse import Namespace

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from lfsr_amd.synth import synth_input
from tests import wide_train_emulation as E
from tests.helpers import model_case, op_input
from tests.test_gpu_internet_train import hip_step, make_net

pytestmark = pytest.mark.gpu
GATE = 1e-4
TAGS = ("a5h8s2", "a3h6w8s4")
BF16_MODES = (capi.WIDE_TRAIN_ARITH_BF16_WGRAD, capi.WIDE_TRAIN_ARITH_BF16)
# (n_img, h, w): a view smaller than the 4 x 32 tile; one past the tile on both axes; the fixture's; exact tiles; more tiles than blocks (a block accumulates across tiles)
GEOMS = ((1, 5, 7), (3, 9, 33), (18, 6, 8), (2, 16, 64), (300, 8, 8))
X_LAYOUTS = {128: ((128, 0), (384, 64)), 320: ((320, 0),)}
DY_LAYOUTS = ((64, 0), (128, 64))
SENTINEL = -12345.5
PAD = 64                      # sentinel floats in front of and behind dw (256 B: dw stays on the 16-byte grid)


@contextlib.contextmanager
def modes(wide_train=capi.WIDE_TRAIN_ARITH_DEFAULT, arith=capi.ARITH_DEFAULT, grad=capi.GRAD_ARITH_DEFAULT, wide=capi.WIDE_ARITH_DEFAULT):
    """the selections for the block; all eight are the default again after it (the settings are process-wide)"""
    try:
        capi.set_wide_train_arithmetic(wide_train)
        capi.set_arithmetic(arith)
        capi.set_grad_arithmetic(grad)
        capi.set_wide_arithmetic(wide)
        yield
    finally:
        capi.set_arithmetic(capi.ARITH_DEFAULT)
        capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT)
        capi.set_gemm_arithmetic(capi.GEMM_ARITH_DEFAULT)
        capi.set_branch_arithmetic(capi.BRANCH_ARITH_DEFAULT)
        capi.set_ang_arithmetic(capi.ANG_ARITH_DEFAULT)
        capi.set_wide_arithmetic(capi.WIDE_ARITH_DEFAULT)
        capi.set_lin_grad_arithmetic(capi.LIN_GRAD_ARITH_DEFAULT)
        capi.set_wide_train_arithmetic(capi.WIDE_TRAIN_ARITH_DEFAULT)


def r(t):
    return t.to(torch.bfloat16).double()


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def wgrad64(x, dy, n_img, h, w):
    """fp64 (64, cin, 3, 3): the zero-padded 3x3 conv's weight gradient from VCL rows x (n_img h w, cin) and dy (n_img h w, 64)"""
    img = lambda t: t.reshape(n_img, h, w, -1).permute(0, 3, 1, 2)
    return torch.nn.grad.conv2d_weight(img(x), (64, x.shape[1], 3, 3), img(dy), padding=1)


@functools.lru_cache(maxsize=None)
def wgrad_case(cin, n_img, h, w, kind="rand", k=0):
    """-> x and dy rows (fp32), the fp64 gradient of the bf16-rounded operands and of the unrounded ones; computed once and never written to.
    kind: "rand"; "chunk": x is zero outside the channels [64 k, 64 k + 64); "corner": dy is zero outside the last pixel of the last view"""
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    rows = n_img * h * w
    x = rnd((rows, cin), 11 + cin + n_img).float()
    dy = rnd((rows, 64), 7 + cin + n_img, 1.0 / rows ** 0.5).float()
    if kind == "chunk":
        keep = torch.zeros(cin)
        keep[64 * k:64 * k + 64] = 1.0
        x = x * keep
    if kind == "corner":
        keep = torch.zeros(rows, 1)
        keep[rows - 1] = 1.0
        dy = dy * keep
    return x, dy, wgrad64(r(x), r(dy), n_img, h, w), wgrad64(x.double(), dy.double(), n_img, h, w)


class DwPool:
    """dw (64, cin, 3, 3) between two runs of sentinel floats inside one allocation"""

    def __init__(self, cin, init=None):
        self.n = 64 * cin * 9
        self.t = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.float32, device="cuda")
        if init is not None:
            self.t[PAD:PAD + self.n] = init.reshape(-1).float().cuda()
        self.ptr = C.c_void_p(self.t.data_ptr() + PAD * 4)
        self.cin = cin

    def read(self):
        torch.cuda.synchronize()
        assert bool((self.t[:PAD] == SENTINEL).all()) and bool((self.t[PAD + self.n:] == SENTINEL).all()), "floats outside dw written"
        return self.t[PAD:PAD + self.n].reshape(64, self.cin, 3, 3).cpu()


def run_op(dyb, dyl, xb, xl, cin, n_img, h, w, pool, accumulate=0):
    lib = capi.load()
    ws = torch.empty(lib.lfsr_conv3x3_wide_wgrad_workspace_floats(cin, n_img, h, w), dtype=torch.float32, device="cuda")
    rc = lib.lfsr_conv3x3_wide_wgrad(dyb.ptr, dyl[0], dyl[1], xb.ptr, xl[0], xl[1], cin, pool.ptr, capi.dev_ptr(ws), ws.numel(), n_img, h, w, accumulate,
                                     capi.stream_ptr())
    assert rc == 0, rc
    return pool.read()


def check_operator(mode, cin, n_img, h, w, kind="rand", k=0, x_layouts=None, dy_layouts=DY_LAYOUTS):
    """every layout pair on guarded buffers (tests/helpers.py: NaN rows around the operands, +-1e3 in their foreign columns) -> the last dw"""
    x, dy, ref, _ = wgrad_case(cin, n_img, h, w, kind, k)
    worst, dw = 0.0, None
    for xl in x_layouts or X_LAYOUTS[cin]:
        xb = op_input(x, xl[0], xl[1], 21)
        x_before = xb.t.clone()
        for dyl in dy_layouts:
            dyb = op_input(dy, dyl[0], dyl[1], 22)
            dy_before = dyb.t.clone()
            with modes(mode):
                dw = run_op(dyb, dyl, xb, xl, cin, n_img, h, w, DwPool(cin))
            e = rel(dw, ref)
            worst = max(worst, e)
            assert bool(torch.isfinite(dw).all())
            assert e <= GATE, (mode, cin, n_img, h, w, kind, k, xl, dyl, e)
            assert torch.equal(dyb.t.view(torch.int32), dy_before.view(torch.int32)), "dy changed"
        assert torch.equal(xb.t.view(torch.int32), x_before.view(torch.int32)), "x changed"
    print(f"WIDE_TRAIN operator mode {mode} cin {cin} n_img {n_img} {h}x{w} {kind} {k}: worst rel-L2 against the fp64 gradient of the rounded operands {worst:.2e}")
    return dw


def plain(t):
    return op_input(t, t.shape[1], 0, 3)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the operator against the fp64 gradient of the rounded operands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("cin", [128, 320])
@pytest.mark.parametrize("mode", BF16_MODES)
def test_operator_against_the_fp64_gradient_of_the_rounded_operands(mode, cin, geom):
    check_operator(mode, cin, *geom)


# ---------------------------------------------------------------------------------------------------------------------
# 2. structure
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,chunk", [(128, 0), (128, 1), (320, 0), (320, 1), (320, 2), (320, 3), (320, 4)])
def test_single_chunk(cin, chunk):
    """x is zero outside one 64-channel chunk: the dw columns outside it are exactly zero (a wrong chunk base or slab column shows), the ones inside pass the gate"""
    dw = check_operator(capi.WIDE_TRAIN_ARITH_BF16_WGRAD, cin, 3, 9, 33, "chunk", chunk, x_layouts=X_LAYOUTS[cin][-1:], dy_layouts=DY_LAYOUTS[-1:])
    inside = torch.zeros(cin, dtype=torch.bool)
    inside[64 * chunk:64 * chunk + 64] = True
    assert bool((dw[:, ~inside] == 0).all())
    assert float(dw[:, inside].abs().max()) > 0


@pytest.mark.parametrize("cin", [128, 320])
def test_corner_pixel(cin):
    """dy is non-zero at the last pixel of the last view only: the taps that reach past the view's bottom or right edge give exactly zero"""
    dw = check_operator(capi.WIDE_TRAIN_ARITH_BF16_WGRAD, cin, 3, 9, 33, "corner", x_layouts=X_LAYOUTS[cin][-1:], dy_layouts=DY_LAYOUTS[-1:])
    assert bool((dw[:, :, 2, :] == 0).all()) and bool((dw[:, :, :, 2] == 0).all())
    assert all(float(dw[:, :, ky, kx].abs().max()) > 0 for ky in (0, 1) for kx in (0, 1))


@pytest.mark.parametrize("cin", [128, 320])
@pytest.mark.parametrize("mode", BF16_MODES)
def test_accumulate_determinism_and_view_additivity(mode, cin):
    n_img, h, w = 18, 6, 8
    x, dy, ref, _ = wgrad_case(cin, n_img, h, w)
    xb, dyb = plain(x), plain(dy)
    xl, dyl = (cin, 0), (64, 0)
    old = rnd((64, cin, 3, 3), 9, 0.5).float()
    with modes(mode):
        dw = run_op(dyb, dyl, xb, xl, cin, n_img, h, w, DwPool(cin))
        again = run_op(dyb, dyl, xb, xl, cin, n_img, h, w, DwPool(cin))
        acc = run_op(dyb, dyl, xb, xl, cin, n_img, h, w, DwPool(cin, old), accumulate=1)
        per_view = torch.zeros_like(dw, dtype=torch.float64)
        for i in range(n_img):
            sl = slice(i * h * w, (i + 1) * h * w)
            per_view += run_op(plain(dy[sl]), dyl, plain(x[sl]), xl, cin, 1, h, w, DwPool(cin)).double()
    assert torch.equal(dw, again)                                    # two runs give the same bits
    assert rel(acc, old.double() + ref) <= GATE                     # += onto a non-zero dw
    assert torch.equal(acc, old + dw)                                # ... which is one fp32 add of what = writes
    assert rel(dw, per_view) <= GATE                                 # n_img views are the sum of the per-view calls


@pytest.mark.parametrize("cin", [128, 320])
def test_modes_are_live_and_the_default_is_the_unrounded_gradient(cin):
    n_img, h, w = 3, 9, 33
    x, dy, ref, exact = wgrad_case(cin, n_img, h, w)
    xb, dyb = plain(x), plain(dy)
    run = lambda: run_op(dyb, (64, 0), xb, (cin, 0), cin, n_img, h, w, DwPool(cin))
    untouched = run()                                                # the switch never touched in this block
    with modes():
        assert torch.equal(run(), untouched)
    # the gate tests/test_gpu_bwd_ops.py applies to lfsr_conv3x3_wgrad: rel-L2 <= 1e-4 and max|err| <= 1e-4 max(1, max|ref|), against the unrounded fp64 gradient
    assert rel(untouched, exact) <= 1e-4
    assert float((untouched.double() - exact).abs().max()) <= 1e-4 * max(1.0, float(exact.abs().max()))
    got = {}
    for mode in BF16_MODES:
        with modes(mode):
            got[mode] = run()
        assert not torch.equal(got[mode], untouched)
        assert rel(got[mode], ref) <= GATE < rel(got[mode], exact)  # it really is the rounded operands' gradient
    assert torch.equal(got[1], got[2])                               # the operator is the same in modes 1 and 2
    with modes(arith=capi.ARITH_F32, wide_train=capi.WIDE_TRAIN_ARITH_BF16):
        assert torch.equal(run(), got[2])                            # LFSR_ARITH_F32 has no bearing on the weight gradient
    with modes(wide=capi.WIDE_ARITH_BF16, grad=capi.GRAD_ARITH_BF16):
        assert torch.equal(run(), untouched)                         # nor do the inference switch or the 64 -> 64 gradient switch reach it
    assert capi.get_wide_train_arithmetic() == capi.WIDE_TRAIN_ARITH_DEFAULT
    assert torch.equal(run(), untouched)


# ---------------------------------------------------------------------------------------------------------------------
# 3. refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_refusals_write_nothing(mode):
    cin, n_img, h, w = 128, 2, 5, 7
    x, dy, ref, _ = wgrad_case(cin, n_img, h, w)
    xb, dyb = op_input(x, 384, 64, 1), op_input(dy, 128, 64, 2)
    lib, st = capi.load(), capi.stream_ptr()
    pool = DwPool(cin)
    n_ws = lib.lfsr_conv3x3_wide_wgrad_workspace_floats(cin, n_img, h, w)
    ws = torch.full((n_ws + 4,), SENTINEL, dtype=torch.float32, device="cuda")
    wsp = C.c_void_p(ws.data_ptr())

    def call(dy_=dyb.ptr, ds=128, do=64, x_=xb.ptr, xs=384, xo=64, cin_=cin, dw_=pool.ptr, ws_=wsp, nws=n_ws, n_=n_img, h_=h, w__=w, acc=0):
        return lib.lfsr_conv3x3_wide_wgrad(dy_, ds, do, x_, xs, xo, cin_, dw_, ws_, nws, n_, h_, w__, acc, st)

    off4 = lambda p: C.c_void_p(p.value + 4)
    with modes(mode):
        bad = [call(dy_=None), call(x_=None), call(dw_=None), call(ws_=None),
               call(cin_=64), call(cin_=192), call(cin_=0), call(cin_=256), call(xs=320, xo=0, cin_=384),
               call(n_=0), call(n_=-1), call(h_=0), call(w__=0), call(h_=-3),
               call(xs=128, xo=64), call(xs=188, xo=64), call(ds=64, do=4), call(ds=124, do=64),
               call(xo=-4), call(do=-4), call(xs=-384), call(ds=-128),
               call(xs=386), call(xo=66), call(ds=130), call(do=62),
               call(dy_=off4(dyb.ptr)), call(x_=off4(xb.ptr)), call(dw_=off4(pool.ptr)), call(ws_=off4(wsp)),
               call(n_=1 << 20, h_=32, w__=32, nws=1 << 40),     # 2^30 rows: far past 2 GiB
               call(n_=1399, h_=32, w__=32, nws=1 << 40),        # 1,432,576 rows x 384 floats: x just past 2 GiB
               call(n_=4195, h_=32, w__=32, xs=128, xo=0, nws=1 << 40)]    # 4,295,680 rows x 128 floats: dy and x just past 2 GiB
        assert bad == [-1] * len(bad), bad
        assert call(nws=n_ws - 1) == -2 and call(nws=0) == -2        # LFSR_E_WS
        torch.cuda.synchronize()
        assert bool((pool.t == SENTINEL).all()) and bool((ws == SENTINEL).all())      # nothing written
        assert call() == 0
        assert rel(pool.read(), ref if mode else wgrad_case(cin, n_img, h, w)[3]) <= GATE
        assert bool((ws[n_ws:] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. whole model
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_refs(tag):
    """-> case, state_dict, input, label, and the gradients of the stock graph: fp64 autograd, under autocast(bfloat16), and the CPU emulation of modes 1 and 2
    (computed once, shared, never written to)"""
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    case, sd, x, _ = model_case("LF_InterNet", tag)
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    _, g64 = E.step_grads(sd, x, label, A, s)
    _, gamp = E.step_grads(sd, x, label, A, s, dtype=torch.float32, autocast=True)
    emul = {m: E.step_grads(sd, x, label, A, s, r=E.r_bf16, flags=E.MODES[m])[1] for m in (1, 2)}
    return case, sd, x, label, g64, gamp, emul


def _flat(g, names):
    return np.concatenate([np.asarray(g[k], np.float64).reshape(-1) for k in names])


def _bucket_dict(net, bucket, ref):
    b = bucket.cpu().numpy()
    return {k: b[net._spans[k][0]:net._spans[k][0] + net._spans[k][1]].reshape(ref[k].shape) for k, _ in net.named_parameters()}


@pytest.mark.parametrize("tag", TAGS)
def test_whole_model(tag):
    case, sd, x, label_np, g64, gamp, emul = model_refs(tag)
    A, s = case["A"], case["s"]
    net, _ = make_net(A, s, sd)
    names = [k for k, _ in net.named_parameters()]
    xg, label = torch.from_numpy(x).cuda(), torch.from_numpy(label_np).cuda()
    l_def, b_def, y_def = hip_step(net, xg, label)
    ws_bytes = {0: net._rt.train_workspace_bytes(case["B"], case["h"], case["w"])}
    e_amp = {k: rel(gamp[k], g64[k]) for k in names}
    eb_amp = rel(_flat(gamp, names), _flat(g64, names))
    fails = []

    # ---- mode 1: the forward as it is, the seventeen wide weight gradients on bf16 operands
    with modes(capi.WIDE_TRAIN_ARITH_BF16_WGRAD):
        l1, b1, y1 = hip_step(net, xg, label)
        ws_bytes[1] = net._rt.train_workspace_bytes(case["B"], case["h"], case["w"])
    assert torch.equal(y1, y_def) and l1 == l_def
    wide_mask = torch.zeros(b_def.numel(), dtype=torch.bool)
    for k in E.WIDE_KEYS:
        off, n = net._spans[k]
        wide_mask[off:off + n] = True
        assert not torch.equal(b1[off:off + n], b_def[off:off + n]), k        # the mode is live in every wide tensor
    assert torch.equal(b1.cpu()[~wide_mask], b_def.cpu()[~wide_mask])         # every other span is bit-equal
    g1 = _bucket_dict(net, b1, g64)
    e1 = {k: rel(g1[k], g64[k]) for k in E.WIDE_KEYS}
    em1 = {k: rel(emul[1][k], g64[k]) for k in E.WIDE_KEYS}
    eb1, ebm1 = rel(_flat(g1, names), _flat(g64, names)), rel(_flat(emul[1], names), _flat(g64, names))
    kmin = min(E.WIDE_KEYS, key=lambda k: e_amp[k] / max(e1[k], 1e-30))
    print(f"internet {tag} mode 1: bucket rel-L2 vs fp64 {eb1:.2e} (emulation {ebm1:.2e}), autocast {eb_amp:.2e}; wide tensors max {max(e1.values()):.2e} "
          f"(emulation {max(em1.values()):.2e}); smallest autocast / hip ratio {e_amp[kmin] / max(e1[kmin], 1e-30):.1f} ({kmin}; "
          f"emulation {min(e_amp[k] / max(em1[k], 1e-30) for k in E.WIDE_KEYS):.1f})")
    bad = {k: (e1[k], e_amp[k]) for k in E.WIDE_KEYS if not e1[k] <= e_amp[k]}
    if bad:
        fails.append(("mode 1 tensors", bad))
    if not eb1 <= eb_amp:
        fails.append(("mode 1 bucket", eb1, eb_amp))

    # ---- mode 2: forward_train's wide convs on bf16 operands as well
    with modes(capi.WIDE_TRAIN_ARITH_BF16):
        l2, b2, y2 = hip_step(net, xg, label)
        ws_bytes[2] = net._rt.train_workspace_bytes(case["B"], case["h"], case["w"])
        with torch.no_grad():
            y2_nograd = net(xg).clone()                        # a no-grad forward does not read this switch ...
    with modes(wide=capi.WIDE_ARITH_BF16):
        with torch.no_grad():
            y_inf_bf16 = net(xg).clone()                       # ... it reads lfsr_set_wide_arithmetic
        _, b_w, y_w = hip_step(net, xg, label)                 # which alone still leaves a training step's bits unchanged
    assert torch.equal(y2_nograd, y_def)
    assert torch.equal(y_w, y_def) and torch.equal(b_w, b_def)
    assert torch.equal(y2, y_inf_bf16) and not torch.equal(y2, y_def)
    g2 = _bucket_dict(net, b2, g64)
    eb2, ebm2 = rel(_flat(g2, names), _flat(g64, names)), rel(_flat(emul[2], names), _flat(g64, names))
    print(f"internet {tag} mode 2: bucket rel-L2 vs fp64 {eb2:.2e} (emulation {ebm2:.2e}), autocast {eb_amp:.2e} (ratio {eb_amp / eb2:.2f}; emulation {eb_amp / ebm2:.2f})")
    if not eb2 <= eb_amp:
        fails.append(("mode 2 bucket", eb2, eb_amp))
    assert not fails, fails

    # ---- further checks
    with modes(arith=capi.ARITH_F32):
        _, _, y_f32 = hip_step(net, xg, label)
    with modes(capi.WIDE_TRAIN_ARITH_BF16, arith=capi.ARITH_F32):
        _, _, y2_f32 = hip_step(net, xg, label)
    assert torch.equal(y2_f32, y_f32)                          # LFSR_ARITH_F32 wins for the forward half
    with modes(capi.WIDE_TRAIN_ARITH_BF16, grad=capi.GRAD_ARITH_BF16):
        _, b2g, _ = hip_step(net, xg, label)
    d = rel(b2g.cpu(), b_def.cpu())
    print(f"internet {tag} mode 2 + GRAD_ARITH_BF16: bucket rel-L2 distance to the default {d:.2e}")
    assert bool(torch.isfinite(b2g).all()) and d <= 5e-2
    _, b_again, y_again = hip_step(net, xg, label)
    assert torch.equal(b_again, b_def) and torch.equal(y_again, y_def)        # the default is what it was
    assert ws_bytes[0] == ws_bytes[1] == ws_bytes[2] > 0


def test_an_lft_training_step_does_not_follow_the_switch():
    """LFT's 64 -> 64 position conv runs the same generic IN_CONV3 weight-gradient kernel the default falls back to"""
    c, sd, x, _ = model_case("LFT", "a5h8s4")
    A, h, w, s, B = c["A"], c["h"], c["w"], c["s"], c["B"]
    M = importlib.import_module("lfsr_amd.model.SR.LFT")
    net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.cuda().train()
    xg = torch.from_numpy(x).cuda()
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).cuda()
    _, b_def, y_def = hip_step(net, xg, label)
    with modes(capi.WIDE_TRAIN_ARITH_BF16):
        _, b, y = hip_step(net, xg, label)
    assert torch.equal(y, y_def) and torch.equal(b, b_def)
