"""GPU: lfsr_set_ang_arithmetic(LFSR_ANG_ARITH_BF16) -- LFSSR's angular 3x3 conv, lfsr_angconv3x3_fwd, on bf16 operands (csrc/ang3x3_bf16.hip: k_ang3x3_bf16),
and LFSSR as a whole under the reduced-precision modes.

Emulation of the operator, r(t) = t.to(torch.bfloat16): pre(x) in fp32 on the CPU (the kernel's own single add and max), r of it and of the weight, then the sum
in fp64 (stock conv2d over the A x A grid).  The kernel rounds no intermediate, so it differs from the emulation by fp32 accumulation over at most K = 576 only:
the project's gate, max abs <= 1e-4 max(1, max|emulation|).  The default-mode result is held to the same gate against the unrounded fp64 sum.
Whole model (tests/lfssr_stock_graph.py): the gates of tests/test_gpu_branch_bf16.py::test_whole_model against the fp64 graph and the stock graph under
torch.autocast(bfloat16).  CPU emulation of the modes (fp64 sums, r on the operands named), rms against the fp64 graph, ang mode / ang + per-view convs / autocast:
a5h8s4 7.31e-4 / 1.08e-3 / 1.78e-3, a3h6w8s2 2.88e-4 / 4.42e-4 / 1.32e-3, a2h5w7s4 2.34e-4 / 3.61e-4 / 1.16e-3.
Every test restores all five arithmetic selections."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lfsr_amd import capi
from tests import lfssr_helpers as H
from tests.helpers import distg_case, epit_case, op_input, op_output, op_output_read, psnr
from tests.lfssr_stock_graph import lfssr_stock
from tests.test_gpu_lfssr import case as lfssr_fp64_case, dev, runtime
from tests.test_gpu_lfssr_ops import ang_case, rnd, run_ang

pytestmark = pytest.mark.gpu
ATOL = 1e-4
GUARD = 4096            # floats in front of and behind an output
SENTINEL = -12345.5


@contextlib.contextmanager
def modes(arith=capi.ARITH_DEFAULT, ang=capi.ANG_ARITH_DEFAULT):
    """the two selections for the block; all five are the default again after it (the settings are process-wide)"""
    try:
        capi.set_arithmetic(arith)
        capi.set_ang_arithmetic(ang)
        yield
    finally:
        capi.set_arithmetic(capi.ARITH_DEFAULT)
        capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT)
        capi.set_gemm_arithmetic(capi.GEMM_ARITH_DEFAULT)
        capi.set_branch_arithmetic(capi.BRANCH_ARITH_DEFAULT)
        capi.set_ang_arithmetic(capi.ANG_ARITH_DEFAULT)


BF16 = functools.partial(modes, ang=capi.ANG_ARITH_BF16)


def r(t):
    return t.to(torch.bfloat16).double()


def gate(ref):
    return ATOL * max(1.0, float(ref.abs().max()))


def emulation(x, wt, bias, in_bias, B, A, npix):
    """fp64 rows of relu(bias + conv over the grid of r(pre(x)) with r(W)); pre in fp32"""
    t = x if in_bias is None else torch.relu(x + in_bias)
    g = r(t).reshape(B, A, A, npix, 64).permute(0, 3, 4, 1, 2).reshape(B * npix, 64, A, A)
    o = torch.relu(F.conv2d(g, r(wt), bias.double(), padding=1))
    return o.reshape(B, npix, 64, A, A).permute(0, 3, 4, 1, 2).reshape(-1, 64)


def check_operator(A, h, w, B, biased, layouts, only_tap=None):
    npix = h * w
    x, wt, bias, in_bias, exact, _ = ang_case(A, h, w, B, biased, only_tap)
    em = emulation(x, wt, bias, in_bias, B, A, npix)
    for xl, yl in layouts:
        y_def = run_ang(x, wt, bias, in_bias, B, A, npix, xl, yl)
        with BF16():
            y = run_ang(x, wt, bias, in_bias, B, A, npix, xl, yl, seed=2)
        e, e_def = float((y.double() - em).abs().max()), float((y_def.double() - exact).abs().max())
        print(f"ANG_BF16 operator A{A} {h}x{w} B{B} {'in_bias' if biased else 'plain'} x{xl} y{yl}: max|gpu - emul| {e:.2e} (gate {gate(em):.2e}), "
              f"default vs exact {e_def:.2e}, emul vs exact {float((em - exact).abs().max()):.2e}")
        assert bool(torch.isfinite(y).all())
        assert e_def <= gate(exact)                     # the yardstick itself: the default operator is the unrounded sum
        assert e <= gate(em)
        assert not torch.equal(y, y_def)                # the mode is live
    return y


# ---------------------------------------------------------------------------------------------------------------------
# 1. the operator against the fp64 emulation
# ---------------------------------------------------------------------------------------------------------------------
# angRes 2 (every view a corner), 3, 5 (an interior view) x views of 1 x 1 (one pixel of a 16-pixel tile), 3 x 5 (15: one ragged tile), 8 x 8 (four tiles) x B 1, 2
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (8, 8)])
@pytest.mark.parametrize("A", [2, 3, 5])
def test_operator_against_the_fp64_emulation(A, hw, B):
    for biased in (False, True):
        check_operator(A, hw[0], hw[1], B, biased, (((64, 0), (64, 0)), ((144, 64), (144, 64))))


@pytest.mark.parametrize("A,h,w", [(6, 3, 5), (7, 2, 3), (8, 1, 3), (9, 3, 3), (4, 5, 5)])
def test_operator_banded_grids(A, h, w):
    """angRes 6..9 run as bands of view rows (a band stages the view row on either side of it; the last band of 7 and 9 is one row); 4: one band of 16 views"""
    check_operator(A, h, w, 2, True, (((144, 64), (64, 0)),))


# ---------------------------------------------------------------------------------------------------------------------
# 2. tap orientation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tap", [(0, 0), (2, 2)])
def test_single_tap_pairs_first_axis_with_u(tap):
    """weights zero except one corner tap: y[b,u,v] = relu(bias + r(W[:, :, tap]) r(a[b, u + tap_u - 1, v + tap_v - 1])) where that view exists, relu(bias) elsewhere"""
    A, h, w, B = 5, 3, 5, 2
    npix = h * w
    got = check_operator(A, h, w, B, True, (((64, 0), (64, 0)),), only_tap=tap)
    x, wt, bias, in_bias, _, _ = ang_case(A, h, w, B, True, tap)
    a = r(torch.relu(x + in_bias)).reshape(B, A, A, npix, 64)
    du, dv = tap[0] - 1, tap[1] - 1
    want = torch.zeros(B, A, A, npix, 64, dtype=torch.float64)
    for u in range(A):
        for v in range(A):
            if 0 <= u + du < A and 0 <= v + dv < A:
                want[:, u, v] = a[:, u + du, v + dv] @ r(wt[:, :, tap[0], tap[1]]).t()
    want = torch.relu(want + bias.double()).reshape(-1, 64)
    assert float((got.double() - want).abs().max()) <= gate(want)
    edge = got.reshape(B, A, A, npix, 64)[:, 0 if du < 0 else A - 1]          # the rows the tap does not reach hold relu(bias) exactly
    assert torch.equal(edge, torch.relu(bias).expand_as(edge))


# ---------------------------------------------------------------------------------------------------------------------
# 3. writes only its rows
# ---------------------------------------------------------------------------------------------------------------------
# 35 pixels: two tiles and 3; angRes 3: one band; 7: three bands, the last of one view row
@pytest.mark.parametrize("A", [3, 7])
def test_writes_only_its_rows(A):
    B, npix = 2, 35
    rows = B * A * A * npix
    xw = rnd((rows, 128), 31 + A).float().cuda()
    wp = capi.pack_conv_weight(rnd((64, 64, 3, 3), 5, 1.0 / 24.0).float().cuda())
    bias, in_bias = rnd((64,), 6, 0.1).float().cuda(), (torch.rand(64, generator=torch.Generator().manual_seed(7)) + 0.5).cuda()
    pool = torch.full((2 * GUARD + rows * 128,), SENTINEL, dtype=torch.float32, device="cuda")
    out = pool[GUARD:GUARD + rows * 128].view(rows, 128)
    with BF16():
        fresh = capi.angconv3x3(xw, wp, bias, B, A, npix, in_bias=in_bias, x_choff=64).clone()
        got = capi.angconv3x3(xw, wp, bias, B, A, npix, in_bias=in_bias, out=out, x_choff=64, out_choff=64)
        torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((pool[:GUARD] == SENTINEL).all()) and bool((pool[GUARD + rows * 128:] == SENTINEL).all()), "written outside its rows"
    assert bool((out[:, :64] == SENTINEL).all()), "written outside its columns"
    assert not bool((out[:, 64:] == SENTINEL).any()), "rows left unwritten"
    assert torch.equal(out[:, 64:], fresh)
    y_def = capi.angconv3x3(xw, wp, bias, B, A, npix, in_bias=in_bias, x_choff=64)
    assert not torch.equal(y_def, fresh)                # the mode was live


# ---------------------------------------------------------------------------------------------------------------------
# 4. determinism and launch-size invariance
# ---------------------------------------------------------------------------------------------------------------------
def test_determinism_and_launch_size_invariance():
    """two blocks of four waves a CU: 512 blocks on 256 CUs; (B, npix) = (10, 1024) is 640 blocks, more than the chip holds at once.  No fp64 work here."""
    A, npix, B = 5, 1024, 10
    n1 = A * A * npix
    x = torch.randn((B * n1, 64), generator=torch.Generator(device="cuda").manual_seed(3), device="cuda")
    wp = capi.pack_conv_weight(rnd((64, 64, 3, 3), 5, 1.0 / 24.0).float().cuda())
    bias, in_bias = rnd((64,), 6, 0.1).float().cuda(), (torch.rand(64, generator=torch.Generator().manual_seed(7)) + 0.5).cuda()
    with BF16():
        y = capi.angconv3x3(x, wp, bias, B, A, npix, in_bias=in_bias)
        y2 = capi.angconv3x3(x, wp, bias, B, A, npix, in_bias=in_bias)
        y1 = capi.angconv3x3(x[:n1].contiguous(), wp, bias, 1, A, npix, in_bias=in_bias)
        torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and float(y.max()) > 0
    assert torch.equal(y, y2)
    assert torch.equal(y[:n1], y1)


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing_under_the_mode():
    """the argument cases of tests/test_gpu_lfssr_ops.py::test_angconv3x3_refusals_write_nothing: the same codes, nothing written"""
    A, h, w, B = 3, 3, 5, 1
    npix = h * w
    x, wt, bias, in_bias, _, _ = ang_case(A, h, w, B, True)
    xb, yb = op_input(x, 144, 64, 1), op_output(x.shape[0], 144, 2)
    wp, bd, ib = capi.pack_conv_weight(wt.cuda()), bias.cuda(), in_bias.cuda()
    lib, st = capi.load(), capi.stream_ptr()
    P = capi.dev_ptr

    def call(x_=xb.ptr, xs=144, xo=64, w_=None, b_=None, ib_=None, y_=yb.ptr, ys=144, yo=64, B_=B, A_=A, n_=npix):
        return lib.lfsr_angconv3x3_fwd(x_, xs, xo, w_ or P(wp), b_ or P(bd), ib_ or P(ib), y_, ys, yo, B_, A_, n_, st)

    off4 = lambda p: C.c_void_p(p.value + 4)
    with BF16():
        bad = [call(A_=1), call(A_=10), call(A_=0), call(B_=0), call(n_=0), call(xs=146), call(xo=66), call(ys=142), call(yo=62), call(xs=100, xo=64),
               call(ys=64, yo=4), call(x_=off4(xb.ptr)), call(y_=off4(yb.ptr)), call(ib_=off4(P(ib))), call(w_=off4(P(wp))), call(x_=None), call(y_=None),
               call(B_=1 << 20, n_=1 << 8),                 # 2^28 * 9 rows of 144 floats: far past 2 GiB
               call(B_=4, A_=8, n_=14564)]                  # 3,728,384 rows x 144 floats = 2^29 + 16,384 floats: just past 2 GiB
        assert bad == [-1] * len(bad), bad
        op_output_read(yb, 0, 0)
        assert call() == 0
        op_output_read(yb, 64, 64)


# ---------------------------------------------------------------------------------------------------------------------
# 6. whole model
# ---------------------------------------------------------------------------------------------------------------------
def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def whole_model_gates(tag, A, s, sd, x, y64):
    """LFSSR at angRes A, scale s on the mosaic x under the three reduced-precision mode combinations against the fp64 output y64: the three criteria of
    test_whole_model (tests/test_gpu_lfssr_geometries.py applies them across its geometry matrix); the default output is bit-equal again afterwards"""
    with torch.autocast("cpu", dtype=torch.bfloat16):
        y_amp = lfssr_stock(x, sd, A, s, dtype=torch.float32).double().numpy()
    label = torch.rand(y64.shape, generator=torch.Generator().manual_seed(2)).numpy()
    rt = runtime(A, s, sd)
    xg = dev(x)
    y_def = rt.forward(xg).cpu().numpy()
    e_amp, e_def = _rms(y_amp, y64), _rms(y_def, y64)
    assert np.abs(y_def - y64).max() <= ATOL * max(1.0, np.abs(y64).max())            # the default is what it was
    fails = []
    for name, arith, ang in (("ang mode", capi.ARITH_DEFAULT, capi.ANG_ARITH_BF16), ("conv mode", capi.ARITH_BF16, capi.ANG_ARITH_DEFAULT),
                             ("ang + conv modes", capi.ARITH_BF16, capi.ANG_ARITH_BF16)):
        with modes(arith=arith, ang=ang):
            y = rt.forward(xg).cpu().numpy()
        dpsnr = psnr(y, label) - psnr(y64, label)
        e = _rms(y, y64)
        print(f"lfssr {tag} {name}: rms {e:.2e} max {np.abs(y - y64).max():.2e} vs fp64; autocast rms {e_amp:.2e} (ratio {e_amp / e:.2f}); "
              f"default mode rms {e_def:.2e}; dPSNR vs label {dpsnr:+.5f} dB (autocast {psnr(y_amp, label) - psnr(y64, label):+.5f})")
        if not abs(dpsnr) <= 0.01:                      # (a) the project's gate
            fails.append((name, "dPSNR", dpsnr))
        if not e <= e_amp:                              # (b) not worse than the reduced-precision path of stock torch
            fails.append((name, "rms", e, e_amp))
        if np.array_equal(y, y_def):                    # (c) the mode is live in the model driver
            fails.append((name, "equal to the default"))
    assert not fails, fails
    assert np.array_equal(rt.forward(xg).cpu().numpy(), y_def)


@pytest.mark.parametrize("tag", list(H.CASES))
def test_whole_model(tag):
    (A, h, w, s, B), sd, x, layers = lfssr_fp64_case(tag)
    whole_model_gates(tag, A, s, sd, x, layers["out"].numpy())


# ---------------------------------------------------------------------------------------------------------------------
# 7. what does not follow the mode
# ---------------------------------------------------------------------------------------------------------------------
def _same_under_the_mode(fn):
    before = fn().clone()
    with BF16():
        y = fn().clone()
    torch.cuda.synchronize()
    return torch.equal(y, before)


def test_what_does_not_follow_the_mode():
    # DistgSSR at 5 x 5: its AngConv is a different operator
    sd, x = distg_case(5, 2, 2, 8, 8)
    rtd = capi.DistgSSRRuntime(5, 2)
    rtd.load_state([(k, torch.from_numpy(v).cuda()) for k, v in sd.items()], torch.device("cuda"))
    xd = torch.from_numpy(x).cuda()
    assert _same_under_the_mode(lambda: rtd.forward(xd))
    # EPIT
    sde, xe = epit_case(5, 2, 1, 8, 8)
    rte = capi.ModelRuntime("epit", 5, 2, 5, 64)
    rte.load_state([(k, torch.from_numpy(v).cuda()) for k, v in sde.items()], torch.device("cuda"))
    xeg = torch.from_numpy(xe).cuda()
    assert _same_under_the_mode(lambda: rte.forward(xeg))
    # LFSSR's other operators
    A, Hh, Ww, B = 3, 5, 7, 2
    n_img = B * A * A
    rows = rnd((n_img * Hh * Ww, 64), 4).float().cuda()
    w64 = capi.pack_conv_weight(rnd((64, 64, 3, 3), 5, 1.0 / 24.0).float().cuda())
    assert _same_under_the_mode(lambda: capi.conv3x3(rows, w64, n_img, Hh, Ww, slope=1.0))
    w256, b256 = capi.pack_ps2_weight(rnd((256, 64, 3, 3), 5, 1.0 / 24.0).float().cuda()), rnd((256,), 6, 0.1).float().cuda()
    assert _same_under_the_mode(lambda: capi.conv3x3_ps2(rows, w256, b256, n_img, Hh, Ww))
    f2 = rnd((n_img * 4 * Hh * Ww, 64), 7).float().cuda()
    lo = torch.rand(n_img, Hh, Ww, generator=torch.Generator().manual_seed(8)).cuda()
    tw = [t.cuda() for t in (rnd((1, 64, 3, 3), 9, 1.0 / 24.0).float(), rnd((1,), 10, 0.1).float(), rnd((4, 1, 3, 3), 11, 1.0 / 3.0).float(), rnd((4,), 12, 0.1).float())]
    assert _same_under_the_mode(lambda: capi.lfssr_tail(f2, tw[0], tw[1], lo, tw[2], tw[3], B, A, Hh, Ww, True))
    # LFSR_ARITH_F32 wins
    (A, h, w, s, B), sd, x = H.lfssr_case("a3h6w8s2")
    rt = runtime(A, s, sd)
    xg = dev(x)
    with modes(arith=capi.ARITH_F32):
        alone = rt.forward(xg).clone()
    with modes(arith=capi.ARITH_F32, ang=capi.ANG_ARITH_BF16):
        both = rt.forward(xg).clone()
    assert torch.equal(alone, both)
    # the mode is live at this geometry (so the comparison above is not vacuous), and after it the default forward is what it was
    default = rt.forward(xg).clone()
    with BF16():
        y = rt.forward(xg).clone()
    assert not torch.equal(y, default)
    assert capi.get_ang_arithmetic() == capi.ANG_ARITH_DEFAULT
    assert torch.equal(rt.forward(xg), default)


# ---------------------------------------------------------------------------------------------------------------------
# 8. graphs
# ---------------------------------------------------------------------------------------------------------------------
def test_graphed_forward_follows_the_ang_arithmetic():
    """a graph captured under the default must not be replayed under the mode: GraphedForward keys its cache on this selection as well"""
    A, h, w, s, B = H.CASES["a3h6w8s2"]
    sd = H.lfssr_state_dict(H.lfssr_spec(s, n_layer=1))
    xg = dev(H.lfssr_case("a3h6w8s2")[2])
    rt = runtime(A, s, sd, n_layer=1)
    gf = capi.GraphedForward(rt)
    y_graph_def = gf(xg).clone()
    y_def = rt.forward(xg).clone()
    with BF16():
        y_graph = gf(xg).clone()
        y_eager = rt.forward(xg).clone()
        torch.cuda.synchronize()
    assert torch.equal(y_graph_def, y_def)
    assert torch.equal(y_graph, y_eager) and not torch.equal(y_graph, y_def)
    assert len(gf.graphs) == 2
    assert torch.equal(gf(xg), y_def)               # back under the default: the first graph again
