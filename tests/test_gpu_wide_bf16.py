"""GPU: lfsr_set_wide_arithmetic(LFSR_WIDE_ARITH_BF16) -- LF_InterNet's wide per-view 3x3 convs (SpaConvSq 128 -> 64, SpaBottle 320 -> 64), lfsr_conv3x3_wide_fwd,
on bf16 operands (csrc/conv3x3_wide_bf16.hip: k_conv3x3_wide_bf16), and LF_InterNet's inference forward under the mode.

Emulation of the operator, r(t) = t.to(torch.bfloat16): r of x and of the weight, the sum in fp64 (stock conv2d, padding 1), LeakyReLU, then the UNROUNDED r1.  The
kernel rounds no intermediate, so it differs from the emulation by fp32 accumulation over at most K = 2880 only: the project's gate,
max abs <= 1e-4 max(1, max|emulation|) (tests/test_gpu_ang_bf16.py).  The kernel's tile is 8 rows x 32 columns of one view.
Whole model (tests/internet_stock_graph.py): the three gates of tests/test_gpu_ang_bf16.py::test_whole_model against the fp64 graph and the stock graph under
torch.autocast(bfloat16).  CPU emulation of the mode (fp64 sums, r on the operands of the two wide convs), rms against the fp64 graph / autocast's:
a5h8s2 5.9e-4 / 1.43e-3, a3h6w8s4 5.5e-4 / 1.25e-3; dPSNR +0.0015 / -0.0003 dB.
Every test restores all six arithmetic selections."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lfsr_amd import capi
from tests.helpers import model_case, op_input, op_output, op_output_read, psnr
from tests.internet_stock_graph import internet_stock

pytestmark = pytest.mark.gpu
ATOL = 1e-4
TAGS = ("a5h8s2", "a3h6w8s4")
# (n_img, h, w): a view smaller than the 8 x 32 tile; one past the tile on both axes; the fixture's; exact tiles; 300 tiles on 256 CUs (a block's second tile)
GEOMS = ((1, 5, 7), (3, 9, 33), (18, 6, 8), (2, 16, 64), (300, 8, 8))
X_LAYOUTS = {128: ((128, 0), (384, 64)), 320: ((320, 0),)}       # the model's rows, and 128 channels from 64 on in rows of 384
Y_LAYOUTS = ((128, 0), (128, 64), (64, 0))


@contextlib.contextmanager
def modes(arith=capi.ARITH_DEFAULT, gemm=capi.GEMM_ARITH_DEFAULT, wide=capi.WIDE_ARITH_DEFAULT):
    """the three selections for the block; all six are the default again after it (the settings are process-wide)"""
    try:
        capi.set_arithmetic(arith)
        capi.set_gemm_arithmetic(gemm)
        capi.set_wide_arithmetic(wide)
        yield
    finally:
        capi.set_arithmetic(capi.ARITH_DEFAULT)
        capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT)
        capi.set_gemm_arithmetic(capi.GEMM_ARITH_DEFAULT)
        capi.set_branch_arithmetic(capi.BRANCH_ARITH_DEFAULT)
        capi.set_ang_arithmetic(capi.ANG_ARITH_DEFAULT)
        capi.set_wide_arithmetic(capi.WIDE_ARITH_DEFAULT)


BF16 = functools.partial(modes, wide=capi.WIDE_ARITH_BF16)


def r(t):
    return t.to(torch.bfloat16).double()


def gate(ref):
    return ATOL * max(1.0, float(ref.abs().max()))


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def conv_rows(x, wt, n_img, h, w):
    """fp64 rows (n_img h w, 64) of the zero-padded 3x3 conv of VCL rows x (n_img h w, cin) with wt (64, cin, 3, 3)"""
    img = x.reshape(n_img, h, w, -1).permute(0, 3, 1, 2)
    return F.conv2d(img, wt, padding=1).permute(0, 2, 3, 1).reshape(n_img * h * w, 64)


@functools.lru_cache(maxsize=None)
def wide_case(cin, n_img, h, w, kind="rand", k=0):
    """-> x rows and weight (fp32), the emulation's pre-activation rows and (small cases) the unrounded ones, computed once and never written to.
    kind: "rand"; "tap": the weight is zero outside tap k; "chunk": outside the input channels [64 k, 64 k + 64); "pixel": x is zero outside one pixel"""
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    x = rnd((n_img * h * w, cin), 11 + cin + n_img).float()
    wt = rnd((64, cin, 3, 3), 5 + cin, 1.0 / (3.0 * cin ** 0.5)).float()
    if kind == "tap":
        keep = torch.zeros(9)
        keep[k] = 1.0
        wt = wt * keep.reshape(3, 3)
    if kind == "chunk":
        keep = torch.zeros(cin)
        keep[64 * k:64 * k + 64] = 1.0
        wt = wt * keep.reshape(1, cin, 1, 1)
    if kind == "pixel":
        keep = torch.zeros(n_img * h * w, 1)
        keep[((n_img - 1) * h + h // 2) * w + w // 2] = 1.0          # the centre of the last image
        x = x * keep
    pre = conv_rows(r(x), r(wt), n_img, h, w)
    exact = conv_rows(x.double(), wt.double(), n_img, h, w) if n_img * h * w <= 4096 else None
    return x, wt, pre, exact


def finish(pre, slope, res):
    y = torch.where(pre >= 0, pre, pre * slope)
    return y if res is None else y + res.double()


def run_wide(xb, yb, wp, cin, n_img, h, w, xl, yl, with_r1, slope):
    """one launch on guarded buffers (tests/helpers.py: NaN rows around x, +-1e3 in its foreign columns, a sentinel tail behind y); r1 = x's own first 64 channels"""
    yb.reset()
    rc = capi.load().lfsr_conv3x3_wide_fwd(xb.ptr, xl[0], xl[1], cin, capi.dev_ptr(wp), yb.ptr, yl[0], yl[1], xb.ptr if with_r1 else None,
                                           xl[0] if with_r1 else 0, xl[1] if with_r1 else 0, n_img, h, w, slope, capi.stream_ptr())
    assert rc == 0, rc
    return op_output_read(yb, yl[1], 64)                     # waits; every float outside the written slice kept its bits


def check_operator(cin, n_img, h, w, kind="rand", k=0, x_layouts=None, y_layouts=Y_LAYOUTS, variants=((False, 0.0), (True, 0.0), (False, 1.0), (True, 1.0))):
    x, wt, pre, exact = wide_case(cin, n_img, h, w, kind, k)
    wp = capi.pack_conv_weight(wt.cuda())
    worst = 0.0
    ybs = {ys: op_output(x.shape[0], ys, 22) for ys in {yl[0] for yl in y_layouts}}
    for xl in x_layouts or X_LAYOUTS[cin]:
        xb = op_input(x, xl[0], xl[1], 21)
        x_before = xb.t.clone()
        for yl in y_layouts:
            for with_r1, slope in variants:
                res = x[:, :64] if with_r1 else None
                em = finish(pre, slope, res)
                with BF16():
                    y = run_wide(xb, ybs[yl[0]], wp, cin, n_img, h, w, xl, yl, with_r1, slope)
                e = float((y.double() - em).abs().max())
                worst = max(worst, e / gate(em))
                assert bool(torch.isfinite(y).all())
                assert e <= gate(em), (cin, n_img, h, w, kind, k, xl, yl, with_r1, slope, e, gate(em))
        if exact is not None:                                # the yardstick itself: the default operator is the unrounded sum, and the mode is live
            yl = y_layouts[0]
            y_def = run_wide(xb, ybs[yl[0]], wp, cin, n_img, h, w, xl, yl, True, 0.0)
            ex = finish(exact, 0.0, x[:, :64])
            assert float((y_def.double() - ex).abs().max()) <= gate(ex)
            with BF16():
                y = run_wide(xb, ybs[yl[0]], wp, cin, n_img, h, w, xl, yl, True, 0.0)
            if kind != "pixel":
                assert not torch.equal(y, y_def)
        assert torch.equal(xb.t.view(torch.int32), x_before.view(torch.int32)), "x / r1 changed"
    print(f"WIDE_BF16 operator cin {cin} n_img {n_img} {h}x{w} {kind} {k}: worst max|gpu - emul| / gate {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the operator against the fp64 emulation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("cin", [128, 320])
def test_operator_against_the_fp64_emulation(cin, geom):
    check_operator(cin, *geom)


# ---------------------------------------------------------------------------------------------------------------------
# 2. taps and chunks
# ---------------------------------------------------------------------------------------------------------------------
ONE = dict(y_layouts=((128, 64),), variants=((True, 1.0),))


@pytest.mark.parametrize("tap", range(9))
def test_single_tap(tap):
    """a wrong shift moves the whole output; geometry one past the tile on both axes"""
    check_operator(128, 3, 9, 33, "tap", tap, **ONE)


@pytest.mark.parametrize("cin,chunk", [(128, 0), (128, 1), (320, 0), (320, 1), (320, 2), (320, 3), (320, 4)])
def test_single_chunk(cin, chunk):
    """a wrong chunk base pairs the weight with other channels (in rows of 384 from channel 64 on: with the +-1e3 of the foreign columns)"""
    check_operator(cin, 3, 9, 33, "chunk", chunk, **ONE)


@pytest.mark.parametrize("cin", [128, 320])
def test_single_pixel(cin):
    """x is zero but for one pixel: the output is the flipped kernel around it, zero elsewhere (plus r1)"""
    check_operator(cin, 3, 9, 33, "pixel", **ONE)
    x, wt, pre, _ = wide_case(cin, 3, 9, 33, "pixel")
    assert int((pre.abs().sum(1) > 0).sum()) == 9


# ---------------------------------------------------------------------------------------------------------------------
# 3. sentinels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", [128, 320])
def test_writes_only_its_slice(cin):
    n_img, h, w, guard, sentinel = 3, 9, 33, 64, -12345.5
    rows = n_img * h * w
    x = rnd((rows, cin), 31 + cin).float().cuda()
    wp = capi.pack_conv_weight(rnd((64, cin, 3, 3), 5, 1.0 / 48.0).float().cuda())
    x0 = x.clone()
    for choff in (0, 64):
        pool = torch.full((rows + guard, 128), sentinel, dtype=torch.float32, device="cuda")
        with BF16():
            fresh = capi.conv3x3_wide(x, cin, wp, n_img, h, w, res1=x).clone()
            got = capi.conv3x3_wide(x, cin, wp, n_img, h, w, res1=x, out=pool, out_choff=choff)
            torch.cuda.synchronize()
        assert got.data_ptr() == pool.data_ptr()
        assert bool((pool[rows:] == sentinel).all()), "guard rows written"
        assert bool((pool[:rows, 64 - choff:128 - choff] == sentinel).all()), "the 64 channels beside the slice written"
        assert not bool((pool[:rows, choff:choff + 64] == sentinel).any()), "rows left unwritten"
        assert torch.equal(pool[:rows, choff:choff + 64], fresh)
        assert torch.equal(x, x0), "x / r1 changed"


# ---------------------------------------------------------------------------------------------------------------------
# 4. determinism and batch independence
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", [128, 320])
def test_determinism_and_batch_independence(cin):
    n_img, h, w = 18, 6, 8
    x = rnd((n_img * h * w, cin), 41).float().cuda()
    wp = capi.pack_conv_weight(rnd((64, cin, 3, 3), 5, 1.0 / 48.0).float().cuda())
    with BF16():
        y = capi.conv3x3_wide(x, cin, wp, n_img, h, w, res1=x)
        y2 = capi.conv3x3_wide(x, cin, wp, n_img, h, w, res1=x)
        singles = [capi.conv3x3_wide(x[i * h * w:(i + 1) * h * w], cin, wp, 1, h, w, res1=x[i * h * w:(i + 1) * h * w]) for i in range(n_img)]
        torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and float(y.max()) > 0
    assert torch.equal(y, y2)
    assert torch.equal(y, torch.cat(singles))


# ---------------------------------------------------------------------------------------------------------------------
# 5. the default is live and distinct
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", [128, 320])
def test_default_is_live_and_distinct(cin):
    n_img, h, w = 3, 9, 33
    x = rnd((n_img * h * w, cin), 51).float().cuda()
    wp = capi.pack_conv_weight(rnd((64, cin, 3, 3), 5, 1.0 / 48.0).float().cuda())
    run = lambda: capi.conv3x3_wide(x, cin, wp, n_img, h, w, res1=x).clone()
    untouched = run()                                        # the switch never touched in this block
    with modes():
        assert torch.equal(run(), untouched)
    with modes(arith=capi.ARITH_F32):
        f32 = run()
    with modes(arith=capi.ARITH_F32, wide=capi.WIDE_ARITH_BF16):
        assert torch.equal(run(), f32)                       # LFSR_ARITH_F32 wins ...
    assert torch.equal(f32, untouched)                       # ... and is the default's kernel for this operator
    with BF16():
        assert not torch.equal(run(), untouched)
    assert capi.get_wide_arithmetic() == capi.WIDE_ARITH_DEFAULT
    assert torch.equal(run(), untouched)


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [capi.WIDE_ARITH_DEFAULT, capi.WIDE_ARITH_BF16])
def test_refusals_write_nothing(wide):
    cin, n_img, h, w = 128, 2, 5, 7
    x, wt, _, _ = wide_case(cin, n_img, h, w)
    xb, yb = op_input(x, 384, 64, 1), op_output(x.shape[0], 128, 2)
    wp = capi.pack_conv_weight(wt.cuda())
    lib, st = capi.load(), capi.stream_ptr()
    P = capi.dev_ptr

    def call(x_=xb.ptr, xs=384, xo=64, cin_=cin, w_=None, y_=yb.ptr, ys=128, yo=64, r_=xb.ptr, rs=384, ro=64, n_=n_img, h_=h, w__=w):
        return lib.lfsr_conv3x3_wide_fwd(x_, xs, xo, cin_, w_ or P(wp), y_, ys, yo, r_, rs, ro, n_, h_, w__, 0.0, st)

    off4 = lambda p: C.c_void_p(p.value + 4)
    with modes(wide=wide):
        bad = [call(x_=None), call(y_=None), lib.lfsr_conv3x3_wide_fwd(xb.ptr, 384, 64, cin, None, yb.ptr, 128, 64, None, 0, 0, n_img, h, w, 0.0, st),
               call(cin_=64), call(cin_=192), call(cin_=0), call(cin_=256), call(xs=320, xo=0, cin_=384),
               call(n_=0), call(n_=-1), call(h_=0), call(w__=0), call(h_=-3),
               call(xs=128, xo=64), call(xs=188, xo=64), call(ys=64, yo=4), call(ys=124, yo=64), call(rs=64, ro=4), call(rs=124, ro=64),
               call(xo=-4), call(yo=-4), call(ro=-4), call(xs=-384), call(ys=-128), call(rs=-384),
               call(xs=386), call(xo=66), call(ys=130), call(yo=62, ys=128), call(rs=386), call(ro=66),
               call(x_=off4(xb.ptr)), call(y_=off4(yb.ptr)), call(r_=off4(xb.ptr)), call(w_=off4(P(wp))),
               call(n_=1 << 20, h_=32, w__=32),             # 2^30 rows: far past 2 GiB
               call(n_=1399, h_=32, w__=32, xs=384),        # 1,432,576 rows x 384 floats = 2^29 + 13,238,272 floats: x just past 2 GiB
               call(n_=4195, h_=32, w__=32, xs=128, xo=0, ys=128, rs=128, ro=0)]   # 4,295,680 rows x 128 floats: x, y and r1 just past 2 GiB
        assert bad == [-1] * len(bad), bad
        op_output_read(yb, 0, 0)                             # nothing written
        assert call() == 0
        op_output_read(yb, 64, 64)
        assert call(r_=None, rs=0, ro=0) == 0                # no residual: its stride and offset are not looked at
        assert call(r_=None, rs=-2, ro=3) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. whole model
# ---------------------------------------------------------------------------------------------------------------------
def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def runtime(case, sd):
    rt = capi.ModelRuntime("internet", case["A"], case["s"], 4, 4)
    rt.load_state([(k, dev(v)) for k, v in sd.items()], torch.device("cuda", 0))
    return rt


@functools.lru_cache(maxsize=None)
def model_refs(tag):
    """-> case, state_dict, input, the fp64 graph's output and stock torch's under autocast(bfloat16) (computed once, shared, never written to)"""
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    case, sd, x, _ = model_case("LF_InterNet", tag)
    y64 = internet_stock(x, sd, case["A"], case["s"]).numpy()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        y_amp = internet_stock(x, sd, case["A"], case["s"], dtype=torch.float32).double().numpy()
    return case, sd, x, y64, y_amp


@pytest.mark.parametrize("tag", TAGS)
def test_whole_model(tag):
    case, sd, x, y64, y_amp = model_refs(tag)
    label = torch.rand(y64.shape, generator=torch.Generator().manual_seed(2)).numpy()
    rt = runtime(case, sd)
    xg = dev(x)
    y_def = rt.forward(xg).cpu().numpy()
    e_amp, e_def = _rms(y_amp, y64), _rms(y_def, y64)
    assert np.abs(y_def - y64).max() <= ATOL * max(1.0, np.abs(y64).max())            # the default is what it was
    fails, got = [], {}
    for name, arith, gemm in (("wide mode", capi.ARITH_DEFAULT, capi.GEMM_ARITH_DEFAULT), ("wide + gemm modes", capi.ARITH_DEFAULT, capi.GEMM_ARITH_BF16),
                              ("wide + conv modes", capi.ARITH_BF16, capi.GEMM_ARITH_DEFAULT)):
        with modes(arith=arith, gemm=gemm, wide=capi.WIDE_ARITH_BF16):
            y = got[name] = rt.forward(xg).cpu().numpy()
        dpsnr = psnr(y, label) - psnr(y64, label)
        e = _rms(y, y64)
        print(f"internet {tag} {name}: rms {e:.2e} max {np.abs(y - y64).max():.2e} vs fp64; autocast rms {e_amp:.2e} (ratio {e_amp / e:.2f}); "
              f"default mode rms {e_def:.2e}; dPSNR vs label {dpsnr:+.5f} dB (autocast {psnr(y_amp, label) - psnr(y64, label):+.5f})")
        if not abs(dpsnr) <= 0.01:                      # (a) the project's gate
            fails.append((name, "dPSNR", dpsnr))
        if not e <= e_amp:                              # (b) not worse than the reduced-precision path of stock torch
            fails.append((name, "rms", e, e_amp))
        if np.array_equal(y, y_def):                    # (c) the mode is live in the model driver
            fails.append((name, "equal to the default"))
    assert not fails, fails
    assert np.array_equal(got["wide + conv modes"], got["wide mode"])      # LF_InterNet's inference has no 64 -> 64 conv
    assert np.array_equal(rt.forward(xg).cpu().numpy(), y_def)


# ---------------------------------------------------------------------------------------------------------------------
# 8. what does not follow the switch
# ---------------------------------------------------------------------------------------------------------------------
def _same_under_the_mode(fn):
    before = fn().clone()
    with BF16():
        y = fn().clone()
    torch.cuda.synchronize()
    return torch.equal(y, before)


def test_a_training_step_does_not_follow_the_switch():
    from lfsr_amd.synth import synth_input
    from tests.test_gpu_internet_train import hip_step, make_net
    case, sd, x, _ = model_case("LF_InterNet", "a3h6w8s4")
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    net, _ = make_net(A, s, sd)
    xg = torch.from_numpy(x).cuda()
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).cuda()
    _, bucket, out = hip_step(net, xg, label)
    with BF16():
        _, bucket_m, out_m = hip_step(net, xg, label)
        with torch.no_grad():
            y_inf = net(xg).clone()                         # ... while the same plugin's inference forward does
    assert torch.equal(out_m, out) and torch.equal(bucket_m, bucket)
    assert not torch.equal(y_inf, out)


def test_other_operators_and_models_do_not_follow_the_switch():
    from tests import lfssr_helpers as H
    from tests.test_gpu_lfssr import runtime as lfssr_runtime
    n_img, Hh, Ww = 18, 5, 7
    rows = rnd((n_img * Hh * Ww, 64), 4).float().cuda()
    w64 = capi.pack_conv_weight(rnd((64, 64, 3, 3), 5, 1.0 / 24.0).float().cuda())
    assert _same_under_the_mode(lambda: capi.conv3x3(rows, w64, n_img, Hh, Ww, slope=1.0))
    w96 = capi.pack_conv_weight(rnd((96, 64, 3, 3), 6, 1.0 / 24.0).float().cuda())
    lib = capi.load()

    def conv_n():
        y = torch.empty((rows.shape[0], 96), device="cuda")
        capi.check(lib.lfsr_conv3x3_n_fwd(capi.dev_ptr(rows), 64, 0, capi.dev_ptr(w96), capi.dev_ptr(y), 96, 0, n_img, Hh, Ww, 96, 0.2, capi.stream_ptr()), "conv3x3_n")
        return y

    assert _same_under_the_mode(conv_n)
    bias = rnd((64,), 7, 0.1).float().cuda()
    assert _same_under_the_mode(lambda: capi.angconv3x3(rows, w64, bias, 2, 3, Hh * Ww))
    # DistgSSR and LFSSR at their smallest fixture cases
    case, sd, x, _ = model_case("DistgSSR", "a3h6w8s2")
    rtd = capi.DistgSSRRuntime(case["A"], case["s"])
    rtd.load_state([(k, dev(v)) for k, v in sd.items()], torch.device("cuda"))
    xd = dev(x)
    assert _same_under_the_mode(lambda: rtd.forward(xd))
    (A, h, w, s, B), sdl, xl = H.lfssr_case("a2h5w7s4")
    rtl = lfssr_runtime(A, s, sdl)
    xlg = dev(xl)
    assert _same_under_the_mode(lambda: rtl.forward(xlg))


# ---------------------------------------------------------------------------------------------------------------------
# 9. plugin and graphs
# ---------------------------------------------------------------------------------------------------------------------
def test_plugin_under_no_grad_follows_the_switch():
    from tests.test_gpu_internet_train import make_net
    case, sd, x, _ = model_case("LF_InterNet", "a3h6w8s4")
    net, _ = make_net(case["A"], case["s"], sd)
    net = net.eval()
    rt = runtime(case, sd)
    xg = dev(x)
    y_def = rt.forward(xg).clone()
    with BF16():
        want = rt.forward(xg).clone()
        with torch.no_grad():
            y = net(xg, None).clone()
    assert torch.equal(y, want) and not torch.equal(y, y_def)
    with torch.no_grad():
        assert torch.equal(net(xg, None), y_def)


def test_graphed_forward_follows_the_wide_arithmetic():
    """a graph captured under the default must not be replayed under the mode: GraphedForward keys its cache on this selection as well"""
    case, sd, x, _ = model_case("LF_InterNet", "a3h6w8s4")
    rt = runtime(case, sd)
    xg = dev(x)
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
