"""GPU: lfsr_set_arithmetic(LFSR_ARITH_BF16) -- the 64 -> 64 per-view 3x3 forward conv on bf16 operands (csrc/conv3x3_bf16.hip): activations and weights rounded
to bf16 (nearest even), exact products, fp32 accumulation / LeakyReLU / residual adds; everything else as under the default.

Operator gates: against the fp64 conv of the SAME rounded operands (torch.Tensor.bfloat16()) the kernel differs by fp32 accumulation only, so the suite's
ATOL = 1e-4 holds as for the fp32 kernels (CPU emulation of the arithmetic: 6.4e-7 on unit-variance input and 0.05-scale weights).
Whole-model gates: |dPSNR| <= 0.01 dB against a label (the project's gate) and an rms error against the fp64 graph not above that of the reference's own
reduced-precision path, the torch port under torch.autocast("cpu", bfloat16), margin 1.0x.  CPU emulation of the mode (bf16-rounded operands of every 3x3
64 -> 64 conv, fp32 otherwise) against autocast, rms error vs fp64: DistgSSR (5,2,1,8,8) 3.9e-4 vs 1.07e-3 (2.7x inside), (3,2,2,6,8) 3.7e-4 vs 1.00e-3,
EPIT (5,2,1,8,8) 4.2e-5 vs 7.7e-4; LFT (5,2,1,8,8), whose unfold + MLP of SpaTrans runs as two such convs per block besides the three of conv_init:
1.57e-4 vs 6.11e-4, ratio 3.9x (conv_init alone: 1.7e-5), dPSNR -0.0002 dB."""
import functools

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from oracle import lfsr_oracle as O
from oracle import lfsr_torch_port as TP
from tests.helpers import arithmetic, distg_case, distg_layers_fp64, epit_case, epit_layers_fp64, lft_case, lft_layers_fp64, psnr

pytestmark = pytest.mark.gpu
ATOL = 1e-4


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def rnd(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def bf16_round(a):
    """fp32 array -> the same values rounded to bf16 (nearest even), as fp64"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().double().numpy()


def to_vcl(x_macpi, A):
    return capi.nchw_to_vcl(dev(x_macpi), A, 1)


def from_vcl(v, B, C, A, h, w, choff=0):
    return capi.vcl_to_nchw(v, B, C, A, h, w, 1, choff).cpu().numpy()


GEOMS = [(1, 5, 8, 8),        # the smallest golden geometry: one ragged tile per view
         (2, 3, 6, 8),
         (3, 2, 5, 7),        # ragged and smaller than a tile both ways
         (2, 1, 37, 70),      # several tile columns and rows per view, ragged both ways
         (5, 4, 32, 32)]      # 320 tiles: more than one persistent round on 256 CUs


@functools.lru_cache(maxsize=None)
def conv_case(B, A, h, w):
    """operands as test_gpu_distgssr.py::test_conv3x3 draws them, and the fp64 conv of the bf16-ROUNDED operands (computed once per geometry)"""
    x = rnd((B, 64, A * h, A * w), 1)
    wt = rnd((64, 64, 3, 3), 2, 0.05)
    r1 = rnd((B, 64, A * h, A * w), 3)
    conv = O.conv2d(bf16_round(x), bf16_round(wt), dilation=(A, A), padding=(A, A))
    return x, wt, r1, conv


@pytest.mark.parametrize("B,A,h,w", GEOMS)
def test_exact_form_on_rounded_operands(B, A, h, w):
    x, wt, r1, conv = conv_case(B, A, h, w)
    wp = capi.pack_conv_weight(dev(wt))
    xv, rv = to_vcl(x, A), to_vcl(r1, A)
    with arithmetic(capi.ARITH_BF16):
        y1 = capi.conv3x3(xv, wp, B * A * A, h, w, slope=0.1)
        y2 = capi.conv3x3(xv, wp, B * A * A, h, w, slope=1.0, res1=rv, res2=rv)
        y3 = capi.conv3x3(xv, wp, B * A * A, h, w, slope=1.0, res2=rv)
        torch.cuda.synchronize()
    r64 = r1.astype(np.float64)
    errs = [np.abs(from_vcl(y1, B, 64, A, h, w) - O.leaky_relu(conv, 0.1)).max(),
            np.abs(from_vcl(y2, B, 64, A, h, w) - (conv + 2 * r64)).max(),
            np.abs(from_vcl(y3, B, 64, A, h, w) - (conv + r64)).max()]
    print(f"bf16 conv {(B, A, h, w)}: max|hip - fp64(rounded operands)| lrelu {errs[0]:.2e}, two residuals {errs[1]:.2e}, lone res2 {errs[2]:.2e}")
    assert max(errs) < ATOL, errs


def test_it_really_is_bf16():
    B, A, h, w = GEOMS[0]
    x, wt, _, conv = conv_case(B, A, h, w)
    exact = O.leaky_relu(O.conv2d(x.astype(np.float64), wt.astype(np.float64), dilation=(A, A), padding=(A, A)), 0.1)
    rounded = O.leaky_relu(conv, 0.1)
    wp = capi.pack_conv_weight(dev(wt))
    xv = to_vcl(x, A)
    y_def = from_vcl(capi.conv3x3(xv, wp, B * A * A, h, w, slope=0.1), B, 64, A, h, w)
    with arithmetic(capi.ARITH_BF16):
        y = from_vcl(capi.conv3x3(xv, wp, B * A * A, h, w, slope=0.1), B, 64, A, h, w)
    assert capi.get_arithmetic() == capi.ARITH_DEFAULT
    d_def, d_rounded, d_exact = np.abs(y - y_def).max(), np.abs(y - rounded).max(), np.abs(y - exact).max()
    print(f"bf16 conv: max|bf16 - default| {d_def:.2e}, vs fp64 of rounded operands {d_rounded:.2e}, vs fp64 of the operands {d_exact:.2e}")
    assert d_def > 1e-4
    assert d_rounded < d_exact and d_rounded < ATOL
    assert np.abs(y_def - exact).max() < ATOL      # (the default is untouched)


def _rows(a):
    """(n, C, h, w) -> VCL rows (n h w, C) at A = 1"""
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1).reshape(-1, a.shape[1]))


@functools.lru_cache(maxsize=None)
def ragged_case():
    n, h, w = 3, 30, 29
    x = rnd((n, 64, h, w), 41)
    wt = rnd((64, 64, 3, 3), 42, 0.05)
    r1 = rnd((n, 64, h, w), 43)
    return n, h, w, x, wt, r1


def test_strided_operands_and_untouched_memory():
    """y in channels [64, 128) of a 144-float row, x at channel offset 16 of an 80-float row, ragged 30 x 29 views: every float outside the 64 output
    channels and a sentinel row behind the last pixel keep their bits"""
    n, h, w, x, wt, r1 = ragged_case()
    M = n * h * w
    ref = _rows(O.leaky_relu(O.conv2d(bf16_round(x), bf16_round(wt), dilation=(1, 1), padding=(1, 1)), 0.1) + r1)
    xbuf = torch.from_numpy(rnd((M, 80), 44)).cuda()
    xbuf[:, 16:80] = dev(_rows(x))
    fill = torch.from_numpy(rnd((M + 1, 144), 45)).cuda()
    buf = fill.clone()
    wp = capi.pack_conv_weight(dev(wt))
    with arithmetic(capi.ARITH_BF16):
        capi.conv3x3(xbuf, wp, n, h, w, slope=0.1, res1=dev(_rows(r1)), out=buf[:M], out_choff=64, x_choff=16)
        torch.cuda.synchronize()
    assert float(np.abs(buf[:M, 64:128].cpu().numpy() - ref).max()) < ATOL
    assert torch.equal(buf[:M, :64], fill[:M, :64]) and torch.equal(buf[:M, 128:], fill[:M, 128:]) and torch.equal(buf[M], fill[M])


def test_unaligned_operands_run_the_fp32_gather_gemm():
    """a y channel offset that is no multiple of 4 floats: the tile kernels do not take it, the call runs the gather-GEMM in fp32 -- checked against the
    fp64 conv of the UNROUNDED operands"""
    n, h, w, x, wt, r1 = ragged_case()
    M = n * h * w
    ref = _rows(O.leaky_relu(O.conv2d(x.astype(np.float64), wt.astype(np.float64), dilation=(1, 1), padding=(1, 1)), 0.1) + r1)
    fill = torch.from_numpy(rnd((M + 1, 72), 46)).cuda()
    buf = fill.clone()
    wp = capi.pack_conv_weight(dev(wt))
    with arithmetic(capi.ARITH_BF16):
        capi.conv3x3(dev(_rows(x)), wp, n, h, w, slope=0.1, res1=dev(_rows(r1)), out=buf[:M], out_choff=6)
        torch.cuda.synchronize()
    assert float(np.abs(buf[:M, 6:70].cpu().numpy() - ref).max()) < ATOL
    assert torch.equal(buf[:M, :6], fill[:M, :6]) and torch.equal(buf[:M, 70:], fill[:M, 70:]) and torch.equal(buf[M], fill[M])


def test_launch_size_invariance_and_determinism():
    """30 x 29 views are 4 tiles each: on 256 CUs 100 images (400 tiles) walk two tiles on 144 of the blocks, 72 images (288 tiles) on 32 of them, 25 images
    (100 tiles) run one tile per block on 100 blocks -- an image's result must not change by a bit with the launch it is part of, nor between two identical
    launches (activation form and two-residual form)"""
    h, w, n = 30, 29, 100
    g = torch.Generator(device="cuda").manual_seed(17)
    x = torch.randn(n * h * w, 64, device="cuda", generator=g)
    r = torch.randn(n * h * w, 64, device="cuda", generator=g)
    wp = capi.pack_conv_weight(torch.randn(64, 64, 3, 3, device="cuda", generator=g) * 0.05)
    forms = [lambda k: capi.conv3x3(x[:k * h * w], wp, k, h, w, slope=0.1),
             lambda k: capi.conv3x3(x[:k * h * w], wp, k, h, w, slope=1.0, res1=r[:k * h * w], res2=r[:k * h * w])]
    with arithmetic(capi.ARITH_BF16):
        for i, f in enumerate(forms):
            y100, y100b, y25, y72 = f(100).clone(), f(100).clone(), f(25).clone(), f(72).clone()
            torch.cuda.synchronize()
            assert torch.equal(y100, y100b), i
            assert torch.equal(y100[:25 * h * w], y25), i
            assert torch.equal(y100[:25 * h * w], y72[:25 * h * w]) and torch.equal(y100[:72 * h * w], y72), i


# ---------------------------------------------------------------------------------------------------------------------
# whole models
# ---------------------------------------------------------------------------------------------------------------------
MODELS = [("distgssr", (5, 2, 1, 8, 8)), ("distgssr", (3, 2, 2, 6, 8)), ("epit", (5, 2, 1, 8, 8)), ("lft", (5, 2, 1, 8, 8))]
_CASE = {"distgssr": distg_case, "epit": epit_case, "lft": lft_case}
_FP64 = {"distgssr": distg_layers_fp64, "epit": epit_layers_fp64, "lft": lft_layers_fp64}
_PORT = {"distgssr": TP.distgssr_forward, "epit": TP.epit_forward, "lft": TP.lft_forward}


def _runtime(name, A, s, sd):
    rt = capi.DistgSSRRuntime(A, s) if name == "distgssr" else capi.ModelRuntime(name, A, s, 5 if name == "epit" else 4, 64)
    rt.load_state([(k, torch.from_numpy(v).cuda()) for k, v in sd.items()], torch.device("cuda"))
    return rt


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


@pytest.mark.parametrize("name,geom", MODELS)
def test_whole_model(name, geom):
    A, s, B, h, w = geom
    sd, x = _CASE[name](A, s, B, h, w)
    y64 = _FP64[name](x, sd, A, s)[0].numpy()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        y_amp = _PORT[name](torch.from_numpy(x), {k: torch.from_numpy(v) for k, v in sd.items()}, A, s).double().numpy()
    label = torch.rand(y64.shape, generator=torch.Generator().manual_seed(2)).numpy()
    rt = _runtime(name, A, s, sd)
    xg = torch.from_numpy(x).cuda()
    y_def = rt.forward(xg).cpu().numpy()
    with arithmetic(capi.ARITH_BF16):
        y = rt.forward(xg).cpu().numpy()
        y_tr = rt.forward_train(xg).cpu().numpy() if name == "distgssr" else None
    dpsnr = psnr(y, label) - psnr(y64, label)
    e, e_amp, e_def = _rms(y, y64), _rms(y_amp, y64), _rms(y_def, y64)
    print(f"{name} {geom}: bf16-conv mode rms {e:.2e} max {np.abs(y - y64).max():.2e} vs fp64; autocast port rms {e_amp:.2e} (ratio {e_amp / e:.2f}); "
          f"default mode rms {e_def:.2e}; dPSNR vs label {dpsnr:+.5f} dB")
    assert abs(dpsnr) <= 0.01                       # (a) the project's gate
    assert e <= e_amp                               # (b) not worse than the reference's own reduced-precision path
    assert not np.array_equal(y, y_def)             # (c) the mode is live in the model drivers
    assert np.abs(y_def - y64).max() < ATOL         #     ... and the default is what it was
    if y_tr is not None:
        assert np.array_equal(y_tr, y)              # (d) forward_train runs the same launches


def test_graphed_forward_follows_the_arithmetic():
    """a graph captured under the default must not be replayed after a mode change: GraphedForward keys its cache on the arithmetic"""
    A, s, B, h, w = 5, 2, 1, 8, 8
    sd, x = distg_case(A, s, B, h, w)
    rt = _runtime("distgssr", A, s, sd)
    xg = torch.from_numpy(x).cuda()
    gf = capi.GraphedForward(rt)
    y_graph_def = gf(xg).clone()
    y_def = rt.forward(xg).clone()
    with arithmetic(capi.ARITH_BF16):
        y_graph = gf(xg).clone()
        y_eager = rt.forward(xg).clone()
        torch.cuda.synchronize()
    assert torch.equal(y_graph_def, y_def)
    assert torch.equal(y_graph, y_eager) and not torch.equal(y_graph, y_def)
    assert len(gf.graphs) == 2
    assert torch.equal(gf(xg), y_def)               # back under the default: the first graph again
