"""GPU: lfsr_set_gemm_arithmetic(LFSR_GEMM_ARITH_BF16) -- the transformers' bias-free linear, LayerNorm + q | k | v projection and feed-forward block on bf16
operands (csrc/gemm_bf16.hip): activations and weights rounded to bf16 (nearest even), exact products, fp32 accumulation / LayerNorm / ReLU / residual add.

Emulation, fp64 on the CPU, r(t) = t.to(torch.bfloat16).double(); y_exact is the same graph without r:
  linear      act(r(x) r(W)^T) (+ res)
  LN-linear   r(LN(x + pe)) r(W[:ln_cols])^T | r(x) r(W[ln_cols:])^T
  FFN         res + r(relu(r(LN(x)) r(W1)^T)) r(W2)^T
Gates.  The linear rounds no intermediate, so it differs from its emulation by fp32 accumulation only: the suite's max abs <= 1e-4 (an fp32 CPU stand-in gives 9.5e-7 at
K = 128 on unit-variance x and W ~ 1 / sqrt(K)); the same holds for the v columns of the LN-linear, which see x itself.  The LN-linear's q | k columns and the FFN round
intermediates the kernel computed in fp32: an element on the other side of a rounding tie moves one operand by a whole bf16 ulp (isolated max-abs differences up to
1.9e-3 in the stand-in), so the gate there is ||y_gpu - y_emul||_2 <= 0.1 ||y_emul - y_exact||_2 (stand-in ratios 0.0025 FFN E = 128, 0.0097 FFN E = 64, 0.0033 LN-linear
E = 64: a tenfold margin); by the triangle inequality the kernel's error against y_exact is then within 10 % of the emulation's (rel-L2 1.9e-3 .. 2.4e-3).
Row counts: 2048 (the threshold below which lfsr_linear_fwd does not reach the row-streaming kernels), 2048 + 37 (ragged against the 16-row wave groups and the 64- /
128-row tiles), 65536 + 101 (more tiles than any grid holds blocks: some waves walk two or three row groups, the last one ragged); the LN-linear and the FFN have no
threshold and start at 32 * 8 + 5.
Whole-model gates: those of tests/test_gpu_conv3x3_bf16.py::test_whole_model.  CPU emulation of the mode with stock torch (every F.linear of the port except the
576 -> 128 token embedding on r-rounded operands), rms against fp64 | autocast port | ratio: EPIT (5,2,2,8,8) 2.87e-5 | 7.76e-4 | 27x, EPIT (3,4,2,12,12) 2.99e-5 |
7.18e-4 | 24x, LFT (5,2,2,8,8) 2.51e-4 | 6.15e-4 | 2.45x, LFT (3,4,2,12,12) 2.22e-4 | 5.46e-4 | 2.46x; dPSNR at most 0.0004 dB; with LFSR_ARITH_BF16 as well EPIT
5.25e-5, LFT 2.52e-4 (that emulation leaves LFT's conv-form token embedding unrounded; on the GPU it follows LFSR_ARITH_BF16).  The GPU's figures are printed and
recorded in DESIGN.md section 6g.
Every test restores all three arithmetic selections."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from oracle import lfsr_torch_port as TP
from tests.helpers import (distg_case, epit_case, epit_layers_fp64, internet_case, internet_layers_fp64, lft_case, lft_layers_fp64, op_input, op_output, op_output_read, psnr)

pytestmark = pytest.mark.gpu
ATOL = 1e-4
LFSR_E_ARG = -1
M_BIG = 65536 + 101
MS_LINEAR = (2048, 2048 + 37, M_BIG)
MS = (32 * 8 + 5, 2048 + 37, M_BIG)
P = capi.dev_ptr


@contextlib.contextmanager
def modes(arith=capi.ARITH_DEFAULT, gemm=capi.GEMM_ARITH_DEFAULT):
    """the two forward selections for the block; all three are the default again after it (the settings are process-wide)"""
    try:
        capi.set_arithmetic(arith)
        capi.set_gemm_arithmetic(gemm)
        yield
    finally:
        capi.set_arithmetic(capi.ARITH_DEFAULT)
        capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT)
        capi.set_gemm_arithmetic(capi.GEMM_ARITH_DEFAULT)


BF16 = functools.partial(modes, gemm=capi.GEMM_ARITH_BF16)


def r(t):
    return t.to(torch.bfloat16).double()


def randn(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).float()


def pack(w):
    return capi.pack_conv_weight(w.reshape(w.shape[0], w.shape[1], 1, 1).contiguous().cuda())


def act(z, slope):
    return torch.where(z >= 0, z, z * slope)


def layer_norm64(x, g, b, eps=1e-5):
    x = x.double()
    return (x - x.mean(-1, keepdim=True)) / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + eps) * g.double() + b.double()


def l2(a):
    return float(torch.linalg.vector_norm(a.double()))


# ---------------------------------------------------------------------------------------------------------------------
# operands, drawn once per shape at the largest row count (smaller launches take the first rows)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_case(K, N):
    x, w, res = randn((M_BIG, K), 100 + K), randn((N, K), 200 + K + N, K ** -0.5), randn((M_BIG, N), 300 + N)
    return x, w, res, r(x) @ r(w).T


@functools.lru_cache(maxsize=None)
def pe_rows_of(form, M, K):
    """the position-encoding row of every token: None, LFT's angular form (A^2 rows, one per view: row (m / (h w)) % A^2) and its spatial form (h w rows, row m % (h w))"""
    if form == "none":
        return None, 0, 0, None
    pe_rows, pe_div = {"views": (25, 64), "pixels": (64, 1)}[form]
    pe = randn((pe_rows, K), 700 + K + pe_rows)
    return pe, pe_rows, pe_div, pe[(torch.arange(M) // pe_div) % pe_rows]


@functools.lru_cache(maxsize=None)
def lnlin_case(K, form):
    N, ln_cols = 3 * K, 2 * K
    x, w = randn((M_BIG, K), 400 + K), randn((N, K), 500 + K, K ** -0.5)
    g, b = 1.0 + 0.3 * randn((K,), 600 + K), randn((K,), 601 + K, 0.2)
    pe, pe_rows, pe_div, per_row = pe_rows_of(form, M_BIG, K)
    xn = layer_norm64(x.double() + (per_row.double() if pe is not None else 0.0), g, b)
    emul = torch.cat([r(xn) @ r(w[:ln_cols]).T, r(x) @ r(w[ln_cols:]).T], 1)
    exact = torch.cat([xn @ w[:ln_cols].double().T, x.double() @ w[ln_cols:].double().T], 1)
    return x, w, g, b, (pe, pe_rows, pe_div), emul, exact


@functools.lru_cache(maxsize=None)
def ffn_case(E, ln):
    H = 2 * E
    x, w1, w2, res = randn((M_BIG, E), 800 + E), randn((H, E), 801 + E, E ** -0.5), randn((E, H), 802 + E, H ** -0.5), randn((M_BIG, E), 803 + E)
    g, b = 1.0 + 0.3 * randn((E,), 804 + E), randn((E,), 805 + E, 0.2)
    xn = layer_norm64(x, g, b) if ln else x.double()
    emul = r(torch.relu(r(xn) @ r(w1).T)) @ r(w2).T
    exact = torch.relu(xn @ w1.double().T) @ w2.double().T
    return x, w1, w2, res, g, b, emul, exact


def run_linear(lib, xb, K, wp, rb, r_choff, yb, y_choff, M, N, slope, x_choff=8):
    return lib.lfsr_linear_fwd(xb.ptr, xb.stride, x_choff, K, P(wp), None, rb.ptr if rb is not None else None, rb.stride if rb is not None else 0, r_choff,
                               yb.ptr, yb.stride, y_choff, M, N, slope, capi.stream_ptr())


def run_lnlin(lib, xb, K, wp, gd, bd, pe3, ped, yb, y_choff, y2b, y2_choff, M, x_choff=4, ln_cols=None, split=None):
    _, pe_rows, pe_div = pe3
    return lib.lfsr_linear_ln_fwd(xb.ptr, xb.stride, x_choff, K, P(wp), P(gd), P(bd), 1e-5, 2 * K if ln_cols is None else ln_cols,
                                  P(ped) if ped is not None else None, K if ped is not None else 0, pe_rows, pe_div,
                                  yb.ptr, yb.stride, y_choff, y2b.ptr, y2b.stride, y2_choff, 2 * K if split is None else split, M, 3 * K, capi.stream_ptr())


def run_ffn(lib, xb, x_choff, E, H, w1p, w2p, gd, bd, rptr, r_stride, r_choff, yb, y_choff, M):
    if gd is None:
        return lib.lfsr_ffn_fwd(xb.ptr, xb.stride, x_choff, P(w1p), P(w2p), rptr, r_stride, r_choff, yb.ptr, yb.stride, y_choff, M, E, H, E, 0.0, capi.stream_ptr())
    return lib.lfsr_ffn_ln_fwd(xb.ptr, xb.stride, x_choff, P(gd), P(bd), 1e-5, P(w1p), P(w2p), rptr, r_stride, r_choff, yb.ptr, yb.stride, y_choff, M, E, H, E, 0.0,
                               capi.stream_ptr())


# ---------------------------------------------------------------------------------------------------------------------
# 1. the linear: exact form on rounded operands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 128])
@pytest.mark.parametrize("N", [64, 128, 256])
def test_linear_exact_form_on_rounded_operands(K, N):
    """x at channel offset 8 of (K + 24)-float rows, res at offset 4 of (N + 8)-float rows, y at offset 12 of (N + 16)-float rows: the columns outside the N output
    channels and the sentinel rows behind row M keep their bits, NaN rows around x are not folded in"""
    lib = capi.load()
    x, w, res, z = linear_case(K, N)
    wp = pack(w)
    worst = 0.0
    for M in MS_LINEAR:
        xb, rb = op_input(x[:M], K + 24, 8, 1), op_input(res[:M], N + 8, 4, 2)
        yb = op_output(M, N + 16, 3)
        for slope in (1.0, 0.0):
            for use_r in (True, False):
                yb.reset()
                with BF16():
                    capi.check(run_linear(lib, xb, K, wp, rb if use_r else None, 4, yb, 12, M, N, slope), "linear")
                    y = op_output_read(yb, 12, N)
                ref = act(z[:M], slope) + (res[:M].double() if use_r else 0.0)
                err = float((y.double() - ref).abs().max())
                worst = max(worst, err)
                assert err <= ATOL, (K, N, M, slope, use_r, err)
    print(f"bf16 linear K {K} N {N}: max|hip - fp64(rounded operands)| {worst:.2e}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. LN-linear and FFN: rounded intermediates, the relative-L2 gate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [128, 64])
@pytest.mark.parametrize("form", ["none", "views", "pixels"])
def test_lnlin_against_the_emulation(K, form):
    lib = capi.load()
    x, w, g, b, pe3, emul, exact = lnlin_case(K, form)
    wp, gd, bd = pack(w), g.cuda(), b.cuda()
    ped = pe3[0].cuda() if pe3[0] is not None else None
    for M in MS:
        xb = op_input(x[:M], K + 12, 4, 4)
        yb, y2b = op_output(M, 2 * K + 8, 5), op_output(M, K + 12, 6)      # q | k at offset 4, v at offset 8
        with BF16():
            capi.check(run_lnlin(lib, xb, K, wp, gd, bd, pe3, ped, yb, 4, y2b, 8, M), "linear_ln")
            y = torch.cat([op_output_read(yb, 4, 2 * K), op_output_read(y2b, 8, K)], 1).double()
        d, scale = l2(y - emul[:M]), l2(emul[:M] - exact[:M])
        v_err = float((y[:, 2 * K:] - emul[:M, 2 * K:]).abs().max())
        print(f"bf16 LN-linear K {K} pe {form} M {M}: ||hip - emul|| / ||emul - exact|| {d / scale:.4f} (rel-L2 of the emulation {scale / l2(exact[:M]):.2e}); v columns max {v_err:.2e}")
        assert d <= 0.1 * scale, (K, form, M, d, scale)
        assert v_err <= ATOL, (K, form, M, v_err)


@pytest.mark.parametrize("E", [128, 64])
@pytest.mark.parametrize("ln", [True, False])
def test_ffn_against_the_emulation(E, ln):
    """res = x (the same rows), res a separate buffer, no res; with the LayerNorm (lfsr_ffn_ln_fwd) and without (lfsr_ffn_fwd)"""
    lib = capi.load()
    x, w1, w2, res, g, b, emul, exact = ffn_case(E, ln)
    w1p, w2p = pack(w1), pack(w2)
    gd, bd = (g.cuda(), b.cuda()) if ln else (None, None)
    for M in MS:
        xb, rb = op_input(x[:M], E + 8, 4, 7), op_input(res[:M], E + 4, 0, 8)
        yb = op_output(M, E + 12, 9)
        for kind, rargs, radd in (("x", (xb.ptr, xb.stride, 4), x[:M].double()), ("buffer", (rb.ptr, rb.stride, 0), res[:M].double()), ("none", (None, 0, 0), 0.0)):
            yb.reset()
            with BF16():
                capi.check(run_ffn(lib, xb, 4, E, 2 * E, w1p, w2p, gd, bd, *rargs, yb, 8, M), "ffn")
                y = op_output_read(yb, 8, E).double()
            d, scale = l2(y - (emul[:M] + radd)), l2(emul[:M] - exact[:M])
            print(f"bf16 FFN E {E} ln {ln} res {kind} M {M}: ||hip - emul|| / ||emul - exact|| {d / scale:.4f} (rel-L2 of the emulation {scale / l2(exact[:M]):.2e})")
            assert d <= 0.1 * scale, (E, ln, kind, M, d, scale)


# ---------------------------------------------------------------------------------------------------------------------
# 3. - 5. the mode is live, what must not follow, launch-size invariance and determinism
# ---------------------------------------------------------------------------------------------------------------------
def _dense_ops(M):
    """the three operators on dense operands -> {name: callable returning the output tensor(s) of one launch}"""
    lib = capi.load()
    K, N = 128, 128
    x, w, res, _ = linear_case(K, N)
    xd, rd, wp = x[:M].cuda(), res[:M].cuda(), pack(w)
    xl, wl, gl, bl, _, _, _ = lnlin_case(128, "none")
    xld, wlp, gld, bld = xl[:M].cuda(), pack(wl), gl.cuda(), bl.cuda()
    xf, w1, w2, _, gf, bf, _, _ = ffn_case(128, True)
    xfd, w1p, w2p, gfd, bfd = xf[:M].cuda(), pack(w1), pack(w2), gf.cuda(), bf.cuda()

    def linear():
        y = torch.zeros(M, N, device="cuda")
        capi.check(lib.lfsr_linear_fwd(P(xd), K, 0, K, P(wp), None, P(rd), N, 0, P(y), N, 0, M, N, 1.0, capi.stream_ptr()), "linear")
        return y

    def lnlin():
        qk, v = torch.zeros(M, 256, device="cuda"), torch.zeros(M, 128, device="cuda")
        capi.check(lib.lfsr_linear_ln_fwd(P(xld), 128, 0, 128, P(wlp), P(gld), P(bld), 1e-5, 256, None, 0, 0, 0, P(qk), 256, 0, P(v), 128, 0, 256, M, 384, capi.stream_ptr()),
                   "linear_ln")
        return torch.cat([qk, v], 1)

    def ffn():
        y = torch.zeros(M, 128, device="cuda")
        capi.check(lib.lfsr_ffn_ln_fwd(P(xfd), 128, 0, P(gfd), P(bfd), 1e-5, P(w1p), P(w2p), P(xfd), 128, 0, P(y), 128, 0, M, 128, 256, 128, 0.0, capi.stream_ptr()), "ffn")
        return y

    return {"linear": linear, "lnlin": lnlin, "ffn": ffn}


@pytest.mark.parametrize("op", ["linear", "lnlin", "ffn"])
def test_the_mode_is_live_and_leaves_the_default_alone(op):
    f = _dense_ops(2048 + 37)[op]
    before = f().clone()
    with BF16():
        y = f().clone()
    assert capi.get_gemm_arithmetic() == capi.GEMM_ARITH_DEFAULT
    after = f().clone()
    torch.cuda.synchronize()
    assert not torch.equal(y, before)
    assert torch.equal(before, after)


@pytest.mark.parametrize("op", ["linear", "ffn"])
def test_arith_f32_wins_over_the_mode(op):
    f = _dense_ops(2048 + 37)[op]
    with modes(arith=capi.ARITH_F32):
        alone = f().clone()
    with modes(arith=capi.ARITH_F32, gemm=capi.GEMM_ARITH_BF16):
        both = f().clone()
    with modes():
        default = f().clone()
    torch.cuda.synchronize()
    assert torch.equal(alone, both)
    assert not torch.equal(alone, default)      # (ARITH_F32 is a different kernel: the comparison above is not vacuous)


def test_what_does_not_follow_the_mode():
    lib = capi.load()
    # a linear below 2048 rows never reaches the row-streaming dispatcher
    f = _dense_ops(2047)["linear"]
    with BF16():
        y = f().clone()
    assert torch.equal(y, f())
    # K = 144, DistgSSR's fuse.0
    M = 4096 + 5
    x, w = randn((M, 144), 900).cuda(), randn((64, 144), 901, 144 ** -0.5)
    wp = pack(w)
    with BF16():
        y = capi.pointwise(x, 144, wp, 64, slope=0.1).clone()
    assert torch.equal(y, capi.pointwise(x, 144, wp, 64, slope=0.1))
    # hence all of DistgSSR
    A, s, B, h, w_ = 5, 2, 1, 8, 8
    sd, xin = distg_case(A, s, B, h, w_)
    rt = capi.DistgSSRRuntime(A, s)
    rt.load_state([(k, torch.from_numpy(v).cuda()) for k, v in sd.items()], torch.device("cuda"))
    xg = torch.from_numpy(xin).cuda()
    with BF16():
        y = rt.forward(xg).clone()
    assert torch.equal(y, rt.forward(xg))
    assert lib.lfsr_get_gemm_arithmetic() == 0


@pytest.mark.parametrize("op", ["linear", "lnlin", "ffn"])
def test_launch_size_invariance_and_determinism(op):
    """rows [0, M1) of a launch of M2 rows (several row groups per wave) equal the launch of M1 rows (one block per tile) bit for bit; two launches are bit-equal"""
    M1, M2 = 2048 + 37, M_BIG
    f1, f2 = _dense_ops(M1)[op], _dense_ops(M2)[op]
    with BF16():
        y1, y2, y2b = f1().clone(), f2().clone(), f2().clone()
        torch.cuda.synchronize()
    assert torch.equal(y2, y2b)
    assert torch.equal(y2[:M1], y1)


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals write nothing
# ---------------------------------------------------------------------------------------------------------------------
def _same_as_default(launch, outs):
    """launch() under the default and under the mode: the same status, and the same bits in every output buffer -- untouched ones where the status is LFSR_E_ARG"""
    results = []
    for ctx in (modes, BF16):
        for o in outs:
            o.reset()
        with ctx():
            rc = launch()
            torch.cuda.synchronize()
        results.append((rc, [o.t.clone() for o in outs]))
    (rc0, t0), (rc1, t1) = results
    assert rc0 == rc1, (rc0, rc1)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(t0, t1))
    if rc1 == LFSR_E_ARG:
        assert all(torch.equal(t.view(torch.int32), o.pristine.view(torch.int32)) for t, o in zip(t1, outs))
    return rc1


def test_refusals_write_nothing():
    lib = capi.load()
    M = 2048 + 37
    # linear: a y channel offset that is no multiple of four floats (the gather-GEMM runs, as without the mode); an x row shorter than offset + channels (refused)
    K, N = 128, 128
    x, w, res, _ = linear_case(K, N)
    wp = pack(w)
    xb, yb = op_input(x[:M], K + 24, 8, 11), op_output(M, N + 16, 12)
    assert _same_as_default(lambda: run_linear(lib, xb, K, wp, None, 0, yb, 6, M, N, 1.0), [yb]) == 0
    xs = op_input(x[:M], K + 4, 4, 13)
    assert _same_as_default(lambda: run_linear(lib, xs, K, wp, None, 0, yb, 12, M, N, 1.0, x_choff=8), [yb]) == LFSR_E_ARG
    # N = 192: the row-streaming dispatcher is reached and the mode's own launcher is what declines (it covers N in {64, 128, 256}): the three-term kernel, its bits
    w192 = pack(randn((192, K), 19, K ** -0.5))
    y192 = op_output(M, 192 + 16, 20)
    assert _same_as_default(lambda: run_linear(lib, xb, K, w192, None, 0, y192, 12, M, 192, 1.0), [y192]) == 0
    # LN-linear: misaligned y2 offset; y rows shorter than offset + q | k columns
    xl, wl, g, b, pe3, _, _ = lnlin_case(128, "none")
    wlp, gd, bd = pack(wl), g.cuda(), b.cuda()
    xlb, qb, vb = op_input(xl[:M], 128 + 12, 4, 14), op_output(M, 256 + 8, 15), op_output(M, 128 + 12, 16)
    assert _same_as_default(lambda: run_lnlin(lib, xlb, 128, wlp, gd, bd, pe3, None, qb, 4, vb, 6, M), [qb, vb]) == LFSR_E_ARG
    assert _same_as_default(lambda: run_lnlin(lib, xlb, 128, wlp, gd, bd, pe3, None, qb, 12, vb, 8, M), [qb, vb]) == LFSR_E_ARG
    # FFN: misaligned y offset; y rows shorter than offset + channels; a shape the mode does not cover, (K1, H, N2) = (128, 128, 128): the default path, its bits
    xf, w1, w2, _, gf, bf, _, _ = ffn_case(128, True)
    w1p, w2p, gfd, bfd = pack(w1), pack(w2), gf.cuda(), bf.cuda()
    xfb, yfb = op_input(xf[:M], 128 + 8, 4, 17), op_output(M, 128 + 12, 18)
    _same_as_default(lambda: run_ffn(lib, xfb, 4, 128, 256, w1p, w2p, gfd, bfd, None, 0, 0, yfb, 6, M), [yfb])      # (the fp32-MFMA kernel stores single floats: it runs)
    assert _same_as_default(lambda: run_ffn(lib, xfb, 4, 128, 256, w1p, w2p, gfd, bfd, None, 0, 0, yfb, 16, M), [yfb]) == LFSR_E_ARG
    w1h, w2h = pack(w1[:128]), pack(w2[:, :128])
    assert _same_as_default(lambda: run_ffn(lib, xfb, 4, 128, 128, w1h, w2h, gfd, bfd, None, 0, 0, yfb, 8, M), [yfb]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. whole models
# ---------------------------------------------------------------------------------------------------------------------
# >= 2048 tokens: the linears are in the mode.  LF_InterNet's only linear in it is the 128 -> 64 angular squeeze over B h w rows: 2048 at (3, 2, 2, 32, 32)
MODELS = [("epit", (5, 2, 2, 8, 8)), ("epit", (3, 4, 2, 12, 12)), ("lft", (5, 2, 2, 8, 8)), ("lft", (3, 4, 2, 12, 12)), ("internet", (3, 2, 2, 32, 32))]
_CASE = {"epit": epit_case, "lft": lft_case, "internet": internet_case}
_FP64 = {"epit": epit_layers_fp64, "lft": lft_layers_fp64, "internet": internet_layers_fp64}
_PORT = {"epit": TP.epit_forward, "lft": TP.lft_forward, "internet": TP.internet_forward}


def _runtime(name, A, s, sd):
    rt = capi.ModelRuntime(name, A, s, *{"epit": (5, 64), "lft": (4, 64), "internet": (4, 4)}[name])
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
    e_amp, e_def = _rms(y_amp, y64), _rms(y_def, y64)
    assert np.abs(y_def - y64).max() < ATOL             # the default is what it was
    for tag, arith in (("gemm mode", capi.ARITH_DEFAULT), ("gemm + conv modes", capi.ARITH_BF16)):
        with modes(arith=arith, gemm=capi.GEMM_ARITH_BF16):
            y = rt.forward(xg).cpu().numpy()
            y_tr = rt.forward_train(xg).cpu().numpy()
        dpsnr = psnr(y, label) - psnr(y64, label)
        e = _rms(y, y64)
        print(f"{name} {geom} {tag}: rms {e:.2e} max {np.abs(y - y64).max():.2e} vs fp64; autocast port rms {e_amp:.2e} (ratio {e_amp / e:.2f}); "
              f"default mode rms {e_def:.2e}; dPSNR vs label {dpsnr:+.5f} dB")
        assert abs(dpsnr) <= 0.01                       # (a) the project's gate
        assert e <= e_amp                               # (b) not worse than the reference's own reduced-precision path
        assert not np.array_equal(y, y_def)             # (c) the mode is live in the model drivers
        assert np.array_equal(y_tr, y)                  # (d) forward_train runs the same launches
    assert np.array_equal(rt.forward(xg).cpu().numpy(), y_def)


def test_internet_at_the_small_geometry_keeps_its_bits():
    """LF_InterNet's 128 -> 64 angular squeeze is a linear over B h w rows: 128 at (5, 2, 2, 8, 8), below the 2048 rows at which lfsr_linear_fwd reaches the
    row-streaming dispatcher -- nothing of this model reads the mode there (from B h w >= 2048 on the squeeze follows it: test_whole_model's last case)"""
    A, s, B, h, w = 5, 2, 2, 8, 8
    sd, x = internet_case(A, s, B, h, w)
    rt = _runtime("internet", A, s, sd)
    xg = torch.from_numpy(x).cuda()
    y_def = rt.forward(xg).clone()
    with BF16():
        y = rt.forward(xg).clone()
    assert torch.equal(y, y_def)


# ---------------------------------------------------------------------------------------------------------------------
# 8. graphs
# ---------------------------------------------------------------------------------------------------------------------
def test_graphed_forward_follows_the_gemm_arithmetic():
    """a graph captured under the default must not be replayed under the mode: GraphedForward keys its cache on both forward selections"""
    A, s, B, h, w = 5, 2, 2, 8, 8
    sd, x = epit_case(A, s, B, h, w)
    rt = _runtime("epit", A, s, sd)
    xg = torch.from_numpy(x).cuda()
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
