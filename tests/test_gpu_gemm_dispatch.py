"""GPU: which kernel the row-GEMM / feed-forward dispatcher (csrc/rowgemm.cpp) runs, for the rows of its chains that no other test pins.

Every check is bit-equality between two routes to the same kernel, with one inequality against the neighbouring kernel so that the equality is not vacuous.
The kernels' accuracy is tested elsewhere (test_gpu_gemm_bf16.py, test_gpu_b3_accuracy.py, test_gpu_transformer_ops.py).  M = 2048 + 37 rows: above the 2048 rows
from which a linear reaches the row-streaming kernels, ragged against every tile.  Modes go through capi.set_* and are restored; selectors through the environment
(the suite's process is a lab process)."""
import contextlib

import pytest
import torch

from lfsr_amd import capi

pytestmark = pytest.mark.gpu
M = 2048 + 37
P = capi.dev_ptr


@contextlib.contextmanager
def route(monkeypatch, arith=capi.ARITH_DEFAULT, gemm=capi.GEMM_ARITH_DEFAULT, **env):
    try:
        capi.set_arithmetic(arith)
        capi.set_gemm_arithmetic(gemm)
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            yield
            torch.cuda.synchronize()
    finally:
        capi.set_arithmetic(capi.ARITH_DEFAULT)
        capi.set_gemm_arithmetic(capi.GEMM_ARITH_DEFAULT)


DEFAULT = {}
F32 = dict(arith=capi.ARITH_F32)
BF16 = dict(gemm=capi.GEMM_ARITH_BF16)


def randn(shape, seed, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).float().cuda()


def pack(w):
    return capi.pack_conv_weight(w.reshape(w.shape[0], w.shape[1], 1, 1).contiguous())


def linear(K, N, bias=False):
    x, wp, b = randn((M, K), 1), pack(randn((N, K), 2 + N, K ** -0.5)), randn((N,), 3) if bias else None

    def f():
        y = torch.zeros(M, N, device="cuda")
        capi.check(capi.load().lfsr_linear_fwd(P(x), K, 0, K, P(wp), P(b) if bias else None, None, 0, 0, P(y), N, 0, M, N, 0.1, capi.stream_ptr()), "linear")
        return y
    return f


def lnlin(K, N, ln_cols):
    x, wp, g, b = randn((M, K), 4), pack(randn((N, K), 5 + N, K ** -0.5)), 1.0 + 0.3 * randn((K,), 6), randn((K,), 7, 0.2)

    def f():
        y = torch.zeros(M, N, device="cuda")
        capi.check(capi.load().lfsr_linear_ln_fwd(P(x), K, 0, K, P(wp), P(g), P(b), 1e-5, ln_cols, None, 0, 0, 0, P(y), N, 0, None, 0, 0, 0, M, N, capi.stream_ptr()),
                   "linear_ln")
        return y
    return f


def ffn(K1, H, N2):
    x, w1p, w2p = randn((M, K1), 8), pack(randn((H, K1), 9 + H, K1 ** -0.5)), pack(randn((N2, H), 10 + H, H ** -0.5))
    g, b = 1.0 + 0.3 * randn((K1,), 11), randn((K1,), 12, 0.2)

    def f():
        y = torch.zeros(M, N2, device="cuda")
        capi.check(capi.load().lfsr_ffn_ln_fwd(P(x), K1, 0, P(g), P(b), 1e-5, P(w1p), P(w2p), P(x), K1, 0, P(y), N2, 0, M, K1, H, N2, 0.0, capi.stream_ptr()), "ffn")
        return y
    return f


def fuse0_dgrad():
    dy, act, wT = randn((M, 64), 13), randn((M, 144), 14), capi.pack_conv_weight_T(randn((64, 144, 1, 1), 15, 0.1))
    return lambda: capi.pointwise_dgrad(dy, wT, 144, act=act, act_slope=0.1)


def bits(f, monkeypatch, r):
    with route(monkeypatch, **r):
        return f().clone()


def test_a_linear_with_a_bias_runs_the_fp32_row_gemm_whatever_the_mode(monkeypatch):
    f = linear(128, 128, bias=True)
    y = bits(f, monkeypatch, DEFAULT)
    assert torch.equal(y, bits(f, monkeypatch, F32)) and torch.equal(y, bits(f, monkeypatch, BF16))
    f = linear(128, 128)
    assert not torch.equal(bits(f, monkeypatch, DEFAULT), bits(f, monkeypatch, F32))


def test_b_linear_the_row_kernels_refuse_runs_the_gather_gemm(monkeypatch):
    f = linear(128, 96)
    assert torch.equal(bits(f, monkeypatch, DEFAULT), bits(f, monkeypatch, dict(LFSR_NO_ROWGEMM="1")))
    f = linear(128, 128)
    assert not torch.equal(bits(f, monkeypatch, DEFAULT), bits(f, monkeypatch, dict(LFSR_NO_ROWGEMM="1")))


def test_c_linear_the_bf16_form_refuses_runs_the_three_term_kernel(monkeypatch):
    f = linear(128, 192)
    assert torch.equal(bits(f, monkeypatch, BF16), bits(f, monkeypatch, DEFAULT))
    f = linear(128, 128)
    assert not torch.equal(bits(f, monkeypatch, BF16), bits(f, monkeypatch, DEFAULT))


def test_d_ln_linear_bf16_and_lnlin_refuse_runs_the_three_term_panel_kernel(monkeypatch):
    f = lnlin(128, 256, 128)
    assert torch.equal(bits(f, monkeypatch, BF16), bits(f, monkeypatch, DEFAULT))
    f = lnlin(128, 384, 128)
    assert not torch.equal(bits(f, monkeypatch, BF16), bits(f, monkeypatch, DEFAULT))


@pytest.mark.parametrize("op", ["ln_linear", "linear", "ffn"])
def test_e_the_f32_selectors_run_what_arith_f32_runs(op, monkeypatch):
    f, sel = {"ln_linear": (lnlin(128, 384, 256), "LFSR_ROWGEMM"), "linear": (linear(128, 128), "LFSR_ROWGEMM"), "ffn": (ffn(128, 256, 128), "LFSR_FFN")}[op]
    y = bits(f, monkeypatch, {sel: "f32"})
    assert torch.equal(y, bits(f, monkeypatch, F32))
    assert not torch.equal(y, bits(f, monkeypatch, DEFAULT))


def test_f_ffn_the_bf16_form_refuses_runs_the_three_term_kernel(monkeypatch):
    f = ffn(64, 96, 64)
    assert torch.equal(bits(f, monkeypatch, BF16), bits(f, monkeypatch, DEFAULT))
    f = ffn(64, 128, 64)
    assert not torch.equal(bits(f, monkeypatch, BF16), bits(f, monkeypatch, DEFAULT))


def test_g_fuse0_dgrad_every_f32_selection_runs_the_fp32_panel(monkeypatch):
    f = fuse0_dgrad()
    y = bits(f, monkeypatch, F32)
    assert torch.equal(y, bits(f, monkeypatch, dict(LFSR_DGRAD_PW="f32"))) and torch.equal(y, bits(f, monkeypatch, dict(LFSR_ROWGEMM="f32")))
    assert not torch.equal(y, bits(f, monkeypatch, DEFAULT))
