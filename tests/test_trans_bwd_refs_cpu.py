"""CPU: the fp64 references tests/test_gpu_trans_bwd_ops.py compares the HIP backward operators with, checked on their own."""
import numpy as np
import pytest
import torch

from oracle import lfsr_oracle as O
from tests.helpers import LFT_NH, LFT_SPA_GEOMS, lft_spa_attn_ref, ln_bwd_closed_form, ln_bwd_ref, tail_bwd_ref, tail_du_rows

F = torch.nn.functional


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


@pytest.mark.parametrize("C,M,pe_rows,pe_div", [(64, 333, 0, 1), (128, 500, 25, 7), (64, 200, 91, 1)])
def test_layernorm_backward_closed_form_is_autograd(C, M, pe_rows, pe_div):
    """the closed form csrc/trans_bwd.hip quotes (dx = rstd (dy g - mean(dy g) - xhat mean(dy g xhat)), dgamma = sum dy xhat, dbeta = sum dy) on x + pe rows"""
    x, gamma, dy = rnd((M, C), 1, 2.0) + rnd((M, 1), 2), 1 + 0.3 * rnd((C,), 3), rnd((M, C), 4)
    per = rnd((pe_rows, C), 5)[(torch.arange(M) // pe_div) % pe_rows] if pe_rows else None
    ref = ln_bwd_ref(x, per, gamma, dy, torch.float64)
    got = ln_bwd_closed_form(x if per is None else x + per, gamma, dy)
    for a, b in zip(got, ref):
        assert float((a - b).abs().max()) < 1e-11


def test_leaky_relu_derivative_at_zero_is_the_slope():
    """torch takes the slope at z = 0 and z = -0 (derivative 1 for z > 0 only), the convention of k_tail_bwd (`z > 0 ? 1 : slope`); the activation itself is 0 there
    under either reading (k_hr_tail forms it with z >= 0)"""
    for dt in (torch.float32, torch.float64):
        z = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 2.0, -3.0], dtype=dt, requires_grad=True)
        y = F.leaky_relu(z, 0.2)
        y.sum().backward()
        assert z.grad.tolist() == pytest.approx([0.2, 0.2, 1.0, 0.2, 1.0, 0.2])
        assert y[:2].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("B,A,h,w,s", [(2, 3, 5, 7, 2), (1, 2, 3, 4, 3), (1, 1, 1, 1, 4)])
def test_tail_reference_rows_and_columns(B, A, h, w, s):
    """tail_du_rows against pixel_unshuffle-style indexing of autograd's dHR, element by element; the planted zeros take the slope"""
    Hs, Ws, s2 = A * h * s, A * w * s, s * s
    hr = rnd((B * Hs * Ws, 64), 10)
    hr.view(-1)[::53] = 0.0
    hr.view(-1)[7::101] = -0.0
    w3, dout = rnd((576,), 11, 0.05), rnd((B * Hs * Ws,), 12)
    du, dw3 = tail_bwd_ref(hr, w3, dout, B, A, h, w, s, 0.2, torch.float64)
    # autograd once more, here: dHR (B, 64, Hs, Ws)
    t = hr.reshape(B, Hs, Ws, 64).permute(0, 3, 1, 2).clone(memory_format=torch.contiguous_format).requires_grad_(True)
    wt = w3.reshape(1, 64, 3, 3).clone().requires_grad_(True)
    F.conv2d(F.leaky_relu(t, 0.2), wt, padding=1).backward(dout.reshape(B, 1, Hs, Ws))
    assert torch.equal(dw3, wt.grad.reshape(-1))
    # pixel_unshuffle sends [b][c][Y s + i][X s + j] to channel c s^2 + i s + j of LR pixel (Y, X) of the mosaic; the rows are the mosaic's pixels view by view
    un = F.pixel_unshuffle(t.grad, s)                                                         # (B, 64 s^2, A h, A w)
    rows = un.reshape(B, 64 * s2, A, h, A, w).permute(0, 2, 4, 3, 5, 1).reshape(-1, 64 * s2)      # (b, u, v, y, x)
    assert torch.equal(du, rows)
    assert torch.equal(tail_du_rows(t.grad, B, A, h, w, s), rows)
    g = np.random.default_rng(0)
    for _ in range(200):                                                                       # ... and the index formula of the header, spelled out
        b, u, v, y, x, c, i, j = (int(g.integers(n)) for n in (B, A, A, h, w, 64, s, s))
        p = (((b * A + u) * A + v) * h + y) * w + x
        assert du[p, c * s2 + i * s + j] == t.grad[b, c, (u * h + y) * s + i, (v * w + x) * s + j]
    # the derivative at the planted zeros: dHR = slope x the gradient of the activation
    ta = F.leaky_relu(t.detach(), 0.2).requires_grad_(True)
    F.conv2d(ta, wt.detach(), padding=1).backward(dout.reshape(B, 1, Hs, Ws))
    zero = t.detach() == 0
    assert int(zero.sum()) > 0 and torch.equal(t.grad[zero], (ta.grad * 0.2)[zero])


def spa_window_ref(q, k, v, d_o, n, h, w):
    """the same attention with every query's 25 window candidates gathered ([i-2, i+3) x [j-2, min(j+3, h, w)); no dense mask): fp64 autograd -> (o, dq, dk, dv)"""
    E, hd = q.shape[1], q.shape[1] // LFT_NH
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    offs = [(di, dj) for di in range(-2, 3) for dj in range(-2, 3)]
    KI = np.stack([ii + di for di, _ in offs], -1).reshape(h * w, 25)
    KJ = np.stack([jj + dj for _, dj in offs], -1).reshape(h * w, 25)
    valid = torch.from_numpy((KI >= 0) & (KI < h) & (KJ >= 0) & (KJ < min(h, w)))
    kidx = torch.from_numpy((np.clip(KI, 0, h - 1) * w + np.clip(KJ, 0, w - 1)).reshape(-1))
    qt, kt, vt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, k, v))
    qq, kk, vv = (t.reshape(n, h * w, LFT_NH, hd) for t in (qt, kt, vt))
    kg, vg = kk[:, kidx].reshape(n, h * w, 25, LFT_NH, hd), vv[:, kidx].reshape(n, h * w, 25, LFT_NH, hd)
    S = torch.einsum("cpnd,cpknd->cpnk", qq, kg) / np.sqrt(hd)
    S = torch.where(valid[None, :, None, :], S, torch.full_like(S, -np.inf))
    out = torch.einsum("cpnk,cpknd->cpnd", torch.softmax(S, -1), vg).reshape(n * h * w, E)
    dq, dk, dv = torch.autograd.grad((out * torch.tensor(d_o, dtype=torch.float64)).sum(), (qt, kt, vt))
    return out.detach().numpy(), dq.numpy(), dk.numpy(), dv.numpy()


@pytest.mark.parametrize("n,h,w", [(2, 7, 9), (4, 3, 5)])
def test_spatial_dense_mask_reference_equals_gathered_window_form(n, h, w):
    q, k, v, d_o = [np.random.default_rng(60 + i).standard_normal((n * h * w, 128)).astype(np.float32) for i in range(4)]
    for a, b in zip(lft_spa_attn_ref(q, k, v, d_o, n, h, w), spa_window_ref(q, k, v, d_o, n, h, w)):
        assert np.isfinite(a).all() and np.isfinite(b).all()
        assert np.abs(a - b).max() < 1e-12


@pytest.mark.parametrize("n,h,w", LFT_SPA_GEOMS)
def test_spatial_cases_have_no_empty_window(n, h, w):
    """every chosen geometry keeps w <= h + 2: no row of the reference's mask is all -inf (an empty window's gradient is unspecified)"""
    mask = O.lft_gen_mask(h, w, 5, np.float64)
    assert w <= h + 2 and bool((mask == 0).any(-1).all())
    if (n, h, w) == (2, 7, 9):          # ... and there the last column sees exactly one key column
        assert int((mask.reshape(h, w, h, w)[3, 8] == 0).any(0).sum()) == 1
