"""GPU: lfsr_window_attn_bwd at the EPI attention's geometry (EPIT.py:93-128) against fp64 autograd of the masked attention built from
O.epit_gen_mask, the reference test_gpu_epit.py::test_epi_attention_vs_masked_mha builds for the forward.  Both paths: the matrix-pipe kernel
k_epi_attn_bwd_mfma (attn_bwd_mfma.hip, the default where it covers the geometry) and the VALU pair (trans_bwd.hip; LFSR_ATTN=valu).

Gate: rel-L2 of each of dQ, dK, dV <= 1e-5.  Stock fp32 autograd sits at 2e-7 on these shapes; 1e-5 is the forward test's own gate and leaves
room for the raw v_exp_f32 of the recomputed softmax."""
import numpy as np
import pytest
import torch

from lfsr_amd import capi
from oracle import lfsr_oracle as O
from tests.helpers import ATTN_SENTINEL, attn_bwd_layout, attn_bwd_run, rel_l2

pytestmark = pytest.mark.gpu
E, NH = 128, 8
# the operands sit inside wider rows at non-zero channel offsets: everything outside them must be left alone
QK_STRIDE, Q_OFF, K_OFF, V_STRIDE, V_OFF, O_STRIDE, O_OFF = attn_bwd_layout(E)      # 288, 16, 148; 144, 8; 136, 4
SENTINEL = ATTN_SENTINEL

# (B, A, h, w): the sequence is A x h (horizontal pass) or A x w (vertical pass) tokens
GEOMS = [(2, 3, 6, 8),       # L = 18 / 24: window wider than the sequence, run-time n1
         (1, 5, 32, 2),      # L = 160 (all ten tiles) / L = 10 (less than one tile)
         (1, 5, 20, 2),      # L = 100: ragged last tile
         (2, 3, 20, 7),      # L = 60: interior band at run-time n1 / L = 21
         (1, 5, 36, 2),      # L = 180: beyond the matrix-pipe kernel, which must hand over to the VALU pair
         (1, 8, 20, 2),      # L = 160 at run-time n1 (k_epi_attn_bwd_mfma<10, 0>: all ten tiles) / L = 16
         (1, 15, 10, 1),     # L = 150, n1 = 15 / a 15-token pass
         (2, 1, 8, 3),       # n1 = 1
         (1, 5, 3, 32),      # the window (5 left, 6 right) wider than a 3-token column / L = 160
         (1, 7, 23, 2)]      # L = 161: one past the bound, the hand-over to the VALU pair at A != 5


def rnd(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def geometry(B, A, h, w, vertical):
    HW = h * w
    if not vertical:
        return (B, A, w, A * A * HW, HW, 1, A, h, A * HW, w)
    return (B, A, h, A * A * HW, A * HW, w, A, w, HW, 1)


def reference(q, k, v, d_o, B, A, h, w, vertical):
    """fp64 autograd of softmax(q k^T / sqrt(hd) + mask) v per head on the sequences of AltFilter.forward (EPIT.py:150/156): (O, dQ, dK, dV) in pixel rows"""
    def to_seq(t):
        t = t.reshape(B, A, A, h, w, E)                                                      # b u v y x e
        if not vertical:
            return t.permute(1, 3, 0, 2, 4, 5).reshape(A * h, B * A * w, E)                  # (u y) (b v x)
        return t.permute(2, 4, 0, 1, 3, 5).reshape(A * w, B * A * h, E)                      # (v x) (b u y)
    n = w if vertical else h
    L, hd = A * n, E // NH
    mask = torch.from_numpy(O.epit_gen_mask(A, n, 2 * A, 11, np.float64))
    qt, kt, vt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, k, v))
    heads = lambda t: to_seq(t).reshape(L, -1, hd).permute(1, 0, 2)
    P = torch.softmax(heads(qt) @ heads(kt).transpose(1, 2) / np.sqrt(hd) + mask, -1)
    out = P @ heads(vt)                                                                      # (N heads, L, hd)
    dseq = heads(torch.tensor(d_o, dtype=torch.float64))
    # the output in pixel rows: scatter back through the same (linear) rearrangement
    ot = torch.zeros(q.shape, dtype=torch.float64, requires_grad=True)
    o_rows, = torch.autograd.grad((heads(ot) * out.detach()).sum(), ot)
    dq, dk, dv = torch.autograd.grad((out * dseq).sum(), (qt, kt, vt))
    return o_rows.numpy(), dq.numpy(), dk.numpy(), dv.numpy()


def run(lib, q, k, v, o, d_o, geom, vertical):
    B, A, h, w = geom
    return attn_bwd_run(lib, q, k, v, o, d_o, NH, geometry(B, A, h, w, vertical) + (A, A, 5, 6, 0))


rel = rel_l2


@pytest.mark.parametrize("vertical", [0, 1])
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "b%da%dh%dw%d" % g)
@pytest.mark.parametrize("path", ["mfma", "valu"])
def test_epi_attention_backward_vs_fp64(path, geom, vertical, monkeypatch):
    lib = capi.load()
    B, A, h, w = geom
    npix = B * A * A * h * w
    q, k, v, d_o = rnd((npix, E), 7), rnd((npix, E), 8), rnd((npix, E), 9), rnd((npix, E), 10)
    o64, dq64, dk64, dv64 = reference(q, k, v, d_o, B, A, h, w, vertical)
    o = o64.astype(np.float32)
    got = {}
    for sel in ("mfma", "valu"):
        if sel == "valu":
            monkeypatch.setenv("LFSR_ATTN", "valu")
        else:
            monkeypatch.delenv("LFSR_ATTN", raising=False)
        dqk, dv = run(lib, q, k, v, o, d_o, geom, vertical)
        dqk2, dv2 = run(lib, q, k, v, o, d_o, geom, vertical)
        got[sel] = (dqk, dv, dqk2, dv2)
        errs = (rel(dqk[:npix, Q_OFF:Q_OFF + E].cpu().numpy(), dq64), rel(dqk[:npix, K_OFF:K_OFF + E].cpu().numpy(), dk64),
                rel(dv[:npix, V_OFF:V_OFF + E].cpu().numpy(), dv64))
        print(f"{sel}: geom {geom} vertical {vertical}: rel-L2 dQ {errs[0]:.2e} dK {errs[1]:.2e} dV {errs[2]:.2e}")
        got[sel] += (errs,)
    dqk, dv, dqk2, dv2, errs = got[path]
    assert max(errs) <= 1e-5, errs
    assert torch.equal(dqk, dqk2) and torch.equal(dv, dv2)          # no float atomics: the same bits from two runs
    keep = torch.ones(QK_STRIDE, dtype=torch.bool)
    keep[Q_OFF:Q_OFF + E] = False
    keep[K_OFF:K_OFF + E] = False
    assert bool((dqk[:, keep.cuda()] == SENTINEL).all())            # channels and rows outside the operands are left untouched
    assert bool((dqk[npix:] == SENTINEL).all()) and bool((dv[npix:] == SENTINEL).all())
    keepv = torch.ones(V_STRIDE, dtype=torch.bool)
    keepv[V_OFF:V_OFF + E] = False
    assert bool((dv[:, keepv.cuda()] == SENTINEL).all())
    L = A * (w if vertical else h)
    if L > 160:      # not covered by the matrix-pipe kernel: both selections run the VALU pair
        assert torch.equal(got["mfma"][0], got["valu"][0]) and torch.equal(got["mfma"][1], got["valu"][1])
    else:            # ... and where it is covered the default is a different kernel (its sums run in another order)
        assert not torch.equal(got["mfma"][0], got["valu"][0])
