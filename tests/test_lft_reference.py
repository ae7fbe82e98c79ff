"""CPU: the LFT reference graph of tests/helpers.py (lft_layers_fp64, the one the GPU tests compare every saved tensor and every gradient
with) against the numpy oracle, which tests/test_oracle_vs_golden.py pins on the reference's golden outputs, and against the torch port
-- on the whole geometry matrix of tests/test_gpu_lft_geometries.py.

The bound between two fp64 restatements is rounding.  Seen on this matrix, outputs of order 1: 3.6e-15 at most against the oracle (its
convolutions and attention are other code), and the same bits as the port once both use fp64 position tables (the same torch ops in the same
order).  The bound is 4e-14, one decade over what was seen.  The port's own _lft_pe returns its tables through .float(): casting them
back to fp64 (the fp64_port fixture of test_gpu_lft_train.py) leaves up to 3e-8 of fp32 rounding in them, and that, not arithmetic, is the
1e-10 by which port and oracle differ otherwise (1.07e-10 on row 2, 1.02e-10 on row 8 here); test_port_position_tables_are_fp32
pins the explanation."""
import time

import numpy as np
import pytest
import torch

from oracle import lfsr_oracle as O
from oracle import lfsr_torch_port as P
from tests.helpers import (LFT_DECISION_KINDS, LFT_MATRIX, LFT_PER_SAMPLE_NPIX, LFT_SAVED, lft_case, lft_keys, lft_layers_fp64, lft_position_encoding, lft_ref_to_rows,
                           lft_rows_to_ref, model_spec)

BOUND = 4e-14
ids = lambda g: "A%ds%dB%dh%dw%d" % g
torch.set_num_threads(min(torch.get_num_threads(), 16))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture
def port_fp64_pe(monkeypatch):
    """the port with position encodings that never passed through fp32"""
    monkeypatch.setattr(P, "_lft_pe", lambda l, d, temperature=10000: lft_position_encoding(l, d, temperature))


def ref_shape(kind, B, A, h, w, s):
    lay, c, _ = LFT_SAVED[kind]
    return {"vcl": (B, c, A * A, h, w), "ang": (A * A, B * h * w, c), "spa": (h * w, B * A * A, c), "hr": (B, 64, A * h * s, A * w * s)}[lay]


def test_spec_does_not_depend_on_angres():
    """model_spec("LFT", 5, s) serves every row: at every (angRes, scale) of the matrix it is the plugin's state_dict, keys, order and shapes"""
    from argparse import Namespace
    from lfsr_amd.model.SR import LFT as M
    for A, s in sorted({g[:2] for g in LFT_MATRIX}):
        net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
        spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        assert model_spec("LFT", 5, s) == spec, (A, s)
        assert len(spec) == 78


def test_position_tables_equal_the_oracles():
    """torch's and numpy's pow differ by an ulp in the frequencies, so an argument of up to 224 moves by 224 x 2.2e-16 and its sine as much"""
    for n, ours, theirs in zip((13, 15, 225), lft_position_encoding([13, 15, 225], 64), O.lft_position_encoding([13, 15, 225], 64, np.float64)):
        assert ours.dtype == torch.float64 and ours.shape == (n, 64)
        assert np.abs(ours.numpy() - theirs).max() <= 2 * 225 * 2.3e-16


def test_port_position_tables_are_fp32():
    """why the port in fp64 and the oracle had been seen 1.3e-10 apart: the port's tables are rounded to fp32 (5e-8 off), ours are not"""
    ours, ports = lft_position_encoding([225], 64)[0], P._lft_pe([225], 64)[0]
    assert ports.dtype == torch.float32
    d = float((ports.double() - ours).abs().max())
    assert 1e-9 < d < 6.1e-8, d


@pytest.mark.parametrize("geom", LFT_MATRIX, ids=ids)
def test_layers_graph_equals_oracle_and_port(geom, port_fp64_pe):
    """rows 1-9 on the numpy oracle and on the port; the last row (5x5 x 32x32, B = 8) on the port for all eight samples and on the oracle for
    sample 0 alone (measured here: 28 s for that sample on 8 cores, under the minute that would have moved the row onto the port alone)"""
    A, s, B, h, w = geom
    sd, x = lft_case(*geom)
    with torch.no_grad():
        y, layers, flips = lft_layers_fp64(x, sd, A, s)
        port = P.lft_forward.__wrapped__(torch.as_tensor(x).double(), {k: torch.tensor(v, dtype=torch.float64) for k, v in sd.items()}, A, s)
    assert y.dtype == torch.float64 and tuple(y.shape) == (B, 1, A * h * s, A * w * s) and bool(torch.isfinite(y).all())
    e_port = float((y - port).abs().max())
    nb = 1 if B * A * A * h * w > LFT_PER_SAMPLE_NPIX else B
    t0 = time.time()
    ref = O.lft_forward(x[:nb], sd, A, s)
    dt = time.time() - t0
    assert np.isfinite(ref).all()
    e_or = float(np.abs(y[:nb].numpy() - ref).max())
    print(f"{geom}: max|layers graph - oracle| = {e_or:.2e} ({nb} of {B} samples, {dt:.1f} s), - port| = {e_port:.2e}, max|ref| = {np.abs(ref).max():.3f}")
    assert e_or <= BOUND and e_port <= BOUND
    assert flips == 0 and sorted(layers) == sorted(lft_keys()) and len(layers) == 33
    for (kind, i), t in layers.items():
        assert tuple(t.shape) == ref_shape(kind, B, A, h, w, s) and t.dtype == torch.float64, (kind, i)
    # the layout maps are each other's inverse, and put view (u, v), pixel (yy, xx) of sample b at row (((b A + u) A + v) h + yy) w + xx
    b, u, v, yy, xx = B - 1, A - 1, 0, h - 1, w // 2
    row = (((b * A + u) * A + v) * h + yy) * w + xx
    for kind, i in ((0, 2), (1, 1), (3, 0), (7, 3), (6, 2), (8, 0)):
        lay, c, _ = LFT_SAVED[kind]
        t = layers[kind, i]
        rows = lft_ref_to_rows(t, lay, B)
        assert tuple(rows.shape) == (B * A * A * h * w, c)
        assert torch.equal(lft_rows_to_ref(rows.reshape(-1), lay, B, A, h, w, s), t), kind
        named = {"vcl": lambda: t[b, :, u * A + v, yy, xx], "ang": lambda: t[u * A + v, (b * h + yy) * w + xx], "spa": lambda: t[yy * w + xx, b * A * A + u * A + v]}[lay]()
        assert torch.equal(rows[row], named), kind
    t = layers[9, 0]                     # the HR pre-activation: the channel-last mosaic (B, A h s, A w s, 64)
    rows = lft_ref_to_rows(t, "hr", B)
    assert torch.equal(lft_rows_to_ref(rows.reshape(-1), "hr", B, A, h, w, s), t)
    Y, X = (u * h + yy) * s + s - 1, (v * w + xx) * s
    assert torch.equal(rows[(b * A * h * s + Y) * A * w * s + X], t[b, :, Y, X])


@pytest.mark.parametrize("geom", (LFT_MATRIX[1], LFT_MATRIX[7]), ids=ids)
def test_gradients_equal_the_ports_autograd(geom, port_fp64_pe):
    from lfsr_amd.synth import synth_input
    A, s, B, h, w = geom
    sd, x = lft_case(*geom)
    label = torch.as_tensor(synth_input((B, 1, A * h * s, A * w * s), seed=2)).double()
    grads = []
    for fn in (lambda p: lft_layers_fp64(x, p, A, s)[0], lambda p: P.lft_forward.__wrapped__(torch.as_tensor(x).double(), p, A, s)):
        p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
        torch.nn.functional.l1_loss(fn(p), label).backward()
        grads.append({k: v.grad.numpy() for k, v in p.items()})
    errs = {k: rel(grads[0][k], grads[1][k]) for k in sd}
    print(f"{geom}: gradient rel-L2, layers graph against the port's autograd: max {max(errs.values()):.2e}")
    assert len(errs) == 78 and max(errs.values()) <= BOUND


def test_forced_masks_of_its_own_decisions_change_nothing():
    """with the graph's own decisions handed back as `forced`, the output is the same and no decision counts as differing; through a B = 1
    slice of them too (what the GPU tests do at the published geometry)"""
    geom = LFT_MATRIX[1]
    A, s, B, h, w = geom
    sd, x = lft_case(*geom)
    with torch.no_grad():
        y, layers, _ = lft_layers_fp64(x, sd, A, s)
        forced = {k: v > 0 for k, v in layers.items() if k[0] in LFT_DECISION_KINDS}
        assert len(forced) == 12
        y2, _, flips = lft_layers_fp64(x, sd, A, s, forced=forced)
        assert flips == 0 and torch.equal(y, y2)
        for i in range(B):
            one = {}
            for k, m in forced.items():
                rows = lft_ref_to_rows(m, LFT_SAVED[k[0]][0], B)
                n = rows.shape[0] // B
                one[k] = lft_rows_to_ref(rows[i * n:(i + 1) * n].reshape(-1), LFT_SAVED[k[0]][0], 1, A, h, w, s)
            y1, _, flips = lft_layers_fp64(x[i:i + 1], sd, A, s, forced=one)
            assert flips == 0 and float((y1 - y[i:i + 1]).abs().max()) <= BOUND
        # one flipped decision is counted
        for k in ((7, 2), (9, 0), (5, 1)):
            f2 = dict(forced)
            f2[k] = forced[k].clone(memory_format=torch.contiguous_format)
            f2[k].view(-1)[3] = ~f2[k].view(-1)[3]
            _, _, flips = lft_layers_fp64(x, sd, A, s, forced=f2)
            assert flips >= 1, k
