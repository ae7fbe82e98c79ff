"""CPU: the EPIT reference graph of tests/helpers.py (epit_layers_fp64, the one the GPU tests compare every saved tensor and every gradient
with) against the numpy oracle, which tests/test_oracle_vs_golden.py pins on the reference's golden outputs, and against the torch port
-- on the whole geometry matrix of tests/test_gpu_epit_geometries.py (the published B = 8 row through one sample).

The bound between two fp64 restatements is rounding.  Seen on this matrix, outputs of order 1: 4.0e-15 at most against the oracle (its
convolutions, layer norms and attention are other code), and the same bits as the port, gradients included (the same torch ops in the same
order).  The bound against the oracle is 4e-14, one decade over what was seen."""
import time

import numpy as np
import pytest
import torch

from oracle import lfsr_oracle as O
from oracle import lfsr_torch_port as P
from tests.helpers import (EPIT_DECISION_KINDS, EPIT_MATRIX, EPIT_SAVED, epit_case, epit_keys, epit_layers_fp64, epit_layout, epit_ref_to_rows,
                           epit_rows_to_ref, epit_samples, model_spec)

BOUND = 4e-14
ids = lambda g: "A%ds%dB%dh%dw%d" % g
torch.set_num_threads(min(torch.get_num_threads(), 16))


def one_sample(geom):
    """the row as this file runs it: the published geometry through its first sample"""
    A, s, B, h, w = geom
    return (A, s, 1 if len(epit_samples(*geom)) > 1 else B, h, w)


def ref_shape(which, index, B, A, h, w, s):
    lay, c, _ = EPIT_SAVED[which]
    return {"vcl": (B, c, A * A, h, w), "tokh": (A * h, B * A * w, c), "tokv": (A * w, B * A * h, c),
            "hr": (B, 64, A * h * s, A * w * s)}[epit_layout(which, index)]


def test_spec_does_not_depend_on_angres():
    """model_spec("EPIT", 5, s) serves every row: at every (angRes, scale) of the matrix it is the plugin's state_dict, keys, order and shapes"""
    from argparse import Namespace
    from lfsr_amd.model.SR import EPIT as M
    for A, s in sorted({g[:2] for g in EPIT_MATRIX}):
        net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
        spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        assert model_spec("EPIT", 5, s) == spec, (A, s)
        assert len(spec) == 71


def test_matrix_token_counts():
    """what the rows' comments promise: (horizontal, vertical) tokens per sequence against the matrix-pipe kernels' bound of 160"""
    assert [(g[0] * g[3], g[0] * g[4]) for g in EPIT_MATRIX] == [(8, 8), (18, 14), (160, 24), (35, 161), (160, 32), (150, 45), (120, 108), (65, 75),
                                                                 (15, 160), (160, 160)]
    assert len(epit_keys()) == 40 and len(epit_keys((0, 1, 2, 3))) == 28 and len(epit_keys(EPIT_DECISION_KINDS)) == 34


@pytest.mark.parametrize("geom", EPIT_MATRIX, ids=ids)
def test_layers_graph_equals_oracle_and_port(geom):
    A, s, B, h, w = one_sample(geom)
    sd, x = epit_case(A, s, B, h, w)
    with torch.no_grad():
        y, layers, flips = epit_layers_fp64(x, sd, A, s)
        port = P.epit_forward.__wrapped__(torch.as_tensor(x).double(), {k: torch.tensor(v, dtype=torch.float64) for k, v in sd.items()}, A, s)
    assert y.dtype == torch.float64 and tuple(y.shape) == (B, 1, A * h * s, A * w * s) and bool(torch.isfinite(y).all())
    assert torch.equal(y, port)
    t0 = time.time()
    ref = O.epit_forward(x, sd, A, s)
    dt = time.time() - t0
    assert np.isfinite(ref).all()
    e_or = float(np.abs(y.numpy() - ref).max())
    print(f"{geom}: max|layers graph - oracle| = {e_or:.2e} ({B} of {geom[2]} samples, {dt:.1f} s), the port's bits, max|ref| = {np.abs(ref).max():.3f}")
    assert e_or <= BOUND
    assert flips == 0 and sorted(layers) == sorted(epit_keys()) and len(layers) == 40
    for (which, i), t in layers.items():
        assert tuple(t.shape) == ref_shape(which, i, B, A, h, w, s) and t.dtype == torch.float64, (which, i)
    # the layout maps are each other's inverse, and put view (u, v), pixel (yy, xx) of sample b at row (((b A + u) A + v) h + yy) w + xx
    b, u, v, yy, xx = B - 1, A - 1, 0, h - 1, w // 2
    row = (((b * A + u) * A + v) * h + yy) * w + xx
    for which, i in ((0, 5), (1, 1), (2, 3), (3, 8), (4, 2), (4, 7), (5, 0)):
        lay, c = epit_layout(which, i), EPIT_SAVED[which][1]
        t = layers[which, i]
        rows = epit_ref_to_rows(t, lay, B, A, h, w)
        assert tuple(rows.shape) == (B * A * A * h * w, c)
        assert torch.equal(epit_rows_to_ref(rows.reshape(-1), lay, B, A, h, w, s), t), (which, i)
        named = {"vcl": lambda: t[b, :, u * A + v, yy, xx], "tokh": lambda: t[u * h + yy, (b * A + v) * w + xx],
                 "tokv": lambda: t[v * w + xx, (b * A + u) * h + yy]}[lay]()
        assert torch.equal(rows[row], named), (which, i)
    t = layers[6, 0]                     # the HR pre-activation: the channel-last mosaic (B, A h s, A w s, 64)
    rows = epit_ref_to_rows(t, "hr", B, A, h, w)
    assert torch.equal(epit_rows_to_ref(rows.reshape(-1), "hr", B, A, h, w, s), t)
    Y, X = (u * h + yy) * s + s - 1, (v * w + xx) * s
    assert torch.equal(rows[(b * A * h * s + Y) * A * w * s + X], t[b, :, Y, X])
    # the tail's input is the last block's output plus the network skip, and every block's input is the one before it moved
    assert not torch.equal(layers[0, 5], layers[0, 4]) and not torch.equal(layers[0, 1], layers[0, 0])


@pytest.mark.parametrize("geom", (EPIT_MATRIX[1], EPIT_MATRIX[3], EPIT_MATRIX[7]), ids=ids)
def test_gradients_equal_the_ports_autograd(geom):
    from lfsr_amd.synth import synth_input
    A, s, B, h, w = geom
    sd, x = epit_case(*geom)
    label = torch.as_tensor(synth_input((B, 1, A * h * s, A * w * s), seed=2)).double()
    grads = []
    for fn in (lambda p: epit_layers_fp64(x, p, A, s)[0], lambda p: P.epit_forward.__wrapped__(torch.as_tensor(x).double(), p, A, s)):
        p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
        torch.nn.functional.l1_loss(fn(p), label).backward()
        grads.append({k: v.grad for k, v in p.items()})
    assert len(grads[0]) == 71
    for k in sd:
        assert torch.equal(grads[0][k], grads[1][k]), k


def test_forced_masks_of_its_own_decisions_change_nothing():
    """with the graph's own decisions handed back as `forced`, the output is the same and no decision counts as differing; through a B = 1
    slice of them too (what the GPU tests do at the published geometry)"""
    geom = EPIT_MATRIX[1]
    A, s, B, h, w = geom
    sd, x = epit_case(*geom)
    with torch.no_grad():
        y, layers, _ = epit_layers_fp64(x, sd, A, s)
        forced = {k: v > 0 for k, v in layers.items() if k[0] in EPIT_DECISION_KINDS}
        assert len(forced) == 34
        assert sum(m.numel() for m in forced.values()) == B * A * A * h * w * (4032 + 64 * s * s)      # the row's decisions
        y2, _, flips = epit_layers_fp64(x, sd, A, s, forced=forced)
        assert flips == 0 and torch.equal(y, y2)
        for i in range(B):
            one = {}
            for k, m in forced.items():
                rows = epit_ref_to_rows(m, epit_layout(*k), B, A, h, w)
                n = rows.shape[0] // B
                one[k] = epit_rows_to_ref(rows[i * n:(i + 1) * n].reshape(-1), epit_layout(*k), 1, A, h, w, s)
            y1, _, flips = epit_layers_fp64(x[i:i + 1], sd, A, s, forced=one)
            assert flips == 0 and float((y1 - y[i:i + 1]).abs().max()) <= BOUND
        # one flipped decision is counted
        for k in ((4, 3), (6, 0), (1, 1), (5, 0), (2, 9), (3, 0)):
            f2 = dict(forced)
            f2[k] = forced[k].clone(memory_format=torch.contiguous_format)
            f2[k].view(-1)[3] = ~f2[k].view(-1)[3]
            _, _, flips = epit_layers_fp64(x, sd, A, s, forced=f2)
            assert flips >= 1, k
