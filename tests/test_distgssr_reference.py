"""CPU: the DistgSSR reference graph of tests/helpers.py (distg_layers_fp64, the one the GPU tests compare every saved tensor and every
gradient with) against the numpy oracle, which tests/test_oracle_vs_golden.py pins on the reference's golden outputs, and against the torch
port -- on the whole geometry matrix of tests/test_gpu_distgssr_geometries.py.

The bound between two fp64 restatements is rounding: outputs are of order 1 and pass through ~70 convolutions of up to 576 terms, and the
oracle's convolutions are other code than torch's, so BOUND is 4e-14 (what tests/test_lft_reference.py holds; seen here: 3e-15 or less on eleven of the thirteen
rows, 7.7e-15 and 1.4e-14 on the two 13x16 scale-3 rows).
Against the port the graph is the same torch ops in the same order: the same bits, output and gradients, with and without forced decisions."""
import time

import numpy as np
import pytest
import torch

from lfsr_amd.synth import synth_input
from oracle import lfsr_oracle as O
from oracle import lfsr_torch_port as P
from tests.helpers import (DISTG_BLOCKS, DISTG_CH, DISTG_MATRIX, DISTG_SAVED, MASK_KINDS, distg_case, distg_keys, distg_layers_fp64,
                           distg_masks_to_ref, distg_ref_to_rows, distg_samples, distg_spec, mask_ref_shape, ref_mask_to_hip)

BOUND = 4e-14
ids = lambda g: "A%ds%dB%dh%dw%d" % g
torch.set_num_threads(min(torch.get_num_threads(), 16))


def leaves(sd, dt=torch.float64):
    return {k: torch.tensor(v, dtype=dt, requires_grad=True) for k, v in sd.items()}


def port_masks(rec):
    """the port's rec dictionary (keys block prefix + kind) -> the (kind, index) keys distg_layers_fp64's `forced` takes"""
    return {(k, i): rec[pre + k] for i, pre in enumerate(DISTG_BLOCKS) for k in MASK_KINDS}


def test_spec_is_the_plugins_state_dict():
    """distg_spec(A, s) at every (angRes, scale) of the matrix is the plugin's state_dict: keys, order and shapes"""
    from argparse import Namespace
    from lfsr_amd.model.SR import DistgSSR as M
    for A, s in sorted({g[:2] for g in DISTG_MATRIX}):
        net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
        spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        assert distg_spec(A, s) == spec, (A, s)
        assert len(spec) == 137


@pytest.mark.parametrize("geom", DISTG_MATRIX, ids=ids)
def test_layers_graph_equals_oracle_and_port(geom):
    """every row on the port, all samples, bit for bit; on the numpy oracle to round-off -- the rows that go one sample at a time on the GPU
    machine (B x 5x5 x 32x32) on sample 0 alone"""
    A, s, B, h, w = geom
    sd, x = distg_case(*geom)
    sdt = {k: torch.tensor(v, dtype=torch.float64) for k, v in sd.items()}
    with torch.no_grad():
        y, layers, flips = distg_layers_fp64(x, sd, A, s)
        port = P.distgssr_forward_graph(torch.as_tensor(x).double(), sdt, A, s)
    assert y.dtype == torch.float64 and tuple(y.shape) == (B, 1, A * h * s, A * w * s) and bool(torch.isfinite(y).all())
    assert torch.equal(y, port)
    nb = 1 if len(distg_samples(*geom)) > 1 else B
    t0 = time.time()
    ref = O.distgssr_forward(x[:nb], sd, A, s)
    dt = time.time() - t0
    assert np.isfinite(ref).all()
    e_or = float(np.abs(y[:nb].numpy() - ref).max())
    print(f"{geom}: max|layers graph - oracle| = {e_or:.2e} ({nb} of {B} samples, {dt:.1f} s), max|ref| = {np.abs(ref).max():.3f}")
    assert e_or <= BOUND
    assert flips == 0 and len(layers) == 10 * 16
    for (kind, i), t in layers.items():
        assert tuple(t.shape) == mask_ref_shape(kind, B, A, h, w) and t.dtype == torch.float64, (kind, i)
    # the rows of every `which`: view (u, v), pixel (yy, xx) of sample b is VCL row (((b A + u) A + v) h + yy) w + xx; AngConv.0 rows are
    # (b, yy, xx); EPIConv.0 rows (b A + u, yy, xx) in the horizontal pass and (b A + v, yy, xx) in the vertical one
    b, u, v, yy, xx, i = B - 1, A - 1, 0, h - 1, w // 2, 9
    Y, X = yy * A + u, xx * A + v                                 # MacPI coordinates
    vrow = (((b * A + u) * A + v) * h + yy) * w + xx
    named = {0: (vrow, layers["S1", i][b, :, Y, X]), 5: (vrow, layers["FZ", i][b, :, Y, X]), 6: (vrow, layers["OUT", i][b, :, Y, X]),
             2: ((b * h + yy) * w + xx, layers["A1", i][b, :, yy, xx]),
             3: (((b * A + u) * h + yy) * w + xx, layers["EH1", i][b, :, Y, xx]),
             4: (((b * A + v) * h + yy) * w + xx, layers["EV1", i][b, :, X, yy]),
             1: (vrow, torch.cat((layers["S2", i][b, :, Y, X], layers["A2", i][b, :, yy, xx].reshape(16, A, A)[:, u, v],
                                  layers["EH2", i][b, :, Y, xx].reshape(A, 32)[v], layers["EV2", i][b, :, X, yy].reshape(A, 32)[u])))}
    for which, (row, want) in named.items():
        rows = distg_ref_to_rows(layers, which, i, B, A, h, w)
        n_rows = {2: B * h * w, 3: B * A * h * w, 4: B * A * h * w}.get(which, B * A * A * h * w)
        assert tuple(rows.shape) == (n_rows, sum(DISTG_CH[k] for k in DISTG_SAVED[which])), which
        assert torch.equal(rows[row], want), which
    assert len(distg_keys()) == 7 * 16


@pytest.mark.parametrize("geom", DISTG_MATRIX, ids=ids)
def test_gradients_equal_the_ports_autograd_bit_for_bit(geom):
    """every row, all 137 gradients; the rows that go one sample at a time on the GPU machine (B x 5x5 x 32x32) on sample 0 alone"""
    A, s, B, h, w = geom
    sd, x = distg_case(*geom)
    label = torch.as_tensor(synth_input((B, 1, A * h * s, A * w * s), seed=2)).double()
    if len(distg_samples(*geom)) > 1:
        x, label = x[:1], label[:1]
    grads = []
    for fn in (lambda p: distg_layers_fp64(x, p, A, s)[0], lambda p: P.distgssr_forward_graph(torch.as_tensor(x).double(), p, A, s)):
        p = leaves(sd)
        torch.nn.functional.l1_loss(fn(p), label).backward()
        grads.append({k: v.grad for k, v in p.items()})
    assert len(grads[0]) == 137
    for k in sd:
        assert torch.equal(grads[0][k], grads[1][k]), k


@pytest.mark.parametrize("geom", (DISTG_MATRIX[4], DISTG_MATRIX[12]), ids=ids)
def test_forced_fp32_decisions_reproduce_the_ports_force(geom):
    """the decisions of an fp32 run of the port, forced into both fp64 graphs: the same output and the same gradients, bit for bit, and the
    decisions counted as differing are those in which the fp32 and the fp64 run of the port differ"""
    A, s, B, h, w = geom
    sd, x = distg_case(*geom)
    label = torch.as_tensor(synth_input((B, 1, A * h * s, A * w * s), seed=2)).double()
    rec32, rec64 = {}, {}
    with torch.no_grad():
        P.distgssr_forward_graph(torch.as_tensor(x), {k: torch.as_tensor(v) for k, v in sd.items()}, A, s, rec=rec32)
        P.distgssr_forward_graph(torch.as_tensor(x).double(), {k: torch.as_tensor(v).double() for k, v in sd.items()}, A, s, rec=rec64)
    assert len(rec32) == 9 * 16
    p1, p2 = leaves(sd), leaves(sd)
    y1, layers, flips = distg_layers_fp64(x, p1, A, s, forced=port_masks(rec32))
    y2 = P.distgssr_forward_graph(torch.as_tensor(x).double(), p2, A, s, force=rec32)
    assert torch.equal(y1, y2)
    # a decision of the forced graph is counted against ITS pre-activation, which follows the forced decisions upstream: at least the first
    # differing decision is seen, and none is counted when there is none
    differ = sum(int((rec32[k] != rec64[k]).sum()) for k in rec64)
    print(f"{geom}: decisions differing between the fp32 and the fp64 port: {differ}; counted by the forced graph: {flips}")
    assert (flips > 0) == (differ > 0)
    torch.nn.functional.l1_loss(y1, label).backward()
    torch.nn.functional.l1_loss(y2, label).backward()
    for k in sd:
        assert torch.equal(p1[k].grad, p2[k].grad), k


def test_forced_masks_of_its_own_decisions_change_nothing():
    """with the graph's own decisions handed back as `forced` the output is the same and no decision counts as differing; through the HIP
    layout maps and a B = 1 slice of them too (what the GPU tests do at the published geometry); one flipped decision is counted"""
    geom = DISTG_MATRIX[3]
    A, s, B, h, w = geom
    sd, x = distg_case(*geom)
    with torch.no_grad():
        y, layers, _ = distg_layers_fp64(x, sd, A, s)
        forced = {k: v > 0 for k, v in layers.items() if k[0] in MASK_KINDS}
        assert len(forced) == 9 * 16
        y2, _, flips = distg_layers_fp64(x, sd, A, s, forced=forced)
        assert flips == 0 and torch.equal(y, y2)
        flat = {(k, i): ref_mask_to_hip(m, k, B, A, h, w) for (k, i), m in forced.items()}
        back = distg_masks_to_ref(flat, B, A, h, w)
        assert all(torch.equal(back[k], forced[k]) for k in forced)
        for i in range(B):
            y1, _, flips = distg_layers_fp64(x[i:i + 1], sd, A, s, forced=distg_masks_to_ref(flat, B, A, h, w, sample=i))
            assert flips == 0 and float((y1 - y[i:i + 1]).abs().max()) <= BOUND
        for k in (("S2", 3), ("EV1", 15), ("A2", 0), ("FZ", 7)):
            f2 = dict(forced)
            f2[k] = forced[k].clone(memory_format=torch.contiguous_format)
            f2[k].view(-1)[3] = ~f2[k].view(-1)[3]
            _, _, flips = distg_layers_fp64(x, sd, A, s, forced=f2)
            assert flips >= 1, k
