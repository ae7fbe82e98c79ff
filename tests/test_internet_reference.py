"""CPU: the LF_InterNet reference graph of tests/helpers.py (internet_layers_fp64, the one the GPU tests compare every saved layer and every
gradient with) against the numpy oracle, which tests/test_oracle_vs_golden.py pins on the reference's golden outputs -- on the whole geometry
matrix of tests/test_gpu_internet_geometries.py.  Both are fp64 restatements of the same graph on different conv implementations, so they
agree to rounding (a few 1e-15 at activations of order 10)."""
import numpy as np
import pytest
import torch

from oracle import lfsr_oracle as O
from tests.helpers import (INTERNET_MATRIX, INTERNET_SAVED, internet_case, internet_keys, internet_layers_fp64, internet_ref_to_rows,
                           internet_rows_to_ref, internet_spec, models_meta)


def test_internet_spec_equals_the_golden_specs():
    cases = models_meta()["models"]["LF_InterNet"]
    seen = 0
    for case in list(cases["cases"].values()) + [cases["full"]]:
        assert internet_spec(case["A"], case["s"]) == [(k, tuple(sh)) for k, sh in case["spec"]]
        seen += 1
    assert seen >= 3


def test_internet_spec_equals_the_plugin_state_dict():
    """at every (angRes, scale) of the matrix: the keys, their order and the shapes of model/SR/LF_InterNet.py's module tree"""
    from argparse import Namespace
    from lfsr_amd.model.SR import LF_InterNet as M
    for A, s in sorted({g[:2] for g in INTERNET_MATRIX}):
        net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
        assert internet_spec(A, s) == [(k, tuple(v.shape)) for k, v in net.state_dict().items()], (A, s)


@pytest.mark.parametrize("geom", INTERNET_MATRIX, ids=lambda g: "A%ds%dB%dh%dw%d" % g)
def test_layers_graph_equals_oracle(geom):
    A, s, B, h, w = geom
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    sd, x = internet_case(*geom)
    y, layers, flips = internet_layers_fp64(x, sd, A, s)
    ref = O.internet_forward(x, sd, A, s)
    y = y.numpy()
    assert y.dtype == np.float64 and y.shape == ref.shape == (B, 1, A * h * s, A * w * s)
    assert np.isfinite(y).all() and np.isfinite(ref).all()
    err = float(np.abs(y - ref).max())
    print(f"{geom}: max|layers graph - oracle| = {err:.2e}, max|ref| = {np.abs(ref).max():.3f}")
    assert err <= 1e-12
    assert flips == 0 and sorted(layers) == sorted(internet_keys())
    for (kind, i), t in layers.items():
        lay = INTERNET_SAVED[kind][2]
        assert tuple(t.shape) == ((B, 64, h, w) if lay == "lr" else (B, 64, h * A, w * A)), (kind, i)
    # the layout maps are each other's inverse, and the VCL one puts view (u, v), pixel (y, x) of sample b at row (((b A + u) A + v) h + y) w + x
    t = layers["spa2", 3]
    rows = internet_ref_to_rows(t, "vcl", A)
    assert torch.equal(internet_rows_to_ref(rows, "vcl", B, A, h, w), t)
    b, u, v, yy, xx = B - 1, A - 1, 0, h - 1, w // 2
    assert torch.equal(rows[(((b * A + u) * A + v) * h + yy) * w + xx], t[b, :, yy * A + u, xx * A + v])
    t = layers["ang2", 5]
    rows = internet_ref_to_rows(t, "lr", A)
    assert torch.equal(internet_rows_to_ref(rows, "lr", B, A, h, w), t)
    assert torch.equal(rows[((B - 1) * h + 1) * w + 2], t[B - 1, :, 1, 2])


def test_forced_masks_of_its_own_decisions_change_nothing():
    """with the graph's own ReLU decisions handed back as `forced`, the output is the same and no decision counts as differing"""
    geom = INTERNET_MATRIX[1]
    A, s = geom[:2]
    sd, x = internet_case(*geom)
    y, layers, _ = internet_layers_fp64(x, sd, A, s)
    forced = {k: v > 0 for k, v in layers.items() if k[0] in ("ang2", "relu_spa", "relu_ang", "relu_spabottle", "relu_angbottle")}
    y2, _, flips = internet_layers_fp64(x, sd, A, s, forced=forced)
    assert flips == 0 and torch.equal(y, y2)
    # one flipped decision is counted and moves the output
    k = ("relu_spa", 7)
    forced[k] = forced[k].clone()
    forced[k][0, 0, 0, 0] = ~forced[k][0, 0, 0, 0]
    _, _, flips = internet_layers_fp64(x, sd, A, s, forced=forced)
    assert flips >= 1
