"""CPU, needs the reference tree: the LFSSR graph of tests/lfssr_helpers.py (lfssr_layers, what the GPU tests compare the HIP path with) against the
reference's model/SR/LFSSR.py, both in fp64, on every named intermediate; the state_dict contract; and the committed fixtures against a fresh run of
their generator.  Where the reference is absent (it does not travel with the repository) there is nothing to compare with and the module is skipped."""
import os

import numpy as np
import pytest
import torch

from tests import lfssr_helpers as H
from tests.golden import make_golden_lfssr as G

pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(G.REF, "model", "SR")), reason="the reference tree is not on this machine")

BOUND = 1e-12     # two fp64 restatements of one graph (tests/test_internet_reference.py holds the same gate); the issue measured 2.5e-15 on one AltFilter


@pytest.mark.parametrize("scale", [2, 4])
def test_spec_equals_the_reference_state_dict(scale):
    from argparse import Namespace
    for A in (2, 5, 9):
        net = G.ref_module().get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=scale))
        assert H.lfssr_spec(scale) == [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert len(H.lfssr_spec(scale)) == (48 if scale == 2 else 94)


@pytest.mark.parametrize("tag", list(H.CASES))
def test_layers_graph_equals_reference_fp64(tag):
    (A, h, w, s, B), sd, x = H.lfssr_case(tag)
    net, _ = G.load_ref(A, s, torch.float64)
    ref = G.ref_layers(net, torch.from_numpy(x).double(), A, s)
    got = H.lfssr_layers(x, sd, A, s)
    assert sorted(got) == sorted(ref) == sorted(n for n in H.LAYER_NAMES if s == 4 or not n.endswith("2"))
    for name in got:
        assert got[name].dtype == torch.float64 and got[name].shape == ref[name].shape, name
        err = float((got[name] - ref[name]).abs().max())
        print(f"{tag} {name}: max|layers - reference| = {err:.2e}, max|ref| = {float(ref[name].abs().max()):.3f}")
        assert err <= BOUND, (name, err)
    assert tuple(got["out"].shape) == (B, 1, A * h * s, A * w * s)


def test_layout_maps():
    t = torch.arange(2 * 4 * 3 * 2 * 5, dtype=torch.float64).reshape(2 * 4, 3, 2, 5)      # B = 2, A = 2
    rows = H.views_to_rows(t)
    assert torch.equal(H.rows_to_views(rows, 8, 2, 5), t)
    b, u, v, y, x = 1, 1, 0, 1, 3
    assert torch.equal(rows[(((b * 2 + u) * 2 + v) * 2 + y) * 5 + x], t[(b * 2 + u) * 2 + v, :, y, x])
    m = torch.arange(2 * 6 * 10, dtype=torch.float64).reshape(2, 1, 6, 10)             # A = 2, views of 3 x 5
    views = H.mosaic_to_views(m, 2)
    assert torch.equal(H.views_to_mosaic(views, 2, 2), m)
    assert views[(b * 2 + u) * 2 + v, 0, y, x] == m[b, 0, u * 3 + y, v * 5 + x]


def test_fixtures_regenerate():
    """a fresh run of the generator gives the committed arrays: the same keys, shapes, strides and specs, and values within the fp32 reference's own
    reordering error (1e-5 of the array's range: the CPU convs sum in an order that depends on the thread count)"""
    arrs, meta = G.generate(None, write=False)
    gold, cm = H.lfssr_golden(), H.lfssr_meta()
    assert sorted(arrs) == sorted(gold.files)
    for k in arrs:
        assert arrs[k].shape == gold[k].shape and arrs[k].dtype == gold[k].dtype == np.float32, k
        assert np.abs(arrs[k] - gold[k]).max() <= 1e-5 * max(1.0, np.abs(gold[k]).max()), k
    assert sorted(meta["cases"]) == sorted(cm["cases"]) == sorted(list(H.CASES) + ["full"])
    for tag, c in meta["cases"].items():
        for f in ("A", "h", "w", "s", "B", "spec", "out_shape"):
            assert c[f] == cm["cases"][tag][f], (tag, f)
        assert c.get("strides") == cm["cases"][tag].get("strides")
        assert cm["cases"][tag]["altblock1_sensitivity"] > 1e-3
    assert cm["torch"] and cm["numpy"]
    assert os.path.getsize(os.path.join(H.GOLDEN, "model_LFSSR.npz")) < 2.5e6
