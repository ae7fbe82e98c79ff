"""CPU: the LFSSR plugin (model/SR/LFSSR.py) imports without a GPU, its state_dict is the recorded contract of the reference at both scales, and it
has no CPU path."""
from argparse import Namespace

import pytest
import torch

from lfsr_amd import capi
from tests import lfssr_helpers as H


def plugin():
    from lfsr_amd.model.SR import LFSSR as M
    return M


@pytest.mark.parametrize("tag", ["a3h6w8s2", "a5h8s4", "a2h5w7s4", "full"])
def test_keys_and_shapes_equal_the_fixture(tag):
    case = H.lfssr_meta()["cases"][tag]
    net = plugin().get_model(Namespace(angRes_in=case["A"], angRes_out=case["A"], scale_factor=case["s"]))
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    assert got == [(k, tuple(sh)) for k, sh in case["spec"]] == H.lfssr_spec(case["s"])
    assert len(got) == (48 if case["s"] == 2 else 94)
    assert [k for k, _ in net.named_parameters()] == [k for k, _ in got]      # no buffers: every entry is a parameter


def test_plugin_surface():
    M = plugin()
    assert M.weights_init(None) is None
    loss = M.get_loss(None)
    a, b = torch.zeros(1, 1, 4, 4), torch.ones(1, 1, 4, 4)
    assert float(loss(a, b)) == 1.0 and float(loss(a, b, [5, 5])) == 1.0      # L1
    with pytest.raises(capi.LfsrError):
        M.get_model(Namespace(angRes_in=5, angRes_out=5, scale_factor=3))     # the reference has net2x and net4x only
    assert M.get_model.trainable is False


def test_cpu_input_raises():
    net = plugin().get_model(Namespace(angRes_in=3, angRes_out=3, scale_factor=2))
    with pytest.raises(capi.LfsrError):
        net(torch.zeros(1, 1, 12, 12), None)
    with torch.no_grad(), pytest.raises(capi.LfsrError):
        net(torch.zeros(1, 1, 12, 12), None)


def test_abi_has_the_inference_life_cycle_only():
    names = [k for k in capi.SIGNATURES if k.startswith("lfsr_lfssr_")]
    assert sorted(names) == sorted(f"lfsr_lfssr_{f}" for f in ("create", "destroy", "packed_bytes", "set_packed", "load_param", "finalize", "workspace_bytes",
                                                             "forward", "conv0_fwd", "tail_fwd"))
    import ctypes as C
    lib = capi.load()
    ctx = C.c_void_p()
    for A, s, n, rc in ((5, 4, 10, 0), (2, 2, 1, 0), (9, 4, 3, 0), (1, 2, 10, -1), (10, 2, 10, -1), (5, 3, 10, -1), (5, 8, 10, -1), (5, 4, 0, -1)):
        assert lib.lfsr_lfssr_create(C.byref(ctx), A, s, n) == rc, (A, s, n)
        if rc == 0:
            assert lib.lfsr_lfssr_packed_bytes(ctx) > 0 and lib.lfsr_lfssr_workspace_bytes(ctx, 1, 3, 5) > 0
            assert lib.lfsr_lfssr_workspace_bytes(ctx, 0, 3, 5) == 0
            assert lib.lfsr_lfssr_load_param(ctx, b"net.conv0.weight", None, 576, None) == -1      # nothing set_packed yet
            assert lib.lfsr_lfssr_finalize(ctx, None) == -1
            lib.lfsr_lfssr_destroy(ctx)
