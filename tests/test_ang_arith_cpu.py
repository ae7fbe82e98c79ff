"""CPU: the library's fifth arithmetic selection, lfsr_set_ang_arithmetic (include/lfsr_hip.h; csrc/options.cpp): LFSR_ANG_ARITH_BF16 is accepted and read back,
any other value is refused without changing the mode, and the switch moves none of the other four nor they it.  And the stock-torch form of the LFSSR graph that
the GPU tests of the mode emulate it with (tests/lfssr_stock_graph.py) is the graph of tests/lfssr_helpers.py::lfssr_layers: equal in fp64 to 1e-12; its hooks
round what they name and nothing else."""
import os
import re

import pytest
import torch

from lfsr_amd import capi
from tests import lfssr_helpers as H
from tests.lfssr_stock_graph import ang_conv2d, lfssr_stock, r_bf16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFSR_E_ARG = -1
BOUND = 1e-12     # two fp64 restatements of one graph (tests/test_lfssr_reference.py holds the same gate)


def _restore(lib):
    lib.lfsr_set_arithmetic(0)
    lib.lfsr_set_grad_arithmetic(0)
    lib.lfsr_set_gemm_arithmetic(0)
    lib.lfsr_set_branch_arithmetic(0)
    lib.lfsr_set_ang_arithmetic(0)


def test_set_get_ang_arithmetic():
    lib = capi.load()
    assert lib.lfsr_get_ang_arithmetic() == 0
    try:
        assert lib.lfsr_set_ang_arithmetic(1) == 0
        assert lib.lfsr_get_ang_arithmetic() == 1
        assert capi.get_ang_arithmetic() == capi.ANG_ARITH_BF16
        capi.set_ang_arithmetic(capi.ANG_ARITH_DEFAULT)
        assert lib.lfsr_get_ang_arithmetic() == 0
        capi.set_ang_arithmetic(capi.ANG_ARITH_BF16)
        assert lib.lfsr_get_ang_arithmetic() == 1
    finally:
        _restore(lib)
    assert lib.lfsr_get_ang_arithmetic() == 0


def test_unknown_ang_arithmetic_is_refused_and_changes_nothing():
    lib = capi.load()
    try:
        for mode in (0, 1):
            assert lib.lfsr_set_ang_arithmetic(mode) == 0
            assert lib.lfsr_set_ang_arithmetic(2) == LFSR_E_ARG and lib.lfsr_set_ang_arithmetic(-1) == LFSR_E_ARG
            assert lib.lfsr_get_ang_arithmetic() == mode
    finally:
        _restore(lib)
    try:
        with pytest.raises(capi.LfsrError):
            capi.set_ang_arithmetic(2)
        assert lib.lfsr_get_ang_arithmetic() == 0
    finally:
        _restore(lib)


def test_the_five_switches_are_independent():
    lib = capi.load()
    try:
        for arith in (0, 1, 2):
            for grad in (0, 1):
                for gemm in (0, 1):
                    for branch in (0, 1):
                        for ang in (0, 1):
                            assert (lib.lfsr_set_arithmetic(arith) == 0 and lib.lfsr_set_grad_arithmetic(grad) == 0 and lib.lfsr_set_gemm_arithmetic(gemm) == 0
                                    and lib.lfsr_set_branch_arithmetic(branch) == 0 and lib.lfsr_set_ang_arithmetic(ang) == 0)
                            others = lambda: (lib.lfsr_get_arithmetic(), lib.lfsr_get_grad_arithmetic(), lib.lfsr_get_gemm_arithmetic(),
                                              lib.lfsr_get_branch_arithmetic())
                            assert others() == (arith, grad, gemm, branch) and lib.lfsr_get_ang_arithmetic() == ang
                            assert lib.lfsr_set_ang_arithmetic(1 - ang) == 0                # moving this one ...
                            assert others() == (arith, grad, gemm, branch)                  # ... leaves the other four
                            assert lib.lfsr_set_ang_arithmetic(ang) == 0
                            assert (lib.lfsr_set_arithmetic((arith + 1) % 3) == 0 and lib.lfsr_set_grad_arithmetic(1 - grad) == 0
                                    and lib.lfsr_set_gemm_arithmetic(1 - gemm) == 0 and lib.lfsr_set_branch_arithmetic(1 - branch) == 0)   # moving the other four ...
                            assert lib.lfsr_get_ang_arithmetic() == ang                     # ... leaves this one
    finally:
        _restore(lib)


def test_python_constants_match_the_header():
    src = open(os.path.join(ROOT, "include", "lfsr_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (LFSR_ANG_ARITH_\w+)\s+(\d+)", src, re.M)}
    assert defs == {"LFSR_ANG_ARITH_DEFAULT": capi.ANG_ARITH_DEFAULT, "LFSR_ANG_ARITH_BF16": capi.ANG_ARITH_BF16} == {"LFSR_ANG_ARITH_DEFAULT": 0, "LFSR_ANG_ARITH_BF16": 1}
    assert "lfsr_set_ang_arithmetic" in capi.SIGNATURES and "lfsr_get_ang_arithmetic" in capi.SIGNATURES


@pytest.mark.parametrize("tag", list(H.CASES))
def test_stock_graph_equals_the_layers_graph_fp64(tag):
    (A, h, w, s, B), sd, x = H.lfssr_case(tag)
    want = H.lfssr_layers(x, sd, A, s)["out"]
    got = lfssr_stock(x, sd, A, s)
    assert got.dtype == torch.float64 and got.shape == want.shape == (B, 1, A * h * s, A * w * s)
    err = float((got - want).abs().max())
    print(f"{tag}: max|stock graph - layers graph| = {err:.2e}, max|out| = {float(want.abs().max()):.3f}")
    assert err <= BOUND, err


def test_stock_angular_conv_is_the_formula_and_its_hook_rounds_both_operands():
    """one angular conv at a grid with an interior view, against lfssr_helpers.angconv (nine shifted products); with the hook it equals the formula on operands
    rounded beforehand, and differs from the unrounded one"""
    B, A, Hh, Ww = 2, 3, 2, 3
    g = torch.Generator().manual_seed(3)
    a = torch.rand((B * A * A, 64, Hh, Ww), generator=g, dtype=torch.float64)
    wt = (torch.rand((64, 64, 3, 3), generator=g, dtype=torch.float64) - 0.5) / 12.0
    b = torch.rand((64,), generator=g, dtype=torch.float64) - 0.5
    plain = ang_conv2d(a, wt, b, B, A)
    assert float((plain - torch.relu(H.angconv(a, wt, b, B, A))).abs().max()) <= BOUND
    hooked = ang_conv2d(a, wt, b, B, A, r_bf16)
    assert float((hooked - torch.relu(H.angconv(r_bf16(a), r_bf16(wt), b, B, A))).abs().max()) <= BOUND
    assert float((hooked - plain).abs().max()) > 1e-5


def test_stock_graph_hooks_are_separate():
    """each hook moves the output, by the order of magnitude the issue records for a bf16 operand rounding (1e-4 .. 1e-3 rms), and the two together differ from each"""
    (A, h, w, s, B), sd, x = H.lfssr_case("a2h5w7s4")
    y = lfssr_stock(x, sd, A, s)
    rms = lambda t: float((t - y).pow(2).mean().sqrt())
    ya, yc, yb = (lfssr_stock(x, sd, A, s, r_ang=ra, r_conv=rc) for ra, rc in ((r_bf16, None), (None, r_bf16), (r_bf16, r_bf16)))
    print(f"a2h5w7s4 rms vs fp64: ang hook {rms(ya):.2e}, conv hook {rms(yc):.2e}, both {rms(yb):.2e}")
    for t in (ya, yc, yb):
        assert 1e-5 < rms(t) < 5e-3
    assert not torch.equal(ya, yc) and not torch.equal(ya, yb) and not torch.equal(yc, yb)
