"""CPU: the library's sixth arithmetic selection, lfsr_set_wide_arithmetic (include/lfsr_hip.h; csrc/options.cpp): LFSR_WIDE_ARITH_BF16 is accepted and read back,
any other value is refused without changing the mode, and the switch moves none of the other five nor they it.  And the stock-torch form of the LF_InterNet graph
that the GPU tests of the mode emulate it with (tests/internet_stock_graph.py) is the graph of oracle/lfsr_torch_port.py::internet_forward: equal in fp64 to
1e-12; its hook rounds the operands of the two wide convs and nothing else."""
import os
import re

import pytest
import torch

from lfsr_amd import capi
from oracle.lfsr_torch_port import internet_forward
from tests.helpers import model_case
from tests.internet_stock_graph import internet_stock, r_bf16, wide_conv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFSR_E_ARG = -1
BOUND = 1e-12     # two fp64 restatements of one graph (tests/test_ang_arith_cpu.py holds the same gate)
TAGS = ("a5h8s2", "a3h6w8s4")


def _restore(lib):
    lib.lfsr_set_arithmetic(0)
    lib.lfsr_set_grad_arithmetic(0)
    lib.lfsr_set_gemm_arithmetic(0)
    lib.lfsr_set_branch_arithmetic(0)
    lib.lfsr_set_ang_arithmetic(0)
    lib.lfsr_set_wide_arithmetic(0)


def test_set_get_wide_arithmetic():
    lib = capi.load()
    assert lib.lfsr_get_wide_arithmetic() == 0
    try:
        assert lib.lfsr_set_wide_arithmetic(1) == 0
        assert lib.lfsr_get_wide_arithmetic() == 1
        assert capi.get_wide_arithmetic() == capi.WIDE_ARITH_BF16
        capi.set_wide_arithmetic(capi.WIDE_ARITH_DEFAULT)
        assert lib.lfsr_get_wide_arithmetic() == 0
        capi.set_wide_arithmetic(capi.WIDE_ARITH_BF16)
        assert lib.lfsr_get_wide_arithmetic() == 1
    finally:
        _restore(lib)
    assert lib.lfsr_get_wide_arithmetic() == 0


def test_unknown_wide_arithmetic_is_refused_and_changes_nothing():
    lib = capi.load()
    try:
        for mode in (0, 1):
            assert lib.lfsr_set_wide_arithmetic(mode) == 0
            assert lib.lfsr_set_wide_arithmetic(2) == LFSR_E_ARG and lib.lfsr_set_wide_arithmetic(-1) == LFSR_E_ARG
            assert lib.lfsr_get_wide_arithmetic() == mode
    finally:
        _restore(lib)
    try:
        with pytest.raises(capi.LfsrError):
            capi.set_wide_arithmetic(2)
        assert lib.lfsr_get_wide_arithmetic() == 0
    finally:
        _restore(lib)


def test_the_six_switches_are_independent():
    lib = capi.load()
    try:
        for arith in (0, 1, 2):
            for grad in (0, 1):
                for gemm in (0, 1):
                    for branch in (0, 1):
                        for ang in (0, 1):
                            for wide in (0, 1):
                                assert (lib.lfsr_set_arithmetic(arith) == 0 and lib.lfsr_set_grad_arithmetic(grad) == 0 and lib.lfsr_set_gemm_arithmetic(gemm) == 0
                                        and lib.lfsr_set_branch_arithmetic(branch) == 0 and lib.lfsr_set_ang_arithmetic(ang) == 0
                                        and lib.lfsr_set_wide_arithmetic(wide) == 0)
                                others = lambda: (lib.lfsr_get_arithmetic(), lib.lfsr_get_grad_arithmetic(), lib.lfsr_get_gemm_arithmetic(),
                                                  lib.lfsr_get_branch_arithmetic(), lib.lfsr_get_ang_arithmetic())
                                assert others() == (arith, grad, gemm, branch, ang) and lib.lfsr_get_wide_arithmetic() == wide
                                assert lib.lfsr_set_wide_arithmetic(1 - wide) == 0              # moving this one ...
                                assert others() == (arith, grad, gemm, branch, ang)             # ... leaves the other five
                                assert lib.lfsr_set_wide_arithmetic(wide) == 0
                                assert (lib.lfsr_set_arithmetic((arith + 1) % 3) == 0 and lib.lfsr_set_grad_arithmetic(1 - grad) == 0
                                        and lib.lfsr_set_gemm_arithmetic(1 - gemm) == 0 and lib.lfsr_set_branch_arithmetic(1 - branch) == 0
                                        and lib.lfsr_set_ang_arithmetic(1 - ang) == 0)          # moving the other five ...
                                assert lib.lfsr_get_wide_arithmetic() == wide                   # ... leaves this one
    finally:
        _restore(lib)


def test_python_constants_match_the_header():
    src = open(os.path.join(ROOT, "include", "lfsr_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (LFSR_WIDE_ARITH_\w+)\s+(\d+)", src, re.M)}
    assert defs == {"LFSR_WIDE_ARITH_DEFAULT": capi.WIDE_ARITH_DEFAULT, "LFSR_WIDE_ARITH_BF16": capi.WIDE_ARITH_BF16} == {"LFSR_WIDE_ARITH_DEFAULT": 0, "LFSR_WIDE_ARITH_BF16": 1}
    for name in ("lfsr_set_wide_arithmetic", "lfsr_get_wide_arithmetic", "lfsr_conv3x3_wide_fwd"):
        assert name in capi.SIGNATURES


def test_operator_refuses_bad_arguments_without_a_device():
    """the argument checks come before anything touches the device: the cases that need no valid pointer"""
    lib = capi.load()
    assert lib.lfsr_conv3x3_wide_fwd(None, 128, 0, 128, None, None, 64, 0, None, 0, 0, 1, 4, 4, 0.0, None) == LFSR_E_ARG
    assert lib.lfsr_conv3x3_wide_fwd(None, 64, 0, 64, None, None, 64, 0, None, 0, 0, 1, 4, 4, 0.0, None) == LFSR_E_ARG


@pytest.mark.parametrize("tag", TAGS)
def test_stock_graph_equals_the_port_fp64(tag):
    case, sd, x, _ = model_case("LF_InterNet", tag)
    A, s = case["A"], case["s"]
    want = internet_forward(torch.from_numpy(x).double(), {k: torch.from_numpy(v).double() for k, v in sd.items()}, A, s)
    got = internet_stock(x, sd, A, s)
    assert got.dtype == torch.float64 and got.shape == want.shape == (case["B"], 1, A * case["h"] * s, A * case["w"] * s)
    err = float((got - want).abs().max())
    print(f"{tag}: max|stock graph - port| = {err:.2e}, max|out| = {float(want.abs().max()):.3f}")
    assert err <= BOUND, err


@pytest.mark.parametrize("tag", TAGS)
def test_stock_graph_hook_moves_the_output_by_a_bf16_rounding(tag):
    """with the hook the graph differs from the unhooked one by the order of magnitude of a bf16 operand rounding: rms between 1e-5 and 5e-3"""
    case, sd, x, _ = model_case("LF_InterNet", tag)
    y = internet_stock(x, sd, case["A"], case["s"])
    yr = internet_stock(x, sd, case["A"], case["s"], r_wide=r_bf16)
    rms = float((yr - y).pow(2).mean().sqrt())
    print(f"{tag}: rms of the wide hook vs fp64 {rms:.2e}")
    assert 1e-5 < rms < 5e-3


def test_hook_rounds_the_two_wide_convs_and_nothing_else():
    """a hook that counts: 16 SpaConvSq + 1 SpaBottle, each called with (activations, weight) of 128 / 320 input channels; and wide_conv with the hook is the
    conv of operands rounded beforehand"""
    case, sd, x, _ = model_case("LF_InterNet", "a3h6w8s4")
    seen = []

    def spy(t):
        seen.append(tuple(t.shape))
        return t

    y = internet_stock(x, sd, case["A"], case["s"], r_wide=spy)
    assert torch.equal(y, internet_stock(x, sd, case["A"], case["s"]))
    acts, wts = seen[0::2], seen[1::2]
    assert [w_ for w_ in wts] == [(64, 128, 3, 3)] * 16 + [(64, 320, 3, 3)]
    assert [a[1] for a in acts] == [128] * 16 + [320]
    g = torch.Generator().manual_seed(3)
    t = torch.rand((2, 128, 9, 12), generator=g, dtype=torch.float64)
    w = (torch.rand((64, 128, 3, 3), generator=g, dtype=torch.float64) - 0.5) / 12.0
    hooked = wide_conv(t, w, 3, r_bf16)
    assert torch.equal(hooked, wide_conv(r_bf16(t), r_bf16(w), 3))
    assert float((hooked - wide_conv(t, w, 3)).abs().max()) > 1e-5
