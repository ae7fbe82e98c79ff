"""CPU: the library's seventh arithmetic selection, lfsr_set_lin_grad_arithmetic (include/lfsr_hip.h; csrc/options.cpp): LFSR_LIN_GRAD_ARITH_BF16 is accepted and
read back, any other value is refused without changing the mode, and the switch moves none of the other six nor they it (this switch is moved while the six sit at
each of three settings, two of them opposite corners, and the reverse).  lfsr_linear_wgrad_workspace_floats answers without a device: positive for every supported (cout, cin), 0 for a
refused shape or row count.  And the stock-torch emulation of the mode the GPU tests print their CPU forecast from (tests/lin_grad_emulation.py): with the
identity in place of the rounding its gradients are those of the unpatched port."""
import os
import re

import pytest
import torch

from lfsr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFSR_E_ARG = -1
SIX = ("arithmetic", "grad_arithmetic", "gemm_arithmetic", "branch_arithmetic", "ang_arithmetic", "wide_arithmetic")
CORNERS = ((0, 0, 0, 0, 0, 0), (2, 1, 1, 1, 1, 1), (1, 0, 1, 0, 1, 0))


def _set_six(lib, vals):
    return all(getattr(lib, f"lfsr_set_{n}")(v) == 0 for n, v in zip(SIX, vals))


def _get_six(lib):
    return tuple(getattr(lib, f"lfsr_get_{n}")() for n in SIX)


def _restore(lib):
    _set_six(lib, (0,) * 6)
    lib.lfsr_set_lin_grad_arithmetic(0)


def test_set_get_lin_grad_arithmetic():
    lib = capi.load()
    assert lib.lfsr_get_lin_grad_arithmetic() == 0
    try:
        assert lib.lfsr_set_lin_grad_arithmetic(1) == 0
        assert lib.lfsr_get_lin_grad_arithmetic() == 1
        assert capi.get_lin_grad_arithmetic() == capi.LIN_GRAD_ARITH_BF16
        capi.set_lin_grad_arithmetic(capi.LIN_GRAD_ARITH_DEFAULT)
        assert lib.lfsr_get_lin_grad_arithmetic() == 0
        capi.set_lin_grad_arithmetic(capi.LIN_GRAD_ARITH_BF16)
        assert lib.lfsr_get_lin_grad_arithmetic() == 1
    finally:
        _restore(lib)
    assert lib.lfsr_get_lin_grad_arithmetic() == 0


def test_unknown_lin_grad_arithmetic_is_refused_and_changes_nothing():
    lib = capi.load()
    try:
        for mode in (0, 1):
            assert lib.lfsr_set_lin_grad_arithmetic(mode) == 0
            assert lib.lfsr_set_lin_grad_arithmetic(2) == LFSR_E_ARG and lib.lfsr_set_lin_grad_arithmetic(-1) == LFSR_E_ARG
            assert lib.lfsr_get_lin_grad_arithmetic() == mode
    finally:
        _restore(lib)
    try:
        with pytest.raises(capi.LfsrError):
            capi.set_lin_grad_arithmetic(2)
        assert lib.lfsr_get_lin_grad_arithmetic() == 0
    finally:
        _restore(lib)


def test_the_seven_switches_are_independent():
    lib = capi.load()
    try:
        for corner in CORNERS:
            for lin in (0, 1):
                assert _set_six(lib, corner) and lib.lfsr_set_lin_grad_arithmetic(lin) == 0
                assert _get_six(lib) == corner and lib.lfsr_get_lin_grad_arithmetic() == lin
                assert lib.lfsr_set_lin_grad_arithmetic(1 - lin) == 0                # moving this one ...
                assert _get_six(lib) == corner                                        # ... leaves the other six
                assert lib.lfsr_set_lin_grad_arithmetic(lin) == 0
                for i, name in enumerate(SIX):                                        # moving each of the other six, and all of them ...
                    moved = (corner[i] + 1) % (3 if i == 0 else 2)
                    assert getattr(lib, f"lfsr_set_{name}")(moved) == 0
                    assert lib.lfsr_get_lin_grad_arithmetic() == lin                  # ... leaves this one
                assert _get_six(lib) == tuple((c + 1) % (3 if i == 0 else 2) for i, c in enumerate(corner))
    finally:
        _restore(lib)


def test_python_constants_and_symbols_match_the_header():
    src = open(os.path.join(ROOT, "include", "lfsr_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (LFSR_LIN_GRAD_ARITH_\w+)\s+(\d+)", src, re.M)}
    assert defs == {"LFSR_LIN_GRAD_ARITH_DEFAULT": capi.LIN_GRAD_ARITH_DEFAULT, "LFSR_LIN_GRAD_ARITH_BF16": capi.LIN_GRAD_ARITH_BF16}
    assert defs == {"LFSR_LIN_GRAD_ARITH_DEFAULT": 0, "LFSR_LIN_GRAD_ARITH_BF16": 1}
    for name in ("lfsr_set_lin_grad_arithmetic", "lfsr_get_lin_grad_arithmetic", "lfsr_linear_wgrad_workspace_floats", "lfsr_linear_wgrad", "lfsr_linear_dgrad"):
        assert name in capi.SIGNATURES and re.search(r"\b%s\(" % name, src)
    assert callable(capi.linear_wgrad) and callable(capi.linear_dgrad)


def test_linear_wgrad_workspace_floats():
    """positive for every supported (cout, cin), the same in both modes, enough for the default's slabs of one 64-row slice; 0 for a refused shape or M"""
    lib = capi.load()
    try:
        for M in (5, 3000, 204800):
            sizes = {}
            for mode in (0, 1):
                assert lib.lfsr_set_lin_grad_arithmetic(mode) == 0
                for cout in (64, 128, 256, 576, 1024):
                    for cin in (64, 128, 256):
                        n = lib.lfsr_linear_wgrad_workspace_floats(M, cout, cin)
                        assert n > 0 and n >= lib.lfsr_pointwise_wgrad_workspace_floats(M, 64, cin) and n >= cout * cin
                        assert sizes.setdefault((cout, cin), n) == n
        for cout, cin in ((32, 64), (144, 64), (64, 96)):
            assert lib.lfsr_linear_wgrad_workspace_floats(3000, cout, cin) == 0
        assert lib.lfsr_linear_wgrad_workspace_floats(0, 64, 64) == 0 and lib.lfsr_linear_wgrad_workspace_floats(-3, 64, 64) == 0
        assert lib.lfsr_linear_wgrad_workspace_floats(2 ** 31 - 128, 64, 64) == 0 and lib.lfsr_linear_wgrad_workspace_floats(2 ** 31 - 129, 64, 64) > 0
    finally:
        _restore(lib)


def test_operator_refuses_bad_arguments_without_a_device():
    """the argument checks come before anything touches the device: the cases that need no valid pointer"""
    lib = capi.load()
    assert lib.lfsr_linear_wgrad(None, 64, None, 64, None, None, 1 << 30, 300, 64, 64, 0, None) == LFSR_E_ARG


# ---- the CPU emulation of the mode (tests/lin_grad_emulation.py) ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["EPIT", "LFT"])
def test_emulation_with_the_identity_is_the_port(name):
    """the patched graph with nothing rounded has the gradients of the unpatched port (fp64: 1e-12 rel-L2 per tensor), and patches every linear the mode computes"""
    from tests import lin_grad_emulation as E
    from tests.helpers import model_case
    tag = {"EPIT": "a3h6w8s3", "LFT": "a3h6w8s2"}[name]
    case, sd, x, _ = model_case(name, tag)
    plain = E.port_grads(name, case, sd, x, torch.float64)
    seen = []
    ident = E.port_grads(name, case, sd, x, torch.float64, rounding=lambda t: t, seen=seen)
    assert set(plain) == set(ident)
    for k in plain:
        d = float((plain[k] - ident[k]).norm() / plain[k].norm().clamp_min(1e-300))
        assert d <= 1e-12, (k, d)
    lin = [k for k in plain if E.is_mode_linear(k)]
    assert lin and set(seen) == set(lin), (sorted(set(lin) - set(seen)), sorted(set(seen) - set(lin)))


def test_emulated_linear_backward_rounds_all_three_operands():
    from tests import lin_grad_emulation as E
    g = torch.Generator().manual_seed(5)
    x = torch.randn(37, 64, generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(128, 64, generator=g, dtype=torch.float64) * 0.1).requires_grad_()
    dy = torch.randn(37, 128, generator=g, dtype=torch.float64)
    y = E.RoundedGradLinear.apply(x, w, E.r_bf16)
    assert torch.equal(y, x @ w.t())                       # the forward is untouched
    y.backward(dy)
    assert torch.equal(x.grad, E.r_bf16(dy) @ E.r_bf16(w.detach()))
    assert torch.equal(w.grad, E.r_bf16(dy).t() @ E.r_bf16(x.detach()))
    assert float((w.grad - dy.t() @ x.detach()).abs().max()) > 1e-5
