"""CPU: the library's eighth arithmetic selection, lfsr_set_wide_train_arithmetic (include/lfsr_hip.h; csrc/options.cpp): its three values are accepted and read
back, any other value is refused without changing the mode, and the switch moves none of the other seven nor they it (at the three corners
tests/test_lin_grad_arith_cpu.py uses).  lfsr_conv3x3_wide_wgrad_workspace_floats answers without a device: positive and the same in the three modes for cin in
{128, 320}, 0 for a refused shape.  And the stock-torch emulation of the modes the GPU tests print their CPU forecast from (tests/wide_train_emulation.py): with
the identity in place of the rounding its gradients are those of the unpatched port, and with bf16 a wide conv's weight gradient is conv2d_weight of the rounded
operands.  Every test restores all eight switches."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lfsr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFSR_E_ARG = -1
SEVEN = ("arithmetic", "grad_arithmetic", "gemm_arithmetic", "branch_arithmetic", "ang_arithmetic", "wide_arithmetic", "lin_grad_arithmetic")
CORNERS = ((0, 0, 0, 0, 0, 0, 0), (2, 1, 1, 1, 1, 1, 1), (1, 0, 1, 0, 1, 0, 1))


def _set_seven(lib, vals):
    return all(getattr(lib, f"lfsr_set_{n}")(v) == 0 for n, v in zip(SEVEN, vals))


def _get_seven(lib):
    return tuple(getattr(lib, f"lfsr_get_{n}")() for n in SEVEN)


def _restore(lib):
    _set_seven(lib, (0,) * 7)
    lib.lfsr_set_wide_train_arithmetic(0)


def test_set_get_wide_train_arithmetic():
    lib = capi.load()
    assert lib.lfsr_get_wide_train_arithmetic() == 0
    try:
        for mode in (1, 2, 0, 2, 1):
            assert lib.lfsr_set_wide_train_arithmetic(mode) == 0
            assert lib.lfsr_get_wide_train_arithmetic() == mode and capi.get_wide_train_arithmetic() == mode
        for mode in (capi.WIDE_TRAIN_ARITH_BF16, capi.WIDE_TRAIN_ARITH_BF16_WGRAD, capi.WIDE_TRAIN_ARITH_DEFAULT):
            capi.set_wide_train_arithmetic(mode)
            assert lib.lfsr_get_wide_train_arithmetic() == mode
    finally:
        _restore(lib)
    assert lib.lfsr_get_wide_train_arithmetic() == 0


def test_unknown_wide_train_arithmetic_is_refused_and_changes_nothing():
    lib = capi.load()
    try:
        for mode in (0, 1, 2):
            assert lib.lfsr_set_wide_train_arithmetic(mode) == 0
            assert lib.lfsr_set_wide_train_arithmetic(3) == LFSR_E_ARG and lib.lfsr_set_wide_train_arithmetic(-1) == LFSR_E_ARG
            assert lib.lfsr_get_wide_train_arithmetic() == mode
    finally:
        _restore(lib)
    try:
        with pytest.raises(capi.LfsrError):
            capi.set_wide_train_arithmetic(3)
        assert lib.lfsr_get_wide_train_arithmetic() == 0
    finally:
        _restore(lib)


def test_the_eight_switches_are_independent():
    lib = capi.load()
    try:
        for corner in CORNERS:
            for wt in (0, 1, 2):
                assert _set_seven(lib, corner) and lib.lfsr_set_wide_train_arithmetic(wt) == 0
                assert _get_seven(lib) == corner and lib.lfsr_get_wide_train_arithmetic() == wt
                for other in ((wt + 1) % 3, (wt + 2) % 3):
                    assert lib.lfsr_set_wide_train_arithmetic(other) == 0             # moving this one ...
                    assert _get_seven(lib) == corner                                  # ... leaves the other seven
                assert lib.lfsr_set_wide_train_arithmetic(wt) == 0
                for i, name in enumerate(SEVEN):                                      # moving each of the other seven, and all of them ...
                    moved = (corner[i] + 1) % (3 if i == 0 else 2)
                    assert getattr(lib, f"lfsr_set_{name}")(moved) == 0
                    assert lib.lfsr_get_wide_train_arithmetic() == wt                 # ... leaves this one
                assert _get_seven(lib) == tuple((c + 1) % (3 if i == 0 else 2) for i, c in enumerate(corner))
    finally:
        _restore(lib)


def test_python_constants_and_symbols_match_the_header():
    src = open(os.path.join(ROOT, "include", "lfsr_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (LFSR_WIDE_TRAIN_ARITH_\w+)\s+(\d+)", src, re.M)}
    assert defs == {"LFSR_WIDE_TRAIN_ARITH_DEFAULT": capi.WIDE_TRAIN_ARITH_DEFAULT, "LFSR_WIDE_TRAIN_ARITH_BF16_WGRAD": capi.WIDE_TRAIN_ARITH_BF16_WGRAD,
                    "LFSR_WIDE_TRAIN_ARITH_BF16": capi.WIDE_TRAIN_ARITH_BF16}
    assert defs == {"LFSR_WIDE_TRAIN_ARITH_DEFAULT": 0, "LFSR_WIDE_TRAIN_ARITH_BF16_WGRAD": 1, "LFSR_WIDE_TRAIN_ARITH_BF16": 2}
    for name in ("lfsr_set_wide_train_arithmetic", "lfsr_get_wide_train_arithmetic", "lfsr_conv3x3_wide_wgrad_workspace_floats", "lfsr_conv3x3_wide_wgrad"):
        assert name in capi.SIGNATURES and re.search(r"\b%s\(" % name, src)
    assert callable(capi.conv3x3_wide_wgrad)


def test_wide_wgrad_workspace_floats():
    """positive for cin in {128, 320}, the same in the three modes, at least one slab; 0 for another cin or a non-positive size"""
    lib = capi.load()
    try:
        sizes = {}
        for mode in (0, 1, 2):
            assert lib.lfsr_set_wide_train_arithmetic(mode) == 0
            for cin in (128, 320):
                for geom in ((1, 5, 7), (18, 6, 8), (300, 8, 8), (200, 32, 32)):
                    n = lib.lfsr_conv3x3_wide_wgrad_workspace_floats(cin, *geom)
                    assert n > 0 and n >= 9 * 64 * cin
                    assert sizes.setdefault((cin, geom), n) == n
            for cin in (64, 192, 0, -128):
                assert lib.lfsr_conv3x3_wide_wgrad_workspace_floats(cin, 18, 6, 8) == 0
            for geom in ((0, 6, 8), (18, 0, 8), (18, 6, 0), (-1, 6, 8), (18, -6, 8), (18, 6, -8)):
                assert lib.lfsr_conv3x3_wide_wgrad_workspace_floats(128, *geom) == 0
    finally:
        _restore(lib)


def test_operator_refuses_null_pointers_without_a_device():
    """the argument checks come before anything touches the device: the cases that need no valid pointer"""
    lib = capi.load()
    try:
        for mode in (0, 1, 2):
            assert lib.lfsr_set_wide_train_arithmetic(mode) == 0
            assert lib.lfsr_conv3x3_wide_wgrad(None, 64, 0, None, 128, 0, 128, None, None, 1 << 30, 18, 6, 8, 0, None) == LFSR_E_ARG
    finally:
        _restore(lib)


def test_train_workspace_bytes_do_not_depend_on_the_switch():
    """no device needed: the layout alone"""
    from tests.helpers import model_case
    lib = capi.load()
    case, sd, _, _ = model_case("LF_InterNet", "a5h8s2")
    rt = capi.ModelRuntime("internet", case["A"], case["s"], 4, 4)
    try:
        sizes = []
        for mode in (0, 1, 2):
            assert lib.lfsr_set_wide_train_arithmetic(mode) == 0
            sizes.append([rt.train_workspace_bytes(B, 32, 32) for B in (1, 2, 8)])
        assert sizes[0] == sizes[1] == sizes[2]
        assert sizes[0][0] > 0 and sizes[0][0] < sizes[0][1] < sizes[0][2]
    finally:
        _restore(lib)


# ---- the CPU emulation of the modes (tests/wide_train_emulation.py) --------------------------------------------------------------------------
def test_emulation_with_the_identity_is_the_port():
    """the patched graph with nothing rounded has the gradients of the unpatched port (fp64: 1e-12 rel-L2 per tensor), and patches exactly the seventeen wide weights"""
    from oracle.lfsr_torch_port import internet_forward
    from lfsr_amd.synth import synth_input
    from tests import wide_train_emulation as E
    from tests.helpers import model_case
    case, sd, x, _ = model_case("LF_InterNet", "a3h6w8s4")
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    params = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
    F.l1_loss(internet_forward.__wrapped__(torch.from_numpy(x).double(), params, A, s), torch.from_numpy(label).double()).backward()
    plain = {k: p.grad.numpy() for k, p in params.items()}
    seen = []
    _, ident = E.step_grads(sd, x, label, A, s, r=lambda t: t, flags=(True, True, True), seen=seen)
    assert set(plain) == set(ident)
    for k in plain:
        d = float(np.linalg.norm(plain[k] - ident[k]) / max(np.linalg.norm(plain[k]), 1e-300))
        assert d <= 1e-12, (k, d)
    assert len(E.WIDE_KEYS) == 17 and sorted(seen) == sorted(E.WIDE_KEYS) and set(E.WIDE_KEYS) <= set(plain)


@pytest.mark.parametrize("cin", [128, 320])
def test_emulated_wide_conv_rounds_the_weight_gradients_operands(cin):
    from tests import wide_train_emulation as E
    A = 3
    g = torch.Generator().manual_seed(5 + cin)
    t = torch.randn(2, cin, 4 * A, 5 * A, generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(64, cin, 3, 3, generator=g, dtype=torch.float64) * 0.05).requires_grad_()
    dy = torch.randn(2, 64, 4 * A, 5 * A, generator=g, dtype=torch.float64)
    y = E.WideConv.apply(t, w, A, E.r_bf16, *E.MODES[1])
    assert torch.equal(y, F.conv2d(t, w, dilation=A, padding=A))                    # mode 1: the forward is untouched
    y.backward(dy)
    td, wd = t.detach(), w.detach()
    exact = torch.nn.grad.conv2d_weight(td, w.shape, dy, dilation=A, padding=A)
    assert torch.equal(w.grad, torch.nn.grad.conv2d_weight(E.r_bf16(td), w.shape, E.r_bf16(dy), dilation=A, padding=A))
    assert float((w.grad - exact).abs().max()) > 1e-5
    assert torch.equal(t.grad, torch.nn.grad.conv2d_input(t.shape, wd, dy, dilation=A, padding=A))      # the data gradient stays exact
    y2 = E.WideConv.apply(td, wd, A, E.r_bf16, *E.MODES[2])
    assert torch.equal(y2, F.conv2d(E.r_bf16(td), E.r_bf16(wd), dilation=A, padding=A)) and not torch.equal(y2, y)
