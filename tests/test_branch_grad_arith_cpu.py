"""CPU: the library's ninth arithmetic selection, lfsr_set_branch_grad_arithmetic (include/lfsr_hip.h; csrc/options.cpp): LFSR_BRANCH_GRAD_ARITH_BF16 is accepted
and read back, any other value is refused without changing the mode, and the switch moves none of the other eight nor they it (at the three corners
tests/test_wide_train_arith_cpu.py uses).  The two workspace queries of its callers answer the same in both modes.  The ISA of csrc/epi0_grad_bf16.hip (MFMAs
issued as asm statements, so the compiler pads no wait states for them) passes tools/check_asm_mfma_hazards.py.  And the stock-torch emulation of the mode
(tests/branch_grad_emulation.py): with the identity in place of the rounding its gradients are those of the port, with bf16 EPIConv.0's gradients are those of the
rounded operands, and on the whole-model geometries of the GPU test its error against fp64 autograd is inside torch.autocast(bfloat16)'s on every parameter.
Every test restores all nine switches."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lfsr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFSR_E_ARG = -1
EIGHT = ("arithmetic", "grad_arithmetic", "gemm_arithmetic", "branch_arithmetic", "ang_arithmetic", "wide_arithmetic", "lin_grad_arithmetic", "wide_train_arithmetic")
VALUES = (3, 2, 2, 2, 2, 2, 2, 3)          # how many values each of the eight takes
CORNERS = ((0, 0, 0, 0, 0, 0, 0, 0), (2, 1, 1, 1, 1, 1, 1, 2), (1, 0, 1, 0, 1, 0, 1, 1))


def _set_eight(lib, vals):
    return all(getattr(lib, f"lfsr_set_{n}")(v) == 0 for n, v in zip(EIGHT, vals))


def _get_eight(lib):
    return tuple(getattr(lib, f"lfsr_get_{n}")() for n in EIGHT)


def _restore(lib):
    _set_eight(lib, (0,) * 8)
    lib.lfsr_set_branch_grad_arithmetic(0)


def test_set_get_branch_grad_arithmetic():
    lib = capi.load()
    assert lib.lfsr_get_branch_grad_arithmetic() == 0
    try:
        for mode in (1, 0, 1, 1, 0):
            assert lib.lfsr_set_branch_grad_arithmetic(mode) == 0
            assert lib.lfsr_get_branch_grad_arithmetic() == mode and capi.get_branch_grad_arithmetic() == mode
        for mode in (capi.BRANCH_GRAD_ARITH_BF16, capi.BRANCH_GRAD_ARITH_DEFAULT):
            capi.set_branch_grad_arithmetic(mode)
            assert lib.lfsr_get_branch_grad_arithmetic() == mode
    finally:
        _restore(lib)
    assert lib.lfsr_get_branch_grad_arithmetic() == 0


def test_unknown_branch_grad_arithmetic_is_refused_and_changes_nothing():
    lib = capi.load()
    try:
        for mode in (0, 1):
            assert lib.lfsr_set_branch_grad_arithmetic(mode) == 0
            assert lib.lfsr_set_branch_grad_arithmetic(2) == LFSR_E_ARG and lib.lfsr_set_branch_grad_arithmetic(-1) == LFSR_E_ARG
            assert lib.lfsr_get_branch_grad_arithmetic() == mode
        with pytest.raises(capi.LfsrError):
            capi.set_branch_grad_arithmetic(2)
        assert lib.lfsr_get_branch_grad_arithmetic() == 1
    finally:
        _restore(lib)


def test_the_nine_switches_are_independent():
    lib = capi.load()
    try:
        for corner in CORNERS:
            for bg in (0, 1):
                assert _set_eight(lib, corner) and lib.lfsr_set_branch_grad_arithmetic(bg) == 0
                assert _get_eight(lib) == corner and lib.lfsr_get_branch_grad_arithmetic() == bg
                assert lib.lfsr_set_branch_grad_arithmetic(1 - bg) == 0               # moving this one ...
                assert _get_eight(lib) == corner                                      # ... leaves the other eight
                assert lib.lfsr_set_branch_grad_arithmetic(bg) == 0
                for i, name in enumerate(EIGHT):                                      # moving each of the other eight, and all of them ...
                    assert getattr(lib, f"lfsr_set_{name}")((corner[i] + 1) % VALUES[i]) == 0
                    assert lib.lfsr_get_branch_grad_arithmetic() == bg                # ... leaves this one
                assert _get_eight(lib) == tuple((c + 1) % VALUES[i] for i, c in enumerate(corner))
        # lfsr_set_arithmetic does not move it, F32 included
        assert lib.lfsr_set_branch_grad_arithmetic(1) == 0
        for mode in (capi.ARITH_F32, capi.ARITH_BF16, capi.ARITH_DEFAULT):
            capi.set_arithmetic(mode)
            assert lib.lfsr_get_branch_grad_arithmetic() == 1
    finally:
        _restore(lib)


def test_python_constants_and_symbols_match_the_header():
    src = open(os.path.join(ROOT, "include", "lfsr_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (LFSR_BRANCH_GRAD_ARITH_\w+)\s+(\d+)", src, re.M)}
    assert defs == {"LFSR_BRANCH_GRAD_ARITH_DEFAULT": capi.BRANCH_GRAD_ARITH_DEFAULT, "LFSR_BRANCH_GRAD_ARITH_BF16": capi.BRANCH_GRAD_ARITH_BF16}
    assert defs == {"LFSR_BRANCH_GRAD_ARITH_DEFAULT": 0, "LFSR_BRANCH_GRAD_ARITH_BF16": 1}
    for name in ("lfsr_set_branch_grad_arithmetic", "lfsr_get_branch_grad_arithmetic"):
        assert name in capi.SIGNATURES and re.search(r"\b%s\(" % name, src)


def test_workspace_queries_do_not_depend_on_the_switch():
    """no device needed: the layouts alone"""
    lib = capi.load()
    rt = capi.DistgSSRRuntime(5, 4)
    geoms = ((1, 5, 6, 9), (2, 5, 32, 32), (8, 5, 32, 32), (1, 5, 40, 24), (2, 3, 8, 8))
    try:
        sizes = []
        for mode in (0, 1):
            assert lib.lfsr_set_branch_grad_arithmetic(mode) == 0
            sizes.append([lib.lfsr_epiconv_hv_bwd_workspace_floats(*g) for g in geoms] + [rt.train_workspace_bytes(B, 32, 32) for B in (1, 2, 8)])
        assert sizes[0] == sizes[1] and all(v > 0 for v in sizes[0])
    finally:
        _restore(lib)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc to emit the ISA")
def test_no_unpadded_hazard_around_the_epi0_gradient_kernels_mfmas():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_asm_mfma_hazards.py"), "epi0_grad_bf16.hip"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    # the weight gradient: one K step x 25 taps per line; the data gradient: 5 taps x 5 lines per phase
    assert "epi0_grad_bf16.hip: 50 bf16 MFMAs checked" in r.stdout, r.stdout


# ---- the CPU emulation of the mode (tests/branch_grad_emulation.py) ---------------------------------------------------------------------------
def test_emulation_with_the_identity_is_the_port():
    """the patched graph with nothing rounded has the gradients of the port (fp64: 1e-12 rel-L2 per tensor) and patches exactly the sixteen EPIConv.0, twice each
    (the horizontal and the vertical pass); at angRes 3 it patches nothing"""
    from oracle.lfsr_torch_port import distgssr_forward_graph
    from lfsr_amd.synth import synth_input
    from tests import branch_grad_emulation as E
    from tests.helpers import distg_case
    for geom in E.GEOMS:
        A, s, B, h, w = geom
        sd, x = distg_case(A, s, B, h, w)
        label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
        params = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
        F.l1_loss(distgssr_forward_graph(torch.from_numpy(x).double(), params, A, s), torch.from_numpy(label).double()).backward()
        seen = []
        _, ident = E.step_grads(sd, x, label, A, s, r=lambda t: t, seen=seen)
        assert set(ident) == set(params)
        for k, p in params.items():
            assert E.rel_l2(ident[k], p.grad.numpy()) <= 1e-12, k
        assert sorted(seen) == (sorted(E.EPI0_KEYS * 2) if A == 5 else [])


def test_emulated_epi0_rounds_its_gradients_operands():
    from tests import branch_grad_emulation as E
    A = 5
    g = torch.Generator().manual_seed(11)
    t = torch.randn(2, 64, 4, 6 * A, generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(32, 64, 1, A * A, generator=g, dtype=torch.float64) * 0.05).requires_grad_()
    dE = torch.randn(2, 32, 4, 6, generator=g, dtype=torch.float64)
    kw = dict(stride=(1, A), padding=(0, A * (A - 1) // 2))
    y = E.Epi0Conv.apply(t, w, A, E.r_bf16)
    assert torch.equal(y, F.conv2d(t, w, **kw))                                      # the forward is untouched
    y.backward(dE)
    td, wd = t.detach(), w.detach()
    assert torch.equal(w.grad, torch.nn.grad.conv2d_weight(E.r_bf16(td), w.shape, E.r_bf16(dE), **kw))
    assert torch.equal(t.grad, torch.nn.grad.conv2d_input(t.shape, E.r_bf16(wd), E.r_bf16(dE), **kw))
    assert float((w.grad - torch.nn.grad.conv2d_weight(td, w.shape, dE, **kw)).abs().max()) > 1e-5
    assert float((t.grad - torch.nn.grad.conv2d_input(t.shape, wd, dE, **kw)).abs().max()) > 1e-5


def test_emulated_mode_is_inside_autocasts_error_on_every_parameter():
    """the whole-model gate of tests/test_gpu_branch_grad_bf16.py, made here without a GPU: per parameter, the emulated mode's rel-L2 error against fp64 autograd is
    not above the port's under torch.autocast("cpu", bfloat16).  Prints the smallest autocast / mode ratio (profiles/branch_grad_bf16_time.md quotes it)."""
    from tests import branch_grad_emulation as E
    smallest = None
    for geom in E.GEOMS:
        names, e, e_amp = E.report(*geom)
        ratio = {k: e_amp[k] / max(e[k], 1e-30) for k in names}
        kmin = min(ratio, key=ratio.get)
        print(f"distgssr {geom}: emulated mode per-parameter rel-L2 median {np.median(list(e.values())):.2e} max {max(e.values()):.2e}; autocast median "
              f"{np.median(list(e_amp.values())):.2e} min {min(e_amp.values()):.2e}; smallest autocast / mode ratio {ratio[kmin]:.2f} ({kmin})")
        bad = {k: (e[k], e_amp[k]) for k in names if not e[k] <= e_amp[k]}
        assert not bad, (geom, bad)
        smallest = ratio[kmin] if smallest is None else min(smallest, ratio[kmin])
    print(f"smallest autocast / mode ratio over both geometries: {smallest:.2f}")
    assert smallest >= 1.0
