"""CPU: the library's fourth arithmetic selection, lfsr_set_branch_arithmetic (include/lfsr_hip.h; csrc/options.cpp): LFSR_BRANCH_ARITH_BF16 is accepted and read
back, any other value is refused without changing the mode, and the switch moves none of lfsr_set_arithmetic / lfsr_set_grad_arithmetic / lfsr_set_gemm_arithmetic
nor they it.  And the ISA of its kernels (csrc/distg_bf16.hip: MFMAs issued as asm statements, so the compiler pads no wait states for them) passes
tools/check_asm_mfma_hazards.py."""
import os
import re
import subprocess
import sys

import pytest

from lfsr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFSR_E_ARG = -1


def _restore(lib):
    lib.lfsr_set_arithmetic(0)
    lib.lfsr_set_grad_arithmetic(0)
    lib.lfsr_set_gemm_arithmetic(0)
    lib.lfsr_set_branch_arithmetic(0)


def test_set_get_branch_arithmetic():
    lib = capi.load()
    assert lib.lfsr_get_branch_arithmetic() == 0
    try:
        assert lib.lfsr_set_branch_arithmetic(1) == 0
        assert lib.lfsr_get_branch_arithmetic() == 1
        assert capi.get_branch_arithmetic() == capi.BRANCH_ARITH_BF16
        capi.set_branch_arithmetic(capi.BRANCH_ARITH_DEFAULT)
        assert lib.lfsr_get_branch_arithmetic() == 0
        capi.set_branch_arithmetic(capi.BRANCH_ARITH_BF16)
        assert lib.lfsr_get_branch_arithmetic() == 1
    finally:
        _restore(lib)
    assert lib.lfsr_get_branch_arithmetic() == 0


def test_unknown_branch_arithmetic_is_refused_and_changes_nothing():
    lib = capi.load()
    try:
        for mode in (0, 1):
            assert lib.lfsr_set_branch_arithmetic(mode) == 0
            assert lib.lfsr_set_branch_arithmetic(2) == LFSR_E_ARG and lib.lfsr_set_branch_arithmetic(-1) == LFSR_E_ARG
            assert lib.lfsr_get_branch_arithmetic() == mode
    finally:
        _restore(lib)
    try:
        with pytest.raises(capi.LfsrError):
            capi.set_branch_arithmetic(2)
        assert lib.lfsr_get_branch_arithmetic() == 0
    finally:
        _restore(lib)


def test_the_four_switches_are_independent():
    lib = capi.load()
    try:
        for arith in (0, 1, 2):
            for grad in (0, 1):
                for gemm in (0, 1):
                    for branch in (0, 1):
                        assert (lib.lfsr_set_arithmetic(arith) == 0 and lib.lfsr_set_grad_arithmetic(grad) == 0 and lib.lfsr_set_gemm_arithmetic(gemm) == 0
                                and lib.lfsr_set_branch_arithmetic(branch) == 0)
                        others = lambda: (lib.lfsr_get_arithmetic(), lib.lfsr_get_grad_arithmetic(), lib.lfsr_get_gemm_arithmetic())
                        assert others() == (arith, grad, gemm) and lib.lfsr_get_branch_arithmetic() == branch
                        assert lib.lfsr_set_branch_arithmetic(1 - branch) == 0          # moving this one ...
                        assert others() == (arith, grad, gemm)                          # ... leaves the other three
                        assert lib.lfsr_set_branch_arithmetic(branch) == 0
                        assert (lib.lfsr_set_arithmetic((arith + 1) % 3) == 0 and lib.lfsr_set_grad_arithmetic(1 - grad) == 0
                                and lib.lfsr_set_gemm_arithmetic(1 - gemm) == 0)       # moving the other three ...
                        assert lib.lfsr_get_branch_arithmetic() == branch               # ... leaves this one
    finally:
        _restore(lib)


def test_python_constants_match_the_header():
    src = open(os.path.join(ROOT, "include", "lfsr_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (LFSR_BRANCH_ARITH_\w+)\s+(\d+)", src, re.M)}
    assert defs == {"LFSR_BRANCH_ARITH_DEFAULT": capi.BRANCH_ARITH_DEFAULT, "LFSR_BRANCH_ARITH_BF16": capi.BRANCH_ARITH_BF16} == {"LFSR_BRANCH_ARITH_DEFAULT": 0, "LFSR_BRANCH_ARITH_BF16": 1}
    assert "lfsr_set_branch_arithmetic" in capi.SIGNATURES and "lfsr_get_branch_arithmetic" in capi.SIGNATURES


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc to emit the ISA")
def test_no_unpadded_hazard_around_the_branch_kernels_mfmas():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_asm_mfma_hazards.py"), "distg_bf16.hip"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    # k_epi_bf16: the step loop holds two steps of 5 taps x 2 row tiles x 2 position tiles = 2 x 20; k_distg_tail_bf16: three copies of the view body (two in the
    # loop, the trailing one) of 4 (EPIConv.2: 2 passes x 2 row tiles) + 20 (fuse.0: 5 K steps x 4 column tiles) = 3 x 24.  (AngConv.2's are fp32 MFMAs.)
    assert "distg_bf16.hip: 112 bf16 MFMAs checked" in r.stdout, r.stdout
