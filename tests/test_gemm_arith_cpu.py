"""CPU: the library's third arithmetic selection, lfsr_set_gemm_arithmetic (include/lfsr_hip.h; csrc/options.cpp): LFSR_GEMM_ARITH_BF16 is accepted and read
back, any other value is refused without changing the mode, and the switch does not move lfsr_set_arithmetic / lfsr_set_grad_arithmetic nor they it.  And the
ISA of its kernels (csrc/gemm_bf16.hip: MFMAs issued as asm statements, so the compiler pads no wait states for them) passes tools/check_asm_mfma_hazards.py."""
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


def test_set_get_gemm_arithmetic():
    lib = capi.load()
    assert lib.lfsr_get_gemm_arithmetic() == 0
    try:
        assert lib.lfsr_set_gemm_arithmetic(1) == 0
        assert lib.lfsr_get_gemm_arithmetic() == 1
        assert capi.get_gemm_arithmetic() == capi.GEMM_ARITH_BF16
        capi.set_gemm_arithmetic(capi.GEMM_ARITH_DEFAULT)
        assert lib.lfsr_get_gemm_arithmetic() == 0
        capi.set_gemm_arithmetic(capi.GEMM_ARITH_BF16)
        assert lib.lfsr_get_gemm_arithmetic() == 1
    finally:
        _restore(lib)
    assert lib.lfsr_get_gemm_arithmetic() == 0


def test_unknown_gemm_arithmetic_is_refused_and_changes_nothing():
    lib = capi.load()
    try:
        for mode in (0, 1):
            assert lib.lfsr_set_gemm_arithmetic(mode) == 0
            assert lib.lfsr_set_gemm_arithmetic(2) == LFSR_E_ARG and lib.lfsr_set_gemm_arithmetic(-1) == LFSR_E_ARG
            assert lib.lfsr_get_gemm_arithmetic() == mode
    finally:
        _restore(lib)
    try:
        with pytest.raises(capi.LfsrError):
            capi.set_gemm_arithmetic(2)
        assert lib.lfsr_get_gemm_arithmetic() == 0
    finally:
        _restore(lib)


def test_the_three_switches_are_independent():
    lib = capi.load()
    try:
        for arith in (0, 1, 2):
            for grad in (0, 1):
                for gemm in (0, 1):
                    assert lib.lfsr_set_arithmetic(arith) == 0 and lib.lfsr_set_grad_arithmetic(grad) == 0 and lib.lfsr_set_gemm_arithmetic(gemm) == 0
                    assert (lib.lfsr_get_arithmetic(), lib.lfsr_get_grad_arithmetic(), lib.lfsr_get_gemm_arithmetic()) == (arith, grad, gemm)
                    assert lib.lfsr_set_gemm_arithmetic(1 - gemm) == 0                                    # moving this one ...
                    assert (lib.lfsr_get_arithmetic(), lib.lfsr_get_grad_arithmetic()) == (arith, grad)   # ... leaves the other two
                    assert lib.lfsr_set_gemm_arithmetic(gemm) == 0
                    assert lib.lfsr_set_arithmetic((arith + 1) % 3) == 0 and lib.lfsr_set_grad_arithmetic(1 - grad) == 0     # moving the other two ...
                    assert lib.lfsr_get_gemm_arithmetic() == gemm                                         # ... leaves this one
    finally:
        _restore(lib)


def test_python_constants_match_the_header():
    src = open(os.path.join(ROOT, "include", "lfsr_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (LFSR_GEMM_ARITH_\w+)\s+(\d+)", src, re.M)}
    assert defs == {"LFSR_GEMM_ARITH_DEFAULT": capi.GEMM_ARITH_DEFAULT, "LFSR_GEMM_ARITH_BF16": capi.GEMM_ARITH_BF16} == {"LFSR_GEMM_ARITH_DEFAULT": 0, "LFSR_GEMM_ARITH_BF16": 1}
    assert "lfsr_set_gemm_arithmetic" in capi.SIGNATURES and "lfsr_get_gemm_arithmetic" in capi.SIGNATURES


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc to emit the ISA")
def test_no_unpadded_hazard_around_the_gemm_kernels_mfmas():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_asm_mfma_hazards.py"), "gemm_bf16.hip"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    # MFMAs per tile and wave, (N / 16) (K / 32): the linears at K = 64, N = 64 / 128 / 256: 8 + 16 + 32; at K = 128: 16 + 32 + 64; LayerNorm + q | k | v: 96 (128, 384)
    # + 24 (64, 192); feed-forward: 64 + 64 (E = 128) + 16 + 16 (E = 64)
    assert "gemm_bf16.hip: 448 bf16 MFMAs checked" in r.stdout, r.stdout
