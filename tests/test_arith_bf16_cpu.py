"""CPU: the third value of the library's arithmetic selection, LFSR_ARITH_BF16 (include/lfsr_hip.h; csrc/options.cpp): accepted, read back, and an unknown
value still refused without changing the mode.  And the ISA of its kernel (csrc/conv3x3_bf16.hip issues its MFMAs as asm statements, so the compiler pads no
wait states for them) passes tools/check_asm_mfma_hazards.py."""
import os
import subprocess
import sys

import pytest

from lfsr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFSR_E_ARG = -1


def test_set_get_arithmetic_bf16():
    lib = capi.load()
    assert lib.lfsr_get_arithmetic() == 0
    try:
        assert lib.lfsr_set_arithmetic(2) == 0
        assert lib.lfsr_get_arithmetic() == 2
        assert capi.get_arithmetic() == 2
    finally:
        assert lib.lfsr_set_arithmetic(0) == 0
    assert lib.lfsr_get_arithmetic() == 0


def test_unknown_arithmetic_is_refused_and_changes_nothing():
    lib = capi.load()
    try:
        for mode in (0, 1, 2):
            assert lib.lfsr_set_arithmetic(mode) == 0
            assert lib.lfsr_set_arithmetic(3) == LFSR_E_ARG and lib.lfsr_set_arithmetic(-1) == LFSR_E_ARG
            assert lib.lfsr_get_arithmetic() == mode
    finally:
        lib.lfsr_set_arithmetic(0)
    with pytest.raises(capi.LfsrError):
        capi.set_arithmetic(3)
    assert lib.lfsr_get_arithmetic() == 0


def test_python_constants():
    assert (capi.ARITH_DEFAULT, capi.ARITH_F32, capi.ARITH_BF16) == (0, 1, 2)
    src = open(os.path.join(ROOT, "include", "lfsr_hip.h")).read()
    assert "#define LFSR_ARITH_BF16 2" in src


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc to emit the ISA")
def test_no_unpadded_hazard_around_the_bf16_conv_mfmas():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_asm_mfma_hazards.py"), "conv3x3_bf16.hip"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "72 bf16 MFMAs checked" in r.stdout
