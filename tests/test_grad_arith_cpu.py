"""CPU: the library's second arithmetic selection, lfsr_set_grad_arithmetic (include/lfsr_hip.h; csrc/options.cpp): LFSR_GRAD_ARITH_BF16 is accepted and read
back, any other value is refused without changing the mode, and the switch and lfsr_set_arithmetic do not move each other.  And the ISA of its two kernels
(csrc/conv3x3_bf16_dgrad.hip, csrc/wgrad_bf16.hip: MFMAs issued as asm statements, so the compiler pads no wait states for them) passes
tools/check_asm_mfma_hazards.py, with the forward's file still at its 72 MFMAs."""
import os
import re
import subprocess
import sys

import pytest

from lfsr_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LFSR_E_ARG = -1


def test_set_get_grad_arithmetic():
    lib = capi.load()
    assert lib.lfsr_get_grad_arithmetic() == 0
    try:
        assert lib.lfsr_set_grad_arithmetic(1) == 0
        assert lib.lfsr_get_grad_arithmetic() == 1
        assert capi.get_grad_arithmetic() == capi.GRAD_ARITH_BF16
        capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT)
        assert lib.lfsr_get_grad_arithmetic() == 0
        capi.set_grad_arithmetic(capi.GRAD_ARITH_BF16)
        assert lib.lfsr_get_grad_arithmetic() == 1
    finally:
        assert lib.lfsr_set_grad_arithmetic(0) == 0
    assert lib.lfsr_get_grad_arithmetic() == 0


def test_unknown_grad_arithmetic_is_refused_and_changes_nothing():
    lib = capi.load()
    try:
        for mode in (0, 1):
            assert lib.lfsr_set_grad_arithmetic(mode) == 0
            assert lib.lfsr_set_grad_arithmetic(2) == LFSR_E_ARG and lib.lfsr_set_grad_arithmetic(-1) == LFSR_E_ARG
            assert lib.lfsr_get_grad_arithmetic() == mode
    finally:
        lib.lfsr_set_grad_arithmetic(0)
    with pytest.raises(capi.LfsrError):
        capi.set_grad_arithmetic(2)
    assert lib.lfsr_get_grad_arithmetic() == 0


def test_the_two_switches_are_independent():
    lib = capi.load()
    try:
        for arith in (0, 1, 2):
            for grad in (0, 1):
                assert lib.lfsr_set_arithmetic(arith) == 0
                assert lib.lfsr_set_grad_arithmetic(grad) == 0
                assert (lib.lfsr_get_arithmetic(), lib.lfsr_get_grad_arithmetic()) == (arith, grad)
                assert lib.lfsr_set_arithmetic(0) == 0                      # moving one ...
                assert lib.lfsr_get_grad_arithmetic() == grad               # ... leaves the other
                assert lib.lfsr_set_arithmetic(arith) == 0
                assert lib.lfsr_set_grad_arithmetic(1 - grad) == 0
                assert lib.lfsr_get_arithmetic() == arith
    finally:
        lib.lfsr_set_arithmetic(0)
        lib.lfsr_set_grad_arithmetic(0)


def test_python_constants_match_the_header():
    src = open(os.path.join(ROOT, "include", "lfsr_hip.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"^#define (LFSR_GRAD_ARITH_\w+)\s+(\d+)", src, re.M)}
    assert defs == {"LFSR_GRAD_ARITH_DEFAULT": capi.GRAD_ARITH_DEFAULT, "LFSR_GRAD_ARITH_BF16": capi.GRAD_ARITH_BF16}
    assert "lfsr_set_grad_arithmetic" in capi.SIGNATURES and "lfsr_get_grad_arithmetic" in capi.SIGNATURES


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc to emit the ISA")
def test_no_unpadded_hazard_around_the_gradient_kernels_mfmas():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_asm_mfma_hazards.py"), "conv3x3_bf16_dgrad.hip", "wgrad_bf16.hip", "conv3x3_bf16.hip"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    # the masked conv: 9 taps x 4 K steps x 2 column tiles; the weight gradient: 8 K steps x (5 + 4) taps of its two wave groups; the forward: what it was
    for f in ("conv3x3_bf16_dgrad.hip", "wgrad_bf16.hip", "conv3x3_bf16.hip"):
        assert f"{f}: 72 bf16 MFMAs checked" in r.stdout, r.stdout
