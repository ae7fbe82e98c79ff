"""CPU: the fused DistgSSR block tail (distg_tail.hip) issues its bf16 MFMAs as asm statements like the other three-term kernels; tools/check_asm_mfma_hazards.py
checks its gfx950 ISA for unpadded VALU -> MFMA and MFMA -> reader hazards."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc to emit the ISA")
def test_distg_tail_has_no_unpadded_hazard_around_asm_mfmas():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_asm_mfma_hazards.py"), "distg_tail.hip"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "distg_tail.hip: 432 bf16 MFMAs checked" in r.stdout, r.stdout
