"""CPU: the streaming loops of k_distg_tail and k_epi_b3<false> keep the rows they have just requested in flight.  tools/check_asm_waits.py compiles both files
to gfx950 ISA with the Makefile's flags and checks that
  * in k_distg_tail's view loop (the innermost loop holding bf16 MFMAs) no s_waitcnt has a vmcnt below the number of loads a body issues for the next view
    (6 at one-view depth: four SpaConv.2 row loads, two t_V row loads; 8 with the two t_H loads every body now issues), that the kernel has no scratch
    and at most 256 VGPRs (two waves per SIMD);
  * in k_epi_b3<false>'s step loop the waits in front of the weights' ds_write_b128 leave at least the four X loads outstanding.
On the revision before this test both checks fail: the view loop had vmcnt(0) and vmcnt(1) in both bodies (its loads of the next t_H row and of the next view
sat behind run-time branches), and the step loop waited vmcnt(1) / vmcnt(0) for its weights behind the X loads."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_hipcc = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc to emit the ISA")


def _run(only):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_asm_waits.py"), "--only", only], capture_output=True, text=True, timeout=900)


@needs_hipcc
def test_distg_tail_view_loop_leaves_the_next_views_loads_in_flight():
    r = _run("tail")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "k_distg_tail: view loop" in r.stdout and "ScratchSize 0" in r.stdout, r.stdout


@needs_hipcc
def test_epi_b3_stage1_step_loop_leaves_the_x_loads_in_flight():
    r = _run("epi")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "k_epi_b3<false>: step loop" in r.stdout and "ScratchSize 0" in r.stdout, r.stdout
