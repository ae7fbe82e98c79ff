"""GPU: a plain `bench.py` run prints the headline and what its timed steps recorded (`roofline`) and nothing that needs work of its own; `--full`
adds the all-fp32-MFMA headline, the per-class pass, the standalone index kernels and the batch-independence check."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("all_fp32_mfma", "roofline_classes", "kernel_ms_per_step", "batch_split_max_abs_diff", "other_workloads", "cpu_baseline")


def run_bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--batch", "4", *extra],
                       env=env, capture_output=True, text=True, timeout=400)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_has_only_the_headline_figures():
    line = run_bench()
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert abs(line["value"] - 4 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert line["config"]["gemm_arithmetic"]["epiconv"] == "bf16x3" and line["dtype"].startswith("f32 (EPI branch")
    assert line["roofline"]["launches_timed"] > 0 and 0 < line["roofline"]["frac"] < 1
    assert not set(FULL_ONLY) & set(line)


def test_full_adds_the_extra_figures():
    line = run_bench("--full", "--no-cpu-baseline", "--no-other-workloads")
    assert line["all_fp32_mfma"]["ms_per_step"] > 0
    assert {c["class"] for c in line["roofline_classes"]} >= {"epiconv", "pointwise", "angconv", "init_conv", "upsample_head"}
    assert line["kernel_ms_per_step"]["conv3x3"] > 0
    assert line["batch_split_max_abs_diff"] == 0.0
    assert "other_workloads" not in line and "cpu_baseline" not in line
