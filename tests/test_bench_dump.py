"""CPU: bench.py's --dump-outputs writer (what the timed path returned, as .npy files under a size cap) and the --steps check.  No torch on the GPU:
the writer takes host arrays as well as tensors."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_outputs_written_whole(tmp_path):
    y = torch.rand(2, 1, 8, 8)
    loss = torch.tensor(0.25)
    rec = bench.dump_outputs(str(tmp_path / "out"), {"loss": loss, "sr": y, "d": np.arange(3, dtype=np.float64)})
    assert set(os.listdir(tmp_path / "out")) == {"loss.npy", "sr.npy", "d.npy"}
    a = np.load(tmp_path / "out" / "sr.npy")
    assert a.dtype == np.float32 and np.array_equal(a, y.numpy())
    assert np.load(tmp_path / "out" / "loss.npy").shape == () and float(np.load(tmp_path / "out" / "loss.npy")) == 0.25
    assert np.load(tmp_path / "out" / "d.npy").dtype == np.float64
    assert rec["arrays"]["sr"]["shape"] == [2, 1, 8, 8] and "sample" not in rec["arrays"]["sr"]
    json.dumps(rec)


def test_large_outputs_sampled_under_the_cap_and_reproducibly(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 40_000)
    big = np.random.default_rng(5).random((4, 1, 100, 100), dtype=np.float32)          # 160 kB
    small = np.ones(100, dtype=np.float32)
    r1 = bench.dump_outputs(str(tmp_path / "a"), {"big": big, "small": small})
    r2 = bench.dump_outputs(str(tmp_path / "b"), {"big": big.copy(), "small": small})
    assert r1["arrays"] == r2["arrays"]
    total = sum(np.load(tmp_path / "a" / f).nbytes for f in os.listdir(tmp_path / "a"))
    assert total <= 40_000
    s1, s2 = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert np.array_equal(s1, s2) and s1.ndim == 1 and 0 < s1.size == r1["arrays"]["big"]["sample"]["elements"]
    assert np.isin(s1, big.reshape(-1)).all()                                             # values of the output itself


def test_steps_must_be_positive():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--steps" in p.stderr
