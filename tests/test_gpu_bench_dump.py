"""GPU: `bench.py --dump-outputs DIR` writes what the timed path computed -- the headline's SR batch equals a fresh forward of the same seeded weights and
patches in this process -- and the result line counts exactly --steps timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_infer_dump_is_the_forward_of_the_seeded_inputs(tmp_path):
    from lfsr_amd import capi
    from lfsr_amd.synth import synth_input, synth_state_dict
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "4", "--no-cpu-baseline", "--no-other-workloads",
           "--no-split-check", "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert abs(line["value"] - 4 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert line["dumped_outputs"]["arrays"]["sr"]["shape"] == [4, 1, 640, 640]
    got = np.load(tmp_path / "sr.npy")
    assert got.dtype == np.float32 and got.shape == (4, 1, 640, 640)
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "models.json")))["models"]["DistgSSR"]["full"]
    sd = synth_state_dict([(k, tuple(s)) for k, s in meta["spec"]], seed=0)
    dev = torch.device("cuda", 0)
    rt = capi.DistgSSRRuntime(5, 4)
    rt.load_state([(k, torch.from_numpy(v).to(dev)) for k, v in sd.items()], dev)
    want = rt.forward(torch.from_numpy(synth_input((4, 1, 160, 160), seed=1)).to(dev)).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-5
