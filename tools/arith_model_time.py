#!/usr/bin/env python3
"""Times the DistgSSR x4 forward through the plugin (model/SR/DistgSSR.py, eval, no_grad) at the bench geometry -- a batch of 5x5 views of 32x32 -- under the
default arithmetic and under capi.ARITH_BF16 (the 64 -> 64 3x3 forward conv on bf16 operands), interleaved in one process: `rounds` timings of `steps` forwards
per mode, two warm-up forwards before every timing; median and max - min of each, and the difference of the two outputs.
usage: python tools/arith_model_time.py [batch] [steps] [rounds]"""
import importlib, json, os, sys
from argparse import Namespace
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lfsr_amd import capi
from lfsr_amd.synth import synth_input, synth_state_dict
B = int(sys.argv[1]) if len(sys.argv) > 1 else 32
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
A, S, H, W = 5, 4, 32, 32
sys.path.insert(0, capi._HERE)
M = importlib.import_module("model.SR.DistgSSR")
sys.path.remove(capi._HERE)
meta = json.load(open(os.path.join(ROOT, "tests", "golden", "models.json")))["models"]["DistgSSR"]["full"]
sd = synth_state_dict([(k, tuple(s)) for k, s in meta["spec"]], seed=0)
net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=S))
net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
net = net.cuda().eval()
x = torch.from_numpy(synth_input((B, 1, A * H, A * W), seed=1)).cuda()
MODES = (("default", capi.ARITH_DEFAULT), ("bf16", capi.ARITH_BF16))
t, out = {name: [] for name, _ in MODES}, {}
with torch.no_grad():
    for _ in range(rounds):
        for name, mode in MODES:
            capi.set_arithmetic(mode)
            for _ in range(2): y = net(x)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); e0.record()
            for _ in range(steps): y = net(x)
            e1.record(); torch.cuda.synchronize()
            t[name].append(e0.elapsed_time(e1) / steps)
            out[name] = y.clone()
capi.set_arithmetic(capi.ARITH_DEFAULT)
for name, _ in MODES:
    v = sorted(t[name])
    print(f"DistgSSR x4 plugin forward B={B} {name:8s}: median {v[len(v) // 2]:7.3f} ms/step  min {v[0]:7.3f}  max {v[-1]:7.3f}  spread {v[-1] - v[0]:6.3f}  ({rounds} x {steps} steps)", flush=True)
d = (out["bf16"] - out["default"]).double()
print(f"bf16 - default: rms {float(d.pow(2).mean().sqrt()):.3e}  max {float(d.abs().max()):.3e}")
