#!/usr/bin/env python3
"""LF_InterNet training step on the HIP path, timed with hipEvents: fwd (with its repack) + L1 + bwd, and the full step with
clip_grad_norm_(1.0) on the flat bucket + AdamW (lfsr_amd.train_step.train_step), 5x5 views of 32x32, B = 8, at x2 and x4.
Prints one JSON line: per scale the median ms of each, the repack alone, the training workspace, the fraction of the arithmetic floor
(3 x 84.65 GFLOP x B at 157.3 TFLOP/s fp32 MFMA), and the operator-level profile's top entries for one step.

    python tools/internet_train_time.py [--iters 10] [--batch 8]
"""
import argparse
import json
import os
import sys
from argparse import Namespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lfsr_amd import capi  # noqa: E402
from lfsr_amd.synth import synth_input, synth_state_dict  # noqa: E402
from lfsr_amd.train_step import train_step  # noqa: E402
from lfsr_amd.model.SR import LF_InterNet as M  # noqa: E402

FWD_GFLOP, PEAK_TFLOPS = 84.65, 157.3


def timed(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def run(scale, B, iters, A=5, h=32, w=32):
    net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=scale)).cuda()
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    crit = M.get_loss(None)
    x = torch.from_numpy(synth_input((B, 1, A * h, A * w), seed=1)).cuda()
    label = torch.from_numpy(synth_input((B, 1, A * h * scale, A * w * scale), seed=2)).cuda()
    opt = torch.optim.AdamW(net.parameters(), lr=1e-4, fused=True)

    def fwd_bwd():
        crit(net(x), label).backward()

    def step():
        train_step(net, crit, opt, x, label)

    def repack():
        net._train_runtime(x.device)

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    r = {"fwd_bwd_ms": timed(fwd_bwd, iters), "step_ms": timed(step, iters), "repack_ms": timed(repack, iters)}
    with torch.no_grad():
        r["inference_fwd_ms"] = timed(lambda: net(x), iters)
    capi.op_profile(True)
    step()
    torch.cuda.synchronize()
    prof = capi.op_profile_read()
    capi.op_profile(False)
    top = sorted(prof.items(), key=lambda kv: -kv[1][0])[:6]
    r["op_profile_top"] = [[f"{op}({a},{b})", round(ms, 3), n] for (op, a, b), (ms, n) in top]
    r["profiled_ms_total"] = round(sum(ms for ms, _ in prof.values()), 3)
    r["train_workspace_GB"] = net._rt.train_workspace_bytes(B, h, w) / 1e9
    floor_ms = 3 * FWD_GFLOP * B / PEAK_TFLOPS
    r["floor_ms"] = floor_ms
    r["floor_fraction"] = floor_ms / r["step_ms"]
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    res = {"tool": "internet_train_time", "config": f"LF_InterNet 5x5 32x32 B={a.batch} fp32", "device": torch.cuda.get_device_name(0)}
    for s in (2, 4):
        res[f"x{s}"] = run(s, a.batch, a.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
