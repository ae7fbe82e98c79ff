#!/usr/bin/env python3
"""LFT training step on the HIP path, timed with hipEvents: fwd (with its repack) + L1 + bwd, and the full step with clip_grad_norm_(1.0)
on the flat bucket + fused AdamW (lfsr_amd.train_step.train_step), 5x5 views of 32x32, x4, B = 8.  In the same process, the yardstick of
what a reference user gets: a stock-torch autograd step (fwd + L1 + bwd) of the port's graph (oracle.lfsr_torch_port.lft_forward) in fp32 on
the same GPU.  Prints one JSON line: the medians, the repack alone, the training workspace, the operator-level profile's top entries for one
step and the fraction of the arithmetic floor (3 x 62.4 GFLOP (windowed count) x B at 157.3 TFLOP/s).

    python tools/lft_train_time.py [--iters 10] [--batch 8]
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
from lfsr_amd.model.SR import LFT as M  # noqa: E402
from oracle.lfsr_torch_port import lft_forward  # noqa: E402

FWD_GFLOP, PEAK_TFLOPS = 62.4, 157.3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--hip-only", action="store_true", help="without the stock-torch yardstick: a short process, for alternating two builds (LFSR_HIP_LIB)")
    a = ap.parse_args()
    A, h, w, s, B, iters = 5, 32, 32, 4, a.batch, a.iters
    net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s)).cuda()
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    crit = M.get_loss(None)
    x = torch.from_numpy(synth_input((B, 1, A * h, A * w), seed=1)).cuda()
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).cuda()
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
    r["op_profile_top"] = [[f"{op}({a_},{b_})", round(ms, 3), n] for (op, a_, b_), (ms, n) in top]
    r["profiled_ms_total"] = round(sum(ms for ms, _ in prof.values()), 3)
    r["train_workspace_GB"] = net._rt.train_workspace_bytes(B, h, w) / 1e9
    floor_ms = 3 * FWD_GFLOP * B / PEAK_TFLOPS
    r["floor_ms"] = floor_ms
    r["floor_fraction"] = floor_ms / r["step_ms"]
    del opt, net
    torch.cuda.empty_cache()

    if not a.hip_only:
        # the stock-torch yardstick: autograd over the port's graph, fp32, same inputs and weights (PE and mask built on the device)
        with torch.device("cuda"):
            params = {k: torch.tensor(v, requires_grad=True) for k, v in sd.items()}

            def torch_step():
                for p in params.values():
                    p.grad = None
                out = lft_forward.__wrapped__(x, params, A, s)
                torch.nn.functional.l1_loss(out, label).backward()

            torch_step()
            torch.cuda.synchronize()
            r["torch_fwd_bwd_ms"] = timed(torch_step, max(3, iters // 2))
        r["speedup_vs_torch"] = r["torch_fwd_bwd_ms"] / r["fwd_bwd_ms"]
    res = {"tool": "lft_train_time", "config": f"LFT 5x5 32x32 x{s} B={B} fp32", "device": torch.cuda.get_device_name(0)}
    res.update({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
