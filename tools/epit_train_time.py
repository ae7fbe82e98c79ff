#!/usr/bin/env python3
"""EPIT training step on the HIP path, timed with hipEvents: fwd (with its repack) + L1 + bwd, and the full step with clip_grad_norm_(1.0)
on the flat bucket + fused AdamW (lfsr_amd.train_step.train_step), 5x5 views of 32x32, x4, B = 8.  The criterion is a local L1 (the reference's
get_loss cannot be called, EPIT.py:178).  In the same process, the yardstick of what a reference user gets: a stock-torch autograd step
(fwd + L1 + bwd) of the port's graph (oracle.lfsr_torch_port.epit_forward) in fp32 on the same GPU.  Prints one JSON line (and writes it to
--out): the medians, the repack alone, the training workspace and the operator-level profile's top entries for one step.  The A/B of the
attention backward's two paths is tools/attn_bwd_time.py.

    python tools/epit_train_time.py [--iters 10] [--batch 8] [--out results/epit_train_time.json]
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
from lfsr_amd.model.SR import EPIT as M  # noqa: E402
from oracle.lfsr_torch_port import epit_forward  # noqa: E402

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
    ap.add_argument("--out", default="results/epit_train_time.json")
    a = ap.parse_args()
    A, h, w, s, B, iters = 5, 32, 32, 4, a.batch, a.iters
    net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s)).cuda()
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    crit = lambda out, lab, info=None: torch.nn.functional.l1_loss(out, lab)      # noqa: E731
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
    top = sorted(prof.items(), key=lambda kv: -kv[1][0])[:8]
    r["op_profile_top"] = [[f"{op}({a_},{b_})", round(ms, 3), n] for (op, a_, b_), (ms, n) in top]
    r["profiled_ms_total"] = round(sum(ms for ms, _ in prof.values()), 3)
    r["train_workspace_GB"] = net._rt.train_workspace_bytes(B, h, w) / 1e9
    del opt, net
    torch.cuda.empty_cache()

    if not a.hip_only:
        # the stock-torch yardstick: autograd over the port's graph, fp32, same inputs and weights (the mask is built on the device)
        with torch.device("cuda"):
            params = {k: torch.tensor(v, requires_grad=True) for k, v in sd.items()}

            def torch_step():
                for p in params.values():
                    p.grad = None
                out = epit_forward.__wrapped__(x, params, A, s)
                torch.nn.functional.l1_loss(out, label).backward()

            torch_step()
            torch.cuda.synchronize()
            r["torch_fwd_bwd_ms"] = timed(torch_step, max(3, iters // 2))
        r["speedup_vs_torch"] = r["torch_fwd_bwd_ms"] / r["fwd_bwd_ms"]
    res = {"tool": "epit_train_time", "config": f"EPIT 5x5 32x32 x{s} B={B} fp32", "device": torch.cuda.get_device_name(0)}
    res.update({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
