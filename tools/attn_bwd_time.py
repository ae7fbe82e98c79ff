#!/usr/bin/env python
"""A/B timing of the EPI attention backward (lfsr_window_attn_bwd at EPIT's geometry, both passes): the matrix-pipe kernel k_epi_attn_bwd_mfma
against the VALU pair (LFSR_ATTN=valu) on the same tensors, inside ONE process, alternating round by round after a warm-up of both.

    python tools/attn_bwd_time.py [--batch 8] [--rounds 12] [--reps 20] [--out results/attn_bwd_time.json]

Per (pass, path): the median over the rounds of the mean time of `reps` back-to-back launches (event-timed), and the spread (max - min) over the rounds."""
import argparse
import json
import os
import sys

os.environ.setdefault("LFSR_LAB", "1")   # (this tool drives the library's A/B selectors, live only under LFSR_LAB)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from lfsr_amd import capi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="results/attn_bwd_time.json")
    a = ap.parse_args()
    lib = capi.load()
    B, A, h, w, E, NH = a.batch, 5, 32, 32, 128, 8
    HW, npix = h * w, a.batch * 25 * h * w
    g = torch.Generator(device="cuda").manual_seed(0)
    qk = torch.randn(npix, 2 * E, device="cuda", generator=g)
    v, o, d_o = (torch.randn(npix, E, device="cuda", generator=g) for _ in range(3))
    dqk, dv, stats = torch.empty_like(qk), torch.empty_like(v), torch.empty(npix * NH * 4, device="cuda")
    geoms = {"horizontal": (B, A, w, A * A * HW, HW, 1, A, h, A * HW, w), "vertical": (B, A, h, A * A * HW, A * HW, w, A, w, HW, 1)}

    def launch(key):
        capi.check(lib.lfsr_window_attn_bwd(capi.dev_ptr(qk), 2 * E, 0, E, capi.dev_ptr(v), E, 0, capi.dev_ptr(o), capi.dev_ptr(d_o), E, 0, capi.dev_ptr(dqk),
                                            capi.dev_ptr(dv), capi.dev_ptr(stats), NH, E // NH, *geoms[key], A, A, 5, 6, 0, capi.stream_ptr()), "attn_bwd")

    def timed(key, path):
        if path == "valu":
            os.environ["LFSR_ATTN"] = "valu"
        else:
            os.environ.pop("LFSR_ATTN", None)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            launch(key)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.reps     # us per launch

    times = {(k, p): [] for k in geoms for p in ("mfma", "valu")}
    for r in range(a.rounds + 2):                     # two warm-up rounds of every (pass, path)
        for k in geoms:
            for p in ("mfma", "valu"):
                t = timed(k, p)
                if r >= 2:
                    times[(k, p)].append(t)
    res = {"tool": "attn_bwd_time", "config": f"EPIT 5x5 32x32 B={B}: 8 heads of 16, 160 tokens per sequence", "device": torch.cuda.get_device_name(0),
           "rounds": a.rounds, "reps": a.reps, "us_per_launch": {}}
    for (k, p), ts in times.items():
        res["us_per_launch"][f"{k}/{p}"] = {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts)), "spread": float(max(ts) - min(ts))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
