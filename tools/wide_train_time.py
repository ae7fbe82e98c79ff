#!/usr/bin/env python3
"""Times LF_InterNet's wide per-view 3x3 convs in training under capi.set_wide_train_arithmetic, every form interleaved in one process: `rounds` timings per form,
a warm-up before every timing; median and max - min (the run-to-run spread) of each.  5x5 views of 32x32, B = 8 (200 views, 204 800 pixels).
  * part ops, for cin 128 and 320: the operator lfsr_conv3x3_wide_wgrad (kernel + slab reduction) in mode 0 (the generic gather weight-gradient kernel) and in
    mode 1 (csrc/wgrad_wide_bf16.hip), and the yardstick a trivial implementation would be: cin / 64 calls of lfsr_conv3x3_wgrad under GRAD_ARITH_BF16 on the same dy
    and the 64-channel slices of x (csrc/wgrad_bf16.hip, each call with its own reduction).  Workspaces are allocated once, outside the timings.  `not_slower`: the
    mode-1 median is no more than the chunk loop's plus the larger of the two spreads.
  * part step: the x2 training step (forward, L1 loss, backward; and the full step with clip_grad_norm_ and AdamW, as tools/internet_train_time.py) through the
    plugin in modes 0, 1, 2, and 2 with GRAD_ARITH_BF16, with the rel-L2 distance of each bucket to the default's.
Without --part every part runs in a fresh child process under its own time limit (--limit seconds), and the JSON lines are gathered into --out.
usage: python tools/wide_train_time.py [--part ops|step] [--reps 20] [--steps 5] [--rounds 7] [--limit 240] [--out results/wide_train_time.json]"""
import argparse
import json
import os
import subprocess
import sys
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
A, H, W, B = 5, 32, 32, 8
N_IMG = B * A * A


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "spread": v[-1] - v[0]}


def part_ops(a):
    import torch
    from lfsr_amd import capi
    lib, P = capi.load(), capi.dev_ptr

    def timed(f, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(n): f()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3      # us

    g = torch.Generator(device="cuda").manual_seed(3)      # random operands (the bf16 pipe holds another clock on zeros)
    M, out = N_IMG * H * W, {}
    for cin in (128, 320):
        dy = torch.randn(M, 64, device="cuda", generator=g); x = torch.randn(M, cin, device="cuda", generator=g)
        dw = torch.empty(64, cin, 3, 3, device="cuda"); dw64 = torch.empty(cin // 64, 64, 64, 3, 3, device="cuda")
        ws = torch.empty(lib.lfsr_conv3x3_wide_wgrad_workspace_floats(cin, N_IMG, H, W), device="cuda")
        ws64 = torch.empty(lib.lfsr_conv3x3_wgrad_workspace_floats(N_IMG, H, W), device="cuda")

        def wide():
            capi.check(lib.lfsr_conv3x3_wide_wgrad(P(dy), 64, 0, P(x), cin, 0, cin, P(dw), P(ws), ws.numel(), N_IMG, H, W, 0, capi.stream_ptr()), "conv3x3_wide_wgrad")

        def chunk_loop():
            for k in range(cin // 64):
                capi.check(lib.lfsr_conv3x3_wgrad(P(dy), 64, 0, P(x), cin, 64 * k, P(dw64[k]), P(ws64), ws64.numel(), N_IMG, H, W, 0, capi.stream_ptr()), "conv3x3_wgrad")

        forms = (("mode0", wide, capi.WIDE_TRAIN_ARITH_DEFAULT, capi.GRAD_ARITH_DEFAULT), ("mode1", wide, capi.WIDE_TRAIN_ARITH_BF16_WGRAD, capi.GRAD_ARITH_DEFAULT),
                 ("chunk_loop_grad_bf16", chunk_loop, capi.WIDE_TRAIN_ARITH_DEFAULT, capi.GRAD_ARITH_BF16))
        t = {name: [] for name, *_ in forms}
        for _ in range(a.rounds):
            for name, f, wt, gr in forms:
                capi.set_wide_train_arithmetic(wt); capi.set_grad_arithmetic(gr)
                for _ in range(3): f()
                t[name].append(timed(f, a.reps))
        capi.set_wide_train_arithmetic(capi.WIDE_TRAIN_ARITH_DEFAULT); capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT)
        r = {k: stats(v) for k, v in t.items()}
        # the two bf16 forms compute the same sums: the distance is fp32 summation order
        capi.set_wide_train_arithmetic(capi.WIDE_TRAIN_ARITH_BF16_WGRAD); wide()
        capi.set_wide_train_arithmetic(capi.WIDE_TRAIN_ARITH_DEFAULT); capi.set_grad_arithmetic(capi.GRAD_ARITH_BF16); chunk_loop()
        capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT); torch.cuda.synchronize()
        loop = torch.cat(list(dw64.double()), 1)
        r["rel_l2_mode1_to_chunk_loop"] = float((dw.double() - loop).norm() / loop.norm())
        r["workspace_MB"] = ws.numel() * 4 / 1e6
        r["chunk_loop_workspace_MB"] = ws64.numel() * 4 / 1e6
        r["not_slower"] = bool(r["mode1"]["median"] <= r["chunk_loop_grad_bf16"]["median"] + max(r["mode1"]["spread"], r["chunk_loop_grad_bf16"]["spread"]))
        out[f"cin{cin}"] = r
        print(f"cin {cin} n_img {N_IMG} {H}x{W}: mode 0 {r['mode0']['median']:7.1f} us (spread {r['mode0']['spread']:5.1f})  mode 1 {r['mode1']['median']:7.1f} us "
              f"(spread {r['mode1']['spread']:5.1f})  chunk loop of the 64 -> 64 kernel under GRAD_ARITH_BF16 {r['chunk_loop_grad_bf16']['median']:7.1f} us "
              f"(spread {r['chunk_loop_grad_bf16']['spread']:5.1f}); not slower: {r['not_slower']}; rel-L2 mode 1 to chunk loop {r['rel_l2_mode1_to_chunk_loop']:.2e}", flush=True)
        del dy, x, ws, ws64
    return out


def part_step(a):
    import torch
    from lfsr_amd import capi
    from lfsr_amd.model.SR import LF_InterNet as Mod
    from lfsr_amd.synth import synth_input, synth_state_dict
    from lfsr_amd.train_step import train_step
    s = 2
    net = Mod.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s)).cuda()
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.train()
    crit = Mod.get_loss(None)
    opt = torch.optim.AdamW(net.parameters(), lr=0.0, fused=True)      # (lr 0: every form steps from the same weights)
    x = torch.from_numpy(synth_input((B, 1, A * H, A * W), seed=1)).cuda()
    label = torch.from_numpy(synth_input((B, 1, A * H * s, A * W * s), seed=2)).cuda()
    forms = (("mode0", capi.WIDE_TRAIN_ARITH_DEFAULT, capi.GRAD_ARITH_DEFAULT), ("mode1", capi.WIDE_TRAIN_ARITH_BF16_WGRAD, capi.GRAD_ARITH_DEFAULT),
             ("mode2", capi.WIDE_TRAIN_ARITH_BF16, capi.GRAD_ARITH_DEFAULT), ("mode2_grad_bf16", capi.WIDE_TRAIN_ARITH_BF16, capi.GRAD_ARITH_BF16))

    def fwd_bwd():
        crit(net(x), label).backward()

    def step():
        train_step(net, crit, opt, x, label)

    def timed(f, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(n): f()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    t, tf, bucket = {k: [] for k, *_ in forms}, {k: [] for k, *_ in forms}, {}
    for _ in range(a.rounds):
        for k, wt, gr in forms:
            capi.set_wide_train_arithmetic(wt); capi.set_grad_arithmetic(gr)
            for _ in range(2): step()
            t[k].append(timed(step, a.steps))
            tf[k].append(timed(fwd_bwd, a.steps))
            for p in net.parameters(): p.grad = None
            fwd_bwd(); torch.cuda.synchronize()
            bucket[k] = net.grad_bucket.double().clone()
    capi.set_wide_train_arithmetic(capi.WIDE_TRAIN_ARITH_DEFAULT); capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT)
    r = {"step_ms": {k: stats(v) for k, v in t.items()}, "fwd_bwd_ms": {k: stats(v) for k, v in tf.items()},
         "bucket_rel_l2_to_default": {k: float((bucket[k] - bucket["mode0"]).norm() / bucket["mode0"].norm()) for k in bucket},
         "train_workspace_GB": net._rt.train_workspace_bytes(B, H, W) / 1e9}
    for k, *_ in forms:
        print(f"LF_InterNet x{s} train step B={B} {k:16s}: step {r['step_ms'][k]['median']:6.2f} ms (spread {r['step_ms'][k]['spread']:.2f})  fwd + bwd "
              f"{r['fwd_bwd_ms'][k]['median']:6.2f} ms (spread {r['fwd_bwd_ms'][k]['spread']:.2f}); bucket rel-L2 to the default {r['bucket_rel_l2_to_default'][k]:.3e}", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["ops", "step"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default="results/wide_train_time.json")
    a = ap.parse_args()
    if a.part:
        r = part_ops(a) if a.part == "ops" else part_step(a)
        print("JSON " + json.dumps({a.part: r}))
        return 0
    res = {"tool": "wide_train_time", "config": f"{A}x{A} views of {H}x{W}, B = {B}", "reps": a.reps, "steps": a.steps, "rounds": a.rounds}
    for part in ("ops", "step"):      # a fresh process and a time limit for each; the first that fails ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(a.reps), "--steps", str(a.steps), "--rounds", str(a.rounds)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        sys.stdout.write("".join(l + "\n" for l in p.stdout.splitlines() if not l.startswith("JSON ")))
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            return p.returncode
        res.update(json.loads([l for l in p.stdout.splitlines() if l.startswith("JSON ")][-1][5:]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
