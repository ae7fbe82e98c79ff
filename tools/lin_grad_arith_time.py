#!/usr/bin/env python3
"""Times the linears' gradients under capi.LIN_GRAD_ARITH_DEFAULT and capi.LIN_GRAD_ARITH_BF16, both forms interleaved in one process: `rounds` timings per form,
a warm-up before every timing; median and max - min (the run-to-run spread) of each.
  * part ops: the two operators, capi.linear_wgrad (kernel(s) + slab reduction) and capi.linear_dgrad (plain; masked + residual where the drivers run it so), at the
    scene geometry M = 8 x 25 x 32 x 32 = 204 800 rows for each (cout, cin) the drivers use; for the weight gradient the bytes of dy and x it must read over its
    time, beside a device copy of the same bytes;
  * part epit / lft: the x4 training step (forward, L1 loss, backward) through the plugin at B = 8, 5x5 views of 32x32, and the rel-L2 distance of the two buckets.
Without --part every part runs in a fresh child process under its own time limit (--limit seconds), and the JSON lines are gathered into --out.
usage: python tools/lin_grad_arith_time.py [--part ops|epit|lft] [--reps 20] [--steps 5] [--rounds 7] [--limit 240] [--out results/lin_grad_arith_time.json]"""
import argparse
import json
import os
import subprocess
import sys
from argparse import Namespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(64, 64), (64, 128), (128, 64), (128, 128), (128, 256), (256, 128), (256, 64), (576, 64), (1024, 64)]
MASKED = {(64, 128), (128, 256)}      # feed_forward.4's data gradient carries the ReLU' mask
M_SCENE = 8 * 25 * 32 * 32


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "spread": v[-1] - v[0]}


def part_ops(a):
    import torch
    from lfsr_amd import capi
    capi.load()
    modes = (("default", capi.LIN_GRAD_ARITH_DEFAULT), ("bf16", capi.LIN_GRAD_ARITH_BF16))

    def timed(f, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(n): f()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3      # us

    def ab(f):
        t = {name: [] for name, _ in modes}
        for _ in range(a.rounds):
            for name, mode in modes:
                capi.set_lin_grad_arithmetic(mode)
                for _ in range(3): f()
                t[name].append(timed(f, a.reps))
        capi.set_lin_grad_arithmetic(capi.LIN_GRAD_ARITH_DEFAULT)
        return {k: stats(v) for k, v in t.items()}

    g = torch.Generator(device="cuda").manual_seed(3)      # random operands (the bf16 pipe holds another clock on zeros)
    M, out = M_SCENE, {}
    for cout, cin in SHAPES:
        dy = torch.randn(M, cout, device="cuda", generator=g); x = torch.randn(M, cin, device="cuda", generator=g)
        wT = capi.pack_conv_weight_T((torch.randn(cout, cin, 1, 1, device="cuda", generator=g) * 0.1))
        dw, dx = torch.empty(cout, cin, device="cuda"), torch.empty(M, cin, device="cuda")
        masked = (cout, cin) in MASKED
        src = torch.empty(M * (cout + cin), device="cuda"); dst = torch.empty_like(src)
        r = {"wgrad_us": ab(lambda: capi.linear_wgrad(dy, x, cout, cin, dw=dw)),
             "dgrad_us": ab(lambda: capi.linear_dgrad(dy, wT, cin, r1=x if masked else None, act=x if masked else None, dx=dx)),
             "copy_us": stats([timed(lambda: dst.copy_(src), a.reps) for _ in range(a.rounds)]), "operand_MB": M * (cout + cin) * 4 / 1e6, "dgrad_masked": masked}
        for k in ("default", "bf16"):
            r[f"wgrad_{k}_GBps"] = r["operand_MB"] / r["wgrad_us"][k]["median"] * 1e3
        r["copy_GBps_read"] = r["operand_MB"] / r["copy_us"]["median"] * 1e3
        out[f"{cout}x{cin}"] = r
        print(f"M={M} ({cout:4d},{cin:3d}) wgrad default {r['wgrad_us']['default']['median']:8.1f} us (spread {r['wgrad_us']['default']['spread']:6.1f})  bf16 "
              f"{r['wgrad_us']['bf16']['median']:8.1f} us (spread {r['wgrad_us']['bf16']['spread']:6.1f}) = {r['wgrad_bf16_GBps']:6.0f} GB/s of operands, copy of the same "
              f"bytes {r['copy_us']['median']:7.1f} us | dgrad{' masked + r1' if masked else ''} default {r['dgrad_us']['default']['median']:8.1f} us "
              f"(spread {r['dgrad_us']['default']['spread']:6.1f})  bf16 {r['dgrad_us']['bf16']['median']:8.1f} us (spread {r['dgrad_us']['bf16']['spread']:6.1f})", flush=True)
        del dy, x, src, dst, dx
    return out


def part_model(a, name):
    import importlib
    import torch
    from lfsr_amd import capi
    from lfsr_amd.synth import synth_input, synth_state_dict
    A, h, w, s, B = 5, 32, 32, 4, 8
    Mod = importlib.import_module("lfsr_amd.model.SR." + name)
    net = Mod.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s)).cuda()
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.train()
    x = torch.from_numpy(synth_input((B, 1, A * h, A * w), seed=1)).cuda()
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).cuda()
    modes = (("default", capi.LIN_GRAD_ARITH_DEFAULT), ("bf16", capi.LIN_GRAD_ARITH_BF16))

    def step():
        torch.nn.functional.l1_loss(net(x), label).backward()

    def timed(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(n): step()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    t, bucket = {k: [] for k, _ in modes}, {}
    for _ in range(a.rounds):
        for k, mode in modes:
            capi.set_lin_grad_arithmetic(mode)
            for _ in range(2): step()
            t[k].append(timed(a.steps))
            for p in net.parameters(): p.grad = None
            step(); torch.cuda.synchronize()
            bucket[k] = net.grad_bucket.double().clone()
    capi.set_lin_grad_arithmetic(capi.LIN_GRAD_ARITH_DEFAULT)
    r = {"step_ms": {k: stats(v) for k, v in t.items()},
         "bucket_rel_l2_bf16_to_default": float((bucket["bf16"] - bucket["default"]).norm() / bucket["default"].norm()),
         "train_workspace_GB": net._rt.train_workspace_bytes(B, h, w) / 1e9}
    print(f"{name} x{s} train step B={B}: default {r['step_ms']['default']['median']:.2f} ms (spread {r['step_ms']['default']['spread']:.2f})  bf16 "
          f"{r['step_ms']['bf16']['median']:.2f} ms (spread {r['step_ms']['bf16']['spread']:.2f}); bucket rel-L2 bf16 to default {r['bucket_rel_l2_bf16_to_default']:.3e}", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["ops", "epit", "lft"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out", default="results/lin_grad_arith_time.json")
    a = ap.parse_args()
    if a.part:
        r = part_ops(a) if a.part == "ops" else part_model(a, {"epit": "EPIT", "lft": "LFT"}[a.part])
        print("JSON " + json.dumps({a.part: r}))
        return 0
    res = {"tool": "lin_grad_arith_time", "rows": M_SCENE, "reps": a.reps, "steps": a.steps, "rounds": a.rounds}
    for part in ("ops", "epit", "lft"):      # a fresh process and a time limit for each; the first that fails ends the run
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
