#!/usr/bin/env python3
"""Times lfsr_angconv3x3_fwd in both of its arithmetics (default; lfsr_set_ang_arithmetic(LFSR_ANG_ARITH_BF16)) beside lfsr_conv3x3_fwd (the per-view 3x3 conv in
the default arithmetic: the same dense FLOP count on the same tensors) at angRes 5, B = 8, views of 32x32 and 64x64, interleaved in this process (`rounds` timings
of `reps` launches each, a warm-up before every timing, random operands), then the whole LFSSR x4 forward at B = 8 on 32x32 views in the four combinations of
LFSR_ANG_ARITH_BF16 and LFSR_ARITH_BF16, interleaved as well.  Device events around launches that end in a synchronise.
usage: python tools/lfssr_time.py [reps] [rounds] [steps]"""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lfsr_amd import capi
from lfsr_amd.synth import synth_input
from tests.lfssr_helpers import lfssr_spec, lfssr_state_dict
capi.load()
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
A, B = 5, 8
EXECUTED = sum((3 - (u in (0, A - 1))) * (3 - (v in (0, A - 1))) for u in range(A) for v in range(A)) / (9.0 * A * A)    # 169 / 225


def timed(fn, arith=capi.ARITH_DEFAULT, ang=capi.ANG_ARITH_DEFAULT):
    capi.set_arithmetic(arith); capi.set_ang_arithmetic(ang)
    try:
        for _ in range(5): fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    finally:
        capi.set_arithmetic(capi.ARITH_DEFAULT); capi.set_ang_arithmetic(capi.ANG_ARITH_DEFAULT)


median = lambda v: sorted(v)[len(v) // 2]
g = torch.Generator(device="cuda").manual_seed(3)
for hw in (32, 64):
    npix, n_img = hw * hw, B * A * A
    M = n_img * npix
    x, y = torch.randn(M, 64, device="cuda", generator=g), torch.empty(M, 64, device="cuda")
    wp = capi.pack_conv_weight(torch.randn(64, 64, 3, 3, device="cuda", generator=g) * 0.05)
    bias, in_bias = torch.randn(64, device="cuda", generator=g) * 0.1, torch.rand(64, device="cuda", generator=g)
    ang = lambda: capi.angconv3x3(x, wp, bias, B, A, npix, in_bias=in_bias, out=y)
    ops = (("angconv3x3", ang, capi.ANG_ARITH_DEFAULT), ("angconv3x3 bf16", ang, capi.ANG_ARITH_BF16),
           ("conv3x3", lambda: capi.conv3x3(x, wp, n_img, hw, hw, slope=1.0, out=y), capi.ANG_ARITH_DEFAULT),
           ("copy x -> y", lambda: y.copy_(x), capi.ANG_ARITH_DEFAULT))      # the same bytes through a streaming kernel: what the box delivers
    t = {name: [] for name, _, _ in ops}
    for _ in range(rounds):
        for name, fn, mode in ops: t[name].append(timed(fn, ang=mode))
    dense = 2.0 * 576 * 64 * M
    for name, _, _ in ops:
        v = sorted(t[name])
        med = median(v)
        work = dense * (EXECUTED if name.startswith("angconv3x3") else 1.0)
        if name.startswith("copy"):
            print(f"{name:15s} A={A} B={B} {hw}x{hw}: median {med:8.1f} us  min {v[0]:8.1f}  max {v[-1]:8.1f}  {2 * 256.0 * M / med * 1e-6:6.2f} TB/s read + written"
                  f"  ({rounds} x {reps} launches)", flush=True)
            continue
        print(f"{name:15s} A={A} B={B} {hw}x{hw}: median {med:8.1f} us  min {v[0]:8.1f}  max {v[-1]:8.1f}  dense {dense / med * 1e-6:6.1f} TFLOP/s"
              f"  executed multiply-adds {work / med * 1e-6:6.1f} TFLOP/s  {2 * 256.0 * M / med * 1e-6:6.2f} TB/s of x + y  ({rounds} x {reps} launches)", flush=True)
    a, b, c, d = (median(t[k]) for k in ("angconv3x3", "angconv3x3 bf16", "conv3x3", "copy x -> y"))
    print(f"at {hw}x{hw}: angconv3x3 / conv3x3 {a / c:.3f}; bf16 / conv3x3 {b / c:.3f}; default / bf16 {a / b:.2f}x; bf16 / copy of the same bytes {b / d:.2f}", flush=True)
    del x, y

if steps == 0: sys.exit(0)     # the operators only
sd = lfssr_state_dict(lfssr_spec(4))
rt = capi.LFSSRRuntime(A, 4)
rt.load_state([(k, torch.from_numpy(v).cuda()) for k, v in sd.items()], torch.device("cuda", 0))
xin = torch.from_numpy(synth_input((B, 1, A * 32, A * 32), seed=1)).cuda()
COMBOS = (("default", capi.ARITH_DEFAULT, capi.ANG_ARITH_DEFAULT), ("ANG_ARITH_BF16", capi.ARITH_DEFAULT, capi.ANG_ARITH_BF16),
          ("ARITH_BF16", capi.ARITH_BF16, capi.ANG_ARITH_DEFAULT), ("ANG_ARITH_BF16 + ARITH_BF16", capi.ARITH_BF16, capi.ANG_ARITH_BF16))
rates = {name: [] for name, _, _ in COMBOS}
prof = {}
try:
    for _ in range(3):
        for name, arith, ang_mode in COMBOS:
            capi.set_arithmetic(arith); capi.set_ang_arithmetic(ang_mode)
            for _ in range(3): rt.forward(xin)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps): rt.forward(xin)
            torch.cuda.synchronize()
            rates[name].append(B * steps / (time.perf_counter() - t0))
    for name, arith, ang_mode in COMBOS:
        capi.set_arithmetic(arith); capi.set_ang_arithmetic(ang_mode)
        capi.op_profile(True)
        rt.forward(xin)
        prof[name] = capi.op_profile_read()
        capi.op_profile(False)
finally:
    capi.set_arithmetic(capi.ARITH_DEFAULT); capi.set_ang_arithmetic(capi.ANG_ARITH_DEFAULT)
for name, _, _ in COMBOS:
    v = rates[name]
    print(f"LFSSR x4 forward, A=5, 32x32, B={B}, {name}: {sorted(v)[1]:.1f} patches/s (median of 3 x {steps} forwards; min {min(v):.1f}, max {max(v):.1f})", flush=True)
    for k, (ms, n) in sorted(prof[name].items(), key=lambda kv: -kv[1][0]): print(f"  op {k[0]:12s} ({k[1]}, {k[2]}): {ms:8.3f} ms over {n} launches (one forward, event-bracketed)")
