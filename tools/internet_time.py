#!/usr/bin/env python3
"""Times lfsr_conv3x3_wide_fwd (LF_InterNet's SpaConvSq 128 -> 64 and SpaBottle 320 -> 64, each with its residual, ReLU) in both of its arithmetics (default: the
gather-GEMM on the fp32 MFMA pipe; lfsr_set_wide_arithmetic(LFSR_WIDE_ARITH_BF16)) beside lfsr_conv3x3_fwd (the 64 -> 64 per-view conv in the default arithmetic on
tensors of the same pixel count) and a copy of the bytes the operator has to move, at angRes 5, B = 8, views of 32x32 and 64x64, interleaved in this process
(`rounds` timings of `reps` launches each, a warm-up before every timing, random operands).  Then the whole LF_InterNet x2 forward at B = 8 on 32x32 views through
ModelRuntime.forward in the default mode and under the switch, interleaved as well.  Device events around launches that end in a synchronise.
The operands are the model's: cin 128 reads rows of 128 whose first 64 channels are the residual and writes channels 0..63 of other rows of 128; cin 320 reads
rows of 320, a residual in rows of 64, and writes rows of 64.
usage: python tools/internet_time.py [reps] [rounds] [steps]"""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lfsr_amd import capi
from lfsr_amd.synth import synth_input, synth_state_dict
from tests.helpers import internet_spec
capi.load()
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 30
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
A, B = 5, 8


def restore():
    capi.set_arithmetic(capi.ARITH_DEFAULT); capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT); capi.set_gemm_arithmetic(capi.GEMM_ARITH_DEFAULT)
    capi.set_branch_arithmetic(capi.BRANCH_ARITH_DEFAULT); capi.set_ang_arithmetic(capi.ANG_ARITH_DEFAULT); capi.set_wide_arithmetic(capi.WIDE_ARITH_DEFAULT)


def timed(fn, wide=capi.WIDE_ARITH_DEFAULT):
    capi.set_wide_arithmetic(wide)
    try:
        for _ in range(5): fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps
    finally:
        restore()


median = lambda v: sorted(v)[len(v) // 2]
g = torch.Generator(device="cuda").manual_seed(3)
for hw in (32, 64):
    n_img = B * A * A
    M = n_img * hw * hw
    x64, y64 = torch.randn(M, 64, device="cuda", generator=g), torch.empty(M, 64, device="cuda")
    w64 = capi.pack_conv_weight(torch.randn(64, 64, 3, 3, device="cuda", generator=g) * 0.05)
    for cin in (128, 320):
        x = torch.randn(M, cin, device="cuda", generator=g)
        wp = capi.pack_conv_weight(torch.randn(64, cin, 3, 3, device="cuda", generator=g) * 0.03)
        if cin == 128:
            y, res, moved = torch.empty(M, 128, device="cuda"), x, 128 + 64                 # floats per pixel: x read (the residual is part of it), y written
        else:
            y, res, moved = torch.empty(M, 64, device="cuda"), torch.randn(M, 64, device="cuda", generator=g), 320 + 64 + 64
        ca, cb = torch.randn(M, moved // 2, device="cuda", generator=g), torch.empty(M, moved // 2, device="cuda")   # a copy reads and writes moved / 2 each
        wide = lambda: capi.conv3x3_wide(x, cin, wp, n_img, hw, hw, slope=0.0, res1=res, out=y)
        ops = ((f"wide {cin} default", wide, capi.WIDE_ARITH_DEFAULT), (f"wide {cin} bf16", wide, capi.WIDE_ARITH_BF16),
               ("conv3x3 64", lambda: capi.conv3x3(x64, w64, n_img, hw, hw, slope=0.0, res1=x64, out=y64), capi.WIDE_ARITH_DEFAULT),
               ("copy", lambda: cb.copy_(ca), capi.WIDE_ARITH_DEFAULT))
        t = {name: [] for name, _, _ in ops}
        for _ in range(rounds):
            for name, fn, mode in ops: t[name].append(timed(fn, mode))
        for name, _, _ in ops:
            v = sorted(t[name])
            med = median(v)
            k = 64 if name.startswith("conv3x3") else cin
            tail = f"{4.0 * moved * M / med * 1e-6:6.2f} TB/s read + written" if name == "copy" else f"dense {2.0 * 9 * k * 64 * M / med * 1e-6:6.1f} TFLOP/s"
            print(f"{name:17s} A={A} B={B} {hw}x{hw}: median {med:8.1f} us  min {v[0]:8.1f}  max {v[-1]:8.1f}  {tail}  ({rounds} x {reps} launches)", flush=True)
        a, b, c, d = (median(t[k]) for k in (f"wide {cin} default", f"wide {cin} bf16", "conv3x3 64", "copy"))
        print(f"at {hw}x{hw}, cin {cin}: default / bf16 {a / b:.2f}x; bf16 / conv3x3 64 {b / c:.2f}; bf16 / copy of its {4 * moved * M / 1e6:.1f} MB {b / d:.2f}", flush=True)
        del x, y, res, ca, cb
    del x64, y64

if steps == 0: sys.exit(0)     # the operators only
sd = synth_state_dict(internet_spec(A, 2), seed=0)
rt = capi.ModelRuntime("internet", A, 2, 4, 4)
rt.load_state([(k, torch.from_numpy(v).cuda()) for k, v in sd.items()], torch.device("cuda", 0))
xin = torch.from_numpy(synth_input((B, 1, A * 32, A * 32), seed=1)).cuda()
COMBOS = (("default", capi.WIDE_ARITH_DEFAULT, capi.GEMM_ARITH_DEFAULT), ("WIDE_ARITH_BF16", capi.WIDE_ARITH_BF16, capi.GEMM_ARITH_DEFAULT),
          ("WIDE_ARITH_BF16 + GEMM_ARITH_BF16", capi.WIDE_ARITH_BF16, capi.GEMM_ARITH_BF16))
ms = {name: [] for name, _, _ in COMBOS}
try:
    for _ in range(3):
        for name, wide_mode, gemm in COMBOS:
            capi.set_wide_arithmetic(wide_mode); capi.set_gemm_arithmetic(gemm)
            for _ in range(3): rt.forward(xin)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps): rt.forward(xin)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3 / steps)
finally:
    restore()
for name, _, _ in COMBOS:
    v = sorted(ms[name])
    print(f"LF_InterNet x2 forward, A=5, 32x32, B={B}, {name}: {v[1]:.3f} ms per forward = {B / v[1] * 1e3:.1f} patches/s (median of 3 x {steps} forwards; "
          f"min {v[0]:.3f} ms, max {v[-1]:.3f} ms)", flush=True)
