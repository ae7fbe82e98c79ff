#!/usr/bin/env python3
"""Times the per-view 3x3 conv op alone at the bench geometry, one line per kernel selection (LFSR_CONV3X3 = '' | wino2 | halo) and one for the bf16-operand
arithmetic (capi.set_arithmetic(ARITH_BF16), nothing selected), with and without a residual operand, and prints the max difference against the direct kernel.
Then the F(4x4,3x3) kernel and the bf16-operand kernel interleaved in this process, `rounds` timings of `reps` launches each: median and max - min of each.
usage: python tools/conv_time.py [n_img] [reps] [rounds]"""
import os, sys
os.environ.setdefault("LFSR_LAB", "1")   # (this tool drives the library's A/B selectors, live only under LFSR_LAB)
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lfsr_amd import capi
if os.environ.get("LFSR_LIB"): capi.LIB_PATH = os.path.abspath(os.environ["LFSR_LIB"])   # a diagnostic build (tools/build_w4_abl.sh)
capi.load()
SELS = os.environ.get("CONV_SELS", ",wino2,halo").split(",")
n_img = int(sys.argv[1]) if len(sys.argv) > 1 else 800
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7
h = w = 32
M = n_img * h * w
g = torch.Generator(device="cuda").manual_seed(3)
x = torch.randn(M, 64, device="cuda", generator=g); r = torch.randn(M, 64, device="cuda", generator=g)
wp = capi.pack_conv_weight(torch.randn(64, 64, 3, 3, device="cuda", generator=g) * 0.05)
y = torch.empty(M, 64, device="cuda")
os.environ["LFSR_CONV3X3"] = "halo"
ref = capi.conv3x3(x, wp, n_img, h, w, slope=0.1, res1=r).clone()


def timed(res):
    """microseconds per launch over `reps` launches of the conv as currently selected"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(reps): capi.conv3x3(x, wp, n_img, h, w, slope=0.1, res1=res, out=y)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def line(name, res):
    for _ in range(5): capi.conv3x3(x, wp, n_img, h, w, slope=0.1, res1=res, out=y)
    us = timed(res)
    err = float((y - ref).abs().max()) if res is not None else float("nan")
    print(f"conv3x3 sel={name:6s} n_img={n_img} res={'y' if res is not None else 'n'}: {us:8.1f} us  {2*576*64*M/us*1e-6:7.1f} TFLOP/s(alg)  max|d vs direct| {err:.2e}", flush=True)


for sel in SELS:
    if sel: os.environ["LFSR_CONV3X3"] = sel
    else: os.environ.pop("LFSR_CONV3X3", None)
    for res in (None, r): line(sel or "wino4", res)
os.environ.pop("LFSR_CONV3X3", None)
capi.set_arithmetic(capi.ARITH_BF16)
for res in (None, r): line("bf16", res)
# the two product forms interleaved: same process, same operands (random: the bf16 pipe holds another clock on zeros), a warm-up before every timing
MODES = (("wino4", capi.ARITH_DEFAULT), ("bf16", capi.ARITH_BF16))
for res in (None, r):
    t = {name: [] for name, _ in MODES}
    for _ in range(rounds):
        for name, mode in MODES:
            capi.set_arithmetic(mode)
            for _ in range(5): capi.conv3x3(x, wp, n_img, h, w, slope=0.1, res1=res, out=y)
            t[name].append(timed(res))
    for name, _ in MODES:
        v = sorted(t[name])
        print(f"interleaved {name:6s} res={'y' if res is not None else 'n'}: median {v[len(v) // 2]:8.1f} us  min {v[0]:8.1f}  max {v[-1]:8.1f}  spread {v[-1] - v[0]:6.1f}  ({rounds} x {reps} launches)", flush=True)
capi.set_arithmetic(capi.ARITH_DEFAULT)
