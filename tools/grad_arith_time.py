#!/usr/bin/env python3
"""Times the gradients of the per-view 3x3 conv under capi.GRAD_ARITH_DEFAULT and capi.GRAD_ARITH_BF16, both forms interleaved in this process: `rounds`
timings per form, a warm-up before every timing; median and max - min of each.
  * the data-gradient operator (capi.conv3x3_dgrad) at 200 and 800 images of 32x32, plain and with the LeakyReLU mask + a residual;
  * the weight-gradient operator (capi.conv3x3_wgrad: the tile kernel plus the slab reduction) at the same two sizes;
  * the DistgSSR x4 training step (forward, L1 loss, backward) through the plugin at a batch of 5x5 views of 32x32, under the four combinations of forward
    (capi.ARITH_DEFAULT / ARITH_BF16) and gradient arithmetic.
usage: python tools/grad_arith_time.py [batch] [reps] [steps] [rounds]"""
import importlib, json, os, sys
from argparse import Namespace
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lfsr_amd import capi
from lfsr_amd.synth import synth_input, synth_state_dict
B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 7
capi.load()
GRADS = (("default", capi.GRAD_ARITH_DEFAULT), ("bf16", capi.GRAD_ARITH_BF16))


def timed(f, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def report(what, t, unit, scale):
    for name, v in t.items():
        v = sorted(x * scale for x in v)
        print(f"{what} {name:16s}: median {v[len(v) // 2]:8.2f} {unit}  min {v[0]:8.2f}  max {v[-1]:8.2f}  spread {v[-1] - v[0]:6.2f}  ({rounds} rounds)", flush=True)


# ---- operators: random operands (the bf16 pipe holds another clock on zeros) ----
h = w = 32
g = torch.Generator(device="cuda").manual_seed(3)
wt = torch.randn(64, 64, 3, 3, device="cuda", generator=g) * 0.05
wT = capi.pack_conv_weight_T(wt)
for n_img in (200, 800):
    M = n_img * h * w
    dy = torch.randn(M, 64, device="cuda", generator=g); x = torch.randn(M, 64, device="cuda", generator=g)
    dw = torch.empty(64, 64, 3, 3, device="cuda")
    ops = (("dgrad plain      ", lambda: capi.conv3x3_dgrad(dy, wT, n_img, h, w)),
           ("dgrad mask + res ", lambda: capi.conv3x3_dgrad(dy, wT, n_img, h, w, res1=x, act=x, act_slope=0.1)),
           ("wgrad + reduce   ", lambda: capi.conv3x3_wgrad(dy, x, n_img, h, w)))
    for what, f in ops:
        t = {name: [] for name, _ in GRADS}
        for _ in range(rounds):
            for name, mode in GRADS:
                capi.set_grad_arithmetic(mode)
                for _ in range(5): f()
                t[name].append(timed(f, reps))
        capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT)
        report(f"n_img={n_img} {what}", t, "us", 1e3)
    del dy, x

# ---- the DistgSSR x4 training step through the plugin ----
A, S = 5, 4
sys.path.insert(0, capi._HERE)
Mod = importlib.import_module("model.SR.DistgSSR")
sys.path.remove(capi._HERE)
meta = json.load(open(os.path.join(ROOT, "tests", "golden", "models.json")))["models"]["DistgSSR"]["full"]
sd = synth_state_dict([(k, tuple(s)) for k, s in meta["spec"]], seed=0)
net = Mod.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=S))
net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
net = net.cuda().train()
xin = torch.from_numpy(synth_input((B, 1, A * h, A * w), seed=1)).cuda()
label = torch.from_numpy(synth_input((B, 1, A * h * S, A * w * S), seed=2)).cuda()


def step():
    torch.nn.functional.l1_loss(net(xin, None), label).backward()


COMBOS = [(f"fwd {fn} / grad {gn}", fm, gm) for fn, fm in (("default", capi.ARITH_DEFAULT), ("bf16", capi.ARITH_BF16)) for gn, gm in GRADS]
t, bucket = {name: [] for name, _, _ in COMBOS}, {}
for _ in range(rounds):
    for name, fm, gm in COMBOS:
        capi.set_arithmetic(fm); capi.set_grad_arithmetic(gm)
        for _ in range(2): step()
        t[name].append(timed(step, steps))
        for p in net.parameters(): p.grad = None
        step(); torch.cuda.synchronize()
        bucket[name] = net.grad_bucket.double().clone()
capi.set_arithmetic(capi.ARITH_DEFAULT); capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT)
report(f"DistgSSR x4 train step B={B}", {k: v for k, v in t.items()}, "ms", 1.0)
ref = bucket[COMBOS[0][0]]
for name, _, _ in COMBOS[1:]:
    print(f"gradient bucket, {name} against {COMBOS[0][0]}: rel-L2 {float((bucket[name] - ref).norm() / ref.norm()):.3e}")
