#!/usr/bin/env python3
"""Times EPIConv.0's gradients under capi.BRANCH_GRAD_ARITH_DEFAULT and capi.BRANCH_GRAD_ARITH_BF16, both forms interleaved in this process: `rounds` timings per
form, a warm-up before every timing; median, min, max and max - min of each.
  * the operator lfsr_epiconv_hv_bwd (capi.epiconv_hv_bwd: packs, stage 2, both data-gradient passes, the merged weight gradient and its reduction) at a batch of
    5x5 views of 32x32;
  * the two kernels alone, through the library's operator hooks (capi.op_profile: a hipEvent pair around each launch inside that operator, one stream): the data
    gradient (two launches per call) and the merged weight gradient (one);
  * the DistgSSR x4 training step (forward, L1 loss, backward) through the plugin at the same batch, under the four combinations of the 3x3 convs' gradient
    arithmetic (capi.GRAD_ARITH_DEFAULT / GRAD_ARITH_BF16) and this switch, and, from one hooked step of each combination, the in-step time per launch of the
    three EPIConv.0 launches and of AngConv.0's data gradient (which shares the chip with the weight gradient in the two-stream order).
usage: python tools/branch_grad_arith_time.py [batch] [reps] [steps] [rounds]"""
import importlib, json, os, sys
from argparse import Namespace
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lfsr_amd import capi
from lfsr_amd.synth import synth_input, synth_state_dict
B = int(sys.argv[1]) if len(sys.argv) > 1 else 8
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 7
capi.load()
MODES = (("default", capi.BRANCH_GRAD_ARITH_DEFAULT), ("bf16", capi.BRANCH_GRAD_ARITH_BF16))
A, h, w = 5, 32, 32


def timed(f, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def report(what, t, unit, scale):
    for name, v in t.items():
        v = sorted(x * scale for x in v)
        print(f"{what} {name:28s}: median {v[len(v) // 2]:8.2f} {unit}  min {v[0]:8.2f}  max {v[-1]:8.2f}  spread {v[-1] - v[0]:6.2f}  ({rounds} rounds)", flush=True)


def hooked(f, n, ops):
    """mean ms per launch of the hooked operators `ops` over n calls of f"""
    capi.op_profile(True)
    for _ in range(n): f()
    torch.cuda.synchronize()
    prof = capi.op_profile_read()
    capi.op_profile(False)
    out = {}
    for (op, _, _), (ms, launches) in prof.items():
        if op in ops:
            tot, cnt = out.get(op, (0.0, 0))
            out[op] = (tot + ms, cnt + launches)
    return {op: tot / max(cnt, 1) for op, (tot, cnt) in out.items()}


# ---- the operator and its two kernels: random operands (the bf16 pipe holds another clock on zeros) ----
g = torch.Generator(device="cuda").manual_seed(3)
npix, nepi = B * A * A * h * w, B * A * h * w
x = torch.randn(npix, 64, device="cuda", generator=g)
dy = torch.randn(npix, 64, device="cuda", generator=g)
eh, ev = torch.randn(nepi, 32, device="cuda", generator=g), torch.randn(nepi, 32, device="cuda", generator=g)
w0 = torch.randn(32, 64, 1, A * A, device="cuda", generator=g) * 0.025
w2 = torch.randn(32 * A, 32, 1, 1, device="cuda", generator=g) * 0.18
dx = torch.zeros(npix, 64, device="cuda")
op = lambda: capi.epiconv_hv_bwd(dy, 0, 32, None, 0, 32, x, eh, ev, w0, w2, dx, B, A, h, w)
KERNELS = ("epi0_dgrad", "epi0_wgrad")
t = {name: [] for name, _ in MODES}
tk = {f"{k} {name}": [] for k in KERNELS for name, _ in MODES}
for _ in range(rounds):
    for name, mode in MODES:
        capi.set_branch_grad_arithmetic(mode)
        for _ in range(5): op()
        t[name].append(timed(op, reps))
        for k, v in hooked(op, reps, KERNELS).items(): tk[f"{k} {name}"].append(v)
capi.set_branch_grad_arithmetic(capi.BRANCH_GRAD_ARITH_DEFAULT)
report(f"B={B} {A}x{A} x {h}x{w} epiconv_hv_bwd", t, "us", 1e3)
report(f"B={B} {A}x{A} x {h}x{w} kernel alone, per launch:", tk, "us", 1e3)
del x, dy, eh, ev, dx
torch.cuda.empty_cache()

# ---- the DistgSSR x4 training step through the plugin ----
S = 4
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


COMBOS = [(f"grad {gn} / branch grad {bn}", gm, bm) for gn, gm in (("default", capi.GRAD_ARITH_DEFAULT), ("bf16", capi.GRAD_ARITH_BF16)) for bn, bm in MODES]
INSTEP = ("epi0_dgrad", "epi0_wgrad", "ang0_dgrad")
t, bucket = {name: [] for name, _, _ in COMBOS}, {}
ti = {f"{k} {name}": [] for name, _, _ in COMBOS for k in INSTEP}
for _ in range(rounds):
    for name, gm, bm in COMBOS:
        capi.set_grad_arithmetic(gm); capi.set_branch_grad_arithmetic(bm)
        for _ in range(2): step()
        t[name].append(timed(step, steps))
        for k, v in hooked(step, 1, INSTEP).items(): ti[f"{k} {name}"].append(v)
        for p in net.parameters(): p.grad = None
        step(); torch.cuda.synchronize()
        bucket[name] = net.grad_bucket.double().clone()
capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT); capi.set_branch_grad_arithmetic(capi.BRANCH_GRAD_ARITH_DEFAULT)
report(f"DistgSSR x4 train step B={B}", t, "ms", 1.0)
report(f"DistgSSR x4 train step B={B}, in-step per launch (hooked step):", ti, "us", 1e3)
ref = bucket[COMBOS[0][0]]
for name, _, _ in COMBOS[1:]:
    print(f"gradient bucket, {name} against {COMBOS[0][0]}: rel-L2 {float((bucket[name] - ref).norm() / ref.norm()):.3e}")
