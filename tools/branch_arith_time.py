#!/usr/bin/env python3
"""Times DistgSSR's EPI branch and block tail under capi.BRANCH_ARITH_DEFAULT and capi.BRANCH_ARITH_BF16, both forms interleaved in this process: `rounds` timings
per form, a warm-up before every timing; median and max - min of each.  Operands from torch.randn (the bf16 matrix pipe holds another clock on zeros).
  * the three launches of a block tail (stage 1 of the angular branch, stage 1 of both EPI passes, the fused tail) at (B, h, w) = (32, 32, 32) and (8, 32, 32), PER
    KERNEL: the model driver's own per-class event pairs (capi.DistgSSRRuntime.profile: classes angconv / epiconv / pointwise are exactly these three launches on
    the fused-tail path) around every launch of a x4 forward on a torch.randn input, divided by the launches; and the operator capi.distg_branch_tail (the three
    launches together) on torch.randn x / spa.  Each kernel with its byte floor (every fp32 operand read or written once) at the rate a float4 copy of the same size
    class reaches in this process, and the acceptance rule of DESIGN.md section 6g: wired only if it beats the default form of the same run by more than either
    form's spread at both geometries;
  * the DistgSSR x4 forward through the plugin at B = 32 (eval, no_grad): default, the mode, capi.ARITH_BF16, and both.
Writes the tables to profiles/branch_bf16_time.md (or the path given with --out).
usage: python tools/branch_arith_time.py [--reps 20] [--steps 5] [--rounds 7] [--out profiles/branch_bf16_time.md]"""
import argparse, os, sys
from argparse import Namespace
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lfsr_amd import capi
from lfsr_amd.synth import synth_state_dict
from lfsr_amd.model.SR import DistgSSR
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "branch_bf16_time.md"))
a = ap.parse_args()
BRANCH = (("default", capi.BRANCH_ARITH_DEFAULT), ("bf16", capi.BRANCH_ARITH_BF16))
A, S, h, w, L = 5, 4, 32, 32, 0.1
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def timed(f, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def stats(v, scale):
    v = sorted(x * scale for x in v)
    return v[len(v) // 2], v[0], v[-1], v[-1] - v[0]


def restore():
    capi.set_arithmetic(capi.ARITH_DEFAULT); capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT); capi.set_gemm_arithmetic(capi.GEMM_ARITH_DEFAULT)
    capi.set_branch_arithmetic(capi.BRANCH_ARITH_DEFAULT)


say("# bf16-operand EPI branch and block tail of DistgSSR (`lfsr_set_branch_arithmetic(LFSR_BRANCH_ARITH_BF16)`): measured times")
say()
say(f"`python tools/branch_arith_time.py --reps {a.reps} --steps {a.steps} --rounds {a.rounds}` on {torch.cuda.get_device_name(0)}: fp32 tensors in HBM, `torch.randn` operands, HIP events around")
say(f"`reps` operator calls (`steps` forwards), a warm-up before every timing, the forms timed **interleaved in one process**, {a.rounds} timings each; spread = max - min.")
say()

net = DistgSSR.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=S)).cuda()
sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 0)
net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
net.eval()
rt = capi.DistgSSRRuntime(A, S)
rt.load_state([(k, torch.from_numpy(v).cuda()) for k, v in sd.items()], torch.device("cuda", 0))
g = torch.Generator(device="cuda").manual_seed(5)

# ---- the three launches of a block tail, per kernel ----
say("## The three launches of a block tail, per kernel (us per launch: the driver's event pairs around each of the 16 blocks' launches in a x4 forward)")
say()
say("| kernel | (B, h, w) | form | median | min | max | spread | byte floor at the copy rate | verdict |")
say("|---|---|---|---|---|---|---|---|---|")
KERNELS = (("angconv", "stage 1 of the angular branch (`k_ang_fused<false>`: not in the mode)", lambda B: B * 1024 * (25 * 64 + 16) * 4),
           ("epiconv", "stage 1 of both EPI passes (`k_epi_b3<false>` / `k_epi_bf16`)", lambda B: B * 1024 * (2 * 25 * 64 + 2 * 5 * 32) * 4),
           ("pointwise", "block tail (`k_distg_tail` / `k_distg_tail_bf16`)", lambda B: B * 1024 * (2 * 25 * 64 + 2 * 5 * 32 + 16) * 4))
wins = {k: [] for k, _, _ in KERNELS}
op_rows = []
for B in (32, 8):
    npix = B * A * A * h * w
    src = torch.randn(npix, 72, device="cuda", generator=g); dst = torch.empty_like(src)      # read + write = the tail's bytes
    t_copy = sorted(timed(lambda: dst.copy_(src), a.reps) for _ in range(a.rounds))[a.rounds // 2]
    rate = 2 * src.numel() * 4 / (t_copy * 1e-3)          # bytes / s of a float4 copy (read + write)
    say(f"| float4 copy of {2 * src.numel() * 4 / 1e6:.0f} MB (read + write) | ({B}, {h}, {w}) | torch `copy_` | {t_copy * 1e3:.1f} | | | | {rate / 1e12:.2f} TB/s | |")
    del src, dst
    x = torch.randn(B, 1, A * h, A * w, device="cuda", generator=g)
    t = {k: {name: [] for name, _ in BRANCH} for k, _, _ in KERNELS}
    for _ in range(a.rounds):
        for name, mode in BRANCH:
            capi.set_branch_arithmetic(mode)
            for _ in range(2): rt.forward(x)
            rt.profile(1)
            for _ in range(a.steps): rt.forward(x)
            rec = rt.profile_read()
            rt.profile(0)
            for k, _, _ in KERNELS:
                t[k][name].append(rec[k][0] / rec[k][1])
    restore()
    for k, what, nbytes in KERNELS:
        sd_, sb_ = stats(t[k]["default"], 1e3), stats(t[k]["bf16"], 1e3)
        ok = sd_[0] - sb_[0] > max(sd_[3], sb_[3])
        wins[k].append(ok)
        floor = nbytes(B) / rate * 1e6
        say(f"| {what} | ({B}, {h}, {w}) | default | {sd_[0]:.1f} | {sd_[1]:.1f} | {sd_[2]:.1f} | {sd_[3]:.1f} | {floor:.0f} us of {nbytes(B) / 1e6:.0f} MB ({floor / sd_[0]:.2f} of its time) | |")
        say(f"| | | `BRANCH_ARITH_BF16` | {sb_[0]:.1f} | {sb_[1]:.1f} | {sb_[2]:.1f} | {sb_[3]:.1f} | {floor:.0f} us ({floor / sb_[0]:.2f} of its time) | "
            f"{'beats the default by more than either spread' if ok else 'does not beat the default by more than the spread'} |")
    # the operator: the three launches together, torch.randn x / spa
    xr = torch.randn(npix, 64, device="cuda", generator=g)
    spa = torch.nn.functional.leaky_relu(torch.randn(npix, 64, device="cuda", generator=g), L)
    p = "disentg.Group.0.Block.0."
    wd = {k: torch.from_numpy(v).cuda() for k, v in sd.items() if k.startswith(p)}
    wp = (capi.pack_conv_weight(wd[p + "AngConv.0.weight"]), capi.pack_conv_weight(wd[p + "AngConv.2.weight"], perm=1, ch=16),
          capi.pack_conv_weight(wd[p + "EPIConv.0.weight"]), capi.pack_conv_weight(wd[p + "EPIConv.2.weight"]), capi.pack_conv_weight(wd[p + "fuse.0.weight"]))
    outs = (torch.empty(npix, 64, device="cuda"), torch.empty(B * h * w, 16, device="cuda"), torch.empty(B * A * h * w, 32, device="cuda"),
            torch.empty(B * A * h * w, 32, device="cuda"))
    f = lambda: capi.distg_branch_tail(xr, spa, *wp, B, A, h, w, L, out=outs)
    to = {name: [] for name, _ in BRANCH}
    for _ in range(a.rounds):
        for name, mode in BRANCH:
            capi.set_branch_arithmetic(mode)
            for _ in range(3): f()
            to[name].append(timed(f, a.reps))
    restore()
    for name, _ in BRANCH:
        s_ = stats(to[name], 1e3)
        op_rows.append(f"| ({B}, {h}, {w}) | {name} | {s_[0]:.1f} | {s_[1]:.1f} | {s_[2]:.1f} | {s_[3]:.1f} |")
    del x, xr, spa, outs
say()
for k, what, _ in KERNELS[1:]:
    say(f"* {what}: {'meets the acceptance rule at both geometries: wired' if all(wins[k]) else 'DOES NOT meet the acceptance rule at both geometries'}.")
say()
say("## The operator `lfsr_distg_branch_tail_fwd` (the three launches together; us per call, `torch.randn` x and spa)")
say()
say("| (B, h, w) | form | median | min | max | spread |")
say("|---|---|---|---|---|---|")
for row in op_rows: say(row)
say()

# ---- the forward through the plugin ----
MODES = (("default", capi.ARITH_DEFAULT, capi.BRANCH_ARITH_DEFAULT), ("`BRANCH_ARITH_BF16`", capi.ARITH_DEFAULT, capi.BRANCH_ARITH_BF16),
         ("`ARITH_BF16`", capi.ARITH_BF16, capi.BRANCH_ARITH_DEFAULT), ("`BRANCH_ARITH_BF16` + `ARITH_BF16`", capi.ARITH_BF16, capi.BRANCH_ARITH_BF16))
say("## DistgSSR x4 forward through the plugin, B = 32, 5x5 views of 32x32 (eval, no_grad; ms per forward)")
say()
say("| arithmetic | median | min | max | spread | rms of (output - default's) |")
say("|---|---|---|---|---|---|")
x = torch.randn(32, 1, A * h, A * w, device="cuda", generator=g)
t, out = {m[0]: [] for m in MODES}, {}
with torch.no_grad():
    for _ in range(a.rounds):
        for mname, am, bm in MODES:
            capi.set_arithmetic(am); capi.set_branch_arithmetic(bm)
            for _ in range(2): y = net(x)
            t[mname].append(timed(lambda: net(x), a.steps))
            out[mname] = y.clone()
restore()
for mname, _, _ in MODES:
    s_ = stats(t[mname], 1.0)
    d = (out[mname] - out["default"]).double()
    say(f"| {mname} | {s_[0]:.3f} | {s_[1]:.3f} | {s_[2]:.3f} | {s_[3]:.3f} | {float(d.pow(2).mean().sqrt()):.2e} |")
with open(a.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
