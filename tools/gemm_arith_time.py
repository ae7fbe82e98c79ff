#!/usr/bin/env python3
"""Times the transformer GEMMs under capi.GEMM_ARITH_DEFAULT and capi.GEMM_ARITH_BF16, both forms interleaved in this process: `rounds` timings per form, a
warm-up before every timing; median and max - min of each.  Operands from torch.randn (the bf16 matrix pipe holds another clock on zeros).
  * the three operators at the EPIT B = 8 geometry (M = 204 800 tokens) and the LFT 64-patch-scene geometry (M = 819 200): the out-projection (linear 128 -> 128 with
    a residual), LayerNorm + position encoding + q | k | v projection (128 -> 384) and the LayerNorm + feed-forward block (128 -> 256 -> 128, res = x); each with its
    byte floor (every fp32 operand read or written once) beside the rate a float4 copy of the same size class reaches in this process;
  * the EPIT (B = 8) and LFT (64 patches) x4 forwards through the plugin, eval / no_grad: default, the mode, and the mode together with capi.ARITH_BF16;
  * the rel-L2 distance of the gradient bucket of one EPIT and one LFT training step (B = 2) under the mode from the default's (recorded, not gated).
Writes the tables to profiles/gemm_bf16_time.md (or the path given with --out).
usage: python tools/gemm_arith_time.py [--reps 20] [--steps 5] [--rounds 7] [--out profiles/gemm_bf16_time.md]"""
import argparse, os, sys
from argparse import Namespace
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lfsr_amd import capi
from lfsr_amd.synth import synth_input, synth_state_dict
from lfsr_amd.model.SR import EPIT, LFT
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_bf16_time.md"))
a = ap.parse_args()
lib = capi.load()
P = capi.dev_ptr
GEMM = (("default", capi.GEMM_ARITH_DEFAULT), ("bf16", capi.GEMM_ARITH_BF16))
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


say("# bf16-operand transformer GEMMs (`lfsr_set_gemm_arithmetic(LFSR_GEMM_ARITH_BF16)`): measured times")
say()
say(f"`python tools/gemm_arith_time.py --reps {a.reps} --steps {a.steps} --rounds {a.rounds}` on {torch.cuda.get_device_name(0)}: fp32 tensors in HBM, `torch.randn` operands, HIP events around")
say(f"`reps` launches (`steps` forwards), a warm-up before every timing, the forms timed **interleaved in one process**, {a.rounds} timings each; spread = max - min.")
say()

# ---- operators ----
K, H = 128, 256
g = torch.Generator(device="cuda").manual_seed(5)
w_out = capi.pack_conv_weight(torch.randn(K, K, 1, 1, device="cuda", generator=g) * K ** -0.5)
w_in = capi.pack_conv_weight(torch.randn(3 * K, K, 1, 1, device="cuda", generator=g) * K ** -0.5)
w1 = capi.pack_conv_weight(torch.randn(H, K, 1, 1, device="cuda", generator=g) * K ** -0.5)
w2 = capi.pack_conv_weight(torch.randn(K, H, 1, 1, device="cuda", generator=g) * H ** -0.5)
gam, bet = torch.rand(K, device="cuda", generator=g) + 0.5, torch.randn(K, device="cuda", generator=g) * 0.1
pe = torch.randn(1024, K, device="cuda", generator=g)
say("## Operators (K = 128; us per call)")
say()
say("| operator | M | form | median | min | max | spread | byte floor at the copy rate | verdict |")
say("|---|---|---|---|---|---|---|---|---|")
for geom, M in (("EPIT B = 8", 8 * 25 * 32 * 32), ("LFT 64-patch scene", 32 * 25 * 32 * 32)):
    x = torch.randn(M, K, device="cuda", generator=g); r = torch.randn(M, K, device="cuda", generator=g)
    y = torch.empty(M, K, device="cuda"); qk = torch.empty(M, 2 * K, device="cuda"); v = torch.empty(M, K, device="cuda")
    src = torch.randn(M, 2 * K, device="cuda", generator=g)
    t_copy = sorted(timed(lambda: qk.copy_(src), a.reps) for _ in range(a.rounds))[a.rounds // 2]
    rate = 2 * src.numel() * 4 / (t_copy * 1e-3)          # bytes / s of a float4 copy (read + write)
    say(f"| float4 copy of {src.numel() * 4 / 1e6:.0f} MB | {M} | torch `copy_` | {t_copy * 1e3:.1f} | | | | {rate / 1e12:.2f} TB/s | |")
    ops = (("out-projection + residual (linear 128 -> 128)", 3 * M * K * 4,
            lambda: capi.check(lib.lfsr_linear_fwd(P(v), K, 0, K, P(w_out), None, P(x), K, 0, P(y), K, 0, M, K, 1.0, capi.stream_ptr()), "out")),
           ("LayerNorm + pe + q/k/v (128 -> 384)", 4 * M * K * 4,
            lambda: capi.check(lib.lfsr_linear_ln_fwd(P(x), K, 0, K, P(w_in), P(gam), P(bet), 1e-5, 2 * K, P(pe), K, 1024, 1, P(qk), 2 * K, 0, P(v), K, 0, 2 * K, M, 3 * K,
                                                      capi.stream_ptr()), "ln")),
           ("LayerNorm + feed-forward (128 -> 256 -> 128, res = x)", 3 * M * K * 4,
            lambda: capi.check(lib.lfsr_ffn_ln_fwd(P(x), K, 0, P(gam), P(bet), 1e-5, P(w1), P(w2), P(x), K, 0, P(y), K, 0, M, K, H, K, 0.0, capi.stream_ptr()), "ffn")))
    v.copy_(r)
    for what, nbytes, f in ops:
        t = {name: [] for name, _ in GEMM}
        for _ in range(a.rounds):
            for name, mode in GEMM:
                capi.set_gemm_arithmetic(mode)
                for _ in range(3): f()
                t[name].append(timed(f, a.reps))
        restore()
        sd_, sb_ = stats(t["default"], 1e3), stats(t["bf16"], 1e3)
        ok = sd_[0] - sb_[0] > max(sd_[3], sb_[3])
        floor = nbytes / rate * 1e6
        say(f"| {what} | {M} ({geom}) | default (three-term) | {sd_[0]:.1f} | {sd_[1]:.1f} | {sd_[2]:.1f} | {sd_[3]:.1f} | {floor:.0f} us ({floor / sd_[0]:.2f} of its time) | |")
        say(f"| | | bf16 operands (`gemm_bf16.hip`) | {sb_[0]:.1f} | {sb_[1]:.1f} | {sb_[2]:.1f} | {sb_[3]:.1f} | {floor:.0f} us ({floor / sb_[0]:.2f} of its time) | "
            f"{'beats the default by more than either spread' if ok else 'DOES NOT beat the default by more than the spread'} |")
    del x, r, y, qk, v, src
say()

# ---- forwards through the plugin ----
A, S, h, w = 5, 4, 32, 32
MODES = (("default", capi.ARITH_DEFAULT, capi.GEMM_ARITH_DEFAULT), ("`GEMM_ARITH_BF16`", capi.ARITH_DEFAULT, capi.GEMM_ARITH_BF16),
         ("`ARITH_BF16`", capi.ARITH_BF16, capi.GEMM_ARITH_DEFAULT), ("`GEMM_ARITH_BF16` + `ARITH_BF16`", capi.ARITH_BF16, capi.GEMM_ARITH_BF16))


def build(mod):
    net = mod.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=S)).cuda()
    sd = synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], 0)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net


say("## x4 forwards through the plugin, 5x5 views of 32x32 (eval, no_grad; ms per forward)")
say()
say("| model | arithmetic | median | min | max | spread | rms of (output - default's) |")
say("|---|---|---|---|---|---|---|")
nets = {}
for name, mod, B in (("EPIT, B = 8", EPIT, 8), ("LFT, 64 patches", LFT, 64)):
    net = nets[name] = build(mod)
    net.eval()
    x = torch.from_numpy(synth_input((B, 1, A * h, A * w), seed=1)).cuda()
    t, out = {m[0]: [] for m in MODES}, {}
    with torch.no_grad():
        for _ in range(a.rounds):
            for mname, am, gm in MODES:
                capi.set_arithmetic(am); capi.set_gemm_arithmetic(gm)
                for _ in range(2): y = net(x)
                t[mname].append(timed(lambda: net(x), a.steps))
                out[mname] = y.clone()
    restore()
    for mname, _, _ in MODES:
        s_ = stats(t[mname], 1.0)
        d = (out[mname] - out["default"]).double()
        say(f"| {name} | {mname} | {s_[0]:.3f} | {s_[1]:.3f} | {s_[2]:.3f} | {s_[3]:.3f} | {float(d.pow(2).mean().sqrt()):.2e} |")
    del x, out
say()

# ---- one training step: how far the gradient bucket moves (recorded, not gated) ----
say("## Gradient bucket of one training step (B = 2, L1 loss) under the mode against the default's")
say()
for name, net in nets.items():
    net.train()
    x = torch.from_numpy(synth_input((2, 1, A * h, A * w), seed=1)).cuda()
    label = torch.from_numpy(synth_input((2, 1, A * h * S, A * w * S), seed=2)).cuda()
    bucket = {}
    for mname, mode in GEMM:
        capi.set_gemm_arithmetic(mode)
        for p_ in net.parameters(): p_.grad = None
        torch.nn.functional.l1_loss(net(x), label).backward()
        torch.cuda.synchronize()
        bucket[mname] = net.grad_bucket.double().clone()
    restore()
    say(f"* {name.split(',')[0]}: rel-L2 {float((bucket['bf16'] - bucket['default']).norm() / bucket['default'].norm()):.3e}")
with open(a.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
