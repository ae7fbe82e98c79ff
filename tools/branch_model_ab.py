#!/usr/bin/env python3
"""Bit comparison of two builds on whole DistgSSR models, one process per library (the model-level companion of tools/branch_ab.py).
  LFSR_HIP_LIB=/path/to/ref/liblfsr_hip.so python tools/branch_model_ab.py dump ref      # the library LFSR_HIP_LIB names
  python tools/branch_model_ab.py dump new                                               # the tree's library
  python tools/branch_model_ab.py cmp ref new
dump: the small DistgSSR golden cases of tests/golden/models.json through the plugin -- a no-grad forward (lfsr_distgssr_forward), then a training step
(forward_train, L1 against synth_input(seed=2), backward) -- under the default, LFSR_DISTG_TAIL=0, lfsr_set_branch_arithmetic(BF16) and lfsr_set_arithmetic(F32);
a5h8s4 also on two patches (3200 view pixels), where the inference forward takes the fused block tail.  Writes results/branch_model_TAG.pt.
cmp: torch.equal on the int32 view of every inference output, training-forward output and gradient bucket."""
import os, sys
os.environ["LFSR_LAB"] = "1"       # LFSR_DISTG_TAIL is read only under LFSR_LAB
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

CASES = [("a5h8s4", 1), ("a3h6w8s2", 1), ("a5h8s4", 2)]       # (golden case, copies of its input along the batch)
MODES = ["default", "LFSR_DISTG_TAIL=0", "branch_bf16", "arith_f32"]
OUT = os.path.join(ROOT, "results")


def dump(tag):
    from lfsr_amd import capi
    from lfsr_amd.synth import synth_input
    from tests.helpers import model_case
    from tests.test_gpu_distgssr_train import load_plugin, build
    M, out = load_plugin(), {}
    for case_tag, mult in CASES:
        case, sd, x, _ = model_case("DistgSSR", case_tag)
        A, s = case["A"], case["s"]
        if mult > 1:
            x = np.concatenate([x] + [0.5 * x[:, :, ::-1].copy()] * (mult - 1), 0)
        xa = torch.from_numpy(x).cuda()
        label = torch.from_numpy(synth_input((xa.shape[0], 1, xa.shape[2] * s, xa.shape[3] * s), seed=2)).cuda()
        for mode in MODES:
            os.environ.pop("LFSR_DISTG_TAIL", None)
            capi.set_arithmetic(capi.ARITH_F32 if mode == "arith_f32" else capi.ARITH_DEFAULT)
            capi.set_branch_arithmetic(capi.BRANCH_ARITH_BF16 if mode == "branch_bf16" else capi.BRANCH_ARITH_DEFAULT)
            if mode == "LFSR_DISTG_TAIL=0":
                os.environ["LFSR_DISTG_TAIL"] = "0"
            net = build(M, A, s, sd)
            with torch.no_grad():
                y_inf = net(xa, None).clone()
            y_tr = net(xa, None)
            torch.nn.functional.l1_loss(y_tr, label).backward()
            torch.cuda.synchronize()
            out[f"{case_tag} B={xa.shape[0]} {mode}"] = (y_inf.cpu(), y_tr.detach().cpu(), net.grad_bucket.detach().cpu().clone())
    capi.set_arithmetic(capi.ARITH_DEFAULT); capi.set_branch_arithmetic(capi.BRANCH_ARITH_DEFAULT)
    os.makedirs(OUT, exist_ok=True)
    torch.save(out, os.path.join(OUT, f"branch_model_{tag}.pt"))
    print(f"{tag}: {len(out)} rows from {capi.LIB_PATH}")


def cmp(ta, tb):
    a, b = (torch.load(os.path.join(OUT, f"branch_model_{t}.pt")) for t in (ta, tb))
    eq = lambda p, q: p.shape == q.shape and torch.equal(p.view(torch.int32), q.view(torch.int32))
    bad = 0
    print(f"| case | selection | inference output | training-forward output | gradient bucket |   ({ta} vs {tb})\n|---|---|---|---|---|")
    for k in a:
        r = [eq(p, q) for p, q in zip(a[k], b[k])]
        bad += r.count(False)
        case, sel = k.rsplit(" ", 1)
        print(f"| {case} | {sel} | " + " | ".join(f"{'equal' if ok else 'DIFFERS'} ({p.numel()})" for ok, p in zip(r, a[k])) + " |")
    for case in sorted({k.rsplit(" ", 1)[0] for k in a}):      # that the selections reached something, within one library
        d = {m: a[f"{case} {m}"][0] for m in MODES}
        print("#", case, "inference vs default:", {m: "same bits" if torch.equal(d[m], d["default"]) else "max|d| %.2e" % float((d[m] - d["default"]).abs().max()) for m in MODES[1:]})
    print("ALL EQUAL" if not bad else f"{bad} DIFFERENCES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else cmp(sys.argv[2], sys.argv[3]))
