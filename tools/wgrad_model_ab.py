#!/usr/bin/env python3
"""Bit comparison of two builds on the training step of the four trainable models, one process per library (the model-level companion of tools/wgrad_ab.py).
  LFSR_HIP_LIB=/path/to/ref/liblfsr_hip.so python tools/wgrad_model_ab.py dump ref      # the library LFSR_HIP_LIB names
  python tools/wgrad_model_ab.py dump new                                               # the tree's library
  python tools/wgrad_model_ab.py cmp ref new
dump: rows of the geometry matrix of tests/modes_refs.py (the inputs and weights of the whole-model tests) through the plugins -- forward_train, L1 against the row's
label, backward (lfsr_distgssr_backward, lfsr_internet_backward, lfsr_lft_backward, lfsr_epit_backward) -- under the default, every lab selector of the weight
gradients and each gradient arithmetic that reaches the model.  Writes results/wgrad_model_TAG.pt.
cmp: torch.equal on the int32 view of every training-forward output and gradient bucket."""
import os, sys
os.environ["LFSR_LAB"] = "1"       # the selectors are read only under LFSR_LAB
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

ROWS = {"DistgSSR": ((5, 3, 2, 13, 16), (5, 2, 1, 33, 6), (3, 3, 1, 13, 16), (7, 2, 1, 5, 6)),      # merged EPI lines; lines of 33: declined; A = 3, A = 7: gather
        "LF_InterNet": ((7, 2, 1, 5, 6), (2, 3, 2, 9, 7)), "EPIT": ((2, 3, 2, 9, 7), (1, 2, 2, 8, 8)), "LFT": ((2, 3, 2, 9, 7), (1, 2, 2, 8, 8))}
SELECTORS = ("LFSR_WGRAD3", "LFSR_WGRAD_EPI", "LFSR_WGRAD_PW", "LFSR_BWD_OVERLAP")
# selection -> (environment, capi setter, its value); per model what can reach it
MODES = {"default": ({}, None, 0), "LFSR_WGRAD3=direct": ({"LFSR_WGRAD3": "direct"}, None, 0), "LFSR_WGRAD_EPI=gather": ({"LFSR_WGRAD_EPI": "gather"}, None, 0),
         "LFSR_WGRAD_PW=gather": ({"LFSR_WGRAD_PW": "gather"}, None, 0), "LFSR_BWD_OVERLAP=0": ({"LFSR_BWD_OVERLAP": "0"}, None, 0),
         "grad_bf16": ({}, "set_grad_arithmetic", 1), "grad_bf16 LFSR_WGRAD3=direct": ({"LFSR_WGRAD3": "direct"}, "set_grad_arithmetic", 1),
         "lin_grad_bf16": ({}, "set_lin_grad_arithmetic", 1), "wide_train 1": ({}, "set_wide_train_arithmetic", 1), "wide_train 2": ({}, "set_wide_train_arithmetic", 2),
         "branch_grad_bf16": ({}, "set_branch_grad_arithmetic", 1)}
REACH = {"DistgSSR": ("default", "LFSR_WGRAD3=direct", "LFSR_WGRAD_EPI=gather", "LFSR_WGRAD_PW=gather", "LFSR_BWD_OVERLAP=0", "grad_bf16", "grad_bf16 LFSR_WGRAD3=direct",
                      "branch_grad_bf16"),
         "LF_InterNet": ("default", "wide_train 1", "wide_train 2", "grad_bf16"), "EPIT": ("default", "lin_grad_bf16", "grad_bf16"), "LFT": ("default", "lin_grad_bf16", "grad_bf16")}
OUT = os.path.join(ROOT, "results")


def dump(tag):
    from lfsr_amd import capi
    from tests.stream_helpers import case, make_net
    out = {}
    for model, rows in ROWS.items():
        for geom in rows:
            sd, x, label = case(model, geom)
            xg, lg = torch.from_numpy(x).cuda(), torch.from_numpy(label).cuda()
            for mode in REACH[model]:
                env, setter, value = MODES[mode]
                for k in SELECTORS:
                    os.environ.pop(k, None)
                os.environ.update(env)
                if setter:
                    getattr(capi, setter)(value)
                net = make_net(model, geom, sd)
                y = net(xg)
                torch.nn.functional.l1_loss(y, lg).backward()
                torch.cuda.synchronize()
                out[f"{model} {geom} | {mode}"] = (y.detach().cpu(), net.grad_bucket.detach().cpu().clone())
                if setter:
                    getattr(capi, setter)(0)
    for k in SELECTORS:
        os.environ.pop(k, None)
    os.makedirs(OUT, exist_ok=True)
    torch.save(out, os.path.join(OUT, f"wgrad_model_{tag}.pt"))
    print(f"{tag}: {len(out)} rows from {capi.LIB_PATH}")


def cmp(ta, tb):
    a, b = (torch.load(os.path.join(OUT, f"wgrad_model_{t}.pt")) for t in (ta, tb))
    eq = lambda p, q: p.shape == q.shape and torch.equal(p.view(torch.int32), q.view(torch.int32))
    bad = 0
    print(f"| model, (A, s, B, h, w) | selection | training-forward output | gradient bucket | bucket vs the default's |   ({ta} vs {tb})\n|---|---|---|---|---|")
    for k in a:
        r = [eq(p, q) for p, q in zip(a[k], b[k])]
        bad += r.count(False)
        case, sel = k.split(" | ")
        d = a[case + " | default"][1]      # that the selection reached something, within one library
        moved = "same bits" if torch.equal(a[k][1], d) else "max|d| %.2e" % float((a[k][1] - d).abs().max())
        print(f"| {case} | {sel} | " + " | ".join(f"{'equal' if ok else 'DIFFERS'} ({p.numel()})" for ok, p in zip(r, a[k])) + f" | {moved} |")
    print("ALL EQUAL" if not bad else f"{bad} DIFFERENCES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(dump(sys.argv[2]) if sys.argv[1] == "dump" else cmp(sys.argv[2], sys.argv[3]))
