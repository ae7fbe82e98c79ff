#!/usr/bin/env python3
"""Generate tests/golden/epit_grads.{npz,json}: EPIT forward + backward with the reference's own model on CPU, fp32 (train.py:256-264
without AMP), in the form of make_golden_lft_grads.py.  The loss is torch.nn.L1Loss()(out, label): the reference's own get_loss indexes
out['SR'] on a tensor (EPIT.py:178) and cannot be called.

Run in the build container only (the reference checkout does not exist on the GPU box):

    python tests/golden/make_golden_epit_grads.py

The reference module is loaded by file path (importing it as ``model.SR.EPIT`` could pick up this project's plugin of the same name).
Inputs are the ``model_case("EPIT", tag)`` weights and input (lfsr_amd.synth), label = synth_input(seed=2).
Per tag: the loss, per-parameter gradient norms and random projections (probe = default_rng([7, index]) normals), full gradients of
<= 2400 elements, and the parameter names in state_dict order."""
import importlib.util
import json
import os
import sys
from argparse import Namespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("LFSR_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import model_case  # noqa: E402

TAGS = ("a5h8s4", "a3h6w8s2", "a3h6w8s3")


def load_ref():
    spec = importlib.util.spec_from_file_location("ref_epit", os.path.join(REF, "model", "SR", "EPIT.py"))
    M = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(M)
    return M


def main():
    torch.set_num_threads(8)
    M = load_ref()
    arrs, meta = {}, {"tags": {}, "label_seed": 2, "probe": "np.random.default_rng([7, i]).standard_normal(shape)"}
    for tag in TAGS:
        case, sd, x, _ = model_case("EPIT", tag)
        A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
        from lfsr_amd.synth import synth_input
        net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        net.train()
        label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2))
        out = net(torch.from_numpy(x), None)
        loss = torch.nn.L1Loss()(out, label)
        loss.backward()
        arrs[f"{tag}::loss"] = np.float64(loss.item())
        names, norms, projs = [], [], []
        for i, (k, p) in enumerate(net.named_parameters()):
            g = p.grad.detach().numpy().astype(np.float64)
            probe = np.random.default_rng([7, i]).standard_normal(g.shape)
            names.append(k)
            norms.append(np.sqrt((g * g).sum()))
            projs.append((g * probe).sum())
            if g.size <= 2400:
                arrs[f"{tag}::grad::{k}"] = g.astype(np.float32)
        arrs[f"{tag}::norms"] = np.array(norms)
        arrs[f"{tag}::projs"] = np.array(projs)
        meta["tags"][tag] = dict(A=A, h=h, w=w, s=s, B=B, names=names)
        print(tag, "loss", loss.item(), "params", len(names))
    np.savez_compressed(os.path.join(HERE, "epit_grads.npz"), **arrs)
    json.dump(meta, open(os.path.join(HERE, "epit_grads.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
