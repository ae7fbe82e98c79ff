#!/usr/bin/env python3
"""Generate the LFSSR fixtures (model_LFSSR.npz, lfssr.json) by running the *reference* implementation in fp32 on the CPU.

    python tests/golden/make_golden_lfssr.py

The reference's ``model/SR/LFSSR.py`` is imported from where it lies (``REF``, as tests/golden/make_golden.py does); nothing of it is copied here.
Weights are not stored: tests/lfssr_helpers.py regenerates them (synth weights with the He gain, see ``lfssr_state_dict``).  For every small case the named
intermediates of ``lfssr_helpers.LAYER_NAMES`` are stored as VCL rows, every ``stride``-th row (the stride is recorded), and the output whole; for the full patch
``out[:, :, ::8, ::8]`` and a checksum.  The generator asserts that the fixtures can see the data path: the altblock1 outputs of the seed-1 and seed-7 inputs
differ by more than 1e-3 in every case."""
import hashlib
import importlib
import json
import os
import sys
from argparse import Namespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from lfsr_amd.synth import synth_input  # noqa: E402
from tests import lfssr_helpers as H  # noqa: E402


def ref_module():
    """the reference's model.SR.LFSSR (our own mirror lives inside the package directory, not on sys.path)"""
    mine = {k: sys.modules.pop(k) for k in [k for k in sys.modules if k == "model" or k.startswith("model.")]}
    sys.path.insert(0, REF)
    try:
        return importlib.import_module("model.SR.LFSSR")
    finally:
        sys.path.remove(REF)
        for k in [k for k in sys.modules if k == "model" or k.startswith("model.")]:
            del sys.modules[k]            # a later `import model.SR.X` must not find the reference's package
        sys.modules.update(mine)


def load_ref(A, s, dtype=torch.float32):
    net = ref_module().get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
    spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    net.load_state_dict({k: torch.from_numpy(v) for k, v in H.lfssr_state_dict(spec).items()})
    return net.to(dtype).eval(), spec


def ref_layers(net, x, A, s):
    """the reference's forward with hooks -> {name: tensor} in the layouts of lfssr_helpers.lfssr_layers"""
    caps = {}

    def keep(name):
        return lambda m, i, o: caps.__setitem__(name, o.detach().clone())

    n = net.net
    hooks = [n.conv0.register_forward_hook(keep("conv0_pre")), n.altblock1[0].register_forward_hook(keep("alt1.0")),
             n.altblock1.register_forward_hook(keep("alt1")), n.fup1.register_forward_hook(keep("fup1")),
             n.res1.register_forward_hook(keep("res1")), n.iup1.register_forward_hook(keep("iup1"))]
    if s == 4:
        hooks += [n.altblock2.register_forward_hook(keep("alt2")), n.fup2.register_forward_hook(keep("fup2"))]
    with torch.no_grad():
        out = net(x, [A, A])
    for hk in hooks:
        hk.remove()
    L = {"conv0": torch.relu(caps["conv0_pre"]), "alt1.0": caps["alt1.0"], "alt1": caps["alt1"], "fup1": caps["fup1"], "sr2x": caps["res1"] + caps["iup1"]}
    if s == 4:
        L["alt2"], L["fup2"] = caps["alt2"], caps["fup2"]
    L["out"] = out
    return L


def sensitivity(net, A, h, w, B):
    """max |altblock1(seed-1 input) - altblock1(seed-7 input)|"""
    outs = []
    for seed in (1, 7):
        lr = H.mosaic_to_views(torch.from_numpy(synth_input((B, 1, A * h, A * w), seed=seed)), A)
        with torch.no_grad():
            outs.append(net.net.altblock1(torch.relu(net.net.conv0(lr))))
    return float((outs[0] - outs[1]).abs().max())


def generate(out_dir, tags=None, write=True):
    """-> (arrays, meta); tags: the cases to run (default: all of them and the full patch)"""
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    arrs, meta = {}, {"torch": torch.__version__, "numpy": np.__version__, "weights_seed": 0, "input_seed": 1, "he_gain": H.HE_GAIN, "cases": {}}
    for tag in (tags if tags is not None else list(H.CASES) + ["full"]):
        A, h, w, s, B = H.FULL if tag == "full" else H.CASES[tag]
        net, spec = load_ref(A, s)
        assert spec == H.lfssr_spec(s)
        sens = sensitivity(net, A, h, w, B)
        assert sens > 1e-3, (tag, sens)
        x = torch.from_numpy(synth_input((B, 1, A * h, A * w), seed=1))
        case = dict(A=A, h=h, w=w, s=s, B=B, spec=[[k, list(sh)] for k, sh in spec], altblock1_sensitivity=sens)
        if tag == "full":
            with torch.no_grad():
                y = net(x, [A, A]).numpy()
            arrs["full_sample"] = y[:, :, ::8, ::8].copy()
            case.update(out_shape=list(y.shape), mean=float(y.mean()), std=float(y.std()), sha256_f32=hashlib.sha256(np.ascontiguousarray(y).tobytes()).hexdigest())
        else:
            L = ref_layers(net, x, A, s)
            case["strides"] = {}
            for name, t in L.items():
                if name == "out":
                    arrs[f"{tag}_out"] = t.numpy()
                    continue
                rows = H.views_to_rows(t)
                st = H.stored_stride(*rows.shape)
                case["strides"][name] = st
                arrs[f"{tag}_{name}"] = rows[::st].numpy().copy()
            case["out_shape"] = list(L["out"].shape)
        meta["cases"][tag] = case
        print(tag, "altblock1 sensitivity %.3g" % sens)
    if write:
        np.savez_compressed(os.path.join(out_dir, "model_LFSSR.npz"), **arrs)
        json.dump(meta, open(os.path.join(out_dir, "lfssr.json"), "w"), indent=1)
        print("fixture bytes:", os.path.getsize(os.path.join(out_dir, "model_LFSSR.npz")))
    return arrs, meta


if __name__ == "__main__":
    generate(HERE)
