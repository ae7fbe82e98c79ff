"""CPU: EPIT training -- the torch port's fp32 gradients pinned to the reference's (tests/golden/epit_grads.*: the reference's own model under
torch.nn.L1Loss, because its get_loss cannot be called), and the host-only parts of the training C ABI (parameter bucket layout, training
workspace sizing)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from lfsr_amd.synth import synth_input
from oracle import lfsr_torch_port as P
from tests.helpers import GOLDEN, model_case

TAGS = ("a5h8s4", "a3h6w8s2", "a3h6w8s3")


def golden():
    return np.load(os.path.join(GOLDEN, "epit_grads.npz")), json.load(open(os.path.join(GOLDEN, "epit_grads.json")))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def port_grads(tag, dtype=torch.float32):
    """loss and {name: grad} of autograd over the torch port, with the golden's inputs and L1 loss"""
    case, sd, x, _ = model_case("EPIT", tag)
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    params = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in sd.items()}
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).to(dtype)
    out = P.epit_forward.__wrapped__(torch.from_numpy(x).to(dtype), params, A, s)
    loss = torch.nn.functional.l1_loss(out, label)
    loss.backward()
    return float(loss.detach()), {k: p.grad.numpy().astype(np.float64) for k, p in params.items()}


@pytest.mark.parametrize("tag", TAGS)
def test_port_gradients_match_reference(tag):
    """fp32 against fp32, no fp64 anywhere: both sides take the same ReLU / LeakyReLU decisions (2.4e-6 at the most when this was written)"""
    npz, meta = golden()
    names = meta["tags"][tag]["names"]
    loss, grads = port_grads(tag)
    assert abs(loss - float(npz[f"{tag}::loss"])) < 1e-6
    assert list(grads.keys()) == names
    for i, k in enumerate(names):
        g = grads[k]
        probe = np.random.default_rng([7, i]).standard_normal(g.shape)
        assert abs(np.sqrt((g * g).sum()) - npz[f"{tag}::norms"][i]) <= 1e-5 * npz[f"{tag}::norms"][i], k
        assert abs((g * probe).sum() - npz[f"{tag}::projs"][i]) <= 1e-5 * np.sqrt((g * g).sum() * probe.size), k
        if f"{tag}::grad::{k}" in npz:
            assert rel(g, npz[f"{tag}::grad::{k}"]) < 1e-5, k


def _ctx(A, s):
    lib = capi.load()
    ctx = C.c_void_p()
    capi.check(lib.lfsr_epit_create(C.byref(ctx), A, s, 5, 64), "epit_create")
    return lib, ctx


def test_bucket_layout_follows_state_dict():
    npz, meta = golden()
    for tag in TAGS:
        case, sd, _, _ = model_case("EPIT", tag)
        lib, ctx = _ctx(case["A"], case["s"])
        try:
            n = lib.lfsr_epit_num_params(ctx)
            assert n == case["n_params"] == sum(v.size for v in sd.values())
            assert len(meta["tags"][tag]["names"]) == 71
            o = 0
            for k in meta["tags"][tag]["names"]:
                off, numel = capi.c_sz(0), capi.c_sz(0)
                capi.check(lib.lfsr_epit_param_offset(ctx, k.encode(), C.byref(off), C.byref(numel)), k)
                assert (off.value, numel.value) == (o, sd[k].size), k
                o += numel.value
            assert o == n
        finally:
            lib.lfsr_epit_destroy(ctx)


def test_internal_entries_and_unknown_keys_refused():
    """the feed-forward weights' pre-split image lives in the packed buffer under no key; nothing outside state_dict has a span"""
    lib, ctx = _ctx(5, 4)
    try:
        for k in (b"altblock.0.epi_trans.feed_forward.1.weight#split", b"altblock.4.epi_trans.attention.in_proj_bias", b"altblock.5.conv.0.weight", b"no.such.weight", b""):
            off, numel = capi.c_sz(0), capi.c_sz(0)
            assert lib.lfsr_epit_param_offset(ctx, k, C.byref(off), C.byref(numel)) != 0, k
    finally:
        lib.lfsr_epit_destroy(ctx)


def test_num_params_angres5():
    lib, ctx = _ctx(5, 4)
    try:
        assert lib.lfsr_epit_num_params(ctx) == 1470080
    finally:
        lib.lfsr_epit_destroy(ctx)


def test_train_workspace_bytes_bounds_and_monotone():
    for s in (2, 4):
        lib, ctx = _ctx(5, s)
        try:
            f = lib.lfsr_epit_train_workspace_bytes
            assert f(ctx, 0, 32, 32) == 0 and f(ctx, 1, 0, 32) == 0 and f(ctx, 1, 32, -1) == 0
            assert f(None, 1, 32, 32) == 0
            sizes = [f(ctx, B, 32, 32) for B in (1, 2, 3, 8, 16)]
            assert all(v > 0 for v in sizes)
            assert all(a < b for a, b in zip(sizes, sizes[1:]))
            # every activation below 2 GiB: the widest rows are max(256, 64 s^2) floats per LR pixel
            widest = max(256, 64 * s * s)
            B_max = ((1 << 31) - 1) // 4 // widest // (25 * 32 * 32)
            assert f(ctx, B_max, 32, 32) > 0
            assert f(ctx, B_max + 1, 32, 32) == 0
        finally:
            lib.lfsr_epit_destroy(ctx)
