"""CPU: LF_InterNet training -- the torch port's gradients pinned to the reference's (tests/golden/internet_grads.*), and the host-only
parts of the training C ABI (parameter bucket layout, training workspace sizing)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from lfsr_amd.synth import synth_input
from oracle.lfsr_torch_port import internet_forward
from tests.helpers import GOLDEN, model_case

TAGS = ("a3h6w8s4", "a5h8s2")


def golden():
    return np.load(os.path.join(GOLDEN, "internet_grads.npz")), json.load(open(os.path.join(GOLDEN, "internet_grads.json")))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def port_grads(tag, dtype=torch.float64):
    """loss and {name: grad} of autograd over the torch port (fp64 by default), with the golden's inputs and L1 loss"""
    case, sd, x, _ = model_case("LF_InterNet", tag)
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    params = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in sd.items()}
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).to(dtype)
    out = internet_forward.__wrapped__(torch.from_numpy(x).to(dtype), params, A, s)
    loss = torch.nn.functional.l1_loss(out, label)
    loss.backward()
    return float(loss.detach()), {k: p.grad.numpy() for k, p in params.items()}


@pytest.mark.parametrize("tag", TAGS)
def test_port_gradients_match_reference(tag):
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
    capi.check(lib.lfsr_internet_create(C.byref(ctx), A, s, 4, 4), "internet_create")
    return lib, ctx


def test_bucket_layout_follows_state_dict():
    npz, meta = golden()
    for tag in TAGS:
        case, sd, _, _ = model_case("LF_InterNet", tag)
        lib, ctx = _ctx(case["A"], case["s"])
        try:
            n = lib.lfsr_internet_num_params(ctx)
            assert n == case["n_params"] == sum(v.size for v in sd.values())
            o = 0
            for k in meta["tags"][tag]["names"]:
                off, numel = capi.c_sz(0), capi.c_sz(0)
                capi.check(lib.lfsr_internet_param_offset(ctx, k.encode(), C.byref(off), C.byref(numel)), k)
                assert (off.value, numel.value) == (o, sd[k].size), k
                o += numel.value
            assert o == n
            assert lib.lfsr_internet_param_offset(ctx, b"no.such.weight", None, None) != 0
        finally:
            lib.lfsr_internet_destroy(ctx)


def test_num_params_angres5():
    lib, ctx = _ctx(5, 2)
    try:
        assert lib.lfsr_internet_num_params(ctx) == 5040320
    finally:
        lib.lfsr_internet_destroy(ctx)


def test_train_workspace_bytes_bounds_and_monotone():
    lib, ctx = _ctx(5, 2)
    try:
        f = lib.lfsr_internet_train_workspace_bytes
        assert f(ctx, 0, 32, 32) == 0 and f(ctx, 1, 0, 32) == 0 and f(ctx, 1, 32, -1) == 0
        assert f(None, 1, 32, 32) == 0
        sizes = [f(ctx, B, 32, 32) for B in (1, 2, 3, 8, 16)]
        assert all(v > 0 for v in sizes)
        assert all(a < b for a, b in zip(sizes, sizes[1:]))
        # the forward's per-tensor bound: B * A^2 * h * w * 320 < 2^31 floats
        B_max = ((1 << 31) - 1) // 320 // (25 * 32 * 32)
        assert f(ctx, B_max, 32, 32) > 0
        assert f(ctx, B_max + 1, 32, 32) == 0
    finally:
        lib.lfsr_internet_destroy(ctx)
    ctx = C.c_void_p()
    capi.check(lib.lfsr_internet_create(C.byref(ctx), 5, 2, 3, 4), "internet_create")   # the forward accepts n_groups = 3; training does not
    try:
        assert lib.lfsr_internet_train_workspace_bytes(ctx, 1, 8, 8) == 0
    finally:
        lib.lfsr_internet_destroy(ctx)
