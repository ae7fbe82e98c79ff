"""GPU: DistgSSR's fused block tail (distg_tail.hip: the branches' second stages, the concat and fuse.0 in one kernel).

Operator: lfsr_distg_branch_tail_fwd against the three-call sequence it replaces (lfsr_angconv_fwd + lfsr_epiconv_hv_fwd + lfsr_pointwise_fwd over a 144-channel
concat) on the same inputs: bit-equal, and no further from an fp64 composition.  Model: batch independence, taps, and the LFSR_DISTG_TAIL=0 selector."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from lfsr_amd.synth import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, L = 5, 0.1


def _weights(seed):
    g = torch.Generator().manual_seed(seed)
    def rnd(*shape, fan):
        return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * (1.0 / fan) ** 0.5
    return {"ang0": rnd(16, 64, A, A, fan=64 * 25), "ang2": rnd(16 * A * A, 16, 1, 1, fan=16), "epi0": rnd(32, 64, 1, A * A, fan=64 * 25),
            "epi2": rnd(32 * A, 32, 1, 1, fan=32), "fuse0": rnd(64, 144, 1, 1, fan=144)}


def _packed(wd):
    cu = {k: v.float().cuda() for k, v in wd.items()}
    return (capi.pack_conv_weight(cu["ang0"]), capi.pack_conv_weight(cu["ang2"], perm=1, ch=16), capi.pack_conv_weight(cu["epi0"]),
            capi.pack_conv_weight(cu["epi2"]), capi.pack_conv_weight(cu["fuse0"]))


def _old_sequence(x, spa, wp, B, h, w):
    """HEAD's operator sequence: the branches into a (npix, 144) concat, then the pointwise fuse.0"""
    npix = x.shape[0]
    cat = torch.zeros((npix, 144), dtype=torch.float32, device=x.device)
    cat[:, :64] = spa
    tmp = torch.empty((B * h * w, 16), dtype=torch.float32, device=x.device)
    capi.angconv(x, wp[0], wp[1], B, A, h, w, L, cat, 64, tmp=tmp)
    capi.epiconv_hv(x, wp[2], wp[3], B, A, h, w, L, cat, 80, 112)
    return capi.pointwise(cat, 144, wp[4], 64, slope=L), tmp


def _fp64_tail(spa, t_a, t_h, t_v, wd, B, h, w):
    """fp64 composition of the tail from the stage-1 activations (VCL rows (b, u, v, y, x); PixelShuffle(A) / PixelShuffle1D channel orders of DistgSSR.py)"""
    lr = lambda z: np.where(z >= 0, z, z * L)
    spa = spa.double().cpu().numpy().reshape(B, A, A, h, w, 64)
    ta = t_a.double().cpu().numpy().reshape(B, h, w, 16)
    th = t_h.double().cpu().numpy().reshape(B, A, h, w, 32)
    tv = t_v.double().cpu().numpy().reshape(B, A, h, w, 32)
    w2a = wd["ang2"].numpy().reshape(16, A, A, 16)                  # out channel c * A^2 + u * A + v
    w2e = wd["epi2"].numpy().reshape(A, 32, 32)                     # out channel f * 32 + c (factor-major)
    ang = lr(np.einsum("byxk,cuvk->buvyxc", ta, w2a))
    eh = lr(np.einsum("buyxk,vck->buvyxc", th, w2e))
    ev = lr(np.einsum("bvyxk,uck->buvyxc", tv, w2e))
    cat = np.concatenate([spa, ang, eh, ev], axis=-1).reshape(-1, 144)
    return lr(cat @ wd["fuse0"].numpy().reshape(64, 144).T)


@pytest.mark.parametrize("B,h,w", [(32, 32, 32), (1, 13, 11), (3, 9, 7)])
def test_tail_operator_matches_the_three_call_sequence(B, h, w):
    torch.manual_seed(B * 100 + h)
    npix = B * A * A * h * w
    x = torch.randn((npix, 64), dtype=torch.float32).cuda()
    spa = torch.nn.functional.leaky_relu(torch.randn((npix, 64), dtype=torch.float32), L).cuda()
    wd = _weights(7 + B)
    wp = _packed(wd)
    y_old, ta_old = _old_sequence(x, spa, wp, B, h, w)
    y_new, t_a, t_h, t_v = capi.distg_branch_tail(x, spa, *wp, B, A, h, w, L)
    torch.cuda.synchronize()
    assert torch.equal(t_a, ta_old)
    assert torch.equal(y_new, y_old), float((y_new - y_old).abs().max())
    if B == 1:      # fp64 composition (small case only): the fused kernel is no further from it than the sequence
        ref = _fp64_tail(spa, t_a, t_h, t_v, wd, B, h, w)
        e_new = np.abs(y_new.double().cpu().numpy() - ref).max()
        e_old = np.abs(y_old.double().cpu().numpy() - ref).max()
        assert e_new <= e_old and e_new < 1e-5 * max(1.0, np.abs(ref).max()), (e_new, e_old)


def test_tail_operator_refuses_uncovered_calls():
    B, h, w = 1, 8, 8
    npix = B * A * A * h * w
    x = torch.randn((npix, 64), dtype=torch.float32).cuda()
    wp = _packed(_weights(3))
    with pytest.raises(capi.LfsrError):
        capi.distg_branch_tail(x, x, *wp, B, A, 40, 8, L)                 # h > 32
    capi.set_arithmetic(capi.ARITH_F32)
    try:
        with pytest.raises(capi.LfsrError):
            capi.distg_branch_tail(x, x, *wp, B, A, h, w, L)              # fp32 arithmetic: the three-call sequence's fp32 kernels
    finally:
        capi.set_arithmetic(capi.ARITH_DEFAULT)


def _rt():
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "models.json")))["models"]["DistgSSR"]["full"]
    sd = synth_state_dict([(k, tuple(s)) for k, s in meta["spec"]], seed=0)
    rt = capi.DistgSSRRuntime(5, 4)
    rt.load_state([(k, torch.from_numpy(v).cuda()) for k, v in sd.items()], torch.device("cuda"))
    return rt


def test_forward_batch_rows_equal_single_forwards_and_taps_change_nothing():
    rt = _rt()
    x = torch.from_numpy(synth_input((32, 1, 160, 160), seed=5)).cuda()
    y = rt.forward(x)
    for i in (0, 13, 31):
        assert torch.equal(y[i:i + 1], rt.forward(x[i:i + 1])), i
    y4, _ = rt.forward(x[:4], taps=[True] * 5)          # block (0,0) on the concat path, the others fused
    assert torch.equal(y4, y[:4])


_AB = r"""
import os, sys, json, torch
sys.path.insert(0, sys.argv[1])
from lfsr_amd import capi
from lfsr_amd.synth import synth_input, synth_state_dict
meta = json.load(open(os.path.join(sys.argv[1], "tests", "golden", "models.json")))["models"]["DistgSSR"]["full"]
sd = synth_state_dict([(k, tuple(s)) for k, s in meta["spec"]], seed=0)
rt = capi.DistgSSRRuntime(5, 4)
rt.load_state([(k, torch.from_numpy(v).cuda()) for k, v in sd.items()], torch.device("cuda"))
x = torch.from_numpy(synth_input((8, 1, 160, 160), seed=9)).cuda()
os.environ["LFSR_DISTG_TAIL"] = "1"
a = rt.forward(x)
os.environ["LFSR_DISTG_TAIL"] = "0"
b = rt.forward(x)
torch.cuda.synchronize()
print("equal" if torch.equal(a, b) else "DIFFER %g" % float((a - b).abs().max()))
"""


def test_old_path_selector_gives_the_same_output():
    env = dict(os.environ, LFSR_LAB="1")
    r = subprocess.run([sys.executable, "-c", _AB, ROOT], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("equal"), r.stdout
