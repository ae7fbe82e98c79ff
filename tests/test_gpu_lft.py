"""GPU: LFT forward (config 'LFT 5x5 x4 full-scene inference') through the C ABI vs the numpy oracle and the reference's
golden outputs, incl. the non-square case that exercises the reference's h-for-w clamp in gen_mask (LFT.py:168)."""
import sys

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from lfsr_amd.dispatch import sr_scene
from lfsr_amd.synth import synth_input, synth_state_dict
from oracle import lfsr_oracle as O
from tests.helpers import arithmetic, model_case, model_spec, psnr

pytestmark = pytest.mark.gpu
ATOL = 1e-4


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def runtime(case, sd):
    rt = capi.ModelRuntime("lft", case["A"], case["s"], 4, 64)
    rt.load_state([(k, dev(v)) for k, v in sd.items()], torch.device("cuda", 0))
    return rt


def test_position_encoding():
    lib = capi.load()
    A, h, w, C = 5, 6, 8, 64
    spa = torch.empty(h * w, C, device="cuda")
    ang = torch.empty(A * A, C, device="cuda")
    capi.check(lib.lfsr_lft_position_fwd(capi.dev_ptr(spa), capi.dev_ptr(ang), A, h, w, C, capi.stream_ptr()), "pe")
    ph, pw, pa = O.lft_position_encoding([h, w, A * A], C, np.float64)
    ref = ((ph[:, None, :] + pw[None, :, :]) / 2).reshape(h * w, C)
    assert np.abs(spa.cpu().numpy() - ref).max() < 1e-6
    assert np.abs(ang.cpu().numpy() - pa).max() < 1e-6


def test_spatial_window_attention_vs_masked_mha():
    """5x5 window predicate with the h-for-w clamp == the reference's dense additive mask (LFT.py:161-174)"""
    lib = capi.load()
    n, h, w, E, NH = 3, 6, 8, 128, 8
    q, k, v = [(np.random.default_rng(s).standard_normal((n * h * w, E))).astype(np.float32) for s in (1, 2, 3)]
    qd, kd, vd = dev(q), dev(k), dev(v)
    o = torch.empty(n * h * w, E, device="cuda")
    capi.check(lib.lfsr_window_attn_fwd(capi.dev_ptr(qd), E, 0, capi.dev_ptr(kd), E, 0, capi.dev_ptr(vd), E, 0, capi.dev_ptr(o), E, 0, NH, E // NH,
                                        n, 1, 1, h * w, 0, 0, h, w, w, 1, 2, 3, 2, 3, h, capi.stream_ptr()), "attn")
    mask = O.lft_gen_mask(h, w, 5, np.float64)
    hd = E // NH
    def heads(t):
        return t.astype(np.float64).reshape(n, h * w, NH, hd).transpose(0, 2, 1, 3)
    S = heads(q) @ heads(k).transpose(0, 1, 3, 2) / np.sqrt(hd) + mask
    Pm = np.exp(S - S.max(-1, keepdims=True))
    Pm /= Pm.sum(-1, keepdims=True)
    ref = (Pm @ heads(v)).transpose(0, 2, 1, 3).reshape(n * h * w, E)
    assert np.abs(o.cpu().numpy() - ref).max() < 1e-5


@pytest.mark.parametrize("B,A,h,w", [(2, 3, 4, 6), (1, 5, 3, 5), (2, 5, 8, 8), (1, 8, 2, 3), (1, 9, 2, 2), (2, 1, 3, 4)])
def test_angular_attention_vs_mha(B, A, h, w):
    """AngTrans attention (LFT.py:236-241): the A*A views at one (y, x) are the sequence, 8 heads of 8, no mask; q | k read from one 128-wide buffer, token stride = one
    view image -- the strided addressing lft.cpp uses -- against dense fp64 multi-head attention.  A = 5 runs k_ang_attn_pair (two queries per thread, four pixels per
    block: 15 sequences leave a block with three), A = 3 and A = 8 (64 tokens, its bound) and A = 1 (one token) the LDS-tiled kernel, A = 9 the generic
    k_window_attn<8>"""
    lib = capi.load()
    E, NH = 64, 8
    AA, HW = A * A, h * w
    npix = B * AA * HW
    q, k, v = [(np.random.default_rng(s).standard_normal((npix, E))).astype(np.float32) for s in (11, 12, 13)]
    qk = dev(np.concatenate([q, k], axis=1))
    vd = dev(v)
    o = torch.empty(npix, E, device="cuda")
    capi.check(lib.lfsr_window_attn_fwd(capi.dev_ptr(qk), 2 * E, 0, capi.dev_ptr(qk), 2 * E, E, capi.dev_ptr(vd), E, 0, capi.dev_ptr(o), E, 0, NH, E // NH,
                                        B, h, w, AA * HW, w, 1, AA, 1, HW, 0, AA, AA, 0, 1, 0, capi.stream_ptr()), "ang attn")
    hd = E // NH
    def seqs(t):      # (B, AA, HW, NH, hd) -> (B, HW, NH, AA, hd)
        return t.astype(np.float64).reshape(B, AA, HW, NH, hd).transpose(0, 2, 3, 1, 4)
    S = seqs(q) @ seqs(k).transpose(0, 1, 2, 4, 3) / np.sqrt(hd)
    Pm = np.exp(S - S.max(-1, keepdims=True))
    Pm /= Pm.sum(-1, keepdims=True)
    ref = (Pm @ seqs(v)).transpose(0, 3, 1, 2, 4).reshape(npix, E)
    assert np.abs(o.cpu().numpy() - ref).max() < 1e-5


@pytest.mark.parametrize("sel", [None, ("LFSR_ATTN_ANG", "lds"), ("LFSR_ATTN_ANG", "loop"), ("LFSR_ATTN_ANG", "l1"), ("LFSR_ATTN_L1", "1")])
def test_angular_attention_kept_forms_vs_mha(sel, monkeypatch):
    """The kept A/B forms of the angular attention at A = 5, the rows of the forward chain (attn.cpp) below k_ang_attn_pair: LFSR_ATTN_ANG=lds runs
    k_window_attn_lds<8, 8> with its batched staging, =loop with its plain staging loop, =l1 and LFSR_ATTN_L1 the generic k_window_attn<8>.  The call, the fp64
    reference and the gate of test_angular_attention_vs_mha at (1, 5, 3, 5): 15 sequences, so the last k_ang_attn_pair block of the default form is ragged"""
    for name in ("LFSR_ATTN", "LFSR_ATTN_ANG", "LFSR_ATTN_L1"):
        monkeypatch.delenv(name, raising=False)
    if sel:
        monkeypatch.setenv(*sel)
    test_angular_attention_vs_mha(1, 5, 3, 5)


@pytest.mark.parametrize("ln_fuse", ["default", "0", "1"])   # default: all norms inside the consuming kernels / every norm its own launch / only the feed-forward norms fused
@pytest.mark.parametrize("tag", ["a5h8s4", "a3h6w8s2", "a3h6w8s3"])     # a3h6w8s3: scale 3, the two-kernel tail
def test_lft_small_vs_golden_and_oracle(tag, ln_fuse, monkeypatch):
    if ln_fuse == "default":
        monkeypatch.delenv("LFSR_LN_FUSE", raising=False)
    else:
        monkeypatch.setenv("LFSR_LN_FUSE", ln_fuse)
    case, sd, x, npz = model_case("LFT", tag)
    y = runtime(case, sd).forward(dev(x)).cpu().numpy()
    gold = npz[tag + "_out"]
    ref = O.lft_forward(x, sd, case["A"], case["s"])
    assert np.abs(y - ref).max() < ATOL
    assert np.abs(y - gold).max() < ATOL
    assert psnr(y, gold) >= 80.0


@pytest.mark.parametrize("tag", ["a5h8s4", "a3h6w8s2"])
def test_lft_fp32_arithmetic_vs_golden_and_oracle(tag):
    """lfsr_set_arithmetic(LFSR_ARITH_F32): every GEMM on fp32 MFMA, the up-sampling tail as k_up_tail2"""
    case, sd, x, npz = model_case("LFT", tag)
    rt = runtime(case, sd)
    with arithmetic(capi.ARITH_F32):
        y = rt.forward(dev(x)).cpu().numpy()
    gold = npz[tag + "_out"]
    assert np.abs(y - O.lft_forward(x, sd, case["A"], case["s"])).max() < ATOL
    assert np.abs(y - gold).max() < ATOL
    assert psnr(y, gold) >= 80.0


@pytest.mark.parametrize("arith", ["default", "f32"])
def test_lft_5x5_ragged_geometry_vs_oracle(arith):
    """h = 13, w = 15, B = 2: two strips of spatial-attention queries per view (the second ragged), the h-for-w column clamp cutting windows (13 < 15), a
    mosaic ragged against the tail's 4 x 32 tiles; the whole output against the fp64 oracle.  (w stays below h + 3: past it the clamp leaves queries without
    keys, and the reference's softmax over an all -inf mask row gives NaN.)"""
    A, s, B, h, w = 5, 4, 2, 13, 15
    sd = synth_state_dict(model_spec("LFT", A, s), seed=0)
    x = synth_input((B, 1, A * h, A * w), seed=9)
    rt = runtime(dict(A=A, s=s), sd)
    with arithmetic(capi.ARITH_F32 if arith == "f32" else capi.ARITH_DEFAULT):
        y = rt.forward(dev(x)).cpu().numpy()
    assert np.abs(y - O.lft_forward(x, sd, A, s)).max() < ATOL


def test_lft_arithmetic_switch_on_one_runtime():
    """default -> F32 -> default on one runtime: the F32 output holds the gate and is not the default's; the default comes back bit for bit"""
    case, sd, x, npz = model_case("LFT", "a3h6w8s2")
    rt = runtime(case, sd)
    xd = dev(x)
    y0 = rt.forward(xd).cpu().numpy()
    with arithmetic(capi.ARITH_F32):
        y1 = rt.forward(xd).cpu().numpy()
    y2 = rt.forward(xd).cpu().numpy()
    ref = O.lft_forward(x, sd, case["A"], case["s"])
    assert np.abs(y1 - ref).max() < ATOL
    assert not np.array_equal(y1, y0)
    assert np.array_equal(y2, y0)


@pytest.mark.parametrize("A,h,w,B", [(3, 6, 8, 2), (5, 8, 8, 1)])
def test_lft_scale3_vs_oracle(A, h, w, B):
    s = 3
    sd = synth_state_dict(model_spec("LFT", A, s), seed=0)
    x = synth_input((B, 1, A * h, A * w), seed=1)
    y = runtime(dict(A=A, s=s), sd).forward(dev(x)).cpu().numpy()
    assert y.shape == (B, 1, A * h * s, A * w * s)
    assert np.abs(y - O.lft_forward(x, sd, A, s)).max() < ATOL


@pytest.mark.parametrize("tag", ["a5h8s4", "a3h6w8s2"])
def test_lft_two_kernel_tail_at_scales_2_and_4(tag, monkeypatch):
    """LFSR_NO_UPTAIL: the tail as lfsr_upsample_ps_fwd + lfsr_hr_tail_fwd, against the oracle and against the fused tail"""
    case, sd, x, npz = model_case("LFT", tag)
    rt = runtime(case, sd)
    monkeypatch.delenv("LFSR_NO_UPTAIL", raising=False)
    y1 = rt.forward(dev(x)).cpu().numpy()
    monkeypatch.setenv("LFSR_NO_UPTAIL", "1")
    y2 = rt.forward(dev(x)).cpu().numpy()
    assert np.abs(y2 - O.lft_forward(x, sd, case["A"], case["s"])).max() < ATOL
    assert np.abs(y2 - y1).max() < ATOL


def test_lft_full_patch_and_scene():
    case, sd, x1, npz = model_case("LFT", "full")
    rt = runtime(case, sd)
    y = rt.forward(dev(x1)).cpu().numpy()
    assert np.abs(y[:, :, ::8, ::8] - npz["full_sample"]).max() < ATOL          # the reference itself, 5x5 x 32x32, x4
    label = synth_input(y.shape, seed=2)
    # full-scene tiling (BASELINE config 5): LFdivide -> batched LFT -> LFintegrate == per-patch loop
    A, h0, w0 = 5, 40, 33
    lr = torch.from_numpy(synth_input((A * h0, A * w0), seed=3)).cuda()
    net = lambda t, info=None: rt.forward(t.contiguous())
    out = sr_scene(net, lr, A, 4, minibatch=5).cpu().numpy()
    sub = capi.lf_divide(lr, A, 32, 16)
    n1, n2 = sub.shape[:2]
    outs = [rt.forward(sub[i, j][None, None].contiguous()).cpu().numpy()[0, 0] for i in range(n1) for j in range(n2)]
    ref = O.lf_integrate(np.stack(outs).reshape(n1, n2, 640, 640), A, 128, 64, h0 * 4, w0 * 4)
    assert np.array_equal(out, ref)
    assert abs(psnr(y, label) - psnr(npz["full_sample"], label[:, :, ::8, ::8])) < 1.0   # sanity only (different supports)


def test_lft_plugin_surface():
    import importlib
    from argparse import Namespace
    sys.path.insert(0, capi._HERE)
    try:
        M = importlib.import_module("model.SR.LFT")
    finally:
        sys.path.remove(capi._HERE)
    case, sd, x, npz = model_case("LFT", "a3h6w8s2")
    net = M.get_model(Namespace(angRes_in=3, angRes_out=3, scale_factor=2))
    assert [k for k in net.state_dict()] == [k for k, _ in case["spec"]]
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to("cuda:0").eval()
    with torch.no_grad():
        y = net(dev(x), [3, 3])
    assert np.abs(y.cpu().numpy() - npz["a3h6w8s2_out"]).max() < ATOL
