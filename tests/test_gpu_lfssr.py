"""GPU: the LFSSR forward through the C ABI and the plugin against the reference's golden outputs and against the fp64 graph of tests/lfssr_helpers.py, at the
project's gate 1e-4 * max(1, max|gold|): the output, and every named intermediate -- the whole model hides them, so they are rebuilt from the operator entry
points the driver calls (and a context of one layer is checked end to end); batching, chunking and the scene dispatcher change no bit; the plugin refuses to
train."""
import functools
import importlib
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from lfsr_amd.dispatch import sr_scene
from lfsr_amd.synth import synth_input
from tests import lfssr_helpers as H
from tests.helpers import psnr

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def runtime(A, s, sd, n_layer=10):
    rt = capi.LFSSRRuntime(A, s, n_layer)
    rt.load_state([(k, dev(v)) for k, v in sd.items()], torch.device("cuda", 0))
    return rt


@functools.lru_cache(maxsize=None)
def case(tag):
    """-> geometry, state_dict, input, the fp64 layers (computed once, shared, never written to)"""
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    geom, sd, x = H.lfssr_case(tag)
    return geom, sd, x, H.lfssr_layers(x, sd, geom[0], geom[3])


def gate(gold):
    return 1e-4 * max(1.0, float(np.abs(gold).max()))


def hip_layers(sd, x, A, s, B, h, w):
    """the driver's launch sequence, operator by operator -> {name: VCL rows on the host} (out: the mosaic)"""
    d = {k: dev(v) for k, v in sd.items()}
    L = {}
    f = capi.lfssr_conv0(dev(x), d["net.conv0.weight"], d["net.conv0.bias"], A)
    L["conv0"] = f.cpu()
    lo = dev(H.mosaic_to_views(torch.from_numpy(x), A).numpy()).reshape(B * A * A, h, w)
    Hh, Ww = h, w
    for li, level in enumerate(("1", "2")[:1 if s == 2 else 2]):
        last = li == (1 if s == 4 else 0)
        for i in range(10):
            p = f"net.altblock{level}.{i}."
            t = capi.conv3x3(f, capi.pack_conv_weight(d[p + "spaconv.weight"]), B * A * A, Hh, Ww, slope=1.0)
            f = capi.angconv3x3(t, capi.pack_conv_weight(d[p + "angconv.weight"]), d[p + "angconv.bias"], B, A, Hh * Ww, in_bias=d[p + "spaconv.bias"])
            if i == 0 and level == "1":
                L["alt1.0"] = f.cpu()
        L["alt" + level] = f.cpu()
        f = capi.conv3x3_ps2(f, capi.pack_ps2_weight(d[f"net.fup{level}.0.weight"]), d[f"net.fup{level}.0.bias"], B * A * A, Hh, Ww)
        L["fup" + level] = f.cpu()
        o = capi.lfssr_tail(f, d[f"net.res{level}.weight"], d[f"net.res{level}.bias"], lo, d[f"net.iup{level}.0.weight"], d[f"net.iup{level}.0.bias"], B, A, Hh, Ww, last)
        if level == "1":
            planes = o if not last else capi.lfssr_tail(f, d["net.res1.weight"], d["net.res1.bias"], lo, d["net.iup1.0.weight"], d["net.iup1.0.bias"], B, A, Hh, Ww, False)
            L["sr2x"] = planes.reshape(-1, 1).cpu()
        lo = o
        Hh, Ww = 2 * Hh, 2 * Ww
    L["out"] = o.cpu()
    return L


@pytest.mark.parametrize("tag", list(H.CASES))
def test_small_vs_golden_and_fp64(tag):
    (A, h, w, s, B), sd, x, ref = case(tag)
    npz, strides = H.lfssr_golden(), H.lfssr_meta()["cases"][tag]["strides"]
    y = runtime(A, s, sd).forward(dev(x)).cpu().numpy()
    gold = npz[tag + "_out"]
    assert y.shape == gold.shape == (B, 1, A * h * s, A * w * s)
    e_gold, e_ref = float(np.abs(y - gold).max()), float(np.abs(y - ref["out"].numpy()).max())
    print(f"LFSSR | {tag} | out | vs golden {e_gold:.3e} | vs fp64 {e_ref:.3e} | gate {gate(gold):.3e}")
    assert e_gold < gate(gold) and e_ref < gate(gold)
    # every named intermediate, from the operator entry points in the driver's order; the chain's output equals the driver's bit for bit
    L = hip_layers(sd, x, A, s, B, h, w)
    assert sorted(L) == sorted(ref)
    assert np.array_equal(L["out"].numpy(), y)
    for name in H.LAYER_NAMES:
        if name == "out" or name not in ref:
            continue
        rows, want = L[name].numpy(), H.views_to_rows(ref[name]).numpy()
        g = npz[f"{tag}_{name}"]
        assert rows.shape == want.shape and rows[::strides[name]].shape == g.shape, name
        e_gold, e_ref = float(np.abs(rows[::strides[name]] - g).max()), float(np.abs(rows - want).max())
        print(f"LFSSR | {tag} | {name} | vs golden {e_gold:.3e} | vs fp64 {e_ref:.3e} | gate {gate(g):.3e}")
        assert e_gold < gate(g) and e_ref < gate(g), name


@pytest.mark.parametrize("tag", ["a3h6w8s2", "a2h5w7s4"])
def test_one_layer_context_vs_fp64(tag):
    """n_layer = 1: conv0, one AltFilter, fup, res + iup per level -- the first AltFilter's result reaches the output through one up-sampling stage only"""
    (A, h, w, s, B), sd, x, _ = case(tag)
    sd1 = {k: sd[k] for k, _ in H.lfssr_spec(s, 1)}
    y = runtime(A, s, sd1, n_layer=1).forward(dev(x)).cpu().numpy()
    ref = H.lfssr_layers(x, sd1, A, s, n_layer=1)["out"].numpy()
    err = float(np.abs(y - ref).max())
    print(f"LFSSR | {tag} | n_layer 1 | vs fp64 {err:.3e} | gate {gate(ref):.3e}")
    assert err < gate(ref)
    # a state_dict of the wrong depth is refused
    with pytest.raises(capi.LfsrError):
        runtime(A, s, sd, n_layer=1)


def test_full_patch():
    (A, h, w, s, B), sd, x, ref = case("full")            # 5x5 views of 32x32, x4 -> (1,1,640,640)
    npz = H.lfssr_golden()
    y = runtime(A, s, sd).forward(dev(x)).cpu().numpy()
    assert y.shape == (1, 1, 640, 640)
    err = float(np.abs(y[:, :, ::8, ::8] - npz["full_sample"]).max())
    want = ref["out"].numpy()
    p, e_full = psnr(y, want), float(np.abs(y - want).max())
    print(f"LFSSR | full | sample vs golden {err:.3e} | gate {gate(npz['full_sample']):.3e} | PSNR vs fp64 {p:.1f} dB | every pixel vs fp64 {e_full:.3e} | gate {gate(want):.3e}")
    assert err < gate(npz["full_sample"])
    assert p >= 80.0
    assert e_full < gate(want)                             # every pixel, not the stride-8 sample: a wrong pixel can pass 80 dB


def plugin():
    sys.path.insert(0, capi._HERE)
    try:
        return importlib.import_module("model.SR.LFSSR")
    finally:
        sys.path.remove(capi._HERE)


def plugin_net(A, s, sd, n_layer=10):
    M = plugin()
    cls = M.get_model if n_layer == 10 else type("get_model_shallow", (M.get_model,), {"n_layer": n_layer})
    net = cls(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.to("cuda:0").eval()


def test_plugin_surface():
    tag = "a3h6w8s2"
    (A, h, w, s, B), sd, x, _ = case(tag)
    M = plugin()
    net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
    assert [k for k in net.state_dict()] == [k for k, _ in H.lfssr_meta()["cases"][tag]["spec"]]
    net = plugin_net(A, s, sd)
    gold = H.lfssr_golden()[tag + "_out"]
    with torch.no_grad():
        y = net(dev(x), None)
    assert np.abs(y.cpu().numpy() - gold).max() < gate(gold)
    assert float(M.get_loss(None)(y, torch.zeros_like(y))) == pytest.approx(float(y.abs().mean()))
    assert M.weights_init(net) is None


def test_grad_enabled_forward_raises():
    (A, h, w, s, B), sd, x, _ = case("a3h6w8s2")
    net = plugin_net(A, s, sd)
    with pytest.raises(capi.LfsrError, match="inference-only"):
        net(dev(x), None)
    for p in net.parameters():
        p.requires_grad_(False)
    y = net(dev(x), None)                                  # frozen parameters: an inference forward
    gold = H.lfssr_golden()["a3h6w8s2_out"]
    assert np.abs(y.cpu().numpy() - gold).max() < gate(gold)


def test_load_state_dict_then_forward_sees_the_new_weights():
    (A, h, w, s, B), sd, x, _ = case("a3h6w8s2")
    net = plugin_net(A, s, sd)
    xd = dev(x)
    with torch.no_grad():
        y0 = net(xd, None).clone()
        sd2 = H.lfssr_state_dict(H.lfssr_spec(s), seed=3)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd2.items()})
        y1 = net(xd, None).clone()
        fresh = runtime(A, s, sd2).forward(xd)
    assert not torch.equal(y0, y1)
    assert torch.equal(y1, fresh)


def test_batch_of_three_equals_three_single_forwards_and_a_chunked_run():
    (A, h, w, s, _), sd, _, _ = case("a2h5w7s4")
    rt = runtime(A, s, sd)
    x = dev(synth_input((3, 1, A * h, A * w), seed=5))
    y = rt.forward(x).clone()
    singles = torch.cat([rt.forward(x[i:i + 1]).clone() for i in range(3)], 0)
    assert torch.equal(y, singles)
    assert rt.widest_row_floats == 1024 and capi.LFSSRRuntime(A, 2, 1).widest_row_floats == 256
    # forced chunks: a limit that admits two patches a launch
    rt.offset_limit = 2 * A * A * h * w * rt.widest_row_floats * 4 + 1
    assert capi.max_patches_per_launch(A, h, w, rt.widest_row_floats, rt.offset_limit) == 2
    calls = []
    inner = rt._f("forward")
    rt._f = lambda fn: (lambda *a: (calls.append(a[3]), inner(*a))[1]) if fn == "forward" else capi.ModelRuntime._f(rt, fn)
    assert torch.equal(rt.forward(x), y)
    assert calls == [2, 1]


def test_forward_refuses_past_the_launch_bound():
    (A, h, w, s, _), sd, _, _ = case("a2h5w7s4")
    rt = runtime(A, s, sd)
    lib = capi.load()
    B = (1 << 29) // (A * A * h * w * 1024) + 1               # the first batch whose widest tensor reaches 2 GiB
    assert lib.lfsr_lfssr_workspace_bytes(rt.ctx, B, h, w) > 0
    out = torch.full((8,), -7.0, device="cuda")
    ws = torch.empty(256, dtype=torch.uint8, device="cuda")
    assert lib.lfsr_lfssr_forward(rt.ctx, capi.dev_ptr(out), capi.dev_ptr(out), B, h, w, capi.dev_ptr(ws), ws.numel(), None) == -1
    assert lib.lfsr_lfssr_forward(rt.ctx, capi.dev_ptr(out), capi.dev_ptr(out), 1, h, w, capi.dev_ptr(ws), ws.numel(), None) == -2     # workspace too small
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_scene_equals_per_patch_loop():
    """sr_scene on a 40 x 33 scene (3 x 3 = 9 patches, ragged crop) at 5x5 x2 through the plugin, two layers deep, against the reference's loop: one patch at a
    time, stitched by lfsr_lf_integrate"""
    A, s, n_layer = 5, 2, 2
    sd = H.lfssr_state_dict(H.lfssr_spec(s, n_layer))
    net = plugin_net(A, s, sd, n_layer)
    h0, w0 = 40, 33
    lr = torch.from_numpy(synth_input((A * h0, A * w0), seed=3)).cuda()
    out = sr_scene(net, lr, A, s, minibatch=4)
    assert tuple(out.shape) == (A, A, h0 * s, w0 * s) and bool(torch.isfinite(out).all())
    sub = capi.lf_divide(lr, A, 32, 16)
    n1, n2 = sub.shape[:2]
    assert n1 * n2 == 9
    with torch.no_grad():
        outs = torch.stack([net(sub[i, j][None, None].contiguous(), None)[0, 0] for i in range(n1) for j in range(n2)])
    ref = capi.lf_integrate(outs.reshape(n1, n2, A * 32 * s, A * 32 * s).contiguous(), A, 32 * s, 16 * s, h0 * s, w0 * s)
    assert torch.equal(out, ref)
    # and one patch against the fp64 graph
    want = H.lfssr_layers(sub[1, 1][None, None].cpu().numpy(), sd, A, s, n_layer=n_layer)["out"].numpy()
    assert np.abs(outs[4].cpu().numpy() - want[0, 0]).max() < gate(want)
