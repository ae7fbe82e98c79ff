"""GPU: DistgSSR's HIP path against fp64 across angular resolutions, scales, view shapes and batch sizes, tensor by tensor, forward and backward.

The geometry matrix (tests/helpers.py:DISTG_MATRIX) reaches what the training tests at angRes 5 on 8x8, 6x9 and 32x32 views and at angRes 3 on
6x8 do not: angRes 1, 7, 9 and 15 (the gather forms of every EPI kernel and gradient, the three-kernel block tail, the 9x9 and 15x15
AngConv.0), scale 3 (k_head_bwd<3> and the 9-row folded head), views past 32 pixels on one side and on both (line form and gather form
accumulating into one dx, the unmerged EPIConv.0 weight gradient, several chunks of k_ang0_dgrad per image), an odd batch, the published training
geometry (B = 8 at 5x5 x 32x32: the grid-stride loops of k_add_inplace, k_head_bwd and k_init_gather9), and even angRes, where the training
forward runs and the backward must refuse.  The reference is helpers.distg_layers_fp64 (pinned on the numpy oracle and, bit for bit, on the torch
port by tests/test_distgssr_reference.py) for the output, for all 7 x 16 tensors lfsr_distgssr_train_saved returns and for every gradient.  Every
row runs the product's default kernels.

Measured figures: profiles/distgssr_geometry_tests.md."""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from lfsr_amd.synth import synth_input
from tests.helpers import (DISTG_MATRIX, arithmetic, distg_case, distg_forced_gradient_gate, distg_hip_masks_flat, distg_keys, distg_layers_fp64,
                           distg_ref_to_rows, distg_samples, distg_saved_rows, distg_spec)
from tests.test_gpu_distgssr_train import build, load_plugin

pytestmark = pytest.mark.gpu
ids = lambda g: "A%ds%dB%dh%dw%d" % g
geoms = pytest.mark.parametrize("geom", DISTG_MATRIX, ids=ids)
ODD_ROWS = tuple(g for g in DISTG_MATRIX if g[0] % 2)
EVEN_ROWS = tuple(g for g in DISTG_MATRIX if g[0] % 2 == 0)
GUARD_ROWS = (DISTG_MATRIX[0], (1, 3, 2, 9, 7), (5, 2, 1, 40, 24))
SENTINEL = -2.0 ** 100
BAND = 1 << 16            # floats behind every buffer
E_ARG, E_WS = -1, -2
torch.set_num_threads(min(torch.get_num_threads(), 16))
HOST = {"s": 0.0}         # seconds of reference work on the host, summed over the file (printed by every test that adds to it)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def gate(ref):
    """the project's forward gate (tests/test_gpu_distgssr.py: ATOL 1e-4 on outputs of order 1)"""
    return 1e-4 * max(1.0, float(torch.as_tensor(ref).abs().max()))


def runtime(A, s, sd):
    rt = capi.DistgSSRRuntime(A, s)
    rt.load_state([(k, dev(v)) for k, v in sd.items()], torch.device("cuda", 0))
    return rt


@functools.lru_cache(maxsize=None)
def fp64_out(geom):
    A, s, B, h, w = geom
    sd, x = distg_case(*geom)
    t0 = time.time()
    with torch.no_grad():
        y = torch.cat([distg_layers_fp64(x[sl], sd, A, s)[0] for sl in distg_samples(*geom)])
    HOST["s"] += time.time() - t0
    return y


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
@geoms
def test_output_vs_fp64_both_arithmetics(geom):
    A, s, B, h, w = geom
    sd, x = distg_case(*geom)
    ref = fp64_out(geom).numpy()
    tol = gate(ref)
    rt = runtime(A, s, sd)
    xg = dev(x)
    for mode, name in ((capi.ARITH_DEFAULT, "default"), (capi.ARITH_F32, "f32")):
        with arithmetic(mode):
            y = rt.forward(xg).cpu().numpy()
            singles = [rt.forward(xg[i:i + 1]).cpu().numpy() for i in range(B)] if B > 1 else []
        assert y.shape == ref.shape
        err = np.abs(y - ref)
        print(f"{geom} {name}: output max|err| {err.max():.3e} mean {err.mean():.3e} gate {tol:.3e} max|ref| {np.abs(ref).max():.3f}; host {HOST['s']:.0f} s so far")
        assert np.isfinite(y).all() and err.max() < tol
        for i, y1 in enumerate(singles):     # the kernel forms differ with the number of pixels: the same gate, not bit-equality
            d = float(np.abs(y[i:i + 1] - y1).max())
            assert d < tol, (i, d)
            assert np.abs(y1 - ref[i:i + 1]).max() < tol, i


def saved_tensors_vs_fp64(geom, rt, xg, y_tr):
    """all 7 x 16 tensors lfsr_distgssr_train_saved returns and the output, as values: under the forward gate per tensor, and mean |err| at most
    8 x the mean error of the same graph in fp32 torch on the CPU (the factor of tests/test_gpu_lft_geometries.py and
    tests/test_gpu_internet_geometries.py: not measured here, it allows for the GPU's longer sequential accumulation chains and the three-term
    bf16 forms against the CPU's blocked sums).  The reference goes through the batch in the slices of distg_samples (every HIP layout is
    sample-major), so the figures of a tensor are summed over them.  -> the saved tensors as they were read"""
    A, s, B, h, w = geom
    sd, x = distg_case(*geom)
    hip = {k: distg_saved_rows(rt, xg, *k).cpu() for k in distg_keys()}
    assert len(hip) == 7 * 16
    got_all = dict(hip)
    got_all["output", 0] = y_tr.cpu().reshape(B, -1)
    stat = {k: dict(emax=0.0, esum=0.0, csum=0.0, rmax=0.0, n=0, finite=True) for k in got_all}
    for sl in distg_samples(*geom):
        nb = sl.stop - sl.start
        t0 = time.time()
        with torch.no_grad():
            y64, L64, _ = distg_layers_fp64(x[sl], sd, A, s)
            y32, L32, _ = distg_layers_fp64(x[sl], sd, A, s, dtype=torch.float32)
        HOST["s"] += time.time() - t0
        for k, got in got_all.items():
            if k[0] == "output":
                ref, cpu32 = y64.reshape(nb, -1), y32.reshape(nb, -1)
            else:
                ref, cpu32 = (distg_ref_to_rows(L, k[0], k[1], nb, A, h, w) for L in (L64, L32))
            assert got.shape[0] % B == 0
            per = got.shape[0] // B
            g = got[sl.start * per:sl.stop * per]
            assert g.shape == ref.shape, (k, g.shape, ref.shape)
            e, st = (g.double() - ref).abs(), stat[k]
            st["emax"], st["rmax"] = max(st["emax"], float(e.max())), max(st["rmax"], float(ref.abs().max()))
            st["esum"] += float(e.sum())
            st["csum"] += float((cpu32.double() - ref).abs().sum())
            st["n"] += e.numel()
            st["finite"] &= bool(torch.isfinite(g).all())
        del L64, L32
    share, ratios, over = {}, {}, {}      # which -> (max err / gate, max err, mean err, CPU fp32 mean err, index) of the index that uses most of its gate
    for k, st in stat.items():
        assert st["n"] == got_all[k].numel(), k                 # no element left out
        tol = 1e-4 * max(1.0, st["rmax"])
        emean, cmean = st["esum"] / st["n"], st["csum"] / st["n"]
        ratios[k] = emean / cmean if cmean > 0 else (0.0 if emean == 0 else float("inf"))
        if k[0] not in share or st["emax"] / tol > share[k[0]][0]:
            share[k[0]] = (st["emax"] / tol, st["emax"], emean, cmean, k[1])
        if not (st["finite"] and st["emax"] < tol):
            over[k] = (st["emax"], tol)
    for kind, (g, emax, emean, cmean, i) in share.items():
        r = max(v for k, v in ratios.items() if k[0] == kind)
        print(f"{geom} which {kind}: index {i} max|err| {emax:.3e} ({g:.4f} of its gate) mean {emean:.3e}, fp32 CPU mean {cmean:.3e}; largest HIP / CPU of the kind {r:.2f}")
    print(f"{geom}: host {HOST['s']:.0f} s so far")
    assert not over, over
    bad = {k: round(v, 2) for k, v in ratios.items() if not v <= 8.0}
    assert not bad, bad
    return hip


@geoms
def test_every_saved_tensor_vs_fp64(geom):
    A, s, B, h, w = geom
    sd, x = distg_case(*geom)
    rt = runtime(A, s, sd)
    xg = dev(x)
    y_inf = rt.forward(xg)
    y_tr = rt.forward_train(xg)
    torch.cuda.synchronize()
    assert torch.equal(y_inf, y_tr)                       # the training forward's output is the inference output, bit for bit
    kept = saved_tensors_vs_fp64(geom, rt, xg, y_tr)
    if A % 2 == 0:                                        # forward-only rows: test_backward_refuses_even_angres
        return
    grads = rt.backward(xg, dev(synth_input((B, 1, A * h * s, A * w * s), seed=2)) - 0.5)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grads).all())
    for k in distg_keys():                                # the backward left what the forward saved alone
        assert torch.equal(kept[k], distg_saved_rows(rt, xg, *k).cpu()), k


def _buffers(rt, geom, train):
    """own allocations, sentinel-filled: (workspace of exactly *_workspace_bytes + band, its byte count, output + band, its element count)"""
    A, s, B, h, w = geom
    n = rt.train_workspace_bytes(B, h, w) if train else rt._f("workspace_bytes")(rt.ctx, B, h, w)
    assert n > 0 and n % 4 == 0
    ws = torch.full((n // 4 + BAND,), SENTINEL, device="cuda")
    n_out = B * A * h * s * A * w * s
    out = torch.full((n_out + BAND,), SENTINEL, device="cuda")
    assert ws.data_ptr() % 16 == 0
    return ws, n, out, n_out


def _intact(t, n):
    return bool((t[n:] == SENTINEL).all())


@pytest.mark.parametrize("geom", GUARD_ROWS, ids=ids)
def test_guard_bands_and_short_workspace(geom):
    assert geom in DISTG_MATRIX
    A, s, B, h, w = geom
    sd, x = distg_case(*geom)
    rt = runtime(A, s, sd)
    lib, st = rt.lib, capi.stream_ptr()
    xg = dev(x)
    # ---- inference
    ws, n, out, n_out = _buffers(rt, geom, False)
    rc = lib.lfsr_distgssr_forward(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n - 1, st)
    torch.cuda.synchronize()
    assert rc == E_WS and bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    rc = lib.lfsr_distgssr_forward(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n, st)
    torch.cuda.synchronize()
    assert rc == 0
    assert _intact(ws, n // 4) and _intact(out, n_out)
    y = rt.forward(xg)
    assert torch.equal(out[:n_out], y.reshape(-1))             # nothing of the sentinel-filled workspace was read before it was written
    # ---- training forward + backward
    ws, n, out, n_out = _buffers(rt, geom, True)
    npar = rt.num_params()
    grads = torch.full((npar + BAND,), SENTINEL, device="cuda")
    dout = dev(synth_input((B, 1, A * h * s, A * w * s), seed=2)) - 0.5
    rc = lib.lfsr_distgssr_forward_train(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n - 1, st)
    torch.cuda.synchronize()
    assert rc == E_WS and bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    rc = lib.lfsr_distgssr_forward_train(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n, st)
    torch.cuda.synchronize()
    assert rc == 0
    assert _intact(ws, n // 4) and _intact(out, n_out) and torch.equal(out[:n_out], y.reshape(-1))
    kept = ws.clone()
    rc = lib.lfsr_distgssr_backward(rt.ctx, xg.data_ptr(), dout.data_ptr(), B, h, w, ws.data_ptr(), n - 1, grads.data_ptr(), npar, st)
    torch.cuda.synchronize()                                   # the backward drains its side stream on error
    assert rc == E_WS and bool((grads == SENTINEL).all()) and torch.equal(ws, kept)
    del kept
    rc = lib.lfsr_distgssr_backward(rt.ctx, xg.data_ptr(), dout.data_ptr(), B, h, w, ws.data_ptr(), n, grads.data_ptr(), npar, st)
    torch.cuda.synchronize()
    assert rc == 0
    assert _intact(ws, n // 4) and _intact(grads, npar) and _intact(out, n_out)
    assert bool(torch.isfinite(grads[:npar]).all()) and bool((grads[:npar] != SENTINEL).all())      # every gradient element was written
    rt.forward_train(xg)
    ref = rt.backward(xg, dout)
    torch.cuda.synchronize()
    assert torch.equal(grads[:npar], ref)


@pytest.mark.parametrize("geom", EVEN_ROWS, ids=ids)
def test_backward_refuses_even_angres(geom):
    """even angRes: the training forward runs and is right (its output against fp64 here, all 7 x 16 saved tensors in
    test_every_saved_tensor_vs_fp64); lfsr_distgssr_backward answers
    LFSR_E_ARG before any launch -- the sentinel-filled bucket and the workspace are as they were -- and the plugin's backward raises"""
    A, s, B, h, w = geom
    assert A % 2 == 0
    sd, x = distg_case(*geom)
    rt = runtime(A, s, sd)
    xg = dev(x)
    y_inf = rt.forward(xg)
    y_tr = rt.forward_train(xg)
    torch.cuda.synchronize()
    assert torch.equal(y_inf, y_tr)
    ref = fp64_out(geom)
    assert float((y_tr.cpu().double() - ref).abs().max()) < gate(ref)
    ws, n, out, n_out = _buffers(rt, geom, True)
    st = capi.stream_ptr()
    assert rt.lib.lfsr_distgssr_forward_train(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:n_out], y_tr.reshape(-1)) and _intact(ws, n // 4) and _intact(out, n_out)
    npar = rt.num_params()
    grads = torch.full((npar + BAND,), SENTINEL, device="cuda")
    dout = dev(synth_input((B, 1, A * h * s, A * w * s), seed=2)) - 0.5
    kept = ws.clone()
    rc = rt.lib.lfsr_distgssr_backward(rt.ctx, xg.data_ptr(), dout.data_ptr(), B, h, w, ws.data_ptr(), n, grads.data_ptr(), npar, st)
    torch.cuda.synchronize()
    assert rc == E_ARG
    assert bool((grads == SENTINEL).all()) and torch.equal(ws, kept)
    with pytest.raises(capi.LfsrError):
        rt.backward(xg, dout)
    net = build(load_plugin(), A, s, sd)
    loss = torch.nn.functional.l1_loss(net(xg, None), dout + 0.5)
    with pytest.raises(capi.LfsrError):
        loss.backward()
    torch.cuda.synchronize()


@pytest.mark.parametrize("A,s,channels", [(0, 2, 64), (16, 2, 64), (5, 1, 64), (5, 5, 64), (5, 4, 32)])
def test_create_refuses_out_of_range(A, s, channels):
    ctx = C.c_void_p()
    assert capi.load().lfsr_distgssr_create(C.byref(ctx), A, s, 4, 4, channels) == E_ARG
    assert not ctx.value
    with pytest.raises(capi.LfsrError):
        capi.DistgSSRRuntime(A, s, channels=channels)


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def hip_step(net, xg, lg):
    """one fwd + L1 + bwd on the plugin -> (bucket, out, the forward's LeakyReLU decisions flat in HIP order, read before the backward)"""
    for p in net.parameters():
        p.grad = None
    out = net(xg, None)
    loss = torch.nn.functional.l1_loss(out, lg)
    masks = distg_hip_masks_flat(net._rt, xg)
    loss.backward()
    torch.cuda.synchronize()
    return net.grad_bucket.clone(), out.detach(), masks


@pytest.mark.parametrize("geom", ODD_ROWS, ids=ids)
def test_gradients_vs_fp64_under_the_hip_decisions(geom):
    A, s, B, h, w = geom
    sd, x = distg_case(*geom)
    net = build(load_plugin(), A, s, sd)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    xg, lg = dev(x), dev(label)
    bucket, out, masks = hip_step(net, xg, lg)
    assert torch.equal(torch.cat([p.grad.reshape(-1) for p in net.parameters()]), net.grad_bucket)
    assert bool(torch.isfinite(bucket).all())
    if s == 3 or B == 8:
        b2, o2, _ = hip_step(net, xg, lg)
        assert torch.equal(bucket, b2) and torch.equal(out, o2)
    distg_forced_gradient_gate(str(geom), net, xg, sd, x, label, A, s, masks, geom, host=HOST)


def test_fuse0_weight_gradient_streaming_and_generic_form(monkeypatch):
    """k_wgrad_pw144, the streaming fuse.0 weight gradient every row above runs, beside the generic split-K kernel that LFSR_WGRAD_PW=gather
    keeps (the model driver launches both itself: lfsr_pointwise_wgrad reaches neither choice).  One forward, hence one set of decisions;
    under the selector all 137 gradients hold the forced-decision gate, the 16 fuse.0 weight gradients have other bits than the default's (the
    selector really changed the kernel) and every other parameter has the same bits (it changed nothing else).  13x16 views at B = 2: 10 400
    rows, ragged in the slabs of both kernels"""
    geom = (5, 3, 2, 13, 16)
    assert geom in DISTG_MATRIX
    A, s, B, h, w = geom
    sd, x = distg_case(*geom)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    xg, lg = dev(x), dev(label)
    monkeypatch.delenv("LFSR_WGRAD_PW", raising=False)
    net = build(load_plugin(), A, s, sd)
    _, out, masks = hip_step(net, xg, lg)
    default = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    monkeypatch.setenv("LFSR_WGRAD_PW", "gather")
    net2 = build(load_plugin(), A, s, sd)
    _, out2, masks2 = hip_step(net2, xg, lg)
    monkeypatch.delenv("LFSR_WGRAD_PW", raising=False)
    assert torch.equal(out, out2) and all(torch.equal(masks[k], masks2[k]) for k in masks)
    errs = distg_forced_gradient_gate(f"{geom} LFSR_WGRAD_PW=gather", net2, xg, sd, x, label, A, s, masks2, geom, host=HOST)
    fuse = [k for k in default if k.endswith("fuse.0.weight")]
    assert len(fuse) == 16
    print(f"{geom} LFSR_WGRAD_PW=gather: fuse.0.weight rel-L2 vs fp64 max {max(errs[k] for k in fuse):.2e}")
    assert all(errs[k] < 1e-4 for k in fuse)
    same = [k for k, p in net2.named_parameters() if torch.equal(p.grad, default[k])]
    assert not set(same) & set(fuse), sorted(set(same) & set(fuse))
    assert set(same) == set(default) - set(fuse), sorted(set(default) - set(fuse) - set(same))
