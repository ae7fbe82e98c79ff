"""GPU: EPIT's HIP path against fp64 across angular resolutions, scales, view shapes and batch sizes, tensor by tensor, forward and backward.

The geometry matrix (tests/helpers.py:EPIT_MATRIX) reaches what the three golden geometries, the scale-3 case, the 8 x 36 fallback and the
32x32 patch at B = 1 do not: every angular resolution from 1 to 15 through the model, the run-time-n1 attention kernels
k_epi_attn_mfma<10, 0> / k_epi_attn_bwd_mfma<10, 0> at their bound of 160 tokens and one token past it, views shorter than the attention
window's halves and than a convolution tile, views wider than 32, and the published training geometry (B = 8 at 5x5 x 32x32), where the
weight-gradient splits turn ragged, k_ew and k_tail_bwd loop and lfsr_add_inplace joins the two passes' weight gradients over a full span.
The reference is helpers.epit_layers_fp64 (pinned on the numpy oracle and on the torch port by tests/test_epit_reference.py) for the
output, for all 40 tensors lfsr_epit_train_saved can return and for every gradient.  Every row runs the product's default kernels.

Measured figures: profiles/epit_geometry_tests.md."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from lfsr_amd.synth import synth_input
from tests.helpers import (EPIT_MATRIX, arithmetic, epit_case, epit_forced_fp64_grads, epit_keys, epit_layers_fp64, epit_layout,
                           epit_ref_to_rows, epit_samples, epit_saved_rows, model_spec)
from tests.test_gpu_epit_train import hip_step, make_net, rel

pytestmark = pytest.mark.gpu
ids = lambda g: "A%ds%dB%dh%dw%d" % g
geoms = pytest.mark.parametrize("geom", EPIT_MATRIX, ids=ids)
GUARD_ROWS = (EPIT_MATRIX[0], EPIT_MATRIX[1], EPIT_MATRIX[3])      # among them a scale-3 row and the 161-token row
FORWARD_KINDS, BACKWARD_KINDS = (0, 1, 2, 3), (4, 5, 6)           # lfsr_epit_train_saved: there after forward_train / after backward
SENTINEL = -2.0 ** 100
BAND = 1 << 16            # floats behind every buffer
E_ARG, E_WS = -1, -2
torch.set_num_threads(min(torch.get_num_threads(), 16))
HOST = {"s": 0.0}         # seconds of reference work on the host, summed over the file (printed by every test that adds to it)
_OUT64 = {}               # geometry -> fp64 output, computed once for the file


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def gate(ref):
    """the project's forward gate (tests/test_gpu_epit.py, tests/test_gpu_lft.py, tests/test_gpu_internet.py)"""
    return 1e-4 * max(1.0, float(torch.as_tensor(ref).abs().max()))


def runtime(A, s, sd):
    rt = capi.ModelRuntime("epit", A, s, 5, 64)
    rt.load_state([(k, dev(v)) for k, v in sd.items()], torch.device("cuda", 0))
    return rt


def decisions(geom):
    """how many ReLU / LeakyReLU decisions the row takes: per LR pixel 3 x 64 in conv_init, per pass 256 + 64 + 64, and 64 s^2 in the tail"""
    A, s, B, h, w = geom
    return B * A * A * h * w * (3 * 64 + 10 * (256 + 64 + 64) + 64 * s * s)


def reference_rows(geom, dtype):
    """(output, {(which, index): rows in HIP order}) of epit_layers_fp64 without forced decisions; rows are sample-major, so per-sample runs concatenate"""
    A, s, B, h, w = geom
    sd, x = epit_case(*geom)
    t0 = time.time()
    ys, rows = [], {k: [] for k in epit_keys()}
    with torch.no_grad():
        for sl in epit_samples(*geom):
            y, L, _ = epit_layers_fp64(x[sl], sd, A, s, dtype=dtype)
            ys.append(y)
            for k in rows:
                rows[k].append(epit_ref_to_rows(L[k], epit_layout(*k), sl.stop - sl.start, A, h, w).contiguous())
            del L
    HOST["s"] += time.time() - t0
    y = torch.cat(ys)
    if dtype == torch.float64:
        _OUT64[geom] = y
    return y, {k: torch.cat(v) for k, v in rows.items()}


def fp64_out(geom):
    if geom not in _OUT64:
        A, s, B, h, w = geom
        sd, x = epit_case(*geom)
        t0 = time.time()
        with torch.no_grad():
            _OUT64[geom] = torch.cat([epit_layers_fp64(x[sl], sd, A, s)[0] for sl in epit_samples(*geom)])
        HOST["s"] += time.time() - t0
    return _OUT64[geom]


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
@geoms
def test_every_saved_tensor_vs_fp64(geom):
    """all 40 tensors lfsr_epit_train_saved can return (28 after the training forward, 12 more that the backward rebuilds) and the output, as
    values: under the forward gate per tensor, and mean |err| at most 8 x the mean error of the same graph in fp32 torch on the CPU.  The
    factor is not measured (tests/test_gpu_internet_geometries.py::test_every_saved_layer_vs_fp64): it allows for the GPU's longer sequential
    accumulation chains (576 terms in the 3x3 convolutions, 256 in the feed-forward) against the CPU's blocked sums and for the three-term
    bf16 forms, and still sits an order of magnitude inside the gate."""
    A, s, B, h, w = geom
    sd, x = epit_case(*geom)
    rt = runtime(A, s, sd)
    xg = dev(x)
    y_inf = rt.forward(xg)
    y_tr = rt.forward_train(xg)
    torch.cuda.synchronize()
    assert torch.equal(y_inf, y_tr)                       # the training forward's output is the inference output, bit for bit
    hip = {k: epit_saved_rows(rt, xg, *k).cpu() for k in epit_keys(FORWARD_KINDS)}
    rt.backward(xg, dev(synth_input((B, 1, A * h * s, A * w * s), seed=2)) - 0.5)
    torch.cuda.synchronize()
    hip.update({k: epit_saved_rows(rt, xg, *k).cpu() for k in epit_keys(BACKWARD_KINDS)})
    for k in epit_keys(FORWARD_KINDS):                    # the backward left what the forward saved alone
        assert torch.equal(hip[k], epit_saved_rows(rt, xg, *k).cpu()), k
    assert len(hip) == 40
    y64, L64 = reference_rows(geom, torch.float64)
    y32, L32 = reference_rows(geom, torch.float32)
    share, ratios, over = {}, {}, {}      # kind -> (max err / gate, max err, mean err, CPU fp32 mean err, index) of the index that uses most of its gate

    def check(key, got, ref, cpu32):
        assert got.shape == ref.shape, (key, got.shape, ref.shape)
        tol = gate(ref)
        e = (got.double() - ref).abs()
        emax, emean, cmean = float(e.max()), float(e.mean()), float((cpu32.double() - ref).abs().mean())
        ratios[key] = emean / cmean if cmean > 0 else (0.0 if emean == 0 else float("inf"))
        if key[0] not in share or emax / tol > share[key[0]][0]:
            share[key[0]] = (emax / tol, emax, emean, cmean, key[1])
        if not (bool(torch.isfinite(got).all()) and emax < tol):
            over[key] = (emax, tol)
    for k in epit_keys():
        check(k, hip.pop(k), L64.pop(k), L32.pop(k))
    check(("output", 0), y_tr.cpu(), y64, y32)
    for kind, (g, emax, emean, cmean, i) in share.items():
        r = max(v for k, v in ratios.items() if k[0] == kind)
        print(f"{geom} which {kind}: index {i} max|err| {emax:.3e} ({g:.4f} of its gate) mean {emean:.3e}, fp32 CPU mean {cmean:.3e}; largest HIP / CPU of the kind {r:.2f}")
    print(f"{geom}: host {HOST['s']:.1f} s so far")
    assert not over, over
    bad = {k: round(v, 2) for k, v in ratios.items() if not v <= 8.0}
    assert not bad, bad


@geoms
def test_output_vs_fp64_both_arithmetics(geom):
    A, s, B, h, w = geom
    sd, x = epit_case(*geom)
    ref = fp64_out(geom).numpy()
    tol = gate(ref)
    rt = runtime(A, s, sd)
    xg = dev(x)
    for mode, name in ((capi.ARITH_DEFAULT, "default"), (capi.ARITH_F32, "f32")):
        with arithmetic(mode):
            y = rt.forward(xg).cpu().numpy()
            y_tr = rt.forward_train(xg).cpu().numpy()
            singles = [rt.forward(xg[i:i + 1]).cpu().numpy() for i in range(B)] if B > 1 else []
        assert y.shape == ref.shape
        err = np.abs(y - ref)
        print(f"{geom} {name}: output max|err| {err.max():.3e} mean {err.mean():.3e} gate {tol:.3e} max|ref| {np.abs(ref).max():.3f}; host {HOST['s']:.1f} s so far")
        assert np.isfinite(y).all() and err.max() < tol
        assert np.array_equal(y, y_tr)           # the training forward's output is the inference output, bit for bit, in this arithmetic too
        for i, y1 in enumerate(singles):         # the kernel forms differ with M: the same gate, not bit-equality
            d = float(np.abs(y[i:i + 1] - y1).max())
            assert d < tol, (i, d)
            assert np.abs(y1 - ref[i:i + 1]).max() < tol, i


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
    A, s, B, h, w = geom
    sd, x = epit_case(*geom)
    rt = runtime(A, s, sd)
    lib, st = rt.lib, capi.stream_ptr()
    xg = dev(x)
    # ---- inference
    ws, n, out, n_out = _buffers(rt, geom, False)
    rc = lib.lfsr_epit_forward(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n - 1, st)
    torch.cuda.synchronize()
    assert rc == E_WS and bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    rc = lib.lfsr_epit_forward(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n, st)
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
    rc = lib.lfsr_epit_forward_train(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n - 1, st)
    torch.cuda.synchronize()
    assert rc == E_WS and bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    rc = lib.lfsr_epit_forward_train(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n, st)
    torch.cuda.synchronize()
    assert rc == 0
    assert _intact(ws, n // 4) and _intact(out, n_out) and torch.equal(out[:n_out], y.reshape(-1))
    kept = ws.clone()
    rc = lib.lfsr_epit_backward(rt.ctx, xg.data_ptr(), dout.data_ptr(), B, h, w, ws.data_ptr(), n - 1, grads.data_ptr(), npar, st)
    torch.cuda.synchronize()
    assert rc == E_WS and bool((grads == SENTINEL).all()) and torch.equal(ws, kept)
    del kept
    rc = lib.lfsr_epit_backward(rt.ctx, xg.data_ptr(), dout.data_ptr(), B, h, w, ws.data_ptr(), n, grads.data_ptr(), npar, st)
    torch.cuda.synchronize()
    assert rc == 0
    assert _intact(ws, n // 4) and _intact(grads, npar) and _intact(out, n_out)
    assert bool(torch.isfinite(grads[:npar]).all()) and bool((grads[:npar] != SENTINEL).all())      # every gradient element was written
    rt.forward_train(xg)
    ref = rt.backward(xg, dout)
    assert torch.equal(grads[:npar], ref)


@pytest.mark.parametrize("A,s,n_block,channels", [(0, 2, 5, 64), (16, 2, 5, 64), (5, 1, 5, 64), (5, 5, 5, 64), (5, 4, 5, 32), (5, 4, 0, 64)])
def test_create_refuses_out_of_range(A, s, n_block, channels):
    ctx = C.c_void_p()
    assert capi.load().lfsr_epit_create(C.byref(ctx), A, s, n_block, channels) == E_ARG
    assert not ctx.value
    with pytest.raises(capi.LfsrError):
        capi.ModelRuntime("epit", A, s, n_block, channels)


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def cpu_fp32_rel(net, xg, sd, x, label, A, s, forced):
    """e_ref of the cancellation allowance: fp32 CPU autograd of the same graph under the same decisions (the HIP path's) against `forced`,
    the fp64 autograd under them"""
    f32, _ = epit_forced_fp64_grads(net._rt, xg, sd, x, label, A, s, dtype=torch.float32)
    return {k: rel(f32[k], forced[k]) for k in sd}


@geoms
def test_gradients_vs_fp64_under_the_hip_decisions(geom):
    """every parameter's gradient (71 state_dict entries) against fp64 autograd of the reference graph under the HIP path's own 34 ReLU /
    LeakyReLU decisions: rel-L2 < 1e-4 per parameter (the yardstick of test_gpu_epit_train.py::test_grads_match_reference_golden), no
    parameter and no element left out.  A parameter that misses it gets the allowance of tests/test_gpu_lft_geometries.py,
    max(1e-4, 3 x e_ref), e_ref being the fp32 CPU autograd of the same graph under the same decisions against fp64: what is cancellation there is cancellation here.
    The forced decisions may not hide a wrong activation: at most 1e-5 of the row's decisions may differ from fp64's own (the reference's own
    fp32 graph shows 1 to 3 in 3.7 to 32 M, tests/test_gpu_epit_train.py)."""
    A, s, B, h, w = geom
    sd, x = epit_case(*geom)
    net, _ = make_net(A, s, sd)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    xg, lg = dev(x), dev(label)
    _, bucket, out = hip_step(net, xg, lg)
    assert torch.equal(torch.cat([p.grad.reshape(-1) for p in net.parameters()]), net.grad_bucket)
    assert bool(torch.isfinite(bucket).all())
    if s == 3 or B == 8:
        _, b2, o2 = hip_step(net, xg, lg)
        assert torch.equal(bucket, b2) and torch.equal(out, o2)
    t0 = time.time()
    forced, flips = epit_forced_fp64_grads(net._rt, xg, sd, x, label, A, s)
    HOST["s"] += time.time() - t0
    names = [k for k, _ in net.named_parameters()]
    assert names == [k for k, _ in model_spec("EPIT", 5, s)] and len(names) == 71 and sum(p.numel() for p in net.parameters()) == bucket.numel()
    errs = {k: rel(p.grad.detach().cpu().numpy(), forced[k]) for k, p in net.named_parameters()}
    v = np.array(list(errs.values()))
    n_dec = decisions(geom)
    print(f"{geom}: gradient rel-L2 vs fp64 median {np.median(v):.2e} max {v.max():.2e} ({max(errs, key=errs.get)}); "
          f"ReLU / LeakyReLU decisions differing from fp64's own: {flips} of {n_dec} (cap {1e-5 * n_dec:.1f}); host {HOST['s']:.1f} s so far")
    assert flips <= 1e-5 * n_dec, (flips, n_dec)
    bad = {k: e for k, e in errs.items() if not e < 1e-4}
    if bad:
        t0 = time.time()
        e_ref = cpu_fp32_rel(net, xg, sd, x, label, A, s, forced)
        HOST["s"] += time.time() - t0
        for k, e in bad.items():
            print(f"{geom}: {k} rel-L2 {e:.3e}, fp32 CPU autograd against fp64 {e_ref[k]:.3e}")
        bad = {k: (e, e_ref[k]) for k, e in bad.items() if not e < max(1e-4, 3 * e_ref[k])}
    assert not bad, bad
