"""GPU: LF_InterNet's HIP path against fp64 across angular resolutions, scales and batch sizes, layer by layer, forward and backward.

The geometry matrix (tests/helpers.py:INTERNET_MATRIX) reaches what the two golden geometries and the 32x32 patch at B = 1 do not: scale 3
(9 of the 16 / 32 padded sub-pixel slots), even and extreme angular resolutions (1, 2, 4, 7, 9), views larger than 32x32, the row-streaming
GEMM forms of inference (>= 2048 LR pixels), and the 64-bit addressing branch of the gather-GEMM for SpaBottle (B >= 3 at 5x5 x 32x32) and
SpaConvSq (B >= 7), which the published training step (B = 8) runs.  The reference is the numpy oracle for the output and
helpers.internet_layers_fp64 (pinned on the oracle by tests/test_internet_reference.py) for every saved layer and every gradient.

Measured figures: profiles/internet_geometry_tests.md."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from lfsr_amd.synth import synth_input, synth_state_dict
from oracle import lfsr_oracle as O
from tests.helpers import (INTERNET_MATRIX, INTERNET_SAVED, arithmetic, forced_fp64_grads, internet_case, internet_keys, internet_layers_fp64,
                           internet_ref_to_rows, internet_saved_rows, internet_spec)
from tests.test_gpu_internet_train import hip_step, make_net, rel

pytestmark = pytest.mark.gpu
geoms = pytest.mark.parametrize("geom", INTERNET_MATRIX, ids=lambda g: "A%ds%dB%dh%dw%d" % g)
GUARD_ROWS = ((7, 2, 1, 5, 6), (2, 3, 2, 9, 7), (5, 3, 2, 13, 16))
SENTINEL = -2.0 ** 100
BAND = 1 << 16            # floats behind every buffer
E_ARG, E_WS = -1, -2
torch.set_num_threads(min(torch.get_num_threads(), 16))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def gate(ref):
    """the project's forward gate (tests/test_gpu_internet.py)"""
    return 1e-4 * max(1.0, float(np.abs(np.asarray(ref)).max()))


def runtime(A, s, sd, n_groups=4):
    rt = capi.ModelRuntime("internet", A, s, n_groups, 4)
    rt.load_state([(k, dev(v)) for k, v in sd.items()], torch.device("cuda", 0))
    return rt


@functools.lru_cache(maxsize=None)
def oracle_out(geom):
    sd, x = internet_case(*geom)
    return O.internet_forward(x, sd, geom[0], geom[1])


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
@geoms
def test_output_vs_oracle_both_arithmetics(geom):
    A, s, B, h, w = geom
    sd, x = internet_case(*geom)
    ref = oracle_out(geom)
    tol = gate(ref)
    rt = runtime(A, s, sd)
    xg = dev(x)
    for mode, name in ((capi.ARITH_DEFAULT, "default"), (capi.ARITH_F32, "f32")):
        with arithmetic(mode):
            y = rt.forward(xg).cpu().numpy()
            singles = [rt.forward(xg[i:i + 1]).cpu().numpy() for i in range(B)] if B > 1 else []
        assert y.shape == ref.shape
        err = np.abs(y - ref)
        print(f"{geom} {name}: output max|err| {err.max():.3e} mean {err.mean():.3e} gate {tol:.3e} max|ref| {np.abs(ref).max():.3f}")
        assert np.isfinite(y).all() and err.max() < tol
        for i, y1 in enumerate(singles):     # the GEMM forms differ with M: the same gate, not bit-equality
            d = float(np.abs(y[i:i + 1] - y1).max())
            assert d < tol, (i, d)
            assert np.abs(y1 - ref[i:i + 1]).max() < tol, i


@geoms
def test_every_saved_layer_vs_fp64(geom):
    """every tensor the training forward saves, as values, under the forward gate per tensor and under 8 x the mean error of the same graph in
    fp32 torch on the CPU.  The factor is not measured: it allows for the GPU's longer sequential accumulation chains (up to 2880 terms) against
    the CPU's blocked sums and for the three-term bf16 forms, and still sits an order of magnitude inside the gate."""
    A, s, B, h, w = geom
    sd, x = internet_case(*geom)
    rt = runtime(A, s, sd)
    xg = dev(x)
    y_inf = rt.forward(xg)
    y_tr = rt.forward_train(xg)
    torch.cuda.synchronize()
    assert torch.equal(y_inf, y_tr)                       # the training forward's output is the inference output, bit for bit
    with torch.no_grad():
        y64, L64, _ = internet_layers_fp64(x, sd, A, s)
        y32, L32, _ = internet_layers_fp64(x, sd, A, s, dtype=torch.float32)
    worst = {}          # kind -> (max err / gate, hip mean err / cpu fp32 mean err, max err, mean err, cpu mean err), the worst index of each

    def check(kind, i, hip, ref, cpu32):
        tol = 1e-4 * max(1.0, float(ref.abs().max()))
        e = (hip - ref).abs()
        emax, emean, cmean = float(e.max()), float(e.mean()), float((cpu32.double() - ref).abs().mean())
        ratio = emean / cmean if cmean > 0 else (0.0 if emean == 0 else float("inf"))
        rec = (emax / tol, ratio, emax, emean, cmean)
        if kind not in worst or rec[1] > worst[kind][1]:
            worst[kind] = rec
        assert bool(torch.isfinite(hip).all()) and emax < tol, (kind, i, emax, tol)
        return ratio
    ratios = {}
    for kind, i in internet_keys():
        lay = INTERNET_SAVED[kind][2]
        hip = internet_saved_rows(rt, xg, kind, i).cpu().double()
        ratios[kind, i] = check(kind, i, hip, internet_ref_to_rows(L64[kind, i], lay, A), internet_ref_to_rows(L32[kind, i], lay, A))
    ratios["output", 0] = check("output", 0, y_tr.cpu().double(), y64, y32)
    for kind, (g, r, emax, emean, cmean) in worst.items():
        print(f"{geom} {kind}: max|err| {emax:.3e} ({g:.4f} of the gate) mean {emean:.3e}; fp32 CPU mean {cmean:.3e}; HIP / CPU {r:.2f}")
    bad = {k: round(v, 2) for k, v in ratios.items() if not v <= 8.0}
    assert not bad, bad


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


@pytest.mark.parametrize("geom", GUARD_ROWS, ids=lambda g: "A%ds%dB%dh%dw%d" % g)
def test_guard_bands_and_short_workspace(geom):
    A, s, B, h, w = geom
    sd, x = internet_case(*geom)
    rt = runtime(A, s, sd)
    lib, st = rt.lib, capi.stream_ptr()
    xg = dev(x)
    # ---- inference
    ws, n, out, n_out = _buffers(rt, geom, False)
    rc = lib.lfsr_internet_forward(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n - 1, st)
    torch.cuda.synchronize()
    assert rc == E_WS and bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    rc = lib.lfsr_internet_forward(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n, st)
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
    rc = lib.lfsr_internet_forward_train(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n - 1, st)
    torch.cuda.synchronize()
    assert rc == E_WS and bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    rc = lib.lfsr_internet_forward_train(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n, st)
    torch.cuda.synchronize()
    assert rc == 0
    assert _intact(ws, n // 4) and _intact(out, n_out) and torch.equal(out[:n_out], y.reshape(-1))
    rc = lib.lfsr_internet_backward(rt.ctx, xg.data_ptr(), dout.data_ptr(), B, h, w, ws.data_ptr(), n - 1, grads.data_ptr(), npar, st)
    torch.cuda.synchronize()
    assert rc == E_WS and bool((grads == SENTINEL).all())
    rc = lib.lfsr_internet_backward(rt.ctx, xg.data_ptr(), dout.data_ptr(), B, h, w, ws.data_ptr(), n, grads.data_ptr(), npar, st)
    torch.cuda.synchronize()
    assert rc == 0
    assert _intact(ws, n // 4) and _intact(grads, npar) and _intact(out, n_out)
    assert bool(torch.isfinite(grads[:npar]).all()) and bool((grads[:npar] != SENTINEL).all())      # every gradient element was written
    rt.forward_train(xg)
    ref = rt.backward(xg, dout)
    assert torch.equal(grads[:npar], ref)


@pytest.mark.parametrize("A,s", [(0, 2), (10, 2), (5, 1), (5, 5)])
def test_create_refuses_out_of_range(A, s):
    ctx = C.c_void_p()
    assert capi.load().lfsr_internet_create(C.byref(ctx), A, s, 4, 4) == E_ARG
    assert not ctx.value
    with pytest.raises(capi.LfsrError):
        capi.ModelRuntime("internet", A, s, 4, 4)


def test_three_groups_refused_before_any_launch():
    """the inference forward instantiates SpaBottle for 5 x 64 input channels only: a 3-group model is refused, and nothing has been written"""
    geom = (5, 2, 1, 8, 8)
    A, s, B, h, w = geom
    sd = synth_state_dict(internet_spec(A, s, n_groups=3), seed=0)
    rt = runtime(A, s, sd, n_groups=3)
    xg = dev(synth_input((B, 1, A * h, A * w), seed=1))
    ws, n, out, n_out = _buffers(rt, geom, False)
    rc = rt.lib.lfsr_internet_forward(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n, capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == E_ARG
    assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    assert rt.train_workspace_bytes(B, h, w) == 0               # and the training path covers 4 x 4 only


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
@geoms
def test_gradients_vs_fp64_under_the_hip_decisions(geom):
    """every parameter's gradient against fp64 autograd of the reference graph under the HIP forward's own ReLU decisions: rel-L2 < 1e-4 per
    parameter (the yardstick of test_gpu_internet_train.py::test_grads_match_reference_golden), no parameter and no element left out"""
    A, s, B, h, w = geom
    sd, x = internet_case(*geom)
    net, _ = make_net(A, s, sd)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    xg, lg = dev(x), dev(label)
    _, bucket, out = hip_step(net, xg, lg)
    assert torch.equal(torch.cat([p.grad.reshape(-1) for p in net.parameters()]), net.grad_bucket)
    assert bool(torch.isfinite(bucket).all())
    if s == 3 or B == 8:
        _, b2, o2 = hip_step(net, xg, lg)
        assert torch.equal(bucket, b2) and torch.equal(out, o2)
    net(xg)                                                    # the saved activations of this input (hip_step's were the same)
    forced, flips = forced_fp64_grads(net._rt, xg, sd, x, label, A, s)
    names = [k for k, _ in net.named_parameters()]
    assert names == [k for k, _ in internet_spec(A, s)] and sum(p.numel() for p in net.parameters()) == bucket.numel()
    errs = {k: rel(p.grad.detach().cpu().numpy(), forced[k]) for k, p in net.named_parameters()}
    v = np.array(list(errs.values()))
    print(f"{geom}: gradient rel-L2 vs fp64 median {np.median(v):.2e} max {v.max():.2e} ({max(errs, key=errs.get)}); "
          f"ReLU decisions differing from fp64's own: {flips}")
    bad = {k: e for k, e in errs.items() if not e < 1e-4}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# past 2 GiB
# ---------------------------------------------------------------------------------------------------------------------
def test_forward_batch_66_concat_past_2_gib():
    """5x5 views of 32x32 at x2, B = 66: the 320-wide concat of the spatial group outputs is 66 x 25 x 1024 x 320 x 4 = 2.163e9 B, the first
    batch past 2^31 bytes, and ModelRuntime sends it as ONE launch sequence (it splits by 256-float rows: at 82).  Every kernel on that path
    addresses with 64 bits there (the gather-GEMM's `else` branch, the row GEMMs hand over to it, the slice copies index with long long)."""
    A, s, B, h, w = 5, 2, 66, 32, 32
    assert B * A * A * h * w * 320 * 4 >= 1 << 31 > (B - 1) * A * A * h * w * 320 * 4
    assert capi.max_patches_per_launch(A, h, w, capi.ModelRuntime.widest_row_floats) >= B
    sd = synth_state_dict(internet_spec(A, s), seed=0)
    x = synth_input((B, 1, A * h, A * w), seed=1)
    rt = runtime(A, s, sd)
    xg = dev(x)
    n = rt._f("workspace_bytes")(rt.ctx, B, h, w)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = torch.full((B, 1, A * h * s, A * w * s), float("nan"), device="cuda")
    rc = rt.lib.lfsr_internet_forward(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n, capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    assert not bool(torch.isnan(out).any())                    # no value left unwritten
    del ws
    for i in (0, 32, 65):
        ref = O.internet_forward(x[i:i + 1], sd, A, s)
        tol = gate(ref)
        y = out[i:i + 1].cpu().numpy()
        y1 = rt.forward(xg[i:i + 1]).cpu().numpy()
        e, d = float(np.abs(y - ref).max()), float(np.abs(y - y1).max())
        print(f"B = 66 sample {i}: max|err| vs oracle {e:.3e}, vs its B = 1 forward {d:.3e}, gate {tol:.3e}")
        assert e < tol and d < tol, (i, e, d)
