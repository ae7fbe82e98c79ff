"""GPU: LFSSR's HIP path against fp64 across angular resolutions, scales, view shapes and batch sizes, layer by layer.

The geometry matrix (tests/lfssr_helpers.py:LFSSR_MATRIX) reaches what the three golden geometries (angRes 5, 3, 2 with views of at most 8x8) and the one 32x32 patch do
not: the banded launches of the angular kernel (angRes 6..9, bands of 4 / 3 / 2 / 2 view rows with a short last band at 6, 7 and 9) chained twenty layers deep with the
spatial conv, the up-sampling conv and the tail; even angRes 4 and scale 4 on a banded grid; the second, partial pass of the grid-stride loops of k_lfssr_ps2 and
k_lfssr_tail; the workspace layout with nothing behind it but sentinels and nothing in it but NaN; the 3x3 selector forms on a conv with no activation, whose bias and ReLU
wait for the next kernel's prologue; the reduced-precision modes at every angRes; and the batch at which the four 64 -> 64 convs of fup2 pass the 1 GiB that the F(4x4)
kernel covers.  The reference is the fp64 graph of tests/lfssr_helpers.py:lfssr_layers, pinned on the reference model by tests/test_lfssr_reference.py.

Measured figures: profiles/lfssr_geometry_tests.md."""
import functools

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from lfsr_amd.synth import synth_input
from tests import lfssr_helpers as H
from tests.helpers import YARDSTICK, arithmetic
from tests.test_gpu_ang_bf16 import whole_model_gates
from tests.test_gpu_lfssr import case, dev, gate, hip_layers, runtime

pytestmark = pytest.mark.gpu
ids = lambda g: "A%ds%dB%dh%dw%d" % g
geoms = pytest.mark.parametrize("geom", H.LFSSR_MATRIX, ids=ids)
GUARD_ROWS = ((7, 2, 1, 5, 6), (4, 4, 2, 6, 5), (3, 4, 1, 33, 28))
SELECTOR_ROWS = ((7, 2, 1, 5, 6), (3, 4, 1, 33, 28))
SENTINEL = -2.0 ** 100
BAND = 1 << 16            # floats behind every buffer
E_WS = -2
torch.set_num_threads(min(torch.get_num_threads(), 16))


@functools.lru_cache(maxsize=None)
def matrix_case(geom):
    """-> state_dict, input, the fp64 layers (computed once, shared, never written to)"""
    sd, x = H.lfssr_matrix_case(*geom)
    return sd, x, H.lfssr_layers(x, sd, geom[0], geom[1])


def test_the_last_row_wraps_both_grid_stride_loops():
    """the launch-cap arithmetic the matrix relies on, so that the row cannot silently stop covering the wrap (the ragged last pass with dead lanes in the butterfly is
    tests/test_gpu_lfssr_ops.py's)"""
    A, s, B, h, w = H.LFSSR_MATRIX[-1]
    rows2 = B * A * A * (2 * h) * (2 * w)                        # level 2: the rows k_lfssr_ps2 reads, a quarter of the pixels k_lfssr_tail writes
    assert rows2 * 64 == 16 * 4 * rows2 == 2128896 > H.GRID_CAP_ITEMS
    assert rows2 * 64 - H.GRID_CAP_ITEMS == 124 * 256            # the second pass is partial: 124 of the 8192 blocks
    assert B * A * A * (2 * h) * (2 * (w - 1)) * 64 <= H.GRID_CAP_ITEMS and B * A * A * (2 * (h - 1)) * (2 * w) * 64 <= H.GRID_CAP_ITEMS      # one row or column less: none
    for g in H.LFSSR_MATRIX[:-1]:                                # and no other row wraps
        assert g[2] * g[0] * g[0] * g[3] * g[4] * (4 if g[1] == 4 else 1) * 64 <= H.GRID_CAP_ITEMS, g


# ---------------------------------------------------------------------------------------------------------------------
# a. the output against fp64 under both fp32 arithmetics
# ---------------------------------------------------------------------------------------------------------------------
@geoms
def test_output_vs_fp64_both_arithmetics(geom):
    A, s, B, h, w = geom
    sd, x, ref = matrix_case(geom)
    want = ref["out"].numpy()
    tol = gate(want)
    rt = runtime(A, s, sd)
    xg = dev(x)
    for mode, name in ((capi.ARITH_DEFAULT, "default"), (capi.ARITH_F32, "f32")):
        with arithmetic(mode):
            yg = rt.forward(xg).clone()
            singles = torch.cat([rt.forward(xg[i:i + 1]).clone() for i in range(B)], 0) if B > 1 else None
        y = yg.cpu().numpy()
        assert y.shape == want.shape == (B, 1, A * h * s, A * w * s)
        err = np.abs(y - want)
        print(f"LFSSRGEO | {geom} | {name} | out | max {err.max():.3e} | mean {err.mean():.3e} | gate {tol:.3e} | share {err.max() / tol:.4f} | max|ref| {np.abs(want).max():.3f}")
        assert np.isfinite(y).all() and err.max() < tol
        if singles is not None:                                  # a sample's bits do not depend on the batch (tests/test_gpu_lfssr.py asserts it at angRes 2)
            assert torch.equal(yg, singles), name


# ---------------------------------------------------------------------------------------------------------------------
# b. every named intermediate against fp64
# ---------------------------------------------------------------------------------------------------------------------
@geoms
def test_every_named_layer_vs_fp64(geom):
    """the LAYER_NAMES present at scale s, rebuilt from the operator entry points in the driver's order (the chain's output is the driver's, bit for bit): each under the
    gate 1e-4 max(1, max|ref tensor|), and its mean error at most helpers.YARDSTICK x that of the same graph in fp32 torch on the CPU"""
    A, s, B, h, w = geom
    sd, x, ref = matrix_case(geom)
    cpu = H.lfssr_layers(x, sd, A, s, dtype=torch.float32)
    y = runtime(A, s, sd).forward(dev(x)).cpu()
    L = hip_layers(sd, x, A, s, B, h, w)
    names = [n for n in H.LAYER_NAMES if n in ref]
    assert sorted(L) == sorted(ref) == sorted(names) and len(names) == (6 if s == 2 else 8)
    assert torch.equal(L["out"], y)
    over = {}
    for name in names:
        rows = (lambda t: t) if name == "out" else H.views_to_rows
        got, want, c32 = L[name].double(), rows(ref[name]), rows(cpu[name]).double()
        assert got.shape == want.shape, name
        tol = 1e-4 * max(1.0, float(want.abs().max()))
        e = (got - want).abs()
        e_max, e_mean, e_cpu = float(e.max()), float(e.mean()), float((c32 - want).abs().mean())
        ratio = e_mean / e_cpu if e_cpu > 0 else (0.0 if e_mean == 0 else float("inf"))
        print(f"LFSSRGEO | {geom} | layer | {name} | max {e_max:.3e} | mean {e_mean:.3e} | gate {tol:.3e} | share {e_max / tol:.4f} | e_cpu {e_cpu:.3e} | ratio {ratio:.2f}")
        assert bool(torch.isfinite(got).all()) and e_max < tol, (name, e_max, tol)          # the gate admits no exception
        if not ratio <= YARDSTICK and (geom, name) not in H.LFSSR_YARDSTICK_EXEMPT:
            over[name] = round(ratio, 2)
    assert not over, over


# ---------------------------------------------------------------------------------------------------------------------
# c. guard bands, the exact workspace, nothing read before it is written
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GUARD_ROWS, ids=ids)
def test_guard_bands_exact_workspace_and_nan_workspace(geom):
    A, s, B, h, w = geom
    sd, x, _ = matrix_case(geom)
    rt = runtime(A, s, sd)
    lib, st = rt.lib, capi.stream_ptr()
    xg = dev(x)
    n = lib.lfsr_lfssr_workspace_bytes(rt.ctx, B, h, w)
    assert n > 0 and n % 4 == 0
    ws = torch.full((n // 4 + BAND,), SENTINEL, device="cuda")
    n_out = B * A * h * s * A * w * s
    out = torch.full((n_out + BAND,), SENTINEL, device="cuda")
    assert ws.data_ptr() % 16 == 0

    def forward(nbytes):
        rc = lib.lfsr_lfssr_forward(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), nbytes, st)
        torch.cuda.synchronize()
        return rc
    assert forward(n - 1) == E_WS
    assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    assert forward(n) == 0
    assert bool((ws[n // 4:] == SENTINEL).all()) and bool((out[n_out:] == SENTINEL).all())
    y = rt.forward(xg)
    assert torch.equal(out[:n_out], y.reshape(-1))
    # no workspace float is read before the forward writes it: a NaN in every one of them, and the same bits come out
    first = out[:n_out].clone()
    ws[:n // 4] = float("nan")
    out[:n_out] = SENTINEL
    assert forward(n) == 0
    assert bool((ws[n // 4:] == SENTINEL).all()) and bool((out[n_out:] == SENTINEL).all())
    assert bool(torch.isfinite(out[:n_out]).all())
    assert torch.equal(out[:n_out], first)


# ---------------------------------------------------------------------------------------------------------------------
# d. the 3x3 selector forms on LFSSR's convs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel", ["halo", "gather", "wino2"])
@pytest.mark.parametrize("geom", SELECTOR_ROWS, ids=ids)
def test_selector_forms(geom, sel, monkeypatch):
    """LFSR_CONV3X3 on the spatial conv of every AltFilter (slope 1, no bias: bias and ReLU are the angular kernel's prologue) and on the four sub-pixel convs of fup"""
    A, s, B, h, w = geom
    sd, x, ref = matrix_case(geom)
    want = ref["out"].numpy()
    rt = runtime(A, s, sd)
    xg = dev(x)
    monkeypatch.delenv("LFSR_CONV3X3", raising=False)
    before = rt.forward(xg).clone()
    monkeypatch.setenv("LFSR_CONV3X3", sel)
    y = rt.forward(xg).clone()
    monkeypatch.delenv("LFSR_CONV3X3")
    after = rt.forward(xg).clone()
    err = np.abs(y.cpu().numpy() - want)
    print(f"LFSSRGEO | {geom} | LFSR_CONV3X3={sel} | out | max {err.max():.3e} | mean {err.mean():.3e} | gate {gate(want):.3e} | "
          f"equal to the unselected forward: {torch.equal(y, before)}")
    assert bool(torch.isfinite(y).all()) and err.max() < gate(want)
    assert torch.equal(after, before)


# ---------------------------------------------------------------------------------------------------------------------
# e. the bf16 modes across the matrix
# ---------------------------------------------------------------------------------------------------------------------
@geoms
def test_bf16_modes(geom):
    A, s, B, h, w = geom
    sd, x, ref = matrix_case(geom)
    whole_model_gates(ids(geom), A, s, sd, x, ref["out"].numpy())


# ---------------------------------------------------------------------------------------------------------------------
# f. past 1 GiB
# ---------------------------------------------------------------------------------------------------------------------
def test_forward_batch_11_fup2_past_1_gib():
    """5x5 views of 32x32 at x4, B = 11: the four 64 -> 64 convs of fup2 write a 256-float-stride tensor of 11 x 25 x 64 x 64 rows, 2^30 bytes and more, which
    lfsr_conv3x3_wino4_launch declines, so they run on the halo kernel, while every other conv of the forward stays on F(4x4).  LFSSRRuntime sends the batch as ONE launch
    sequence (it splits at 2 GiB: B = 21), which is what sr_scene does with a minibatch above 10."""
    (A, h, w, s, _), sd, x0, ref = case("full")
    B = 11
    assert (A, h, w, s) == (5, 32, 32, 4)
    assert 11 * 25 * 64 * 64 * 256 * 4 >= 1 << 30 > 10 * 25 * 64 * 64 * 256 * 4
    assert capi.max_patches_per_launch(5, 32, 32, 1024) >= 11
    rt = runtime(A, s, sd)
    assert rt.widest_row_floats == 1024 and rt.offset_limit == 1 << 31
    x = np.concatenate([x0] + [synth_input((1, 1, A * h, A * w), seed=100 + i) for i in range(1, B)], 0)
    xg = dev(x)
    n = rt.lib.lfsr_lfssr_workspace_bytes(rt.ctx, B, h, w)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = torch.full((B, 1, A * h * s, A * w * s), float("nan"), device="cuda")
    rc = rt.lib.lfsr_lfssr_forward(rt.ctx, xg.data_ptr(), out.data_ptr(), B, h, w, ws.data_ptr(), n, capi.stream_ptr())
    torch.cuda.synchronize()
    del ws                                                       # about 3.3 GB
    torch.cuda.empty_cache()
    assert rc == 0
    assert not bool(torch.isnan(out).any())                      # no value left unwritten
    want = ref["out"].numpy()
    e = float(np.abs(out[:1].cpu().numpy() - want).max())
    print(f"LFSSRGEO | B = 11 | sample 0 | every pixel vs fp64 {e:.3e} | gate {gate(want):.3e} | workspace {n / 1e9:.2f} GB")
    assert e < gate(want)
    for i in (5, 10):
        y1 = rt.forward(xg[i:i + 1]).cpu().numpy()
        d = float(np.abs(out[i:i + 1].cpu().numpy() - y1).max())
        print(f"LFSSRGEO | B = 11 | sample {i} | vs its B = 1 forward {d:.3e} | gate {gate(y1):.3e}")
        assert d < gate(y1), (i, d)
