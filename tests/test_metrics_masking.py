"""N2 / N3.  CPU part: the oracle's SSIM restatement against scipy's gaussian_filter (the routine skimage calls;
skimage itself is not installed, so the reference's cal_metrics cannot be run here: SSIM parity is pinned on scipy only).
GPU part: device metrics and view masking against the oracle / the reference's slice-assignment semantics."""
import random
from argparse import Namespace

import numpy as np
import pytest
import torch

from oracle import lfsr_oracle as O


def test_oracle_gauss_matches_scipy():
    nd = pytest.importorskip("scipy.ndimage")
    img = np.random.default_rng(0).random((37, 29))
    assert np.abs(O._gauss11(img) - nd.gaussian_filter(img, sigma=1.5, truncate=3.5, mode="reflect")).max() < 1e-14


def test_oracle_ssim_identity_and_psnr():
    x = np.random.default_rng(1).random((1, 1, 2 * 16, 2 * 20))
    ps, ss = O.view_psnr_ssim(x, x, 2)
    assert np.isinf(ps).all() and np.allclose(ss, 1.0)
    y = x + 0.1
    ps, _ = O.view_psnr_ssim(x, y, 2)
    assert np.allclose(ps, 20.0)


@pytest.mark.gpu
def test_device_metrics_vs_oracle():
    from lfsr_amd import capi
    from lfsr_amd.utils.metrics import cal_metrics, view_metrics
    rng = np.random.default_rng(2)
    for (B, A, H, W) in [(2, 5, 128, 128), (1, 3, 24, 40), (1, 2, 11, 11)]:
        lab = rng.random((B, 1, A * H, A * W)).astype(np.float32)
        out = np.clip(lab + 0.05 * rng.standard_normal(lab.shape).astype(np.float32), 0, 1)
        ps, ss = view_metrics(torch.from_numpy(lab).cuda(), torch.from_numpy(out).cuda(), A)
        rps, rss = O.view_psnr_ssim(lab, out, A)
        assert np.abs(ps.cpu().numpy() - rps).max() < 1e-9
        assert np.abs(ss.cpu().numpy() - rss).max() < 1e-10
        pm, sm = cal_metrics(Namespace(angRes_in=A, task="SR"), torch.from_numpy(lab).cuda(), torch.from_numpy(out).cuda())
        assert abs(pm - rps.mean()) < 1e-9 and abs(sm - rss.mean()) < 1e-10
    with pytest.raises(capi.LfsrError):
        view_metrics(torch.zeros(1, 1, 10, 10, device="cuda"), torch.zeros(1, 1, 10, 10, device="cuda"), 2)   # 5x5 views < 11x11 window


def _vm_tile():
    """(VM_TR, VM_TW): the output rows and columns of one SSIM tile of k_view_metrics, read from the kernel's source so that the rows
    below which straddle a tile edge move with it"""
    import os
    import re
    from lfsr_amd import PKG_DIR
    src = open(os.path.join(PKG_DIR, "csrc", "metrics.hip")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % n, src).group(1)) for n in ("VM_TR", "VM_TW"))


VM_TR, VM_TW = _vm_tile()
# (B, A, H, W) of the views.  The SSIM map of an H x W view is (H - 10) x (W - 10); the kernel walks it in VM_TR x VM_TW tiles.
METRIC_SHAPES = {
    "TR8_ragged_rows": (1, 2, 27, 160),       # the row tiles the W-dependent LDS layout took up to width 349: 8 rows, the last tile ragged
    "TR4": (1, 1, 23, 214),
    "TR2": (1, 1, 13, 300),
    "TR1_w349": (1, 1, 12, 349),              # the last width that layout accepted
    "w350_two_rows": (1, 1, 12, 350),         # the first it refused; two output rows
    "w625_one_row_B2": (2, 2, 11, 625),       # the widest baseline view; one output row; B > 1
    "one_column": (1, 1, 434, 11),            # tall and narrow: one output column
    "real_view": (1, 1, 432, 624),            # one view of real size
    # one tile: a row and a column short of it, exactly it, one over
    "tile_minus1": (1, 1, 10 + VM_TR - 1, 10 + VM_TW - 1),
    "tile_exact": (1, 1, 10 + VM_TR, 10 + VM_TW),
    "tile_plus1": (1, 1, 10 + VM_TR + 1, 10 + VM_TW + 1),
    # two tiles each way, and the two edges against each other (rows over / columns short and the reverse)
    "two_tiles_minus1": (1, 2, 10 + 2 * VM_TR - 1, 10 + 2 * VM_TW - 1),
    "two_tiles_exact": (1, 1, 10 + 2 * VM_TR, 10 + 2 * VM_TW),
    "two_tiles_plus1": (1, 1, 10 + 2 * VM_TR + 1, 10 + 2 * VM_TW + 1),
    "rows_plus1_cols_minus1": (1, 1, 10 + VM_TR + 1, 10 + VM_TW - 1),
    "rows_minus1_cols_plus1": (1, 1, 10 + VM_TR - 1, 10 + VM_TW + 1),
}
_METRIC_CASES = {}


def _metric_case(name):
    """(label, out, per-view PSNR, per-view SSIM) of METRIC_SHAPES[name]: fp32 mosaics and the oracle's fp64 values, computed once"""
    if name not in _METRIC_CASES:
        B, A, H, W = METRIC_SHAPES[name]
        rng = np.random.default_rng(sorted(METRIC_SHAPES).index(name) + 20)
        lab = rng.random((B, 1, A * H, A * W)).astype(np.float32)
        out = np.clip(lab + 0.05 * rng.standard_normal(lab.shape).astype(np.float32), 0, 1)
        _METRIC_CASES[name] = (lab, out) + O.view_psnr_ssim(lab, out, A)
    return _METRIC_CASES[name]


def _mean_pos(v):
    """cal_metrics' mean (utils/utils.py:126-131): the sum over all views divided by the number of views whose value is > 0"""
    n = int((v > 0).sum())
    return float(v.sum() / n) if n > 0 else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(METRIC_SHAPES))
def test_device_metrics_any_view_size(name):
    """lfsr_view_metrics at every row tile of the former layout, past its width limit, and on both sides of every tile edge of the present one:
    per-view values against the oracle under the gates of test_device_metrics_vs_oracle, cal_metrics against the reference's means, nothing
    written outside the B*A*A doubles, two calls bit-equal, a host label (train.py:296,322) equal to a device label, and the PSNR-only form"""
    from lfsr_amd import capi
    from lfsr_amd.utils.metrics import cal_metrics, view_metrics
    B, A, H, W = METRIC_SHAPES[name]
    lab, out, rps, rss = _metric_case(name)
    lab_h, lab_d, out_d = torch.from_numpy(lab), torch.from_numpy(lab).cuda(), torch.from_numpy(out).cuda()
    ps, ss = view_metrics(lab_d, out_d, A)
    dps, dss = np.abs(ps.cpu().numpy() - rps).max(), np.abs(ss.cpu().numpy() - rss).max()
    print(f"{name} {METRIC_SHAPES[name]}: max |dPSNR| {dps:.2e}, max |dSSIM| {dss:.2e}")
    assert ps.shape == (B, A, A) and ss.shape == (B, A, A) and ps.dtype == torch.float64
    assert dps < 1e-9
    assert dss < 1e-10
    pm, sm = cal_metrics(Namespace(angRes_in=A, task="SR"), lab_d, out_d)
    assert abs(pm - _mean_pos(rps)) < 1e-9 and abs(sm - _mean_pos(rss)) < 1e-10
    # sentinel-filled buffers with a guard band either side, through the C ABI
    n, G, fill = B * A * A, 64, -12345.5
    pbuf, sbuf = (torch.full((G + n + G,), fill, dtype=torch.float64, device="cuda") for _ in range(2))
    capi.check(capi.load().lfsr_view_metrics(capi.dev_ptr(lab_d), capi.dev_ptr(out_d), capi.dev_ptr(pbuf[G:G + n]), capi.dev_ptr(sbuf[G:G + n]),
                                             B, A, H, W, capi.stream_ptr()), "view_metrics")
    for buf, want in ((pbuf, ps), (sbuf, ss)):
        assert torch.equal(buf[G:G + n], want.reshape(-1))                 # a second call: the same bits
        assert bool((buf[:G] == fill).all()) and bool((buf[G + n:] == fill).all())
    ps_h, ss_h = view_metrics(lab_h, out_d, A)                             # host label, moved to out's device
    assert ps_h.is_cuda and torch.equal(ps_h, ps) and torch.equal(ss_h, ss)
    assert cal_metrics(Namespace(angRes_in=A, task="SR"), lab_h, out_d) == (pm, sm)
    ps_only, none = view_metrics(lab_d, out_d, A, want_ssim=False)         # ssim == nullptr
    assert none is None and torch.equal(ps_only, ps)


@pytest.mark.gpu
def test_device_identity_host_inputs_and_refusals():
    from lfsr_amd import capi
    from lfsr_amd.utils.metrics import cal_metrics, view_metrics
    lab, out, _, _ = _metric_case("w350_two_rows")
    x = torch.from_numpy(out).cuda()
    ps, ss = view_metrics(x, x.clone(), 1)                                 # identical label and output at a wide shape
    assert bool(torch.isinf(ps).all()) and bool((ps > 0).all()) and float((ss - 1.0).abs().max()) < 1e-10      # the SSIM gate: 1 up to round-off
    # no CPU fallback: a host output raises whatever the label is, and nothing is computed on the host
    for label in (torch.from_numpy(lab), torch.from_numpy(lab).cuda()):
        with pytest.raises(capi.LfsrError):
            view_metrics(label, torch.from_numpy(out), 1)
        with pytest.raises(capi.LfsrError):
            cal_metrics(Namespace(angRes_in=1, task="SR"), label, torch.from_numpy(out))
    from lfsr_amd.utils.utils import ycbcr2rgb_views
    y, cc = torch.from_numpy(out[0, 0]), torch.from_numpy(np.stack([lab[0, 0], out[0, 0]]))
    want = ycbcr2rgb_views(y.cuda(), cc.cuda(), 1)
    assert want.is_cuda and torch.equal(ycbcr2rgb_views(y.cuda(), cc, 1), want)       # host Sr_SAI_cbcr (train.py:297,332): moved to y's device
    for c in (cc, cc.cuda()):
        with pytest.raises(capi.LfsrError):
            ycbcr2rgb_views(y, c, 1)                                                  # host Sr_SAI_y: no CPU fallback
    # views below the 11 x 11 window: SSIM is refused before anything is written, on either side; the PSNR-only form takes them as before
    rng = np.random.default_rng(40)
    for (A, H, W) in [(2, 10, 350), (2, 350, 10), (2, 5, 5)]:
        a = rng.random((1, 1, A * H, A * W)).astype(np.float32)
        b = np.clip(a + 0.05 * rng.standard_normal(a.shape).astype(np.float32), 0, 1)
        ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        n, fill = A * A, -12345.5
        pbuf, sbuf = (torch.full((n,), fill, dtype=torch.float64, device="cuda") for _ in range(2))
        rc = capi.load().lfsr_view_metrics(capi.dev_ptr(ad), capi.dev_ptr(bd), capi.dev_ptr(pbuf), capi.dev_ptr(sbuf), 1, A, H, W, capi.stream_ptr())
        torch.cuda.synchronize()
        assert rc == -1 and bool((pbuf == fill).all()) and bool((sbuf == fill).all())
        ps_only, _ = view_metrics(ad, bd, A, want_ssim=False)
        d = (a.astype(np.float64) - b.astype(np.float64)) ** 2
        ref = 10 * np.log10(1.0 / d.reshape(A, H, A, W).mean(axis=(1, 3)))
        assert np.abs(ps_only.cpu().numpy()[0] - ref).max() < 1e-9


def _aux():
    import json
    import os
    from tests.helpers import GOLDEN
    return json.load(open(os.path.join(GOLDEN, "aux.json"))), np.load(os.path.join(GOLDEN, "aux.npz"))


def test_mask_view_selection_matches_reference_sequence():
    """host logic (no GPU): under the same ``random.seed`` the plan of 8 training-mode calls -- skip decisions and chosen views -- equals
    what the reference's MaskedAngularPretraining produced (tests/golden/aux.json, generated by running the reference)."""
    from lfsr_amd.utils.masked_pretraining import MaskedAngularPretraining, ProgressiveMasking
    meta, _ = _aux()
    mm = meta["masking"]
    for case, calls in mm["cases"].items():
        strategy, value = case.split("_")
        m = MaskedAngularPretraining(angRes=mm["A"], mask_ratio=mm["mask_ratio"], mask_strategy=strategy, mask_value=value).train()
        random.seed(mm["python_random_seed"])
        got = [m.plan() for _ in range(mm["calls"])]
        assert [None if g is None else [list(v) for v in g] for g in got] == calls, case
    pm = ProgressiveMasking(angRes=mm["A"], start_ratio=0.1, end_ratio=0.4, warmup_epochs=20)
    for ep, ratio, n in mm["progressive"]:
        pm.set_epoch(ep)
        assert pm.masker.mask_ratio == ratio and pm.masker.num_masked == n


def test_oracle_color_vs_reference_vectors():
    """N4 oracle pinned on the reference's own rgb2ycbcr / ycbcr2rgb (utils/utils.py:181-204) driven as train.py:332-334 does"""
    from lfsr_amd.utils.utils import rgb2ycbcr
    meta, arr = _aux()
    for key, c in meta["ycbcr"]["cases"].items():
        got = O.sr_views_rgb_u8(arr["ycc_y_" + key].astype(np.float64), arr["ycc_cbcr_" + key].astype(np.float64), c["A"])
        assert np.array_equal(got, arr["rgb_u8_" + key]), key
    assert np.array_equal(rgb2ycbcr(arr["rgb_in"]), arr["ycbcr_of_rgb"])


@pytest.mark.gpu
def test_device_masking_vs_reference_vectors():
    """zero / mean (single and multi-view: every view its own mean) outputs against the tensors the reference produced; 'noise' keeps the
    unmasked views and draws N(0, 0.1^2) in the masked ones"""
    import hashlib
    from lfsr_amd.synth import synth_input
    from lfsr_amd.utils.masked_pretraining import MaskedAngularPretraining
    meta, arr = _aux()
    mm = meta["masking"]
    A, h, w = mm["A"], mm["h"], mm["w"]
    x = torch.from_numpy(synth_input((mm["B"], 1, A * h, A * w), seed=mm["input_seed"])).cuda()
    for case, calls in mm["cases"].items():
        strategy, value = case.split("_")
        m = MaskedAngularPretraining(angRes=A, mask_ratio=mm["mask_ratio"], mask_strategy=strategy, mask_value=value).train()
        random.seed(mm["python_random_seed"])
        for c, idx in enumerate(calls):
            y, info = m(x)
            if idx is None:
                assert y is x and not info["masked"]
                continue
            assert [list(v) for v in info["mask_indices"]] == idx
            if value == "zero":
                assert hashlib.sha256(np.ascontiguousarray(y.cpu().numpy()).tobytes()).hexdigest() == mm["zero_sha256"][f"{strategy}_{c}"]
            else:
                assert np.abs(y.cpu().numpy() - arr[f"mask_{strategy}_{value}_{c}"]).max() < 1e-6, (case, c)
    m = MaskedAngularPretraining(angRes=A, mask_ratio=0.3, mask_strategy="grid", mask_value="noise").train()
    random.seed(1)
    y, info = None, {"masked": False}
    while not info["masked"]:
        y, info = m(x)
    keep = torch.ones(A, A, dtype=torch.bool)
    for (i, j) in info["mask_indices"]:
        keep[i, j] = False
        v = y[:, :, i * h:(i + 1) * h, j * w:(j + 1) * w]
        assert abs(float(v.mean())) < 0.05 and 0.05 < float(v.std()) < 0.2
    full = keep.repeat_interleave(h, 0).repeat_interleave(w, 1).cuda()
    assert torch.equal(y[:, :, full], x[:, :, full])


@pytest.mark.gpu
def test_device_masking_matches_reference_semantics():
    from lfsr_amd.utils.masked_pretraining import MaskedAngularPretraining, ProgressiveMasking
    A, h, w = 5, 6, 8
    x = torch.rand(3, 1, A * h, A * w, device="cuda")
    for strategy in ("random", "grid", "corners", "center"):
        m = MaskedAngularPretraining(angRes=A, mask_ratio=0.3, mask_strategy=strategy).train()
        random.seed(4)
        applied = 0
        for _ in range(8):
            y, info = m(x)
            if not info["masked"]:
                assert y is x
                continue
            applied += 1
            ref = x.clone()
            for (i, j) in info["mask_indices"]:            # masked_pretraining.py:112-120
                ref[:, :, i * h:(i + 1) * h, j * w:(j + 1) * w] = 0
            assert torch.equal(y, ref)
            assert (A // 2, A // 2) not in info["mask_indices"]
            assert len(info["mask_indices"]) == min(max(1, int(25 * 0.3)), 4 if strategy == "corners" else 24)
        assert applied > 0
    m.eval()
    assert m(x)[0] is x                                   # train-time only
    pm = ProgressiveMasking(angRes=A, start_ratio=0.1, end_ratio=0.3, warmup_epochs=10)
    pm.set_epoch(5)
    assert pm.masker.num_masked == max(1, int(25 * 0.2))


# ---- N4: YCbCr -> RGB uint8 views + BMP files (train.py:329-341) -------------------------------------------------------------
def _read_bmp(path):
    import struct
    b = open(path, "rb").read()
    assert b[:2] == b"BM"
    off = struct.unpack("<I", b[10:14])[0]
    w, h, planes, bpp = struct.unpack("<iiHH", b[18:30])
    assert planes == 1 and bpp == 24 and h > 0
    row = (w * 3 + 3) // 4 * 4
    body = np.frombuffer(b, dtype=np.uint8, count=row * h, offset=off).reshape(h, row)[:, :w * 3].reshape(h, w, 3)
    return body[::-1, :, ::-1]   # bottom-up BGR -> top-down RGB


def test_oracle_ycbcr_roundtrip_and_bmp_writer(tmp_path):
    from lfsr_amd.utils.utils import rgb2ycbcr, write_bmp, save_views_bmp
    rng = np.random.default_rng(7)
    rgb = rng.random((9, 13, 3))
    ycc = rgb2ycbcr(rgb)
    assert np.abs(O.ycbcr2rgb(ycc) - rgb).max() < 1e-12          # the two reference formulas are inverses
    img = (rng.random((7, 5, 3)) * 255).astype(np.uint8)         # odd width: row padding
    write_bmp(str(tmp_path / "a.bmp"), img)
    assert np.array_equal(_read_bmp(str(tmp_path / "a.bmp")), img)
    views = (rng.random((2, 3, 4, 6, 3)) * 255).astype(np.uint8)
    save_views_bmp(tmp_path / "scene", views)
    assert np.array_equal(_read_bmp(str(tmp_path / "scene" / "View_1_2.bmp")), views[1, 2])


@pytest.mark.gpu
def test_device_ycbcr2rgb_views_vs_oracle():
    """bit-exact uint8 against the reference's float64 numpy arithmetic, incl. values on both sides of the clip"""
    from lfsr_amd.utils.utils import ycbcr2rgb_views
    rng = np.random.default_rng(8)
    for (A, h, w) in [(5, 32, 32), (3, 7, 10), (2, 128, 96)]:
        y = (rng.random((A * h, A * w)) * 1.2 - 0.1).astype(np.float32)
        cc = (rng.random((2, A * h, A * w)) * 1.2 - 0.1).astype(np.float32)
        got = ycbcr2rgb_views(torch.from_numpy(y)[None, None].cuda(), torch.from_numpy(cc)[None].cuda(), A).cpu().numpy()
        ref = O.sr_views_rgb_u8(y.astype(np.float64), cc.astype(np.float64), A)
        assert got.shape == (A, A, h, w, 3) and np.array_equal(got, ref)
    meta, arr = _aux()      # and against the uint8 views the reference itself produced (train.py:332-334 on utils.py:191-204)
    for key, c in meta["ycbcr"]["cases"].items():
        got = ycbcr2rgb_views(torch.from_numpy(arr["ycc_y_" + key])[None, None].cuda(), torch.from_numpy(arr["ycc_cbcr_" + key])[None].cuda(), c["A"])
        assert np.array_equal(got.cpu().numpy(), arr["rgb_u8_" + key]), key
