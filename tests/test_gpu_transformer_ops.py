"""GPU: the EPIT / LFT operators that the whole-model tests reach only at a few geometries -- the up-sampling tail in all its kernel forms, the two-kernel
tail, LFT's 3x3 token embedding (lfsr_conv3x3_n_fwd), the 5x5 spatial window attention in the model's call shape and LayerNorm with its position term --
each against an fp64 reference built from the oracle's primitives, at ragged and tile-boundary geometries, with operands read out of wider buffers and
guard values around every output."""
import numpy as np
import pytest
import torch

from lfsr_amd import capi
from oracle import lfsr_oracle as O

pytestmark = pytest.mark.gpu
ATOL = 1e-4
SENTINEL = -2.0 ** 100        # guard value (exact in fp32): any write into a guard band changes it
F64 = np.float64


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def rnd(shape, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def wide(a, stride, choff, fill=float("nan")):
    """(rows, c) -> a (rows, stride) device buffer holding `a` in columns [choff, choff + c) and `fill` elsewhere"""
    buf = np.full((a.shape[0], stride), fill, np.float32)
    buf[:, choff:choff + a.shape[1]] = a
    return dev(buf)


# ---------------------------------------------------------------------------------------------------------------------
# up-sampling tail (EPIT.py:44-49, LFT.py:52-57): the last four lines of O.epit_forward / O.lft_forward
# ---------------------------------------------------------------------------------------------------------------------
def vcl_to_mosaic(f, B, A, h, w):
    """VCL rows [b][u][v][y][x] x 64 -> the SAI mosaic (B, 64, A h, A w)"""
    return f.reshape(B, A, A, h, w, -1).transpose(0, 5, 1, 3, 2, 4).reshape(B, -1, A * h, A * w)


def hr_pre_ref(f, w0, B, A, h, w, s):
    """PixelShuffle_s(conv1x1(F)) in fp64, NCHW (B, 64, A h s, A w s)"""
    return O.pixel_shuffle(O.conv2d(vcl_to_mosaic(f.astype(F64), B, A, h, w), w0.astype(F64)), s)


def hr_tail_ref(hr, w3, x, B, A, h, w, s, slope):
    """conv3x3(LeakyReLU(HR)) over the whole mosaic + the per-view bicubic skip, fp64"""
    up = O.conv2d(O.leaky_relu(hr, slope), w3.astype(F64), padding=(1, 1))
    lr = x.astype(F64).reshape(B, 1, A, h, A, w).transpose(0, 1, 2, 4, 3, 5)
    sr = O.interp_bicubic(lr.reshape(B * A * A, 1, h, w), s).reshape(B, 1, A, A, h * s, w * s)
    return up + sr.transpose(0, 1, 2, 4, 3, 5).reshape(B, 1, A * h * s, A * w * s)


def tail_operands(B, A, h, w, s, seed):
    f = rnd((B * A * A * h * w, 64), seed)
    w0 = rnd((64 * s * s, 64, 1, 1), seed + 1, 0.125)
    w3 = rnd((1, 64, 3, 3), seed + 2, 0.05)
    x = np.random.default_rng(seed + 3).random((B, 1, A * h, A * w)).astype(np.float32)
    return f, w0, w3, x


class Tail:
    """the device operands of one tail geometry; w0 packed as the runtimes pack upsampling.0 (perm 1, ch 64), w3 raw (1, 64, 3, 3)"""

    def __init__(self, f, w0, w3, x, B, A, h, w, s):
        self.B, self.A, self.h, self.w, self.s = B, A, h, w, s
        self.f = f
        self.w0p = capi.pack_conv_weight(dev(w0), perm=1, ch=64)
        self.w3d, self.xd = dev(w3), dev(x)
        self.n_out = B * A * h * s * A * w * s

    def up_tail(self, slope, f_stride=64, f_choff=0, guard=4096, s=None):
        """lfsr_up_tail_fwd into an output buffer with `guard` sentinel floats behind it -> (out (B,1,Hs,Ws), guard band), both numpy"""
        fd = wide(self.f, f_stride, f_choff)
        out = torch.full((self.n_out + guard,), SENTINEL, device="cuda")
        capi.check(capi.load().lfsr_up_tail_fwd(capi.dev_ptr(fd), f_stride, f_choff, capi.dev_ptr(self.w0p), capi.dev_ptr(self.w3d), capi.dev_ptr(self.xd),
                                                capi.dev_ptr(out), self.B, self.A, self.h, self.w, self.s if s is None else s, slope, capi.stream_ptr()), "up_tail")
        o = out.cpu().numpy()
        return o[:self.n_out].reshape(self.B, 1, self.A * self.h * self.s, self.A * self.w * self.s), o[self.n_out:]


# (B, A, h, w, slope): the mosaic ragged against the 4 x 32 LR tile in both directions, several tile columns, tiles straddling view borders; LeakyReLU slopes
# 0.2 (what EPIT / LFT pass) and 0.1
TAIL_GEOMS = [(1, 5, 8, 8, 0.2), (2, 3, 6, 8, 0.1), (1, 5, 32, 32, 0.2), (3, 2, 5, 7, 0.1), (1, 1, 37, 70, 0.2), (2, 7, 5, 9, 0.1)]
F_LAYOUTS = [(64, 0), (128, 0), (128, 64)]      # (f_stride, f_choff): the model's contiguous rows, and the operand as either half of 128-wide rows (other half NaN)


def tail_forms(s):
    """(name, LFSR_UPTAIL selector, arithmetic, three-term form?) of every kernel form lfsr_up_tail_fwd has at scale s"""
    forms = [("default", None, capi.ARITH_DEFAULT, True),          # k_up_tail3 at s = 2, k_up_tail4 at s = 4
             ("arith_f32", None, capi.ARITH_F32, False),           # k_up_tail2
             ("v1", "v1", capi.ARITH_DEFAULT, False)]              # k_up_tail
    if s == 4:
        forms.append(("uptail3", "3", capi.ARITH_DEFAULT, True))    # k_up_tail3<4>
    return forms


@pytest.mark.parametrize("s", [2, 4])
def test_up_tail_every_form_vs_fp64(s, monkeypatch):
    errs = {}
    try:
        for gi, (B, A, h, w, slope) in enumerate(TAIL_GEOMS):
            f, w0, w3, x = tail_operands(B, A, h, w, s, 100 + gi)
            ref = hr_tail_ref(hr_pre_ref(f, w0, B, A, h, w, s), w3, x, B, A, h, w, s, slope)
            T = Tail(f, w0, w3, x, B, A, h, w, s)
            for name, sel, arith, _ in tail_forms(s):
                if sel is None:
                    monkeypatch.delenv("LFSR_UPTAIL", raising=False)
                else:
                    monkeypatch.setenv("LFSR_UPTAIL", sel)
                capi.set_arithmetic(arith)
                for f_stride, f_choff in F_LAYOUTS:
                    y, guard = T.up_tail(slope, f_stride, f_choff)
                    err = np.abs(y - ref)
                    what = (name, (B, A, h, w), slope, f_stride, f_choff)
                    assert err.max() < ATOL, (what, float(err.max()))
                    assert np.all(guard == SENTINEL), what
                    if f_stride == 64:
                        errs.setdefault(name, []).append((err.mean(), err.max()))
    finally:
        capi.set_arithmetic(capi.ARITH_DEFAULT)
        monkeypatch.delenv("LFSR_UPTAIL", raising=False)
    # the three-term forms against the fp32-MFMA form (k_up_tail2) by tests/test_gpu_b3_accuracy.py's yardstick
    ef = np.array(errs["arith_f32"])
    for name, _, _, three in tail_forms(s):
        if three:
            e = np.array(errs[name])
            print(f"s={s} {name}: mean |err| {e[:, 0].mean():.2e} vs fp32 form {ef[:, 0].mean():.2e}; max {e[:, 1].max():.2e} vs {ef[:, 1].max():.2e}")
            assert e[:, 0].mean() <= 1.1 * ef[:, 0].mean(), name
            assert e[:, 1].max() <= 1.5 * ef[:, 1].max(), name


def test_up_tail_refusals_leave_output_untouched():
    """s = 3 (the fused tail has s in {2, 4}), f_stride < f_choff + 64 and f_choff % 4 != 0 are refused before any launch.  The buffers would hold even a
    wrongly accepted launch: 128-wide operand rows, weights and output sized for s = 4."""
    lib = capi.load()
    B, A, h, w = 1, 3, 6, 8
    T = Tail(*tail_operands(B, A, h, w, 4, 7), B, A, h, w, 4)           # (upsampling.0 packed for s = 4: the largest weight any of these calls could read)
    fd = wide(T.f, 128, 0, fill=1.0)
    out = torch.full((B * A * h * 4 * A * w * 4,), SENTINEL, device="cuda")
    for f_stride, f_choff, s in ((128, 0, 3), (64, 4, 2), (96, 64, 4), (128, 2, 2), (128, 62, 4)):
        with pytest.raises(capi.LfsrError):
            capi.check(lib.lfsr_up_tail_fwd(capi.dev_ptr(fd), f_stride, f_choff, capi.dev_ptr(T.w0p), capi.dev_ptr(T.w3d), capi.dev_ptr(T.xd), capi.dev_ptr(out),
                                            B, A, h, w, s, 0.2, capi.stream_ptr()), "up_tail")
        torch.cuda.synchronize()
        assert torch.all(out == SENTINEL), (f_stride, f_choff, s)


# ---------------------------------------------------------------------------------------------------------------------
# two-kernel tail: lfsr_upsample_ps_fwd (HR pre-activation, channel-last) + lfsr_hr_tail_fwd -- the tail at scale 3, under LFSR_NO_UPTAIL, and the HR map
# the LFT backward takes its LeakyReLU decisions from
# ---------------------------------------------------------------------------------------------------------------------
def upsample_ps(T, f_stride=64, f_choff=0, guard=4096):
    fd = wide(T.f, f_stride, f_choff)
    Hs, Ws = T.A * T.h * T.s, T.A * T.w * T.s
    n = T.B * Hs * Ws * 64
    hr = torch.full((n + guard,), SENTINEL, device="cuda")
    capi.check(capi.load().lfsr_upsample_ps_fwd(capi.dev_ptr(fd), f_stride, f_choff, capi.dev_ptr(T.w0p), capi.dev_ptr(hr), T.B, T.A, T.h, T.w, T.s,
                                                capi.stream_ptr()), "upsample_ps")
    return hr[:n].reshape(T.B, Hs, Ws, 64), hr[n:].cpu().numpy()


def hr_tail(T, hr, slope, guard=4096):
    out = torch.full((T.n_out + guard,), SENTINEL, device="cuda")
    capi.check(capi.load().lfsr_hr_tail_fwd(capi.dev_ptr(hr), capi.dev_ptr(T.w3d), capi.dev_ptr(T.xd), capi.dev_ptr(out), T.B, T.A, T.h, T.w, T.s, slope,
                                            capi.stream_ptr()), "hr_tail")
    o = out.cpu().numpy()
    return o[:T.n_out].reshape(T.B, 1, T.A * T.h * T.s, T.A * T.w * T.s), o[T.n_out:]


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("B,A,h,w", [(2, 3, 6, 8), (1, 5, 7, 13)])
def test_upsample_ps_vs_fp64(B, A, h, w, s):
    f, w0, w3, x = tail_operands(B, A, h, w, s, 200 + s)
    T = Tail(f, w0, w3, x, B, A, h, w, s)
    ref = hr_pre_ref(f, w0, B, A, h, w, s).transpose(0, 2, 3, 1)          # channel-last (B, A h s, A w s, 64)
    for f_stride, f_choff in F_LAYOUTS:
        hr, guard = upsample_ps(T, f_stride, f_choff)
        assert np.abs(hr.cpu().numpy() - ref).max() < ATOL, (f_stride, f_choff)
        assert np.all(guard == SENTINEL)


@pytest.mark.parametrize("s", [2, 3, 4])
@pytest.mark.parametrize("slope", [0.2, 0.1])
def test_hr_tail_vs_fp64(s, slope):
    B, A, h, w = 2, 3, 5, 7
    f, w0, w3, x = tail_operands(B, A, h, w, s, 300 + s)
    T = Tail(f, w0, w3, x, B, A, h, w, s)
    hr = rnd((B, A * h * s, A * w * s, 64), 310 + s)
    y, guard = hr_tail(T, dev(hr), slope)
    ref = hr_tail_ref(hr.astype(F64).transpose(0, 3, 1, 2), w3, x, B, A, h, w, s, slope)
    assert np.abs(y - ref).max() < ATOL
    assert np.all(guard == SENTINEL)


@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("B,A,h,w", [(1, 5, 8, 8), (3, 2, 5, 7)])
def test_two_kernel_tail_equals_fused_tail(B, A, h, w, s):
    f, w0, w3, x = tail_operands(B, A, h, w, s, 400 + s)
    T = Tail(f, w0, w3, x, B, A, h, w, s)
    hr, _ = upsample_ps(T)
    y2, _ = hr_tail(T, hr.contiguous(), 0.2)
    y1, _ = T.up_tail(0.2)
    assert np.abs(y1 - y2).max() < ATOL


# ---------------------------------------------------------------------------------------------------------------------
# lfsr_conv3x3_n_fwd: LFT's unfold(3x3) + Linear(576 -> N) token embedding (LFT.py:176-182) == a per-view zero-padded 3x3 conv 64 -> N
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [128, 96, 40])            # Npad 128 / 96 / 64: launch_gemm's two-column-tile (Npad % 64 == 0) and one-column-tile instantiations
@pytest.mark.parametrize("slope", [1.0, 0.2])
@pytest.mark.parametrize("n_img,h,w", [(1, 32, 32), (3, 7, 13), (2, 9, 5)])
def test_conv3x3_n_vs_fp64(n_img, h, w, N, slope):
    lib = capi.load()
    x = rnd((n_img * h * w, 64), 500 + N)
    wt = rnd((N, 64, 3, 3), 501 + N, 0.05)
    wp = capi.pack_conv_weight(dev(wt))
    z = O.conv2d(x.astype(F64).reshape(n_img, h, w, 64).transpose(0, 3, 1, 2), wt.astype(F64), padding=(1, 1))
    ref = (z if slope == 1.0 else O.leaky_relu(z, slope)).transpose(0, 2, 3, 1).reshape(n_img * h * w, N)
    for (xs, xc), (ys, yc) in (((64, 0), (N, 0)), ((128, 64), (256, 128))):
        xd = wide(x, xs, xc)
        y = torch.full((n_img * h * w + 16, ys), SENTINEL, device="cuda")      # 16 guard rows after the output
        capi.check(lib.lfsr_conv3x3_n_fwd(capi.dev_ptr(xd), xs, xc, capi.dev_ptr(wp), capi.dev_ptr(y), ys, yc, n_img, h, w, N, slope, capi.stream_ptr()), "conv3x3_n")
        yh = y.cpu().numpy()
        assert np.abs(yh[:n_img * h * w, yc:yc + N] - ref).max() < ATOL, (xs, xc, ys, yc)
        keep = np.ones(yh.shape, bool)
        keep[:n_img * h * w, yc:yc + N] = False
        assert np.all(yh[keep] == SENTINEL), (xs, xc, ys, yc)


# ---------------------------------------------------------------------------------------------------------------------
# spatial window attention (LFT.py:161-199): 8 heads of 16, 5 x 5 window with the column window clamped by h (LFT.py:168)
# ---------------------------------------------------------------------------------------------------------------------
E, NH = 128, 8


def window_attn_ref(q, k, v, n, h, w, chunk=4):
    """fp64 attention of every query over the keys of its window [i-2, i+3) x [j-2, min(j+3, h, w)), gathered (25 candidates per query).  A query whose
    window is empty (j >= h + 2) gives NaN, as softmax over the reference's all -inf mask row does."""
    hd = E // NH
    ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    offs = [(di, dj) for di in range(-2, 3) for dj in range(-2, 3)]
    KI = np.stack([ii + di for di, _ in offs], -1).reshape(h * w, 25)
    KJ = np.stack([jj + dj for _, dj in offs], -1).reshape(h * w, 25)
    valid = (KI >= 0) & (KI < h) & (KJ >= 0) & (KJ < min(h, w))
    kidx = (np.clip(KI, 0, h - 1) * w + np.clip(KJ, 0, w - 1)).reshape(-1)
    out = np.empty((n, h * w, NH, hd))
    with np.errstate(invalid="ignore"):
        for i0 in range(0, n, chunk):
            c = min(chunk, n - i0)
            sl = slice(i0 * h * w, (i0 + c) * h * w)
            qq, kk, vv = [t[sl].astype(F64).reshape(c, h * w, NH, hd) for t in (q, k, v)]
            kg = kk[:, kidx].reshape(c, h * w, 25, NH, hd)
            vg = vv[:, kidx].reshape(c, h * w, 25, NH, hd)
            S = np.einsum("cpnd,cpknd->cpnk", qq, kg) / np.sqrt(hd)
            S = np.where(valid[None, :, None, :], S, -np.inf)
            Pm = np.exp(S - S.max(-1, keepdims=True))
            Pm /= Pm.sum(-1, keepdims=True)
            out[i0:i0 + c] = np.einsum("cpnk,cpknd->cpnd", Pm, vg)
    return out.reshape(n * h * w, E)


def dense_attn_ref(q, k, v, n, h, w):
    """the reference's own form: dense scores with O.lft_gen_mask's additive -inf mask (LFT.py:161-174)"""
    hd = E // NH
    mask = O.lft_gen_mask(h, w, 5, F64)

    def heads(t):
        return t.astype(F64).reshape(n, h * w, NH, hd).transpose(0, 2, 1, 3)
    with np.errstate(invalid="ignore"):
        S = heads(q) @ heads(k).transpose(0, 1, 3, 2) / np.sqrt(hd) + mask
        Pm = np.exp(S - S.max(-1, keepdims=True))
        Pm /= Pm.sum(-1, keepdims=True)
    return (Pm @ heads(v)).transpose(0, 2, 1, 3).reshape(n * h * w, E)


@pytest.mark.parametrize("n,h,w", [(3, 6, 8), (2, 7, 13), (2, 13, 7)])
def test_windowed_reference_equals_dense_masked_form(n, h, w):
    q, k, v = [rnd((n * h * w, E), s) for s in (21, 22, 23)]
    a, b = window_attn_ref(q, k, v, n, h, w), dense_attn_ref(q, k, v, n, h, w)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    assert np.nanmax(np.abs(a - b)) < 1e-12


def spatial_attn(q, k, v, n, h, w, o_stride=256, o_choff=64):
    """the call lft.cpp makes: q | k interleaved in one 256-wide buffer (k at column 128), v at stride 128; o into a 128-column slice of wider rows"""
    lib = capi.load()
    qk = dev(np.concatenate([q, k], axis=1))
    vd = dev(v)
    o = torch.full((n * h * w + 8, o_stride), SENTINEL, device="cuda")
    capi.check(lib.lfsr_window_attn_fwd(capi.dev_ptr(qk), 256, 0, capi.dev_ptr(qk), 256, 128, capi.dev_ptr(vd), 128, 0, capi.dev_ptr(o), o_stride, o_choff, NH, E // NH,
                                        n, 1, 1, h * w, 0, 0, h, w, w, 1, 2, 3, 2, 3, h, capi.stream_ptr()), "spatial attn")
    oh = o.cpu().numpy()
    keep = np.ones(oh.shape, bool)
    keep[:n * h * w, o_choff:o_choff + E] = False
    assert np.all(oh[keep] == SENTINEL)
    return oh[:n * h * w, o_choff:o_choff + E]


def check_attn(o, ref):
    assert np.array_equal(np.isnan(o), np.isnan(ref))
    assert np.nanmax(np.abs(o - ref)) < 1e-5


# (n_img, h, w):
#   (25, 32, 32): four strips of 8 query rows per image, 100 (image, strip) pairs -- not a multiple of 8, so the units go in plain order;
#   (8, 32, 32): 8 images x 4 strips = nblk 32 pairs, 32 x 8 heads = 256 units and a grid of min(2 x CUs, 256) = 256 blocks: nblk % 8 == 0 and
#                grid % 8 == 0, so k_win_attn_mfma takes the XCD-range remap (p.remap = 1);
#   (3, 13, 7): ragged strips (13 = 8 + 5 rows) and a column clamp h = 13 beyond n2 = 7 (clip2 > n2: the image edge bounds the window);
#   (2, 7, 13): clip2 = h = 7 < n2 = 13: the clamp cuts the window, and queries in columns 9 .. 12 see no key at all (NaN, as in the reference);
#   (1, 9, 40): n2 > 32 -- k_win_attn_mfma refuses it and the LDS-tiled VALU kernel k_window_attn_lds<16, 2> runs.
@pytest.mark.parametrize("n,h,w", [(25, 32, 32), (8, 32, 32), (3, 13, 7), (2, 7, 13), (1, 9, 40)])
def test_spatial_window_attention_model_call_shape(n, h, w, monkeypatch):
    monkeypatch.delenv("LFSR_ATTN", raising=False)
    monkeypatch.delenv("LFSR_ATTN_L1", raising=False)
    q, k, v = [rnd((n * h * w, E), s) for s in (31, 32, 33)]
    check_attn(spatial_attn(q, k, v, n, h, w), window_attn_ref(q, k, v, n, h, w))


@pytest.mark.parametrize("sel", [("LFSR_ATTN", "valu"), ("LFSR_ATTN_L1", "1")])   # the LDS-tiled VALU kernel / the one-thread-per-(query, head) kernel
def test_spatial_window_attention_valu_forms(sel, monkeypatch):
    n, h, w = 3, 13, 7
    monkeypatch.setenv(*sel)
    q, k, v = [rnd((n * h * w, E), s) for s in (41, 42, 43)]
    check_attn(spatial_attn(q, k, v, n, h, w), window_attn_ref(q, k, v, n, h, w))


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm with the position term (LFT.py:190-197, 236-241): pe[(row / pe_div) % pe_rows], strided slices, past the grid cap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,M", [(64, 140001), (128, 70001), (64, 1000), (128, 999)])   # the large M: past 8192 blocks x (16 | 8) rows, the grid-stride loop runs
@pytest.mark.parametrize("pe_form", ["none", "ang", "spa"])
def test_layernorm_position_term_and_slices(C, M, pe_form):
    lib = capi.load()
    A, h, w = 5, 7, 13
    x = (rnd((M, C), 61, 2.0) + rnd((M, 1), 62)).astype(np.float32)
    g, b = (1 + 0.3 * rnd((C,), 63)).astype(np.float32), rnd((C,), 64, 0.2)
    if pe_form == "ang":           # LFT's AngTrans: one PE row per view, rows of a view contiguous (pe_rows = A^2, pe_div = h w)
        pe_rows, pe_div = A * A, h * w
    elif pe_form == "spa":         # LFT's SpaTrans: one PE row per position of a view (pe_rows = h w, pe_div = 1)
        pe_rows, pe_div = h * w, 1
    else:
        pe_rows, pe_div = 0, 1
    pe = rnd((max(pe_rows, 1), C), 65)
    ped = wide(pe, C + 16, 0)
    x_stride, x_choff, y_stride, y_choff = C + 64, 32, C + 128, 64
    xd, gd, bd = wide(x, x_stride, x_choff), dev(g), dev(b)
    y = torch.full((M + 8, y_stride), SENTINEL, device="cuda")
    capi.check(lib.lfsr_layernorm_fwd(capi.dev_ptr(xd), x_stride, x_choff, capi.dev_ptr(ped) if pe_rows else None, C + 16, pe_rows, pe_div,
                                      capi.dev_ptr(gd), capi.dev_ptr(bd), capi.dev_ptr(y), y_stride, y_choff, M, C, 1e-5, capi.stream_ptr()), "layernorm")
    xr = x.astype(F64)
    if pe_rows:
        xr = xr + pe.astype(F64)[(np.arange(M) // pe_div) % pe_rows]
    ref = O.layer_norm(xr, g.astype(F64), b.astype(F64))
    yh = y.cpu().numpy()
    assert np.abs(yh[:M, y_choff:y_choff + C] - ref).max() < 1e-5
    keep = np.ones(yh.shape, bool)
    keep[:M, y_choff:y_choff + C] = False
    assert np.all(yh[keep] == SENTINEL)
