"""GPU: the forward operator entry points of DistgSSR (lfsr_conv3x3_fwd, lfsr_epiconv_fwd / _hv_fwd, lfsr_angconv_fwd, lfsr_pointwise_fwd,
lfsr_initconv_fwd, lfsr_fold_head + lfsr_upsample_head_fwd) in every selectable kernel form, element by element against the fp64 numpy oracle
(oracle/lfsr_oracle.py) on the fp32 operands widened to fp64.  The forward-side counterpart of tests/test_gpu_bwd_ops.py.

Every value comparison (tests/helpers.py::fwd_op_gate) holds the project's gate max|err| <= 1e-4 * max(1, max|ref|) and a yardstick: the HIP mean
error is at most 8 x the mean error of the same operator evaluated in fp32 on the CPU with stock torch ops on the same operands (the ratio
tests/test_gpu_distgssr_geometries.py asserts for whole-model tensors).  Every ratio is printed (`FWDOP ...` lines, pytest -s);
profiles/distgssr_forward_op_tests.md holds the worst per form.

Operands are unit-variance normal + 0.5 (a wrong zero padding shows).  Inputs sit at a channel offset inside wider rows whose foreign columns
hold +-1e3, between NaN rows in front of row 0 and behind row M - 1 of the same allocation; outputs sit inside wider rows of random finite
values followed by sentinel rows, and every float outside the written channel range must keep its bits.  Entry points are called through
capi.load() wherever the capi wrappers cannot express an operand (x_choff, residual strides, tmp = NULL)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lfsr_amd import capi
from oracle import lfsr_oracle as O
from tests.helpers import (arithmetic, fwd_op_gate, macpi_to_rows, op_input, op_output, op_output_read, set_selectors)

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)

E_ARG = -1
SELECTORS = ("LFSR_CONV3X3", "LFSR_CONV_TAIL", "LFSR_CONV_NOTAIL", "LFSR_CONV_NOHALF", "LFSR_EPI", "LFSR_EPI_ORDER", "LFSR_ANG", "LFSR_ROWGEMM", "LFSR_NO_ROWGEMM",
             "LFSR_B3_NB")
P = capi.dev_ptr


def _select(monkeypatch, **env):
    set_selectors(monkeypatch, SELECTORS, **env)


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _data(g, *shape):
    return torch.randn(*shape, generator=g) + 0.5


def _lrelu(v, slope):
    """the activation of every entry point here: v >= 0 ? v : slope * v, any slope (slope 1: none)"""
    return torch.where(v >= 0, v, v * slope)


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# =====================================================================================================================
# lfsr_conv3x3_fwd
# =====================================================================================================================
# (n_img, h, w): views smaller than one F(4x4) tile (8 x 32 pixels); one aligned tile; ALIGNED with two tile columns and two tile rows; one past
# the tile both ways; ragged views of several tiles; 300 tiles on 256 CUs (a second persistent round, the half-tile remainder of the F(4x4)
# kernel, the channel-split tail launch of the F(2x2) and halo kernels)
C3_ROWS = [(3, 1, 1), (2, 1, 37), (2, 9, 1), (5, 3, 5), (3, 8, 32), (2, 16, 64), (2, 9, 33), (7, 13, 40), (2, 33, 70), (300, 8, 32)]
C3_SELS = ["", "wino2", "halo", "gather"]
# form -> (slope, r1, r2).  Slopes outside [0, 1) take the select epilogue (ACT == 2 of k_conv3x3_wino4)
C3_FORMS = {"lrelu0.1": (0.1, 0, 0), "lrelu0.1+r1": (0.1, 1, 0), "lrelu0.1+r1+r2": (0.1, 1, 1), "linear+r1+r2": (1.0, 1, 1), "linear+r2": (1.0, 0, 1),
            "relu": (0.0, 0, 0), "lrelu0.2": (0.2, 0, 0), "slope2.0": (2.0, 0, 0), "slope-0.5": (-0.5, 0, 0), "slope2.0+r1+r2": (2.0, 1, 1)}
# x at offset 16 of an 80-float row, y at offset 64 of a 144-float row (the concat buffer of the three-kernel block path), r1 dense, r2 at 8 of 72
C3_LAYOUT = {"x": (80, 16), "y": (144, 64), "r1": (64, 0), "r2": (72, 8)}


@functools.lru_cache(maxsize=None)
def _c3_case(n_img, h, w):
    """fp32 operands of one 64 -> 64 per-view 3x3 conv and its pre-activation in fp64 (oracle) and in fp32 (stock torch on the CPU), as VCL rows"""
    g = torch.Generator().manual_seed(7000 + 131 * n_img + 17 * h + w)
    x = _data(g, n_img, 64, h, w)
    wt = torch.randn(64, 64, 3, 3, generator=g) * 0.05
    r1, r2 = _data(g, n_img, 64, h, w), _data(g, n_img, 64, h, w)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, 64).contiguous()
    pre64 = rows(_t64(O.conv2d(x.double().numpy(), wt.double().numpy(), padding=(1, 1))))
    pre32 = rows(F.conv2d(x, wt, padding=1))
    return {"x": rows(x), "wt": wt, "r1": rows(r1), "r2": rows(r2), "pre64": pre64, "pre32": pre32}


def _c3_refs(case, form):
    slope, use1, use2 = C3_FORMS[form]
    ref, cpu = _lrelu(case["pre64"], slope), _lrelu(case["pre32"], slope)
    for use, k in ((use1, "r1"), (use2, "r2")):
        if use:
            ref, cpu = ref + case[k].double(), cpu + case[k]
    return ref, cpu


class _C3Run:
    """the device operands of one conv case under one layout; run(form) -> the 64 output channels (footprint checked)"""

    def __init__(self, geom, lay=C3_LAYOUT):
        self.geom, self.lay, self.case = geom, lay, _c3_case(*geom)
        self.wp = capi.pack_conv_weight(self.case["wt"].cuda())
        self.x, self.r1, self.r2 = (op_input(self.case[k], *lay[k], seed=i) for i, k in enumerate(("x", "r1", "r2")))
        self.y = op_output(self.case["x"].shape[0], lay["y"][0], seed=3)

    def launch(self, form, x=None, y=None):
        slope, use1, use2 = C3_FORMS[form]
        x, y = x or (self.x.ptr, *self.lay["x"]), y or (self.y.ptr, *self.lay["y"])
        n_img, h, w = self.geom
        return capi.load().lfsr_conv3x3_fwd(*x, P(self.wp), *y, self.r1.ptr if use1 else None, *(self.lay["r1"] if use1 else (0, 0)),
                                            self.r2.ptr if use2 else None, *(self.lay["r2"] if use2 else (0, 0)), n_img, h, w, slope, capi.stream_ptr())

    def run(self, form):
        self.y.reset()
        capi.check(self.launch(form), "conv3x3_fwd")
        return op_output_read(self.y, self.lay["y"][1], 64)


@pytest.mark.parametrize("sel", C3_SELS)
@pytest.mark.parametrize("n_img,h,w", C3_ROWS)
def test_conv3x3_every_row_selection_and_form(n_img, h, w, sel, monkeypatch):
    """the whole cross product: ten rows x four selections x ten epilogue forms, r1 and r2 different tensors at strides of their own"""
    _select(monkeypatch, LFSR_CONV3X3=sel)
    run = _C3Run((n_img, h, w))
    for form in C3_FORMS:
        got = run.run(form)
        ref, cpu = _c3_refs(run.case, form)
        fwd_op_gate(got, ref, cpu, "conv3x3", f"{sel or 'default'} {form}", (n_img, h, w))


def test_conv3x3_selected_forms_differ(monkeypatch):
    """LFSR_CONV3X3 really changes the kernel: F(4x4,3x3), F(2x2,3x3) and the direct 9-tap form are three different roundings of the same sums, in the plain
    form and through the two-residual epilogue, and each of them differs from the gather-GEMM's.  halo and gather are both direct sums: tap by tap, k ascending, on
    v_mfma_f32_32x32x2_f32 from a zero accumulator, the same epilogue arithmetic -- the same bits, pinned as such (a difference cannot be asserted for this pair)"""
    run = _C3Run((7, 13, 40))
    for form in ("lrelu0.1", "lrelu0.1+r1+r2", "slope2.0"):
        out = {}
        for sel in C3_SELS:
            _select(monkeypatch, LFSR_CONV3X3=sel)
            out[sel] = run.run(form)
        assert not _bits_equal(out[""], out["wino2"]) and not _bits_equal(out[""], out["halo"]) and not _bits_equal(out["wino2"], out["halo"]), form
        assert not _bits_equal(out[""], out["gather"]) and not _bits_equal(out["wino2"], out["gather"]), form
        assert _bits_equal(out["halo"], out["gather"]), form


@pytest.mark.parametrize("which", ["y", "r1", "r2"])
def test_conv3x3_unaligned_operand_runs_the_gather_gemm(which, monkeypatch):
    """y, r1 or r2 at a channel offset of 2: no 16-byte channel vectors, so whatever is selected the gather-GEMM runs -- the same bits under all four selections, the
    bits LFSR_CONV3X3=gather gives on aligned operands, and right"""
    geom = (7, 13, 40)
    lay = dict(C3_LAYOUT, **{which: (C3_LAYOUT[which][0] + 2, C3_LAYOUT[which][1] + 2)})
    run, form = _C3Run(geom, lay), "lrelu0.1+r1+r2"
    ref, cpu = _c3_refs(run.case, form)
    got = []
    for sel in C3_SELS:
        _select(monkeypatch, LFSR_CONV3X3=sel)
        got.append(run.run(form))
        fwd_op_gate(got[-1], ref, cpu, "conv3x3", f"{sel or 'default'} {which}+2 (gather-GEMM)", geom)
    assert all(_bits_equal(got[0], o) for o in got[1:])
    _select(monkeypatch, LFSR_CONV3X3="gather")
    assert _bits_equal(_C3Run(geom).run(form), got[0])
    _select(monkeypatch)
    assert not _bits_equal(_C3Run(geom).run(form), got[0])          # aligned, the default is the F(4x4) kernel


def test_conv3x3_fp32_arithmetic_changes_no_bit(monkeypatch):
    """include/lfsr_hip.h: the 3x3 convs compute on fp32 MFMA in either arithmetic"""
    _select(monkeypatch)
    for geom in ((7, 13, 40), (3, 8, 32)):
        run = _C3Run(geom)
        for form in ("lrelu0.1+r1+r2", "slope-0.5"):
            base = run.run(form)
            with arithmetic(capi.ARITH_F32):
                assert _bits_equal(run.run(form), base), (geom, form)


# =====================================================================================================================
# lfsr_epiconv_fwd / lfsr_epiconv_hv_fwd
# =====================================================================================================================
# (B, A, h, w).  Fused geometries (A odd, A <= 5, h, w <= 32), LINES = 8 EPI lines a tile: item-major block order when A h and A w are multiples of 8
EPI_A5 = [(1, 5, 8, 8),        # item-major, grid 10: no XCD swizzle
          (4, 5, 8, 8),        # grid 40: with the swizzle
          (1, 5, 8, 16),       # 5 and 10 tiles per item
          (1, 5, 17, 9),       # ragged last group, pass-major order
          (1, 5, 1, 1),        # the smallest fused view
          (1, 5, 3, 32)]       # a full-width view
EPI_A13 = [(2, 3, 6, 8), (1, 3, 8, 8), (2, 1, 9, 7)]        # k_epi_fused<0>
EPI_GATHER = [(1, 7, 5, 6), (1, 2, 6, 6), (1, 4, 5, 7), (1, 5, 33, 8), (1, 5, 8, 33), (1, 9, 4, 4)]      # outside the fused kernels: two gather-GEMM launches a pass
EPI_X = (80, 16)


def epi_kernel(geom, sel="", f32=False, slope=0.1):
    """the kernel behind lfsr_epiconv_fwd / _hv_fwd on 16-byte aligned outputs, read from distg_branch.cpp (lfsr_epi_run, the chain behind both entry points) and the launchers it names (epi_b3.hip, epi_fused.hip)"""
    _, A, h, w = geom
    if sel == "gather" or not (A % 2 == 1 and A <= 5 and h <= 32 and w <= 32):
        return "gather-GEMM"
    if A != 5:
        return "k_epi_fused<0>"
    if sel == "direct":
        return "k_epi_fused<5>"
    return "k_epi_wino5" if sel == "wino" or f32 or not 0.0 <= slope <= 1.0 else "epi_b3"


def _ps1d(x, f):      # DistgSSR.py:114-131
    B, fC, Hh, Ww = x.shape
    return x.reshape(B, f, fC // f, Hh, Ww).permute(0, 2, 3, 4, 1).reshape(B, fC // f, Hh, Ww * f)


@functools.lru_cache(maxsize=None)
def _epi_case(B, A, h, w, slope=0.1):
    """EPIConv (DistgSSR.py:91-97) on the MacPI tensor and on its transpose (:108): outputs and stage-1 activations as the entry points lay them out, fp64 (oracle)
    and fp32 (stock torch on the CPU)"""
    g = torch.Generator().manual_seed(8000 + 1000 * B + 100 * A + 10 * h + w)
    x = _data(g, B, 64, h * A, w * A)
    w1 = torch.randn(32, 64, 1, A * A, generator=g) * 0.03
    w2 = torch.randn(32 * A, 32, 1, 1, generator=g) * 0.15
    pad = A * (A - 1) // 2

    def ref(t):
        e = O.leaky_relu(O.conv2d(t, w1.double().numpy(), stride=(1, A), padding=(0, pad)), slope)
        return _t64(e), _t64(O.pixel_shuffle1d(O.leaky_relu(O.conv2d(e, w2.double().numpy()), slope), A))

    def cpu(t):
        e = _lrelu(F.conv2d(t, w1, stride=(1, A), padding=(0, pad)), slope)
        return e, _ps1d(_lrelu(F.conv2d(e, w2), slope), A)
    out = {"x": macpi_to_rows(x, A), "w1": w1, "w2": w2}
    for tag, f, xin, xt in (("64", ref, x.double().numpy(), np.ascontiguousarray(x.double().numpy().transpose(0, 1, 3, 2))), ("32", cpu, x, x.transpose(2, 3).contiguous())):
        e_h, y_h = f(xin)
        e_v, y_v = f(xt)
        out["yh" + tag], out["yv" + tag] = macpi_to_rows(y_h, A), macpi_to_rows(y_v.transpose(2, 3), A)
        out["eh" + tag] = e_h.reshape(B, 32, h, A, w).permute(0, 3, 2, 4, 1).reshape(-1, 32).contiguous()      # rows (b A + u, y, x): include/lfsr_hip.h, e_h
        out["ev" + tag] = e_v.reshape(B, 32, w, A, h).permute(0, 3, 4, 2, 1).reshape(-1, 32).contiguous()      # rows (b A + v, y, x): e_v
    return out


class _EpiRun:
    def __init__(self, geom, slope=0.1, y_stride=144):
        self.geom, self.slope, self.case = geom, slope, _epi_case(*geom, slope)
        B, A, h, w = geom
        self.w1p, self.w2p = capi.pack_conv_weight(self.case["w1"].cuda()), capi.pack_conv_weight(self.case["w2"].cuda())
        self.x = op_input(self.case["x"], *EPI_X, seed=1)
        self.y = op_output(B * A * A * h * w, y_stride, seed=2)
        self.t = op_output(B * A * h * w, 32, seed=3)

    def single(self, vertical, choff=112, tmp=True):
        """lfsr_epiconv_fwd -> (rc, y channels, tmp rows)"""
        B, A, h, w = self.geom
        self.y.reset(); self.t.reset()
        rc = capi.load().lfsr_epiconv_fwd(self.x.ptr, *EPI_X, P(self.w1p), P(self.w2p), self.t.ptr if tmp else None, self.y.ptr, self.y.stride, choff, B, A, h, w,
                                          int(vertical), self.slope, capi.stream_ptr())
        return rc, op_output_read(self.y, choff, 32 if rc == 0 else 0), op_output_read(self.t, 0, 32 if rc == 0 and tmp else 0)

    def both(self, choff_h=80, choff_v=112, tmp=True):
        """lfsr_epiconv_hv_fwd -> (rc, horizontal channels, vertical channels); tmp is scratch there"""
        B, A, h, w = self.geom
        self.y.reset(); self.t.reset()
        rc = capi.load().lfsr_epiconv_hv_fwd(self.x.ptr, *EPI_X, P(self.w1p), P(self.w2p), self.t.ptr if tmp else None, self.y.ptr, self.y.stride, choff_h, choff_v,
                                             B, A, h, w, self.slope, capi.stream_ptr())
        torch.cuda.synchronize()
        if rc:
            return rc, op_output_read(self.y, 0, 0), op_output_read(self.t, 0, 0)
        if tmp:       # include/lfsr_hip.h: tmp is scratch here -- the fused kernels leave it alone, the gather-GEMM path leaves the vertical pass's stage-1 activation
            gather = epi_kernel(self.geom, os.environ.get("LFSR_EPI", ""), slope=self.slope) == "gather-GEMM" or (self.y.stride | choff_h | choff_v) & 3
            t = op_output_read(self.t, 0, 32 if gather else 0)
            if gather:
                fwd_op_gate(t, self.case["ev64"], self.case["ev32"], "epiconv_hv tmp", "[gather-GEMM] v", self.geom)
        lo, hi = min(choff_h, choff_v), max(choff_h, choff_v)
        got = op_output_read(self.y, lo, hi + 32 - lo, holes=((lo + 32, hi),))
        return rc, got[:, choff_h - lo:choff_h - lo + 32].contiguous(), got[:, choff_v - lo:choff_v - lo + 32].contiguous()

    def check_all(self, sel, f32=False):
        """both single passes (output and tmp) and the two-pass call, every value against fp64; -> their bits"""
        c, geom = self.case, self.geom
        form = f"{'ARITH_F32' if f32 else sel or 'default'}{'' if self.slope == 0.1 else f' slope {self.slope}'} [{epi_kernel(geom, sel, f32, self.slope)}]"
        bits = {}
        for v, k in ((0, "h"), (1, "v")):
            rc, y, t = self.single(v)
            capi.check(rc, "epiconv_fwd")
            fwd_op_gate(y, c["y" + k + "64"], c["y" + k + "32"], "epiconv", f"{form} {k}", geom)
            fwd_op_gate(t, c["e" + k + "64"], c["e" + k + "32"], "epiconv tmp", f"{form} {k}", geom)
            bits[k], bits["t" + k] = y, t
        rc, yh, yv = self.both()
        capi.check(rc, "epiconv_hv_fwd")
        fwd_op_gate(yh, c["yh64"], c["yh32"], "epiconv_hv", f"{form} h", geom)
        fwd_op_gate(yv, c["yv64"], c["yv32"], "epiconv_hv", f"{form} v", geom)
        bits["hv_h"], bits["hv_v"] = yh, yv
        return bits


def _same(a, b, keys=None):
    return all(_bits_equal(a[k], b[k]) for k in (keys or a))


@pytest.mark.parametrize("B,A,h,w", EPI_A5)
def test_epiconv_angres5_every_form(B, A, h, w, monkeypatch):
    """the fused geometries at angRes 5 under LFSR_EPI unset (epi_b3.hip: three-term bf16), wino (k_epi_wino5), direct (k_epi_fused<5>), gather (two gather-GEMM
    launches a pass) and under ARITH_F32, which is documented to run the fp32-MFMA kernel LFSR_EPI=wino names"""
    run, bits = _EpiRun((B, A, h, w)), {}
    for sel in ("", "wino", "direct", "gather"):
        _select(monkeypatch, LFSR_EPI=sel)
        bits[sel] = run.check_all(sel)
    _select(monkeypatch)
    with arithmetic(capi.ARITH_F32):
        bits["f32"] = run.check_all("", f32=True)
    assert _same(bits["f32"], bits["wino"])
    for sel in bits:                           # one launch for both passes or one launch a pass: the same kernel on the same tiles
        assert _bits_equal(bits[sel]["h"], bits[sel]["hv_h"]) and _bits_equal(bits[sel]["v"], bits[sel]["hv_v"]), sel
    if (B, A, h, w) == (4, 5, 8, 8):      # enough values that two different roundings cannot agree everywhere
        for a, b in (("", "wino"), ("", "direct"), ("", "gather"), ("wino", "direct"), ("wino", "gather")):
            assert not _bits_equal(bits[a]["hv_h"], bits[b]["hv_h"]) and not _bits_equal(bits[a]["v"], bits[b]["v"]), (a, b)
        assert not _bits_equal(bits["direct"]["hv_h"], bits["gather"]["hv_h"]) and not _bits_equal(bits["direct"]["v"], bits["gather"]["v"])


@pytest.mark.parametrize("B,A,h,w", EPI_A13)
def test_epiconv_angres1_and_3_every_form(B, A, h, w, monkeypatch):
    """k_epi_fused<0> (LFSR_EPI unset; there is no three-term form below angRes 5, so ARITH_F32 runs the same kernel: equal bits) and LFSR_EPI=gather"""
    run, bits = _EpiRun((B, A, h, w)), {}
    for sel in ("", "gather"):
        _select(monkeypatch, LFSR_EPI=sel)
        bits[sel] = run.check_all(sel)
    _select(monkeypatch)
    with arithmetic(capi.ARITH_F32):
        assert _same(run.check_all("", f32=True), bits[""])
    if A == 3:        # 9 taps summed per line position in the fused kernel's order against the gather-GEMM's: other bits
        assert not _bits_equal(bits[""]["hv_h"], bits["gather"]["hv_h"]) and not _bits_equal(bits[""]["v"], bits["gather"]["v"])
    else:             # angRes 1: one tap, K = 64 summed k ascending by both -- the same bits; test_epiconv_selector_reaches_the_named_launcher tells the two apart
        assert _same(bits[""], bits["gather"])


@pytest.mark.parametrize("B,A,h,w", EPI_GATHER)
def test_epiconv_gather_only_geometries(B, A, h, w, monkeypatch):
    """angRes 7 and 9, even angRes, views past 32 pixels on either side: the gather-GEMM path whatever is selected"""
    _select(monkeypatch)
    run = _EpiRun((B, A, h, w))
    base = run.check_all("")
    _select(monkeypatch, LFSR_EPI="direct")
    assert _same(run.check_all("direct"), base)


@pytest.mark.parametrize("B,A,h,w", [(1, 5, 8, 8), (4, 5, 8, 8), (1, 5, 8, 16), (1, 3, 8, 8)])
def test_epiconv_hv_block_order_changes_no_bit(B, A, h, w, monkeypatch):
    """LFSR_EPI_ORDER reaches lfsr_epi_f32_launch (k_epi_wino5, k_epi_fused<5>, k_epi_fused<0>) for the two-pass call on geometries whose lines fill whole
    tiles: unset = item-major blocks with the XCD swizzle when the grid is a multiple of 8, `item` = item-major without it, `pass` = pass-major.  Only which block
    computes which tile changes: equal bits, and right.  epi_b3.hip (the default at angRes 5) does not read it"""
    run = _EpiRun((B, A, h, w))
    c = run.case
    for sel in (("wino", "direct", "") if A == 5 else ("",)):
        out = {}
        for order in ("", "pass", "item"):
            _select(monkeypatch, LFSR_EPI=sel, LFSR_EPI_ORDER=order)
            rc, yh, yv = run.both()
            capi.check(rc, "epiconv_hv_fwd")
            fwd_op_gate(yh, c["yh64"], c["yh32"], "epiconv_hv", f"{sel or 'default'} order={order or 'unset'} [{epi_kernel(run.geom, sel)}] h", run.geom)
            fwd_op_gate(yv, c["yv64"], c["yv32"], "epiconv_hv", f"{sel or 'default'} order={order or 'unset'} [{epi_kernel(run.geom, sel)}] v", run.geom)
            out[order] = (yh, yv)
        for order in ("pass", "item"):
            assert _bits_equal(out[order][0], out[""][0]) and _bits_equal(out[order][1], out[""][1]), (sel, order)


@pytest.mark.parametrize("B,A,h,w", [(1, 5, 8, 8), (1, 3, 8, 8), (2, 1, 9, 7)])
def test_epiconv_selector_reaches_the_named_launcher(B, A, h, w, monkeypatch):
    """an observable beside the bits (at angRes 1 the fused kernel and the gather-GEMM give the same): lfsr_epi_run brackets any fused launch with an `epi_fused`
    record of the operator timing hooks, the gather-GEMM path has none.  Unset, wino and direct reach it; gather does not"""
    run = _EpiRun((B, A, h, w))
    for sel in ("", "wino", "direct", "gather"):
        _select(monkeypatch, LFSR_EPI=sel)
        capi.op_profile(True)
        try:
            rc, _, _ = run.both()
            capi.check(rc, "epiconv_hv_fwd")
            rc, _, _ = run.single(1)
            capi.check(rc, "epiconv_fwd")
            ops = {k[0]: v[1] for k, v in capi.op_profile_read().items()}
        finally:
            capi.op_profile(False)
        assert ops.get("epiconv_hv") == 1 and ops.get("epiconv") == 1, ops
        assert ops.get("epi_fused", 0) == (0 if sel == "gather" else 2), (sel, ops)


def test_epiconv_unaligned_output_runs_the_gather_gemm(monkeypatch):
    """a channel offset of 82 on a fused geometry: no 16-byte output vectors, the gather-GEMM runs -- the bits of LFSR_EPI=gather at an aligned offset, and right"""
    geom = (1, 5, 8, 8)
    run = _EpiRun(geom)
    c = run.case
    _select(monkeypatch)
    for v, k in ((0, "h"), (1, "v")):
        rc, y, t = run.single(v, choff=82)
        capi.check(rc, "epiconv_fwd")
        fwd_op_gate(y, c["y" + k + "64"], c["y" + k + "32"], "epiconv", f"default choff 82 [gather-GEMM] {k}", geom)
        fwd_op_gate(t, c["e" + k + "64"], c["e" + k + "32"], "epiconv tmp", f"default choff 82 [gather-GEMM] {k}", geom)
        _select(monkeypatch, LFSR_EPI="gather")
        rc, yg, tg = run.single(v)
        _select(monkeypatch)
        assert rc == 0 and _bits_equal(y, yg) and _bits_equal(t, tg)
    rc, yh, yv = run.both(choff_h=46, choff_v=82)
    capi.check(rc, "epiconv_hv_fwd")
    _select(monkeypatch, LFSR_EPI="gather")
    rc, gh, gv = run.both()
    assert rc == 0 and _bits_equal(yh, gh) and _bits_equal(yv, gv)


def test_epiconv_tmp_null(monkeypatch):
    """tmp = NULL: fine wherever a fused kernel runs (both entry points), LFSR_E_ARG with nothing written where the gather-GEMM path needs the scratch"""
    _select(monkeypatch)
    run = _EpiRun((1, 5, 8, 8))
    c = run.case
    rc, yh, yv = run.both(tmp=False)
    capi.check(rc, "epiconv_hv_fwd")
    fwd_op_gate(yh, c["yh64"], c["yh32"], "epiconv_hv", "default tmp=NULL [epi_b3] h", run.geom)
    fwd_op_gate(yv, c["yv64"], c["yv32"], "epiconv_hv", "default tmp=NULL [epi_b3] v", run.geom)
    rc, y, _ = run.single(1, tmp=False)
    capi.check(rc, "epiconv_fwd")
    fwd_op_gate(y, c["yv64"], c["yv32"], "epiconv", "default tmp=NULL [epi_b3] v", run.geom)
    for geom in ((1, 7, 5, 6), (1, 5, 33, 8)):
        run = _EpiRun(geom)
        assert run.both(tmp=False)[0] == E_ARG                 # (the readers assert that every float of y and tmp kept its bits)
        assert run.single(0, tmp=False)[0] == E_ARG
    _select(monkeypatch, LFSR_EPI="gather")
    assert _EpiRun((1, 5, 8, 8)).both(tmp=False)[0] == E_ARG


def test_epiconv_slope_outside_the_three_term_kernels_range(monkeypatch):
    """epi_b3.hip forms LeakyReLU as max(v, slope v) and declines a slope outside [0, 1]; the call then runs the fp32-MFMA kernel LFSR_EPI=wino names, whose
    activation is the select form: slope 1.5 is right against fp64, in that kernel's bits"""
    _select(monkeypatch)
    run = _EpiRun((1, 5, 8, 16), slope=1.5)
    base = run.check_all("")
    _select(monkeypatch, LFSR_EPI="wino")
    assert _same(run.check_all("wino"), base)


# =====================================================================================================================
# lfsr_angconv_fwd
# =====================================================================================================================
ANG_ROWS = [(2, 1, 9, 7), (3, 2, 5, 7), (2, 3, 6, 8), (1, 4, 6, 5), (1, 5, 8, 8), (2, 5, 32, 32), (1, 7, 5, 6), (1, 9, 4, 4)]


@functools.lru_cache(maxsize=None)
def _ang_case(B, A, h, w):
    g = torch.Generator().manual_seed(9000 + 1000 * B + 100 * A + 10 * h + w)
    x = _data(g, B, 64, h * A, w * A)
    w1 = torch.randn(16, 64, A, A, generator=g) * 0.03
    w2 = torch.randn(16 * A * A, 16, 1, 1, generator=g) * 0.2
    t64 = O.leaky_relu(O.conv2d(x.double().numpy(), w1.double().numpy(), stride=(A, A)), 0.1)
    y64 = O.pixel_shuffle(O.leaky_relu(O.conv2d(t64, w2.double().numpy()), 0.1), A)
    t32 = F.leaky_relu(F.conv2d(x, w1, stride=A), 0.1)
    y32 = F.pixel_shuffle(F.leaky_relu(F.conv2d(t32, w2), 0.1), A)
    a16 = lambda t: t.permute(0, 2, 3, 1).reshape(-1, 16).contiguous()            # rows (b, y, x)
    return {"x": macpi_to_rows(x, A), "w1": w1, "w2": w2, "y64": macpi_to_rows(_t64(y64), A), "y32": macpi_to_rows(y32, A), "t64": a16(_t64(t64)), "t32": a16(t32)}


def _ang_run(geom, y_lay, form):
    """lfsr_angconv_fwd, output and tmp gated against fp64 -> (y channels, tmp rows)"""
    B, A, h, w = geom
    c = _ang_case(*geom)
    w1p, w2p = capi.pack_conv_weight(c["w1"].cuda()), capi.pack_conv_weight(c["w2"].cuda(), perm=1, ch=16)
    x, y, t = op_input(c["x"], *EPI_X, seed=1), op_output(B * A * A * h * w, y_lay[0], seed=2), op_output(B * h * w, 16, seed=3)
    capi.check(capi.load().lfsr_angconv_fwd(x.ptr, *EPI_X, P(w1p), P(w2p), t.ptr, y.ptr, *y_lay, B, A, h, w, 0.1, capi.stream_ptr()), "angconv_fwd")
    got, tmp = op_output_read(y, y_lay[1], 16), op_output_read(t, 0, 16)
    fwd_op_gate(got, c["y64"], c["y32"], "angconv", form, geom)
    fwd_op_gate(tmp, c["t64"], c["t32"], "angconv tmp", form, geom)
    return got, tmp


@pytest.mark.parametrize("B,A,h,w", ANG_ROWS)
def test_angconv_every_form(B, A, h, w, monkeypatch):
    """the fused kernel (angRes <= 5, LFSR_ANG unset) and the two gather-GEMM launches (LFSR_ANG=gather; angRes 7 and 9 whatever is selected); y at offset 64 of
    a 144-float row.  y at offset 66 of a 148-float row has no 16-byte vectors and is documented to take the gather-GEMM path: LFSR_ANG=gather's bits"""
    geom = (B, A, h, w)
    _select(monkeypatch)
    fused = _ang_run(geom, (144, 64), f"default [{'k_ang_fused' if A <= 5 else 'gather-GEMM'}]")
    fallback = _ang_run(geom, (148, 66), "default y at 66 of 148 [gather-GEMM]")
    _select(monkeypatch, LFSR_ANG="gather")
    gather = _ang_run(geom, (144, 64), "gather [gather-GEMM]")
    assert _bits_equal(fallback[0], gather[0]) and _bits_equal(fallback[1], gather[1])
    if A > 5:
        assert _bits_equal(fused[0], gather[0]) and _bits_equal(fused[1], gather[1])
    else:
        assert not _bits_equal(fused[0], gather[0]) and not _bits_equal(fused[1], gather[1])         # LFSR_ANG=gather really ran the other kernels
    with arithmetic(capi.ARITH_F32):          # include/lfsr_hip.h: the angular branch computes on fp32 MFMA either way
        _select(monkeypatch)
        f32 = _ang_run(geom, (144, 64), f"ARITH_F32 [{'k_ang_fused' if A <= 5 else 'gather-GEMM'}]")
    assert _bits_equal(f32[0], fused[0]) and _bits_equal(f32[1], fused[1])


# =====================================================================================================================
# lfsr_pointwise_fwd
# =====================================================================================================================
PW_SHAPES = [(144, 64, False), (144, 64, True), (64, 64, False), (64, 128, False), (64, 40, False), (32, 160, True), (16, 400, True)]      # (cin, N, bias)
PW_M = [1, 63, 65, 1000, 2047, 2048, 2049, 2111, 5003]
PW_SELS = {"default": {}, "rowgemm=f32": {"LFSR_ROWGEMM": "f32"}, "no_rowgemm": {"LFSR_NO_ROWGEMM": "1"}, "ARITH_F32": {}}


def pw_kernel(cin, N, bias, M, sel):
    """the kernel lfsr_pointwise_fwd launches, read from gemm_gather.hip (the entry point) and rowgemm.hip (lfsr_rowgemm_launch): from 2048 rows on, unless
    LFSR_NO_ROWGEMM is set, the row-streaming GEMM takes K in {64, 128, 144} with N a multiple of 64 on 16-byte aligned operands -- bias-free and under the default
    arithmetic the three-term bf16 kernel (K = 144: 160 operand columns of which 16 are masked), else the fp32-MFMA one; everything else is the gather-GEMM"""
    if M < 2048 or sel == "no_rowgemm" or cin not in (64, 128, 144) or N % 64:
        return "gather"
    return "rowgemm_b3" if sel == "default" and not bias else "rowgemm_f32"


@functools.lru_cache(maxsize=None)
def _pw_case(cin, N, bias):
    g = torch.Generator().manual_seed(100 * cin + N + int(bias))
    x = _data(g, max(PW_M), cin)
    wt = torch.randn(N, cin, generator=g) * 0.1
    b = torch.randn(N, generator=g) if bias else None
    y64 = _t64(O.leaky_relu(O.linear(x.double().numpy(), wt.double().numpy(), b.double().numpy() if bias else None), 0.1))
    return x, wt, b, y64, F.leaky_relu(F.linear(x, wt, b), 0.1)


@pytest.mark.parametrize("cin,N,bias", PW_SHAPES)
def test_pointwise_every_shape_m_and_selection(cin, N, bias, monkeypatch):
    """M on both sides of the 2048-row switch and ragged in every tiling; x at columns 8.. of a wider row (cin 144: columns 8..151 of 160 floats), y inside a wider
    row with guard rows behind M.  Selections that reach one kernel give the same bits; the three-term bf16 kernel gives other bits than either fp32 form; the two
    fp32 forms give the same bits"""
    x, wt, b, y64, y32 = _pw_case(cin, N, bias)
    wp = capi.pack_conv_weight(wt.reshape(N, cin, 1, 1).cuda())
    bd = b.cuda() if bias else None
    xs, ys = cin + 16, N + 12
    for M in PW_M:
        xin, y = op_input(x[:M], xs, 8, seed=M), op_output(M, ys, seed=M + 1)
        got = {}
        for sel, env in PW_SELS.items():
            _select(monkeypatch, **env)
            y.reset()
            with arithmetic(capi.ARITH_F32 if sel == "ARITH_F32" else capi.ARITH_DEFAULT):
                capi.check(capi.load().lfsr_pointwise_fwd(xin.ptr, xs, 8, cin, P(wp), P(bd) if bias else None, y.ptr, ys, 8, M, N, 0.1, capi.stream_ptr()), "pointwise_fwd")
                got[sel] = op_output_read(y, 8, N)
            fwd_op_gate(got[sel], y64[:M], y32[:M], "pointwise", f"({cin},{N},{'bias' if bias else 'no bias'}) {sel} [{pw_kernel(cin, N, bias, M, sel)}]", M)
        kern = {sel: pw_kernel(cin, N, bias, M, sel) for sel in PW_SELS}
        sels = list(PW_SELS)
        for i, a in enumerate(sels):
            for c in sels[i + 1:]:
                if kern[a] == kern[c]:
                    assert _bits_equal(got[a], got[c]), (M, a, c)
                elif "rowgemm_b3" in (kern[a], kern[c]):
                    assert not _bits_equal(got[a], got[c]), (M, a, c)
                else:      # k_rowgemm (fp32) against the gather-GEMM: both sum k ascending on v_mfma_f32_32x32x2_f32 from zero and add the bias afterwards -- the
                    assert _bits_equal(got[a], got[c]), (M, a, c)      # same bits, pinned (no difference to assert; LFSR_NO_ROWGEMM shows against k_rowgemm_b3)


# =====================================================================================================================
# lfsr_initconv_fwd
# =====================================================================================================================
@pytest.mark.parametrize("B,A,h,w", [(3, 5, 32, 32), (1, 7, 3, 4), (2, 1, 9, 7), (3, 2, 5, 7)])
def test_initconv_strided_output(B, A, h, w):
    """init_conv fused with SAI2MacPI, y at offset 64 of a 144-float row; (3,5,32,32) has 76 800 pixels = 4 800 blocks of work against the 4 096-block cap: the
    grid-stride second pass runs.  Gate 1e-5, as tests/test_gpu_distgssr.py::test_initconv"""
    g = torch.Generator().manual_seed(11000 + 100 * A + h)
    x = _data(g, B, 1, A * h, A * w)                      # SAI mosaic
    wt = torch.randn(64, 1, 3, 3, generator=g) * 0.3
    ref = macpi_to_rows(_t64(O.conv2d(O.sai2macpi(x.double().numpy(), A), wt.double().numpy(), dilation=(A, A), padding=(A, A))), A)
    views = x.reshape(B, A, h, A, w).permute(0, 1, 3, 2, 4).reshape(B * A * A, 1, h, w)
    cpu = F.conv2d(views, wt, padding=1).permute(0, 2, 3, 1).reshape(-1, 64)
    xd, wd = x.cuda(), wt.cuda()
    y = op_output(B * A * A * h * w, 144, seed=5)
    capi.check(capi.load().lfsr_initconv_fwd(P(xd), P(wd), y.ptr, 144, 64, B, A, h, w, capi.stream_ptr()), "initconv_fwd")
    fwd_op_gate(op_output_read(y, 64, 64), ref, cpu, "initconv", "default", (B, A, h, w), tol=1e-5, relative=False)


# =====================================================================================================================
# lfsr_fold_head + lfsr_upsample_head_fwd
# =====================================================================================================================
@pytest.mark.parametrize("B,A,h,w", [(2, 5, 8, 8), (1, 3, 7, 13), (1, 5, 6, 7), (3, 5, 32, 32)])
@pytest.mark.parametrize("s", [2, 3, 4])
def test_fold_head_and_upsample_head_every_scale(s, B, A, h, w):
    """k_head<2>, k_head<3>, k_head4_lanes (s = 4, w a multiple of 4) and k_head<4> (s = 4, w = 7 and 13), f at offset 64 of a 144-float row; the folded matrix
    and bias too"""
    g = torch.Generator().manual_seed(12000 + 100 * s + 10 * A + w)
    f = _data(g, B, 64, A * h, A * w)                    # MacPI features
    xlr = _data(g, B, 1, A * h, A * w)                   # SAI mosaic
    w0 = torch.randn(64 * s * s, 64, 1, 1, generator=g) * 0.1
    b0 = torch.randn(64 * s * s, generator=g) * 0.1
    w2 = torch.randn(1, 64, 1, 1, generator=g) * 0.1
    ref, cpu = [], []
    for i in range(B):                                   # one sample at a time: the (64 s^2)-channel intermediate of a whole batch is 0.6 GB in fp64
        fi = f[i:i + 1]
        up = O.conv2d(O.pixel_shuffle(O.conv2d(O.macpi2sai(fi.double().numpy(), A), w0.double().numpy(), b0.double().numpy()), s), w2.double().numpy())
        ref.append(_t64(up + O.interp_bilinear(xlr[i:i + 1].double().numpy(), s)))
        fs = fi.reshape(1, 64, h, A, w, A).permute(0, 1, 3, 2, 5, 4).reshape(1, 64, A * h, A * w)          # MacPI2SAI
        cpu.append(F.conv2d(F.pixel_shuffle(F.conv2d(fs, w0, b0), s), w2) + F.interpolate(xlr[i:i + 1], scale_factor=s, mode="bilinear", align_corners=False))
    ref, cpu = torch.cat(ref), torch.cat(cpu)
    lib, st = capi.load(), capi.stream_ptr()
    w0d, b0d, w2d, xd = w0.cuda(), b0.cuda(), w2.cuda(), xlr.cuda()
    wf, bf = op_output(s * s, 64, seed=1), op_output(1, s * s, seed=2)
    capi.check(lib.lfsr_fold_head(P(w0d), P(b0d), P(w2d), wf.ptr, bf.ptr, 64, s, st), "fold_head")
    wf_ref = torch.einsum("k,kqc->qc", w2.double().reshape(64), w0.double().reshape(64, s * s, 64))      # out[ij] = sum_k w2[k] (w0[k s^2 + ij] . f + b0[k s^2 + ij])
    bf_ref = torch.einsum("k,kq->q", w2.double().reshape(64), b0.double().reshape(64, s * s)).reshape(1, -1)
    fwd_op_gate(op_output_read(wf, 0, 64), wf_ref, torch.einsum("k,kqc->qc", w2.reshape(64), w0.reshape(64, s * s, 64)), "fold_head wf", f"s={s}", (B, A, h, w))
    fwd_op_gate(op_output_read(bf, 0, s * s), bf_ref, torch.einsum("k,kq->q", w2.reshape(64), b0.reshape(64, s * s)).reshape(1, -1), "fold_head bf", f"s={s}", (B, A, h, w))
    fin = op_input(macpi_to_rows(f, A), 144, 64, seed=3)
    out = op_output(B * A * h * s, A * w * s, seed=4)
    capi.check(lib.lfsr_upsample_head_fwd(fin.ptr, 144, 64, wf.ptr, bf.ptr, P(xd), out.ptr, B, A, h, w, s, st), "upsample_head_fwd")
    kernel = "k_head4_lanes" if s == 4 and w % 4 == 0 else f"k_head<{s}>"
    fwd_op_gate(op_output_read(out, 0, A * w * s), ref.reshape(-1, A * w * s), cpu.reshape(-1, A * w * s), "upsample_head", f"s={s} [{kernel}]", (B, A, h, w))


# =====================================================================================================================
# refusals: LFSR_E_ARG and every output float at its sentinel
# =====================================================================================================================
def _refused(rc, *outs):
    torch.cuda.synchronize()
    assert rc == E_ARG, rc
    for o in outs:
        op_output_read(o, 0, 0)         # asserts that every float kept its bits


def test_conv3x3_refusals():
    run = _C3Run((2, 9, 33))
    n_img, h, w = run.geom
    lib, st, f = capi.load(), capi.stream_ptr(), "lrelu0.1+r1+r2"
    xs, xo = C3_LAYOUT["x"]
    ys, yo = C3_LAYOUT["y"]
    _refused(run.launch(f, x=(run.x.ptr, xs + 2, xo + 2)), run.y)                     # a misaligned x_choff (and stride)
    _refused(run.launch(f, x=(run.x.ptr, xs, xo + 2)), run.y)
    _refused(run.launch(f, x=(run.x.ptr, xs, xs - 60)), run.y)                        # strides shorter than offset + 64
    _refused(run.launch(f, y=(run.y.ptr, ys, ys - 60)), run.y)
    _refused(run.launch(f, y=(run.y.ptr, 60, 0)), run.y)
    args = lambda r1s, r2s, n, hh, ww: (run.x.ptr, xs, xo, P(run.wp), run.y.ptr, ys, yo, run.r1.ptr, r1s, 0, run.r2.ptr, r2s, 8, n, hh, ww, 0.1, st)
    _refused(lib.lfsr_conv3x3_fwd(*args(60, 72, n_img, h, w)), run.y)                 # ... the residuals' too
    _refused(lib.lfsr_conv3x3_fwd(*args(64, 68, n_img, h, w)), run.y)
    for n, hh, ww in ((0, h, w), (n_img, 0, w), (n_img, h, -1)):                      # non-positive sizes
        _refused(lib.lfsr_conv3x3_fwd(*args(64, 72, n, hh, ww)), run.y)
    capi.check(lib.lfsr_conv3x3_fwd(*args(64, 72, n_img, h, w)), "conv3x3_fwd")       # (the same call with nothing wrong runs)
    torch.cuda.synchronize()


def test_epiconv_and_angconv_refusals():
    B, A, h, w = 1, 5, 8, 8
    run = _EpiRun((B, A, h, w))
    lib, st = capi.load(), capi.stream_ptr()
    xs, xo = EPI_X
    for bad in ({"xo": xo + 2}, {"xs": xo + 60}, {"ys": 112 + 28}, {"B": 0}, {"A": 0}, {"h": 0}, {"w": -3}):
        a = {**dict(xs=xs, xo=xo, ys=144, B=B, A=A, h=h, w=w), **bad}
        run.y.reset(); run.t.reset()
        for vertical in (0, 1):
            _refused(lib.lfsr_epiconv_fwd(run.x.ptr, a["xs"], a["xo"], P(run.w1p), P(run.w2p), run.t.ptr, run.y.ptr, a["ys"], 112, a["B"], a["A"], a["h"], a["w"], vertical,
                                          0.1, st), run.y, run.t)
        _refused(lib.lfsr_epiconv_hv_fwd(run.x.ptr, a["xs"], a["xo"], P(run.w1p), P(run.w2p), run.t.ptr, run.y.ptr, a["ys"], 80, 112, a["B"], a["A"], a["h"], a["w"], 0.1, st),
                 run.y, run.t)
    c = _ang_case(B, A, h, w)
    w1p, w2p = capi.pack_conv_weight(c["w1"].cuda()), capi.pack_conv_weight(c["w2"].cuda(), perm=1, ch=16)
    x, y, t = op_input(c["x"], *EPI_X, seed=1), op_output(B * A * A * h * w, 144, seed=2), op_output(B * h * w, 16, seed=3)
    for bad in ({"xo": xo + 2}, {"xs": xo + 60}, {"ys": 64 + 12}, {"B": 0}, {"A": -1}, {"h": 0}, {"w": 0}):
        a = {**dict(xs=xs, xo=xo, ys=144, B=B, A=A, h=h, w=w), **bad}
        _refused(lib.lfsr_angconv_fwd(x.ptr, a["xs"], a["xo"], P(w1p), P(w2p), t.ptr, y.ptr, a["ys"], 64, a["B"], a["A"], a["h"], a["w"], 0.1, st), y, t)
    _refused(lib.lfsr_angconv_fwd(x.ptr, xs, xo, P(w1p), P(w2p), None, y.ptr, 144, 64, B, A, h, w, 0.1, st), y, t)          # tmp is an output here: never NULL


def test_pointwise_initconv_and_head_refusals():
    lib, st, M = capi.load(), capi.stream_ptr(), 3000
    g = torch.Generator().manual_seed(5)
    x, y = op_input(_data(g, M, 144), 160, 8, seed=1), op_output(M, 76, seed=2)
    wp = torch.randn(64 * 160, generator=g).cuda()
    pw = lambda xs, xo, cin, ys, yo, m, n: lib.lfsr_pointwise_fwd(x.ptr, xs, xo, cin, P(wp), None, y.ptr, ys, yo, m, n, 0.1, st)
    _refused(pw(160, 8, 48, 76, 8, M, 64), y)                   # cin outside {16, 32, 64, 144}: refused behind the row-GEMM's refusal (M >= 2048) ...
    _refused(pw(160, 8, 48, 76, 8, 1000, 64), y)                # ... and by the gather-GEMM's switch
    _refused(pw(160, 10, 144, 76, 8, M, 64), y)                 # a misaligned x_choff
    _refused(pw(150, 8, 144, 76, 8, M, 64), y)                  # strides shorter than offset + channels
    _refused(pw(160, 8, 144, 76, 16, M, 64), y)
    _refused(pw(160, 8, 144, 76, 8, 0, 64), y)                  # non-positive sizes
    _refused(pw(160, 8, 144, 76, 8, M, 0), y)
    B, A, h, w = 2, 3, 5, 7
    xd, wd = _data(g, B, 1, A * h, A * w).cuda(), torch.randn(64, 1, 3, 3, generator=g).cuda()
    yi = op_output(B * A * A * h * w, 144, seed=3)
    ic = lambda ys, yo, b, a, hh, ww: lib.lfsr_initconv_fwd(P(xd), P(wd), yi.ptr, ys, yo, b, a, hh, ww, st)
    for bad in ((144, 66, B, A, h, w), (146, 64, B, A, h, w), (120, 64, B, A, h, w), (144, 64, 0, A, h, w), (144, 64, B, 0, h, w), (144, 64, B, A, -1, w), (144, 64, B, A, h, 0)):
        _refused(ic(*bad), yi)
    w0d, b0d, w2d = torch.randn(64 * 16, 64, generator=g).cuda(), torch.randn(64 * 16, generator=g).cuda(), torch.randn(64, generator=g).cuda()
    wfo, bfo = op_output(16, 64, seed=6), op_output(1, 16, seed=7)
    for C_, s_, w0p, w2p in ((32, 2, P(w0d), P(w2d)), (128, 2, P(w0d), P(w2d)), (64, 0, P(w0d), P(w2d)), (64, -2, P(w0d), P(w2d)), (64, 4, None, P(w2d)), (64, 4, P(w0d), None)):
        _refused(lib.lfsr_fold_head(w0p, P(b0d), w2p, wfo.ptr, bfo.ptr, C_, s_, st), wfo, bfo)           # lfsr_fold_head: C = 64 only, s > 0, no NULL weight
    fin = op_input(_data(g, B * A * A * h * w, 64), 144, 64, seed=4)
    wf, bf = torch.randn(25 * 64, generator=g).cuda(), torch.randn(25, generator=g).cuda()
    out = op_output(B * A * h * 5, A * w * 5, seed=5)
    hd = lambda fs, fo, b, a, hh, ww, s: lib.lfsr_upsample_head_fwd(fin.ptr, fs, fo, P(wf), P(bf), P(xd), out.ptr, b, a, hh, ww, s, st)
    for bad in ((144, 64, B, A, h, w, 5), (144, 64, B, A, h, w, 1), (144, 66, B, A, h, w, 4), (120, 64, B, A, h, w, 4), (144, 64, 0, A, h, w, 4), (144, 64, B, A, 0, w, 2),
                (144, 64, B, A, h, -2, 3)):
        _refused(hd(*bad), out)
