"""GPU: LFSSR's four operators at the C ABI against fp64, with stock torch conv2d in fp32 on the CPU as the yardstick (tests/helpers.py: op_gate) -- operands inside
wider rows behind NaN guard rows, outputs in front of sentinel rows; the refusals; two runs, the same bits.

lfsr_angconv3x3_fwd: angRes 2 (every view a corner), 3 and 5 (an interior view) x views of 1 x 1 (one pixel of a 16-pixel tile), 3 x 5 (15: one ragged tile) and
8 x 8 (four tiles) x B 1 and 2 (view A^2 of sample 0 is view 0 of sample 1) x no prologue / an ALL-POSITIVE in_bias (a view outside the grid that went through the
prologue would add relu(0 + bias) > 0) x the dense and the 144-wide layout for x and y independently; angRes 6..9 (the banded launches) at one geometry each.

lfsr_lfssr_conv0_fwd, lfsr_conv3x3_ps2_fwd, lfsr_lfssr_tail_fwd: 3 x 3 views of 5 x 7 at B 2, views of one pixel, a 9 x 9 grid, and sizes just past the launch cap, at which a thread of
their grid-stride loops takes a second, ragged pass (measured figures: profiles/lfssr_geometry_tests.md)."""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

from lfsr_amd import capi
from tests.helpers import OP_SENTINEL, op_gate, op_input, op_output, op_output_read
from tests.lfssr_helpers import GRID_CAP_ITEMS

pytestmark = pytest.mark.gpu

LAYOUTS = ((64, 0), (144, 64))


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


@functools.lru_cache(maxsize=None)
def ang_case(A, h, w, B, biased, only_tap=None):
    """-> x rows, weight, bias, in_bias (or None), the fp64 result rows and the fp32 CPU result rows, computed once"""
    npix = h * w
    x = rnd((B * A * A * npix, 64), 11 + A).float()
    wt = rnd((64, 64, 3, 3), 5, 1.0 / 24.0).float()
    if only_tap is not None:
        keep = torch.zeros(3, 3)
        keep[only_tap] = 1.0
        wt = wt * keep
    bias = rnd((64,), 6, 0.1).float()
    in_bias = (torch.rand(64, generator=torch.Generator().manual_seed(7)) + 0.5).float() if biased else None

    def ref(dtype):
        t = x.to(dtype)
        if in_bias is not None:
            t = torch.relu(t + in_bias.to(dtype))
        g = t.reshape(B, A, A, npix, 64).permute(0, 3, 4, 1, 2).reshape(B * npix, 64, A, A)       # the reference's (N h w, c, an, an)
        o = torch.relu(F.conv2d(g, wt.to(dtype), bias.to(dtype), padding=1))
        return o.reshape(B, npix, 64, A, A).permute(0, 3, 4, 1, 2).reshape(-1, 64)

    return x, wt, bias, in_bias, ref(torch.float64), ref(torch.float32)


def run_ang(x, wt, bias, in_bias, B, A, npix, xl, yl, seed=0):
    xb = op_input(x, xl[0], xl[1], 21 + seed)
    yb = op_output(x.shape[0], yl[0], 22 + seed)
    wp = capi.pack_conv_weight(wt.cuda())
    bd, ib = bias.cuda(), in_bias.cuda() if in_bias is not None else None
    rc = capi.load().lfsr_angconv3x3_fwd(xb.ptr, xl[0], xl[1], capi.dev_ptr(wp), capi.dev_ptr(bd), capi.dev_ptr(ib) if ib is not None else None,
                                         yb.ptr, yl[0], yl[1], B, A, npix, capi.stream_ptr())
    assert rc == 0, rc
    return op_output_read(yb, yl[1], 64)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (8, 8)])
@pytest.mark.parametrize("A", [2, 3, 5])
def test_angconv3x3_vs_fp64(A, hw, B):
    h, w = hw
    for biased in (False, True):
        x, wt, bias, in_bias, ref, cpu = ang_case(A, h, w, B, biased)
        for xl in LAYOUTS:
            for yl in LAYOUTS:
                got = run_ang(x, wt, bias, in_bias, B, A, h * w, xl, yl)
                op_gate(got, ref, cpu, "angconv3x3", "in_bias" if biased else "plain", f"A{A} {h}x{w} B{B} x{xl} y{yl}", tag="LFSSROP")


@pytest.mark.parametrize("A,h,w", [(6, 3, 5), (7, 2, 3), (8, 1, 3), (9, 3, 3), (4, 5, 5)])
def test_angconv3x3_banded_grids(A, h, w):
    """angRes 6..9 run as bands of view rows (a band stages the view row on either side of it); 4: the widest grid that is one band of 16 views"""
    x, wt, bias, in_bias, ref, cpu = ang_case(A, h, w, 2, True)
    got = run_ang(x, wt, bias, in_bias, 2, A, h * w, (144, 64), (64, 0))
    op_gate(got, ref, cpu, "angconv3x3", "in_bias", f"A{A} {h}x{w} B2", tag="LFSSROP")


@pytest.mark.parametrize("tap", [(0, 0), (2, 2)])
def test_angconv3x3_single_tap_pairs_first_axis_with_u(tap):
    """weights zero except one corner tap: y[b,u,v] = relu(bias + W[:, :, tap] a[b, u + tap_u - 1, v + tap_v - 1]) where that view exists, relu(bias) elsewhere"""
    A, h, w, B = 5, 3, 5, 2
    npix = h * w
    x, wt, bias, in_bias, ref, cpu = ang_case(A, h, w, B, True, only_tap=tap)
    got = run_ang(x, wt, bias, in_bias, B, A, npix, (64, 0), (64, 0))
    op_gate(got, ref, cpu, "angconv3x3", "one tap", f"tap{tap}", tag="LFSSROP")
    a = torch.relu(x.double() + in_bias.double()).reshape(B, A, A, npix, 64)
    du, dv = tap[0] - 1, tap[1] - 1
    want = torch.zeros(B, A, A, npix, 64, dtype=torch.float64)
    for u in range(A):
        for v in range(A):
            if 0 <= u + du < A and 0 <= v + dv < A:
                want[:, u, v] = a[:, u + du, v + dv] @ wt[:, :, tap[0], tap[1]].double().t()
    want = torch.relu(want + bias.double()).reshape(-1, 64)
    assert float((got.double() - want).abs().max()) <= 1e-4 * max(1.0, float(want.abs().max()))
    # the rows the tap does not reach hold relu(bias) exactly
    edge = got.reshape(B, A, A, npix, 64)[:, 0 if du < 0 else A - 1]
    assert torch.equal(edge, torch.relu(bias).expand_as(edge))


def test_angconv3x3_two_runs_same_bits_and_batch_invariance():
    A, h, w, B = 5, 3, 5, 2
    x, wt, bias, in_bias, _, _ = ang_case(A, h, w, B, True)
    a = run_ang(x, wt, bias, in_bias, B, A, h * w, (144, 64), (144, 64))
    b = run_ang(x, wt, bias, in_bias, B, A, h * w, (144, 64), (144, 64), seed=4)
    assert torch.equal(a, b)
    half = x.shape[0] // 2
    one = run_ang(x[half:], wt, bias, in_bias, 1, A, h * w, (64, 0), (64, 0))
    assert torch.equal(one, a[half:])


def test_angconv3x3_refusals_write_nothing():
    A, h, w, B = 3, 3, 5, 1
    npix = h * w
    x, wt, bias, in_bias, _, _ = ang_case(A, h, w, B, True)
    xb, yb = op_input(x, 144, 64, 1), op_output(x.shape[0], 144, 2)
    wp, bd, ib = capi.pack_conv_weight(wt.cuda()), bias.cuda(), in_bias.cuda()
    lib, st = capi.load(), capi.stream_ptr()
    P = capi.dev_ptr

    def call(x_=xb.ptr, xs=144, xo=64, w_=None, b_=None, ib_=None, y_=yb.ptr, ys=144, yo=64, B_=B, A_=A, n_=npix):
        return lib.lfsr_angconv3x3_fwd(x_, xs, xo, w_ or P(wp), b_ or P(bd), ib_ or P(ib), y_, ys, yo, B_, A_, n_, st)

    off4 = lambda p: C.c_void_p(p.value + 4)
    bad = [call(A_=1), call(A_=10), call(A_=0), call(B_=0), call(n_=0), call(xs=146), call(xo=66), call(ys=142), call(yo=62), call(xs=100, xo=64), call(ys=64, yo=4),
           call(x_=off4(xb.ptr)), call(y_=off4(yb.ptr)), call(ib_=off4(P(ib))), call(w_=off4(P(wp))), call(x_=None), call(y_=None),
           call(B_=1 << 20, n_=1 << 8),                 # 2^28 * 9 rows of 144 floats: far past 2 GiB
           call(B_=4, A_=8, n_=14564)]                  # 3,728,384 rows x 144 floats = 2^29 + 16,384 floats: just past 2 GiB
    assert bad == [-1] * len(bad), bad
    op_output_read(yb, 0, 0)
    assert call() == 0
    op_output_read(yb, 64, 64)


# ---- conv0, the up-sampling conv, the tail: (A, B, h, w) --------------------------------------------------------------------------------------------
# BASE: odd h and w, a batch boundary (the refusals are checked there); ONE_PIXEL: views of one pixel, every tap but the centre off the image (the tail's output views are
# 2 x 2); A9: the mosaic addressing at the largest grid; WRAP / WRAP0: past the 8192 blocks of 256 threads a launch is capped at (lfsr_cap_grid), so that a thread takes a
# second pass, with a count that is no multiple of 256 -- a ragged last block, and in the tail a last 16-lane butterfly group with dead lanes

BASE, ONE_PIXEL, A9, WRAP, WRAP0 = (3, 2, 5, 7), (2, 1, 1, 1), (9, 1, 2, 3), (3, 1, 61, 61), (3, 1, 121, 121)
MOSAIC_GUARD = 1024          # NaN floats in front of and behind conv0's mosaic and the tail's LR planes
op_ids = lambda g: "A%dB%dh%dw%d" % g if isinstance(g, tuple) else None


def wraps(items):
    """the count is past the launch cap and leaves a ragged last block"""
    return items > GRID_CAP_ITEMS and items % 256 != 0


def views_to_rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


@pytest.mark.parametrize("geom", [BASE, ONE_PIXEL, A9, WRAP0], ids=op_ids)
def test_conv0_vs_fp64(geom):
    A0, B0, H0, W0 = geom
    if geom == WRAP0:
        assert B0 * A0 * A0 * H0 * W0 == 131769 and wraps(131769 * 16)               # 2,108,304 items: 8235.56 blocks
    x = torch.rand(B0, 1, A0 * H0, A0 * W0, generator=torch.Generator().manual_seed(3))
    wt, bias = rnd((64, 1, 3, 3), 1, 1.0 / 3.0).float(), rnd((64,), 2, 0.1).float()
    views = x.reshape(B0, A0, H0, A0, W0).permute(0, 1, 3, 2, 4).reshape(-1, 1, H0, W0)
    ref, cpu = (views_to_rows(torch.relu(F.conv2d(views.to(d), wt.to(d), bias.to(d), padding=1))) for d in (torch.float64, torch.float32))
    M = ref.shape[0]
    lib, outs = capi.load(), []
    xbuf = torch.full((x.numel() + 2 * MOSAIC_GUARD,), float("nan"))       # the mosaic behind and in front of NaN: a tap that leaves it shows
    xbuf[MOSAIC_GUARD:MOSAIC_GUARD + x.numel()] = x.reshape(-1)
    xbuf, wd, bd = xbuf.cuda(), wt.cuda(), bias.cuda()
    xd = xbuf[MOSAIC_GUARD:MOSAIC_GUARD + x.numel()]
    for k in range(2):
        yb = op_output(M, 144, 30 + k)
        assert lib.lfsr_lfssr_conv0_fwd(capi.dev_ptr(xd), capi.dev_ptr(wd), capi.dev_ptr(bd), yb.ptr, 144, 64, B0, A0, H0, W0, capi.stream_ptr()) == 0
        outs.append(op_output_read(yb, 64, 64))
    op_gate(outs[0], ref, cpu, "lfssr_conv0", "bias+relu", f"A{A0} {H0}x{W0} B{B0}", tag="LFSSROP")
    assert torch.equal(outs[0], outs[1])
    if geom != BASE:
        return
    yb = op_output(M, 144, 33)
    bad = [lib.lfsr_lfssr_conv0_fwd(capi.dev_ptr(xd), capi.dev_ptr(wd), capi.dev_ptr(bd), yb.ptr, ys, yo, B, A0, H0, W0, None)
           for ys, yo, B in ((146, 64, B0), (144, 66, B0), (100, 64, B0), (144, 64, 0))]
    bad.append(lib.lfsr_lfssr_conv0_fwd(None, capi.dev_ptr(wd), capi.dev_ptr(bd), yb.ptr, 144, 64, B0, A0, H0, W0, None))
    assert bad == [-1] * 5
    op_output_read(yb, 0, 0)


@pytest.mark.parametrize("geom", [BASE, ONE_PIXEL, WRAP], ids=op_ids)
def test_conv3x3_ps2_vs_fp64(geom):
    A0, B0, H0, W0 = geom
    n_img = B0 * A0 * A0
    if geom == WRAP:
        assert n_img * H0 * W0 == 33489 and wraps(33489 * 64)                        # 2,143,296 items: 8372.25 blocks
    xin = rnd((n_img, 64, H0, W0), 4).float()
    wt, bias = rnd((256, 64, 3, 3), 5, 1.0 / 24.0).float(), rnd((256,), 6, 0.1).float()
    ref, cpu = (views_to_rows(torch.relu(F.pixel_shuffle(F.conv2d(xin.to(d), wt.to(d), bias.to(d), padding=1), 2))) for d in (torch.float64, torch.float32))
    rows = views_to_rows(xin)
    lib, outs = capi.load(), []
    wp, bd = capi.pack_ps2_weight(wt.cuda()), bias.cuda()
    tmp = torch.empty((rows.shape[0], 256), device="cuda")
    for k in range(2):
        xb, yb = op_input(rows, 144, 64, 40 + k), op_output(4 * rows.shape[0], 144, 42 + k)
        assert lib.lfsr_conv3x3_ps2_fwd(xb.ptr, 144, 64, capi.dev_ptr(wp), capi.dev_ptr(bd), capi.dev_ptr(tmp), yb.ptr, 144, 64, n_img, H0, W0, capi.stream_ptr()) == 0
        outs.append(op_output_read(yb, 64, 64))
    op_gate(outs[0], ref, cpu, "conv3x3_ps2", "bias+ps2+relu", f"{n_img} views {H0}x{W0}", tag="LFSSROP")
    assert torch.equal(outs[0], outs[1])
    if geom != BASE:
        return
    xb, yb = op_input(rows, 144, 64, 44), op_output(4 * rows.shape[0], 144, 45)
    args = dict(xs=144, xo=64, ys=144, yo=64, n=n_img)
    bad = []
    for over in (dict(xs=146), dict(xo=66), dict(ys=142), dict(yo=62), dict(ys=100), dict(n=0), dict(n=1 << 26)):
        a = dict(args, **over)
        bad.append(lib.lfsr_conv3x3_ps2_fwd(xb.ptr, a["xs"], a["xo"], capi.dev_ptr(wp), capi.dev_ptr(bd), capi.dev_ptr(tmp), yb.ptr, a["ys"], a["yo"], a["n"], H0, W0, None))
    bad.append(lib.lfsr_conv3x3_ps2_fwd(xb.ptr, 144, 64, capi.dev_ptr(wp), capi.dev_ptr(bd), None, yb.ptr, 144, 64, n_img, H0, W0, None))
    assert bad == [-1] * 8
    op_output_read(yb, 0, 0)


@pytest.mark.parametrize("mosaic", [0, 1])
@pytest.mark.parametrize("geom", [BASE, ONE_PIXEL, A9, WRAP], ids=op_ids)
def test_tail_vs_fp64(geom, mosaic):
    A0, B0, H0, W0 = geom
    n_img = B0 * A0 * A0
    if geom == WRAP:
        assert n_img * 4 * H0 * W0 == 133956 and 133956 % 16 and wraps(133956 * 16)   # 2,143,296 items, 8372.25 blocks: the last butterfly group has dead lanes
    f = rnd((n_img, 64, 2 * H0, 2 * W0), 7).float()
    lo = torch.rand(n_img, 1, H0, W0, generator=torch.Generator().manual_seed(8))
    w_res, b_res = rnd((1, 64, 3, 3), 9, 1.0 / 24.0).float(), rnd((1,), 10, 0.1).float()
    w_iup, b_iup = rnd((4, 1, 3, 3), 11, 1.0 / 3.0).float(), rnd((4,), 12, 0.1).float()

    def ref(d):
        o = F.conv2d(f.to(d), w_res.to(d), b_res.to(d), padding=1) + F.pixel_shuffle(F.conv2d(lo.to(d), w_iup.to(d), b_iup.to(d), padding=1), 2)
        if mosaic:
            o = o.reshape(B0, A0, A0, 2 * H0, 2 * W0).permute(0, 1, 3, 2, 4)
        return o.reshape(1, -1)

    rows = views_to_rows(f)
    n_out = n_img * 4 * H0 * W0
    lobuf = torch.full((lo.numel() + 2 * MOSAIC_GUARD,), float("nan"))         # the LR planes behind and in front of NaN
    lobuf[MOSAIC_GUARD:MOSAIC_GUARD + lo.numel()] = lo.reshape(-1)
    lobuf = lobuf.cuda()
    dev = [t.cuda() for t in (w_res, b_res)] + [lobuf[MOSAIC_GUARD:MOSAIC_GUARD + lo.numel()]] + [t.cuda() for t in (w_iup, b_iup)]
    lib, outs = capi.load(), []
    for k in range(2):
        fb = op_input(rows, 144, 64, 50 + k)
        pool = torch.full((8 + n_out + 8,), OP_SENTINEL, device="cuda")      # sentinels in front of the first output pixel and behind the last
        out = pool[8:]
        rc = lib.lfsr_lfssr_tail_fwd(fb.ptr, 144, 64, capi.dev_ptr(dev[0]), capi.dev_ptr(dev[1]), capi.dev_ptr(dev[2]), capi.dev_ptr(dev[3]), capi.dev_ptr(dev[4]),
                                     capi.dev_ptr(out), B0, A0, H0, W0, mosaic, capi.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((out[n_out:] == OP_SENTINEL).all()) and bool((pool[:8] == OP_SENTINEL).all())
        outs.append(out[:n_out].cpu().reshape(1, -1))
    op_gate(outs[0], ref(torch.float64), ref(torch.float32), "lfssr_tail", "mosaic" if mosaic else "planes", f"A{A0} {H0}x{W0} B{B0}", tag="LFSSROP")
    assert torch.equal(outs[0], outs[1])
    if geom != BASE:
        return
    fb = op_input(rows, 144, 64, 52)
    out = torch.full((n_out + 8,), OP_SENTINEL, device="cuda")
    P = capi.dev_ptr
    bad = [lib.lfsr_lfssr_tail_fwd(fb.ptr, fs, fo, P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), P(dev[4]), P(out), B, A0, H0, W0, m, None)
           for fs, fo, B, m in ((146, 64, B0, mosaic), (144, 66, B0, mosaic), (100, 64, B0, mosaic), (144, 64, 0, mosaic), (144, 64, B0, 2))]
    bad.append(lib.lfsr_lfssr_tail_fwd(fb.ptr, 144, 64, P(dev[0]), P(dev[1]), None, P(dev[3]), P(dev[4]), P(out), B0, A0, H0, W0, mosaic, None))
    assert bad == [-1] * 6
    torch.cuda.synchronize()
    assert bool((out == OP_SENTINEL).all())
