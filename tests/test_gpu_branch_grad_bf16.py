"""GPU: lfsr_set_branch_grad_arithmetic(LFSR_BRANCH_GRAD_ARITH_BF16) -- EPIConv.0's EPI-line weight and data gradients on bf16 operands (csrc/epi0_grad_bf16.hip)
behind lfsr_epiconv_hv_bwd and lfsr_distgssr_backward.
  * exact form: with a stage 2 that is exact in fp32 (one power of two per column of w2), dw0 and dx are conv2d_weight / conv2d_input of the bf16-ROUNDED operands in
    fp64, to fp32 accumulation of at most 160-term sums (dw0 rel-L2 <= 1e-4, max |dx - ref| < 1e-4);
  * it really is bf16 (rel-L2 to the default's > 1e-3, to fp64 of the unrounded operands <= 1e-2 = 4 x the 2.35e-3 of two independently rounded operands) and the
    default's bits do not move;
  * coverage edges: where no EPI-line kernel applies the mode changes no bit; where one pass is covered only dx moves; the LFSR_LAB gather selectors win;
  * more chunks than the data gradient's grid, strided dy, sentinel bands, LFSR_E_WS / LFSR_E_ARG with nothing written, determinism, batch invariance;
  * whole DistgSSR steps: forward and loss untouched, the bucket holds the .grads, nothing downstream of the last EPIConv.0 moves, per-parameter error against fp64
    autograd under the HIP forward's decisions not above torch.autocast(bfloat16)'s, one-stream and two-stream order agree, the default is reproduced bit for bit."""
import contextlib
import functools
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lfsr_amd import capi
from tests import helpers as TH
from tests.test_gpu_bwd_ops import BAND, E_ARG, E_WS, EPI_GEOMS, SENTINEL, P, _close, _epi_case, _ps1d, _select
from tests.test_gpu_grad_bf16 import _distg_plugin, _distg_refs, _flat, _rel_np, _step, grad_arithmetic, r16, rel

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)


@contextlib.contextmanager
def branch_grad(mode):
    """lfsr_set_branch_grad_arithmetic(mode) for the block, the default again after it (the setting is process-wide)"""
    capi.set_branch_grad_arithmetic(mode)
    try:
        yield
    finally:
        capi.set_branch_grad_arithmetic(capi.BRANCH_GRAD_ARITH_DEFAULT)


BF16, DEFAULT = 1, 0      # LFSR_BRANCH_GRAD_ARITH_BF16 / _DEFAULT (tests/test_branch_grad_arith_cpu.py holds them to the header)


def _kw(A):
    return dict(stride=(1, A), padding=(0, A * (A - 1) // 2))


def _e_rows(e, B, A, h, w, vert):
    """stage-1 activation of a pass, (B, 32, h A, w) / (B, 32, w A, h) in the reference's layout -> rows (b A + u, y, x) / (b A + v, y, x)"""
    if not vert:
        return e.float().reshape(B, 32, h, A, w).permute(0, 3, 2, 4, 1).reshape(-1, 32).contiguous().cuda()
    return e.float().reshape(B, 32, w, A, h).permute(0, 3, 4, 2, 1).reshape(-1, 32).contiguous().cuda()


def _dy_buffer(gh, gv, A):
    """dLoss/dy_h at channels 8..39, dLoss/dy_v at 48..79 of one 80-float-row buffer, every other channel the sentinel"""
    n = gh.shape[0] * gh.shape[2] * gh.shape[3]
    dyb = torch.full((n, 80), SENTINEL, device="cuda")
    capi.nchw_to_vcl(gh.float().contiguous().cuda(), A, 1, out=dyb, choff=8)
    capi.nchw_to_vcl(gv.float().contiguous().cuda(), A, 1, out=dyb, choff=48)
    return dyb


def _run(c, mode, slope):
    """one lfsr_epiconv_hv_bwd under `mode` on the prepared case c -> (dx NCHW on the CPU, dw0, dw2 on the CPU)"""
    B, A, h, w = c["geom"]
    with branch_grad(mode):
        dxv = capi.nchw_to_vcl(c["dx0"].cuda(), A, 1)
        dw0, dw2 = capi.epiconv_hv_bwd(c["dyb"], 8, 48, c["out"], 0, 32, c["xv"], c["eh"], c["ev"], c["w0"].cuda(), c["w2"].cuda(), dxv, B, A, h, w, slope)
        torch.cuda.synchronize()
    return capi.vcl_to_nchw(dxv, B, 64, A, h, w, 1).cpu(), dw0.cpu(), dw2.cpu()


# ---- the exact form: stage 2 exact in fp32, references on rounded operands ---------------------------------------------------------------------------
def _pow2_w2(A, gen):
    """(32 A, 32, 1, 1) with exactly one entry of +-1, +-0.5 or +-2 per column and zeros elsewhere"""
    w2 = torch.zeros(32 * A, 32, 1, 1)
    rows = torch.randint(0, 32 * A, (32,), generator=gen)
    vals = torch.tensor([1.0, -1.0, 0.5, -0.5, 2.0, -2.0])[torch.randint(0, 6, (32,), generator=gen)]
    w2[rows, torch.arange(32), 0, 0] = vals
    return w2


def _unshuffle1d(dy, A):
    """the adjoint of _ps1d: (B, 32, H, W A) -> (B, 32 A, H, W)"""
    B, C, H, WA = dy.shape
    return dy.reshape(B, C, H, WA // A, A).permute(0, 4, 1, 2, 3).reshape(B, A * C, H, WA // A)


@functools.lru_cache(maxsize=None)
def _exact_case(B, A, h, w, slope=0.25):
    """y = None (dy is the gradient at the stage-2 pre-activation), random non-zero stage-1 activations, a power-of-two w2: dE = LeakyReLU'(e) * (w2^t dy) is one exact
    product per element, so the fp64 reference's dE rounds to the bf16 values the GPU's rounds to"""
    gen = torch.Generator().manual_seed(977 * B + 31 * h + w)
    x, w0, _, dyh, dyv, dx0 = _epi_case(B, A, h, w)
    w2 = _pow2_w2(A, gen)
    e_h = torch.randn(B, 32, h * A, w, generator=gen)
    e_v = torch.randn(B, 32, w * A, h, generator=gen)
    assert bool((e_h != 0).all()) and bool((e_v != 0).all())
    W2 = w2[:, :, 0, 0].double()
    dw0_ref = torch.zeros(w0.shape, dtype=torch.float64)
    dx_ref = dx0.double().clone()
    for vert in (0, 1):
        t = x.double().permute(0, 1, 3, 2).contiguous() if vert else x.double()
        e = e_v if vert else e_h
        dz = _unshuffle1d((dyv.permute(0, 1, 3, 2) if vert else dyh).double(), A)
        dE = torch.einsum("jn,bjhw->bnhw", W2, dz) * torch.where(e > 0, 1.0, slope).double()
        assert torch.equal(dE.float().double(), dE)                                  # exact in fp32: what the fp32 stage 2 forms
        dw0_ref += torch.nn.grad.conv2d_weight(r16(t), w0.shape, r16(dE), **_kw(A))
        g = torch.nn.grad.conv2d_input(t.shape, r16(w0), r16(dE), **_kw(A))
        dx_ref += g.permute(0, 1, 3, 2) if vert else g
    c = dict(geom=(B, A, h, w), x=x, w0=w0, w2=w2, dx0=dx0, out=None, xv=capi.nchw_to_vcl(x.cuda(), A, 1), eh=_e_rows(e_h, B, A, h, w, 0), ev=_e_rows(e_v, B, A, h, w, 1),
             dyb=_dy_buffer(dyh, dyv, A), dw0_ref=dw0_ref, dx_ref=dx_ref)
    return c


def _exact_gates(c, slope=0.25):
    dx, dw0, dw2 = _run(c, BF16, slope)
    r, e = rel(dw0, c["dw0_ref"]), float((dx.double() - c["dx_ref"]).abs().max())
    print(f"{c['geom']}: dw0 rel-L2 to the rounded-operand form {r:.2e}, max |dx - ref| {e:.2e}")
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dw0).all())
    assert r <= 1e-4
    assert e < 1e-4
    _, _, dw2_def = _run(c, DEFAULT, slope)
    assert torch.equal(dw2, dw2_def)
    return dx, dw0, dw2


@pytest.mark.parametrize("B,A,h,w", [(2, 5, 32, 32), (1, 5, 6, 9), (1, 5, 32, 7)])
def test_gradients_are_the_exact_form_on_rounded_operands(B, A, h, w):
    """(2, 5, 32, 32): 640 lines, more than the weight gradient's persistent grid (accumulators carry across lines, both LDS buffers in use); the others: ragged,
    unequal line lengths for the two passes"""
    _exact_gates(_exact_case(B, A, h, w))


def test_data_gradient_with_more_chunks_than_its_grid():
    """(9, 5, 32, 32): 288 five-line chunks per pass for 256 blocks"""
    _exact_gates(_exact_case(9, 5, 32, 32))


# ---- against fp64 autograd of the unrounded operands ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _auto_case(B, A, h, w):
    """_epi_case with its random w2, slope 0.1, y given: the fp64 autograd reference of tests/test_gpu_bwd_ops.py::test_epiconv_hv_bwd_every_form"""
    x, w0, w2, dyh, dyv, dx0 = _epi_case(B, A, h, w)
    xr, w0r, w2r = x.double().requires_grad_(True), w0.double().requires_grad_(True), w2.double().requires_grad_(True)

    def epi(t):
        e = F.leaky_relu(F.conv2d(t, w0r, **_kw(A)), 0.1)
        return e, _ps1d(F.leaky_relu(F.conv2d(e, w2r), 0.1), A)
    e_h, yh = epi(xr)
    e_v, yv = epi(xr.permute(0, 1, 3, 2).contiguous())
    yv = yv.permute(0, 1, 3, 2)
    ((yh * dyh.double()).sum() + (yv * dyv.double()).sum()).backward()
    xv = capi.nchw_to_vcl(x.cuda(), A, 1)
    out = torch.full((xv.shape[0], 64), SENTINEL, device="cuda")
    capi.nchw_to_vcl(yh.detach().float().cuda(), A, 1, out=out, choff=0)
    capi.nchw_to_vcl(yv.detach().float().contiguous().cuda(), A, 1, out=out, choff=32)
    eh, ev = _e_rows(e_h.detach(), B, A, h, w, 0), _e_rows(e_v.detach(), B, A, h, w, 1)
    assert bool((out != 0).all()) and bool((eh != 0).all()) and bool((ev != 0).all())
    return dict(geom=(B, A, h, w), x=x, w0=w0, w2=w2, dx0=dx0, out=out, xv=xv, eh=eh, ev=ev, dyb=_dy_buffer(dyh, dyv, A),
                dx64=xr.grad + dx0.double(), dw0_64=w0r.grad, dw2_64=w2r.grad)


def test_it_really_is_bf16_and_the_default_is_untouched():
    c = _auto_case(2, 5, 32, 32)
    dx_d, dw0_d, dw2_d = _run(c, DEFAULT, 0.1)
    dx, dw0, dw2 = _run(c, BF16, 0.1)
    to_def = (rel(dw0, dw0_d), rel(dx - c["dx0"], dx_d - c["dx0"]))
    to_64 = (rel(dw0, c["dw0_64"]), rel(dx.double() - c["dx0"].double(), c["dx64"] - c["dx0"].double()))
    print(f"rel-L2 (dw0, dx) of the mode to the default {to_def[0]:.2e} {to_def[1]:.2e}, to fp64 autograd {to_64[0]:.2e} {to_64[1]:.2e}")
    assert min(to_def) > 1e-3
    assert max(to_64) <= 1e-2
    assert torch.equal(dw2, dw2_d)
    again = _run(c, DEFAULT, 0.1)
    assert all(torch.equal(a, b) for a, b in zip(again, (dx_d, dw0_d, dw2_d)))
    _close(dx_d, c["dx64"], "dx")
    _close(dw0_d, c["dw0_64"], "dw0")
    _close(dw2_d, c["dw2_64"], "dw2")


@pytest.mark.parametrize("B,A,h,w", [(2, 3, 8, 8), (1, 7, 5, 6), (2, 1, 9, 7), (1, 5, 33, 36)])
def test_the_mode_changes_no_bit_where_nothing_is_covered(B, A, h, w):
    assert (B, A, h, w) in EPI_GEOMS
    c = _auto_case(B, A, h, w)
    assert all(torch.equal(a, b) for a, b in zip(_run(c, BF16, 0.1), _run(c, DEFAULT, 0.1)))


@pytest.mark.parametrize("B,A,h,w", [(1, 5, 40, 24), (1, 5, 24, 40)])
def test_one_covered_pass_moves_dx_only(B, A, h, w):
    """one pass has lines of 24 pixels (the EPI-line data gradient), the other of 40 (the gather-GEMM); the merged weight gradient does not apply"""
    assert (B, A, h, w) in EPI_GEOMS
    c = _auto_case(B, A, h, w)
    dx_d, dw0_d, dw2_d = _run(c, DEFAULT, 0.1)
    dx, dw0, dw2 = _run(c, BF16, 0.1)
    assert torch.equal(dw0, dw0_d) and torch.equal(dw2, dw2_d)
    assert not torch.equal(dx, dx_d)
    r = rel(dx.double() - c["dx0"].double(), c["dx64"] - c["dx0"].double())
    print(f"{(B, A, h, w)}: dx rel-L2 to fp64 autograd {r:.2e}")
    assert r <= 1e-2


def test_the_gather_selectors_win(monkeypatch):
    c = _auto_case(2, 5, 32, 32)
    _select(monkeypatch, LFSR_WGRAD_EPI="gather", LFSR_DGRAD_EPI="gather")
    try:
        assert all(torch.equal(a, b) for a, b in zip(_run(c, BF16, 0.1), _run(c, DEFAULT, 0.1)))
    finally:
        _select(monkeypatch)


# ---- memory the call must not touch, refusals ---------------------------------------------------------------------------------------------------------------
def _raw(c, mode, ws_floats_given, slope=0.1, A=None, dx_fill=SENTINEL):
    """the C entry point on sentinel-filled outputs (dx, which is accumulated into: dx_fill) and a workspace with a sentinel band behind workspace_floats
    -> (rc, dx, dw0, dw2, band)"""
    lib, (B, A0, h, w) = capi.load(), c["geom"]
    A = A or A0
    need = lib.lfsr_epiconv_hv_bwd_workspace_floats(B, A0, h, w)
    ws = torch.full((need + BAND,), SENTINEL, device="cuda")
    dx = torch.full((c["xv"].shape[0], 64), dx_fill, device="cuda")
    dw0, dw2 = torch.full(c["w0"].shape, SENTINEL, device="cuda"), torch.full(c["w2"].shape, SENTINEL, device="cuda")
    w0g, w2g = c["w0"].cuda(), c["w2"].cuda()
    with branch_grad(mode):
        rc = lib.lfsr_epiconv_hv_bwd(P(c["dyb"]), 80, 8, 48, P(c["out"]), 64, 0, 32, P(c["xv"]), P(c["eh"]), P(c["ev"]), P(w0g), P(w2g), P(dx), P(dw0), P(dw2),
                                     P(ws), need + ws_floats_given, B, A, h, w, slope, capi.stream_ptr())
        torch.cuda.synchronize()
    return rc, dx, dw0, dw2, ws[need:]


@pytest.mark.parametrize("mode", [DEFAULT, BF16])
def test_strided_dy_workspace_band_and_refusals(mode):
    """dy at channel offsets 8 / 48 of 80-float rows (every case of this file); nothing behind workspace_floats is written; one float short: LFSR_E_WS, even angRes:
    LFSR_E_ARG, both with dx, dw0 and dw2 untouched -- in the mode as without it"""
    c = _auto_case(1, 5, 6, 9)
    rc, dx, dw0, dw2, band = _raw(c, mode, 0, dx_fill=0.0)
    assert rc == 0 and bool((band == SENTINEL).all())
    assert bool((c["dyb"][:, :8] == SENTINEL).all()) and bool((c["dyb"][:, 40:48] == SENTINEL).all())
    for t in (dx, dw0, dw2):
        assert bool(torch.isfinite(t).all()) and not bool((t == SENTINEL).any())
    want = _run(dict(c, dx0=torch.zeros_like(c["dx0"])), mode, 0.1)      # the same call through capi: the band and the exact workspace size change nothing
    B, A, h, w = c["geom"]
    assert torch.equal(capi.vcl_to_nchw(dx, B, 64, A, h, w, 1).cpu(), want[0]) and torch.equal(dw0.cpu(), want[1]) and torch.equal(dw2.cpu(), want[2])
    for rc_want, kw in ((E_WS, dict(ws_floats_given=-1)), (E_ARG, dict(ws_floats_given=0, A=4))):
        rc, dx, dw0, dw2, band = _raw(c, mode, **kw)
        assert rc == rc_want
        assert all(bool((t == SENTINEL).all()) for t in (dx, dw0, dw2, band))


def test_determinism_and_batch_invariance():
    c2 = _exact_case(2, 5, 32, 32)
    a, b = _run(c2, BF16, 0.25), _run(c2, BF16, 0.25)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    npix, nepi = 25 * 32 * 32, 5 * 32 * 32
    c1 = dict(c2, geom=(1, 5, 32, 32), dx0=c2["dx0"][:1], xv=c2["xv"][:npix].contiguous(), eh=c2["eh"][:nepi].contiguous(), ev=c2["ev"][:nepi].contiguous(),
              dyb=c2["dyb"][:npix].contiguous())
    dx1, dw0_1, _ = _run(c1, BF16, 0.25)
    assert torch.equal(dx1[0], a[0][0])
    assert not torch.equal(dw0_1, a[1])


# ---- whole DistgSSR steps -------------------------------------------------------------------------------------------------------------------------------------------
LAST = "disentg.Group.3.Block.3."


@pytest.mark.parametrize("A,s,B,h,w", [(5, 2, 1, 8, 8), (3, 2, 2, 6, 8)])
def test_distgssr_whole_model(A, s, B, h, w, monkeypatch):
    sd, x, label_np, g64, gamp = _distg_refs(A, s, B, h, w)
    names = [k for k, _ in TH.distg_spec(A, s)]
    M = _distg_plugin()
    net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net = net.to("cuda:0").train()
    assert [k for k, _ in net.named_parameters()] == names and len(names) == 137
    xg, label = torch.from_numpy(x).cuda(), torch.from_numpy(label_np).cuda()
    y_def, l_def, g_def, b_def = _step(net, xg, label)
    masks = TH.distg_hip_masks_flat(net._rt, xg)          # the default forward's LeakyReLU decisions (the forward does not read the switch)
    with branch_grad(BF16):
        y, l, g, b = _step(net, xg, label)
        assert torch.equal(torch.cat([p.grad.reshape(-1) for p in net.parameters()]), net.grad_bucket)
        # one stream: the same launches in another order, the same bits
        monkeypatch.setenv("LFSR_BWD_OVERLAP", "0")
        _, _, _, b_one = _step(net, xg, label)
        monkeypatch.delenv("LFSR_BWD_OVERLAP")
    assert torch.equal(y, y_def) and l == l_def           # the forward does not read the switch
    assert torch.equal(b_one, b)
    if A != 5:                                            # nothing is covered
        assert torch.equal(b, b_def)
    else:
        assert not torch.equal(b, b_def)
        same = [k for k in names if (k.startswith(LAST) and k != LAST + "EPIConv.0.weight") or k in ("disentg.conv.weight", "disentg.Group.3.conv.weight")
                or k.startswith("upsample.")]
        assert len(same) == 7 + 2 + 3
        for k in same:                                    # nothing upstream of these reads the mode
            assert np.array_equal(g[k], g_def[k]), k
        assert not np.array_equal(g[LAST + "EPIConv.0.weight"], g_def[LAST + "EPIConv.0.weight"])
    # every parameter against fp64 autograd under the HIP forward's decisions, not above autocast's error for that parameter
    forced, flips = TH.distg_forced_fp64_grads(net._rt, xg, sd, x, label_np, A, s, masks=masks)
    e = {k: _rel_np(g[k], forced[k]) for k in names}
    e_amp = {k: _rel_np(gamp[k], g64[k]) for k in names}
    ratio = {k: e_amp[k] / max(e[k], 1e-30) for k in names}
    eb, eb_amp = _rel_np(_flat(g, names), _flat(forced, names)), _rel_np(_flat(gamp, names), _flat(g64, names))
    v = np.array(list(e.values()))
    kmin = min(ratio, key=ratio.get)
    print(f"distgssr {(A, s, B, h, w)} bf16 EPIConv.0 gradients: per-parameter rel-L2 median {np.median(v):.2e} max {v.max():.2e}, bucket {eb:.2e}; "
          f"autocast median {np.median(list(e_amp.values())):.2e} max {max(e_amp.values()):.2e}, bucket {eb_amp:.2e}; "
          f"smallest autocast / hip ratio {ratio[kmin]:.2f} ({kmin}); decisions differing from fp64's own {flips}")
    bad = {k: (e[k], e_amp[k]) for k in names if not e[k] <= e_amp[k]}
    assert not bad, bad
    assert eb <= eb_amp
    # with the 3x3 convs' gradients and the forward on bf16 as well: the bucket against plain fp64 autograd, not above autocast's
    with TH.arithmetic(capi.ARITH_BF16), grad_arithmetic(capi.GRAD_ARITH_BF16), branch_grad(BF16):
        _, _, g2, _ = _step(net, xg, label)
    eb2 = _rel_np(_flat(g2, names), _flat(g64, names))
    print(f"distgssr {(A, s, B, h, w)} bf16 forward + every bf16 gradient: bucket rel-L2 {eb2:.2e}, autocast {eb_amp:.2e} (ratio {eb_amp / eb2:.2f})")
    assert eb2 <= eb_amp
    # the default is what it was
    _, _, _, b_again = _step(net, xg, label)
    assert torch.equal(b_again, b_def)
