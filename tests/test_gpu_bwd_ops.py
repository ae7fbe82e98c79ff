"""GPU: the operator-level backward entry points of the C ABI (SURVEY 8b export list) through ctypes, against fp64 autograd over stock
torch CPU ops of the same layer (what the reference's train.py:256-264 differentiates, in double precision), and the RCCL all-reduce entry
point.  Every comparison holds two gates: rel-L2 <= 1e-4 per tensor and, element by element, the project's forward gate
max|err| <= 1e-4 * max(1, max|ref|) -- a wrong border row of one image or one wrong element of a weight gradient can hide inside a tensor's
norm.  The kernel forms behind each entry point are selected with monkeypatch.setenv (tests/conftest.py makes the selectors live)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lfsr_amd import capi

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)


def _vcl(t):       # (n_img, C, h, w) -> (n_img*h*w, C) contiguous on the GPU
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous().cuda()


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


SENTINEL = -2.0 ** 100
BAND = 1 << 16
E_ARG, E_WS = -1, -2
SELECTORS = ("LFSR_DGRAD3", "LFSR_WGRAD3", "LFSR_DGRAD_PW", "LFSR_WGRAD_PW", "LFSR_DGRAD_ANG", "LFSR_WGRAD_EPI", "LFSR_DGRAD_EPI")


def _close(got, ref, what=""):
    """both gates: rel-L2 <= 1e-4 and max|err| <= 1e-4 * max(1, max|ref|), against an fp64 reference"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what
    r, e, tol = _rel(got, ref), float((got - ref).abs().max()), 1e-4 * max(1.0, float(ref.abs().max()))
    assert r <= 1e-4 and e <= tol, (what, r, e, tol)


def _select(monkeypatch, **env):
    """exactly the given selectors (None / "" = unset)"""
    for k in SELECTORS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if v:
            monkeypatch.setenv(k, v)


def _embed(rows, stride, choff):
    """rows (n, c) -> an (n, stride) fp32 GPU buffer holding them at channel offset choff, every other channel the sentinel"""
    buf = torch.full((rows.shape[0], stride), SENTINEL, dtype=torch.float32)
    buf[:, choff:choff + rows.shape[1]] = rows.float()
    return buf.cuda()


def _others_intact(buf, choff, c):
    return bool((buf[:, :choff] == SENTINEL).all()) and bool((buf[:, choff + c:] == SENTINEL).all())


@pytest.mark.parametrize("n_img,h,w", [(50, 32, 32), (7, 13, 40), (3, 5, 6)])
def test_conv3x3_dgrad_wgrad(n_img, h, w, monkeypatch):
    g = torch.Generator().manual_seed(n_img)
    x = torch.randn(n_img, 64, h, w, generator=g)
    wt = torch.randn(64, 64, 3, 3, generator=g) * 0.05
    dy = torch.randn(n_img, 64, h, w, generator=g)
    skip = torch.randn(n_img, 64, h, w, generator=g)
    pre = torch.randn(n_img, 64, h, w, generator=g)             # pre-activation of the layer in front: x = lrelu(pre)
    xin = F.leaky_relu(pre, 0.1)
    x64 = xin.double().requires_grad_(True)
    wr = wt.double().requires_grad_(True)
    F.conv2d(x64, wr, padding=1).backward(dy.double())
    dx_ref, dw_ref = x64.grad, wr.grad
    wT = capi.pack_conv_weight_T(wt.cuda())
    dx = capi.conv3x3_dgrad(_vcl(dy), wT, n_img, h, w)
    assert _rel(dx.cpu(), _vcl_cpu(dx_ref)) <= 1e-4
    _close(dx, _vcl_cpu(dx_ref))
    # through the LeakyReLU in front (mask from the saved activation) plus a skip gradient
    act = F.leaky_relu(pre, 0.1)
    dx2 = capi.conv3x3_dgrad(_vcl(dy), wT, n_img, h, w, res1=_vcl(skip), act=_vcl(act), act_slope=0.1)
    ref2 = dx_ref * torch.where(act > 0, 1.0, 0.1) + skip
    assert _rel(dx2.cpu(), _vcl_cpu(ref2)) <= 1e-4
    _close(dx2, _vcl_cpu(ref2))
    for sel in ("", "direct"):          # the Winograd-domain (F(2x2,3x3) adjoint) kernel, default, and the direct-form one
        _select(monkeypatch, LFSR_WGRAD3=sel)
        dw = capi.conv3x3_wgrad(_vcl(dy), _vcl(xin.detach()), n_img, h, w)
        assert _rel(dw.cpu(), dw_ref) <= 1e-4, sel
        _close(dw, dw_ref, sel)
        dw2 = capi.conv3x3_wgrad(_vcl(dy), _vcl(xin.detach()), n_img, h, w, dw=dw.clone())      # accumulate
        assert _rel(dw2.cpu(), 2 * dw_ref) <= 1e-4, sel
        _close(dw2, 2 * dw_ref, sel)
    _select(monkeypatch)


def _vcl_cpu(t):
    return t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("M,cin", [(25600, 144), (3000, 144)])
def test_pointwise_dgrad_wgrad(M, cin):
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, cin, generator=g)
    wt = (torch.randn(64, cin, generator=g) * 0.1)
    dy = torch.randn(M, 64, generator=g)
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    F.linear(xr, wr).backward(dy.double())
    wT = capi.pack_conv_weight_T(wt.reshape(64, cin, 1, 1).cuda())
    dx = capi.pointwise_dgrad(dy.cuda(), wT, cin)
    assert _rel(dx.cpu(), xr.grad) <= 1e-4
    _close(dx, xr.grad)
    dxm = capi.pointwise_dgrad(dy.cuda(), wT, cin, act=x.cuda(), act_slope=0.1)
    assert _rel(dxm.cpu(), xr.grad * torch.where(x > 0, 1.0, 0.1)) <= 1e-4
    _close(dxm, xr.grad * torch.where(x > 0, 1.0, 0.1))
    dw = capi.pointwise_wgrad(dy.cuda(), x.cuda(), 64, cin)
    assert _rel(dw.cpu(), wr.grad) <= 1e-4
    _close(dw, wr.grad)


def _ps1d(x, f):      # DistgSSR.py:114-131
    B, fC, Hh, Ww = x.shape
    return x.reshape(B, f, fC // f, Hh, Ww).permute(0, 2, 3, 4, 1).reshape(B, fC // f, Hh, Ww * f)


@pytest.mark.parametrize("B,A,h,w", [(2, 5, 32, 32), (1, 5, 6, 9), (2, 3, 8, 8)])
def test_angconv_bwd_vs_autograd(B, A, h, w):
    """lfsr_angconv_bwd against autograd of the reference's AngConv layers (DistgSSR.py:84-90) on stock torch CPU ops: dx (accumulated into a
    given gradient), dW0, dW2; stage-1 activation taken from lfsr_angconv_fwd's tmp output"""
    g = torch.Generator().manual_seed(B * 100 + h)
    x = torch.randn(B, 64, h * A, w * A, generator=g)
    w0 = torch.randn(16, 64, A, A, generator=g) * (1.0 / (64 * A * A) ** 0.5)
    w2 = torch.randn(16 * A * A, 16, 1, 1, generator=g) * 0.25
    dy = torch.randn(B, 16, h * A, w * A, generator=g)
    dx0 = torch.randn(B, 64, h * A, w * A, generator=g)
    xr, w0r, w2r = x.double().requires_grad_(True), w0.double().requires_grad_(True), w2.double().requires_grad_(True)
    y_ref = F.pixel_shuffle(F.leaky_relu(F.conv2d(F.leaky_relu(F.conv2d(xr, w0r, stride=A), 0.1), w2r), 0.1), A)
    y_ref.backward(dy.double())
    xv = capi.nchw_to_vcl(x.cuda(), A, 1)
    out = torch.zeros((xv.shape[0], 16), device="cuda")
    a16 = torch.empty((B * h * w, 16), device="cuda")
    capi.angconv(xv, capi.pack_conv_weight(w0.cuda()), capi.pack_conv_weight(w2.cuda(), perm=1, ch=16), B, A, h, w, 0.1, out, 0, tmp=a16)
    assert float((capi.vcl_to_nchw(out, B, 16, A, h, w, 1).cpu() - y_ref.detach()).abs().max()) <= 1e-4
    dxv = capi.nchw_to_vcl(dx0.cuda(), A, 1)
    dw0, dw2 = capi.angconv_bwd(capi.nchw_to_vcl(dy.cuda(), A, 1), 0, out, 0, xv, a16, w0.cuda(), w2.cuda(), dxv, B, A, h, w)
    assert _rel(capi.vcl_to_nchw(dxv, B, 64, A, h, w, 1).cpu() - dx0, xr.grad) <= 1e-4
    assert _rel(dw0.cpu(), w0r.grad) <= 1e-4
    assert _rel(dw2.cpu(), w2r.grad) <= 1e-4
    _close(capi.vcl_to_nchw(dxv, B, 64, A, h, w, 1).cpu(), xr.grad + dx0, "dx")      # (dx0 of order 1: its rounding in the sum is inside the gate)
    _close(dw0, w0r.grad, "dw0")
    _close(dw2, w2r.grad, "dw2")


@pytest.mark.parametrize("B,A,h,w", [(2, 5, 32, 32), (1, 5, 6, 9), (2, 3, 8, 8)])
def test_epiconv_hv_bwd_vs_autograd(B, A, h, w):
    """lfsr_epiconv_hv_bwd against autograd of the reference's EPIConv applied to the tensor and to its transpose with shared weights
    (DistgSSR.py:91-97,108): dx accumulated, dW0 / dW2 summed over both passes; gradients arrive in two channel slices of one VCL buffer"""
    g = torch.Generator().manual_seed(B * 100 + w)
    x = torch.randn(B, 64, h * A, w * A, generator=g)
    w0 = torch.randn(32, 64, 1, A * A, generator=g) * (1.0 / (64 * A * A) ** 0.5)
    w2 = torch.randn(32 * A, 32, 1, 1, generator=g) * 0.18
    dyh = torch.randn(B, 32, h * A, w * A, generator=g)
    dyv = torch.randn(B, 32, h * A, w * A, generator=g)
    dx0 = torch.randn(B, 64, h * A, w * A, generator=g)
    xr, w0r, w2r = x.double().requires_grad_(True), w0.double().requires_grad_(True), w2.double().requires_grad_(True)

    def epi(t):
        e = F.leaky_relu(F.conv2d(t, w0r, stride=(1, A), padding=(0, A * (A - 1) // 2)), 0.1)
        return _ps1d(F.leaky_relu(F.conv2d(e, w2r), 0.1), A)
    yh, yv = epi(xr), epi(xr.permute(0, 1, 3, 2).contiguous()).permute(0, 1, 3, 2)
    (yh * dyh.double()).sum().backward(retain_graph=True)
    (yv * dyv.double()).sum().backward()
    xv = capi.nchw_to_vcl(x.cuda(), A, 1)
    w0p, w2p = capi.pack_conv_weight(w0.cuda()), capi.pack_conv_weight(w2.cuda())
    out = torch.zeros((xv.shape[0], 64), device="cuda")
    eh, ev = torch.empty((B * A * h * w, 32), device="cuda"), torch.empty((B * A * h * w, 32), device="cuda")
    capi.epiconv(xv, w0p, w2p, B, A, h, w, False, 0.1, out, 0, tmp=eh)
    capi.epiconv(xv, w0p, w2p, B, A, h, w, True, 0.1, out, 32, tmp=ev)
    assert float((capi.vcl_to_nchw(out, B, 32, A, h, w, 1, choff=0).cpu() - yh.detach()).abs().max()) <= 1e-4
    assert float((capi.vcl_to_nchw(out, B, 32, A, h, w, 1, choff=32).cpu() - yv.detach()).abs().max()) <= 1e-4
    dyb = torch.zeros((xv.shape[0], 80), device="cuda")             # dLoss/dy_h at channels 8..39, dLoss/dy_v at 48..79 of one buffer
    capi.nchw_to_vcl(dyh.cuda(), A, 1, out=dyb, choff=8)
    capi.nchw_to_vcl(dyv.cuda(), A, 1, out=dyb, choff=48)
    dxv = capi.nchw_to_vcl(dx0.cuda(), A, 1)
    dw0, dw2 = capi.epiconv_hv_bwd(dyb, 8, 48, out, 0, 32, xv, eh, ev, w0.cuda(), w2.cuda(), dxv, B, A, h, w)
    assert _rel(capi.vcl_to_nchw(dxv, B, 64, A, h, w, 1).cpu() - dx0, xr.grad) <= 1e-4
    assert _rel(dw0.cpu(), w0r.grad) <= 1e-4
    assert _rel(dw2.cpu(), w2r.grad) <= 1e-4
    _close(capi.vcl_to_nchw(dxv, B, 64, A, h, w, 1).cpu(), xr.grad + dx0, "dx")
    _close(dw0, w0r.grad, "dw0")
    _close(dw2, w2r.grad, "dw2")


def test_upsample_head_dgrad():
    B, A, h, w, s = 2, 5, 8, 8, 4
    g = torch.Generator().manual_seed(3)
    f = torch.randn(B, 64, A * h, A * w, generator=g)                      # SAI-mosaic NCHW features (after MacPI2SAI)
    w0 = torch.randn(64 * s * s, 64, 1, 1, generator=g) * 0.1
    b0 = torch.randn(64 * s * s, generator=g) * 0.1
    w2 = torch.randn(1, 64, 1, 1, generator=g) * 0.1
    dout = torch.randn(B, 1, A * h * s, A * w * s, generator=g)
    fr = f.double().requires_grad_(True)
    F.conv2d(F.pixel_shuffle(F.conv2d(fr, w0.double(), b0.double()), s), w2.double()).backward(dout.double())
    lib = capi.load()
    wf = torch.empty(s * s * 64, device="cuda"); bf = torch.empty(s * s, device="cuda")
    w0d, b0d, w2d, doutd = w0.cuda(), b0.cuda(), w2.cuda(), dout.cuda()          # (kept alive across the asynchronous launches)
    capi.check(lib.lfsr_fold_head(capi.dev_ptr(w0d), capi.dev_ptr(b0d), capi.dev_ptr(w2d), capi.dev_ptr(wf), capi.dev_ptr(bf), 64, s,
                                  capi.stream_ptr()), "fold_head")
    npix = B * A * A * h * w
    df = torch.empty(npix, 64, device="cuda"); g16 = torch.empty(npix, 16, device="cuda")
    capi.check(lib.lfsr_upsample_head_dgrad(capi.dev_ptr(doutd), capi.dev_ptr(wf), capi.dev_ptr(df), capi.dev_ptr(g16), B, A, h, w, s,
                                            capi.stream_ptr()), "upsample_head_dgrad")
    got = capi.vcl_to_nchw(df, B, 64, A, h, w, 0).cpu()                   # VCL -> SAI mosaic NCHW
    assert _rel(got, fr.grad) <= 1e-4
    _close(got, fr.grad)


def test_rccl_allreduce_single_rank():
    """world size 1 on the one GPU of this box: the RCCL communicator is created through the C ABI and the in-place sum is the identity;
    the N > 1 path is the same call (the driver's multi-GPU leg exercises torch.distributed's RCCL backend by default)."""
    if not capi.load().lfsr_comm_available():
        pytest.skip("librccl not present")
    comm = capi.RcclComm(1, 0)
    t = torch.arange(3581568, dtype=torch.float32, device="cuda") * 1e-3        # the flat DistgSSR gradient bucket's size
    ref = t.clone()
    comm.allreduce_(t)
    torch.cuda.synchronize()
    assert torch.equal(t, ref)
    comm.close()


# ---------------------------------------------------------------------------------------------------------------------
# every operator in every kernel form, with the operands laid out as the models lay them out (strided, at channel offsets, inside wider
# buffers) and beyond, element by element against fp64
# ---------------------------------------------------------------------------------------------------------------------
C3_GEOMS = [(50, 32, 32), (7, 13, 40), (3, 5, 6), (2, 33, 70)]
P = capi.dev_ptr


@functools.lru_cache(maxsize=None)
def _conv3_case(n_img, h, w):
    """fp32 operands and fp64 references of one 3x3 layer behind a LeakyReLU(0.1): act (the conv's input, the saved activation; exact zeros
    planted, where the derivative is the slope: the act > 0 convention), wt, dy, r1 -> dx = conv^T(dy) * LeakyReLU'(act) + r1 and dw"""
    g = torch.Generator().manual_seed(1000 + n_img)
    act = F.leaky_relu(torch.randn(n_img, 64, h, w, generator=g), 0.1)
    act.view(-1)[::97] = 0.0
    wt = torch.randn(64, 64, 3, 3, generator=g) * 0.05
    dy = torch.randn(n_img, 64, h, w, generator=g)
    r1 = torch.randn(n_img, 64, h, w, generator=g)
    x64, w64 = act.double().requires_grad_(True), wt.double().requires_grad_(True)
    F.conv2d(x64, w64, padding=1).backward(dy.double())
    dx = x64.grad * torch.where(act > 0, 1.0, 0.1).double() + r1.double()
    return act, wt, dy, r1, _vcl_cpu(dx), w64.grad


def _dgrad3(case, n_img, h, w, lay):
    """lfsr_conv3x3_dgrad with (stride, channel offset) per operand from `lay`; -> (dx rows, the whole dx buffer)"""
    act, wt, dy, r1, _, _ = case
    wT = capi.pack_conv_weight_T(wt.cuda())
    bufs = {k: _embed(_vcl_cpu(t), *lay[k]) for k, t in (("dy", dy), ("act", act), ("r1", r1))}
    dx = torch.full((n_img * h * w, lay["dx"][0]), SENTINEL, device="cuda")
    capi.check(capi.load().lfsr_conv3x3_dgrad(P(bufs["dy"]), *lay["dy"], P(wT), P(dx), *lay["dx"], P(bufs["r1"]), *lay["r1"], P(bufs["act"]), *lay["act"], 0.1,
                                              n_img, h, w, capi.stream_ptr()), "conv3x3_dgrad")
    torch.cuda.synchronize()
    assert _others_intact(dx, lay["dx"][1], 64)
    return dx[:, lay["dx"][1]:lay["dx"][1] + 64].contiguous(), dx


# dy and act as DistgSSR's backward has them (the 144-wide concat rows; act at the fuse.0 input's offset 64), r1 and dx inside wider buffers
MODEL_LAYOUT = {"dy": (144, 16), "act": (144, 64), "r1": (80, 12), "dx": (96, 20)}


@pytest.mark.parametrize("sel", ["", "wino2", "halo"])
@pytest.mark.parametrize("n_img,h,w", C3_GEOMS)
def test_conv3x3_dgrad_every_form_strided_operands(n_img, h, w, sel, monkeypatch):
    case = _conv3_case(n_img, h, w)
    _select(monkeypatch, LFSR_DGRAD3=sel)
    dx, _ = _dgrad3(case, n_img, h, w, MODEL_LAYOUT)
    _close(dx, case[4], sel)


def test_conv3x3_dgrad_unaligned_operands_run_the_gather_gemm(monkeypatch):
    """a channel offset of 2 on act, r1 and dx: no 16-byte channel vectors, so whatever is selected the gather-GEMM runs -- the same bits under
    every selection, other bits than the tile kernel's on aligned operands, and right.  dy off the 16-byte grid is refused by every kernel,
    the gather-GEMM included: LFSR_E_ARG and nothing written"""
    n_img, h, w = 7, 13, 40
    case = _conv3_case(n_img, h, w)
    lay = {"dy": (144, 16), "act": (66, 2), "r1": (66, 2), "dx": (70, 2)}
    dyb, dxb = _embed(_vcl_cpu(case[2]), 70, 2), torch.full((n_img * h * w, 64), SENTINEL, device="cuda")
    rc = capi.load().lfsr_conv3x3_dgrad(P(dyb), 70, 2, P(capi.pack_conv_weight_T(case[1].cuda())), P(dxb), 64, 0, None, 0, 0, None, 0, 0, 1.0, n_img, h, w, capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == E_ARG and bool((dxb == SENTINEL).all())
    got = []
    for sel in ("", "wino2", "halo"):
        _select(monkeypatch, LFSR_DGRAD3=sel)
        dx, _ = _dgrad3(case, n_img, h, w, lay)
        _close(dx, case[4], sel)
        got.append(dx)
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    for k in ("act", "r1", "dx"):                  # each operand alone off the 16-byte grid is enough
        _select(monkeypatch)
        dx, _ = _dgrad3(case, n_img, h, w, dict(MODEL_LAYOUT, **{k: (MODEL_LAYOUT[k][0] + 2, MODEL_LAYOUT[k][1] + 2)}))
        _close(dx, case[4], k)
        assert torch.equal(dx, got[0]), k
    aligned, _ = _dgrad3(case, n_img, h, w, MODEL_LAYOUT)
    assert not torch.equal(aligned, got[0])


def test_conv3x3_dgrad_selected_forms_differ_from_the_default(monkeypatch):
    """LFSR_DGRAD3 really changes the kernel: F(4x4), F(2x2) and the direct 9-tap form give three different roundings of the same sums"""
    n_img, h, w = 7, 13, 40
    case = _conv3_case(n_img, h, w)
    out = {}
    for sel in ("", "wino2", "halo"):
        _select(monkeypatch, LFSR_DGRAD3=sel)
        out[sel], _ = _dgrad3(case, n_img, h, w, MODEL_LAYOUT)
    assert not torch.equal(out[""], out["wino2"]) and not torch.equal(out[""], out["halo"]) and not torch.equal(out["wino2"], out["halo"])


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("sel", ["", "direct"])
@pytest.mark.parametrize("n_img,h,w", C3_GEOMS + [(300, 6, 6)])       # (300, 6, 6): more tiles than the 256 persistent blocks on small views
def test_conv3x3_wgrad_every_form_exact_workspace(n_img, h, w, sel, accumulate, monkeypatch):
    act, wt, dy, _, _, dw_ref = _conv3_case(n_img, h, w)
    lib, st = capi.load(), capi.stream_ptr()
    _select(monkeypatch, LFSR_WGRAD3=sel)
    dyb, xb = _embed(_vcl_cpu(dy), 144, 64), _vcl(act)
    n_ws = lib.lfsr_conv3x3_wgrad_workspace_floats(n_img, h, w)
    assert n_ws > 0
    ws = torch.full((n_ws + BAND,), SENTINEL, device="cuda")
    dw0 = torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(5)) * 100.0 if accumulate else torch.full((64, 64, 3, 3), SENTINEL)
    dw = dw0.cuda()
    rc = lib.lfsr_conv3x3_wgrad(P(dyb), 144, 64, P(xb), 64, 0, P(dw), P(ws), n_ws - 1, n_img, h, w, accumulate, st)
    torch.cuda.synchronize()
    assert rc == E_WS and torch.equal(dw.cpu(), dw0) and bool((ws == SENTINEL).all())
    rc = lib.lfsr_conv3x3_wgrad(P(dyb), 144, 64, P(xb), 64, 0, P(dw), P(ws), n_ws, n_img, h, w, accumulate, st)
    torch.cuda.synchronize()
    assert rc == 0 and bool((ws[n_ws:] == SENTINEL).all())
    _close(dw, dw_ref + dw0.double() if accumulate else dw_ref, (sel, accumulate))


def test_conv3x3_wgrad_selected_form_differs_from_the_default(monkeypatch):
    n_img, h, w = 7, 13, 40
    act, wt, dy, _, _, _ = _conv3_case(n_img, h, w)
    out = []
    for sel in ("", "direct"):
        _select(monkeypatch, LFSR_WGRAD3=sel)
        out.append(capi.conv3x3_wgrad(_vcl(dy), _vcl(act), n_img, h, w))
        torch.cuda.synchronize()
    assert not torch.equal(out[0], out[1])


# (cout, cin) of lfsr_pointwise_dgrad / _wgrad: fuse.0 of DistgSSR, and the 1x1 / linear shapes of the LFT and LF_InterNet backward on the same
# launchers (64 and 128 wide tokens, the 256-wide feed-forward and AngBottle input, the 16-column gathered rows of the first convs, and
# LF_InterNet's AngFE.0 rows of A^2 samples padded to a multiple of 4: 12, 28 and 52 columns at angRes 3, 5 and 7, the only K here that is
# neither 16 nor a multiple of 64) and DistgSSR's 16-row folded head
PW_SHAPES = [(64, 144), (64, 64), (64, 128), (64, 256), (64, 16), (64, 12), (64, 28), (64, 52), (16, 64)]


@functools.lru_cache(maxsize=None)
def _pw_case(M, cout, cin):
    g = torch.Generator().manual_seed(M + 7 * cin + cout)
    x = torch.randn(M, cin, generator=g)
    x.view(-1)[::89] = 0.0                      # exact zeros in the saved activation
    wt = torch.randn(cout, cin, generator=g) * 0.1
    dy = torch.randn(M, cout, generator=g)
    xr, wr = x.double().requires_grad_(True), wt.double().requires_grad_(True)
    F.linear(xr, wr).backward(dy.double())
    return x, wt, dy, xr.grad, wr.grad


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("cout,cin", PW_SHAPES)
@pytest.mark.parametrize("M", [1500, 3000, 25600, 70001])
def test_pointwise_dgrad_wgrad_every_form(M, cout, cin, masked, monkeypatch):
    """M = 1500 is below the 2048 rows from which the fuse.0 data gradient leaves the gather-GEMM; 70001 is ragged in every tiling"""
    x, wt, dy, dx_ref, dw_ref = _pw_case(M, cout, cin)
    lib, st = capi.load(), capi.stream_ptr()
    dyb = _embed(dy, cout + 8, 4)
    if cout == 64:
        wT = capi.pack_conv_weight_T(wt.reshape(cout, cin, 1, 1).cuda())
        actb = _embed(x, cin + 12, 8) if masked else None
        ref = dx_ref * torch.where(x > 0, 1.0, 0.1).double() if masked else dx_ref
        got = {}
        for sel in ("", "f32", "gather"):
            _select(monkeypatch, LFSR_DGRAD_PW=sel)
            dx = torch.full((M, cin + 8), SENTINEL, device="cuda")
            capi.check(lib.lfsr_pointwise_dgrad(P(dyb), cout + 8, 4, cout, P(wT), P(dx), cin + 8, 4, cin, P(actb) if masked else None, cin + 12 if masked else 0,
                                                8 if masked else 0, 0.1, M, st), "pointwise_dgrad")
            torch.cuda.synchronize()
            assert _others_intact(dx, 4, cin), sel
            got[sel] = dx[:, 4:4 + cin].contiguous()
            _close(got[sel], ref, sel)
        if cin == 144 and M >= 2048 and masked:  # the selectors reach the fuse.0 shape from 2048 rows on.  Masked, the default is the three-term bf16
            assert not torch.equal(got[""], got["gather"]) and not torch.equal(got[""], got["f32"])   # row kernel: other bits than either fp32 form
        if cin == 144 and M >= 2048 and not masked:    # unmasked, the default is the fp32 row-GEMM already: fp32 MFMA over K = 64 in the order of the
            assert torch.equal(got[""], got["f32"]) and torch.equal(got[""], got["gather"])           # gather-GEMM, the same bits
    _select(monkeypatch)
    xb = _embed(x, cin + 4, 4)
    # (LFSR_WGRAD_PW moves the PW144 form of the weight-gradient dispatcher alone, which only the model driver submits, not this entry point:
    # tests/test_gpu_distgssr_geometries.py::test_fuse0_weight_gradient_streaming_and_generic_form)
    n_ws = lib.lfsr_pointwise_wgrad_workspace_floats(M, cout, cin)
    ws = torch.full((n_ws + BAND,), SENTINEL, device="cuda")
    dw = torch.full((cout, cin), SENTINEL, device="cuda")
    rc = lib.lfsr_pointwise_wgrad(P(dyb), cout + 8, 4, cout, P(xb), cin + 4, 4, cin, P(dw), P(ws), n_ws - 1, M, 0, st)
    torch.cuda.synchronize()
    assert rc == E_WS and bool((dw == SENTINEL).all())
    capi.check(lib.lfsr_pointwise_wgrad(P(dyb), cout + 8, 4, cout, P(xb), cin + 4, 4, cin, P(dw), P(ws), n_ws, M, 0, st), "pointwise_wgrad")
    torch.cuda.synchronize()
    assert bool((ws[n_ws:] == SENTINEL).all())
    _close(dw, dw_ref, "dw")
    dw2 = dw.clone()
    capi.check(lib.lfsr_pointwise_wgrad(P(dyb), cout + 8, 4, cout, P(xb), cin + 4, 4, cin, P(dw2), P(ws), n_ws, M, 1, st), "pointwise_wgrad")      # accumulate
    torch.cuda.synchronize()
    _close(dw2, 2 * dw_ref, "dw accumulated")


@pytest.mark.parametrize("cout,cin", [(32, 64), (64, 6), (64, 0), (128, 64)])
def test_pointwise_refused_shapes_write_nothing(cout, cin):
    """lfsr_pointwise_dgrad is built for cout = 64 and whole float4 rows; lfsr_pointwise_wgrad for cout <= 64: LFSR_E_ARG, nothing written"""
    lib, st, M = capi.load(), capi.stream_ptr(), 3000
    dy = torch.randn(M, 128, device="cuda")
    x = torch.randn(M, 64, device="cuda")
    wT = torch.randn(256 * 256, device="cuda")
    dx = torch.full((M, 64), SENTINEL, device="cuda")
    rc = lib.lfsr_pointwise_dgrad(P(dy), 128, 0, cout, P(wT), P(dx), 64, 0, cin, None, 0, 0, 1.0, M, st)
    torch.cuda.synchronize()
    assert rc == E_ARG and bool((dx == SENTINEL).all())
    if cout > 64 or cin <= 0:
        dw = torch.full((128, 64), SENTINEL, device="cuda")
        ws = torch.full((1 << 22,), SENTINEL, device="cuda")
        rc = lib.lfsr_pointwise_wgrad(P(dy), 128, 0, cout, P(x), 64, 0, cin, P(dw), P(ws), ws.numel(), M, 0, st)
        torch.cuda.synchronize()
        assert rc == E_ARG and bool((dw == SENTINEL).all()) and bool((ws == SENTINEL).all())


def _ang_case(B, A, h, w):
    g = torch.Generator().manual_seed(B * 100 + h + 31 * A)
    x = torch.randn(B, 64, h * A, w * A, generator=g)
    w0 = torch.randn(16, 64, A, A, generator=g) * (1.0 / (64 * A * A) ** 0.5)
    w2 = torch.randn(16 * A * A, 16, 1, 1, generator=g) * 0.25
    dy = torch.randn(B, 16, h * A, w * A, generator=g)
    dx0 = torch.randn(B, 64, h * A, w * A, generator=g)
    return x, w0, w2, dy, dx0


ANG_GEOMS = [(2, 5, 32, 32), (1, 5, 6, 9), (2, 3, 8, 8), (1, 1, 9, 7), (1, 7, 5, 6), (1, 9, 4, 4), (1, 3, 33, 40)]


@pytest.mark.parametrize("with_y", [True, False])
@pytest.mark.parametrize("B,A,h,w", ANG_GEOMS)
def test_angconv_bwd_every_form(B, A, h, w, with_y, monkeypatch):
    """lfsr_angconv_bwd in its streaming and gather data-gradient forms, with the forward output (the entry point masks dy itself) and with
    y = NULL (dy is already the gradient at the stage-2 pre-activation, as inside the model).  The saved activations handed in are the fp64
    graph's own, rounded to fp32: the decisions are then the reference's, and what is compared is arithmetic"""
    x, w0, w2, dy, dx0 = _ang_case(B, A, h, w)
    xr, w0r, w2r = x.double().requires_grad_(True), w0.double().requires_grad_(True), w2.double().requires_grad_(True)
    a1 = F.leaky_relu(F.conv2d(xr, w0r, stride=A), 0.1)
    y2 = F.leaky_relu(F.conv2d(a1, w2r), 0.1)
    y_ref = F.pixel_shuffle(y2, A)
    y_ref.backward(dy.double())
    xv = capi.nchw_to_vcl(x.cuda(), A, 1)
    yv = capi.nchw_to_vcl(y_ref.detach().float().cuda(), A, 1)
    a16 = a1.detach().float().permute(0, 2, 3, 1).reshape(-1, 16).contiguous().cuda()
    assert bool((yv != 0).all()) and bool((a16 != 0).all())
    if with_y:
        dyv = capi.nchw_to_vcl(dy.cuda(), A, 1)
    else:
        dyv = capi.nchw_to_vcl((dy.double() * torch.where(y_ref.detach() > 0, 1.0, 0.1)).float().cuda(), A, 1)
    got = {}
    for sel in ("", "gather"):
        _select(monkeypatch, LFSR_DGRAD_ANG=sel)
        dxv = capi.nchw_to_vcl(dx0.cuda(), A, 1)
        dw0, dw2 = capi.angconv_bwd(dyv, 0, yv if with_y else None, 0, xv, a16, w0.cuda(), w2.cuda(), dxv, B, A, h, w)
        torch.cuda.synchronize()
        got[sel] = capi.vcl_to_nchw(dxv, B, 64, A, h, w, 1).cpu()
        _close(got[sel], xr.grad + dx0.double(), ("dx", sel))
        _close(dw0, w0r.grad, ("dw0", sel))
        _close(dw2, w2r.grad, ("dw2", sel))
    if (B, A, h, w) == (2, 5, 32, 32):
        assert not torch.equal(got[""], got["gather"])          # the selector really changed the kernel
    _select(monkeypatch)


def _epi_case(B, A, h, w):
    g = torch.Generator().manual_seed(B * 100 + w + 31 * A)
    x = torch.randn(B, 64, h * A, w * A, generator=g)
    w0 = torch.randn(32, 64, 1, A * A, generator=g) * (1.0 / (64 * A * A) ** 0.5)
    w2 = torch.randn(32 * A, 32, 1, 1, generator=g) * 0.18
    dyh = torch.randn(B, 32, h * A, w * A, generator=g)
    dyv = torch.randn(B, 32, h * A, w * A, generator=g)
    dx0 = torch.randn(B, 64, h * A, w * A, generator=g)
    return x, w0, w2, dyh, dyv, dx0


EPI_GEOMS = [(2, 5, 32, 32), (1, 5, 6, 9), (2, 3, 8, 8), (1, 5, 40, 24), (1, 5, 24, 40), (1, 5, 33, 36), (1, 7, 5, 6), (2, 1, 9, 7)]


@pytest.mark.parametrize("with_y", [True, False])
@pytest.mark.parametrize("B,A,h,w", EPI_GEOMS)
def test_epiconv_hv_bwd_every_form(B, A, h, w, with_y, monkeypatch):
    """lfsr_epiconv_hv_bwd with the line forms and the gather forms of the EPIConv.0 gradients: views past 32 pixels on one side (the line form
    for one pass, the gather-GEMM for the other, both accumulating into one dx; the unmerged weight gradient) and on both, angRes 7 and 1"""
    x, w0, w2, dyh, dyv, dx0 = _epi_case(B, A, h, w)
    xr, w0r, w2r = x.double().requires_grad_(True), w0.double().requires_grad_(True), w2.double().requires_grad_(True)

    def epi(t):
        e = F.leaky_relu(F.conv2d(t, w0r, stride=(1, A), padding=(0, A * (A - 1) // 2)), 0.1)
        return e, _ps1d(F.leaky_relu(F.conv2d(e, w2r), 0.1), A)
    e_h, yh = epi(xr)
    e_v, yv = epi(xr.permute(0, 1, 3, 2).contiguous())
    yv = yv.permute(0, 1, 3, 2)
    ((yh * dyh.double()).sum() + (yv * dyv.double()).sum()).backward()
    xv = capi.nchw_to_vcl(x.cuda(), A, 1)
    out = torch.full((xv.shape[0], 64), SENTINEL, device="cuda")
    capi.nchw_to_vcl(yh.detach().float().cuda(), A, 1, out=out, choff=0)
    capi.nchw_to_vcl(yv.detach().float().contiguous().cuda(), A, 1, out=out, choff=32)
    eh = e_h.detach().float().reshape(B, 32, h, A, w).permute(0, 3, 2, 4, 1).reshape(-1, 32).contiguous().cuda()       # rows (b A + u, y, x)
    ev = e_v.detach().float().reshape(B, 32, w, A, h).permute(0, 3, 4, 2, 1).reshape(-1, 32).contiguous().cuda()       # rows (b A + v, y, x)
    assert bool((out != 0).all()) and bool((eh != 0).all()) and bool((ev != 0).all())
    gh, gv = dyh.double(), dyv.double()
    if not with_y:
        gh, gv = gh * torch.where(yh.detach() > 0, 1.0, 0.1), gv * torch.where(yv.detach() > 0, 1.0, 0.1)
    dyb = torch.full((xv.shape[0], 80), SENTINEL, device="cuda")             # dLoss/dy_h at channels 8..39, dLoss/dy_v at 48..79 of one buffer
    capi.nchw_to_vcl(gh.float().cuda(), A, 1, out=dyb, choff=8)
    capi.nchw_to_vcl(gv.float().cuda(), A, 1, out=dyb, choff=48)
    got = {}
    for sel in ("", "gather"):
        _select(monkeypatch, LFSR_WGRAD_EPI=sel, LFSR_DGRAD_EPI=sel)
        dxv = capi.nchw_to_vcl(dx0.cuda(), A, 1)
        dw0, dw2 = capi.epiconv_hv_bwd(dyb, 8, 48, out if with_y else None, 0, 32, xv, eh, ev, w0.cuda(), w2.cuda(), dxv, B, A, h, w)
        torch.cuda.synchronize()
        got[sel] = (capi.vcl_to_nchw(dxv, B, 64, A, h, w, 1).cpu(), dw0.cpu())
        _close(got[sel][0], xr.grad + dx0.double(), ("dx", sel))
        _close(dw0, w0r.grad, ("dw0", sel))
        _close(dw2, w2r.grad, ("dw2", sel))
    if (B, A, h, w) == (2, 5, 32, 32):                  # the selectors really changed the kernels
        assert not torch.equal(got[""][0], got["gather"][0]) and not torch.equal(got[""][1], got["gather"][1])
    _select(monkeypatch)


@pytest.mark.parametrize("A", [2, 4])
def test_branch_backwards_refuse_even_angres(A):
    """lfsr_angconv_bwd and lfsr_epiconv_hv_bwd: LFSR_E_ARG at even A, with dx, dw0 and dw2 untouched"""
    lib, st, B, h, w = capi.load(), capi.stream_ptr(), 1, 6, 5
    npix = B * A * A * h * w
    g = lambda *shape: torch.randn(*shape, device="cuda")
    ws = torch.full((1 << 22,), SENTINEL, device="cuda")
    for name, c1, w0s, w2s, rows in (("ang", 16, (16, 64, A, A), (16 * A * A, 16, 1, 1), B * h * w), ("epi", 32, (32, 64, 1, A * A), (32 * A, 32, 1, 1), B * A * h * w)):
        dy, y, x, a, e2, w0, w2 = g(npix, 64), g(npix, 64), g(npix, 64), g(rows, c1), g(rows, c1), g(*w0s), g(*w2s)
        dx, dw0, dw2 = (torch.full(sh, SENTINEL, device="cuda") for sh in ((npix, 64), w0s, w2s))
        if name == "ang":
            rc = lib.lfsr_angconv_bwd(P(dy), 64, 0, P(y), 64, 0, P(x), P(a), P(w0), P(w2), P(dx), P(dw0), P(dw2), P(ws), ws.numel(), B, A, h, w, 0.1, st)
        else:
            rc = lib.lfsr_epiconv_hv_bwd(P(dy), 64, 0, 32, P(y), 64, 0, 32, P(x), P(a), P(e2), P(w0), P(w2), P(dx), P(dw0), P(dw2), P(ws), ws.numel(), B, A, h, w, 0.1, st)
        torch.cuda.synchronize()
        assert rc == E_ARG, name
        assert all(bool((t == SENTINEL).all()) for t in (dx, dw0, dw2, ws)), name


@pytest.mark.parametrize("B,A,h,w", [(2, 5, 8, 8), (1, 3, 7, 13), (3, 5, 32, 32)])      # the last: 76 800 pixels, the grid-stride loop of k_head_bwd runs
@pytest.mark.parametrize("s", [2, 3, 4])
def test_fold_head_and_upsample_head_dgrad_every_scale(s, B, A, h, w):
    """lfsr_fold_head + lfsr_upsample_head_dgrad: df and g16 (the un-shuffled output gradient, s^2 of 16 columns, the rest zero) against fp64"""
    g = torch.Generator().manual_seed(3 + s)
    f = torch.randn(B, 64, A * h, A * w, generator=g)
    w0 = torch.randn(64 * s * s, 64, 1, 1, generator=g) * 0.1
    b0 = torch.randn(64 * s * s, generator=g) * 0.1
    w2 = torch.randn(1, 64, 1, 1, generator=g) * 0.1
    dout = torch.randn(B, 1, A * h * s, A * w * s, generator=g)
    fr = f.double().requires_grad_(True)
    F.conv2d(F.pixel_shuffle(F.conv2d(fr, w0.double(), b0.double()), s), w2.double()).backward(dout.double())
    t = torch.zeros(B, s * s, A * h, A * w, dtype=torch.float64, requires_grad=True)         # the folded s^2-channel conv's output
    F.pixel_shuffle(t, s).backward(dout.double())
    g16_ref = torch.cat((t.grad, torch.zeros(B, 16 - s * s, A * h, A * w, dtype=torch.float64)), 1)
    lib = capi.load()
    wf = torch.empty(s * s * 64, device="cuda"); bf = torch.empty(s * s, device="cuda")
    w0d, b0d, w2d, doutd = w0.cuda(), b0.cuda(), w2.cuda(), dout.cuda()
    capi.check(lib.lfsr_fold_head(P(w0d), P(b0d), P(w2d), P(wf), P(bf), 64, s, capi.stream_ptr()), "fold_head")
    wf_ref = torch.einsum("k,kqc->qc", w2.double().reshape(64), w0.double().reshape(64, s * s, 64))     # out[ij] = sum_k w2[k] (w0[k s^2 + ij] . f + b0[k s^2 + ij])
    _close(wf.reshape(s * s, 64), wf_ref, "wf")
    _close(bf, torch.einsum("k,kq->q", w2.double().reshape(64), b0.double().reshape(64, s * s)), "bf")
    npix = B * A * A * h * w
    df = torch.full((npix + BAND // 64, 64), SENTINEL, device="cuda"); g16 = torch.full((npix + BAND // 16, 16), SENTINEL, device="cuda")
    capi.check(lib.lfsr_upsample_head_dgrad(P(doutd), P(wf), P(df), P(g16), B, A, h, w, s, capi.stream_ptr()), "upsample_head_dgrad")
    torch.cuda.synchronize()
    assert bool((df[npix:] == SENTINEL).all()) and bool((g16[npix:] == SENTINEL).all())
    _close(capi.vcl_to_nchw(df[:npix].contiguous(), B, 64, A, h, w, 0).cpu(), fr.grad, "df")
    got16 = capi.vcl_to_nchw(g16[:npix].contiguous(), B, 16, A, h, w, 0).cpu()
    _close(got16, g16_ref, "g16")
    assert torch.equal(got16.double(), g16_ref.float().double())            # a copy: exact
