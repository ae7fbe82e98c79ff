"""The operator table of tests/test_gpu_streams.py: C entry point -> builder.  A builder makes the smallest ragged arguments the operator accepts (the shapes of
the operator's own test file where it has one) and returns (call, inputs, scrub) for stream_helpers.run_late: `inputs` are the device tensors the call reads,
`scrub` what it owns (explicit outputs between sentinel bands, explicit workspaces).  Outputs a capi wrapper allocates itself are fresh memory in either leg.

tests/test_stream_table_cpu.py asserts that every entry point of include/lfsr_hip.h whose last parameter is the caller's stream is in OPS, is driven by a
whole-model case of tests/test_gpu_streams.py (MODEL_COVERED) or is in EXEMPT."""
import ctypes as C

MODELS = ("distgssr", "epit", "lft", "internet", "lfssr")
TRAINABLE = ("distgssr", "epit", "lft", "internet")
# what the whole-model cases drive: the plugin's forward (forward), a training step (load_param, finalize, forward_train, backward)
MODEL_COVERED = {f"lfsr_{m}_{fn}" for m in MODELS for fn in ("load_param", "finalize", "forward")} | {f"lfsr_{m}_{fn}" for m in TRAINABLE for fn in ("forward_train", "backward")}
EXEMPT = {
    "lfsr_allreduce": "needs a communicator; run single-rank in tests/test_gpu_bwd_ops.py",
    "lfsr_distgssr_forward_taps": "lfsr_distgssr_forward with copies of five activations; test_distgssr_taps_late runs it at the fused-tail row",
}

OPS = {}
RAG = (3, 7, 13)              # (n_img, h, w)
LF = (1, 5, 6, 9)             # (B, A, h, w)
M_ROWS = 3000


def op(name):
    def deco(f):
        assert name not in OPS, name
        OPS[name] = f
        return f
    return deco


def rn(*shape, seed, scale=1.0):
    import torch
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()


def ru(*shape, seed):
    import torch
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _capi():
    from lfsr_amd import capi
    return capi


def _banded(*a, **k):
    from tests.stream_helpers import Banded
    return Banded(*a, **k)


def _simple(fn, *tensors):
    """an operator whose wrapper allocates its own output: every tensor argument is an input"""
    return (lambda *t: fn(*t)), list(tensors), []


# ---- index operators ---------------------------------------------------------------------------------------------------------------------------------------------
@op("lfsr_sai2macpi")
def _():
    return _simple(lambda x: _capi().sai2macpi(x, 5), rn(2, 3, 5 * 6, 5 * 9, seed=1))


@op("lfsr_macpi2sai")
def _():
    return _simple(lambda x: _capi().macpi2sai(x, 5), rn(2, 3, 5 * 6, 5 * 9, seed=2))


@op("lfsr_pixel_shuffle2d")
def _():
    return _simple(lambda x: _capi().pixel_shuffle2d(x, 2), rn(2, 3 * 4, 7, 13, seed=3))


@op("lfsr_pixel_shuffle1d")
def _():
    return _simple(lambda x: _capi().pixel_shuffle1d(x, 5), rn(2, 3 * 5, 7, 13, seed=4))


@op("lfsr_image_extend")
def _():
    return _simple(lambda x: _capi().image_extend(x, [2, 3, 1, 4]), rn(3, 7, 13, seed=5))


@op("lfsr_lf_divide")
def _():
    return _simple(lambda x: _capi().lf_divide(x, 5, 32, 16), rn(5 * 40, 5 * 33, seed=6))


_TILES = (3, 2, 3, 8, 4, 7, 11)       # (A, numU, numV, pz, stride, h, w): a ragged crop in both directions


@op("lfsr_lf_integrate")
def _():
    A, nu, nv, pz, st, h, w = _TILES
    return _simple(lambda s: _capi().lf_integrate(s, A, pz, st, h, w), rn(nu, nv, A * pz, A * pz, seed=7))


@op("lfsr_lf_crop_tiles")
def _():
    A, nu, nv, pz, st, h, w = _TILES
    return _simple(lambda s: _capi().lf_crop_tiles(s, A, pz, st), rn(nu * nv, A * pz, A * pz, seed=8))


@op("lfsr_lf_place_tiles")
def _():
    import torch
    A, nu, nv, pz, st, h, w = _TILES
    out = _banded((A, A, h, w), init=torch.zeros(A, A, h, w))
    return (lambda t: _capi().lf_place_tiles(t, out.t, A, nu, nv, 0, st)), [rn(nu * nv, A, A, st, st, seed=9)], [out]


@op("lfsr_nchw_to_vcl")
def _():
    B, A, h, w = LF
    out = _banded((B * A * A * h * w, 80), init=None)

    def call(x):
        return _capi().nchw_to_vcl(x, A, 1, out=out.t, choff=8)[:, 8:72]
    return call, [rn(B, 64, A * h, A * w, seed=10)], [out]


@op("lfsr_vcl_to_nchw")
def _():
    B, A, h, w = LF
    return _simple(lambda v: _capi().vcl_to_nchw(v, B, 64, A, h, w, 1, choff=8), rn(B * A * A * h * w, 80, seed=11))


@op("lfsr_pack_conv_weight")
def _():
    return _simple(lambda w: _capi().pack_conv_weight(w), rn(64, 64, 3, 3, seed=12, scale=0.05))


@op("lfsr_pack_conv_weight_tr")
def _():
    return _simple(lambda w: _capi().pack_conv_weight_T(w), rn(64, 64, 3, 3, seed=13, scale=0.05))


# ---- DistgSSR's forward operators ---------------------------------------------------------------------------------------------------------------------------------
def _w33(seed):
    return rn(64, 64, 3, 3, seed=seed, scale=0.05)


@op("lfsr_conv3x3_fwd")
def _():
    n, h, w = RAG
    wp = _capi().pack_conv_weight(_w33(20))
    return _simple(lambda x, wp_, r: _capi().conv3x3(x, wp_, n, h, w, slope=0.1, res1=r), rn(n * h * w, 64, seed=21), wp, rn(n * h * w, 64, seed=22))


@op("lfsr_pointwise_fwd")
def _():
    wp = _capi().pack_conv_weight(rn(64, 144, 1, 1, seed=23, scale=0.1))
    return _simple(lambda x, wp_, b: _capi().pointwise(x, 144, wp_, 64, slope=0.1, bias=b), rn(M_ROWS, 144, seed=24), wp, rn(64, seed=25))


def _branch_weights(A, seed):
    capi = _capi()
    return (capi.pack_conv_weight(rn(16, 64, A, A, seed=seed, scale=0.03)), capi.pack_conv_weight(rn(A * A * 16, 16, 1, 1, seed=seed + 1, scale=0.2), perm=1, ch=16),
            capi.pack_conv_weight(rn(32, 64, 1, A * A, seed=seed + 2, scale=0.03)), capi.pack_conv_weight(rn(A * 32, 32, 1, 1, seed=seed + 3, scale=0.15)))


@op("lfsr_angconv_fwd")
def _():
    import torch
    B, A, h, w = LF
    npix = B * A * A * h * w
    w1, w2, _, _ = _branch_weights(A, 30)
    out, tmp = _banded((npix, 144), init=torch.zeros(npix, 144)), _banded((B * h * w, 16))

    def call(x, a, b):
        _capi().angconv(x, a, b, B, A, h, w, 0.1, out.t, 64, tmp=tmp.t)
        return out.t, tmp.t
    return call, [rn(npix, 64, seed=34), w1, w2], [out, tmp]


@op("lfsr_epiconv_fwd")
def _():
    import torch
    B, A, h, w = LF
    npix = B * A * A * h * w
    _, _, w1, w2 = _branch_weights(A, 35)
    out, tmp = _banded((npix, 144), init=torch.zeros(npix, 144)), _banded((B * A * h * w, 32))

    def call(x, a, b):
        _capi().epiconv(x, a, b, B, A, h, w, True, 0.1, out.t, 112, tmp=tmp.t)
        return out.t, tmp.t
    return call, [rn(npix, 64, seed=39), w1, w2], [out, tmp]


@op("lfsr_epiconv_hv_fwd")
def _():
    import torch
    B, A, h, w = LF
    npix = B * A * A * h * w
    _, _, w1, w2 = _branch_weights(A, 40)
    out = _banded((npix, 144), init=torch.zeros(npix, 144))
    return (lambda x, a, b: _capi().epiconv_hv(x, a, b, B, A, h, w, 0.1, out.t, 80, 112)), [rn(npix, 64, seed=44), w1, w2], [out]


@op("lfsr_distg_branch_tail_fwd")
def _():
    B, A, h, w = 1, 5, 13, 11           # tests/test_gpu_distg_fuse.py's ragged case
    npix = B * A * A * h * w
    wa0, wa2, we0, we2 = _branch_weights(A, 45)
    wf = _capi().pack_conv_weight(rn(64, 144, 1, 1, seed=49, scale=0.08))
    outs = [_banded(s) for s in ((npix, 64), (B * h * w, 16), (B * A * h * w, 32), (B * A * h * w, 32))]

    def call(x, spa, *wts):
        return _capi().distg_branch_tail(x, spa, *wts, B, A, h, w, 0.1, out=tuple(o.t for o in outs))
    return call, [rn(npix, 64, seed=50), rn(npix, 64, seed=51), wa0, wa2, we0, we2, wf], outs


@op("lfsr_initconv_fwd")
def _():
    B, A, h, w = LF
    return _simple(lambda x, wt: _capi().initconv(x, wt, A), ru(B, 1, A * h, A * w, seed=52), rn(64, 1, 3, 3, seed=53, scale=0.3))


def _head(s, seed):
    return rn(64 * s * s, 64, 1, 1, seed=seed, scale=0.1), rn(64 * s * s, seed=seed + 1, scale=0.1), rn(1, 64, 1, 1, seed=seed + 2, scale=0.1)


def _fold(w0, b0, w2, s):
    import torch
    capi = _capi()
    wf, bf = torch.empty(s * s * 64, device="cuda"), torch.empty(s * s, device="cuda")
    capi.check(capi.load().lfsr_fold_head(capi.dev_ptr(w0), capi.dev_ptr(b0), capi.dev_ptr(w2), capi.dev_ptr(wf), capi.dev_ptr(bf), 64, s, capi.stream_ptr()), "fold_head")
    return wf, bf


@op("lfsr_fold_head")
def _():
    s = 3
    wf, bf = _banded((s * s * 64,)), _banded((s * s,))

    def call(w0, b0, w2):
        capi = _capi()
        capi.check(capi.load().lfsr_fold_head(capi.dev_ptr(w0), capi.dev_ptr(b0), capi.dev_ptr(w2), capi.dev_ptr(wf.t), capi.dev_ptr(bf.t), 64, s, capi.stream_ptr()),
                   "fold_head")
        return wf.t, bf.t
    return call, list(_head(s, 54)), [wf, bf]


@op("lfsr_upsample_head_fwd")
def _():
    B, A, h, w = LF
    s = 3
    w0, b0, w2 = _head(s, 57)
    # (the wrapper folds the head first: lfsr_fold_head and lfsr_upsample_head_fwd back to back on the caller's stream)
    return _simple(lambda f, a, b, c, x: _capi().upsample_head(f, a, b, c, x, A, s), rn(B * A * A * h * w, 64, seed=60), w0, b0, w2, ru(B, 1, A * h, A * w, seed=61))


# ---- DistgSSR's backward operators --------------------------------------------------------------------------------------------------------------------------------
@op("lfsr_conv3x3_dgrad")
def _():
    n, h, w = RAG
    wT = _capi().pack_conv_weight_T(_w33(62))
    return _simple(lambda dy, wT_, r, a: _capi().conv3x3_dgrad(dy, wT_, n, h, w, res1=r, act=a, act_slope=0.1),
                   rn(n * h * w, 64, seed=63), wT, rn(n * h * w, 64, seed=64), rn(n * h * w, 64, seed=65))


@op("lfsr_conv3x3_wgrad")
def _():
    import torch
    capi = _capi()
    n, h, w = RAG
    dw = _banded((64, 64, 3, 3), init=torch.randn(64, 64, 3, 3, generator=torch.Generator().manual_seed(66)))      # accumulated into
    ws = _banded((capi.load().lfsr_conv3x3_wgrad_workspace_floats(n, h, w),))

    def call(dy, x):
        capi.check(capi.load().lfsr_conv3x3_wgrad(capi.dev_ptr(dy), 64, 0, capi.dev_ptr(x), 64, 0, capi.dev_ptr(dw.t), capi.dev_ptr(ws.t), ws.t.numel(), n, h, w, 1,
                                                  capi.stream_ptr()), "conv3x3_wgrad")
        return dw.t
    return call, [rn(n * h * w, 64, seed=67), rn(n * h * w, 64, seed=68)], [dw, ws]


@op("lfsr_pointwise_dgrad")
def _():
    wT = _capi().pack_conv_weight_T(rn(64, 144, 1, 1, seed=69, scale=0.1))
    return _simple(lambda dy, wT_, a: _capi().pointwise_dgrad(dy, wT_, 144, act=a, act_slope=0.1), rn(M_ROWS, 64, seed=70), wT, rn(M_ROWS, 144, seed=71))


@op("lfsr_pointwise_wgrad")
def _():
    capi = _capi()
    dw = _banded((64, 144))
    ws = _banded((capi.load().lfsr_pointwise_wgrad_workspace_floats(M_ROWS, 64, 144),))

    def call(dy, x):
        capi.check(capi.load().lfsr_pointwise_wgrad(capi.dev_ptr(dy), 64, 0, 64, capi.dev_ptr(x), 144, 0, 144, capi.dev_ptr(dw.t), capi.dev_ptr(ws.t), ws.t.numel(), M_ROWS, 0,
                                                    capi.stream_ptr()), "pointwise_wgrad")
        return dw.t
    return call, [rn(M_ROWS, 64, seed=72), rn(M_ROWS, 144, seed=73)], [dw, ws]


@op("lfsr_upsample_head_dgrad")
def _():
    B, A, h, w = LF
    s = 3
    npix = B * A * A * h * w
    wf, _ = _fold(*_head(s, 74), s)
    df, g16 = _banded((npix, 64)), _banded((npix, 16))

    def call(dout, wf_):
        capi = _capi()
        capi.check(capi.load().lfsr_upsample_head_dgrad(capi.dev_ptr(dout), capi.dev_ptr(wf_), capi.dev_ptr(df.t), capi.dev_ptr(g16.t), B, A, h, w, s, capi.stream_ptr()),
                   "upsample_head_dgrad")
        return df.t, g16.t
    return call, [rn(B, 1, A * h * s, A * w * s, seed=77), wf], [df, g16]


def _branch_bwd(name, seed):
    """the forward of one branch on the default stream (its saved activations are inputs of the backward), then the backward as the call"""
    import torch
    capi = _capi()
    B, A, h, w = 2, 5, 3, 7
    npix = B * A * A * h * w
    x = rn(npix, 64, seed=seed)
    dx0 = torch.randn(npix, 64, generator=torch.Generator().manual_seed(seed + 1))
    dx = _banded((npix, 64), init=dx0)                                  # accumulated into
    if name == "ang":
        w0, w2 = rn(16, 64, A, A, seed=seed + 2, scale=0.03), rn(A * A * 16, 16, 1, 1, seed=seed + 3, scale=0.2)
        y, a16 = torch.zeros(npix, 16, device="cuda"), torch.empty(B * h * w, 16, device="cuda")
        capi.angconv(x, capi.pack_conv_weight(w0), capi.pack_conv_weight(w2, perm=1, ch=16), B, A, h, w, 0.1, y, 0, tmp=a16)
        ws = _banded((capi.load().lfsr_angconv_bwd_workspace_floats(B, A, h, w),))
        dw0, dw2 = _banded(tuple(w0.shape)), _banded(tuple(w2.shape))
        P = capi.dev_ptr

        def call(dy, y_, x_, a_, w0_, w2_):
            capi.check(capi.load().lfsr_angconv_bwd(P(dy), 16, 0, P(y_), 16, 0, P(x_), P(a_), P(w0_), P(w2_), P(dx.t), P(dw0.t), P(dw2.t), P(ws.t), ws.t.numel(),
                                                    B, A, h, w, 0.1, capi.stream_ptr()), "angconv_bwd")
            return dx.t, dw0.t, dw2.t
        return call, [rn(npix, 16, seed=seed + 4), y, x, a16, w0, w2], [dx, dw0, dw2, ws]
    w0, w2 = rn(32, 64, 1, A * A, seed=seed + 2, scale=0.03), rn(A * 32, 32, 1, 1, seed=seed + 3, scale=0.15)
    w0p, w2p = capi.pack_conv_weight(w0), capi.pack_conv_weight(w2)
    y = torch.zeros(npix, 64, device="cuda")
    eh, ev = torch.empty(B * A * h * w, 32, device="cuda"), torch.empty(B * A * h * w, 32, device="cuda")
    capi.epiconv(x, w0p, w2p, B, A, h, w, False, 0.1, y, 0, tmp=eh)
    capi.epiconv(x, w0p, w2p, B, A, h, w, True, 0.1, y, 32, tmp=ev)
    ws = _banded((capi.load().lfsr_epiconv_hv_bwd_workspace_floats(B, A, h, w),))
    dw0, dw2 = _banded(tuple(w0.shape)), _banded(tuple(w2.shape))
    P = capi.dev_ptr

    def call(dy, y_, x_, eh_, ev_, w0_, w2_):
        capi.check(capi.load().lfsr_epiconv_hv_bwd(P(dy), 80, 8, 48, P(y_), 64, 0, 32, P(x_), P(eh_), P(ev_), P(w0_), P(w2_), P(dx.t), P(dw0.t), P(dw2.t), P(ws.t), ws.t.numel(),
                                                   B, A, h, w, 0.1, capi.stream_ptr()), "epiconv_hv_bwd")
        return dx.t, dw0.t, dw2.t
    return call, [rn(npix, 80, seed=seed + 4), y, x, eh, ev, w0, w2], [dx, dw0, dw2, ws]


@op("lfsr_angconv_bwd")
def _():
    return _branch_bwd("ang", 80)


@op("lfsr_epiconv_hv_bwd")
def _():
    return _branch_bwd("epi", 90)


# ---- the transformers' operators ----------------------------------------------------------------------------------------------------------------------------------
def _lin_w(N, K, seed):
    return _capi().pack_conv_weight(rn(N, K, 1, 1, seed=seed, scale=0.1))


def _ln(C_, seed):
    return 1 + 0.3 * rn(C_, seed=seed), rn(C_, seed=seed + 1, scale=0.2)


@op("lfsr_layernorm_fwd")
def _():
    M, C_ = 999, 128
    A, h, w = 5, 7, 13
    g, b = _ln(C_, 100)
    y = _banded((M, C_ + 128))

    def call(x, pe, g_, b_):      # the strided slices of tests/test_gpu_transformer_ops.py, LFT's spatial position term
        capi = _capi()
        P = capi.dev_ptr
        capi.check(capi.load().lfsr_layernorm_fwd(P(x), C_ + 64, 32, P(pe), C_ + 16, h * w, 1, P(g_), P(b_), P(y.t), C_ + 128, 64, M, C_, 1e-5, capi.stream_ptr()),
                   "layernorm")
        return y.t[:, 64:64 + C_]
    return call, [rn(M, C_ + 64, seed=102), rn(h * w, C_ + 16, seed=103), g, b], [y]


@op("lfsr_linear_fwd")
def _():
    K, N = 128, 128
    y = _banded((M_ROWS, N))

    def call(x, wp, r):
        capi = _capi()
        P = capi.dev_ptr
        capi.check(capi.load().lfsr_linear_fwd(P(x), K, 0, K, P(wp), None, P(r), N, 0, P(y.t), N, 0, M_ROWS, N, 1.0, capi.stream_ptr()), "linear")
        return y.t
    return call, [rn(M_ROWS, K, seed=104), _lin_w(N, K, 105), rn(M_ROWS, N, seed=106)], [y]


def _ffn(with_ln, seed):
    K1, H = 128, 256
    g, b = _ln(K1, seed)
    y = _banded((M_ROWS, K1))

    def call(x, w1, w2, g_, b_):
        capi = _capi()
        P = capi.dev_ptr
        lib = capi.load()
        if with_ln:
            rc = lib.lfsr_ffn_ln_fwd(P(x), K1, 0, P(g_), P(b_), 1e-5, P(w1), P(w2), P(x), K1, 0, P(y.t), K1, 0, M_ROWS, K1, H, K1, 0.0, capi.stream_ptr())
        else:
            rc = lib.lfsr_ffn_fwd(P(x), K1, 0, P(w1), P(w2), P(x), K1, 0, P(y.t), K1, 0, M_ROWS, K1, H, K1, 0.0, capi.stream_ptr())
        capi.check(rc, "ffn")
        return y.t
    return call, [rn(M_ROWS, K1, seed=seed + 2), _lin_w(H, K1, seed + 3), _lin_w(K1, H, seed + 4), g, b], [y]


@op("lfsr_ffn_fwd")
def _():
    return _ffn(False, 110)


@op("lfsr_ffn_ln_fwd")
def _():
    return _ffn(True, 115)


@op("lfsr_linear_ln_fwd")
def _():
    K, N, split = 128, 384, 256
    g, b = _ln(K, 120)
    qk, v = _banded((M_ROWS, split)), _banded((M_ROWS, N - split))

    def call(x, wp, g_, b_, pe):
        capi = _capi()
        P = capi.dev_ptr
        capi.check(capi.load().lfsr_linear_ln_fwd(P(x), K, 0, K, P(wp), P(g_), P(b_), 1e-5, split, P(pe), K, 7, 3, P(qk.t), split, 0, P(v.t), N - split, 0, split,
                                                  M_ROWS, N, capi.stream_ptr()), "linear_ln")
        return qk.t, v.t
    return call, [rn(M_ROWS, K, seed=122), _lin_w(N, K, 123), g, b, rn(7, K, seed=124)], [qk, v]


_SPA = (3, 6, 8)              # (n, h, w) of the 5x5 spatial window attention (tests/helpers.py:LFT_SPA_GEOMS): every query sees a key
_E, _NH = 128, 8


def _spa_geometry(n, h, w):
    return (n, 1, 1, h * w, 0, 0, h, w, w, 1, 2, 3, 2, 3, h)


@op("lfsr_window_attn_fwd")
def _():
    n, h, w = _SPA
    o = _banded((n * h * w, 256))

    def call(qk, v):
        capi = _capi()
        P = capi.dev_ptr
        capi.check(capi.load().lfsr_window_attn_fwd(P(qk), 256, 0, P(qk), 256, 128, P(v), 128, 0, P(o.t), 256, 64, _NH, _E // _NH, *_spa_geometry(n, h, w),
                                                    capi.stream_ptr()), "window_attn")
        return o.t[:, 64:64 + _E]
    return call, [rn(n * h * w, 256, seed=125), rn(n * h * w, 128, seed=126)], [o]


@op("lfsr_window_attn_bwd")
def _():
    import torch
    capi = _capi()
    P = capi.dev_ptr
    n, h, w = _SPA
    npix = n * h * w
    qk, v = rn(npix, 256, seed=127), rn(npix, 128, seed=128)
    o = torch.empty(npix, 128, device="cuda")
    capi.check(capi.load().lfsr_window_attn_fwd(P(qk), 256, 0, P(qk), 256, 128, P(v), 128, 0, P(o), 128, 0, _NH, _E // _NH, *_spa_geometry(n, h, w), capi.stream_ptr()), "attn")
    dqk, dv, stats = _banded((npix, 256)), _banded((npix, 128)), _banded((npix * _NH * 4,))

    def call(qk_, v_, o_, d_o):
        capi.check(capi.load().lfsr_window_attn_bwd(P(qk_), 256, 0, 128, P(v_), 128, 0, P(o_), P(d_o), 128, 0, P(dqk.t), P(dv.t), P(stats.t), _NH, _E // _NH,
                                                    *_spa_geometry(n, h, w), capi.stream_ptr()), "window_attn_bwd")
        return dqk.t, dv.t
    return call, [qk, v, o, rn(npix, 128, seed=129)], [dqk, dv, stats]


@op("lfsr_layernorm_bwd")
def _():
    capi = _capi()
    P = capi.dev_ptr
    M, C_ = M_ROWS, 64
    n_ws = capi.load().lfsr_layernorm_bwd_workspace_floats(C_)
    dx, dg, db, ws = _banded((M, C_)), _banded((C_,)), _banded((C_,)), _banded((n_ws,))

    def call(x, pe, g, dy, r):
        capi.check(capi.load().lfsr_layernorm_bwd(P(x), P(pe), 25, 120, P(g), P(dy), P(r), P(dx.t), P(dg.t), P(db.t), P(ws.t), n_ws, M, C_, capi.stream_ptr()), "layernorm_bwd")
        return dx.t, dg.t, db.t
    return call, [rn(M, C_, seed=130), rn(25, C_, seed=131), _ln(C_, 132)[0], rn(M, C_, seed=134), rn(M, C_, seed=135)], [dx, dg, db, ws]


@op("lfsr_linear_dgrad")
def _():
    cout, cin = 256, 128
    wT = _capi().pack_conv_weight_T(rn(cout, cin, 1, 1, seed=136, scale=0.1))
    dx = _banded((M_ROWS, cin))
    return ((lambda dy, wT_, r, a: _capi().linear_dgrad(dy, wT_, cin, r1=r, act=a, dx=dx.t)),
            [rn(M_ROWS, cout, seed=137), wT, rn(M_ROWS, cin, seed=138), rn(M_ROWS, cin, seed=139)], [dx])


@op("lfsr_linear_wgrad")
def _():
    import torch
    capi = _capi()
    P = capi.dev_ptr
    cout, cin = 256, 128
    dw = _banded((cout, cin), init=torch.randn(cout, cin, generator=torch.Generator().manual_seed(140)))       # accumulated into
    ws = _banded((capi.load().lfsr_linear_wgrad_workspace_floats(M_ROWS, cout, cin),))

    def call(dy, x):
        capi.check(capi.load().lfsr_linear_wgrad(P(dy), cout, P(x), cin, P(dw.t), P(ws.t), ws.t.numel(), M_ROWS, cout, cin, 1, capi.stream_ptr()), "linear_wgrad")
        return dw.t
    return call, [rn(M_ROWS, cout, seed=141), rn(M_ROWS, cin, seed=142)], [dw, ws]


_TAIL = (2, 3, 5, 7)          # (B, A, h, w)


def _tail_weights(s, seed):
    return _capi().pack_conv_weight(rn(64 * s * s, 64, 1, 1, seed=seed, scale=0.125), perm=1, ch=64), rn(1, 64, 3, 3, seed=seed + 1, scale=0.05)


@op("lfsr_up_tail_bwd")
def _():
    capi = _capi()
    P = capi.dev_ptr
    B, A, h, w = _TAIL
    s = 3
    npix = B * A * A * h * w
    n_ws = capi.load().lfsr_up_tail_bwd_workspace_floats()
    du, dw3, ws = _banded((npix, 64 * s * s)), _banded((1, 64, 3, 3)), _banded((n_ws,))

    def call(dout, w3, hr):
        capi.check(capi.load().lfsr_up_tail_bwd(P(dout), P(w3), P(hr), P(du.t), P(dw3.t), P(ws.t), n_ws, B, A, h, w, s, 0.2, capi.stream_ptr()), "up_tail_bwd")
        return du.t, dw3.t
    return call, [rn(B, 1, A * h * s, A * w * s, seed=143), _tail_weights(s, 144)[1], rn(B, A * h * s, A * w * s, 64, seed=146)], [du, dw3, ws]


@op("lfsr_pack_up0_weight_tr")
def _():
    s = 3
    out = _banded((64, 64 * s * s))

    def call(wp):
        capi = _capi()
        capi.check(capi.load().lfsr_pack_up0_weight_tr(capi.dev_ptr(wp), capi.dev_ptr(out.t), s, capi.stream_ptr()), "pack_up0_weight_tr")
        return out.t
    return call, [_tail_weights(s, 147)[0]], [out]


@op("lfsr_conv3x3_n_fwd")
def _():
    n, h, w = RAG
    N = 96
    y = _banded((n * h * w, 256))

    def call(x, wp):
        capi = _capi()
        P = capi.dev_ptr
        capi.check(capi.load().lfsr_conv3x3_n_fwd(P(x), 128, 64, P(wp), P(y.t), 256, 128, n, h, w, N, 0.2, capi.stream_ptr()), "conv3x3_n")
        return y.t[:, 128:128 + N]
    return call, [rn(n * h * w, 128, seed=149), _capi().pack_conv_weight(rn(N, 64, 3, 3, seed=150, scale=0.05))], [y]


@op("lfsr_lft_position_fwd")
def _():
    A, h, w, C_ = 5, 6, 8, 64
    spa, ang = _banded((h * w, C_)), _banded((A * A, C_))

    def call():
        capi = _capi()
        capi.check(capi.load().lfsr_lft_position_fwd(capi.dev_ptr(spa.t), capi.dev_ptr(ang.t), A, h, w, C_, capi.stream_ptr()), "position")
        return spa.t, ang.t
    return call, [], [spa, ang]           # no inputs: what the case shows is that the two tables are written on the caller's stream, behind the delay


def _tail_fwd(which):
    B, A, h, w = _TAIL
    s = 2
    w0p, w3 = _tail_weights(s, 151)
    Hs, Ws = A * h * s, A * w * s
    capi = _capi()
    P = capi.dev_ptr
    if which == "ps":
        hr = _banded((B, Hs, Ws, 64))

        def call(f, w0):
            capi.check(capi.load().lfsr_upsample_ps_fwd(P(f), 128, 64, P(w0), P(hr.t), B, A, h, w, s, capi.stream_ptr()), "upsample_ps")
            return hr.t
        return call, [rn(B * A * A * h * w, 128, seed=153), w0p], [hr]
    out = _banded((B, 1, Hs, Ws))
    x = ru(B, 1, A * h, A * w, seed=154)
    if which == "fused":
        def call(f, w0, w3_, x_):
            capi.check(capi.load().lfsr_up_tail_fwd(P(f), 128, 64, P(w0), P(w3_), P(x_), P(out.t), B, A, h, w, s, 0.2, capi.stream_ptr()), "up_tail")
            return out.t
        return call, [rn(B * A * A * h * w, 128, seed=155), w0p, w3, x], [out]

    def call(hr, w3_, x_):
        capi.check(capi.load().lfsr_hr_tail_fwd(P(hr), P(w3_), P(x_), P(out.t), B, A, h, w, s, 0.2, capi.stream_ptr()), "hr_tail")
        return out.t
    return call, [rn(B, Hs, Ws, 64, seed=156), w3, x], [out]


@op("lfsr_upsample_ps_fwd")
def _():
    return _tail_fwd("ps")


@op("lfsr_up_tail_fwd")
def _():
    return _tail_fwd("fused")


@op("lfsr_hr_tail_fwd")
def _():
    return _tail_fwd("hr")


# ---- the steps either side of the hot path ------------------------------------------------------------------------------------------------------------------------
@op("lfsr_view_metrics")
def _():
    from lfsr_amd.utils.metrics import view_metrics
    B, A, H, W = 2, 3, 12, 13
    label = ru(B, 1, A * H, A * W, seed=160)
    return _simple(lambda a, b: view_metrics(a, b, A), label, (label + 0.05 * rn(B, 1, A * H, A * W, seed=161)).clamp(0, 1))


def _mask(fill_per_view):
    import torch
    B, C_, A, h, w = 2, 3, 5, 6, 9
    flags = (torch.arange(A * A) % 3 == 1).to(torch.uint8).cuda()
    y = _banded((B, C_, A * h, A * w))

    def call(x, m, fill):
        capi = _capi()
        P = capi.dev_ptr
        if fill_per_view:
            rc = capi.load().lfsr_mask_views_fill(P(x), P(y.t), P(m), P(fill), B, C_, A, h, w, capi.stream_ptr())
        else:
            rc = capi.load().lfsr_mask_views(P(x), P(y.t), P(m), 0.25, B, C_, A, h, w, capi.stream_ptr())
        capi.check(rc, "mask_views")
        return y.t
    return call, [rn(B, C_, A * h, A * w, seed=162), flags, rn(A * A, seed=163)], [y]


@op("lfsr_mask_views")
def _():
    return _mask(False)


@op("lfsr_mask_views_fill")
def _():
    return _mask(True)


@op("lfsr_ycbcr2rgb_views")
def _():
    from lfsr_amd.utils.utils import ycbcr2rgb_views
    A, h, w = 3, 7, 13
    return _simple(lambda y, cc: ycbcr2rgb_views(y, cc, A), ru(A * h, A * w, seed=164), ru(2, A * h, A * w, seed=165))


# ---- LF_InterNet's wide convs, LFSSR's operators ------------------------------------------------------------------------------------------------------------------
@op("lfsr_conv3x3_wide_fwd")
def _():
    n, h, w = 2, 9, 33            # w = 33: one past the 32-pixel tile of the wide convs
    cin = 128
    wp = _capi().pack_conv_weight(rn(64, cin, 3, 3, seed=170, scale=0.03))
    return _simple(lambda x, wp_: _capi().conv3x3_wide(x, cin, wp_, n, h, w, res1=x), rn(n * h * w, cin, seed=171), wp)


@op("lfsr_conv3x3_wide_wgrad")
def _():
    import torch
    capi = _capi()
    P = capi.dev_ptr
    n, h, w = 2, 9, 33
    cin = 128
    dw = _banded((64, cin, 3, 3), init=torch.randn(64, cin, 3, 3, generator=torch.Generator().manual_seed(172)))      # accumulated into
    ws = _banded((capi.load().lfsr_conv3x3_wide_wgrad_workspace_floats(cin, n, h, w),))

    def call(dy, x):
        capi.check(capi.load().lfsr_conv3x3_wide_wgrad(P(dy), 64, 0, P(x), cin, 0, cin, P(dw.t), P(ws.t), ws.t.numel(), n, h, w, 1, capi.stream_ptr()), "wide_wgrad")
        return dw.t
    return call, [rn(n * h * w, 64, seed=173), rn(n * h * w, cin, seed=174)], [dw, ws]


@op("lfsr_angconv3x3_fwd")
def _():
    B, A, h, w = 2, 3, 3, 5
    wp = _capi().pack_conv_weight(_w33(175))
    return _simple(lambda x, wp_, b, ib: _capi().angconv3x3(x, wp_, b, B, A, h * w, in_bias=ib), rn(B * A * A * h * w, 64, seed=176), wp, rn(64, seed=177, scale=0.1),
                   ru(64, seed=178))


@op("lfsr_lfssr_conv0_fwd")
def _():
    B, A, h, w = 2, 3, 5, 7
    return _simple(lambda x, wt, b: _capi().lfssr_conv0(x, wt, b, A), ru(B, 1, A * h, A * w, seed=179), rn(64, 1, 3, 3, seed=180, scale=0.3), rn(64, seed=181, scale=0.1))


@op("lfsr_conv3x3_ps2_fwd")
def _():
    n, h, w = 18, 5, 7
    capi = _capi()
    P = capi.dev_ptr
    wp = capi.pack_ps2_weight(rn(256, 64, 3, 3, seed=182, scale=0.05))
    out, tmp = _banded((n * h * w * 4, 64)), _banded((n * h * w, 256))

    def call(x, wp_, b):
        capi.check(capi.load().lfsr_conv3x3_ps2_fwd(P(x), 64, 0, P(wp_), P(b), P(tmp.t), P(out.t), 64, 0, n, h, w, capi.stream_ptr()), "conv3x3_ps2")
        return out.t
    return call, [rn(n * h * w, 64, seed=183), wp, rn(256, seed=184, scale=0.1)], [out, tmp]


@op("lfsr_lfssr_tail_fwd")
def _():
    B, A, h, w = 2, 3, 5, 7
    return _simple(lambda f, wr, br, lo, wi, bi: _capi().lfssr_tail(f, wr, br, lo, wi, bi, B, A, h, w, True),
                   rn(B * A * A * 4 * h * w, 64, seed=185), rn(1, 64, 3, 3, seed=186, scale=0.05), rn(1, seed=187), ru(B * A * A, h, w, seed=188),
                   rn(4, 1, 3, 3, seed=189, scale=0.3), rn(4, seed=190, scale=0.1))
