"""GPU: the backward operators csrc/trans_bwd.hip shares between the LFT and EPIT training drivers, each through its C-ABI entry point against fp64 autograd of the
same operation on stock torch CPU ops: lfsr_layernorm_bwd (k_ln_bwd<64|128> + k_colsum), lfsr_linear_dgrad (LfsrTransBwd::dgemm: the gather-GEMM with the ReLU' mask
and the residual), lfsr_up_tail_bwd + lfsr_pack_up0_weight_tr (k_tail_bwd, k_pack_up0_T) and lfsr_window_attn_bwd at LFT's two geometries.

Gates.  Every value: max|err| <= 1e-4 * max(1, max|ref|), and mean|err| <= YARDSTICK (8) x the mean error of the same operator in fp32 on the CPU (tests.helpers.op_gate).
Attention: rel-L2 <= 1e-5 per dQ, dK, dV, the gate of tests/test_gpu_epit_attn_bwd.py.  Inputs carry NaN guard rows in front of and behind [0, M); outputs lie in
sentinel-filled buffers (strided ones inside wider rows) with tail rows behind, and every float outside the operand must keep its bits; every operator runs twice and
must give the same bits (no float atomics).  The references themselves are checked without a GPU in tests/test_trans_bwd_refs_cpu.py.

The spatial attention cases keep to geometries where every query sees at least one key (w <= h + 2): the forward of a query with an empty window is NaN, as the
reference's softmax over an all -inf mask row, and its gradient is unspecified.  profiles/trans_bwd_op_tests.md has the measured figures."""
import functools

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from tests.helpers import (LFT_NH, LFT_SPA_GEOMS, OP_SENTINEL, attn_bwd_layout, attn_bwd_run, attn_bwd_untouched, lft_ang_attn_ref, lft_spa_attn_ref, ln_bwd_ref,
                           op_gate, op_input, op_output, op_output_read, rel_l2, tail_bwd_ref)

pytestmark = pytest.mark.gpu
E_ARG, E_WS = -1, -2
BAND = 4096                     # sentinel floats behind a workspace
RED_BLOCKS = 1024               # LFSR_RED_BLOCKS: the grid cap of k_ln_bwd and k_tail_bwd
P = capi.dev_ptr


def rnd(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def workspace(n):
    return torch.full((n + BAND,), OP_SENTINEL, device="cuda")


def intact(t):
    torch.cuda.synchronize()
    return bool((t == OP_SENTINEL).all())


def untouched(buf):
    """an OpBuffer output that no launch may have written"""
    torch.cuda.synchronize()
    return bool((buf.t.view(torch.int32) == buf.pristine.view(torch.int32)).all())


# ---------------------------------------------------------------------------------------------------------------------
# lfsr_layernorm_bwd
# ---------------------------------------------------------------------------------------------------------------------
LN_A, LN_H, LN_W = 5, 7, 13      # the position forms of tests/test_gpu_transformer_ops.py::test_layernorm_position_term_and_slices


def ln_rows(C):
    """M: fewer rows than one block holds (RPB = 16 | 8 rows), exactly the grid cap, the first grid-stride row, ragged everywhere"""
    rpb = 256 // (C // 4)
    return (5, rpb * RED_BLOCKS, rpb * RED_BLOCKS + 1, 70001)


def pe_form(form):
    return {"none": (0, 1), "ang": (LN_A * LN_A, LN_H * LN_W), "spa": (LN_H * LN_W, 1)}[form]      # (pe_rows, pe_div)


@functools.lru_cache(maxsize=2)
def ln_case(C, M, form):
    x = rnd((M, C), 61, 2.0) * (0.5 + torch.rand((M, 1), generator=torch.Generator().manual_seed(66))) + rnd((M, 1), 62)      # a per-row offset and scale
    gamma = 1 + 0.3 * rnd((C,), 63)
    dy, r = rnd((M, C), 64), rnd((M, C), 67)
    pe_rows, pe_div = pe_form(form)
    pe = rnd((max(pe_rows, 1), C), 65)
    per = pe[(torch.arange(M) // pe_div) % pe_rows] if pe_rows else None
    return dict(x=x, gamma=gamma, dy=dy, r=r, pe=pe, ref=ln_bwd_ref(x, per, gamma, dy, torch.float64), cpu=ln_bwd_ref(x, per, gamma, dy, torch.float32))


def ln_call(lib, c, C, M, form, r_mode, ws, ws_floats, seed):
    """one launch on fresh buffers -> (rc, dx, dgamma, dbeta) (OpBuffers)"""
    pe_rows, pe_div = pe_form(form)
    x, dy, g = op_input(c["x"], C, 0, 1), op_input(c["dy"], C, 0, 2), op_input(c["gamma"].reshape(1, C), C, 0, 3)
    pe = op_input(c["pe"], C, 0, 4) if pe_rows else None
    dx, dg, db = op_output(M, C, seed), op_output(1, C, seed + 1), op_output(1, C, seed + 2)
    r = None
    if r_mode == "distinct":
        r = op_input(c["r"], C, 0, 5).ptr
    elif r_mode == "dx":
        dx.t[:M] = c["r"].cuda()
        dx.pristine[:M] = dx.t[:M]
        r = dx.ptr
    rc = lib.lfsr_layernorm_bwd(x.ptr, pe.ptr if pe else None, pe_rows, pe_div, g.ptr, dy.ptr, r, dx.ptr, dg.ptr, db.ptr, P(ws), ws_floats, M, C, capi.stream_ptr())
    torch.cuda.synchronize()
    return rc, dx, dg, db


@pytest.mark.parametrize("form", ["none", "ang", "spa"])
@pytest.mark.parametrize("mi", range(4), ids=["below_block", "cap", "cap+1", "ragged"])
@pytest.mark.parametrize("C", [64, 128])
def test_layernorm_backward_vs_fp64(C, mi, form):
    lib, M = capi.load(), ln_rows(C)[mi]
    c = ln_case(C, M, form)
    n_ws = lib.lfsr_layernorm_bwd_workspace_floats(C)
    assert n_ws == RED_BLOCKS * 2 * C
    ws = workspace(n_ws)
    for r_mode in ("null", "distinct", "dx"):
        outs = []
        for run in range(2):
            rc, dx, dg, db = ln_call(lib, c, C, M, form, r_mode, ws, n_ws, 10)
            capi.check(rc, "layernorm_bwd")
            outs.append([op_output_read(dx, 0, C), op_output_read(dg, 0, C), op_output_read(db, 0, C)])
            assert bool((ws[n_ws:] == OP_SENTINEL).all())
        assert all(torch.equal(a, b) for a, b in zip(*outs)), "two runs, other bits"
        add = 0 if r_mode == "null" else c["r"]
        row = f"C={C} M={M}"
        op_gate(outs[0][0], c["ref"][0] + add, c["cpu"][0] + add, "ln_bwd dx", f"pe={form} r={r_mode}", row, tag="BWDOP")
        op_gate(outs[0][1].reshape(-1), c["ref"][1], c["cpu"][1], "ln_bwd dgamma", f"pe={form} r={r_mode}", row, tag="BWDOP")
        op_gate(outs[0][2].reshape(-1), c["ref"][2], c["cpu"][2], "ln_bwd dbeta", f"pe={form} r={r_mode}", row, tag="BWDOP")


@pytest.mark.parametrize("C", [64, 128])
def test_layernorm_backward_refusals_write_nothing(C):
    """a workspace one float short: LFSR_E_WS; C = 96, M = 0, a null operand: LFSR_E_ARG; nothing written in any of them"""
    lib, M = capi.load(), 70
    c = ln_case(C, M, "ang")
    n_ws = lib.lfsr_layernorm_bwd_workspace_floats(C)
    assert lib.lfsr_layernorm_bwd_workspace_floats(96) == 0
    ws = workspace(n_ws)
    rc, dx, dg, db = ln_call(lib, c, C, M, "ang", "null", ws, n_ws - 1, 20)
    assert rc == E_WS and untouched(dx) and untouched(dg) and untouched(db) and intact(ws)
    st = capi.stream_ptr()
    x, dy, g = op_input(c["x"], C, 0, 1), op_input(c["dy"], C, 0, 2), op_input(c["gamma"].reshape(1, C), C, 0, 3)
    dx, dg, db = op_output(M, C, 20), op_output(1, C, 21), op_output(1, C, 22)
    for args in ((x.ptr, None, 0, 1, g.ptr, dy.ptr, None, dx.ptr, dg.ptr, db.ptr, P(ws), n_ws, M, 96),
                 (x.ptr, None, 0, 1, g.ptr, dy.ptr, None, dx.ptr, dg.ptr, db.ptr, P(ws), n_ws, 0, C),
                 (x.ptr, None, 0, 1, None, dy.ptr, None, dx.ptr, dg.ptr, db.ptr, P(ws), n_ws, M, C),
                 (x.ptr, None, 0, 1, g.ptr, dy.ptr, None, dx.ptr, dg.ptr, db.ptr, None, n_ws, M, C),
                 (x.ptr, x.ptr, 0, 1, g.ptr, dy.ptr, None, dx.ptr, dg.ptr, db.ptr, P(ws), n_ws, M, C)):      # a position term of no rows
        assert lib.lfsr_layernorm_bwd(*args, st) == E_ARG
        assert untouched(dx) and untouched(dg) and untouched(db) and intact(ws)


# ---------------------------------------------------------------------------------------------------------------------
# lfsr_linear_dgrad: every (cout -> cin) lfsr_trans_sublayer_bwd and lfsr_trans_tail_bwd launch, (cout, cin, masked)
# ---------------------------------------------------------------------------------------------------------------------
LIN_SHAPES = [(64, 128, True), (128, 256, True),                                   # feed_forward.4 of the angular / spatial sublayer: ReLU' of the hidden rows
              (128, 64, False), (256, 128, False), (64, 64, False), (128, 128, False),      # feed_forward.1, in_proj (q | k and v), out_proj, LFT's linear.0
              (256, 64, False), (576, 64, False), (1024, 64, False)]               # upsampling.0 at s = 2, 3, 4
LIN_ROWS = (1500, 3000, 70001)                                                     # as PW_SHAPES of tests/test_gpu_bwd_ops.py: 70001 is ragged in every tiling


@functools.lru_cache(maxsize=1)
def lin_case(M, cout, cin):
    g = torch.Generator().manual_seed(M + 7 * cin + cout)
    act = torch.randn(M, cin, generator=g)
    act.view(-1)[::89] = 0.0                      # exact zeros in the saved activation (and negative values): the mask is act > 0
    wt = torch.randn(cout, cin, generator=g) * 0.1
    dy, r1 = torch.randn(M, cout, generator=g), torch.randn(M, cin, generator=g)
    return dict(act=act, wt=wt, dy=dy, r1=r1, ref=dy.double() @ wt.double(), cpu=dy @ wt)


@pytest.mark.parametrize("M", LIN_ROWS)
@pytest.mark.parametrize("cout,cin,masked", LIN_SHAPES, ids=lambda v: str(v))
def test_linear_dgrad_vs_fp64(cout, cin, masked, M):
    lib, st = capi.load(), capi.stream_ptr()
    c = lin_case(M, cout, cin)
    wT = capi.pack_conv_weight_T(c["wt"].reshape(cout, cin, 1, 1).cuda())
    dy = op_input(c["dy"], cout, 0, 1)
    act = op_input(c["act"], cin + 12, 0, 2) if masked else None
    r1 = op_input(c["r1"], cin + 4, 0, 3)
    keep = (c["act"] > 0) if masked else torch.ones(M, cin, dtype=torch.bool)
    dx_stride = cin + 8
    for r_mode in ("null", "distinct") + (("dx",) if cout == cin else ()):
        outs = []
        for run in range(2):
            dx = op_output(M, dx_stride, 10)
            if r_mode == "dx":
                dx.t[:M, :cin] = c["r1"].cuda()
                dx.pristine[:M, :cin] = dx.t[:M, :cin]
            rp, rs = {"null": (None, 0), "distinct": (r1.ptr, cin + 4), "dx": (dx.ptr, dx_stride)}[r_mode]
            capi.check(lib.lfsr_linear_dgrad(dy.ptr, cout, P(wT), dx.ptr, dx_stride, rp, rs, act.ptr if masked else None, cin + 12 if masked else 0, M, cin, st),
                       "linear_dgrad")
            outs.append(op_output_read(dx, 0, cin))
        assert torch.equal(outs[0], outs[1]), "two runs, other bits"
        add = 0 if r_mode == "null" else c["r1"]
        op_gate(outs[0], c["ref"] * keep + add, c["cpu"] * keep + add, "linear_dgrad", f"{cout}->{cin} masked={masked} r1={r_mode}", f"M={M}", tag="BWDOP")


def test_linear_dgrad_refusals_write_nothing():
    """cout = 32 or 144, cin = 6, a stride below its row or off the float4 grid, M = 0, a null operand: LFSR_E_ARG, nothing written"""
    lib, st, M = capi.load(), capi.stream_ptr(), 300
    dy = torch.randn(M, 1024, device="cuda")
    wT = torch.randn(1024 * 256, device="cuda")
    r1 = torch.randn(M, 256, device="cuda")
    dx = op_output(M, 256, 30)
    d, w, r = P(dy), P(wT), P(r1)
    for args in ((d, 32, w, dx.ptr, 64, None, 0, None, 0, M, 64), (d, 144, w, dx.ptr, 64, None, 0, None, 0, M, 64), (d, 64, w, dx.ptr, 64, None, 0, None, 0, M, 6),
                 (d, 64, w, dx.ptr, 256, None, 0, None, 0, M, 96), (d, 64, w, dx.ptr, 60, None, 0, None, 0, M, 64), (d, 64, w, dx.ptr, 66, None, 0, None, 0, M, 64),
                 (d, 64, w, dx.ptr, 64, r, 32, None, 0, M, 64), (d, 64, w, dx.ptr, 64, r, 70, None, 0, M, 64), (d, 64, w, dx.ptr, 64, None, 0, r, 60, M, 64),
                 (d, 64, w, dx.ptr, 64, None, 0, r, 65, M, 64), (d, 64, w, dx.ptr, 64, None, 0, None, 0, 0, 64), (None, 64, w, dx.ptr, 64, None, 0, None, 0, M, 64),
                 (d, 64, None, dx.ptr, 64, None, 0, None, 0, M, 64), (d, 64, w, None, 64, None, 0, None, 0, M, 64)):
        assert lib.lfsr_linear_dgrad(*args, st) == E_ARG, args[1:]
        assert untouched(dx), args[1:]


# ---------------------------------------------------------------------------------------------------------------------
# lfsr_up_tail_bwd, lfsr_pack_up0_weight_tr
# ---------------------------------------------------------------------------------------------------------------------
# (B, A, h, w): the whole HR map is edge; 18 views, h != w, view boundaries inside the mosaic; 4225 LR pixels, past the 4096 that 1024 blocks of 4 cover
TAIL_GEOMS = [(1, 1, 1, 1), (2, 3, 5, 7), (1, 5, 13, 13)]
SLOPE = 0.2


@functools.lru_cache(maxsize=1)
def tail_case(B, A, h, w, s):
    npx = B * A * h * s * A * w * s
    hr = rnd((npx, 64), 71 + s)
    hr.view(-1)[::53] = 0.0                       # exact zeros and exact negative zeros: the derivative there is the slope (z > 0 ? 1 : slope), as torch's
    hr.view(-1)[7::101] = -0.0
    w3, dout = rnd((576,), 72 + s, 0.05), rnd((npx,), 73 + s)
    return dict(hr=hr, w3=w3, dout=dout, ref=tail_bwd_ref(hr, w3, dout, B, A, h, w, s, SLOPE, torch.float64),
                cpu=tail_bwd_ref(hr, w3, dout, B, A, h, w, s, SLOPE, torch.float32))


def tail_call(lib, c, B, A, h, w, s, ws, ws_floats):
    npix, Ws = B * A * A * h * w, A * w * s
    hr, w3, dout = op_input(c["hr"], 64, 0, 1), op_input(c["w3"].reshape(1, 576), 576, 0, 2), op_input(c["dout"].reshape(-1, Ws), Ws, 0, 3)
    du, dw3 = op_output(npix, 64 * s * s, 10), op_output(1, 576, 11)
    rc = lib.lfsr_up_tail_bwd(dout.ptr, w3.ptr, hr.ptr, du.ptr, dw3.ptr, P(ws), ws_floats, B, A, h, w, s, SLOPE, capi.stream_ptr())
    torch.cuda.synchronize()
    return rc, du, dw3


@pytest.mark.parametrize("B,A,h,w", TAIL_GEOMS)
@pytest.mark.parametrize("s", [2, 3, 4])
def test_up_tail_backward_vs_fp64(s, B, A, h, w):
    lib = capi.load()
    c = tail_case(B, A, h, w, s)
    n_ws = lib.lfsr_up_tail_bwd_workspace_floats()
    assert n_ws == RED_BLOCKS * 576
    ws = workspace(n_ws)
    outs = []
    for run in range(2):
        rc, du, dw3 = tail_call(lib, c, B, A, h, w, s, ws, n_ws)
        capi.check(rc, "up_tail_bwd")
        outs.append([op_output_read(du, 0, 64 * s * s), op_output_read(dw3, 0, 576)])
        assert bool((ws[n_ws:] == OP_SENTINEL).all())
    assert all(torch.equal(a, b) for a, b in zip(*outs)), "two runs, other bits"
    op_gate(outs[0][0], c["ref"][0], c["cpu"][0], "up_tail_bwd du", f"s={s}", (B, A, h, w), tag="BWDOP")
    op_gate(outs[0][1].reshape(-1), c["ref"][1], c["cpu"][1], "up_tail_bwd dw3", f"s={s}", (B, A, h, w), tag="BWDOP")


def test_up_tail_backward_refusals_write_nothing():
    lib, (B, A, h, w) = capi.load(), TAIL_GEOMS[1]
    c = tail_case(B, A, h, w, 2)
    n_ws = lib.lfsr_up_tail_bwd_workspace_floats()
    ws = workspace(n_ws)
    rc, du, dw3 = tail_call(lib, c, B, A, h, w, 2, ws, n_ws - 1)
    assert rc == E_WS and untouched(du) and untouched(dw3) and intact(ws)
    hr, w3, dout = op_input(c["hr"], 64, 0, 1), op_input(c["w3"].reshape(1, 576), 576, 0, 2), op_input(c["dout"].reshape(-1, A * w * 2), A * w * 2, 0, 3)
    st = capi.stream_ptr()
    for args in ((dout.ptr, w3.ptr, hr.ptr, du.ptr, dw3.ptr, P(ws), n_ws, B, A, h, w, 1), (dout.ptr, w3.ptr, hr.ptr, du.ptr, dw3.ptr, P(ws), n_ws, B, A, h, w, 5),
                 (dout.ptr, w3.ptr, hr.ptr, du.ptr, dw3.ptr, P(ws), n_ws, 0, A, h, w, 2), (dout.ptr, w3.ptr, hr.ptr, du.ptr, dw3.ptr, P(ws), n_ws, B, A, h, -w, 2),
                 (None, w3.ptr, hr.ptr, du.ptr, dw3.ptr, P(ws), n_ws, B, A, h, w, 2), (dout.ptr, w3.ptr, hr.ptr, du.ptr, dw3.ptr, None, n_ws, B, A, h, w, 2)):
        assert lib.lfsr_up_tail_bwd(*args, SLOPE, st) == E_ARG, args[6:]
        assert untouched(du) and untouched(dw3) and intact(ws), args[6:]


@pytest.mark.parametrize("s", [2, 3, 4])
def test_pack_up0_weight_tr_is_the_permutation(s):
    """out[k][c s^2 + ij] = Wp[(ij 64 + c) 64 + k], exactly"""
    lib, s2 = capi.load(), s * s
    wp = rnd((64 * s2 * 64,), 80 + s)
    src = op_input(wp.reshape(64 * s2, 64), 64, 0, 1)
    ref = wp.reshape(s2, 64, 64).permute(2, 1, 0).reshape(64, 64 * s2)         # [ij][c][k] -> [k][c][ij]
    for run in range(2):
        out = op_output(64, 64 * s2, 5)
        capi.check(lib.lfsr_pack_up0_weight_tr(src.ptr, out.ptr, s, capi.stream_ptr()), "pack_up0_weight_tr")
        assert np.array_equal(op_output_read(out, 0, 64 * s2).numpy(), ref.numpy())
    out = op_output(64, 64 * 25, 6)
    for s_bad in (1, 5):
        assert lib.lfsr_pack_up0_weight_tr(src.ptr, out.ptr, s_bad, capi.stream_ptr()) == E_ARG and untouched(out)


# ---------------------------------------------------------------------------------------------------------------------
# lfsr_window_attn_bwd at LFT's geometries
# ---------------------------------------------------------------------------------------------------------------------
def attn_both_selections(monkeypatch, q, k, v, d_o, ref, geometry, what):
    """the default selection and LFSR_ATTN=valu, each run twice -> {selection: (dqk, dv)}; both hold the rel-L2 gate, leave everything else alone and repeat their bits"""
    lib = capi.load()
    npix, E = q.shape
    _, qo, ko, _, vo, _, _ = attn_bwd_layout(E)
    o64, dq64, dk64, dv64 = ref
    o = o64.astype(np.float32)
    got = {}
    for sel in ("default", "valu"):
        if sel == "valu":
            monkeypatch.setenv("LFSR_ATTN", "valu")
        else:
            monkeypatch.delenv("LFSR_ATTN", raising=False)
        dqk, dv = attn_bwd_run(lib, q, k, v, o, d_o, LFT_NH, geometry)
        dqk2, dv2 = attn_bwd_run(lib, q, k, v, o, d_o, LFT_NH, geometry)
        errs = (rel_l2(dqk[:npix, qo:qo + E].cpu().numpy(), dq64), rel_l2(dqk[:npix, ko:ko + E].cpu().numpy(), dk64), rel_l2(dv[:npix, vo:vo + E].cpu().numpy(), dv64))
        print(f"BWDOP | attn_bwd | {what} | {sel} | rel-L2 dQ {errs[0]:.2e} dK {errs[1]:.2e} dV {errs[2]:.2e}")
        got[sel] = (dqk, dv, dqk2, dv2, errs)
    monkeypatch.delenv("LFSR_ATTN", raising=False)
    for sel, (dqk, dv, dqk2, dv2, errs) in got.items():
        assert max(errs) <= 1e-5, (what, sel, errs)
        assert torch.equal(dqk, dqk2) and torch.equal(dv, dv2), (what, sel)
        assert attn_bwd_untouched(dqk, dv, npix, E), (what, sel)
    return {sel: g[:2] for sel, g in got.items()}


def attn_operands(npix, E, seed):
    return [np.random.default_rng(seed + i).standard_normal((npix, E)).astype(np.float32) for i in range(4)]


# (B, A, h, w): a single view (softmax over one key: dQ = dK = 0 exactly); A^2 = 9; 25 views, the benchmark's angRes; 49 views
@pytest.mark.parametrize("B,A,h,w", [(2, 1, 3, 5), (1, 3, 6, 8), (2, 5, 4, 3), (1, 7, 2, 3)])
def test_angular_attention_backward_vs_fp64(B, A, h, w, monkeypatch):
    """the call of lft_train.hip's AngTrans: heads of 8, dense over the A^2 views of a pixel (n2 = 1, st2 = 0).  Heads of 8 have no matrix-pipe kernel: both
    selections run the VALU pair"""
    AA, HW = A * A, h * w
    q, k, v, d_o = attn_operands(B * AA * HW, 64, 50)
    geometry = (B, h, w, AA * HW, w, 1, AA, 1, HW, 0, AA, AA, 0, 1, 0)
    got = attn_both_selections(monkeypatch, q, k, v, d_o, lft_ang_attn_ref(q, k, v, d_o, B, A, h, w), geometry, f"angular {(B, A, h, w)}")
    assert torch.equal(got["default"][0], got["valu"][0]) and torch.equal(got["default"][1], got["valu"][1])


@pytest.mark.parametrize("n,h,w", LFT_SPA_GEOMS)
def test_spatial_attention_backward_vs_fp64(n, h, w, monkeypatch):
    """the call of lft_train.hip's SpaTrans: heads of 16, window [i-2, i+3) x [j-2, min(j+3, h, w)) on st1 = w, st2 = 1.
    (3,6,8): clip2 = h < n2 cuts the last columns' windows; (2,13,7): clip2 > n2; (2,7,9): w = h + 2, the last column sees exactly one key column; (1,1,1): one
    pixel; (4,3,5): h <= 3, every row visible from every row, which the matrix-pipe kernel's gate accepts -- the default selection runs k_epi_attn_bwd_mfma on a 2-D
    window there (other bits than the VALU pair), and refuses everywhere else (the same bits): h > 3, and the one-token sequence of (1,1,1), whose dQ = dK = 0 and
    dV = dO only the VALU pair returns exactly (lfsr_epi_attn_bwd_mfma_launch hands it over; before it did, the default selection left rounding residue in dQ and dK
    there -- an infinite rel-L2 against the zero reference -- and dV at rel-L2 9.2e-8)."""
    q, k, v, d_o = attn_operands(n * h * w, 128, 60)
    geometry = (n, 1, 1, h * w, 0, 0, h, w, w, 1, 2, 3, 2, 3, h)
    got = attn_both_selections(monkeypatch, q, k, v, d_o, lft_spa_attn_ref(q, k, v, d_o, n, h, w), geometry, f"spatial {(n, h, w)}")
    same = torch.equal(got["default"][0], got["valu"][0]) and torch.equal(got["default"][1], got["valu"][1])
    print(f"BWDOP | attn_bwd | spatial {(n, h, w)} | default selection ran {'the VALU pair' if same else 'k_epi_attn_bwd_mfma'}")
    assert same == ((n, h, w) != (4, 3, 5))
