"""GPU: lfsr_set_branch_arithmetic(LFSR_BRANCH_ARITH_BF16) -- DistgSSR's EPI branch (stage 1) and fused block tail at angRes 5 on bf16 operands
(csrc/distg_bf16.hip: k_epi_bf16, k_distg_tail_bf16).

Emulation, fp64 on the CPU, r(t) = t.to(torch.bfloat16).double(): the block of tests/helpers.py::distg_layers_fp64 (stock torch conv2d / pixel_shuffle) from the
SpaConv.2 output on, with
  EPIConv.0 (both passes)  conv(r(x), r(W))
  EPIConv.2 (both passes)  conv(r(t_H | t_V), r(W))          t = the post-LeakyReLU stage-1 result
  fuse.0                   conv(r(spa | ang | epiH | epiV), r(W))
and everything else (AngConv.0, AngConv.2, LeakyReLU) unrounded; y_exact is the same block without r.
Gates.  t_A is not in the mode: bit-equal to the default's.  t_H / t_V round no intermediate, so they differ from the emulation by fp32 accumulation over K = 1600
only: the suite's max abs <= 1e-4.  y passes through intermediates the kernel rounded after fp32 accumulation (an element on the other side of a rounding tie moves
an operand by a whole bf16 ulp), so the gate is the project's: ||y - y_emul||_2 <= 0.1 ||y_emul - y_exact||_2.
Whole-model gates: those of tests/test_gpu_conv3x3_bf16.py::test_whole_model.  CPU emulation of the mode with stock torch, rms against the
fp64 graph: (5, 2, 2, 8, 8) 2.82e-5 alone, 3.87e-4 with LFSR_ARITH_BF16 (autocast port 1.07e-3); (5, 4, 1, 10, 9) 2.85e-5 / 4.14e-4 (1.01e-3).
Every test restores all four arithmetic selections."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from oracle import lfsr_torch_port as TP
from tests.helpers import distg_case, distg_layers_fp64, epit_case, macpi_to_rows, psnr

pytestmark = pytest.mark.gpu
A, L = 5, 0.1
ATOL = 1e-4
GUARD = 4096            # floats in front of and behind every output
SENTINEL = -12345.5
F = torch.nn.functional


@contextlib.contextmanager
def modes(arith=capi.ARITH_DEFAULT, branch=capi.BRANCH_ARITH_DEFAULT):
    """the two selections for the block; all four are the default again after it (the settings are process-wide)"""
    try:
        capi.set_arithmetic(arith)
        capi.set_branch_arithmetic(branch)
        yield
    finally:
        capi.set_arithmetic(capi.ARITH_DEFAULT)
        capi.set_grad_arithmetic(capi.GRAD_ARITH_DEFAULT)
        capi.set_gemm_arithmetic(capi.GEMM_ARITH_DEFAULT)
        capi.set_branch_arithmetic(capi.BRANCH_ARITH_DEFAULT)


BF16 = functools.partial(modes, branch=capi.BRANCH_ARITH_BF16)


def r(t):
    return t.to(torch.bfloat16).double()


def l2(a):
    return float(torch.linalg.vector_norm(a.double()))


def _raw_weights(seed):
    """the draws of tests/test_gpu_distg_tail_edges.py::_weights, unpacked (fp32, CPU): AngConv.0, AngConv.2, EPIConv.0, EPIConv.2, fuse.0"""
    g = torch.Generator().manual_seed(seed)
    def rnd(*shape, fan):
        return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * (1.0 / fan) ** 0.5).float()
    return (rnd(16, 64, A, A, fan=64 * 25), rnd(16 * A * A, 16, 1, 1, fan=16), rnd(32, 64, 1, A * A, fan=64 * 25), rnd(32 * A, 32, 1, 1, fan=32),
            rnd(64, 144, 1, 1, fan=144))


def _pack(raw):
    w = [t.cuda() for t in raw]
    return (capi.pack_conv_weight(w[0]), capi.pack_conv_weight(w[1], perm=1, ch=16), capi.pack_conv_weight(w[2]), capi.pack_conv_weight(w[3]),
            capi.pack_conv_weight(w[4]))


def _rows_to_macpi(rows, B, h, w):
    """VCL rows (B A^2 h w, C), view u A + v -> NCHW MacPI (B, C, h A, w A): the inverse of helpers.macpi_to_rows"""
    C = rows.shape[1]
    return rows.reshape(B, A, A, h, w, C).permute(0, 5, 3, 1, 4, 2).reshape(B, C, h * A, w * A).contiguous()


def _block_fp64(x_rows, spa_rows, raw, B, h, w, rnd):
    """the block of distg_layers_fp64 from the SpaConv.2 output on, with `rnd` on the operands the mode rounds -> (y rows, t_A, t_H, t_V) in the operator's layouts"""
    wa0, wa2, we0, we2, wf = [t.double() for t in raw]
    z, spa = _rows_to_macpi(x_rows.double(), B, h, w), _rows_to_macpi(spa_rows.double(), B, h, w)
    lr = lambda t: F.leaky_relu(t, L)
    a1 = lr(F.conv2d(z, wa0, stride=A))                                      # (B, 16, h, w)
    ang = F.pixel_shuffle(lr(F.conv2d(a1, wa2)), A)

    def epi(t):
        e = lr(F.conv2d(rnd(t), rnd(we0), stride=(1, A), padding=(0, A * (A - 1) // 2)))
        return e, TP.pixel_shuffle1d(lr(F.conv2d(rnd(e), rnd(we2))), A)
    eh, epih = epi(z)                                                        # eh (B, 32, h A, w): [b, n, y A + u, x]
    ev, epiv = epi(z.permute(0, 1, 3, 2).contiguous())                       # ev (B, 32, w A, h): [b, n, x A + v, y]
    epiv = epiv.permute(0, 1, 3, 2)
    cat = torch.cat((spa, ang, epih, epiv), dim=1)
    y = lr(F.conv2d(rnd(cat), rnd(wf)))
    t_a = a1.permute(0, 2, 3, 1).reshape(-1, 16)
    t_h = eh.reshape(B, 32, h, A, w).permute(0, 3, 2, 4, 1).reshape(-1, 32)      # rows (b, u, y, x)
    t_v = ev.reshape(B, 32, w, A, h).permute(0, 3, 4, 2, 1).reshape(-1, 32)      # rows (b, v, y, x)
    return macpi_to_rows(y, A), t_a, t_h, t_v


def _operands(B, h, w):
    torch.manual_seed(B * 1000 + h * 10 + w)
    npix = B * A * A * h * w
    x = torch.randn((npix, 64), dtype=torch.float32, device="cuda")
    spa = F.leaky_relu(torch.randn((npix, 64), dtype=torch.float32, device="cuda"), L)
    return x, spa


# ---------------------------------------------------------------------------------------------------------------------
# 1. the operator against the fp64 emulation
# ---------------------------------------------------------------------------------------------------------------------
# (2, 8, 8): 8 tiles, most waves own none; (1, 5, 3): one ragged tile of 15 macro-pixels; (3, 9, 7): tiles that straddle patches
@pytest.mark.parametrize("B,h,w", [(2, 8, 8), (1, 5, 3), (3, 9, 7)])
def test_operator_against_the_fp64_emulation(B, h, w):
    x, spa = _operands(B, h, w)
    raw = _raw_weights(11 + B)
    wp = _pack(raw)
    y_def, ta_def, th_def, tv_def = [t.clone() for t in capi.distg_branch_tail(x, spa, *wp, B, A, h, w, L)]
    with BF16():
        y, t_a, t_h, t_v = [t.clone() for t in capi.distg_branch_tail(x, spa, *wp, B, A, h, w, L)]
        torch.cuda.synchronize()
    y_em, _, th_em, tv_em = _block_fp64(x.cpu(), spa.cpu(), raw, B, h, w, r)
    y_ex, _, th_ex, tv_ex = _block_fp64(x.cpu(), spa.cpu(), raw, B, h, w, lambda t: t)
    e_h, e_v = float((t_h.cpu().double() - th_em).abs().max()), float((t_v.cpu().double() - tv_em).abs().max())
    num, den = l2(y.cpu().double() - y_em), l2(y_em - y_ex)
    print(f"BRANCH_BF16 operator ({B}, {h}, {w}): t_H max|gpu - emul| {e_h:.2e}, t_V {e_v:.2e} (emul vs exact: {float((th_em - th_ex).abs().max()):.2e}); "
          f"y ||gpu - emul|| / ||emul - exact|| = {num:.3e} / {den:.3e} = {num / den:.4f}; default y vs exact max {float((y_def.cpu().double() - y_ex).abs().max()):.2e}")
    # the reference itself: the default operator is the unrounded block
    assert float((y_def.cpu().double() - y_ex).abs().max()) <= ATOL and float((th_def.cpu().double() - th_ex).abs().max()) <= ATOL
    assert float((tv_def.cpu().double() - tv_ex).abs().max()) <= ATOL
    assert torch.equal(t_a, ta_def)                       # AngConv.0 is not in the mode
    assert e_h <= ATOL and e_v <= ATOL
    assert num <= 0.1 * den
    assert not torch.equal(y, y_def) and not torch.equal(t_h, th_def) and not torch.equal(t_v, tv_def)      # the mode is live in both kernels


# ---------------------------------------------------------------------------------------------------------------------
# 2. writes only its rows
# ---------------------------------------------------------------------------------------------------------------------
def _guarded(rows, cols):
    """a (rows, cols) tensor in the middle of a sentinel-filled allocation; 16-byte aligned like a fresh one"""
    pool = torch.full((2 * GUARD + rows * cols,), SENTINEL, dtype=torch.float32, device="cuda")
    return pool, pool[GUARD:GUARD + rows * cols].view(rows, cols)


@pytest.mark.parametrize("B,h,w", [(1, 5, 3), (3, 9, 7)])
def test_writes_only_its_rows(B, h, w):
    x, spa = _operands(B, h, w)
    wp = _pack(_raw_weights(11 + B))
    npix = B * A * A * h * w
    pools, outs = zip(*[_guarded(rr, c) for rr, c in ((npix, 64), (B * h * w, 16), (B * A * h * w, 32), (B * A * h * w, 32))])
    with BF16():
        ref = [t.clone() for t in capi.distg_branch_tail(x, spa, *wp, B, A, h, w, L)]
        got = capi.distg_branch_tail(x, spa, *wp, B, A, h, w, L, out=outs)
        torch.cuda.synchronize()
    assert got[0].data_ptr() == outs[0].data_ptr()
    for name, pool, o, rf in zip(("y", "t_a", "t_h", "t_v"), pools, outs, ref):
        assert bool((pool[:GUARD] == SENTINEL).all()) and bool((pool[GUARD + o.numel():] == SENTINEL).all()), name + ": written outside its rows"
        assert not bool((o == SENTINEL).any()), name + ": rows left unwritten"
        assert torch.equal(o, rf), name


# ---------------------------------------------------------------------------------------------------------------------
# 3. launch-size invariance and determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_launch_size_invariance_and_determinism():
    """k_distg_tail_bf16 runs two blocks of 8 waves per CU: 4096 waves on 256 CUs, so the existing edge test's (40, 32, 32) = 2560 tiles would leave every wave at
    most one tile.  (66, 32, 32): 4224 tiles, some waves own two (the hand-over between tiles); k_epi_bf16 walks 2640 groups of 8 lines on 256 blocks: ten full
    rounds and a last one cut into sub-groups.  The first patch's rows equal a B = 1 launch bit for bit, and two launches are bit-equal.  No fp64 work here."""
    B, h, w = 66, 32, 32
    x, spa = _operands(B, h, w)
    wp = _pack(_raw_weights(7))
    n1 = A * A * h * w
    with BF16():
        y, _, t_h, t_v = capi.distg_branch_tail(x, spa, *wp, B, A, h, w, L)
        y2, _, t_h2, t_v2 = capi.distg_branch_tail(x, spa, *wp, B, A, h, w, L)
        y1, _, t_h1, t_v1 = capi.distg_branch_tail(x[:n1].contiguous(), spa[:n1].contiguous(), *wp, 1, A, h, w, L)
        torch.cuda.synchronize()
    assert torch.equal(y, y2) and torch.equal(t_h, t_h2) and torch.equal(t_v, t_v2)
    assert torch.equal(y[:n1], y1) and torch.equal(t_h[:A * h * w], t_h1) and torch.equal(t_v[:A * h * w], t_v1)


# ---------------------------------------------------------------------------------------------------------------------
# 4. whole model
# ---------------------------------------------------------------------------------------------------------------------
def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def _distg(A_, s, sd):
    rt = capi.DistgSSRRuntime(A_, s)
    rt.load_state([(k, torch.from_numpy(v).cuda()) for k, v in sd.items()], torch.device("cuda"))
    return rt


# both run the fused tail ((5, 2, 2, 8, 8): 3200 pixels, (5, 4, 1, 10, 9): 2250, at least the driver's 2048) and have ragged tiles
@pytest.mark.parametrize("geom", [(5, 2, 2, 8, 8), (5, 4, 1, 10, 9)])
def test_whole_model(geom):
    A_, s, B, h, w = geom
    sd, x = distg_case(A_, s, B, h, w)
    y64 = distg_layers_fp64(x, sd, A_, s)[0].numpy()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        y_amp = TP.distgssr_forward(torch.from_numpy(x), {k: torch.from_numpy(v) for k, v in sd.items()}, A_, s).double().numpy()
    label = torch.rand(y64.shape, generator=torch.Generator().manual_seed(2)).numpy()
    rt = _distg(A_, s, sd)
    xg = torch.from_numpy(x).cuda()
    y_def = rt.forward(xg).cpu().numpy()
    e_amp, e_def = _rms(y_amp, y64), _rms(y_def, y64)
    assert np.abs(y_def - y64).max() < ATOL             # the default is what it was
    for tag, arith in (("branch mode", capi.ARITH_DEFAULT), ("branch + conv modes", capi.ARITH_BF16)):
        with modes(arith=arith, branch=capi.BRANCH_ARITH_BF16):
            y = rt.forward(xg).cpu().numpy()
        dpsnr = psnr(y, label) - psnr(y64, label)
        e = _rms(y, y64)
        print(f"distgssr {geom} {tag}: rms {e:.2e} max {np.abs(y - y64).max():.2e} vs fp64; autocast port rms {e_amp:.2e} (ratio {e_amp / e:.2f}); "
              f"default mode rms {e_def:.2e}; dPSNR vs label {dpsnr:+.5f} dB")
        assert abs(dpsnr) <= 0.01                       # (a) the project's gate
        assert e <= e_amp                               # (b) not worse than the reference's own reduced-precision path
        assert not np.array_equal(y, y_def)             # (c) the mode is live in the model driver
    assert np.array_equal(rt.forward(xg).cpu().numpy(), y_def)


# ---------------------------------------------------------------------------------------------------------------------
# 5. what does not follow the mode
# ---------------------------------------------------------------------------------------------------------------------
def _same_under_the_mode(rt, xg, fn="forward"):
    before = getattr(rt, fn)(xg).clone()
    with BF16():
        y = getattr(rt, fn)(xg).clone()
    torch.cuda.synchronize()
    return torch.equal(y, before)


def test_what_does_not_follow_the_mode():
    # 1600 pixels: below the 2048 from which the model driver runs the fused tail
    sd, x = distg_case(5, 2, 1, 8, 8)
    rt = _distg(5, 2, sd)
    assert _same_under_the_mode(rt, torch.from_numpy(x).cuda())
    # angRes 3
    sd3, x3 = distg_case(3, 2, 2, 6, 8)
    assert _same_under_the_mode(_distg(3, 2, sd3), torch.from_numpy(x3).cuda())
    # the training forward keeps the three-kernel sequence
    sd, x = distg_case(5, 2, 2, 8, 8)
    rt = _distg(5, 2, sd)
    xg = torch.from_numpy(x).cuda()
    assert _same_under_the_mode(rt, xg, "forward_train")
    # LFSR_ARITH_F32 wins
    with modes(arith=capi.ARITH_F32):
        alone = rt.forward(xg).clone()
    with modes(arith=capi.ARITH_F32, branch=capi.BRANCH_ARITH_BF16):
        both = rt.forward(xg).clone()
    default = rt.forward(xg).clone()
    assert torch.equal(alone, both)
    # after the mode the default forward is what it was, and the mode was live at this geometry (so the comparisons above are not vacuous)
    with BF16():
        y = rt.forward(xg).clone()
    assert not torch.equal(y, default)
    assert capi.get_branch_arithmetic() == capi.BRANCH_ARITH_DEFAULT
    assert torch.equal(rt.forward(xg), default)
    # EPIT
    sde, xe = epit_case(5, 2, 1, 8, 8)
    rte = capi.ModelRuntime("epit", 5, 2, 5, 64)
    rte.load_state([(k, torch.from_numpy(v).cuda()) for k, v in sde.items()], torch.device("cuda"))
    assert _same_under_the_mode(rte, torch.from_numpy(xe).cuda())


# ---------------------------------------------------------------------------------------------------------------------
# 6. graphs
# ---------------------------------------------------------------------------------------------------------------------
def test_graphed_forward_follows_the_branch_arithmetic():
    """a graph captured under the default must not be replayed under the mode: GraphedForward keys its cache on this selection as well"""
    sd, x = distg_case(5, 2, 2, 8, 8)
    rt = _distg(5, 2, sd)
    xg = torch.from_numpy(x).cuda()
    gf = capi.GraphedForward(rt)
    y_graph_def = gf(xg).clone()
    y_def = rt.forward(xg).clone()
    with BF16():
        y_graph = gf(xg).clone()
        y_eager = rt.forward(xg).clone()
        torch.cuda.synchronize()
    assert torch.equal(y_graph_def, y_def)
    assert torch.equal(y_graph, y_eager) and not torch.equal(y_graph, y_def)
    assert len(gf.graphs) == 2
    assert torch.equal(gf(xg), y_def)               # back under the default: the first graph again
