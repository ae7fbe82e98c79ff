"""GPU: lfsr_set_lin_grad_arithmetic(LFSR_LIN_GRAD_ARITH_BF16) -- the weight gradient (csrc/lin_wgrad_bf16.hip) and the data gradient (csrc/lin_dgrad_bf16.hip) of
the transformers' linears on bf16-rounded operands, fp32 accumulation -- and the operator lfsr_linear_wgrad in both modes; everything else, the forwards included, as
it was.

Operators, at every (cout, cin) the EPIT and LFT drivers run and M in {5, 3000, 70001}.  Default lfsr_linear_wgrad: the bits of lfsr_pointwise_wgrad per 64-row
slice (dy_choff = n0), and the gate of tests/test_gpu_trans_bwd_ops.py against fp64 (tests.helpers.op_gate).  Under the mode a kernel differs from the fp64 product
of the SAME rounded operands (torch.Tensor.bfloat16()) by fp32 accumulation only: rel-L2 <= 1e-4 for the weight gradient, max|err| < 1e-4 for the data gradient
(dy ~ N(0, 1), weights x 0.1): the gates of tests/test_gpu_grad_bf16.py.

Whole models (EPIT, LFT through their plugins in .train(), L1 against synth_input(seed = 2)): the gradient bucket's rel-L2 error against fp64 autograd under the HIP
forward's own decisions (TH.epit_forced_fp64_grads / TH.lft_forced_fp64_grads) not above that of the reference's own reduced-precision path -- the stock graph
under torch.autocast("cpu", bfloat16) against its plain fp64 autograd -- margin 1.0x; the same per tensor for every linear weight the mode computes
(tests/lin_grad_emulation.py: MODE_LINEARS); every other tensor printed.  What the CPU emulation of the mode (that file: the same graphs with dy, W and x rounded
in the linears' backward) forecast before any GPU run, autocast error / emulated error:
    case            bucket (emulated | autocast | ratio)     smallest ratio of a mode linear                       smallest ratio of any other tensor
    EPIT a5h8s4     2.12e-4 | 4.55e-3 | 21.5x                4.81x  altblock.0.epi_trans.attention.in_proj_weight   4.21x  altblock.2.epi_trans.norm.bias
    EPIT a3h6w8s3   2.89e-4 | 1.33e-2 | 46.0x                13.3x  altblock.4.epi_trans.attention.in_proj_weight   12.4x  altblock.3.epi_trans.norm.weight
    LFT a5h8s4      1.94e-3 | 1.80e-2 | 9.26x                5.34x  altblock.3.spa_trans.attention.in_proj_weight   6.68x  altblock.3.spa_trans.feed_forward.0.weight
    LFT a3h6w8s2    2.19e-3 | 2.37e-2 | 10.8x                5.82x  altblock.3.spa_trans.attention.in_proj_weight   6.73x  altblock.2.spa_trans.norm.weight
No tensor of the emulation lies outside autocast's error, so every named weight is gated at 1.0x and none at the 1.5x-of-its-emulated-error allowance.
Measured on the GPU (hip bucket error | autocast | ratio; smallest ratio of a mode linear; of any other tensor): EPIT a5h8s4 2.12e-4 | 4.79e-3 | 22.6x; 5.40x; 4.96x.
EPIT a3h6w8s3 2.89e-4 | 1.08e-2 | 37.2x; 11.0x; 11.4x.  LFT a5h8s4 2.00e-3 | 1.79e-2 | 8.96x; 5.28x; 5.20x.  LFT a3h6w8s2 2.18e-3 | 2.44e-2 | 11.2x; 7.39x; 7.62x.
profiles/lin_grad_bf16_time.md has the times."""
import contextlib
import functools
import importlib
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lfsr_amd import capi
from lfsr_amd.synth import synth_input
from tests import helpers as TH
from tests import lin_grad_emulation as EMU
from tests.helpers import OP_SENTINEL, op_gate, op_input, op_output, op_output_read

pytestmark = pytest.mark.gpu
torch.set_num_threads(8)
ATOL = 1e-4
E_ARG, E_WS = -1, -2
BAND = 4096                     # sentinel floats behind a workspace
P = capi.dev_ptr

# (cout, cin): every driver call -- feed_forward.4 / .1, in_proj (q | k and v), out_proj, linear_in / linear_out, linear.0 -- both extremes of either dimension,
# and upsampling.0 at scales 2, 3, 4
SHAPES = [(64, 64), (64, 128), (128, 64), (128, 128), (128, 256), (256, 128), (256, 64), (576, 64), (1024, 64)]
ROWS = (5,          # fewer rows than one MFMA K step
        3000,
        70001)      # ragged in every tiling and more row tiles than blocks: the accumulators carry across tiles


@contextlib.contextmanager
def lin_grad_arithmetic(mode):
    """lfsr_set_lin_grad_arithmetic(mode) for the block, the default again after it (the setting is process-wide)"""
    capi.set_lin_grad_arithmetic(mode)
    try:
        yield
    finally:
        capi.set_lin_grad_arithmetic(capi.LIN_GRAD_ARITH_DEFAULT)


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def r16(t):
    """the same values rounded to bf16 (nearest even), as fp64"""
    return t.float().bfloat16().double()


def workspace(n):
    return torch.full((n + BAND,), OP_SENTINEL, device="cuda")


def intact(ws, n):
    torch.cuda.synchronize()
    return bool((ws[n:] == OP_SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------
# lfsr_linear_wgrad
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def wgrad_case(M, cout, cin):
    g = torch.Generator().manual_seed(3 * M + 7 * cin + cout)
    dy, x, dw0 = torch.randn(M, cout, generator=g), torch.randn(M, cin, generator=g), torch.randn(cout, cin, generator=g)
    return dict(dy=dy, x=x, dw0=dw0, ref=dy.double().t() @ x.double(), cpu=dy.t() @ x, ref_r=r16(dy).t() @ r16(x))


def wgrad_call(lib, dy, dys, x, xs, dw, ws, n_ws, M, cout, cin, accumulate):
    return lib.lfsr_linear_wgrad(dy.ptr, dys, x.ptr, xs, P(dw), P(ws), n_ws, M, cout, cin, accumulate, capi.stream_ptr())


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("cout,cin", SHAPES, ids=lambda v: str(v))
def test_linear_wgrad_default_is_the_sliced_pointwise_wgrad_and_fp64(cout, cin, M):
    lib, st = capi.load(), capi.stream_ptr()
    c = wgrad_case(M, cout, cin)
    dys, xs = cout + 8, cin + 12
    dy, x = op_input(c["dy"], dys, 0, 1), op_input(c["x"], xs, 0, 2)
    n_ws = lib.lfsr_linear_wgrad_workspace_floats(M, cout, cin)
    assert n_ws > 0
    ws = workspace(n_ws)
    # the code as it stands: lfsr_pointwise_wgrad on each 64-row slice
    want = torch.empty(cout, cin, device="cuda")
    n_pw = lib.lfsr_pointwise_wgrad_workspace_floats(M, 64, cin)
    ws_pw = workspace(n_pw)
    for n0 in range(0, cout, 64):
        capi.check(lib.lfsr_pointwise_wgrad(dy.ptr, dys, n0, 64, x.ptr, xs, 0, cin, P(want[n0:n0 + 64]), P(ws_pw), n_pw, M, 0, st), "pointwise_wgrad")
    for accumulate in (0, 1):
        dw0 = c["dw0"] if accumulate else torch.full((cout, cin), OP_SENTINEL)
        dw = dw0.cuda()
        capi.check(wgrad_call(lib, dy, dys, x, xs, dw, ws, n_ws, M, cout, cin, accumulate), "linear_wgrad")
        assert intact(ws, n_ws)
        if accumulate:
            assert torch.equal(dw, c["dw0"].cuda() + want)      # (one fp32 add per element in either)
        else:
            assert torch.equal(dw, want), "the default is not the sliced pointwise weight gradient"
        add = c["dw0"] if accumulate else 0
        op_gate(dw, c["ref"] + add, c["cpu"] + add, "linear_wgrad", f"{cout}x{cin} accumulate={accumulate}", f"M={M}", tag="LINGRAD")


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("cout,cin", SHAPES, ids=lambda v: str(v))
def test_linear_wgrad_bf16_is_the_exact_form_on_rounded_operands(cout, cin, M):
    lib = capi.load()
    c = wgrad_case(M, cout, cin)
    n_ws = lib.lfsr_linear_wgrad_workspace_floats(M, cout, cin)
    ws = workspace(n_ws)
    dense = (op_input(c["dy"], cout, 0, 1), cout, op_input(c["x"], cin, 0, 2), cin)
    strided = (op_input(c["dy"], cout + 8, 0, 3), cout + 8, op_input(c["x"], cin + 12, 0, 4), cin + 12)
    with lin_grad_arithmetic(capi.LIN_GRAD_ARITH_BF16):
        assert lib.lfsr_linear_wgrad_workspace_floats(M, cout, cin) == n_ws          # the workspace does not depend on the mode
        for form, (dy, dys, x, xs) in (("dense", dense), ("strided", strided)):
            for accumulate in (0, 1):
                outs = []
                for run in range(2):
                    dw = (c["dw0"] if accumulate else torch.full((cout, cin), OP_SENTINEL)).cuda()
                    capi.check(wgrad_call(lib, dy, dys, x, xs, dw, ws, n_ws, M, cout, cin, accumulate), "linear_wgrad")
                    assert intact(ws, n_ws)
                    outs.append(dw)
                assert torch.equal(outs[0], outs[1]), "two runs, other bits"
                e = rel(outs[0], c["ref_r"] + (c["dw0"].double() if accumulate else 0.0))
                print(f"LINGRAD | bf16 wgrad {cout}x{cin} M={M} {form} accumulate={accumulate}: rel-L2 vs fp64(rounded operands) {e:.2e}")
                assert bool(torch.isfinite(outs[0]).all()) and e <= 1e-4


def test_linear_wgrad_refusals_write_nothing():
    """in both modes: cout = 32 or 144, cin = 6 or 96, a stride below its row or off the float4 grid, M = 0, a null operand: LFSR_E_ARG; a workspace one float short:
    LFSR_E_WS; nothing written in any of them"""
    lib, st, M = capi.load(), capi.stream_ptr(), 300
    dy = torch.randn(M, 1024, device="cuda")
    x = torch.randn(M, 256, device="cuda")
    fill = torch.randn(1024, 256, device="cuda")
    dw = fill.clone()
    n_ws = lib.lfsr_linear_wgrad_workspace_floats(M, 1024, 256)
    ws = workspace(n_ws)
    d, xx, w, s = P(dy), P(x), P(dw), P(ws)
    for mode in (capi.LIN_GRAD_ARITH_DEFAULT, capi.LIN_GRAD_ARITH_BF16):
        with lin_grad_arithmetic(mode):
            for args in ((d, 1024, xx, 256, w, s, n_ws, M, 32, 64, 0), (d, 1024, xx, 256, w, s, n_ws, M, 144, 64, 0), (d, 1024, xx, 256, w, s, n_ws, M, 64, 6, 0),
                         (d, 1024, xx, 256, w, s, n_ws, M, 64, 96, 0), (d, 60, xx, 256, w, s, n_ws, M, 64, 64, 0), (d, 66, xx, 256, w, s, n_ws, M, 64, 64, 0),
                         (d, 1024, xx, 32, w, s, n_ws, M, 64, 64, 0), (d, 1024, xx, 70, w, s, n_ws, M, 64, 64, 0), (d, 1024, xx, 256, w, s, n_ws, 0, 64, 64, 0),
                         (None, 1024, xx, 256, w, s, n_ws, M, 64, 64, 0), (d, 1024, None, 256, w, s, n_ws, M, 64, 64, 0), (d, 1024, xx, 256, None, s, n_ws, M, 64, 64, 0),
                         (d, 1024, xx, 256, w, None, n_ws, M, 64, 64, 0)):
                assert lib.lfsr_linear_wgrad(*args, st) == E_ARG, (mode, args[1::2])
                torch.cuda.synchronize()
                assert torch.equal(dw, fill) and bool((ws == OP_SENTINEL).all()), (mode, args[1::2])
            for cout, cin in ((64, 64), (1024, 64), (256, 128)):
                n = lib.lfsr_linear_wgrad_workspace_floats(M, cout, cin)
                assert lib.lfsr_linear_wgrad(d, 1024, xx, 256, w, s, n - 1, M, cout, cin, 0, st) == E_WS
                torch.cuda.synchronize()
                assert torch.equal(dw, fill) and bool((ws == OP_SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------
# lfsr_linear_dgrad under the mode
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def dgrad_case(M, cout, cin):
    """lin_case of tests/test_gpu_trans_bwd_ops.py, and the fp64 forms of the rounded and of the exact operands"""
    g = torch.Generator().manual_seed(M + 7 * cin + cout)
    act = torch.randn(M, cin, generator=g)
    act.view(-1)[::89] = 0.0                      # exact zeros in the saved activation (and negative values): the mask is act > 0
    wt = torch.randn(cout, cin, generator=g) * 0.1
    dy, r1 = torch.randn(M, cout, generator=g), torch.randn(M, cin, generator=g)
    return dict(act=act, wt=wt, dy=dy, r1=r1, ref_r=r16(dy) @ r16(wt), ref_e=dy.double() @ wt.double())


def dgrad_run(lib, c, M, cout, cin, wT, dy, r_mode, masked, r1, act, dx_stride, seed=10):
    dx = op_output(M, dx_stride, seed)
    if r_mode == "dx":
        dx.t[:M, :cin] = c["r1"].cuda()
        dx.pristine[:M, :cin] = dx.t[:M, :cin]
    rp, rs = {"null": (None, 0), "distinct": (r1.ptr, cin + 4), "dx": (dx.ptr, dx_stride)}[r_mode]
    capi.check(lib.lfsr_linear_dgrad(dy.ptr, cout, P(wT), dx.ptr, dx_stride, rp, rs, act.ptr if masked else None, cin + 12 if masked else 0, M, cin,
                                     capi.stream_ptr()), "linear_dgrad")
    return op_output_read(dx, 0, cin)             # (asserts that the columns beyond cin and the rows behind M kept their bits)


@pytest.mark.parametrize("M", ROWS)
@pytest.mark.parametrize("cout,cin", SHAPES, ids=lambda v: str(v))
def test_linear_dgrad_bf16_is_the_exact_form_on_rounded_operands(cout, cin, M):
    lib = capi.load()
    c = dgrad_case(M, cout, cin)
    wT = capi.pack_conv_weight_T(c["wt"].reshape(cout, cin, 1, 1).cuda())
    dy, act, r1 = op_input(c["dy"], cout, 0, 1), op_input(c["act"], cin + 12, 0, 2), op_input(c["r1"], cin + 4, 0, 3)
    forms = [("null", False), ("null", True), ("distinct", True)] + ([("dx", False)] if cout == cin else [])
    with lin_grad_arithmetic(capi.LIN_GRAD_ARITH_BF16):
        for r_mode, masked in forms:
            outs = [dgrad_run(lib, c, M, cout, cin, wT, dy, r_mode, masked, r1, act, cin + 8) for run in range(2)]
            assert torch.equal(outs[0], outs[1]), "two runs, other bits"
            keep = (c["act"] > 0) if masked else torch.ones(M, cin, dtype=torch.bool)
            ref = c["ref_r"] * keep + (0 if r_mode == "null" else c["r1"].double())
            e = float((outs[0].double() - ref).abs().max())
            print(f"LINGRAD | bf16 dgrad {cout}->{cin} M={M} r1={r_mode} masked={masked}: max|hip - fp64(rounded operands)| {e:.2e}")
            assert bool(torch.isfinite(outs[0]).all()) and e < ATOL


def test_it_really_is_bf16_and_the_default_is_untouched():
    lib, M = capi.load(), 3000
    for cout, cin in ((256, 128), (1024, 64)):
        cw, cd = wgrad_case(M, cout, cin), dgrad_case(M, cout, cin)
        dyw, xw = cw["dy"].cuda(), cw["x"].cuda()
        dyd, wT = cd["dy"].cuda(), capi.pack_conv_weight_T(cd["wt"].reshape(cout, cin, 1, 1).cuda())
        ops = {"wgrad": (lambda: capi.linear_wgrad(dyw, xw, cout, cin), cw["ref_r"], cw["ref"]),
               "dgrad": (lambda: capi.linear_dgrad(dyd, wT, cin), cd["ref_r"], cd["ref_e"])}
        for name, (f, ref_r, ref_e) in ops.items():
            before = f().clone()
            with lin_grad_arithmetic(capi.LIN_GRAD_ARITH_BF16):
                got = f().clone()
            assert capi.get_lin_grad_arithmetic() == capi.LIN_GRAD_ARITH_DEFAULT
            after = f().clone()
            torch.cuda.synchronize()
            d_def, d_r, d_e = rel(got, before), rel(got, ref_r), rel(got, ref_e)
            print(f"LINGRAD | bf16 {name} {cout}x{cin}: rel-L2 to the default {d_def:.2e}, to fp64 of rounded operands {d_r:.2e}, to fp64 of the operands {d_e:.2e}")
            assert d_def > 1e-3, name                       # the rounding alone is 2.35e-3
            assert d_r < d_e, name
            assert torch.equal(before, after), name         # the default's bits, before and after a round trip through the mode
            assert rel(before, ref_e) <= 1e-4, name


# ---------------------------------------------------------------------------------------------------------------------
# whole models
# ---------------------------------------------------------------------------------------------------------------------
def _net(name, case, sd):
    M = importlib.import_module("lfsr_amd.model.SR." + name)
    net = M.get_model(Namespace(angRes_in=case["A"], angRes_out=case["A"], scale_factor=case["s"]))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.cuda().train()


def _step(net, xg, label):
    for p in net.parameters():
        p.grad = None
    out = net(xg)
    loss = F.l1_loss(out, label)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), float(loss.detach()), {k: p.grad.detach().cpu().double() for k, p in net.named_parameters()}, net.grad_bucket.clone()


@functools.lru_cache(maxsize=None)
def _port_refs(name, tag):
    """plain fp64 autograd of the stock graph, and its gradient under torch.autocast("cpu", bfloat16) (the reference's own reduced-precision path)"""
    case, sd, x, _ = TH.model_case(name, tag)
    return EMU.port_grads(name, case, sd, x, torch.float64), EMU.port_grads(name, case, sd, x, torch.float32, autocast=True)


@pytest.mark.parametrize("name,tag", [("EPIT", "a5h8s4"), ("EPIT", "a3h6w8s3"), ("LFT", "a5h8s4"), ("LFT", "a3h6w8s2")])
def test_transformer_whole_model(name, tag):
    case, sd, x, _ = TH.model_case(name, tag)
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    g64, gamp = _port_refs(name, tag)
    net = _net(name, case, sd)
    names = [k for k, _ in net.named_parameters()]
    assert set(names) == set(g64)
    xg = torch.from_numpy(x).cuda()
    label_np = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    label = torch.from_numpy(label_np).cuda()
    y_def, l_def, g_def, b_def = _step(net, xg, label)
    ws_bytes = net._rt.train_workspace_bytes(B, h, w)
    with lin_grad_arithmetic(capi.LIN_GRAD_ARITH_BF16):
        assert net._rt.train_workspace_bytes(B, h, w) == ws_bytes            # the workspace does not depend on the mode
        y, l, g, b = _step(net, xg, label)
        assert torch.equal(torch.cat([p.grad.reshape(-1) for p in net.parameters()]), net.grad_bucket)      # the bucket holds the .grads
        # fp64 autograd under the HIP forward's own decisions (read after this backward; the forward does not read the switch)
        forced_fn = {"EPIT": TH.epit_forced_fp64_grads, "LFT": TH.lft_forced_fp64_grads}[name]
        forced, flips = forced_fn(net._rt, xg, sd, x, label_np, A, s)
    assert torch.equal(y, y_def) and l == l_def                              # the forward does not read the switch
    assert not torch.equal(b, b_def) and bool(torch.isfinite(b).all())       # the mode is live
    flat = lambda d: torch.cat([torch.as_tensor(d[k]).double().reshape(-1) for k in names])
    e = {k: rel(g[k], forced[k]) for k in names}
    e_amp = {k: rel(gamp[k], g64[k]) for k in names}
    ratio = {k: e_amp[k] / max(e[k], 1e-30) for k in names}
    eb, eb_amp = rel(flat(g), flat(forced)), rel(flat(gamp), flat(g64))
    lin = [k for k in names if EMU.is_mode_linear(k)]
    other = [k for k in names if k not in lin]
    kl, ko = min(lin, key=ratio.get), min(other, key=ratio.get)
    print(f"LINGRAD | {name} {tag}: bucket rel-L2 {eb:.2e}, autocast {eb_amp:.2e} (ratio {eb_amp / eb:.2f}); {len(lin)} mode linears: smallest autocast / hip ratio "
          f"{ratio[kl]:.2f} ({kl}); {len(other)} other tensors: smallest ratio {ratio[ko]:.2f} ({ko}); decisions differing from fp64's own {flips}; "
          f"bucket distance to the default {rel(b, b_def):.2e}")
    for k in other:
        print(f"LINGRAD |   {name} {tag} {k}: hip {e[k]:.2e} autocast {e_amp[k]:.2e} ratio {ratio[k]:.2f}")
    assert eb <= eb_amp
    bad = {k: (e[k], e_amp[k]) for k in lin if not e[k] <= e_amp[k]}
    assert not bad, bad
    # the default is what it was
    _, _, _, b_again = _step(net, xg, label)
    assert torch.equal(b_again, b_def)


@pytest.mark.parametrize("name,tag", [("DistgSSR", "a3h6w8s2"), ("LF_InterNet", "a3h6w8s4")])
def test_the_other_drivers_do_not_read_the_switch(name, tag):
    case, sd, x, _ = TH.model_case(name, tag)
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    net = _net(name, case, sd)
    xg = torch.from_numpy(x).cuda()
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).cuda()
    b_def = _step(net, xg, label)[3]
    with lin_grad_arithmetic(capi.LIN_GRAD_ARITH_BF16):
        b = _step(net, xg, label)[3]
    assert bool(torch.isfinite(b).all()) and torch.equal(b, b_def)
