"""GPU: the nine process-wide arithmetic switches on the four trainable models (EPIT, LFT, LF_InterNet, DistgSSR) across geometry rows, alone and together,
forward and one training step, against the fp64 stock graph.

Every gate is either the project's 0.01 dB or the error of the stock graph itself under torch.autocast("cpu", bfloat16) at margin 1.0 (tests/modes_refs.py
computes both legs once per row); no figure comes from the HIP code.  The rows (tests/modes_refs.py:ROWS) reach what the per-switch whole-model tests, at one or
two 8x8 golden geometries with one switch on, do not: even and extreme angRes, scale 3, ragged views, a batch boundary, lines of 33 pixels (one past what the
EPI-line and block-tail kernels cover: the driver has to hand over to the fp32 kernels) and LF_InterNet's first row past the 2048-row threshold of the row GEMMs.

reach() below states which switch changes what at which row, read from the launchers' and the drivers' coverage conditions (cited beside each entry).  It is asserted in both
directions: reached means the bits differ from the default's, not reached means bit-equal.

Measured figures: profiles/modes_geometry_tests.md (every line this file prints starts with `MODESGEO |`)."""
import importlib
import time
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lfsr_amd import capi
from tests import helpers as TH
from tests import modes_refs as R

pytestmark = pytest.mark.gpu
ATOL = 1e-4
ids = lambda c: "%s-A%ds%dB%dh%dw%d" % ((c[0],) + tuple(c[1]))
CASES = [(m, g) for m in R.MODELS for g in R.ROWS[m]]
TRAIN_CASES = [c for c in CASES if R.has_backward(*c)]

# switch -> its reduced-precision value
ON = {"arith": capi.ARITH_BF16, "grad": capi.GRAD_ARITH_BF16, "gemm": capi.GEMM_ARITH_BF16, "branch": capi.BRANCH_ARITH_BF16, "ang": capi.ANG_ARITH_BF16,
      "wide": capi.WIDE_ARITH_BF16, "lin_grad": capi.LIN_GRAD_ARITH_BF16, "wide_train": capi.WIDE_TRAIN_ARITH_BF16, "branch_grad": capi.BRANCH_GRAD_ARITH_BF16}
FORWARD_SWITCHES = ("arith", "gemm", "branch", "wide", "ang")
LEG_G = {"grad": capi.GRAD_ARITH_BF16, "lin_grad": capi.LIN_GRAD_ARITH_BF16, "branch_grad": capi.BRANCH_GRAD_ARITH_BF16,
         "wide_train": capi.WIDE_TRAIN_ARITH_BF16_WGRAD}
assert set(ON) == set(TH.MODE_SWITCHES)

# (model, (A, s, B, h, w), parameter) -> the measured autocast / HIP ratio of a per-parameter gate of leg G that is waived because the CPU emulation of the same
# switches (tests/modes_refs.py:emulation) misses the same inequality there; test_training_step checks that condition, the 5 % cap and the row's worst autocast
# error every time.  The bucket gates admit no waiver.
WAIVED = {}


def reach(model, geom, train):
    """the switches that change the no-grad forward (train=False) or the bucket of a training step (train=True) of `model` at `geom`; csrc/ file:line of the
    condition beside each"""
    A, s, B, h, w = geom
    transformer = model in ("EPIT", "LFT")
    out = set()
    # ARITH_BF16: the 64 -> 64 per-view 3x3 forward conv, conv3x3.cpp:51 (the dispatcher of lfsr_conv3x3_fwd; its bf16 launcher declines no geometry,
    # conv3x3_bf16_kernel.h:242-264).  DistgSSR's forward and training forward (distgssr.cpp:276, 438), EPIT's and LFT's convs; LF_InterNet has no such conv
    # (internet.hip:195-224, internet_train.hip:340-359: wide convs, gather-GEMMs and linears only)
    if transformer or model == "DistgSSR":
        out.add("arith")
    # GEMM_ARITH_BF16: the LN-linears and feed-forward blocks of EPIT / LFT at every row count (rowgemm.cpp:41, 53: no threshold); a plain linear only from 2048 rows
    # (rowgemm.cpp:26) with K in {64, 128} and no bias (rowgemm.cpp:28-29): LF_InterNet's 128 -> 64 AngConvSq over B h w rows (internet.hip:210,
    # internet_train.hip:347-348); DistgSSR's fuse.0 has K = 144 and keeps the default (rowgemm.cpp:29)
    if transformer or (model == "LF_InterNet" and B * h * w >= 2048):
        out.add("gemm")
    # BRANCH_ARITH_BF16: the two launches of the fused block tail (lfsr_distg_epi1_run / _tail2_run, distg_branch.cpp), which only the inference forward takes (the
    # training forward keeps the three-kernel sequence) and only where its tail_ok holds (LFSR_ROWGEMM_MIN_ROWS = 2048 view pixels or more, and
    # lfsr_distg_tail_covers: A = 5, h <= 32, w <= 32).  At lines of 33 the driver runs the unfused fp32 branches and the switch reaches nothing
    # (the launchers of distg_bf16.hip have bounds of their own; lfsr_distg_tail_covers, which lfsr_distg_branch_tail_fwd checks too, is narrower than both, so neither
    # launcher is ever asked for a view it declines)
    if model == "DistgSSR" and not train and A == 5 and h <= 32 and w <= 32 and B * A * A * h * w >= 2048:
        out.add("branch")
    # WIDE_ARITH_BF16: lfsr_conv3x3_wide_run (internet.hip:88), the inference forward's SpaConvSq and SpaBottle (internet.hip:211, 222); the training forward reads
    # the wide-train switch instead (internet_train.hip:333-335)
    if model == "LF_InterNet" and not train:
        out.add("wide")
    # ANG_ARITH_BF16: lfsr_angconv3x3_fwd alone (ang3x3.hip:121), LFSSR's operator: none of the four
    if train:
        # GRAD_ARITH_BF16: the 3x3 data gradient (conv3x3.cpp:53) of all four backwards (trans_bwd.hip:541, internet_train.hip:394-395, DistgSSR's conv backward) and
        # the 64 -> 64 weight gradient (the CONV3 chain of wgrad.cpp)
        out.add("grad")
        # LIN_GRAD_ARITH_BF16: dgemm_launch (trans_bwd.hip) and the LINEAR form of lfsr_wgrad_run (wgrad.cpp) of the shared transformer backward: EPIT and LFT
        if transformer:
            out.add("lin_grad")
        # BRANCH_GRAD_ARITH_BF16: EPIConv.0's EPI-line gradients at A = 5: the data gradient per pass with lines of at most 32 pixels (bwd_ops.hip:272-274,
        # branch_bwd.cpp:107; epi0_grad_bf16.hip:279), the merged weight gradient with both sides at most 32 (branch_bwd.cpp:120, wgrad.hip:765-767;
        # epi0_grad_bf16.hip:267)
        if model == "DistgSSR" and A == 5 and min(h, w) <= 32:
            out.add("branch_grad")
        # WIDE_TRAIN_ARITH_BF16(_WGRAD): the seventeen wide weight gradients (internet_train.hip:218) and, at 2, forward_train's wide convs (internet_train.hip:333)
        if model == "LF_InterNet":
            out.add("wide_train")
    return out


def make_net(model, geom, sd):
    A, s = geom[0], geom[1]
    M = importlib.import_module("lfsr_amd.model.SR." + model)
    net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.cuda().train()


def step(net, xg, label):
    """one forward + L1 + backward through the plugin -> (output, loss, {name: .grad}, bucket)"""
    for p in net.parameters():
        p.grad = None
    out = net(xg)
    loss = F.l1_loss(out, label)
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().clone(), float(loss.detach()), {k: p.grad.detach().cpu().double().numpy() for k, p in net.named_parameters()}, net.grad_bucket.clone()


def forced_grads(model, net, xg, ref, geom):
    """fp64 autograd of the stock graph under the decisions the HIP forward took (read from the training workspace after a step of xg) -> ({name: gradient}, flips)"""
    A, s = geom[0], geom[1]
    sd, x, label = ref["sd"], ref["x"], ref["label"]
    if model == "EPIT":
        return TH.epit_forced_fp64_grads(net._rt, xg, sd, x, label, A, s)
    if model == "LFT":
        return TH.lft_forced_fp64_grads(net._rt, xg, sd, x, label, A, s)
    if model == "DistgSSR":
        return TH.distg_forced_fp64_grads(net._rt, xg, sd, x, label, A, s)
    net(xg)        # LF_InterNet: the saved activations of this input again (the backward reuses some of them)
    return TH.forced_fp64_grads(net._rt, xg, sd, x, label, A, s)


def test_the_rows_are_the_ones_the_gates_were_written_for():
    """the arithmetic the row comments and the reach table rely on, so that a row cannot silently stop covering its boundary"""
    assert (2, 2, 2, 32, 33) in R.ROWS["LF_InterNet"] and 2 * 32 * 33 == 2112 == 2048 + 64 and 2112 // 2 < 2048      # ragged against 2048 and against the batch boundary
    assert [g for g in R.ROWS["LF_InterNet"] if g[2] * g[3] * g[4] >= 2048] == [(2, 2, 2, 32, 33)]
    assert len(R.ROWS["EPIT"]) == len(TH.EPIT_MATRIX) - 1 and len(R.ROWS["LFT"]) == len(TH.LFT_MATRIX) - 1
    dist = R.ROWS["DistgSSR"]
    assert [g for g in dist if "branch" in reach("DistgSSR", g, False)] == [(5, 3, 2, 13, 16)]
    assert [g for g in dist if R.has_backward("DistgSSR", g) and "branch_grad" in reach("DistgSSR", g, True)] == [(5, 3, 2, 13, 16), (5, 2, 1, 33, 6), (5, 4, 1, 6, 33)]
    assert [g for g in dist if not R.has_backward("DistgSSR", g)] == [(2, 3, 2, 9, 7)]
    for m, g in CASES:
        assert "ang" not in reach(m, g, False) | reach(m, g, True)


# ---------------------------------------------------------------------------------------------------------------------
# the no-grad forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_forward(case):
    model, geom = case
    ref = R.refs(model, geom)
    y64, e_amp = ref["y64"], ref["e_amp_out"]
    label = torch.rand(y64.shape, generator=torch.Generator().manual_seed(2)).numpy()
    net = make_net(model, geom, ref["sd"])
    xg = torch.from_numpy(ref["x"]).cuda()

    def forward():
        with torch.no_grad():
            y = net(xg)
        torch.cuda.synchronize()
        return y.clone()

    t0 = time.time()
    yd = forward()
    y_def = yd.cpu().numpy()
    assert y_def.shape == y64.shape and np.abs(y_def - y64).max() <= ATOL * max(1.0, np.abs(y64).max())      # the default is what it was
    assert np.isfinite(e_amp) and e_amp > 0
    live = reach(model, geom, False)
    assert live <= set(FORWARD_SWITCHES)
    combos = [(k,) for k in FORWARD_SWITCHES if k in live] + [FORWARD_SWITCHES]
    fails = []
    for combo in combos:
        with TH.modes(**{k: ON[k] for k in combo}):
            y = forward()
        yn = y.cpu().numpy()
        dpsnr = TH.psnr(yn, label) - TH.psnr(y64, label)
        e = R.rms(yn, y64)
        print(f"MODESGEO | {model} | {geom} | fwd | {'+'.join(combo)} | rms {e:.3e} | autocast {e_amp:.3e} | ratio {e_amp / max(e, 1e-300):.2f} | "
              f"max {np.abs(yn - y64).max():.3e} | dPSNR {dpsnr:+.5f} | default rms {R.rms(y_def, y64):.3e}")
        if not (np.isfinite(yn).all() and abs(dpsnr) <= 0.01):            # (a) the project's gate
            fails.append((combo, "dPSNR", dpsnr))
        if not e <= e_amp:                                                   # (b) not worse than the stock graph's own reduced-precision path
            fails.append((combo, "rms", e, e_amp))
        if torch.equal(y, yd) != (not (set(combo) & live)):                  # (c) live where the table says so
            fails.append((combo, "equal to the default" if set(combo) & live else "differs from the default"))
    # the other direction of the table: a switch that does not reach this forward changes no bit
    for k in ON:
        if k not in live:
            with TH.modes(**{k: ON[k]}):
                if not torch.equal(forward(), yd):
                    fails.append((k, "not in the reach table, yet the output moved"))
    # LFSR_ARITH_F32 wins over every other forward switch
    with TH.modes(arith=capi.ARITH_F32):
        y_f32 = forward()
    with TH.modes(arith=capi.ARITH_F32, **{k: ON[k] for k in FORWARD_SWITCHES if k != "arith"}):
        if not torch.equal(forward(), y_f32):
            fails.append(("ARITH_F32 with the other forward switches differs from ARITH_F32 alone",))
    assert all(v == 0 for v in TH.modes_now().values())
    if not torch.equal(forward(), yd):
        fails.append(("the default's bits did not come back",))
    print(f"MODESGEO | {model} | {geom} | fwd | live {sorted(live)} | wall {time.time() - t0:.1f} s | reference legs {ref['seconds']:.1f} s")
    assert not fails, fails


# ---------------------------------------------------------------------------------------------------------------------
# one training step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", TRAIN_CASES, ids=ids)
def test_training_step(case):
    model, geom = case
    A, s, B, h, w = geom
    ref = R.refs(model, geom)
    names, g64, e_amp, eb_amp = ref["names"], ref["g64"], ref["e_amp"], ref["e_amp_bucket"]
    net = make_net(model, geom, ref["sd"])
    assert [k for k, _ in net.named_parameters()] == names
    xg, label = torch.from_numpy(ref["x"]).cuda(), torch.from_numpy(ref["label"]).cuda()
    t0 = time.time()
    y0, l0, _, b0 = step(net, xg, label)
    ws0 = net._rt.train_workspace_bytes(B, h, w)
    assert ws0 > 0 and bool(torch.isfinite(b0).all()) and np.isfinite(eb_amp) and eb_amp > 0
    live = reach(model, geom, True)
    fails = []

    # ---- the reach table, both directions, one switch at a time
    for k in ON:
        with TH.modes(**{k: ON[k]}):
            y, _, _, b = step(net, xg, label)
            if net._rt.train_workspace_bytes(B, h, w) != ws0:
                fails.append((k, "the training workspace depends on the switch"))
        same = torch.equal(b, b0) and torch.equal(y, y0)
        if same != (k not in live):
            fails.append((k, "in the reach table, yet no bit moved" if k in live else "not in the reach table, yet the step moved"))

    # ---- leg G: the gradient switches only
    with TH.modes(**LEG_G):
        yG, lG, gG, bG = step(net, xg, label)
        assert torch.equal(torch.cat([p.grad.reshape(-1) for p in net.parameters()]), net.grad_bucket)      # the bucket holds the .grads
        assert net._rt.train_workspace_bytes(B, h, w) == ws0
        tf = time.time()
        forced, flips = forced_grads(model, net, xg, ref, geom)      # (the forward does not read these switches: its decisions are the default's)
        t_forced = time.time() - tf
    assert torch.equal(yG, y0) and lG == l0                          # the forward does not read the gradient switches
    assert bool(torch.isfinite(bG).all())
    assert not torch.equal(bG, b0)                                   # GRAD reaches every backward
    e = {k: TH.rel_l2(gG[k], forced[k]) for k in names}
    ebG = TH.rel_l2(R.flat(gG, names), R.flat(forced, names))
    ratio = {k: (e_amp[k] / e[k] if e[k] > 0 else float("inf")) for k in names}
    kmin = min(ratio, key=ratio.get)
    v = np.array(list(e.values()))
    print(f"MODESGEO | {model} | {geom} | legG | bucket {ebG:.3e} | autocast {eb_amp:.3e} | ratio {eb_amp / ebG:.2f} | per-parameter median {np.median(v):.3e} max {v.max():.3e} | "
          f"autocast median {np.median(list(e_amp.values())):.3e} max {max(e_amp.values()):.3e} | smallest ratio {ratio[kmin]:.2f} ({kmin}) | flips {flips} | "
          f"forced fp64 {t_forced:.1f} s")
    if not ebG <= eb_amp:                                            # the bucket gate admits no waiver
        fails.append(("leg G bucket", ebG, eb_amp))
    over = {k: (e[k], e_amp[k]) for k in names if not e[k] <= e_amp[k]}
    waived = [k for k in over if (model, geom, k) in WAIVED]
    if waived:
        e_emul, _, _ = R.emulation(model, geom)
        assert len(waived) <= 0.05 * len(names), waived
        for k in waived:
            print(f"MODESGEO | {model} | {geom} | legG | waived {k} | hip {e[k]:.3e} | autocast {e_amp[k]:.3e} | emulation {e_emul[k]:.3e}")
            assert e_emul[k] > e_amp[k], (k, "the emulation meets the gate: no waiver")
            assert e[k] <= max(e_amp.values()), (k, e[k])
    over = {k: v_ for k, v_ in over.items() if k not in waived}
    if over:
        fails.append(("leg G parameters", over))

    # ---- leg A: every switch at once, forward ones included
    with TH.modes(**ON):
        yA, lA, gA, bA = step(net, xg, label)
        assert net._rt.train_workspace_bytes(B, h, w) == ws0
    ebA = TH.rel_l2(R.flat(gA, names), R.flat(g64, names))
    print(f"MODESGEO | {model} | {geom} | legA | bucket {ebA:.3e} | autocast {eb_amp:.3e} | ratio {eb_amp / ebA:.2f} | output rms vs fp64 {R.rms(yA.cpu().numpy(), ref['y64']):.3e} | "
          f"autocast {ref['e_amp_out']:.3e}")
    if not (bool(torch.isfinite(bA).all()) and bool(torch.isfinite(yA).all()) and np.isfinite(lA)):
        fails.append(("leg A is not finite",))
    if not ebA <= eb_amp:
        fails.append(("leg A bucket", ebA, eb_amp))

    # ---- the default is what it was
    assert all(v_ == 0 for v_ in TH.modes_now().values())
    y1, l1, _, b1 = step(net, xg, label)
    if not (torch.equal(y1, y0) and torch.equal(b1, b0) and l1 == l0):
        fails.append(("the default step's bits did not come back",))
    print(f"MODESGEO | {model} | {geom} | train | live {sorted(live)} | wall {time.time() - t0:.1f} s | reference legs {ref['seconds']:.1f} s")
    assert not fails, fails


def test_even_angres_distgssr_has_no_backward():
    """the forward-only row stays forward-only under every switch: the training forward runs, the backward refuses"""
    model, geom = "DistgSSR", (2, 3, 2, 9, 7)
    assert (model, geom) in CASES and (model, geom) not in TRAIN_CASES
    ref = R.refs(model, geom)
    net = make_net(model, geom, ref["sd"])
    xg, label = torch.from_numpy(ref["x"]).cuda(), torch.from_numpy(ref["label"]).cuda()
    for kw in ({}, ON):
        with TH.modes(**kw):
            loss = F.l1_loss(net(xg), label)
            with pytest.raises(capi.LfsrError):
                loss.backward()
            torch.cuda.synchronize()
