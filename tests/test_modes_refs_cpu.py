"""No GPU: the reference legs and the emulation of tests/test_gpu_modes_geometries.py (tests/modes_refs.py), and helpers.modes.

  * at the golden tags the generalised legs are, bit for bit, what the per-switch tests compute there (lin_grad_emulation.port_grads, wide_train_emulation.step_grads,
    test_gpu_grad_bf16._distg_refs);
  * the autocast yardsticks are finite and non-zero on every row, so that no gate of the GPU test is vacuous; where a parameter's fp64 gradient is exactly zero (LFT
    at angRes 1: a softmax over one key is constant, so nothing reaches the angular LayerNorm) autocast's is exactly zero too and the gate asks for exact zeros;
  * the emulation of the gradient switches, on the rows under 3000 view pixels, patches the operators it claims to, is transparent with the rounding taken out, and
    meets every gate the GPU test applies to leg G -- the flat bucket and each parameter: the gates are ones the arithmetic can meet, and the waiver table of the GPU
    test has no entry to justify;
  * the per-parameter gate has teeth where the gate it backs had none: a LeakyReLU' mask lost in one layer's bf16 data gradient, planted in the emulation, stays ten
    times inside 5e-2 of the bucket and is outside some parameter's own autocast error every time."""
import numpy as np
import pytest
import torch

from lfsr_amd import capi
from tests import helpers as TH
from tests import lin_grad_emulation as LG
from tests import modes_refs as R
from tests import wide_train_emulation as WT

torch.set_num_threads(min(torch.get_num_threads(), 16))
CASES = [(m, g) for m in R.MODELS for g in R.ROWS[m]]
SMALL = [c for c in CASES if R.view_pixels(c[1]) < R.EMULATION_MAX_VIEW_PIXELS]
ids = lambda c: "%s-A%ds%dB%dh%dw%d" % ((c[0],) + tuple(c[1]))
# the parameters whose gradient is exactly zero in fp64: (model, row) -> name suffixes
ZERO_GRADS = {("LFT", (1, 2, 2, 8, 8)): ("ang_trans.norm.weight", "ang_trans.norm.bias")}
TAGS = [("EPIT", "a5h8s4"), ("EPIT", "a3h6w8s3"), ("LFT", "a5h8s4"), ("LFT", "a3h6w8s2"), ("LF_InterNet", "a5h8s2"), ("LF_InterNet", "a3h6w8s4")]


def test_modes_sets_and_restores_all_nine():
    assert len(TH.MODE_SWITCHES) == 9
    on = {"arith": capi.ARITH_BF16, "grad": capi.GRAD_ARITH_BF16, "gemm": capi.GEMM_ARITH_BF16, "branch": capi.BRANCH_ARITH_BF16, "ang": capi.ANG_ARITH_BF16,
          "wide": capi.WIDE_ARITH_BF16, "lin_grad": capi.LIN_GRAD_ARITH_BF16, "wide_train": capi.WIDE_TRAIN_ARITH_BF16, "branch_grad": capi.BRANCH_GRAD_ARITH_BF16}
    assert set(on) == set(TH.MODE_SWITCHES) and all(v != 0 for v in on.values())
    zero = dict.fromkeys(on, 0)
    assert TH.modes_now() == zero
    with TH.modes(**on):
        assert TH.modes_now() == on
        with TH.modes(gemm=capi.GEMM_ARITH_BF16):           # a nested block states the whole selection
            assert TH.modes_now() == {**zero, "gemm": capi.GEMM_ARITH_BF16}
        assert TH.modes_now() == zero
    for k, v in on.items():
        with TH.modes(**{k: v}):
            assert TH.modes_now() == {**zero, k: v}
        assert TH.modes_now() == zero
    with pytest.raises(RuntimeError):
        with TH.modes(wide_train=capi.WIDE_TRAIN_ARITH_BF16_WGRAD, arith=capi.ARITH_F32):
            assert TH.modes_now() == {**zero, "wide_train": 1, "arith": 1}
            capi.set_ang_arithmetic(capi.ANG_ARITH_BF16)    # set behind its back: restored as well
            raise RuntimeError("out")
    assert TH.modes_now() == zero
    with pytest.raises(AssertionError):
        with TH.modes(angular=1):
            pass
    assert TH.modes_now() == zero


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("name,tag", TAGS)
def test_legs_at_the_golden_tags_are_the_per_switch_tests_own(name, tag):
    c, sd, x, _ = TH.model_case(name, tag)
    geom = (c["A"], c["s"], c["B"], c["h"], c["w"])
    ref = R.refs(name, geom)
    _same(ref["sd"], sd)
    assert np.array_equal(ref["x"], x)
    if name == "LF_InterNet":
        y64, g64 = WT.step_grads(sd, x, ref["label"], geom[0], geom[1])
        y_amp, g_amp = WT.step_grads(sd, x, ref["label"], geom[0], geom[1], dtype=torch.float32, autocast=True)
        assert np.array_equal(ref["y64"], y64.double().numpy()) and np.array_equal(ref["y_amp"], y_amp.double().numpy())
    else:
        g64 = {k: v.numpy() for k, v in LG.port_grads(name, c, sd, x, torch.float64).items()}
        g_amp = {k: v.numpy() for k, v in LG.port_grads(name, c, sd, x, torch.float32, autocast=True).items()}
    _same(ref["g64"], g64)
    _same(ref["g_amp"], g_amp)


@pytest.mark.parametrize("geom", [(5, 2, 1, 8, 8), (3, 2, 2, 6, 8)])
def test_distgssr_legs_at_the_whole_model_geometries(geom):
    from tests.test_gpu_grad_bf16 import _distg_refs
    sd, x, label, g64, g_amp = _distg_refs(*geom)
    ref = R.refs("DistgSSR", geom)
    _same(ref["sd"], sd)
    assert np.array_equal(ref["x"], x) and np.array_equal(ref["label"], label)
    _same(ref["g64"], g64)
    _same(ref["g_amp"], g_amp)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_yardsticks_are_finite_and_non_zero(case):
    model, geom = case
    ref = R.refs(model, geom)
    assert np.isfinite(ref["y64"]).all() and np.isfinite(ref["y_amp"]).all()
    assert np.isfinite(ref["e_amp_out"]) and ref["e_amp_out"] > 0
    assert np.isfinite(ref["e_amp_bucket"]) and ref["e_amp_bucket"] > 0
    zero = [k for k in ref["names"] if not np.any(ref["g64"][k])]
    assert zero == [k for k in ref["names"] if k.endswith(ZERO_GRADS.get(case, ("\0",)))], zero
    for k in ref["names"]:
        assert np.isfinite(ref["g64"][k]).all() and np.isfinite(ref["g_amp"][k]).all(), k
        if k in zero:
            assert not np.any(ref["g_amp"][k]) and ref["e_amp"][k] == 0, k       # the gate there: exact zeros (helpers.rel_l2)
        else:
            assert np.isfinite(ref["e_amp"][k]) and ref["e_amp"][k] > 0, k
    print(f"MODESREF | {model} | {geom} | output rms {ref['e_amp_out']:.3e} | bucket {ref['e_amp_bucket']:.3e} | per-parameter min "
          f"{min(v for k, v in ref['e_amp'].items() if k not in zero):.3e} max {max(ref['e_amp'].values()):.3e} | zero gradients {len(zero)} | {ref['seconds']:.1f} s")


def test_conv64_backward_is_the_gradient_of_the_rounded_operands():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 64, 1, 5, 7, generator=g, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(64, 64, 1, 3, 3, generator=g, dtype=torch.float64) * 0.05).requires_grad_(True)
    dy = torch.randn(2, 64, 1, 5, 7, generator=g, dtype=torch.float64)
    seen = []
    with R.emulate_conv64({"w": w}, R.r_bf16, seen):
        y = torch.nn.functional.conv3d(x, w, padding=(0, 1, 1))
    assert seen == ["w"] and torch.equal(y, torch.nn.functional.conv3d(x, w, padding=(0, 1, 1)))
    y.backward(dy)
    xr, wr = R.r_bf16(x.detach()).requires_grad_(True), R.r_bf16(w.detach()).requires_grad_(True)
    torch.nn.functional.conv3d(xr, wr, padding=(0, 1, 1)).backward(R.r_bf16(dy))
    assert torch.allclose(x.grad, xr.grad, rtol=0, atol=1e-12) and torch.allclose(w.grad, wr.grad, rtol=0, atol=1e-12)
    assert not torch.allclose(x.grad, torch.nn.grad.conv3d_input(x.shape, w.detach(), dy, padding=(0, 1, 1)), rtol=0, atol=1e-6)      # the rounding is there


@pytest.mark.parametrize("case", SMALL, ids=ids)
def test_emulation_of_the_gradient_switches(case):
    model, geom = case
    ref = R.refs(model, geom)
    names, e_amp = ref["names"], ref["e_amp"]
    e, seen, eb = R.emulation(model, geom)
    # it patched what it claims to
    conv64 = [k for k in names if R.is_conv64(ref["sd"][k].shape)]
    want = set(conv64)
    if model in ("EPIT", "LFT"):
        want |= {k for k in names if LG.is_mode_linear(k)}
    if model == "LF_InterNet":
        want |= set(WT.WIDE_KEYS)
    assert set(seen) == want and len(want) > 0, (sorted(want - set(seen)), sorted(set(seen) - want))     # (no row this small has A = 5: EPIConv.0 stays stock)
    assert geom[0] != 5 or model != "DistgSSR"
    # with the rounding taken out it is the plain graph
    _, g_id = R.step_grads(model, geom, ref["sd"], ref["x"], ref["label"], r=lambda t: t)
    assert max(R.rel_l2(g_id[k], ref["g64"][k]) for k in names) <= 1e-12
    # and with it, it is live and inside every gate of leg G
    ratio = {k: e_amp[k] / e[k] for k in names if e[k] > 0}
    kmin = min(ratio, key=ratio.get)
    print(f"MODESREF | {model} | {geom} | emulation of leg G | bucket {eb:.3e} | autocast {ref['e_amp_bucket']:.3e} | ratio {ref['e_amp_bucket'] / eb:.2f} | "
          f"per-parameter max {max(e.values()):.3e} | smallest autocast / emulation ratio {ratio[kmin]:.2f} ({kmin})")
    assert 0 < eb <= ref["e_amp_bucket"]
    over = {k: (e[k], e_amp[k]) for k in names if not e[k] <= e_amp[k]}
    assert not over, over


# (model, row, (conv, the slope of the LeakyReLU it reads, which use of the conv)): a shared AltFilter conv in its vertical pass, the second conv of LFT's head, a
# SpaConv.2 and the last fuse.2
FAULTS = [("EPIT", (2, 3, 2, 9, 7), ("altblock.2.conv.2.weight", 0.2, 1)), ("LFT", (2, 3, 2, 9, 7), ("conv_init.2.weight", 0.2, 0)),
          ("DistgSSR", (1, 3, 2, 9, 7), ("disentg.Group.2.Block.1.SpaConv.2.weight", 0.1, 0)), ("DistgSSR", (3, 3, 1, 13, 16), ("disentg.Group.3.Block.3.fuse.2.weight", 0.1, 0))]


@pytest.mark.parametrize("model,geom,fault", FAULTS, ids=lambda v: v if isinstance(v, str) else None)
def test_a_lost_mask_in_one_layer_passes_the_old_gate_and_fails_the_per_parameter_one(model, geom, fault):
    """the case the per-parameter gate of leg G exists for, planted in the emulation: ONE 3x3 data gradient on the bf16 path loses the LeakyReLU' mask in every fourth
    channel.  The bucket stays within 5e-2 of the unbroken one (the gate LFSR_GRAD_ARITH_BF16 had on EPIT, LFT and LF_InterNet) and, in three of the four cases, inside
    autocast's bucket error as well; some parameter is outside its own autocast error every time"""
    ref = R.refs(model, geom)
    names = ref["names"]
    assert ref["sd"][fault[0]].shape[:2] == (64, 64)
    g_ok = R.step_grads(model, geom, ref["sd"], ref["x"], ref["label"], r=R.r_bf16)[1]
    g_bad = R.step_grads(model, geom, ref["sd"], ref["x"], ref["label"], r=R.r_bf16, fault=fault)[1]
    d = R.rel_l2(R.flat(g_bad, names), R.flat(g_ok, names))
    eb = R.rel_l2(R.flat(g_bad, names), R.flat(ref["g64"], names))
    over = [k for k in names if not R.rel_l2(g_bad[k], ref["g64"][k]) <= ref["e_amp"][k]]
    print(f"MODESREF | {model} | {geom} | lost mask in {fault[0]} | bucket distance to the unbroken emulation {d:.3e} | bucket vs fp64 {eb:.3e} | autocast "
          f"{ref['e_amp_bucket']:.3e} | parameters outside their gate {len(over)} of {len(names)}")
    assert 0 < d <= 5e-2
    assert over
