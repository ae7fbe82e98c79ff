"""GPU: lfsr_linear_wgrad and lfsr_conv3x3_wide_wgrad with exactly *_workspace_floats floats of workspace and a sentinel-filled guard behind it.

Both operators size their workspace through the weight-gradient dispatcher (csrc/wgrad.cpp: lfsr_wgrad_part_floats, the most any kernel of the form's chain needs in
any mode) and run the kernel it picks on that buffer; a kernel that writes more slabs than the size function counted writes into the guard.  Each case runs in the
default mode and in the operator's bf16 mode, with accumulate 0 and 1, and is compared with the fp64 gradient at the tolerances of the neighbouring tests of the
operator: tests/test_gpu_lin_grad_bf16.py (default: op_gate at 1e-4 against fp64 with the fp32 CPU yardstick; bf16: rel-L2 <= 1e-4 against fp64 of the rounded
operands) and tests/test_gpu_wide_train_bf16.py (rel-L2 <= 1e-4 against fp64 of the operands, rounded in the bf16 mode).

Already asserted in this form (exact workspace, guard, fp64, both modes, both accumulate values) by tests/test_gpu_lin_grad_bf16.py: the linear at M = 70001 for
(64, 64) and (256, 128).  They are not repeated; the linear rows here are M = 300.  tests/test_gpu_wide_train_bf16.py passes an exact workspace without a guard, so
every wide case is here."""
import pytest
import torch

from lfsr_amd import capi
from tests.helpers import op_gate
from tests.test_gpu_lin_grad_bf16 import rel, wgrad_case as linear_case
from tests.test_gpu_wide_train_bf16 import wgrad_case as wide_case

pytestmark = pytest.mark.gpu
SENTINEL = -12345.5
GUARD = 4096
P = capi.dev_ptr


def guarded(n):
    return torch.full((n + GUARD,), SENTINEL, device="cuda")


def intact(ws, n):
    torch.cuda.synchronize()
    return bool((ws[n:] == SENTINEL).all())


@pytest.fixture
def default_modes():
    yield
    capi.set_lin_grad_arithmetic(capi.LIN_GRAD_ARITH_DEFAULT)
    capi.set_wide_train_arithmetic(capi.WIDE_TRAIN_ARITH_DEFAULT)


@pytest.mark.parametrize("bf16", (0, 1), ids=("default", "bf16"))
@pytest.mark.parametrize("cout,cin", [(64, 64), (256, 128)], ids=str)
def test_linear_wgrad_at_exactly_its_workspace(cout, cin, bf16, default_modes):
    M = 300
    lib, st = capi.load(), capi.stream_ptr()
    c = linear_case(M, cout, cin)
    dy, x = c["dy"].cuda(), torch.cat([c["x"], torch.full((M, 4), 1e3)], 1).cuda()      # x in rows of cin + 4
    n_ws = lib.lfsr_linear_wgrad_workspace_floats(M, cout, cin)
    capi.set_lin_grad_arithmetic(capi.LIN_GRAD_ARITH_BF16 if bf16 else capi.LIN_GRAD_ARITH_DEFAULT)
    assert lib.lfsr_linear_wgrad_workspace_floats(M, cout, cin) == n_ws > 0              # the same in either mode
    for accumulate in (0, 1):
        ws = guarded(n_ws)
        dw = (c["dw0"] if accumulate else torch.full((cout, cin), SENTINEL)).cuda()
        assert lib.lfsr_linear_wgrad(P(dy), cout, P(x), cin + 4, P(dw), P(ws), n_ws - 1, M, cout, cin, accumulate, st) == -2      # LFSR_E_WS, nothing written
        capi.check(lib.lfsr_linear_wgrad(P(dy), cout, P(x), cin + 4, P(dw), P(ws), n_ws, M, cout, cin, accumulate, st), "linear_wgrad")
        assert intact(ws, n_ws), "floats behind the workspace written"
        add = c["dw0"] if accumulate else 0
        if bf16:
            e = rel(dw, c["ref_r"] + (c["dw0"].double() if accumulate else 0.0))
            print(f"WGRADWS | linear bf16 {cout}x{cin} M={M} accumulate={accumulate}: workspace {n_ws}, rel-L2 vs fp64(rounded operands) {e:.2e}")
            assert bool(torch.isfinite(dw).all()) and e <= 1e-4
        else:
            op_gate(dw, c["ref"] + add, c["cpu"] + add, "linear_wgrad", f"{cout}x{cin} accumulate={accumulate} workspace={n_ws}", f"M={M}", tag="WGRADWS")


@pytest.mark.parametrize("bf16", (0, 1), ids=("default", "bf16"))
@pytest.mark.parametrize("geom", [(2, 5, 33), (3, 4, 32)], ids=str)
@pytest.mark.parametrize("cin", [128, 320])
def test_conv3x3_wide_wgrad_at_exactly_its_workspace(cin, geom, bf16, default_modes):
    n_img, h, w = geom
    lib, st = capi.load(), capi.stream_ptr()
    x, dy, ref_rounded, ref_exact = wide_case(cin, n_img, h, w)
    ref = ref_rounded if bf16 else ref_exact
    xg, dyg = x.cuda(), dy.cuda()
    dw0 = torch.randn(64, cin, 3, 3, generator=torch.Generator().manual_seed(cin + h)) * float(ref.abs().mean())
    n_ws = lib.lfsr_conv3x3_wide_wgrad_workspace_floats(cin, n_img, h, w)
    capi.set_wide_train_arithmetic(capi.WIDE_TRAIN_ARITH_BF16_WGRAD if bf16 else capi.WIDE_TRAIN_ARITH_DEFAULT)
    assert lib.lfsr_conv3x3_wide_wgrad_workspace_floats(cin, n_img, h, w) == n_ws > 0
    for accumulate in (0, 1):
        ws = guarded(n_ws)
        dw = (dw0 if accumulate else torch.full((64, cin, 3, 3), SENTINEL)).cuda()
        assert lib.lfsr_conv3x3_wide_wgrad(P(dyg), 64, 0, P(xg), cin, 0, cin, P(dw), P(ws), n_ws - 1, n_img, h, w, accumulate, st) == -2
        capi.check(lib.lfsr_conv3x3_wide_wgrad(P(dyg), 64, 0, P(xg), cin, 0, cin, P(dw), P(ws), n_ws, n_img, h, w, accumulate, st), "conv3x3_wide_wgrad")
        assert intact(ws, n_ws), "floats behind the workspace written"
        e = rel(dw, ref + (dw0.double() if accumulate else 0.0))
        print(f"WGRADWS | wide {'bf16' if bf16 else 'default'} cin {cin} {geom} accumulate={accumulate}: workspace {n_ws}, rel-L2 vs fp64 {e:.2e}")
        assert bool(torch.isfinite(dw).all()) and e <= 1e-4
