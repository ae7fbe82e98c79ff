"""GPU: the fused DistgSSR block tail at the shapes where its load pipeline can go wrong (distg_tail.hip requests a tile's first rows before the weight
staging, a view's rows one body ahead, a t_H row through an out-of-range offset on the views that want none, and the next tile's first rows during the last view).

capi.distg_branch_tail against the three-call sequence it replaces, bit for bit, with y and the t buffers placed inside larger allocations filled with a
sentinel: nothing outside the operator's own rows may be written."""
import pytest
import torch

from lfsr_amd import capi

pytestmark = pytest.mark.gpu
A, L = 5, 0.1
GUARD = 4096            # floats in front of and behind every output
SENTINEL = -12345.5
ROWGEMM_MIN = 2048      # rows from which lfsr_pointwise_fwd takes the bf16 row-GEMM


def _weights(seed):
    g = torch.Generator().manual_seed(seed)
    def rnd(*shape, fan):
        return ((torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * (1.0 / fan) ** 0.5).float().cuda()
    return (capi.pack_conv_weight(rnd(16, 64, A, A, fan=64 * 25)), capi.pack_conv_weight(rnd(16 * A * A, 16, 1, 1, fan=16), perm=1, ch=16),
            capi.pack_conv_weight(rnd(32, 64, 1, A * A, fan=64 * 25)), capi.pack_conv_weight(rnd(32 * A, 32, 1, 1, fan=32)),
            capi.pack_conv_weight(rnd(64, 144, 1, 1, fan=144)))


def _old_sequence(x, spa, wp, B, h, w):
    """the operator sequence the tail replaces: the branches into a (npix, 144) concat, then the pointwise fuse.0.  Below ROWGEMM_MIN rows lfsr_pointwise_fwd
    runs the fp32 gather-GEMM and not the three-term bf16 row-GEMM whose arithmetic the tail reproduces, so a smaller concat is followed by zero rows up to that
    count (a row's result depends on that row alone) and the first npix rows of the result are the reference."""
    npix = x.shape[0]
    cat = torch.zeros((max(npix, ROWGEMM_MIN), 144), dtype=torch.float32, device=x.device)
    cat[:npix, :64] = spa
    tmp = torch.empty((B * h * w, 16), dtype=torch.float32, device=x.device)
    capi.angconv(x, wp[0], wp[1], B, A, h, w, L, cat[:npix], 64, tmp=tmp)
    capi.epiconv_hv(x, wp[2], wp[3], B, A, h, w, L, cat[:npix], 80, 112)
    return capi.pointwise(cat, 144, wp[4], 64, slope=L)[:npix], tmp


def _guarded(rows, cols):
    """a (rows, cols) tensor in the middle of a sentinel-filled allocation; 16-byte aligned like a fresh one"""
    pool = torch.full((2 * GUARD + rows * cols,), SENTINEL, dtype=torch.float32, device="cuda")
    return pool, pool[GUARD:GUARD + rows * cols].view(rows, cols)


# (40, 32, 32): 2560 tiles on 2048 waves, some waves own two tiles (the hand-over between tiles); (2, 8, 8): 8 tiles, most waves of a block own none (their
# prologue loads must be harmless); (1, 5, 3): 15 macro-pixels, one ragged tile with absent rows in every load and store; (3, 9, 7): tiles that straddle patches
@pytest.mark.parametrize("B,h,w", [(40, 32, 32), (2, 8, 8), (1, 5, 3), (3, 9, 7)])
def test_tail_equals_the_three_call_sequence_and_writes_only_its_rows(B, h, w):
    torch.manual_seed(B * 1000 + h * 10 + w)
    npix = B * A * A * h * w
    x = torch.randn((npix, 64), dtype=torch.float32, device="cuda")
    spa = torch.nn.functional.leaky_relu(torch.randn((npix, 64), dtype=torch.float32, device="cuda"), L)
    wp = _weights(11 + B)
    y_old, ta_old = _old_sequence(x, spa, wp, B, h, w)
    pools, outs = zip(*[_guarded(r, c) for r, c in ((npix, 64), (B * h * w, 16), (B * A * h * w, 32), (B * A * h * w, 32))])
    y, t_a, t_h, t_v = capi.distg_branch_tail(x, spa, *wp, B, A, h, w, L, out=outs)
    torch.cuda.synchronize()
    assert y.data_ptr() == outs[0].data_ptr()
    assert torch.equal(t_a, ta_old)
    assert torch.equal(y, y_old), float((y - y_old).abs().max())
    for name, pool, o in zip(("y", "t_a", "t_h", "t_v"), pools, outs):
        assert bool((pool[:GUARD] == SENTINEL).all()) and bool((pool[GUARD + o.numel():] == SENTINEL).all()), name + ": written outside its rows"
        assert not bool((o == SENTINEL).any()), name + ": rows left unwritten"
