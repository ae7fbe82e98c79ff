"""GPU: every driver and every operator off the default stream.

The argument no other test varies is `void* stream`: the whole suite runs on the default stream, where every launch is serialised behind every other and a launch
that drops its stream (or work a driver puts on a stream of its own without the right events) computes the right thing.  Here every call runs on a side stream whose
inputs arrive late (tests/stream_helpers.py:run_late): the stream is held back by a delay, the inputs are NaN until copies queued behind the delay fill them in, and
every buffer the call owns is NaN.  The reference is the same call on the default stream, which the fp64 tests of each operator and model gate; the drivers promise
a fixed summation order, so the comparison is bit equality.  Each case asserts that the delay was still running when the call's last launch had been queued.

  whole models, forward          the five plugins at the rows that choose different launch sequences
  whole models, a training step  the four trainable plugins (the repack -- load_param, finalize -- forward_train, the loss and the backward all on the side stream);
                                 DistgSSR's two-stream backward against its one-stream form; two steps back to back with no synchronisation between them
  every operator entry point     tests/stream_ops.py:OPS (tests/test_stream_table_cpu.py asserts the table covers include/lfsr_hip.h)
  two contexts, two streams      two runtimes of one model with their own weights, late on two streams at once, issued alternately

Measured host issue times, the delay and the wall time: profiles/stream_tests.md (every line this file prints starts with `STREAMS |`)."""
import pytest
import torch
import torch.nn.functional as F

from lfsr_amd import capi
from lfsr_amd.synth import synth_input
from tests import lfssr_helpers as LH
from tests import modes_refs as R
from tests import stream_helpers as SH
from tests import stream_ops
from tests.stream_helpers import case, make_net

pytestmark = pytest.mark.gpu

# (A, s, B, h, w) per model: rows of tests/modes_refs.py:ROWS (tests/lfssr_helpers.py:LFSSR_MATRIX for LFSSR) that take different launch sequences
FWD_ROWS = {
    "DistgSSR": ((5, 3, 2, 13, 16),        # the fused block tail
                 (5, 2, 1, 33, 6),         # lines of 33: the unfused branches
                 (3, 3, 1, 13, 16)),       # A = 3: the gather EPI forward, three-kernel block tail
    "LF_InterNet": ((2, 2, 2, 32, 33),     # past the 2048-row threshold of the row GEMMs
                    (7, 2, 1, 5, 6)),
    "EPIT": ((2, 3, 2, 9, 7),              # odd ragged views, even A, the two-kernel tail of scale 3
             (5, 3, 2, 13, 15)),           # the N1 = 5 MFMA attention kernels
    "LFT": ((2, 3, 2, 9, 7),
            (5, 3, 2, 13, 15)),
    "LFSSR": ((2, 2, 3, 9, 7),             # odd ragged views, every view a corner
              (7, 2, 1, 5, 6)),            # banded angular launches
}
TRAIN_ROWS = {
    "DistgSSR": ((7, 2, 1, 5, 6),),        # (A = 5 and A = 3: test_distgssr_backward_two_streams_one_stream_default_stream)
    "LF_InterNet": ((7, 2, 1, 5, 6), (2, 3, 2, 9, 7)),
    "EPIT": ((2, 3, 2, 9, 7), (1, 2, 2, 8, 8)),
    "LFT": ((2, 3, 2, 9, 7), (1, 2, 2, 8, 8)),
}
OVERLAP_ROWS = ((5, 3, 2, 13, 16), (3, 3, 1, 13, 16))
ids = lambda c: "%s-A%ds%dB%dh%dw%d" % ((c[0],) + tuple(c[1]))
FWD_CASES = [(m, g) for m in FWD_ROWS for g in FWD_ROWS[m]]
TRAIN_CASES = [(m, g) for m in TRAIN_ROWS for g in TRAIN_ROWS[m]]


def test_the_rows_are_rows_of_the_geometry_matrices():
    for m, g in FWD_CASES + TRAIN_CASES + [("DistgSSR", g) for g in OVERLAP_ROWS]:
        assert g in (LH.LFSSR_MATRIX if m == "LFSSR" else R.ROWS[m]), (m, g)
    for m, g in TRAIN_CASES + [("DistgSSR", g) for g in OVERLAP_ROWS]:
        assert R.has_backward(m, g)
    assert all(len(FWD_ROWS[m]) >= 2 for m in FWD_ROWS) and len(FWD_ROWS) == 5


def forward_job(net, xg, slot=0):
    """the plugin's no-grad forward; the weights are packed beforehand, on the default stream"""
    def call(x):
        with torch.no_grad():
            return net(x)
    with torch.cuda.stream(torch.cuda.default_stream()):
        call(xg)
    torch.cuda.synchronize()
    return call, [xg], [net._rt.ws, net._rt.tws], slot


def step_call(net):
    """one forward + L1 + backward through the plugin, everything on the current stream -> (output, gradient bucket)"""
    def call(x, label):
        for p in net.parameters():
            p.grad = None
        out = net(x)
        F.l1_loss(out, label).backward()
        return out.detach(), net.grad_bucket
    return call


def step_scrub(net):
    """the two workspaces and the packed weights: a training forward repacks every parameter on the caller's stream"""
    rt = net._rt
    return [rt.ws, rt.tws, lambda: SH.nan_fill(rt.packed)]


def trained_net(model, geom):
    sd, x, label = case(model, geom)
    net = make_net(model, geom, sd)
    xg, lg = torch.from_numpy(x).cuda(), torch.from_numpy(label).cuda()
    with torch.cuda.stream(torch.cuda.default_stream()):
        step_call(net)(xg, lg)              # creates the runtime and its workspaces
    torch.cuda.synchronize()
    return net, xg, lg


# ---------------------------------------------------------------------------------------------------------------------
# the harness itself
# ---------------------------------------------------------------------------------------------------------------------
def test_harness_catches_a_launch_on_the_wrong_stream():
    """a call that puts one of its kernels on the default stream instead of the caller's: the late leg must differ (the stray kernel reads NaN while the delay spins)"""
    x = torch.rand(4096, device="cuda")

    def stray(t):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return t * 2.0

    with pytest.raises(AssertionError, match="differs on a side stream"):
        SH.run_late(stray, [x], what="planted stray launch", delay_ms=50)
    SH.run_late(lambda t: t * 2.0, [x], what="the same kernel on the caller's stream", delay_ms=50)


def test_harness_refuses_a_case_whose_delay_has_ended():
    x = torch.rand(4096, device="cuda")

    def slow(t):
        torch.cuda.current_stream().synchronize()        # the host waits for the delay: the inputs are in place before the launch
        return t * 2.0

    with pytest.raises(AssertionError, match="proves nothing"):
        SH.run_late(slow, [x], what="host waits", delay_ms=5)


# ---------------------------------------------------------------------------------------------------------------------
# whole models
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FWD_CASES, ids=ids)
def test_forward_late(c):
    model, geom = c
    sd, x, _ = case(model, geom)
    net = make_net(model, geom, sd)
    call, inputs, scrub, _ = forward_job(net, torch.from_numpy(x).cuda())
    (y,) = SH.run_late(call, inputs, scrub, what=f"{model} {geom} forward")
    assert bool(torch.isfinite(y).all())


def test_distgssr_taps_late():
    """lfsr_distgssr_forward_taps: the forward with copies of five activations, at the fused-tail row"""
    geom = (5, 3, 2, 13, 16)
    sd, x, _ = case("DistgSSR", geom)
    net = make_net("DistgSSR", geom, sd)
    call, inputs, scrub, _ = forward_job(net, torch.from_numpy(x).cuda())
    rt = net._rt

    def taps(t):
        out, bufs = rt.forward(t, taps=[True] * 5)
        return [out] + bufs
    got = SH.run_late(taps, inputs, scrub, what=f"DistgSSR {geom} forward_taps")
    assert len(got) == 6


@pytest.mark.parametrize("c", TRAIN_CASES, ids=ids)
def test_training_step_late(c):
    model, geom = c
    net, xg, lg = trained_net(model, geom)
    out, bucket = SH.run_late(step_call(net), [xg, lg], step_scrub(net), what=f"{model} {geom} training step")
    assert bool(torch.isfinite(bucket).all()) and bool(torch.isfinite(out).all())
    assert SH.bits_equal(torch.cat([p.grad.reshape(-1) for p in net.parameters()]), bucket)


@pytest.mark.parametrize("geom", OVERLAP_ROWS, ids=lambda g: "A%ds%dB%dh%dw%d" % g)
def test_distgssr_backward_two_streams_one_stream_default_stream(geom, monkeypatch):
    """lfsr_distgssr_backward runs the angular and EPI branch gradients on a stream of its own between four events (the product default); LFSR_BWD_OVERLAP=0 keeps
    one stream.  Default arithmetic.  The two forms late on a side stream, and the one-stream form on the default stream, all give the default stream's bucket."""
    monkeypatch.delenv("LFSR_BWD_OVERLAP", raising=False)
    net, xg, lg = trained_net("DistgSSR", geom)
    call, scrub = step_call(net), step_scrub(net)
    want = SH.reference(call, [xg, lg])                                # two streams, issued from the default stream
    SH.run_late(call, [xg, lg], scrub, what=f"DistgSSR {geom} step, two-stream backward", want=want)
    monkeypatch.setenv("LFSR_BWD_OVERLAP", "0")
    one = SH.reference(call, [xg, lg])
    assert SH.bits_equal(one[0], want[0]) and SH.bits_equal(one[1], want[1]), "one stream and two streams differ on the default stream"
    SH.run_late(call, [xg, lg], scrub, what=f"DistgSSR {geom} step, one-stream backward", want=want)


@pytest.mark.parametrize("c", [("DistgSSR", (5, 3, 2, 13, 16)), ("LF_InterNet", (7, 2, 1, 5, 6)), ("EPIT", (2, 3, 2, 9, 7)), ("LFT", (2, 3, 2, 9, 7))], ids=ids)
def test_two_training_steps_back_to_back(c):
    """two steps on the side stream with nothing between them, the second on another input: the second bucket is the second step's own (DistgSSR: the join of
    step 1 against the fork of step 2, and the reuse of the four events)"""
    model, geom = c
    net, xg, lg = trained_net(model, geom)
    x2 = torch.from_numpy(synth_input(tuple(xg.shape), seed=7)).cuda()
    l2 = torch.from_numpy(synth_input(tuple(lg.shape), seed=8)).cuda()
    one = step_call(net)
    want = SH.reference(one, [x2, l2])

    def two(xa, la, xb, lb):
        one(xa, la)
        return one(xb, lb)
    SH.run_late(two, [xg, lg, x2, l2], step_scrub(net), what=f"{model} {geom} two steps", want=want)
    assert not SH.bits_equal(want[1], SH.reference(one, [xg, lg])[1])         # the two steps' buckets differ: the check is live


# ---------------------------------------------------------------------------------------------------------------------
# every operator entry point
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(stream_ops.OPS))
def test_operator_late(name):
    with torch.cuda.stream(torch.cuda.default_stream()):
        call, inputs, scrub = stream_ops.OPS[name]()
    torch.cuda.synchronize()
    SH.run_late(call, inputs, scrub, what=name)


# ---------------------------------------------------------------------------------------------------------------------
# two contexts, two streams
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [("DistgSSR", (5, 3, 2, 13, 16)), ("EPIT", (5, 3, 2, 13, 15))], ids=ids)
def test_two_contexts_two_streams(c):
    """two runtimes of one model, each with its own weights (seeds 0 and 1) and its own input, late on two streams at once, two forwards each, issued alternately
    from the host: device scratch or host state shared between contexts would mix them"""
    model, geom = c
    jobs = []
    nets = []
    for seed in (0, 1):
        sd, x, _ = case(model, geom, seed)
        nets.append((make_net(model, geom, sd), x))
    for rnd in (0, 1):
        for slot, (net, x) in enumerate(nets):
            xg = torch.from_numpy(x if rnd == 0 else synth_input(x.shape, seed=20 + slot)).cuda()
            jobs.append(forward_job(net, xg, slot))
    got = SH.run_late_many(jobs, what=f"{model} {geom} two contexts")
    assert not SH.bits_equal(got[0][0], got[1][0]) and not SH.bits_equal(got[0][0], got[2][0])
