"""What tests/test_gpu_streams.py and tests/test_gpu_graph.py share: run_late(), which runs a call on a side stream whose inputs arrive only after every launch of
the call has been queued, and compares it bit for bit with the same call on the default stream.

Why late inputs: on the default stream every launch is serialised behind every other, so a launch that drops its stream argument (passes 0 or a stale stream)
computes the right thing.  Here the caller's stream S is held back by a delay kernel, the inputs are NaN until copies queued on S *behind* the delay fill them in,
and every buffer the call owns is NaN as well.  A launch that is not ordered behind S runs while the delay still spins, reads NaN, and the output differs from the
default-stream result.  `assert not gate.query()` after the call returns proves that the delay outlived the host's issue of the whole call: without that the case
would show nothing, and it fails saying so.

The delay is torch.cuda._sleep, calibrated once per process; its length (DELAY_MS) is sized in profiles/stream_tests.md."""
import time

import torch

BAND = 64                     # sentinel elements on either side of an explicitly passed output
DELAY_MS = 80.0               # 10 x the slowest host issue time of a call of tests/test_gpu_streams.py, a DistgSSR training step (profiles/stream_tests.md)
_CAL = {}


def cycles_per_ms():
    """spin cycles of torch.cuda._sleep per millisecond, measured once with two events around one _sleep(10**7)"""
    if "c" not in _CAL:
        torch.cuda._sleep(10 ** 6)       # (first use: module load)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(10 ** 7)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        assert ms > 0
        _CAL["c"] = 10 ** 7 / ms
        print(f"STREAMS | calibration | _sleep(1e7) = {ms:.3f} ms | {_CAL['c']:.0f} cycles / ms")
    return _CAL["c"]


def delay(ms=None):
    """queue the delay on the current stream.  _sleep takes a 32-bit cycle count on some builds: long delays are queued in pieces"""
    if not hasattr(torch.cuda, "_sleep"):      # a chain of matmuls instead; the gate.query() check is what counts
        a = torch.ones(4096, 4096, device="cuda")
        for _ in range(64):
            a = (a @ a) * 0
        return
    n = int((DELAY_MS if ms is None else ms) * cycles_per_ms())
    piece = 10 ** 9
    while n > 0:
        torch.cuda._sleep(min(n, piece))
        n -= piece


def nan_fill(t):
    """every byte 0xFF: NaN in every floating type, -1 / the largest value in the integer ones"""
    if t.numel():
        t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


class Banded:
    """an output buffer handed to a call explicitly: `t` (the given shape) sits between two bands of BAND elements whose bytes are 0xFF.  scrub() refills the bands
    and sets t to `init` (an accumulated-into output starts from the same values in both legs) or NaN; intact() tells whether the bands still hold their bytes"""

    def __init__(self, shape, init=None, dtype=torch.float32, device="cuda"):
        n = 1
        for d in shape:
            n *= int(d)
        self.buf = torch.empty(n + 2 * BAND, dtype=dtype, device=device)
        self.t = self.buf[BAND:BAND + n].view(*shape)
        self.init = None if init is None else init.to(device=device, dtype=dtype).reshape(shape).clone()
        self.scrub()

    def scrub(self):
        nan_fill(self.buf)
        if self.init is not None:
            self.t.copy_(self.init)

    def intact(self):
        b = self.buf.view(torch.uint8)
        e = self.buf.element_size()
        return bool((b[:BAND * e] == 0xFF).all()) and bool((b[-BAND * e:] == 0xFF).all())


def _scrub(items):
    """tensors and dicts / lists of tensors are filled with 0xFF bytes, Banded buffers scrubbed, callables called; -> the Banded ones"""
    bands = []
    for it in items or ():
        if it is None:
            continue
        if isinstance(it, Banded):
            it.scrub()
            bands.append(it)
        elif isinstance(it, torch.Tensor):
            nan_fill(it)
        elif isinstance(it, dict):
            bands += _scrub(list(it.values()))
        elif isinstance(it, (list, tuple)):
            bands += _scrub(it)
        elif callable(it):
            it()
        else:
            raise TypeError(type(it))
    return bands


def _outputs(y):
    if isinstance(y, torch.Tensor):
        return [y]
    return [t for t in y if t is not None]


def _late_copy(t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        return t
    if t.is_floating_point():
        return torch.full_like(t, float("nan"))
    return nan_fill(torch.empty_like(t))


def bits_equal(a, b):
    """the same bytes (torch.equal would call a NaN, which some operators produce by design, unequal to itself)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def fresh_stream():
    """torch.cuda.Stream() whose work does not queue behind, or in front of, the default stream's.  The runtime maps its streams onto a few hardware queues, and a
    stream that shares the default stream's queue would serialise a stray default-stream launch behind the delay and hide it: such a stream is passed over (probed
    with a 3 ms delay and one default-stream kernel)."""
    dflt = torch.cuda.default_stream()
    for _ in range(16):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            delay(3.0)
            gate = torch.cuda.Event()
            gate.record()
        with torch.cuda.stream(dflt):
            probe = torch.zeros(8, device="cuda") + 1
            ev = torch.cuda.Event()
            ev.record()
        ev.synchronize()
        independent = not gate.query()
        s.synchronize()
        del probe
        if independent:
            return s
    raise AssertionError("no stream independent of the default stream among 16 new ones")


def reference(call, inputs):
    """the reference leg: the call on the default stream, synchronised, its outputs cloned"""
    with torch.cuda.stream(torch.cuda.default_stream()):
        y = call(*inputs)
    torch.cuda.synchronize()
    return [t.detach().clone() for t in _outputs(y)]


def run_late_many(jobs, what="", delay_ms=None, want=None):
    """jobs: [(call, inputs, scrub, slot)].  Jobs with the same slot share one side stream (issued in list order); every stream is held back by its own delay,
    behind which the inputs of its jobs are copied into place.  The calls are issued from the host in list order, so jobs of different slots alternate.
    Each job's outputs must equal bit for bit its own reference leg (the same call alone on the default stream, run first, in list order).  -> [outputs per job]"""
    if want is None:
        want = [reference(call, inputs) for call, inputs, _, _ in jobs]
    bands = []
    for _, _, scrub, _ in jobs:
        bands += _scrub(scrub)
    slots = sorted({j[3] for j in jobs})
    cycles_per_ms()
    streams = {s: fresh_stream() for s in slots}
    live = [[_late_copy(t) for t in inputs] for _, inputs, _, _ in jobs]
    torch.cuda.synchronize()
    gates = {}
    for s in slots:
        with torch.cuda.stream(streams[s]):
            delay(delay_ms)
            gates[s] = torch.cuda.Event()
            gates[s].record()
            for (_, inputs, _, slot), lv in zip(jobs, live):
                if slot == s:
                    for dst, src in zip(lv, inputs):
                        if isinstance(src, torch.Tensor) and src.is_cuda:
                            dst.copy_(src)
    got = []
    t0 = time.perf_counter()
    for (call, _, _, slot), lv in zip(jobs, live):
        with torch.cuda.stream(streams[slot]):
            got.append(_outputs(call(*lv)))
    host_ms = (time.perf_counter() - t0) * 1e3
    done = {s: gates[s].query() for s in slots}           # right after the last call returned on the host
    for s in slots:
        streams[s].synchronize()
    torch.cuda.synchronize()
    print(f"STREAMS | {what} | host issue {host_ms:.2f} ms | delay {DELAY_MS if delay_ms is None else delay_ms:.0f} ms")
    assert not any(done.values()), (f"{what}: the delay on the side stream had already ended when the last launch was queued (host issue {host_ms:.1f} ms): "
                                    "the inputs were in place before the call, so this run proves nothing about stream order")
    for j, (w, g) in enumerate(zip(want, got)):
        assert len(w) == len(g), (what, j)
        for i, (a, b) in enumerate(zip(w, g)):
            b = b.detach()
            assert a.shape == b.shape and a.dtype == b.dtype, (what, j, i)
            assert bits_equal(a, b), (f"{what}: output {i} of call {j} differs on a side stream with late inputs from the default-stream result "
                                                f"({int((a != b).sum())} of {a.numel()} elements; NaN in the late leg: {bool(torch.isnan(b.float()).any())})")
    for b in bands:
        assert b.intact(), f"{what}: a sentinel band beside an output was written"
    return got


def run_late(call, inputs, scrub=(), what="", delay_ms=None, want=None):
    """call(*inputs) -> a tensor or a sequence of tensors.  Reference leg on the default stream; scrub (tensors, dicts of tensors, Banded buffers, callables:
    everything the call owns becomes NaN); late leg on a fresh stream behind the delay.  -> the late leg's outputs, already asserted bit-equal to the reference"""
    return run_late_many([(call, inputs, scrub, 0)], what, delay_ms, None if want is None else [want])[0]


# ---- the whole-model cases: the five plugins at a row (A, s, B, h, w) of the geometry matrices ----------------------------------------------------------------------
PLUGINS = {"distgssr": "DistgSSR", "epit": "EPIT", "lft": "LFT", "internet": "LF_InterNet", "lfssr": "LFSSR"}      # runtime name -> plugin


def case(model, geom, seed=0):
    """-> state_dict, input, label (numpy fp32); seed 0: the weights of every whole-model test, another seed: other weights of the same shapes"""
    from lfsr_amd.synth import synth_input, synth_state_dict
    A, s, B, h, w = geom
    if model == "LFSSR":
        from tests import lfssr_helpers as LH
        sd, x = LH.lfssr_matrix_case(*geom)
        label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    else:
        from tests import modes_refs as R
        sd, x, label = R.case(model, geom)
    if seed:
        sd = synth_state_dict([(k, v.shape) for k, v in sd.items()], seed=seed)
        if model == "LFSSR":
            from tests import lfssr_helpers as LH
            sd = {k: (v * LH.HE_GAIN).astype(v.dtype) if v.ndim == 4 and v.shape[1] == 64 else v for k, v in sd.items()}
        x = synth_input(x.shape, seed=10 + seed)
    return sd, x, label


def make_net(model, geom, sd):
    """the plugin of `model` with the state_dict loaded, on the device"""
    import importlib
    from argparse import Namespace
    M = importlib.import_module("lfsr_amd.model.SR." + model)
    net = M.get_model(Namespace(angRes_in=geom[0], angRes_out=geom[0], scale_factor=geom[1]))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.cuda().train()
