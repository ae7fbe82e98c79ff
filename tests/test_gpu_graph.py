"""GPU: a runtime's forward captured into a HIP graph (capi.GraphedForward) replays the eager launches: bit-equal outputs, also for a second input of the same shape.

All five runtimes, at the headline 5x5 32x32 x4 geometry and at a small ragged one, with the workspace scrubbed between replays; a graph owns the workspace it was
captured with (a forward at another shape, graphed or eager, must not hand that memory back to the allocator under a live graph: checked through references only);
the graph key follows every forward arithmetic switch that reaches the model; and one training step (forward_train + backward) of the four trainable runtimes
replays from a graph, where lfsr_distgssr_backward takes its one-stream form by its own check."""
import json
import os
import weakref

import pytest
import torch

from lfsr_amd import capi
from lfsr_amd.synth import synth_input, synth_state_dict
from tests import helpers as TH
from tests import stream_helpers as SH
from tests.test_gpu_modes_geometries import ON, reach

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = tuple(SH.PLUGINS)                 # distgssr, epit, lft, internet, lfssr
TRAINABLE = ("distgssr", "epit", "lft", "internet")


def _runtime(name):
    key = {"distgssr": "DistgSSR", "epit": "EPIT", "lft": "LFT"}[name]
    meta = json.load(open(os.path.join(ROOT, "tests", "golden", "models.json")))["models"][key]["full"]
    sd = synth_state_dict([(k, tuple(s)) for k, s in meta["spec"]], seed=0)
    rt = capi.DistgSSRRuntime(5, 4) if name == "distgssr" else capi.ModelRuntime(name, 5, 4, 5 if name == "epit" else 4, 64)
    rt.load_state([(k, torch.from_numpy(v).cuda()) for k, v in sd.items()], torch.device("cuda"))
    return rt


@pytest.mark.parametrize("name,B", [("epit", 1), ("distgssr", 2), ("lft", 1)])
def test_graph_replay_equals_eager(name, B):
    rt = _runtime(name)
    gf = capi.GraphedForward(rt)
    for seed in (3, 4):                                   # the second input replays the graph captured for the first
        x = torch.from_numpy(synth_input((B, 1, 160, 160), seed=seed)).cuda()
        y_graph = gf(x).clone()
        y_eager = rt.forward(x)
        torch.cuda.synchronize()
        assert torch.equal(y_graph, y_eager), (name, seed)
    assert len(gf.graphs) == 1


def loaded_runtime(name, A, s):
    """the runtime of the plugin of `name` at (A, s) with the synth weights (seed 0) packed, and the plugin that keeps it alive"""
    model = SH.PLUGINS[name]
    sd, _, _ = SH.case(model, (A, s, 1, 8, 8))
    net = SH.make_net(model, (A, s), sd)
    rt = net._runtime(torch.device("cuda", torch.cuda.current_device()))
    torch.cuda.synchronize()
    return rt, net


def lr_input(A, B, h, w, seed):
    return torch.from_numpy(synth_input((B, 1, A * h, A * w), seed=seed)).cuda()


def scrub_workspace(rt):
    """NaN into the inference workspace: a replay that relied on what an earlier run left there would show"""
    for t in rt.ws.values():
        SH.nan_fill(t)


# (A, s, B, h, w): the headline geometry and a small ragged one (A = 3: off every A = 5 kernel; 6 x 8 views, a batch boundary)
GEOMETRIES = ((5, 4, 1, 32, 32), (3, 2, 2, 6, 8))


@pytest.mark.parametrize("name", NAMES)
def test_graph_replay_two_geometries_scrubbed_workspace(name):
    for A, s, B, h, w in GEOMETRIES:
        rt, net = loaded_runtime(name, A, s)
        xs = [lr_input(A, B, h, w, seed) for seed in (3, 4)]
        eager = [rt.forward(x).clone() for x in xs]
        gf = capi.GraphedForward(rt)
        assert torch.equal(gf(xs[0]), eager[0]), (name, A, "capture")
        for i in (1, 0, 1):                              # the second input reaches the graph's static input only through gf
            scrub_workspace(rt)
            y = gf(xs[i])
            torch.cuda.synchronize()
            assert torch.equal(y, eager[i]), (name, (A, s, B, h, w), i)
        assert len(gf.graphs) == 1
        assert not torch.equal(eager[0], eager[1])


@pytest.mark.parametrize("name", NAMES)
def test_graph_owns_the_workspace_it_was_captured_with(name):
    """ModelRuntime keeps one workspace and drops it when the geometry changes; the launches of a captured graph hold that workspace's raw pointer.  After a graphed
    forward at a second shape and an eager one at a third, graph 1's workspace must still be alive -- held by the GraphedForward entry -- and graph 1 must replay to
    the same bits.  (Ownership is checked through references: nothing is released under a live graph to make the point.)"""
    A, s = 3, 2
    rt, net = loaded_runtime(name, A, s)
    x1, x2, x3 = lr_input(A, 2, 6, 8, 3), lr_input(A, 1, 5, 7, 4), lr_input(A, 1, 8, 6, 5)
    gf = capi.GraphedForward(rt)
    y1 = gf(x1).clone()
    assert len(rt.ws) == 1
    ws1 = weakref.ref(next(iter(rt.ws.values())))        # no strong reference is kept here
    y2 = gf(x2).clone()
    y3 = rt.forward(x3).clone()
    torch.cuda.synchronize()
    assert ws1() is not None, "the workspace graph 1 was captured with has been handed back to the allocator while the graph is alive"
    assert any(ws1() is t for g in gf.graphs.values() for t in g[3]), "something other than the GraphedForward entry holds the workspace"
    y1b = gf(x1).clone()
    torch.cuda.synchronize()
    assert torch.equal(y1b, y1), name
    assert torch.equal(y1, rt.forward(x1)) and torch.equal(y2, rt.forward(x2)) and torch.equal(y3, rt.forward(x3))
    assert torch.equal(gf(x2), y2) and len(gf.graphs) == 2


# model -> the row (A, s, B, h, w) of tests/modes_refs.py:ROWS (LFSSR: tests/lfssr_helpers.py:LFSSR_MATRIX) at which the most forward switches reach it
KEY_ROWS = {"distgssr": (5, 3, 2, 13, 16), "epit": (2, 3, 2, 9, 7), "lft": (2, 3, 2, 9, 7), "internet": (2, 2, 2, 32, 33), "lfssr": (2, 2, 3, 9, 7)}


def forward_switches(name):
    if name == "lfssr":
        return ["ang"]
    return sorted(reach(SH.PLUGINS[name], KEY_ROWS[name], train=False))


def test_the_key_rows_reach_every_forward_switch():
    assert forward_switches("distgssr") == ["arith", "branch"] and forward_switches("internet") == ["gemm", "wide"]
    assert forward_switches("epit") == forward_switches("lft") == ["arith", "gemm"]
    assert {k for n in NAMES for k in forward_switches(n)} == {"arith", "gemm", "branch", "wide", "ang"}      # the five components of GraphedForward's key


@pytest.mark.parametrize("name", NAMES)
def test_graph_key_follows_the_forward_switches(name):
    """a graph holds the kernels of the modes it was captured in: with a switch on, gf captures a new graph that equals eager under the mode; back at the default
    the first graph is replayed; the two modes' outputs differ, so a missing key component would show"""
    A, s, B, h, w = KEY_ROWS[name]
    rt, net = loaded_runtime(name, A, s)
    x = lr_input(A, B, h, w, 3)
    gf = capi.GraphedForward(rt)
    y_def = rt.forward(x).clone()
    assert torch.equal(gf(x), y_def) and len(gf.graphs) == 1
    for n, k in enumerate(forward_switches(name), start=2):
        with TH.modes(**{k: ON[k]}):
            y_on = rt.forward(x).clone()
            assert torch.equal(gf(x), y_on), (name, k)
            assert len(gf.graphs) == n, (name, k)
        assert all(v == 0 for v in TH.modes_now().values())
        assert torch.equal(gf(x), y_def), (name, k, "back at the default")
        assert len(gf.graphs) == n, (name, k)
        assert not torch.equal(y_on, y_def), (name, k, "the switch does not reach this row: the check is not live")


TRAIN_ROWS = {"distgssr": (5, 3, 2, 13, 16), "epit": (2, 3, 2, 9, 7), "lft": (2, 3, 2, 9, 7), "internet": (7, 2, 1, 5, 6)}


@pytest.mark.parametrize("name", TRAINABLE)
def test_training_step_replays_from_a_graph(name):
    """forward_train + backward captured once and replayed with new inputs and output gradients: output and gradient bucket bit-equal to the eager step.  Under
    capture lfsr_distgssr_backward keeps one stream (eager: two), the same bits."""
    A, s, B, h, w = TRAIN_ROWS[name]
    rt, net = loaded_runtime(name, A, s)
    n = rt.num_params()
    out_shape = (B, 1, A * h * s, A * w * s)
    sx, sd_ = lr_input(A, B, h, w, 3), torch.from_numpy(synth_input(out_shape, seed=13)).cuda() - 0.5
    sg = torch.empty(n, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                        # warm-up off the capture, as GraphedForward does: first-launch attribute calls, the training workspace
        for _ in range(2):
            rt.forward_train(sx)
            rt.backward(sx, sd_, sg)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sy = rt.forward_train(sx)
        rt.backward(sx, sd_, sg)
    tws = tuple(rt.tws.values())                         # the captured launches hold its pointer
    seen = []
    for seed in (5, 6):
        x, d = lr_input(A, B, h, w, seed), torch.from_numpy(synth_input(out_shape, seed=10 + seed)).cuda() - 0.5
        sx.copy_(x)
        sd_.copy_(d)
        SH.nan_fill(sg)
        graph.replay()
        torch.cuda.synchronize()
        y_g, g_g = sy.clone(), sg.clone()
        y_e = rt.forward_train(x)
        g_e = rt.backward(x, d)
        torch.cuda.synchronize()
        assert tuple(rt.tws.values())[0] is tws[0]
        assert torch.equal(y_g, y_e), (name, seed)
        assert torch.equal(g_g, g_e), (name, seed, int((g_g != g_e).sum()))
        assert bool(torch.isfinite(g_g).all())
        seen.append(g_g)
    assert not torch.equal(seen[0], seen[1])
