"""GPU: LFT training through the HIP path (lfsr_lft_forward_train / _backward, the whole-model autograd node of lfsr_amd.hip_model)."""
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from lfsr_amd.synth import synth_input, synth_state_dict
from oracle import lfsr_torch_port as P
from tests.helpers import GOLDEN, lft_forced_fp64_grads, model_case

pytestmark = pytest.mark.gpu
TAGS = ("a5h8s4", "a3h6w8s2")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def make_net(A, s, sd=None):
    from lfsr_amd.model.SR import LFT as M
    net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
    if sd is not None:
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.cuda(), M


def spec_sd(A, s, seed=0):
    net, _ = make_net(A, s)
    return synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed)


def hip_step(net, x, label):
    """one fwd + L1 + bwd on the plugin -> (loss, bucket, out)"""
    for p in net.parameters():
        p.grad = None
    out = net(x)
    loss = torch.nn.functional.l1_loss(out, label)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), net.grad_bucket.clone(), out.detach()


@pytest.fixture
def fp64_port(monkeypatch):
    """the port's graph in fp64 throughout: its position encodings come back as fp32 and are cast here"""
    orig = P._lft_pe
    monkeypatch.setattr(P, "_lft_pe", lambda l, d, temperature=10000: [t.double() for t in orig(l, d, temperature)])


def port_grads(sd, x, label, A, s, dtype=torch.float64):
    params = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in sd.items()}
    out = P.lft_forward.__wrapped__(torch.as_tensor(x).to(dtype), params, A, s)
    loss = torch.nn.functional.l1_loss(out, torch.as_tensor(label).to(dtype))
    loss.backward()
    return float(loss.detach()), {k: p.grad.numpy() for k, p in params.items()}


def forced_fp64_grads(rt, xg, sd, x, label, A, s):
    """fp64 autograd of the reference graph with every ReLU / LeakyReLU decision taken from what the HIP path computed, and the number of
    those decisions that differ from fp64's own: tests/helpers.py::lft_forced_fp64_grads"""
    return lft_forced_fp64_grads(rt, xg, sd, x, label, A, s)


def check_against_port(net, bucket, ref):
    errs = []
    for k, _ in net.named_parameters():
        off, n = net._spans[k]
        errs.append(rel(bucket[off:off + n].cpu().numpy().reshape(ref[k].shape), ref[k]))
    errs = np.array(errs)
    return float(np.median(errs)), float(errs.max())


@pytest.mark.parametrize("tag", TAGS)
def test_grads_match_reference_golden(tag, fp64_port):
    npz = np.load(os.path.join(GOLDEN, "lft_grads.npz"))
    names = json.load(open(os.path.join(GOLDEN, "lft_grads.json")))["tags"][tag]["names"]
    case, sd, x, _ = model_case("LFT", tag)
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    net, _ = make_net(A, s, sd)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    xg = torch.from_numpy(x).cuda()
    loss, bucket, _ = hip_step(net, xg, torch.from_numpy(label).cuda())
    forced, flips = forced_fp64_grads(net._rt, xg, sd, x, label, A, s)
    print(f"{tag}: ReLU / LeakyReLU decisions of the HIP path that differ from fp64: {flips}")
    assert abs(loss - float(npz[f"{tag}::loss"])) < 1e-6
    assert [k for k, _ in net.named_parameters()] == names
    # every parameter against the reference's golden; where the GPU's fp32 rounding took the other side of a tie (flips > 0) the gradients
    # below it legitimately differ: then the reference graph with the GPU's decisions is the 1e-4 yardstick and the golden gets the fp64 gate
    gate = 1e-4 if flips == 0 else 1e-2
    for i, (k, p) in enumerate(net.named_parameters()):
        g = p.grad.detach().cpu().numpy().astype(np.float64)
        probe = np.random.default_rng([7, i]).standard_normal(g.shape)
        nrm = np.sqrt((g * g).sum())
        assert abs(nrm - npz[f"{tag}::norms"][i]) <= gate * npz[f"{tag}::norms"][i], k
        assert abs((g * probe).sum() - npz[f"{tag}::projs"][i]) <= gate * nrm * np.sqrt(probe.size), k
        if f"{tag}::grad::{k}" in npz:
            assert rel(g, npz[f"{tag}::grad::{k}"]) < gate, k
        assert rel(g, forced[k]) < 1e-4, k


@pytest.mark.parametrize("tag", TAGS)
def test_grads_match_fp64_port_and_bucket(tag, fp64_port):
    case, sd, x, _ = model_case("LFT", tag)
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    net, _ = make_net(A, s, sd)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    xg = torch.from_numpy(x).cuda()
    _, bucket, _ = hip_step(net, xg, torch.from_numpy(label).cuda())
    forced, flips = forced_fp64_grads(net._rt, xg, sd, x, label, A, s)
    _, ref = port_grads(sd, x, label, A, s)
    med, mx = check_against_port(net, bucket, forced)
    med0, mx0 = check_against_port(net, bucket, ref)
    print(f"{tag}: rel-L2 vs fp64 with the HIP decisions median {med:.2e} max {mx:.2e}; vs fp64 median {med0:.2e} max {mx0:.2e} ({flips} decisions differ)")
    assert med <= 5e-5 and mx <= 1e-2
    assert mx0 <= 1e-2
    cat = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    assert torch.equal(cat, net.grad_bucket)


def test_baseline_geometry_against_fp64(fp64_port):
    A, s, B, h, w = 5, 4, 1, 32, 32
    sd = spec_sd(A, s)
    net, _ = make_net(A, s, sd)
    x = synth_input((B, 1, A * h, A * w), seed=1)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    xg = torch.from_numpy(x).cuda()
    _, bucket, _ = hip_step(net, xg, torch.from_numpy(label).cuda())
    forced, flips = forced_fp64_grads(net._rt, xg, sd, x, label, A, s)
    _, ref = port_grads(sd, x, label, A, s)
    med, mx = check_against_port(net, bucket, forced)
    med0, mx0 = check_against_port(net, bucket, ref)
    print(f"BASELINE 5x5 32x32 x4: rel-L2 vs fp64 with the HIP decisions median {med:.2e} max {mx:.2e}; vs fp64 median {med0:.2e} max {mx0:.2e} "
          f"({flips} decisions differ)")
    assert med <= 5e-5 and mx < 1e-4      # per parameter, as tests/test_gpu_lft_geometries.py holds at this patch with B = 8 (worst seen there: 1.1e-06)
    assert mx0 <= 1e-2


def test_scale3_grads_match_fp64_port_and_bucket(fp64_port):
    """s = 3: the training forward's two-kernel tail, k_tail_bwd with s^2 = 9 (its element-wise store branch) and k_pack_up0_T with s2 = 9; every parameter's
    gradient against the fp64 port with the HIP path's ReLU / LeakyReLU decisions, the bucket against the concatenated .grad"""
    A, s, B, h, w = 3, 3, 2, 6, 8
    sd = spec_sd(A, s)
    net, _ = make_net(A, s, sd)
    x = synth_input((B, 1, A * h, A * w), seed=1)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    xg = torch.from_numpy(x).cuda()
    loss, bucket, out = hip_step(net, xg, torch.from_numpy(label).cuda())
    forced, flips = forced_fp64_grads(net._rt, xg, sd, x, label, A, s)
    print(f"s=3: ReLU / LeakyReLU decisions of the HIP path that differ from fp64: {flips}")
    for k, p in net.named_parameters():
        assert rel(p.grad.detach().cpu().numpy(), forced[k]) < 1e-4, k
    cat = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    assert torch.equal(cat, net.grad_bucket)
    ref_out = P.lft_forward.__wrapped__(torch.as_tensor(x).double(), {k: torch.tensor(v, dtype=torch.float64) for k, v in sd.items()}, A, s)
    assert float((out.cpu().double() - ref_out).abs().max()) < 1e-4


@pytest.mark.parametrize("arith", ["default", "f32"])
def test_train_forward_output_bit_equal_to_inference(arith):
    case, sd, x, _ = model_case("LFT", "a3h6w8s2")
    net, _ = make_net(case["A"], case["s"], sd)
    xg = torch.from_numpy(x).cuda()
    if arith == "f32":
        capi.set_arithmetic(capi.ARITH_F32)
    try:
        with torch.no_grad():
            y0 = net(xg).clone()
        y1 = net(xg)
    finally:
        capi.set_arithmetic(capi.ARITH_DEFAULT)
    assert y1.requires_grad
    assert torch.equal(y0, y1.detach())


def test_backward_deterministic():
    case, sd, x, _ = model_case("LFT", "a5h8s4")
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    net, _ = make_net(A, s, sd)
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).cuda()
    xg = torch.from_numpy(x).cuda()
    _, b1, _ = hip_step(net, xg, label)
    _, b2, _ = hip_step(net, xg, label)
    assert torch.equal(b1, b2)


DECISIONS = [(5, 0), (5, 1), (8, 0), (9, 0)] + [(6, b) for b in range(4)] + [(7, b) for b in range(4)]   # lfsr_lft_train_saved


def decisions(rt, x):
    """the ReLU / LeakyReLU decisions of the last forward_train + backward, as one flat bool tensor per (which, index), per sample"""
    B = x.shape[0]
    return {k: (rt.train_saved(x, *k) > 0).reshape(B, -1).cpu() for k in DECISIONS}


def test_batch_linearity():
    A, s, h, w = 5, 2, 8, 8
    sd = spec_sd(A, s)
    net, _ = make_net(A, s, sd)
    x = torch.from_numpy(synth_input((4, 1, A * h, A * w), seed=3)).cuda()
    label = torch.from_numpy(synth_input((4, 1, A * h * s, A * w * s), seed=4)).cuda()
    _, b4, _ = hip_step(net, x, label)
    d4 = decisions(net._rt, x)
    singles, flips = [], 0
    for i in range(4):
        singles.append(hip_step(net, x[i:i + 1], label[i:i + 1])[1])
        flips += sum(int((d[0] != d4[k][i]).sum()) for k, d in decisions(net._rt, x[i:i + 1]).items())
    singles = torch.stack(singles).mean(0)
    errs = np.array([rel(b4[o:o + n].cpu(), singles[o:o + n].cpu()) for o, n in net._spans.values()])
    print(f"batch linearity: rel-L2 median {np.median(errs):.2e} max {errs.max():.2e}; decisions differing between B = 4 and B = 1: {flips}")
    # B = 4 and B = 1 run kernels whose fp32 rounding differs in the last bit; where that puts a pre-activation on the other side of 0
    # (measured: one of ~2.5M feed-forward ReLUs) the parameters below it move by ~1e-3 in a case this small, as against fp64 (see the
    # golden test): then the gate is the fp64 one
    if flips == 0:
        assert errs.max() < 1e-4
    else:
        assert np.median(errs) <= 1e-3 and errs.max() <= 1e-2


def test_accumulation_and_zero_grad():
    case, sd, x, _ = model_case("LFT", "a3h6w8s2")
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    labels = [synth_input((B, 1, A * h * s, A * w * s), seed=sd_) for sd_ in (2, 5)]
    net, _ = make_net(A, s, sd)
    xg = torch.from_numpy(x).cuda()
    lg = [torch.from_numpy(lab).cuda() for lab in labels]
    b1, b2 = hip_step(net, xg, lg[0])[1], hip_step(net, xg, lg[1])[1]      # each micro-batch alone (the backward is deterministic)
    span = {k: slice(o, o + n) for k, (o, n) in net._spans.items()}
    g1, g2 = ({k: bk[span[k]].view_as(p).cpu().numpy() for k, p in net.named_parameters()} for bk in (b1, b2))
    for p in net.parameters():
        p.grad = None
    for lab in lg:              # two micro-batches, accumulated into p.grad
        torch.nn.functional.l1_loss(net(xg), lab).backward()
    for k, p in net.named_parameters():
        assert rel(p.grad.cpu().numpy(), g1[k] + g2[k]) < 1e-6, k
    # zero_grad(set_to_none=False), then one backward: p.grad += into the zeroed tensors
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    opt.zero_grad(set_to_none=False)
    torch.nn.functional.l1_loss(net(xg), lg[0]).backward()
    for k, p in net.named_parameters():
        assert np.array_equal(p.grad.cpu().numpy(), g1[k]), k


def test_stale_workspace_raises():
    case, sd, x, _ = model_case("LFT", "a5h8s4")
    net, _ = make_net(case["A"], case["s"], sd)
    xg = torch.from_numpy(x).cuda()
    y1 = net(xg)
    y2 = net(xg)
    with pytest.raises(capi.LfsrError):
        y1.sum().backward()
    y2.sum().backward()


def test_inference_between_training_forward_and_backward():
    case, sd, x, _ = model_case("LFT", "a5h8s4")
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    net, _ = make_net(A, s, sd)
    xg = torch.from_numpy(x).cuda()
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).cuda()
    _, ref, _ = hip_step(net, xg, label)
    y = net(xg)
    with torch.no_grad():
        net(xg[:, :, : A * (h // 2), : A * (w // 2)].contiguous())     # another shape: the inference workspace is replaced, the training one stays
    torch.nn.functional.l1_loss(y, label).backward()
    assert torch.equal(net.grad_bucket, ref)


def test_fused_adamw_steps_repack():
    from lfsr_amd.train_step import train_step
    case, sd, x, _ = model_case("LFT", "a3h6w8s2")
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    net, M = make_net(A, s, sd)
    crit = M.get_loss(None)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, fused=True)
    xg = torch.from_numpy(x).cuda()
    lg = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).cuda()
    for _ in range(2):
        train_step(net, crit, opt, xg, lg)
    with torch.no_grad():
        y = net(xg).cpu().numpy()
    upd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    assert any(not np.array_equal(upd[k].numpy(), sd[k]) for k in sd)
    ref = P.lft_forward(torch.from_numpy(x), upd, A, s).numpy()
    assert np.abs(y - ref).max() < 1e-4


def test_train_step_runs():
    from lfsr_amd.train_step import train_step
    A, s, h, w, B = 5, 4, 8, 8, 2
    net, M = make_net(A, s, spec_sd(A, s))
    crit = M.get_loss(None)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-4)
    x = torch.from_numpy(synth_input((B, 1, A * h, A * w), seed=6)).cuda()
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=7)).cuda()
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    loss, _ = train_step(net, crit, opt, x, label)
    assert np.isfinite(float(loss))
    assert torch.isfinite(net.grad_bucket).all()
    assert any(not torch.equal(before[k], v) for k, v in net.state_dict().items())


def test_reference_loop_shape_amp_gradscaler_clip():
    A, s, h, w, B = 5, 4, 8, 8, 2
    net, M = make_net(A, s, spec_sd(A, s))
    crit = M.get_loss(None)
    opt = torch.optim.Adam(net.parameters(), lr=2e-4)
    scaler = torch.amp.GradScaler("cuda")
    losses = []
    for it in range(3):      # train.py:243-268
        x = torch.from_numpy(synth_input((B, 1, A * h, A * w), seed=10 + it)).cuda()
        label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=20 + it)).cuda()
        with torch.amp.autocast("cuda"):
            out = net(x, [A, A])
            loss = crit(out, label, [A, A])
        opt.zero_grad()
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm=1.0)
        scaler.step(opt)
        scaler.update()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses))


def test_oversize_batch_refused_before_allocation():
    A, s = 5, 4
    net, _ = make_net(A, s, spec_sd(A, s))
    h = w = 64
    B = ((1 << 31) - 1) // 4 // (64 * s * s) // (A * A * h * w) + 1     # the HR rows (64 s^2 floats per LR pixel) reach 2 GiB
    x = torch.zeros((B, 1, A * h, A * w), device="cuda")
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(capi.LfsrError):
        net(x)
    assert net._rt.train_workspace_bytes(B, h, w) == 0
    assert net._rt.train_workspace_bytes(8, 32, 32) > 0 and net._rt.train_workspace_bytes(16, 32, 32) > 0
    assert torch.cuda.memory_allocated() <= before + (64 << 20)     # (the weight repack only: no training workspace)
