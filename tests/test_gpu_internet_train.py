"""GPU: LF_InterNet training through the HIP path (lfsr_internet_forward_train / _backward, the whole-model autograd node of lfsr_amd.hip_model)."""
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from lfsr_amd.synth import synth_input, synth_state_dict
from oracle.lfsr_torch_port import internet_forward
from tests.helpers import GOLDEN, forced_fp64_grads, internet_layers_fp64, internet_ref_to_rows, internet_saved_rows, model_case

pytestmark = pytest.mark.gpu
TAGS = ("a3h6w8s4", "a5h8s2")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def make_net(A, s, sd=None):
    from lfsr_amd.model.SR import LF_InterNet as M
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


def port_grads(sd, x, label, A, s, dtype=torch.float64):
    params = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in sd.items()}
    out = internet_forward.__wrapped__(torch.as_tensor(x).to(dtype), params, A, s)
    loss = torch.nn.functional.l1_loss(out, torch.as_tensor(label).to(dtype))
    loss.backward()
    return float(loss.detach()), {k: p.grad.numpy() for k, p in params.items()}


def check_against_port(net, bucket, ref):
    errs = []
    for k, _ in net.named_parameters():
        off, n = net._spans[k]
        errs.append(rel(bucket[off:off + n].cpu().numpy().reshape(ref[k].shape), ref[k]))
    errs = np.array(errs)
    return float(np.median(errs)), float(errs.max())


@pytest.mark.parametrize("tag", TAGS)
def test_grads_match_reference_golden(tag):
    npz = np.load(os.path.join(GOLDEN, "internet_grads.npz"))
    names = json.load(open(os.path.join(GOLDEN, "internet_grads.json")))["tags"][tag]["names"]
    case, sd, x, _ = model_case("LF_InterNet", tag)
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    net, _ = make_net(A, s, sd)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    xg = torch.from_numpy(x).cuda()
    loss, bucket, _ = hip_step(net, xg, torch.from_numpy(label).cuda())
    forced, flips = forced_fp64_grads(net._rt, xg, sd, x, label, A, s)
    print(f"{tag}: ReLU decisions of the HIP forward that differ from fp64: {flips}")
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
def test_grads_match_fp64_port_and_bucket(tag):
    case, sd, x, _ = model_case("LF_InterNet", tag)
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    net, _ = make_net(A, s, sd)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    _, bucket, _ = hip_step(net, torch.from_numpy(x).cuda(), torch.from_numpy(label).cuda())
    _, ref = port_grads(sd, x, label, A, s)
    med, mx = check_against_port(net, bucket, ref)
    print(f"{tag}: rel-L2 vs fp64 median {med:.2e} max {mx:.2e}")
    assert med <= 5e-5 and mx <= 1e-2
    cat = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    assert torch.equal(cat, net.grad_bucket)


def _relu_flips_spa(rt, xg, sd, x, A, s):
    """ReLU decisions of SpaConvSq (16 layers) that differ between the HIP forward's saved values and the fp64 graph"""
    with torch.no_grad():
        _, layers, _ = internet_layers_fp64(x, sd, A, s)
    return sum(int(((internet_ref_to_rows(layers["relu_spa", i], "vcl", A) > 0) != (internet_saved_rows(rt, xg, "relu_spa", i) > 0).cpu()).sum())
               for i in range(16))


def test_baseline_geometry_against_fp64():
    A, s, B, h, w = 5, 2, 1, 32, 32
    sd = spec_sd(A, s)
    net, _ = make_net(A, s, sd)
    x = synth_input((B, 1, A * h, A * w), seed=1)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    xg = torch.from_numpy(x).cuda()
    _, bucket, _ = hip_step(net, xg, torch.from_numpy(label).cuda())
    flips = _relu_flips_spa(net._rt, xg, sd, x, A, s)
    _, ref = port_grads(sd, x, label, A, s)
    med, mx = check_against_port(net, bucket, ref)
    print(f"BASELINE 5x5 32x32 x2: rel-L2 vs fp64 median {med:.2e} max {mx:.2e}; SpaConvSq ReLU decisions differing from fp64: {flips}")
    assert med <= 5e-5 and mx <= 1e-2


def test_train_forward_output_bit_equal_to_inference():
    case, sd, x, _ = model_case("LF_InterNet", "a5h8s2")
    net, _ = make_net(case["A"], case["s"], sd)
    xg = torch.from_numpy(x).cuda()
    with torch.no_grad():
        y0 = net(xg).clone()
    y1 = net(xg)
    assert y1.requires_grad
    assert torch.equal(y0, y1.detach())


def test_backward_deterministic():
    case, sd, x, _ = model_case("LF_InterNet", "a3h6w8s4")
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    net, _ = make_net(A, s, sd)
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).cuda()
    xg = torch.from_numpy(x).cuda()
    _, b1, _ = hip_step(net, xg, label)
    _, b2, _ = hip_step(net, xg, label)
    assert torch.equal(b1, b2)


def test_batch_linearity():
    A, s, h, w = 5, 2, 16, 16
    sd = spec_sd(A, s)
    net, _ = make_net(A, s, sd)
    x = torch.from_numpy(synth_input((8, 1, A * h, A * w), seed=3)).cuda()
    label = torch.from_numpy(synth_input((8, 1, A * h * s, A * w * s), seed=4)).cuda()
    _, b8, _ = hip_step(net, x, label)
    singles = torch.stack([hip_step(net, x[i:i + 1], label[i:i + 1])[1] for i in range(8)]).mean(0)
    for k, _ in net.named_parameters():
        off, n = net._spans[k]
        # both sides are fp32 sums in different orders (split counts differ with B): measured median 1.5e-5, worst 6.5e-5, and B = 8 and
        # the mean of the singles each sit ~2e-5 from fp64 on the worst parameter -- rounding, not a batch dependence
        assert rel(b8[off:off + n].cpu(), singles[off:off + n].cpu()) < 1e-4, k


def test_accumulation_and_zero_grad():
    case, sd, x, _ = model_case("LF_InterNet", "a5h8s2")        # (no ReLU decision of this case is within fp32 rounding of 0)
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    labels = [synth_input((B, 1, A * h * s, A * w * s), seed=sd_) for sd_ in (2, 5)]
    net, _ = make_net(A, s, sd)
    xg = torch.from_numpy(x).cuda()
    for p in net.parameters():
        p.grad = None
    for lab in labels:          # two micro-batches, accumulated into p.grad
        torch.nn.functional.l1_loss(net(xg), torch.from_numpy(lab).cuda()).backward()
    g1 = port_grads(sd, x, labels[0], A, s, torch.float32)[1]
    g2 = port_grads(sd, x, labels[1], A, s, torch.float32)[1]
    for k, p in net.named_parameters():
        assert rel(p.grad.cpu().numpy(), g1[k] + g2[k]) < 1e-4, k
    # zero_grad(set_to_none=False), then one backward: p.grad += into the zeroed tensors
    opt = torch.optim.SGD(net.parameters(), lr=0.0)
    opt.zero_grad(set_to_none=False)
    torch.nn.functional.l1_loss(net(xg), torch.from_numpy(labels[0]).cuda()).backward()
    for k, p in net.named_parameters():
        assert rel(p.grad.cpu().numpy(), g1[k]) < 1e-4, k


def test_stale_workspace_raises():
    case, sd, x, _ = model_case("LF_InterNet", "a3h6w8s4")
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    net, _ = make_net(A, s, sd)
    xg = torch.from_numpy(x).cuda()
    y1 = net(xg)
    y2 = net(xg)
    with pytest.raises(capi.LfsrError):
        y1.sum().backward()
    y2.sum().backward()


def test_inference_between_training_forward_and_backward():
    case, sd, x, _ = model_case("LF_InterNet", "a3h6w8s4")
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    net, _ = make_net(A, s, sd)
    xg = torch.from_numpy(x).cuda()
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).cuda()
    _, ref, _ = hip_step(net, xg, label)
    y = net(xg)
    with torch.no_grad():
        net(xg[:1])              # another shape: the inference workspace is replaced, the training one stays
    torch.nn.functional.l1_loss(y, label).backward()
    assert torch.equal(net.grad_bucket, ref)


def test_fused_adamw_steps_repack():
    from lfsr_amd.train_step import train_step
    case, sd, x, _ = model_case("LF_InterNet", "a3h6w8s4")
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
    ref = internet_forward(torch.from_numpy(x), upd, A, s).numpy()
    assert np.abs(y - ref).max() < 1e-4


def test_reference_loop_shape_amp_gradscaler_clip():
    A, s, h, w, B = 5, 2, 8, 8, 2
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
    A, s = 5, 2
    net, _ = make_net(A, s, spec_sd(A, s))
    h = w = 64
    B = ((1 << 31) - 1) // 320 // (A * A * h * w) + 1
    x = torch.zeros((B, 1, A * h, A * w), device="cuda")
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(capi.LfsrError):
        net(x)
    assert net._rt.train_workspace_bytes(B, h, w) == 0
    assert torch.cuda.memory_allocated() <= before + (64 << 20)     # (the weight repack only: no training workspace)
