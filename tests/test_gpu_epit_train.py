"""GPU: EPIT training through the HIP path (lfsr_epit_forward_train / _backward, the whole-model autograd node of lfsr_amd.hip_model), case for
case what tests/test_gpu_lft_train.py holds for LFT, plus what is EPIT's own: the weights an AltFilter shares between its two passes, and the
geometry whose vertical pass runs the VALU attention backward while its horizontal pass runs the matrix-pipe kernel.

The criterion is a local L1: the reference's get_loss indexes out['SR'] on a tensor (EPIT.py:178) and the plugin keeps that verbatim.

Gates.  Measured on the CPU at seven geometries (the three golden tags, A5 s2 B2 8x12, A3 s4 B2 6x8, A3 s2 B1 20x8, A5 s4 B1 16x16): the reference's
fp32 gradients are within 1.2e-6 (rel-L2 per parameter) of fp64 autograd with the same ReLU / LeakyReLU decisions, and up to 2.2e-3 from free
fp64, from 1-3 flipped decisions in 3.7-32 M.  So 1e-4 against the forced-fp64 gradients leaves two orders of magnitude for kernel round-off,
and the 1e-2 gate that applies where a decision flipped about 5x."""
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

from lfsr_amd import capi
from lfsr_amd.synth import synth_input, synth_state_dict
from oracle import lfsr_torch_port as P
from tests.epit_train_helpers import epit_forced_fp64_grads
from tests.helpers import GOLDEN, model_case

pytestmark = pytest.mark.gpu
TAGS = ("a5h8s4", "a3h6w8s2", "a3h6w8s3")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def make_net(A, s, sd=None):
    from lfsr_amd.model.SR import EPIT as M
    net = M.get_model(Namespace(angRes_in=A, angRes_out=A, scale_factor=s))
    if sd is not None:
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return net.cuda(), M


def spec_sd(A, s, seed=0):
    net, _ = make_net(A, s)
    return synth_state_dict([(k, tuple(v.shape)) for k, v in net.state_dict().items()], seed)


def l1(out, label, info=None):
    """the criterion a caller brings: the plugin's get_loss keeps the reference's quirk"""
    return torch.nn.functional.l1_loss(out, label)


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
    out = P.epit_forward.__wrapped__(torch.as_tensor(x).to(dtype), params, A, s)
    loss = torch.nn.functional.l1_loss(out, torch.as_tensor(label).to(dtype))
    loss.backward()
    return float(loss.detach()), {k: p.grad.numpy() for k, p in params.items()}


def forced_fp64_grads(rt, xg, sd, x, label, A, s):
    """fp64 autograd of the reference graph with every ReLU / LeakyReLU decision taken from what the HIP path computed, and the number of
    those decisions that differ from fp64's own: tests/epit_train_helpers.py::epit_forced_fp64_grads"""
    return epit_forced_fp64_grads(rt, xg, sd, x, label, A, s)


def check_against_port(net, bucket, ref):
    errs = []
    for k, _ in net.named_parameters():
        off, n = net._spans[k]
        errs.append(rel(bucket[off:off + n].cpu().numpy().reshape(ref[k].shape), ref[k]))
    errs = np.array(errs)
    return float(np.median(errs)), float(errs.max())


@pytest.mark.parametrize("tag", TAGS)
def test_grads_match_reference_golden(tag):
    npz = np.load(os.path.join(GOLDEN, "epit_grads.npz"))
    names = json.load(open(os.path.join(GOLDEN, "epit_grads.json")))["tags"][tag]["names"]
    case, sd, x, _ = model_case("EPIT", tag)
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
def test_grads_match_fp64_port_and_bucket(tag):
    case, sd, x, _ = model_case("EPIT", tag)
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
    assert med <= 5e-5 and mx < 1e-4      # per parameter (tests/test_gpu_epit_geometries.py holds every row of its matrix to the same)
    assert mx0 <= 1e-2
    cat = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    assert torch.equal(cat, net.grad_bucket)


def test_baseline_geometry_against_fp64():
    A, s, B, h, w = 5, 4, 1, 32, 32
    sd = spec_sd(A, s)
    net, _ = make_net(A, s, sd)
    x = synth_input((B, 1, A * h, A * w), seed=1)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    xg = torch.from_numpy(x).cuda()
    _, bucket, _ = hip_step(net, xg, torch.from_numpy(label).cuda())
    forced, flips = forced_fp64_grads(net._rt, xg, sd, x, label, A, s)
    med, mx = check_against_port(net, bucket, forced)
    print(f"BASELINE 5x5 32x32 x4: rel-L2 vs fp64 with the HIP decisions median {med:.2e} max {mx:.2e} ({flips} decisions differ)")
    assert med <= 5e-5 and mx < 1e-4      # per parameter


def test_scale3_grads_match_fp64_port_and_bucket():
    """s = 3: the training forward's two-kernel tail, the tail backward with s^2 = 9 (its element-wise store branch) and the upsampling.0 dgrad pack with s2 = 9; every parameter's
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
    ref_out = P.epit_forward.__wrapped__(torch.as_tensor(x).double(), {k: torch.tensor(v, dtype=torch.float64) for k, v in sd.items()}, A, s)
    assert float((out.cpu().double() - ref_out).abs().max()) < 1e-4


@pytest.mark.parametrize("arith", ["default", "f32"])
def test_train_forward_output_bit_equal_to_inference(arith):
    case, sd, x, _ = model_case("EPIT", "a3h6w8s2")
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
    case, sd, x, _ = model_case("EPIT", "a5h8s4")
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    net, _ = make_net(A, s, sd)
    label = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).cuda()
    xg = torch.from_numpy(x).cuda()
    _, b1, _ = hip_step(net, xg, label)
    _, b2, _ = hip_step(net, xg, label)
    assert torch.equal(b1, b2)


DECISIONS = [(1, 0), (1, 1), (5, 0), (6, 0)] + [(k, j) for k in (2, 3, 4) for j in range(10)]   # lfsr_epit_train_saved: all 34


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
    # the parameters below it move by ~1e-3 in a case this small, as against fp64 (see the golden test): then the gate is the fp64 one
    if flips == 0:
        assert errs.max() < 1e-4
    else:
        assert np.median(errs) <= 1e-3 and errs.max() <= 1e-2


def test_accumulation_and_zero_grad():
    case, sd, x, _ = model_case("EPIT", "a3h6w8s2")
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
    case, sd, x, _ = model_case("EPIT", "a5h8s4")
    net, _ = make_net(case["A"], case["s"], sd)
    xg = torch.from_numpy(x).cuda()
    y1 = net(xg)
    y2 = net(xg)
    with pytest.raises(capi.LfsrError):
        y1.sum().backward()
    y2.sum().backward()


def test_inference_between_training_forward_and_backward():
    case, sd, x, _ = model_case("EPIT", "a5h8s4")
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
    case, sd, x, _ = model_case("EPIT", "a3h6w8s2")
    A, h, w, s, B = case["A"], case["h"], case["w"], case["s"], case["B"]
    net, _ = make_net(A, s, sd)
    crit = l1
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, fused=True)
    xg = torch.from_numpy(x).cuda()
    lg = torch.from_numpy(synth_input((B, 1, A * h * s, A * w * s), seed=2)).cuda()
    for _ in range(2):
        train_step(net, crit, opt, xg, lg)
    with torch.no_grad():
        y = net(xg).cpu().numpy()
    upd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    assert any(not np.array_equal(upd[k].numpy(), sd[k]) for k in sd)
    ref = P.epit_forward(torch.from_numpy(x), upd, A, s).numpy()
    assert np.abs(y - ref).max() < 1e-4


def test_train_step_runs():
    from lfsr_amd.train_step import train_step
    A, s, h, w, B = 5, 4, 8, 8, 2
    net, _ = make_net(A, s, spec_sd(A, s))
    crit = l1
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
    net, _ = make_net(A, s, spec_sd(A, s))
    crit = l1
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


def _case(A, s, B, h, w):
    sd = spec_sd(A, s)
    net, _ = make_net(A, s, sd)
    x = synth_input((B, 1, A * h, A * w), seed=1)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    return sd, net, x, label


def test_fallback_geometry_valu_vertical_mfma_horizontal():
    """A = 5, x2, B = 1, LR views of 8 x 36.  Horizontal pass: sequences of A h = 40 tokens, on k_epi_attn_bwd_mfma.  Vertical pass: A w = 180 > 160, which the
    matrix-pipe kernel refuses, on the VALU pair.  The gates of the golden test."""
    A, s, B, h, w = 5, 2, 1, 8, 36
    sd, net, x, label = _case(A, s, B, h, w)
    xg = torch.from_numpy(x).cuda()
    hip_step(net, xg, torch.from_numpy(label).cuda())
    forced, flips = forced_fp64_grads(net._rt, xg, sd, x, label, A, s)
    _, ref = port_grads(sd, x, label, A, s)
    errs = {k: rel(p.grad.detach().cpu().numpy(), forced[k]) for k, p in net.named_parameters()}
    errs0 = {k: rel(p.grad.detach().cpu().numpy(), ref[k]) for k, p in net.named_parameters()}
    print(f"8 x 36: rel-L2 vs fp64 with the HIP decisions max {max(errs.values()):.2e}; vs fp64 max {max(errs0.values()):.2e} ({flips} decisions differ)")
    assert max(errs.values()) < 1e-4, max(errs, key=errs.get)
    assert max(errs0.values()) < (1e-4 if flips == 0 else 1e-2), max(errs0, key=errs0.get)


@pytest.mark.parametrize("geom", [(5, 2, 1, 8, 8), (3, 2, 2, 6, 8), (3, 4, 1, 5, 12)], ids=["a5", "a3-runtime-n1", "a3-h-ne-w"])
def test_shared_weights_get_both_passes(geom):
    """one epi_trans and one conv stack serve both passes of an AltFilter: the gradient of a shared weight is the sum of the two contributions, which
    is what autograd of the reference graph returns.  Probe: conv.4.weight of a middle AltFilter; also at a run-time n1 (A = 3) and with h != w, where
    the two passes see sequences of different length."""
    A, s, B, h, w = geom
    sd, net, x, label = _case(A, s, B, h, w)
    xg = torch.from_numpy(x).cuda()
    hip_step(net, xg, torch.from_numpy(label).cuda())
    forced, flips = forced_fp64_grads(net._rt, xg, sd, x, label, A, s)
    for k in ("altblock.2.conv.4.weight", "altblock.2.epi_trans.linear_in.weight", "altblock.2.epi_trans.norm.weight"):
        g = dict(net.named_parameters())[k].grad.detach().cpu().numpy()
        e = rel(g, forced[k])
        print(f"{geom} {k}: rel-L2 vs fp64 with the HIP decisions {e:.2e} ({flips} decisions differ)")
        assert e < 1e-4, k
