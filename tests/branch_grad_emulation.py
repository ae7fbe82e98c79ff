"""The DistgSSR graph of oracle/lfsr_torch_port.py (distgssr_forward_graph, op for op) on leaf parameters the caller supplies, with EPIConv.0 of every block
replaced by an autograd function whose BACKWARD rounds what lfsr_set_branch_grad_arithmetic(LFSR_BRANCH_GRAD_ARITH_BF16) rounds: the CPU emulation of the mode,
the check made without a GPU that the whole-model gate of tests/test_gpu_branch_grad_bf16.py is one the arithmetic can meet.

Epi0Conv(t, w, A, r): the forward is the stock conv (the forward does not read the switch); the backward is
  dw = conv2d_weight(r(t), r(dE))      (csrc/epi0_grad_bf16.hip: the weight gradient)
  dt = conv2d_input(r(w), r(dE))       (the data gradient)
accumulated in the graph's dtype.  The rounding applies where the library's EPI-line kernels do (covered()): angRes 5 and lines of at most 32 pixels; elsewhere
the function is the stock conv in both directions.  Everything else of the graph is stock torch in the graph's dtype."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.lfsr_torch_port import macpi2sai, pixel_shuffle1d, sai2macpi

GEOMS = ((5, 2, 1, 8, 8), (3, 2, 2, 6, 8))      # (A, s, B, h, w): the whole-model geometries of the GPU test
EPI0_KEYS = tuple(f"disentg.Group.{g}.Block.{b}.EPIConv.0.weight" for g in range(4) for b in range(4))


def r_bf16(t):
    """round to bf16, nearest even, once; the value back in t's dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def covered(A, line_len):
    """where lfsr_epi0_dgrad_launch / lfsr_wgrad_epi0_launch take their EPI-line kernels (the whole-model geometries here have h, w <= 32)"""
    return A == 5 and line_len <= 32


class Epi0Conv(torch.autograd.Function):
    """1 x A^2 conv, stride (1, A), padding (0, A (A - 1) / 2), of a MacPI (or its transpose) t (B, 64, H, W A) with w (32, 64, 1, A^2)"""

    @staticmethod
    def forward(ctx, t, w, A, r):
        ctx.save_for_backward(t, w)
        ctx.cfg = (A, r)
        return F.conv2d(t, w, stride=(1, A), padding=(0, A * (A - 1) // 2))

    @staticmethod
    def backward(ctx, dE):
        t, w = ctx.saved_tensors
        A, r = ctx.cfg
        kw = dict(stride=(1, A), padding=(0, A * (A - 1) // 2))
        return torch.nn.grad.conv2d_input(t.shape, r(w), r(dE), **kw), torch.nn.grad.conv2d_weight(r(t), w.shape, r(dE), **kw), None, None


def distg_graph(x, p, A, s, r=None, seen=None, rec=None, force=None, n_group=4, n_block=4):
    """SAI mosaic x (B, 1, A h, A w), p: key -> leaf tensor -> the SR mosaic.  r is None: stock F.conv2d everywhere (what autocast sees); otherwise EPIConv.0 is
    Epi0Conv with r where covered().  seen: a list that receives the keys whose conv went through Epi0Conv.  rec / force: the LeakyReLU decisions, recorded / applied
    in order of evaluation (a list of boolean tensors): the same graph with another run's discrete decisions, which separates arithmetic error from flips at
    pre-activations within round-off of zero (tests/helpers.py: distg_forced_fp64_grads does the same for the GPU's)."""
    it = iter(force) if force is not None else None

    def lr(t):
        y = torch.where(next(it), t, 0.1 * t) if it is not None else F.leaky_relu(t, 0.1)
        if rec is not None:
            rec.append(y.detach() > 0)
        return y

    def block(t, pre):
        spa = lr(F.conv2d(t, p[pre + "SpaConv.0.weight"], dilation=A, padding=A))
        spa = lr(F.conv2d(spa, p[pre + "SpaConv.2.weight"], dilation=A, padding=A))
        ang = lr(F.conv2d(t, p[pre + "AngConv.0.weight"], stride=A))
        ang = F.pixel_shuffle(lr(F.conv2d(ang, p[pre + "AngConv.2.weight"])), A)

        def epi(u):
            key = pre + "EPIConv.0.weight"
            if r is not None and covered(A, u.shape[3] // A):
                if seen is not None:
                    seen.append(key)
                e = lr(Epi0Conv.apply(u, p[key], A, r))
            else:
                e = lr(F.conv2d(u, p[key], stride=(1, A), padding=(0, A * (A - 1) // 2)))
            return pixel_shuffle1d(lr(F.conv2d(e, p[pre + "EPIConv.2.weight"])), A)
        epih = epi(t)
        epiv = epi(t.permute(0, 1, 3, 2).contiguous()).permute(0, 1, 3, 2)
        buf = lr(F.conv2d(torch.cat((spa, ang, epih, epiv), dim=1), p[pre + "fuse.0.weight"]))
        return F.conv2d(buf, p[pre + "fuse.2.weight"], dilation=A, padding=A) + t

    x_up = F.interpolate(x, scale_factor=s, mode="bilinear", align_corners=False)
    buf0 = F.conv2d(sai2macpi(x, A), p["init_conv.weight"], dilation=A, padding=A)
    buf = buf0
    for g in range(n_group):
        gin = buf
        for b in range(n_block):
            buf = block(buf, f"disentg.Group.{g}.Block.{b}.")
        buf = F.conv2d(buf, p[f"disentg.Group.{g}.conv.weight"], dilation=A, padding=A) + gin
    buf = F.conv2d(buf, p["disentg.conv.weight"], dilation=A, padding=A) + buf0
    up = F.conv2d(macpi2sai(buf, A), p["upsample.0.weight"], p["upsample.0.bias"])
    return F.conv2d(F.pixel_shuffle(up, s), p["upsample.2.weight"]) + x_up


def step_grads(sd, x, label, A, s, dtype=torch.float64, r=None, seen=None, rec=None, force=None, autocast=False):
    """one forward + L1 + backward on fresh leaves made from the numpy state_dict -> (output, {key: gradient as an fp64 numpy array})"""
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        y = distg_graph(torch.from_numpy(x).to(dtype), p, A, s, r, seen, rec, force)
        loss = F.l1_loss(y.to(dtype), torch.from_numpy(label).to(dtype))
    loss.backward()
    return y.detach(), {k: v.grad.double().numpy() for k, v in p.items()}


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / max(np.linalg.norm(b), 1e-300))


def report(A, s, B, h, w):
    """-> (names, e_mode, e_amp): per-parameter rel-L2 error against fp64 autograd of the emulated mode (fp32 graph under fp64's LeakyReLU decisions, EPIConv.0's
    backward on bf16-rounded operands) and of the port under torch.autocast("cpu", bfloat16)"""
    from lfsr_amd.synth import synth_input
    from tests.helpers import distg_case, distg_spec
    sd, x = distg_case(A, s, B, h, w)
    label = synth_input((B, 1, A * h * s, A * w * s), seed=2)
    names = [k for k, _ in distg_spec(A, s)]
    masks = []
    _, g64 = step_grads(sd, x, label, A, s, rec=masks)
    _, gmode = step_grads(sd, x, label, A, s, dtype=torch.float32, r=r_bf16, force=masks)
    _, gamp = step_grads(sd, x, label, A, s, dtype=torch.float32, autocast=True)
    return names, {k: rel_l2(gmode[k], g64[k]) for k in names}, {k: rel_l2(gamp[k], g64[k]) for k in names}


if __name__ == "__main__":
    for geom in GEOMS:
        names, e, e_amp = report(*geom)
        kmin = min(names, key=lambda k: e_amp[k] / max(e[k], 1e-30))
        print(f"{geom}: emulated mode max {max(e.values()):.2e}, autocast min {min(e_amp.values()):.2e}, smallest autocast / mode ratio "
              f"{e_amp[kmin] / max(e[kmin], 1e-30):.2f} ({kmin})")
