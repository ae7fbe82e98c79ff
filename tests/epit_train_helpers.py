"""Helper of tests/test_gpu_epit_train.py (no tests here): the reference graph of EPIT in fp64 with the HIP path's ReLU / LeakyReLU decisions.

A pre-activation within fp32 rounding of 0 is a legitimate tie whose two sides have different gradients downstream (one flipped pixel moves the
gradient of a small case by ~1e-3).  To judge the kernels' arithmetic apart from such ties, epit_forced_fp64_grads runs fp64 autograd of
oracle.lfsr_torch_port.epit_forward with every one of its 34 activation decisions taken from what the HIP path computed (lfsr_epit_train_saved,
read after the backward): 3 in conv_init; per block and pass the feed-forward ReLU, conv.0 and conv.2; the tail's HR LeakyReLU.  The sign of
the L1 loss's gradient is taken from the HIP output as well."""
import torch

from oracle import lfsr_torch_port as P


class _ForcedF:
    """stands in for torch.nn.functional inside the port: relu / leaky_relu take their decisions from `masks`, in call order"""

    def __init__(self, masks):
        self._masks, self._next, self.flips = masks, 0, 0

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    def _act(self, z, slope):
        m = self._masks[self._next]
        self._next += 1
        assert m.shape == z.shape, (self._next, tuple(m.shape), tuple(z.shape))
        self.flips += int((m != (z > 0)).sum())
        return torch.where(m, z, z * slope)

    def relu(self, z, *a, **k):
        return self._act(z, 0.0)

    def leaky_relu(self, z, slope=0.01, *a, **k):
        return self._act(z, slope)


def epit_hip_masks(rt, xg, A, s, nblk=5):
    """the 34 decision tensors of the HIP path (value > 0), in the order and layout in which the port's graph takes them"""
    B, h, w = xg.shape[0], xg.shape[2] // A, xg.shape[3] // A

    def rows(which, index, C):
        return (rt.train_saved(xg, which, index) > 0).cpu().reshape(B, A, A, h, w, C)          # b u v y x c

    views = lambda t: t.permute(0, 5, 1, 2, 3, 4).reshape(B, -1, A * A, h, w)                   # (b, c, views, h, w)
    masks = [views(rows(1, 0, 64)), views(rows(1, 1, 64)), views(rows(5, 0, 64))]
    for b in range(nblk):
        for vert in (0, 1):
            j = 2 * b + vert
            hid = rows(4, j, 256)
            if not vert:
                masks.append(hid.permute(1, 3, 0, 2, 4, 5).reshape(A * h, B * A * w, 256))      # tokens (u y), sequences (b v x)
            else:
                masks.append(hid.permute(2, 4, 0, 1, 3, 5).reshape(A * w, B * A * h, 256))      # tokens (v x), sequences (b u y)
            masks += [views(rows(2, j, 64)), views(rows(3, j, 64))]
    hr = (rt.train_saved(xg, 6, 0) > 0).cpu().reshape(B, A * h * s, A * w * s, 64)
    masks.append(hr.permute(0, 3, 1, 2))
    return masks


def epit_forced_fp64_grads(rt, xg, sd, x, label, A, s):
    """-> ({name: fp64 gradient}, number of the HIP path's decisions that differ from fp64's own).  Call after the HIP backward of xg."""
    masks = epit_hip_masks(rt, xg, A, s)
    out_hip = rt.forward(xg).cpu().double()                  # bit-equal to the training forward's output; runs in the inference workspace
    lab = torch.as_tensor(label, dtype=torch.float64)
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
    forced, real = _ForcedF(masks), P.F
    P.F = forced
    try:
        y = P.epit_forward.__wrapped__(torch.as_tensor(x, dtype=torch.float64), p, A, s)
    finally:
        P.F = real
    assert forced._next == len(masks) == 34
    ((y * torch.sign(out_hip - lab)).sum() / y.numel()).backward()
    return {k: v.grad.numpy() for k, v in p.items()}, forced.flips
