"""What the LFSSR tests share: the state_dict contract, weights at which the network keeps its signal, the reference graph restated in torch
with named intermediates, and the fixtures of tests/golden/make_golden_lfssr.py.

Layouts.  The reference keeps its features as (B A^2, C, H, W) per-view images, image index (b A + u) A + v; ``lfssr_layers`` returns its
intermediates that way.  ``views_to_rows`` turns them into the library's VCL rows p = (((b A + u) A + v) H + y) W + x of C channels."""
import json
import os

import numpy as np

from lfsr_amd.synth import synth_input, synth_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HE_GAIN = float(np.sqrt(6.0))   # U(-b, b) with b = sqrt(6 / fan_in): the variance He's init gives a ReLU network

# tag -> (A, h, w, s, B): an interior view and a ragged pixel tile (64 pixels = 4 tiles of 16; 48; 35 = 2 tiles + 3), a batch boundary, and a grid of corners only
CASES = {"a5h8s4": (5, 8, 8, 4, 1), "a3h6w8s2": (3, 6, 8, 2, 2), "a2h5w7s4": (2, 5, 7, 4, 2)}
FULL = (5, 32, 32, 4, 1)
LAYER_NAMES = ("conv0", "alt1.0", "alt1", "fup1", "sr2x", "alt2", "fup2", "out")
# (A, s, B, h, w) and what each row reaches (tests/test_gpu_lfssr_geometries.py).  The angular kernel takes 16 consecutive pixels of one sample and a band of view rows:
# the whole grid up to angRes 5, 4 / 3 / 2 / 2 rows at 6 / 7 / 8 / 9; k_lfssr_conv0, k_lfssr_ps2 and k_lfssr_tail are launched on at most 8192 blocks of 256 threads
LFSSR_MATRIX = ((7, 2, 1, 5, 6),       # bands of 3 + 3 + 1 view rows; 30 pixels: one tile and a ragged one
                (9, 2, 1, 4, 4),       # largest angRes: bands of 2, the last band one row
                (8, 4, 1, 3, 5),       # bands of 2 that divide the grid; scale 4 on a banded grid, level-2 views of 6 x 10
                (6, 2, 2, 3, 3),       # bands of 4 + 2; a batch boundary on a banded grid; 9 pixels: less than one 16-pixel tile
                (4, 4, 2, 6, 5),       # even A, the widest grid that is one band; scale 4, B = 2
                (2, 2, 3, 9, 7),       # every view a corner; B = 3; odd ragged views
                (5, 4, 2, 8, 8),       # the benchmark's angRes at scale 4 with a batch boundary
                (3, 4, 1, 33, 28))     # views larger than 32x32; level 2 has 9 x 66 x 56 = 33,264 rows: k_lfssr_ps2 (x 64) and k_lfssr_tail (16 x 133,056) have 2,128,896
#                                        items each, past the 8192 x 256 = 2,097,152 threads of a capped launch -- the smallest shape at which both grid-stride loops take a
#                                        second, partial pass inside the model
GRID_CAP_ITEMS = 8192 * 256            # lfsr_cap_grid: past this many work items a thread of the three kernels above takes a second pass
# (A, s, B, h, w), layer -> the measured HIP / CPU-fp32 mean-error ratio of a layer that is inside the gate and above helpers.YARDSTICK for a reason of arithmetic by design
# (profiles/lfssr_geometry_tests.md); the gate admits no exception
LFSSR_YARDSTICK_EXEMPT = {}
STORED_FLOATS = 8192            # an intermediate's rows are stored every `stride`-th, so that no stored array is larger than this


def lfssr_spec(scale, n_layer=10):
    """(key, shape) in the order of the reference's state_dict (model/SR/LFSSR.py: net2x / net4x); the shapes do not depend on angRes"""
    spec = [("net.conv0.weight", (64, 1, 3, 3)), ("net.conv0.bias", (64,))]
    for level in ("1", "2")[:1 if scale == 2 else 2]:
        for i in range(n_layer):
            for conv in ("spaconv", "angconv"):
                spec += [(f"net.altblock{level}.{i}.{conv}.weight", (64, 64, 3, 3)), (f"net.altblock{level}.{i}.{conv}.bias", (64,))]
        spec += [(f"net.fup{level}.0.weight", (256, 64, 3, 3)), (f"net.fup{level}.0.bias", (256,)),
                 (f"net.res{level}.weight", (1, 64, 3, 3)), (f"net.res{level}.bias", (1,)),
                 (f"net.iup{level}.0.weight", (4, 1, 3, 3)), (f"net.iup{level}.0.bias", (4,))]
    return spec


def lfssr_state_dict(spec, seed=0):
    """synth weights with every 4-D weight of 64 input channels scaled by sqrt(6): LFSSR has no residual, and at the 1 / sqrt(fan_in) bound of
    ``synth_state_dict`` two different inputs leave altblock1 3e-8 apart -- a model-level test would pass with a broken data path"""
    sd = synth_state_dict(spec, seed)
    for k, v in sd.items():
        if v.ndim == 4 and v.shape[1] == 64:
            sd[k] = (v * np.float32(HE_GAIN)).astype(np.float32)
    return sd


def lfssr_case(tag):
    """-> (A, h, w, s, B), state_dict (numpy fp32), input mosaic (numpy fp32)"""
    A, h, w, s, B = FULL if tag == "full" else CASES[tag]
    return (A, h, w, s, B), lfssr_state_dict(lfssr_spec(s)), synth_input((B, 1, A * h, A * w), seed=1)


def lfssr_matrix_case(A, s, B, h, w):
    """a row of LFSSR_MATRIX -> state_dict (numpy fp32), input mosaic (numpy fp32): the weights and the input seed of lfssr_case"""
    return lfssr_state_dict(lfssr_spec(s)), synth_input((B, 1, A * h, A * w), seed=1)


def lfssr_meta():
    return json.load(open(os.path.join(GOLDEN, "lfssr.json")))


def lfssr_golden():
    return np.load(os.path.join(GOLDEN, "model_LFSSR.npz"))


def stored_stride(rows, ch):
    """the row stride at which an intermediate of (rows, ch) is stored: odd, so that it walks through every column of an even-width view"""
    st = -(-rows * ch // STORED_FLOATS)
    return st | 1 if st > 1 else 1


def views_to_rows(t):
    """(n_img, C, H, W) per-view images -> VCL rows (n_img H W, C)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def rows_to_views(r, n_img, H, W):
    return r.reshape(n_img, H, W, -1).permute(0, 3, 1, 2).contiguous()


def mosaic_to_views(x, A):
    """SAI mosaic (B, 1, A h, A w) -> (B A^2, 1, h, w)"""
    B, _, Hh, Ww = x.shape
    h, w = Hh // A, Ww // A
    return x.reshape(B, A, h, A, w).permute(0, 1, 3, 2, 4).reshape(B * A * A, 1, h, w).contiguous()


def views_to_mosaic(t, B, A):
    n, _, H, W = t.shape
    return t.reshape(B, A, A, H, W).permute(0, 1, 3, 2, 4).reshape(B, 1, A * H, A * W).contiguous()


def spaconv(x, w, b=None):
    """per-view 3x3, zero pad 1: out[n,o,y,x] = sum_{c,dy,dx} w[o,c,dy+1,dx+1] x[n,c,y+dy,x+dx]; nine shifted products (the formula, not conv2d)"""
    import torch
    n, c, H, W = x.shape
    xp = torch.zeros((n, c, H + 2, W + 2), dtype=x.dtype)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    out = torch.zeros((n, w.shape[0], H, W), dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            out += torch.einsum("oc,nchw->nohw", w[:, :, ky, kx], xp[:, :, ky:ky + H, kx:kx + W])
    return out if b is None else out + b.view(1, -1, 1, 1)


def angconv(a, w, b, B, A):
    """the angular conv of the issue's formula on (B A^2, C, H, W): out[b,u,v] = bias + sum over the taps (du, dv) whose view (u+du, v+dv) lies in the grid
    of w[:, :, du+1, dv+1] applied to a[b,u+du,v+dv]; the first kernel axis pairs with u"""
    import torch
    n, c, H, W = a.shape
    g = a.reshape(B, A, A, c, H, W)
    out = torch.zeros((B, A, A, w.shape[0], H, W), dtype=a.dtype)
    for du in (-1, 0, 1):
        for dv in (-1, 0, 1):
            u0, u1, v0, v1 = max(0, -du), min(A, A - du), max(0, -dv), min(A, A - dv)
            if u1 <= u0 or v1 <= v0:
                continue
            out[:, u0:u1, v0:v1] += torch.einsum("oc,buvchw->buvohw", w[:, :, du + 1, dv + 1], g[:, u0 + du:u1 + du, v0 + dv:v1 + dv])
    return (out + b.view(1, 1, 1, -1, 1, 1)).reshape(n, w.shape[0], H, W)


def pixel_shuffle2(t):
    """(n, 4 C, H, W), channel 4 c + 2 i + j -> (n, C, 2 H, 2 W) at (2 y + i, 2 x + j)"""
    n, c4, H, W = t.shape
    return t.reshape(n, c4 // 4, 2, 2, H, W).permute(0, 1, 4, 2, 5, 3).reshape(n, c4 // 4, 2 * H, 2 * W).contiguous()


def lfssr_layers(x, sd, A, s, dtype=None, n_layer=10):
    """the LFSSR graph (issue formula; checked against the reference in tests/test_lfssr_reference.py) -> {name: tensor}: the LAYER_NAMES present at scale s,
    per-view images (B A^2, C, H, W) but for `out`, the SAI mosaic (B, 1, A s h, A s w)"""
    import torch
    dtype = dtype or torch.float64
    p = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}
    x = torch.from_numpy(np.asarray(x)).to(dtype)
    B = x.shape[0]
    lr = mosaic_to_views(x, A)
    L = {}
    f = torch.relu(spaconv(lr, p["net.conv0.weight"], p["net.conv0.bias"]))
    L["conv0"] = f
    lo = lr
    for level in ("1", "2")[:1 if s == 2 else 2]:
        for i in range(n_layer):
            pre = f"net.altblock{level}.{i}."
            a = torch.relu(spaconv(f, p[pre + "spaconv.weight"], p[pre + "spaconv.bias"]))
            f = torch.relu(angconv(a, p[pre + "angconv.weight"], p[pre + "angconv.bias"], B, A))
            if i == 0 and level == "1":
                L["alt1.0"] = f
        L["alt" + level] = f
        f = torch.relu(pixel_shuffle2(spaconv(f, p[f"net.fup{level}.0.weight"], p[f"net.fup{level}.0.bias"])))
        L["fup" + level] = f
        res = spaconv(f, p[f"net.res{level}.weight"], p[f"net.res{level}.bias"])
        lo = res + pixel_shuffle2(spaconv(lo, p[f"net.iup{level}.0.weight"], p[f"net.iup{level}.0.bias"]))
        if level == "1":
            L["sr2x"] = lo
    L["out"] = views_to_mosaic(lo, B, A)
    return L
