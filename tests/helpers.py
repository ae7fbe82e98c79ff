import contextlib
import json
import os

import numpy as np

from lfsr_amd.synth import synth_input, synth_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def models_meta():
    return json.load(open(os.path.join(GOLDEN, "models.json")))


def model_case(name, tag):
    """-> (case dict, state_dict (numpy fp32), input (numpy fp32), golden arrays npz)"""
    meta = models_meta()["models"][name]
    case = meta["full"] if tag == "full" else meta["cases"][tag]
    sd = synth_state_dict([(k, tuple(s)) for k, s in case["spec"]], seed=0)
    x = synth_input((case["B"], 1, case["A"] * case["h"], case["A"] * case["w"]), seed=1)
    npz = np.load(os.path.join(GOLDEN, f"model_{name}.npz"))
    return case, sd, x, npz


def model_spec(name, A, s):
    """(key, shape) list of `name` at angRes A and scale s: the golden case with that angRes, with upsampling.0 (64 s^2 outputs: the one
    parameter whose shape follows the scale) resized"""
    case = next(c for c in models_meta()["models"][name]["cases"].values() if c["A"] == A)
    return [(k, (64 * s * s,) + tuple(sh[1:]) if k == "upsampling.0.weight" else tuple(sh)) for k, sh in case["spec"]]


@contextlib.contextmanager
def arithmetic(mode):
    """lfsr_set_arithmetic(mode) for the block, the default again after it (the setting is process-wide)"""
    from lfsr_amd import capi
    capi.set_arithmetic(mode)
    try:
        yield
    finally:
        capi.set_arithmetic(capi.ARITH_DEFAULT)


# switch -> (capi setter, capi getter, the name of capi's default value): the nine process-wide arithmetic selections
MODE_SWITCHES = {"arith": ("set_arithmetic", "get_arithmetic", "ARITH_DEFAULT"),
                 "grad": ("set_grad_arithmetic", "get_grad_arithmetic", "GRAD_ARITH_DEFAULT"),
                 "gemm": ("set_gemm_arithmetic", "get_gemm_arithmetic", "GEMM_ARITH_DEFAULT"),
                 "branch": ("set_branch_arithmetic", "get_branch_arithmetic", "BRANCH_ARITH_DEFAULT"),
                 "ang": ("set_ang_arithmetic", "get_ang_arithmetic", "ANG_ARITH_DEFAULT"),
                 "wide": ("set_wide_arithmetic", "get_wide_arithmetic", "WIDE_ARITH_DEFAULT"),
                 "lin_grad": ("set_lin_grad_arithmetic", "get_lin_grad_arithmetic", "LIN_GRAD_ARITH_DEFAULT"),
                 "wide_train": ("set_wide_train_arithmetic", "get_wide_train_arithmetic", "WIDE_TRAIN_ARITH_DEFAULT"),
                 "branch_grad": ("set_branch_grad_arithmetic", "get_branch_grad_arithmetic", "BRANCH_GRAD_ARITH_DEFAULT")}


@contextlib.contextmanager
def modes(**switches):
    """the given selections (keys of MODE_SWITCHES -> a value of that switch) for the block, every other one at its default; all nine are the default again after
    it, whatever the block did (the settings are process-wide)"""
    from lfsr_amd import capi
    unknown = set(switches) - set(MODE_SWITCHES)
    assert not unknown, unknown

    def reset():
        for setter, _, default in MODE_SWITCHES.values():
            getattr(capi, setter)(getattr(capi, default))
    try:
        reset()
        for k, v in switches.items():
            getattr(capi, MODE_SWITCHES[k][0])(v)
        yield
    finally:
        reset()


def modes_now():
    """{switch: the value the next launch runs in}"""
    from lfsr_amd import capi
    return {k: getattr(capi, getter)() for k, (_, getter, _) in MODE_SWITCHES.items()}


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return float("inf") if mse == 0 else 10.0 * np.log10(1.0 / mse)


# ---------------------------------------------------------------------------------------------------------------------
# LeakyReLU' masks of the DistgSSR training forward: the HIP path's saved activations (lfsr_distgssr_train_saved) <-> the layouts of the
# reference graph (oracle/lfsr_torch_port.py:distg_block's rec / force dictionaries)
# ---------------------------------------------------------------------------------------------------------------------
MASK_KINDS = ("S1", "S2", "A1", "A2", "EH1", "EH2", "EV1", "EV2", "FZ")
_SAVED = {"S1": (0, None), "S2": (1, (0, 64)), "A1": (2, None), "A2": (1, (64, 80)), "EH1": (3, None), "EH2": (1, (80, 112)),
          "EV1": (4, None), "EV2": (1, (112, 144)), "FZ": (5, None)}      # kind -> (which of lfsr_distgssr_train_saved, channel slice of the concat buffer)
_PERMS = {}


def mask_ref_shape(kind, B, A, h, w):
    return {"S1": (B, 64, h * A, w * A), "S2": (B, 64, h * A, w * A), "FZ": (B, 64, h * A, w * A), "OUT": (B, 64, h * A, w * A), "A1": (B, 16, h, w),
            "A2": (B, 16 * A * A, h, w),
            "EH1": (B, 32, h * A, w), "EH2": (B, 32 * A, h * A, w), "EV1": (B, 32, w * A, h), "EV2": (B, 32 * A, w * A, h)}[kind]


def _ref_to_hip(kind, t, B, A, h, w):
    """a tensor in the reference layout of `kind` -> flat, in the order the HIP path stores that activation"""
    import torch
    import torch.nn.functional as F

    def vcl(z):   # NCHW MacPI (B,C,h*A,w*A) -> [b][u][v][y][x][c]
        return z.reshape(B, z.shape[1], h, A, w, A).permute(0, 3, 5, 2, 4, 1).reshape(-1)

    def ps1d(z, f):   # DistgSSR.py:114-131 (factor-major channel order)
        Bz, fC, Hh, Ww = z.shape
        return z.reshape(Bz, f, fC // f, Hh, Ww).permute(0, 2, 3, 4, 1).reshape(Bz, fC // f, Hh, Ww * f)
    if kind in ("S1", "S2", "FZ", "OUT"):
        return vcl(t)
    if kind == "A1":
        return t.permute(0, 2, 3, 1).reshape(-1)
    if kind == "A2":
        return vcl(F.pixel_shuffle(t, A))
    if kind == "EH1":
        return t.reshape(B, 32, h, A, w).permute(0, 3, 2, 4, 1).reshape(-1)
    if kind == "EV1":
        return t.reshape(B, 32, w, A, h).permute(0, 3, 4, 2, 1).reshape(-1)
    if kind == "EH2":
        return vcl(ps1d(t, A))
    if kind == "EV2":
        return vcl(ps1d(t, A).permute(0, 1, 3, 2))
    raise KeyError(kind)


def mask_perm(kind, B, A, h, w):
    """perm with hip_flat[i] = ref_flat[perm[i]] (an index tensor pushed through the reference -> HIP layout map; cached)"""
    import torch
    key = (kind, B, A, h, w)
    if key not in _PERMS:
        shp = mask_ref_shape(kind, B, A, h, w)
        n = int(np.prod(shp))
        _PERMS[key] = _ref_to_hip(kind, torch.arange(n, dtype=torch.float64).reshape(shp), B, A, h, w).long()
    return _PERMS[key]


def hip_saved_mask(rt, x, kind, index):
    """LeakyReLU output signs (> 0) of block `index` as the HIP training forward saved them, flat in HIP order (CPU bool tensor)"""
    which, sl = _SAVED[kind]
    v = rt.train_saved(x, which, index)
    if sl is not None:
        v = v.reshape(-1, 144)[:, sl[0]:sl[1]]
    return (v > 0).reshape(-1).cpu()


def hip_mask_to_ref(mask_flat, kind, B, A, h, w):
    """the same mask in the reference graph's layout (what distg_block's `force` consumes)"""
    import torch
    shp = mask_ref_shape(kind, B, A, h, w)
    out = torch.empty(int(np.prod(shp)), dtype=torch.bool)
    out[mask_perm(kind, B, A, h, w)] = mask_flat
    return out.reshape(shp)


def ref_mask_to_hip(mask_ref, kind, B, A, h, w):
    return mask_ref.reshape(-1)[mask_perm(kind, B, A, h, w)]


# ---------------------------------------------------------------------------------------------------------------------
# LF_InterNet: the parameter table at any angRes / scale, the reference graph with every intermediate the HIP training forward saves
# (lfsr_internet_train_saved), and the maps between the graph's layouts and the HIP path's rows
# ---------------------------------------------------------------------------------------------------------------------
# (A, s, B, h, w) and what each row reaches
INTERNET_MATRIX = ((7, 2, 1, 5, 6),       # 49 gather taps, 3136 Ang2Spa GEMM columns, AngFE rows padded 49 -> 52
                   (2, 3, 2, 9, 7),       # even A (no centre view), scale 3, odd ragged views, AngFE rows 4 wide exactly
                   (4, 4, 1, 6, 5),       # even A, A^2 = 16, scale 4
                   (5, 3, 2, 13, 16),     # the benchmark's angRes at scale 3; 81.25 row tiles of 128 pixels, 3.25 tiles of LR pixels
                   (3, 2, 3, 33, 40),     # views larger than 32x32; 3960 LR pixels: the row-streaming GEMM forms in inference
                   (9, 2, 1, 4, 4),       # largest accepted angRes, AngFE rows padded 81 -> 84
                   (1, 2, 2, 8, 8),       # smallest accepted angRes: one gather tap
                   (5, 2, 3, 32, 32),     # SpaBottle's gather spans >= 2 GiB: 64-bit addresses
                   (5, 2, 8, 32, 32))     # SpaBottle and SpaConvSq on them: the published training geometry


def internet_spec(A, s, n_groups=4, n_layers=4):
    """(key, shape) list of LF_InterNet at angRes A and scale s: lfsr_internet_create's table (model/SR/LF_InterNet.py's state_dict)"""
    spec = [("AngFE.0.weight", (64, 1, A, A)), ("SpaFE.0.weight", (64, 1, 3, 3))]
    for g in range(n_groups):
        for l in range(n_layers):
            q = f"CascadeInterBlock.body.{g}.chained_layers.{l}."
            spec += [(q + "Spa2Ang.weight", (64, 64, A, A)), (q + "Ang2Spa.0.weight", (A * A * 64, 64, 1, 1)),
                     (q + "AngConvSq.weight", (64, 128, 1, 1)), (q + "SpaConvSq.weight", (64, 128, 3, 3))]
    spec += [("BottleNeck.AngBottle.weight", (64, 64 * n_groups, 1, 1)), ("BottleNeck.Ang2Spa.0.weight", (A * A * 64, 64, 1, 1)),
             ("BottleNeck.SpaBottle.weight", (64, 64 * (n_groups + 1), 3, 3)),
             ("ReconBlock.PreConv.weight", (64 * s * s, 64, 3, 3)), ("ReconBlock.FinalConv.weight", (1, 64, 1, 1))]
    return spec


def internet_case(A, s, B, h, w):
    """-> (state_dict, input): synth_state_dict seed 0 / synth_input seed 1, as the golden cases"""
    return synth_state_dict(internet_spec(A, s), seed=0), synth_input((B, 1, A * h, A * w), seed=1)


# kind -> (which of lfsr_internet_train_saved, channel slice of the 128-wide rows, layout, per chain layer)
INTERNET_SAVED = {"xs": (0, (0, 64), "vcl", True), "spa2": (0, (64, 128), "vcl", True), "xa": (1, (0, 64), "lr", True), "ang2": (1, (64, 128), "lr", True),
                  "relu_spa": (2, None, "vcl", True), "relu_ang": (3, None, "lr", True), "relu_spabottle": (4, None, "vcl", False),
                  "relu_angbottle": (5, None, "lr", False)}
INTERNET_RELU_KINDS = ("ang2", "relu_spa", "relu_ang", "relu_spabottle", "relu_angbottle")      # the tensors whose signs are ReLU decisions


def internet_keys():
    """every (kind, index) the training forward saves: 6 per chain layer x 16, and the BottleNeck's two"""
    return [(k, i) for k, (_, _, _, per) in INTERNET_SAVED.items() for i in (range(16) if per else (0,))]


def internet_ref_to_rows(t, layout, A):
    """reference layout -> the HIP path's rows x 64: MacPI (B,64,h*A,w*A) -> VCL [b][u][v][y][x][c]; (B,64,h,w) -> LR rows [b][y][x][c]"""
    B, Cc = t.shape[:2]
    if layout == "lr":
        return t.permute(0, 2, 3, 1).reshape(-1, Cc)
    h, w = t.shape[2] // A, t.shape[3] // A
    return t.reshape(B, Cc, h, A, w, A).permute(0, 3, 5, 2, 4, 1).reshape(-1, Cc)


def internet_rows_to_ref(v, layout, B, A, h, w):
    """the inverse: rows x 64 in HIP order -> the reference layout"""
    if layout == "lr":
        return v.reshape(B, h, w, -1).permute(0, 3, 1, 2)
    return v.reshape(B, A, A, h, w, -1).permute(0, 5, 3, 1, 4, 2).reshape(B, -1, h * A, w * A)


def internet_saved_rows(rt, xg, kind, index=0):
    """what forward_train(xg) saved for (kind, index), as rows x 64 in HIP order (a GPU tensor)"""
    which, sl, _, _ = INTERNET_SAVED[kind]
    v = rt.train_saved(xg, which, index)
    return v.reshape(-1, 64) if sl is None else v.reshape(-1, 128)[:, sl[0]:sl[1]]


def internet_hip_masks(rt, xg, A):
    """the ReLU decisions (> 0) of forward_train(xg), in the reference layouts: what internet_layers_fp64's `forced` takes"""
    B, h, w = xg.shape[0], xg.shape[2] // A, xg.shape[3] // A
    return {(k, i): internet_rows_to_ref((internet_saved_rows(rt, xg, k, i) > 0).cpu(), INTERNET_SAVED[k][2], B, A, h, w)
            for k, i in internet_keys() if k in INTERNET_RELU_KINDS}


def internet_layers_fp64(x, params, A, s, forced=None, dtype=None):
    """LF_InterNet's graph (model/SR/LF_InterNet.py:33-141) on stock torch CPU ops -> (output, layers, flips).
    layers[(kind, index)]: every tensor of INTERNET_SAVED in the reference layout (spatial: MacPI NCHW, angular: (B,64,h,w)).
    params: {key: tensor} (fp64 unless `dtype` says otherwise; they may require grad).  forced: {(kind, index): bool mask in the reference
    layout} for the five ReLU kinds -- the decisions are then the caller's, and flips counts those that differ from the graph's own."""
    import torch
    F = torch.nn.functional
    dtype = dtype or torch.float64
    p = {k: torch.as_tensor(v).to(dtype) for k, v in params.items()}
    xd = torch.as_tensor(x).to(dtype)
    B, _, Hh, Ww = xd.shape
    h, w = Hh // A, Ww // A
    L, flips = {}, 0

    def relu(z, key):
        nonlocal flips
        if forced is None:
            y = F.relu(z)
        else:
            m = forced[key]
            flips += int(((z > 0) != m).sum())
            y = z * m.to(z.dtype)
        L[key] = y
        return y
    m = xd.reshape(B, 1, A, h, A, w).permute(0, 1, 3, 2, 5, 4).reshape(B, 1, h * A, w * A)           # SAI2MacPI
    xa, xs = F.conv2d(m, p["AngFE.0.weight"], stride=A), F.conv2d(m, p["SpaFE.0.weight"], dilation=A, padding=A)
    ba, bs, oa_l, os_l = xa, xs, [], []
    for g in range(4):
        for l in range(4):
            q, i = f"CascadeInterBlock.body.{g}.chained_layers.{l}.", g * 4 + l
            L["xs", i], L["xa", i] = bs, ba
            ang2 = relu(F.conv2d(bs, p[q + "Spa2Ang.weight"], stride=A), ("ang2", i))
            spa2 = L["spa2", i] = F.pixel_shuffle(F.conv2d(ba, p[q + "Ang2Spa.0.weight"]), A)
            oa = relu(F.conv2d(torch.cat((ba, ang2), 1), p[q + "AngConvSq.weight"]), ("relu_ang", i)) + ba
            os_ = relu(F.conv2d(torch.cat((bs, spa2), 1), p[q + "SpaConvSq.weight"], dilation=A, padding=A), ("relu_spa", i)) + bs
            ba, bs = oa, os_
        oa_l.append(ba)
        os_l.append(bs)
    a = relu(F.conv2d(torch.cat(oa_l, 1), p["BottleNeck.AngBottle.weight"]), ("relu_angbottle", 0))
    cs = torch.cat((torch.cat(os_l, 1), F.pixel_shuffle(F.conv2d(a, p["BottleNeck.Ang2Spa.0.weight"]), A)), 1)
    out = relu(F.conv2d(cs, p["BottleNeck.SpaBottle.weight"], dilation=A, padding=A), ("relu_spabottle", 0)) + xs
    pre = F.conv2d(out, p["ReconBlock.PreConv.weight"], dilation=A, padding=A)
    pre = pre.reshape(B, pre.shape[1], h, A, w, A).permute(0, 1, 3, 2, 5, 4).reshape(B, pre.shape[1], A * h, A * w)      # MacPI2SAI
    y = F.conv2d(F.pixel_shuffle(pre, s), p["ReconBlock.FinalConv.weight"])
    return y, L, flips


def forced_fp64_grads(rt, xg, sd, x, label, A, s):
    """fp64 autograd of the reference graph with every ReLU decision taken from what the HIP training forward saved (lfsr_internet_train_saved),
    and the number of those decisions that differ from fp64's own.  A pre-activation within fp32 rounding of 0 (seen: -1.9e-8 in fp64,
    +8.6e-9 on the GPU) is a legitimate tie whose two sides have different gradients downstream; this graph makes the same choices."""
    import torch
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
    y, _, flips = internet_layers_fp64(x, p, A, s, forced=internet_hip_masks(rt, xg, A))
    torch.nn.functional.l1_loss(y, torch.as_tensor(label, dtype=torch.float64)).backward()
    return {k: v.grad.numpy() for k, v in p.items()}, flips


# ---------------------------------------------------------------------------------------------------------------------
# LFT: the geometry matrix, the reference graph with every tensor lfsr_lft_train_saved can return, and the maps between the graph's
# layouts and the HIP path's rows
# ---------------------------------------------------------------------------------------------------------------------
# (A, s, B, h, w) and what each row reaches.  w <= h + 2 everywhere: the reference clamps the column window with h (LFT.py:168), so at
# w >= h + 3 the last columns' queries have no key; the numpy oracle then returns NaN (softmax over an all -inf row) while torch's SDPA on
# the CPU does not, and there is no reference to compare with.
LFT_MATRIX = ((7, 2, 1, 5, 6),        # 49 angular tokens on k_window_attn_lds<8, 8>; odd A other than 3, 5
              (2, 3, 2, 9, 7),        # even A, scale 3, h > w, odd ragged view
              (4, 4, 1, 6, 8),        # even A, scale 4, w = h + 2: the widest view the reference's clamp leaves without an empty window
              (8, 2, 1, 4, 5),        # A^2 = 64: the upper bound of the LDS angular kernel
              (9, 2, 1, 4, 4),        # A^2 = 81: the generic k_window_attn<8>
              (15, 2, 1, 3, 4),       # largest accepted angRes (225 tokens, 225 position-embedding rows)
              (1, 2, 2, 8, 8),        # smallest: one-token angular attention
              (5, 3, 2, 13, 15),      # the benchmark's angRes at scale 3; npix 9 750: k_tail_bwd loops with s^2 = 9; w = h + 2 at A = 5
              (3, 2, 1, 40, 36),      # views wider than 32: spatial attention off the 5x5 MFMA kernel, several conv tiles per row, fwd and bwd
              (5, 4, 8, 32, 32))      # the published training geometry: the ragged weight-gradient splits and the grid-stride loops of k_ew

# which of lfsr_lft_train_saved -> (layout, floats per row, number of indices); 0-5 are there after forward_train, 6-9 after backward
LFT_SAVED = {0: ("vcl", 64, 5), 1: ("ang", 64, 4), 2: ("spa", 128, 4), 3: ("spa", 128, 4), 4: ("spa", 128, 4), 5: ("vcl", 64, 2),
             6: ("ang", 128, 4), 7: ("spa", 256, 4), 8: ("vcl", 64, 1), 9: ("hr", 64, 1)}
LFT_DECISION_KINDS = (5, 6, 7, 8, 9)      # the tensors whose signs are ReLU / LeakyReLU decisions
LFT_PER_SAMPLE_NPIX = 50000               # above this many LR pixels the fp64 work is done one sample at a time (dense masked attention)


def lft_keys(kinds=tuple(LFT_SAVED)):
    """every (which, index) of `kinds`: 23 after forward_train and 10 more after backward"""
    return [(k, i) for k in kinds for i in range(LFT_SAVED[k][2])]


def lft_case(A, s, B, h, w):
    """-> (state_dict, input): synth_state_dict seed 0 / synth_input seed 1, as the golden cases.  LFT's parameter shapes do not depend on
    angRes (tests/test_lft_reference.py asserts it), so the golden angRes-5 spec serves every A"""
    return synth_state_dict(model_spec("LFT", 5, s), seed=0), synth_input((B, 1, A * h, A * w), seed=1)


def lft_ref_to_rows(t, layout, B):
    """reference layout -> the HIP path's rows [b][u][v][y][x][c] (VCL).  vcl: (B, c, A^2, h, w); ang: AngTrans tokens (A^2, B h w, c);
    spa: SpaTrans tokens (h w, B A^2, c); hr: (B, 64, A h s, A w s) -> the channel-last mosaic's rows"""
    if layout == "vcl":
        return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])
    if layout == "ang":
        return t.reshape(t.shape[0], B, -1, t.shape[2]).permute(1, 0, 2, 3).reshape(-1, t.shape[2])
    if layout == "spa":
        return t.permute(1, 0, 2).reshape(-1, t.shape[2])
    if layout == "hr":
        return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    raise KeyError(layout)


def lft_rows_to_ref(v, layout, B, A, h, w, s=1):
    """the inverse: flat values in HIP order -> the reference layout"""
    AA = A * A
    if layout == "vcl":
        return v.reshape(B, AA, h, w, -1).permute(0, 4, 1, 2, 3)
    if layout == "ang":
        c = v.numel() // (B * AA * h * w)
        return v.reshape(B, AA, h * w, c).permute(1, 0, 2, 3).reshape(AA, B * h * w, c)
    if layout == "spa":
        return v.reshape(B * AA, h * w, -1).permute(1, 0, 2)
    if layout == "hr":
        return v.reshape(B, A * h * s, A * w * s, 64).permute(0, 3, 1, 2)
    raise KeyError(layout)


def lft_saved_rows(rt, xg, kind, index=0):
    """what forward_train(xg) (kinds 0-5) or the backward after it (6-9) left for (kind, index), as rows in HIP order (a GPU tensor)"""
    return rt.train_saved(xg, kind, index).reshape(-1, LFT_SAVED[kind][1])


def lft_hip_masks(rt, xg, A, s, sample=None):
    """the ReLU / LeakyReLU decisions (> 0) the HIP path took, read after its backward, in the reference layouts: what lft_layers_fp64's
    `forced` takes.  sample = i: the decisions of sample i alone, as a B = 1 graph takes them (rows are sample-major)"""
    B, h, w = xg.shape[0], xg.shape[2] // A, xg.shape[3] // A
    out = {}
    for k, i in lft_keys(LFT_DECISION_KINDS):
        m = (lft_saved_rows(rt, xg, k, i) > 0).cpu()
        if sample is not None:
            n = m.shape[0] // B
            m = m[sample * n:(sample + 1) * n]
        out[k, i] = lft_rows_to_ref(m, LFT_SAVED[k][0], B if sample is None else 1, A, h, w, s)
    return out


def lft_position_encoding(lengths, dim, temperature=10000):
    """PositionEncoding.forward LFT.py:106-130 in fp64 (sin of the even columns then cos of the odd ones, concatenated)"""
    import torch
    grid = torch.arange(dim, dtype=torch.float64)
    grid = temperature ** (2 * torch.div(grid, 2, rounding_mode="floor") / dim)
    out = []
    for n in lengths:
        pos = torch.arange(n, dtype=torch.float64).view(-1, 1) / grid
        out.append(torch.cat([pos[:, 0::2].sin(), pos[:, 1::2].cos()], dim=1))
    return out


def lft_layers_fp64(x, params, A, s, forced=None, dtype=None):
    """LFT's graph (model/SR/LFT.py:67-98, as oracle/lfsr_torch_port.py::lft_forward states it) on stock torch CPU ops, fp64 throughout
    including the position encodings -> (output, layers, flips).
    layers[(which, index)]: every tensor lfsr_lft_train_saved can return, detached, in the reference's layout (LFT_SAVED; lft_ref_to_rows).
    params: {key: tensor} (fp64 unless `dtype` says otherwise; they may require grad).  forced: {(which, index): bool mask in the reference
    layout} for LFT_DECISION_KINDS -- the decisions are then the caller's, and flips counts those that differ from the graph's own."""
    import torch
    F = torch.nn.functional
    dtype = dtype or torch.float64
    p = {k: torch.as_tensor(v).to(dtype) for k, v in params.items()}
    xd = torch.as_tensor(x).to(dtype)
    B, _, Hh, Ww = xd.shape
    h, w, AA = Hh // A, Ww // A, A * A
    L, flips = {}, 0

    def act(z, key, slope, keep_pre=False):
        nonlocal flips
        if forced is None:
            y = F.leaky_relu(z, slope) if slope else F.relu(z)
        else:
            m = forced[key]
            flips += int(((z > 0) != m).sum())
            y = torch.where(m, z, z * slope)
        L[key] = (z if keep_pre else y).detach()
        return y

    def conv133(z, wt):       # nn.Conv3d(k=(1,3,3), pad=(0,1,1), bias=False)
        return F.conv3d(z, wt, padding=(0, 1, 1))

    def mha(qk, v, pre, mask=None):      # nn.MultiheadAttention(need_weights=False), (L, N, E), 8 heads, no biases
        in_w, out_w = p[pre + "attention.in_proj_weight"], p[pre + "attention.out_proj.weight"]
        Ln, N, E = qk.shape
        heads = lambda z: z.reshape(Ln, N * 8, E // 8).transpose(0, 1)
        o = F.scaled_dot_product_attention(heads(F.linear(qk, in_w[:E])), heads(F.linear(qk, in_w[E:2 * E])), heads(F.linear(v, in_w[2 * E:])),
                                           attn_mask=mask)
        return F.linear(o.transpose(0, 1).reshape(Ln, N, E), out_w)

    def ffn(tok, pre, key):
        ff = F.layer_norm(tok, tok.shape[-1:], p[pre + "feed_forward.0.weight"], p[pre + "feed_forward.0.bias"])
        return F.linear(act(F.linear(ff, p[pre + "feed_forward.1.weight"]), key, 0.0), p[pre + "feed_forward.4.weight"]) + tok
    # the views and their bicubic skip (LFT.py:263-273)
    lr = xd.reshape(B, 1, A, h, A, w).permute(0, 1, 2, 4, 3, 5)
    skip = F.interpolate(lr.reshape(B * AA, 1, h, w), scale_factor=s, mode="bicubic", align_corners=False)
    skip = skip.reshape(B, 1, A, A, h * s, w * s).permute(0, 1, 2, 4, 3, 5).reshape(B, 1, A * h * s, A * w * s)
    buf = conv133(lr.reshape(B, 1, AA, h, w), p["conv_init0.0.weight"])
    t = act(conv133(buf, p["conv_init.0.weight"]), (5, 0), 0.2)
    t = act(conv133(t, p["conv_init.2.weight"]), (5, 1), 0.2)
    buf = act(conv133(t, p["conv_init.4.weight"]), (8, 0), 0.2) + buf
    c = buf.shape[1]
    ph, pw, pa = (e.to(dtype) for e in lft_position_encoding([h, w, AA], c))
    spa_pos = ((ph[:, None, :] + pw[None, :, :]) / 2).permute(2, 0, 1).reshape(1, c, 1, h, w)
    # SpaTrans.gen_mask LFT.py:161-174: 5x5 window, the column clamp uses h
    i_, j_ = torch.arange(h).view(h, 1, 1, 1), torch.arange(w).view(1, w, 1, 1)
    ii, jj = torch.arange(h).view(1, 1, h, 1), torch.arange(w).view(1, 1, 1, w)
    ok = (ii >= i_ - 2) & (ii < i_ + 3) & (jj >= j_ - 2) & (jj < torch.clamp(j_ + 3, max=h))
    mask = torch.full((h, w, h, w), float("-inf"), dtype=dtype)
    mask[ok] = 0.0
    mask = mask.reshape(h * w, h * w)
    t = buf
    nblk = 1 + max(int(k.split(".")[1]) for k in p if k.startswith("altblock."))
    for i in range(nblk):
        L[0, i] = t.detach()
        pre = f"altblock.{i}.ang_trans."          # AngTrans LFT.py:233-246
        tok = t.permute(2, 0, 3, 4, 1).reshape(AA, B * h * w, c)
        tn = F.layer_norm(tok + pa.reshape(AA, 1, c), (c,), p[pre + "norm.weight"], p[pre + "norm.bias"])
        tok = mha(tn, tok, pre) + tok
        L[1, i] = tok.detach()
        tok = ffn(tok, pre, (6, i))
        t = tok.reshape(AA, B, h, w, c).permute(1, 4, 0, 2, 3)
        pre = f"altblock.{i}.spa_trans."          # SpaTrans LFT.py:188-203
        wm = p[pre + "MLP.weight"]

        def sai2token(z):   # F.unfold(k3, pad 1) + Linear(576 -> 128), LFT.py:176-182
            n = z.shape[0] * z.shape[2]
            u = F.unfold(z.permute(0, 2, 1, 3, 4).reshape(n, c, h, w), kernel_size=3, padding=1)   # (n, 576, h w)
            return F.linear(u.permute(2, 0, 1), wm)
        tok = sai2token(t)
        L[3, i] = tok.detach()
        tn = F.layer_norm(tok + sai2token(spa_pos), tok.shape[-1:], p[pre + "norm.weight"], p[pre + "norm.bias"])
        tok = mha(tn, tok, pre, mask) + tok
        L[2, i] = tok.detach()
        tok = ffn(tok, pre, (7, i))
        L[4, i] = tok.detach()
        t = F.conv3d(tok.reshape(h, w, B, AA, -1).permute(2, 4, 3, 0, 1), p[pre + "linear.0.weight"])
    t = t + buf
    L[0, nblk] = t.detach()
    mosaic = t.reshape(B, c, A, A, h, w).permute(0, 1, 2, 4, 3, 5).reshape(B, c, A * h, A * w)
    up = F.pixel_shuffle(F.conv2d(mosaic, p["upsampling.0.weight"]), s)
    y = F.conv2d(act(up, (9, 0), 0.2, keep_pre=True), p["upsampling.3.weight"], padding=1) + skip
    return y, L, flips


def lft_forced_fp64_grads(rt, xg, sd, x, label, A, s):
    """fp64 autograd of lft_layers_fp64 under L1 `mean` loss with every ReLU / LeakyReLU decision taken from what the HIP path computed
    (lfsr_lft_train_saved, read after the backward), and the number of those decisions that differ from fp64's own.  A pre-activation within
    fp32 rounding of 0 is a legitimate tie whose two sides have different gradients downstream (one flipped tail pixel moves the gradient of
    a small case by ~1e-3); this graph makes the same choices.  Large batches go one sample at a time: the batch gradient of a mean loss is
    the mean of the per-sample gradients, each under that sample's slice of the decisions."""
    import torch
    B, h, w = x.shape[0], x.shape[2] // A, x.shape[3] // A
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
    lab = torch.as_tensor(label, dtype=torch.float64)
    flips = 0
    if B > 1 and B * A * A * h * w > LFT_PER_SAMPLE_NPIX:
        for i in range(B):
            y, _, f = lft_layers_fp64(x[i:i + 1], p, A, s, forced=lft_hip_masks(rt, xg, A, s, sample=i))
            (torch.nn.functional.l1_loss(y, lab[i:i + 1]) / B).backward()
            flips += f
            del y
    else:
        y, _, flips = lft_layers_fp64(x, p, A, s, forced=lft_hip_masks(rt, xg, A, s))
        torch.nn.functional.l1_loss(y, lab).backward()
    return {k: v.grad.numpy() for k, v in p.items()}, flips


# ---------------------------------------------------------------------------------------------------------------------
# DistgSSR: the geometry matrix, the parameter table at any angRes / scale, the reference graph with every tensor
# lfsr_distgssr_train_saved can return, and the maps between the graph's layouts and the HIP path's rows (_ref_to_hip / mask_perm above)
# ---------------------------------------------------------------------------------------------------------------------
# (A, s, B, h, w) and what each row reaches
DISTG_MATRIX = ((7, 2, 1, 5, 6),        # A != 5: gather EPI forward, three-kernel block tail, gather forms of every EPI gradient; npix 1470 < 2048: gather fuse.0 dgrad
                (9, 2, 1, 4, 4),        # 81 views, 9x9 AngConv.0
                (15, 2, 1, 3, 4),       # the largest angRes lfsr_distgssr_create accepts
                (1, 3, 2, 9, 7),        # one view, EPI lines of one pixel group, scale 3, odd ragged views
                (3, 3, 2, 13, 16),      # the fp32 fused-EPI kernels at A = 3, scale 3, odd h in the two-row Winograd weight-gradient tiles
                (5, 3, 2, 13, 16),      # the bench angRes: k_distg_tail, epi_b3, line-form gradients on ragged lines, k_head_bwd<3>
                (5, 2, 1, 40, 24),      # h > 32 >= w: line form for the horizontal pass, gather for the vertical, unmerged EPIConv.0 wgrad, two row tiles per view
                (5, 4, 1, 24, 40),      # the transpose of the row above
                (3, 2, 1, 33, 40),      # both view sides past 32 at A = 3; k_ang0_dgrad runs 6 chunks of 220 pixels
                (5, 4, 3, 32, 32),      # an odd batch at the bench geometry
                (5, 4, 8, 32, 32),      # the published training geometry: 204 800 pixels, past the block caps of k_add_inplace, k_head_bwd, k_init_gather9
                (4, 2, 1, 6, 5),        # even A: forward-only rows (the backward must refuse)
                (2, 3, 2, 9, 7))
DISTG_PER_SAMPLE_NPIX = 50000             # above this many LR pixels the fp64 work is done one sample at a time
# which of lfsr_distgssr_train_saved -> the kinds its rows hold side by side, and each kind's channels per row (all post-LeakyReLU values; "OUT" is
# the block output, the only one that is no decision)
DISTG_SAVED = {0: ("S1",), 1: ("S2", "A2", "EH2", "EV2"), 2: ("A1",), 3: ("EH1",), 4: ("EV1",), 5: ("FZ",), 6: ("OUT",)}
DISTG_CH = {"S1": 64, "S2": 64, "A2": 16, "EH2": 32, "EV2": 32, "A1": 16, "EH1": 32, "EV1": 32, "FZ": 64, "OUT": 64}
DISTG_BLOCKS = tuple(f"disentg.Group.{g}.Block.{b}." for g in range(4) for b in range(4))


def distg_spec(A, s):
    """(key, shape) list of DistgSSR at angRes A and scale s: lfsr_distgssr_create's table (model/SR/DistgSSR.py's state_dict), 137 entries"""
    AA = A * A
    spec = [("init_conv.weight", (64, 1, 3, 3))]
    for g in range(4):
        for b in range(4):
            p = f"disentg.Group.{g}.Block.{b}."
            spec += [(p + "SpaConv.0.weight", (64, 64, 3, 3)), (p + "SpaConv.2.weight", (64, 64, 3, 3)),
                     (p + "AngConv.0.weight", (16, 64, A, A)), (p + "AngConv.2.weight", (AA * 16, 16, 1, 1)),
                     (p + "EPIConv.0.weight", (32, 64, 1, AA)), (p + "EPIConv.2.weight", (A * 32, 32, 1, 1)),
                     (p + "fuse.0.weight", (64, 144, 1, 1)), (p + "fuse.2.weight", (64, 64, 3, 3))]
        spec.append((f"disentg.Group.{g}.conv.weight", (64, 64, 3, 3)))
    spec += [("disentg.conv.weight", (64, 64, 3, 3)), ("upsample.0.weight", (64 * s * s, 64, 1, 1)), ("upsample.0.bias", (64 * s * s,)),
             ("upsample.2.weight", (1, 64, 1, 1))]
    return spec


def distg_case(A, s, B, h, w):
    """-> (state_dict, input): synth_state_dict seed 0 / synth_input seed 1, as the golden cases"""
    return synth_state_dict(distg_spec(A, s), seed=0), synth_input((B, 1, A * h, A * w), seed=1)


def distg_keys():
    """every (which, index) of lfsr_distgssr_train_saved: 7 x 16"""
    return [(k, i) for k in DISTG_SAVED for i in range(16)]


def distg_samples(A, s, B, h, w):
    """the slices of the batch the fp64 graph takes at once: the whole batch, or one sample at a time at the published geometry"""
    return [slice(i, i + 1) for i in range(B)] if B > 1 and B * A * A * h * w > DISTG_PER_SAMPLE_NPIX else [slice(0, B)]


def distg_layers_fp64(x, params, A, s, forced=None, dtype=None):
    """DistgSSR's graph (model/SR/DistgSSR.py:29-36, 104-111, op for op as oracle/lfsr_torch_port.py::distgssr_forward_graph states it) on stock
    torch CPU ops -> (output, layers, flips).
    layers[(kind, index)]: the LeakyReLU outputs of MASK_KINDS and the block output "OUT" of block index = group * 4 + block, detached, in the
    reference's layouts (mask_ref_shape): every value lfsr_distgssr_train_saved can return (DISTG_SAVED; distg_ref_to_rows).
    params: {key: tensor} (fp64 unless `dtype` says otherwise; they may require grad).  forced: {(kind, index): bool mask in the reference
    layout} for MASK_KINDS -- the decisions are then the caller's (y = t where mask else 0.1 t, the port's `force=`), and flips counts those
    that differ from the graph's own."""
    import torch
    from oracle.lfsr_torch_port import macpi2sai, pixel_shuffle1d, sai2macpi
    F = torch.nn.functional
    dtype = dtype or torch.float64
    p = {k: torch.as_tensor(v).to(dtype) for k, v in params.items()}
    xd = torch.as_tensor(x).to(dtype)
    L, flips = {}, 0

    def block(z, pre, i):
        def lr(t, kind):
            nonlocal flips
            if forced is None:
                y = F.leaky_relu(t, 0.1)
            else:
                m = forced[kind, i]
                flips += int(((t > 0) != m).sum())
                y = torch.where(m, t, 0.1 * t)
            L[kind, i] = y.detach()
            return y
        spa = lr(F.conv2d(z, p[pre + "SpaConv.0.weight"], dilation=A, padding=A), "S1")
        spa = lr(F.conv2d(spa, p[pre + "SpaConv.2.weight"], dilation=A, padding=A), "S2")
        ang = lr(F.conv2d(z, p[pre + "AngConv.0.weight"], stride=A), "A1")
        ang = F.pixel_shuffle(lr(F.conv2d(ang, p[pre + "AngConv.2.weight"]), "A2"), A)

        def epi(t, tag):
            e = lr(F.conv2d(t, p[pre + "EPIConv.0.weight"], stride=(1, A), padding=(0, A * (A - 1) // 2)), tag + "1")
            return pixel_shuffle1d(lr(F.conv2d(e, p[pre + "EPIConv.2.weight"]), tag + "2"), A)
        epih = epi(z, "EH")
        epiv = epi(z.permute(0, 1, 3, 2).contiguous(), "EV").permute(0, 1, 3, 2)
        buf = torch.cat((spa, ang, epih, epiv), dim=1)
        buf = lr(F.conv2d(buf, p[pre + "fuse.0.weight"]), "FZ")
        out = F.conv2d(buf, p[pre + "fuse.2.weight"], dilation=A, padding=A) + z
        L["OUT", i] = out.detach()
        return out
    x_up = F.interpolate(xd, scale_factor=s, mode="bilinear", align_corners=False)
    buf0 = F.conv2d(sai2macpi(xd, A), p["init_conv.weight"], dilation=A, padding=A)
    buf = buf0
    for g in range(4):
        gin = buf
        for b in range(4):
            buf = block(buf, f"disentg.Group.{g}.Block.{b}.", g * 4 + b)
        buf = F.conv2d(buf, p[f"disentg.Group.{g}.conv.weight"], dilation=A, padding=A) + gin
    buf = F.conv2d(buf, p["disentg.conv.weight"], dilation=A, padding=A) + buf0
    up = F.conv2d(macpi2sai(buf, A), p["upsample.0.weight"], p["upsample.0.bias"])
    up = F.conv2d(F.pixel_shuffle(up, s), p["upsample.2.weight"])
    return up + x_up, L, flips


def distg_ref_to_rows(layers, which, index, B, A, h, w):
    """the reference's tensors of (which, index) as the HIP path stores them: rows in HIP order, the kinds of DISTG_SAVED[which] side by side
    (which 1: the 144-wide concat buffer)"""
    import torch
    return torch.cat([_ref_to_hip(k, layers[k, index], B, A, h, w).reshape(-1, DISTG_CH[k]) for k in DISTG_SAVED[which]], 1)


def distg_saved_rows(rt, xg, which, index=0):
    """what forward_train(xg) saved for (which, index), as rows in HIP order (a GPU view of the training workspace)"""
    return rt.train_saved(xg, which, index).reshape(-1, sum(DISTG_CH[k] for k in DISTG_SAVED[which]))


def distg_hip_masks_flat(rt, xg):
    """the LeakyReLU decisions (> 0) of forward_train(xg), flat in HIP order: {(kind, index): CPU bool tensor}"""
    return {(k, i): hip_saved_mask(rt, xg, k, i) for i in range(16) for k in MASK_KINDS}


def distg_masks_to_ref(flat, B, A, h, w, sample=None):
    """the same decisions in the reference layouts: what distg_layers_fp64's `forced` takes.  sample = i: the decisions of sample i alone, as a
    B = 1 graph takes them (every HIP layout is sample-major)"""
    out = {}
    for (k, i), m in flat.items():
        if sample is not None:
            n = m.numel() // B
            m = m[sample * n:(sample + 1) * n]
        out[k, i] = hip_mask_to_ref(m, k, B if sample is None else 1, A, h, w)
    return out


def distg_forced_fp64_grads(rt, xg, sd, x, label, A, s, masks=None):
    """fp64 autograd of distg_layers_fp64 under L1 `mean` loss with every LeakyReLU decision taken from what the HIP training forward saved
    (lfsr_distgssr_train_saved; `masks`: distg_hip_masks_flat read earlier), and the number of those decisions that differ from fp64's own.  A
    pre-activation within fp32 rounding of 0 is a legitimate tie whose two sides have different gradients downstream; this graph makes the same
    choices.  Large batches go one sample at a time: the batch gradient of a mean loss is the mean of the per-sample gradients, each under that
    sample's slice of the decisions."""
    import torch
    B, h, w = x.shape[0], x.shape[2] // A, x.shape[3] // A
    masks = distg_hip_masks_flat(rt, xg) if masks is None else masks
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
    lab = torch.as_tensor(label, dtype=torch.float64)
    flips = 0
    for sl in distg_samples(A, s, B, h, w):
        n = sl.stop - sl.start
        y, _, f = distg_layers_fp64(x[sl], p, A, s, forced=distg_masks_to_ref(masks, B, A, h, w, sample=None if n == B else sl.start))
        (torch.nn.functional.l1_loss(y, lab[sl]) * (n / B)).backward()
        flips += f
        del y
    return {k: v.grad.numpy() for k, v in p.items()}, flips


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def distg_cpu_fp32_rel(geom, sd, x, label):
    """e_ref of the cancellation allowance: fp32 CPU autograd of the same graph against fp64 autograd, each under its own decisions"""
    A, s, B, h, w = geom
    import torch
    out = []
    for dt in (torch.float32, torch.float64):
        p = {k: torch.tensor(v, dtype=dt, requires_grad=True) for k, v in sd.items()}
        for sl in distg_samples(*geom):
            y, _, _ = distg_layers_fp64(x[sl], p, A, s, dtype=dt)
            (torch.nn.functional.l1_loss(y, torch.as_tensor(label[sl]).to(dt)) * ((sl.stop - sl.start) / B)).backward()
            del y
        out.append({k: v.grad.numpy() for k, v in p.items()})
    return {k: _rel_l2(out[0][k], out[1][k]) for k in sd}


def distg_forced_gradient_gate(tag, net, xg, sd, x, label, A, s, masks, geom, host=None):
    """every parameter's gradient (137 state_dict entries) against fp64 autograd of the reference graph under the HIP forward's own LeakyReLU
    decisions: rel-L2 < 1e-4 per parameter, no parameter and no element left out.  A parameter that misses it gets the allowance of
    test_gpu_distgssr_train.py::test_grads_full_geometry_vs_torch_port_autograd, max(1e-4, 3 x e_ref), e_ref being the fp32 CPU autograd of the same
    graph against fp64 under its own decisions: what is cancellation there is cancellation here (upsample.0.bias, a sum of +-1/N).
    host: a {"s": seconds} counter of reference work on the host, added to.  -> {parameter: rel-L2}"""
    import time
    host = {"s": 0.0} if host is None else host
    t0 = time.time()
    forced, flips = distg_forced_fp64_grads(net._rt, xg, sd, x, label, A, s, masks=masks)
    host["s"] += time.time() - t0
    names = [k for k, _ in net.named_parameters()]
    assert names == [k for k, _ in distg_spec(A, s)] and len(names) == 137 and sum(p.numel() for p in net.parameters()) == net.grad_bucket.numel()
    errs = {k: _rel_l2(p.grad.detach().cpu().numpy(), forced[k]) for k, p in net.named_parameters()}
    v = np.array(list(errs.values()))
    print(f"{tag}: gradient rel-L2 vs fp64 median {np.median(v):.2e} max {v.max():.2e} ({max(errs, key=errs.get)}); "
          f"LeakyReLU decisions differing from fp64's own: {flips}; host {host['s']:.0f} s so far")
    bad = {k: e for k, e in errs.items() if not e < 1e-4}
    if bad:
        t0 = time.time()
        e_ref = distg_cpu_fp32_rel(geom, sd, x, label)
        host["s"] += time.time() - t0
        for k, e in bad.items():
            print(f"{tag}: {k} rel-L2 {e:.3e}, fp32 CPU autograd against fp64 {e_ref[k]:.3e}")
        bad = {k: (e, e_ref[k]) for k, e in bad.items() if not e < max(1e-4, 3 * e_ref[k])}
    assert not bad, bad
    return errs


# ---------------------------------------------------------------------------------------------------------------------
# EPIT: the geometry matrix, the reference graph with every tensor lfsr_epit_train_saved can return, and the maps between the graph's
# layouts and the HIP path's rows
# ---------------------------------------------------------------------------------------------------------------------
# (A, s, B, h, w) and what each row reaches.  The horizontal pass runs sequences of A h tokens, the vertical pass of A w; the matrix-pipe
# attention kernels (forward and backward) cover up to 160 tokens, k_epi_attn_mfma<10, 0> / k_epi_attn_bwd_mfma<10, 0> at every A != 5.
EPIT_MATRIX = ((1, 2, 2, 8, 8),       # n1 = 1; 8 tokens, less than one 16-token tile; npix 128, under the 2048-row switch between gather-GEMM and row-GEMM
               (2, 3, 2, 9, 7),       # even A; scale 3 (two-kernel tail, s^2 = 9 dgrad pack and store branch); 18 / 14 tokens; odd ragged view
               (4, 4, 1, 40, 6),      # exactly 160 tokens at run-time n1: all ten tiles full; views taller than 32; 24 tokens in the other pass
               (7, 2, 1, 5, 23),      # 35 tokens on MFMA and 161, one past the bound: the vertical pass on the VALU kernels at A != 5; h = 5 = the window's left half
               (8, 2, 1, 20, 4),      # 160 tokens with tiles aligned on two columns of 8; w = 4, narrower than the window, one Winograd tile
               (15, 2, 1, 10, 3),     # largest accepted angRes; 150 tokens, ragged last tile, every key tile in every query's band; 45 tokens
               (3, 2, 1, 40, 36),     # views wider than 32 in both directions; 120 / 108 tokens; several conv tiles per row, forward and backward
               (5, 3, 2, 13, 15),     # the benchmark's angRes at scale 3; 65 / 75 tokens on the N1 = 5 kernels, ragged; k_tail_bwd with s^2 = 9
               (5, 2, 1, 3, 32),      # h = 3, shorter than the window's halves (5, 6) and than a 4x4 conv tile; 15 / 160 tokens
               (5, 4, 8, 32, 32))     # the published training geometry: ragged weight-gradient splits, the loops of k_ew and k_tail_bwd, lfsr_add_inplace

# which of lfsr_epit_train_saved -> (layout, floats per row, number of indices); 0-3 are there after forward_train, 4-6 after backward.
# "tok": the feed-forward hidden rows, in the reference a token tensor of the pass (even index: horizontal, odd: vertical)
EPIT_SAVED = {0: ("vcl", 64, 6), 1: ("vcl", 64, 2), 2: ("vcl", 64, 10), 3: ("vcl", 64, 10), 4: ("tok", 256, 10), 5: ("vcl", 64, 1), 6: ("hr", 64, 1)}
EPIT_DECISION_KINDS = (1, 2, 3, 4, 5, 6)  # the tensors whose signs are ReLU / LeakyReLU decisions: 2 + 10 + 10 + 10 + 1 + 1 = 34
EPIT_PER_SAMPLE_NPIX = 50000              # above this many LR pixels the fp64 work is done one sample at a time


def epit_keys(kinds=tuple(EPIT_SAVED)):
    """every (which, index) of `kinds`: 28 after forward_train and 12 more after backward"""
    return [(k, i) for k in kinds for i in range(EPIT_SAVED[k][2])]


def epit_case(A, s, B, h, w):
    """-> (state_dict, input): synth_state_dict seed 0 / synth_input seed 1, as the golden cases.  EPIT's parameter shapes do not depend on
    angRes (tests/test_epit_reference.py asserts it), so the golden angRes-5 spec serves every A"""
    return synth_state_dict(model_spec("EPIT", 5, s), seed=0), synth_input((B, 1, A * h, A * w), seed=1)


def epit_samples(A, s, B, h, w):
    """the slices of the batch the fp64 graph takes at once: the whole batch, or one sample at a time at the published geometry"""
    return [slice(i, i + 1) for i in range(B)] if B > 1 and B * A * A * h * w > EPIT_PER_SAMPLE_NPIX else [slice(0, B)]


def epit_layout(which, index):
    """the layout of (which, index): "vcl", "hr", or the token layout of its pass, "tokh" (tokens (u y), sequences (b v x)) / "tokv" ((v x), (b u y))"""
    lay = EPIT_SAVED[which][0]
    return lay if lay != "tok" else ("tokv" if index % 2 else "tokh")


def epit_ref_to_rows(t, layout, B, A, h, w):
    """reference layout -> the HIP path's rows [b][u][v][y][x][c] (VCL).  vcl: (B, c, A^2, h, w); tokh: (A h, B A w, c); tokv: (A w, B A h, c);
    hr: (B, 64, A h s, A w s) -> the channel-last mosaic's rows"""
    if layout == "vcl":
        return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])
    if layout == "tokh":
        return t.reshape(A, h, B, A, w, -1).permute(2, 0, 3, 1, 4, 5).reshape(-1, t.shape[-1])
    if layout == "tokv":
        return t.reshape(A, w, B, A, h, -1).permute(2, 3, 0, 4, 1, 5).reshape(-1, t.shape[-1])
    if layout == "hr":
        return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])
    raise KeyError(layout)


def epit_rows_to_ref(v, layout, B, A, h, w, s=1):
    """the inverse: flat values in HIP order -> the reference layout"""
    if layout == "vcl":
        return v.reshape(B, A * A, h, w, -1).permute(0, 4, 1, 2, 3)
    if layout == "tokh":
        return v.reshape(B, A, A, h, w, -1).permute(1, 3, 0, 2, 4, 5).reshape(A * h, B * A * w, -1)
    if layout == "tokv":
        return v.reshape(B, A, A, h, w, -1).permute(2, 4, 0, 1, 3, 5).reshape(A * w, B * A * h, -1)
    if layout == "hr":
        return v.reshape(B, A * h * s, A * w * s, 64).permute(0, 3, 1, 2)
    raise KeyError(layout)


def epit_saved_rows(rt, xg, which, index=0):
    """what forward_train(xg) (which 0-3) or the backward after it (4-6) left for (which, index), as rows in HIP order (a GPU tensor)"""
    return rt.train_saved(xg, which, index).reshape(-1, EPIT_SAVED[which][1])


def epit_hip_masks(rt, xg, A, s, sample=None):
    """the 34 ReLU / LeakyReLU decisions (> 0) the HIP path took, read after its backward, in the reference layouts: what epit_layers_fp64's
    `forced` takes.  sample = i: the decisions of sample i alone, as a B = 1 graph takes them (rows are sample-major)"""
    B, h, w = xg.shape[0], xg.shape[2] // A, xg.shape[3] // A
    out = {}
    for k, i in epit_keys(EPIT_DECISION_KINDS):
        m = (epit_saved_rows(rt, xg, k, i) > 0).cpu()
        if sample is not None:
            n = m.shape[0] // B
            m = m[sample * n:(sample + 1) * n]
        out[k, i] = epit_rows_to_ref(m, epit_layout(k, i), B if sample is None else 1, A, h, w, s)
    return out


def epit_layers_fp64(x, params, A, s, forced=None, dtype=None):
    """EPIT's graph (model/SR/EPIT.py:51-71, op for op as oracle/lfsr_torch_port.py::epit_forward states it) on stock torch CPU ops
    -> (output, layers, flips).
    layers[(which, index)]: every tensor lfsr_epit_train_saved can return, detached, in the reference's layout (EPIT_SAVED; epit_ref_to_rows).
    params: {key: tensor} (fp64 unless `dtype` says otherwise; they may require grad).  forced: {(which, index): bool mask in the reference
    layout} for EPIT_DECISION_KINDS -- the decisions are then the caller's, and flips counts those that differ from the graph's own."""
    import torch
    from oracle.lfsr_torch_port import _bicubic_views, _conv133, _mha, _window_mask
    F = torch.nn.functional
    dtype = dtype or torch.float64
    p = {k: torch.as_tensor(v).to(dtype) for k, v in params.items()}
    xd = torch.as_tensor(x).to(dtype)
    B, _, Hh, Ww = xd.shape
    h, w = Hh // A, Ww // A
    L, flips = {}, 0

    def act(z, key, slope, keep_pre=False):
        nonlocal flips
        if forced is None:
            y = F.leaky_relu(z, slope) if slope else F.relu(z)
        else:
            m = forced[key]
            assert m.shape == z.shape, (key, tuple(m.shape), tuple(z.shape))
            flips += int(((z > 0) != m).sum())
            y = torch.where(m, z, z * slope)
        L[key] = (z if keep_pre else y).detach()
        return y

    def trans(buf, pre, key):      # BasicTrans.forward EPIT.py:110-128; buf (b, c, sequences, tokens of one angular row, tokens of one line)
        b, c, n, v, l = buf.shape
        mask = _window_mask(v, l, A, A, 5, 6, l)         # mask_field [2 A, 11]
        tok = F.linear(buf.permute(3, 4, 0, 2, 1).reshape(v * l, b * n, c), p[pre + "linear_in.weight"])
        tn = F.layer_norm(tok, tok.shape[-1:], p[pre + "norm.weight"], p[pre + "norm.bias"])
        tok = _mha(tn, tn, tok, p[pre + "attention.in_proj_weight"], p[pre + "attention.out_proj.weight"], 8, mask) + tok
        ff = F.layer_norm(tok, tok.shape[-1:], p[pre + "feed_forward.0.weight"], p[pre + "feed_forward.0.bias"])
        tok = F.linear(act(F.linear(ff, p[pre + "feed_forward.1.weight"]), key, 0.0), p[pre + "feed_forward.4.weight"]) + tok
        return F.linear(tok, p[pre + "linear_out.weight"]).reshape(v, l, b, n, -1).permute(2, 4, 3, 0, 1)
    views, skip = _bicubic_views(xd, A, h, w, s)
    buf = _conv133(views, p["conv_init0.0.weight"])
    t = act(_conv133(buf, p["conv_init.0.weight"]), (1, 0), 0.2)
    t = act(_conv133(t, p["conv_init.2.weight"]), (1, 1), 0.2)
    buf = act(_conv133(t, p["conv_init.4.weight"]), (5, 0), 0.2) + buf
    t = buf
    c = buf.shape[1]
    nblk = 1 + max(int(k.split(".")[1]) for k in p if k.startswith("altblock."))
    for i in range(nblk):
        pre = f"altblock.{i}."
        L[0, i] = t.detach()
        shortcut = t

        def conv(z, j):
            z = act(_conv133(z, p[pre + "conv.0.weight"]), (2, j), 0.2)
            z = act(_conv133(z, p[pre + "conv.2.weight"]), (3, j), 0.2)
            return _conv133(z, p[pre + "conv.4.weight"])
        z = t.reshape(B, c, A, A, h, w).permute(0, 1, 3, 5, 2, 4).reshape(B, c, A * w, A, h)        # horizontal: tokens (u y)
        z = trans(z, pre + "epi_trans.", (4, 2 * i))
        z = z.reshape(B, c, A, w, A, h).permute(0, 1, 4, 2, 5, 3).reshape(B, c, A * A, h, w)
        t = conv(z, 2 * i) + shortcut
        z = t.reshape(B, c, A, A, h, w).permute(0, 1, 2, 4, 3, 5).reshape(B, c, A * h, A, w)        # vertical: tokens (v x)
        z = trans(z, pre + "epi_trans.", (4, 2 * i + 1))
        z = z.reshape(B, c, A, h, A, w).permute(0, 1, 2, 4, 3, 5).reshape(B, c, A * A, h, w)
        t = conv(z, 2 * i + 1) + shortcut
    t = t + buf
    L[0, nblk] = t.detach()
    mosaic = t.reshape(B, c, A, A, h, w).permute(0, 1, 2, 4, 3, 5).reshape(B, c, A * h, A * w)
    up = F.pixel_shuffle(F.conv2d(mosaic, p["upsampling.0.weight"]), s)
    y = F.conv2d(act(up, (6, 0), 0.2, keep_pre=True), p["upsampling.3.weight"], padding=1) + skip
    return y, L, flips


def epit_forced_fp64_grads(rt, xg, sd, x, label, A, s, dtype=None):
    """-> ({name: fp64 gradient}, number of the HIP path's decisions that differ from fp64's own).  Call after the HIP backward of xg.
    fp64 autograd of epit_layers_fp64 under L1 `mean` loss with every one of its 34 activation decisions taken from what the HIP path computed
    (lfsr_epit_train_saved): 3 in conv_init; per block and pass the feed-forward ReLU, conv.0 and conv.2; the tail's HR LeakyReLU.  A
    pre-activation within fp32 rounding of 0 is a legitimate tie whose two sides have different gradients downstream (one flipped pixel moves
    the gradient of a small case by ~1e-3); this graph makes the same choices.  The sign of the L1 loss's gradient is taken from the HIP
    output as well.  Large batches go one sample at a time: the batch gradient of a mean loss is the mean of the per-sample gradients, each
    under that sample's slice of the decisions.  dtype: the same autograd in another precision (torch.float32: the e_ref of the cancellation
    allowance, fp32 CPU autograd under the same decisions)."""
    import torch
    dtype = dtype or torch.float64
    B, h, w = x.shape[0], x.shape[2] // A, x.shape[3] // A
    out_hip = rt.forward(xg).cpu().double()                  # bit-equal to the training forward's output; runs in the inference workspace
    lab = torch.as_tensor(label, dtype=torch.float64)
    sign = torch.sign(out_hip - lab).to(dtype)
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in sd.items()}
    flips = 0
    for sl in epit_samples(A, s, B, h, w):
        n = sl.stop - sl.start
        forced = epit_hip_masks(rt, xg, A, s, sample=None if n == B else sl.start)
        assert len(forced) == 34
        y, _, f = epit_layers_fp64(x[sl], p, A, s, forced=forced, dtype=dtype)
        ((y * sign[sl]).sum() / sign.numel()).backward()
        flips += f
        del y
    return {k: v.grad.numpy() for k, v in p.items()}, flips


# ---------------------------------------------------------------------------------------------------------------------
# operator-level forward tests (tests/test_gpu_distg_fwd_ops.py): operands inside wider, guarded allocations; the two value gates
# ---------------------------------------------------------------------------------------------------------------------
OP_SENTINEL = -2.0 ** 100
OP_GUARD_ROWS = 320          # NaN rows in front of and behind an input's [0, M) rows (the row-streaming kernels walk 256-row tiles past M behind a bounds check)
OP_TAIL_ROWS = 8             # sentinel rows behind an output's last pixel
YARDSTICK = 8.0              # HIP mean error <= 8 x the fp32 CPU mean error (tests/test_gpu_distgssr_geometries.py asserts the same ratio)
# (operator, form, row) -> why the yardstick is not asserted there (the hard gate still is); profiles/distgssr_forward_op_tests.md has the measured ratios
YARDSTICK_EXEMPT = {}


def set_selectors(monkeypatch, names, **env):
    """exactly the given kernel selectors of `names` (None / "" = unset)"""
    for k in names:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in names, k
        if v:
            monkeypatch.setenv(k, v)


def macpi_to_rows(t, A):
    """NCHW MacPI (B, C, h A, w A), element [b, c, y A + u, x A + v] -> VCL rows (B A^2 h w, C), view u A + v (torch, any dtype, on the CPU)"""
    B, C, Hh, Ww = t.shape
    h, w = Hh // A, Ww // A
    return t.reshape(B, C, h, A, w, A).permute(0, 3, 5, 2, 4, 1).reshape(-1, C).contiguous()


class OpBuffer:
    """a device allocation with an operand inside: ptr = the address of row 0 of the operand (a ctypes void pointer)"""

    def __init__(self, t, first_row, rows, stride, pristine=None):
        import ctypes
        self.t, self.rows, self.stride, self.pristine = t, rows, stride, pristine
        self.ptr = ctypes.c_void_p(t.data_ptr() + first_row * stride * 4)

    def reset(self):
        self.t.copy_(self.pristine)


def op_input(rows, stride, choff, seed):
    """fp32 rows (M, c) at channel offset choff of `stride`-float rows whose foreign columns hold +-1e3 (finite: the K = 144 row-GEMM multiplies masked columns by
    zero weights), with OP_GUARD_ROWS rows of NaN in front and behind inside the same allocation: a kernel that folds a row outside [0, M) in shows it"""
    import torch
    M, c = rows.shape
    assert stride >= choff + c
    body = (torch.randint(0, 2, (M, stride), generator=torch.Generator().manual_seed(seed)).float() * 2 - 1) * 1e3
    body[:, choff:choff + c] = rows.float()
    buf = torch.full((M + 2 * OP_GUARD_ROWS, stride), float("nan"))
    buf[OP_GUARD_ROWS:OP_GUARD_ROWS + M] = body
    return OpBuffer(buf.cuda(), OP_GUARD_ROWS, M, stride)


def op_output(M, stride, seed):
    """an output of M rows inside `stride`-float rows of random finite values, OP_TAIL_ROWS sentinel rows behind the last one"""
    import torch
    t = torch.randn(M + OP_TAIL_ROWS, stride, generator=torch.Generator().manual_seed(seed)) * 3.0
    t[M:] = OP_SENTINEL
    d = t.cuda()
    return OpBuffer(d, 0, M, stride, pristine=d.clone())


def op_output_read(buf, choff, c, holes=()):
    """waits for the device, asserts that every float outside channels [choff, choff + c) of rows [0, M) -- and inside the column ranges `holes` -- kept its bits
    (c = 0: the whole allocation), and returns the written channels on the CPU"""
    import torch
    torch.cuda.synchronize()
    keep = torch.ones(buf.t.shape, dtype=torch.bool, device=buf.t.device)
    keep[:buf.rows, choff:choff + c] = False
    for lo, hi in holes:
        keep[:buf.rows, lo:hi] = True
    same = buf.t.view(torch.int32) == buf.pristine.view(torch.int32)
    assert bool((same | ~keep).all()), "an output float outside the operand's channel range changed"
    return buf.t[:buf.rows, choff:choff + c].cpu().contiguous()


def op_gate(got, ref, cpu, op, form, row, tol=1e-4, relative=True, tag="FWDOP"):
    """the two gates of an operator output against its fp64 reference: max|err| <= tol * max(1, max|ref|) (relative=False: tol itself), and mean|err| <= YARDSTICK x
    the mean error of `cpu`, the same operator in fp32 on the CPU with stock torch ops.  Prints the figures first (`tag`: the first column of that line)
    -> (max error / gate, yardstick ratio)"""
    import torch
    got, ref, cpu = got.detach().double().cpu(), ref.detach().double().cpu(), cpu.detach().double().cpu()
    assert got.shape == ref.shape == cpu.shape, (op, form, row, got.shape, ref.shape, cpu.shape)
    assert bool(torch.isfinite(got).all()), (op, form, row)
    err = (got - ref).abs()
    e_max, e_mean, e_cpu = float(err.max()), float(err.mean()), float((cpu - ref).abs().mean())
    gate = tol * max(1.0, float(ref.abs().max())) if relative else tol
    ratio = e_mean / e_cpu if e_cpu > 0 else (0.0 if e_mean == 0 else float("inf"))
    print(f"{tag} | {op} | {form} | {row} | max {e_max:.3e} | mean {e_mean:.3e} | e_cpu {e_cpu:.3e} | ratio {ratio:.2f} | gate {gate:.3e}")
    assert e_max <= gate, (op, form, row, e_max, gate)
    if (op, form, row) not in YARDSTICK_EXEMPT:
        assert e_mean <= YARDSTICK * e_cpu, (op, form, row, e_mean, e_cpu, ratio)
    return e_max / gate, ratio


fwd_op_gate = op_gate        # the name the forward operator tests call it by


# ---------------------------------------------------------------------------------------------------------------------
# operator-level tests of lfsr_window_attn_bwd (tests/test_gpu_epit_attn_bwd.py, tests/test_gpu_trans_bwd_ops.py): q | k, v, o / dO in wider rows at
# non-zero channel offsets, dQ | dK and dV into sentinel-filled buffers with two rows behind the last pixel
# ---------------------------------------------------------------------------------------------------------------------
ATTN_SENTINEL = -777.25


def rel_l2(a, b):
    """rel-L2 of a against the fp64 reference b.  A reference that is exactly zero (the softmax over a single key is constant: dQ = dK = 0) asks for exact zeros"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    num, den = float(np.linalg.norm(a - b)), float(np.linalg.norm(b))
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def attn_bwd_layout(E):
    """(qk_stride, q_choff, k_choff, v_stride, v_choff, o_stride, o_choff) of these tests for heads that fill E columns"""
    return (2 * E + 32, 16, E + 20, E + 16, 8, E + 8, 4)


def attn_bwd_run(lib, q, k, v, o, d_o, nheads, geometry):
    """lfsr_window_attn_bwd on (npix, E) numpy operands laid out by attn_bwd_layout; geometry: its arguments from ns0 to clip2 -> (dqk, dv), device buffers"""
    import torch
    from lfsr_amd import capi
    npix, E = q.shape
    qs, qo, ko, vs, vo, os_, oo = attn_bwd_layout(E)

    def wide(a, stride, off):
        return torch.from_numpy(np.pad(a, ((0, 0), (off, stride - off - a.shape[1])))).cuda()
    qk = wide(np.concatenate([q, np.zeros((npix, ko - qo - E), np.float32), k], 1), qs, qo)
    vd, od, dod = wide(v, vs, vo), wide(o, os_, oo), wide(d_o, os_, oo)
    dqk = torch.full((npix + 2, qs), ATTN_SENTINEL, device="cuda")
    dv = torch.full((npix + 2, vs), ATTN_SENTINEL, device="cuda")
    stats = torch.empty(npix * nheads * 4, device="cuda")
    capi.check(lib.lfsr_window_attn_bwd(capi.dev_ptr(qk), qs, qo, ko, capi.dev_ptr(vd), vs, vo, capi.dev_ptr(od), capi.dev_ptr(dod), os_, oo, capi.dev_ptr(dqk),
                                        capi.dev_ptr(dv), capi.dev_ptr(stats), nheads, E // nheads, *geometry, capi.stream_ptr()), "attn_bwd")
    torch.cuda.synchronize()
    return dqk, dv


def attn_bwd_untouched(dqk, dv, npix, E):
    """every float outside the dQ | dK and dV column ranges of rows [0, npix) still holds the sentinel"""
    import torch
    qs, qo, ko, vs, vo, _, _ = attn_bwd_layout(E)
    keep = torch.ones(qs, dtype=torch.bool)
    keep[qo:qo + E] = False
    keep[ko:ko + E] = False
    keepv = torch.ones(vs, dtype=torch.bool)
    keepv[vo:vo + E] = False
    return (bool((dqk[:, keep.cuda()] == ATTN_SENTINEL).all()) and bool((dqk[npix:] == ATTN_SENTINEL).all()) and bool((dv[npix:] == ATTN_SENTINEL).all())
            and bool((dv[:, keepv.cuda()] == ATTN_SENTINEL).all()))


# ---------------------------------------------------------------------------------------------------------------------
# fp64 references of the backward operators the LFT and EPIT training drivers share (tests/test_gpu_trans_bwd_ops.py; checked on their own, without
# a GPU, by tests/test_trans_bwd_refs_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------
LFT_NH = 8
# (n, h, w) of the spatial attention cases: every query sees at least one key (w <= h + 2), tests/test_trans_bwd_refs_cpu.py asserts it on the mask
LFT_SPA_GEOMS = ((3, 6, 8), (2, 13, 7), (2, 7, 9), (1, 1, 1), (4, 3, 5))


def ln_bwd_ref(x, pe_rows_of_x, gamma, dy, dtype):
    """autograd of torch.nn.functional.layer_norm(x + pe rows) * gamma (+ beta) in `dtype` -> (dx, dgamma, dbeta); pe_rows_of_x: (M, C) or None"""
    import torch
    xt = torch.as_tensor(x).detach().to(dtype).clone().requires_grad_(True)
    g = torch.as_tensor(gamma).detach().to(dtype).clone().requires_grad_(True)
    b = torch.zeros_like(g).requires_grad_(True)
    xin = xt if pe_rows_of_x is None else xt + torch.as_tensor(pe_rows_of_x).to(dtype)
    torch.nn.functional.layer_norm(xin, xin.shape[-1:], g, b, 1e-5).backward(torch.as_tensor(dy).to(dtype))
    return xt.grad, g.grad, b.grad


def ln_bwd_closed_form(x, gamma, dy, eps=1e-5):
    """the closed form trans_bwd.hip quotes: dx = rstd (dy g - mean(dy g) - xhat mean(dy g xhat)), dgamma = sum dy xhat, dbeta = sum dy (torch, the dtype of x)"""
    mu = x.mean(-1, keepdim=True)
    rstd = 1.0 / ((x - mu).pow(2).mean(-1, keepdim=True) + eps).sqrt()
    xh = (x - mu) * rstd
    gy = dy * gamma
    dx = rstd * (gy - gy.mean(-1, keepdim=True) - xh * (gy * xh).mean(-1, keepdim=True))
    return dx, (dy * xh).sum(0), dy.sum(0)


def tail_du_rows(d_hr, B, A, h, w, s):
    """dHR (B, 64, A h s, A w s) -> the rows lfsr_up_tail_bwd writes: p = (b, u, v, y, x), column c s^2 + i s + j = dHR[b][c][(u h + y) s + i][(v w + x) s + j]"""
    return d_hr.reshape(B, 64, A, h, s, A, w, s).permute(0, 2, 5, 3, 6, 1, 4, 7).reshape(B * A * A * h * w, 64 * s * s)


def tail_bwd_ref(hr_rows, w3, dout, B, A, h, w, s, slope, dtype):
    """autograd of conv2d(leaky_relu(HR, slope), w3, padding=1) on the (B, A h s, A w s) mosaic in `dtype`; hr_rows: the channel-last HR map (pixels, 64)
    -> (du rows, dw3 (576,)).  At HR == 0 (and -0) torch's leaky_relu backward takes the slope (`x > 0 ? g : g * slope`): the project's convention"""
    import torch
    Hs, Ws = A * h * s, A * w * s
    hr = torch.as_tensor(hr_rows).detach().to(dtype).reshape(B, Hs, Ws, 64).permute(0, 3, 1, 2).clone(memory_format=torch.contiguous_format).requires_grad_(True)
    wt = torch.as_tensor(w3).detach().to(dtype).reshape(1, 64, 3, 3).clone().requires_grad_(True)
    out = torch.nn.functional.conv2d(torch.nn.functional.leaky_relu(hr, slope), wt, padding=1)
    out.backward(torch.as_tensor(dout).to(dtype).reshape(B, 1, Hs, Ws))
    return tail_du_rows(hr.grad, B, A, h, w, s), wt.grad.reshape(-1)


def _attn_autograd(q, k, v, d_o, to_heads, mask):
    """fp64 autograd of softmax(q k^T / sqrt(hd) + mask) v; to_heads: pixel rows (npix, E) -> (..., tokens, hd), a permutation -> (o, dq, dk, dv) in pixel rows"""
    import torch
    qt, kt, vt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, k, v))
    hd = to_heads(qt).shape[-1]
    S = to_heads(qt) @ to_heads(kt).transpose(-1, -2) / np.sqrt(hd)
    out = torch.softmax(S if mask is None else S + mask, -1) @ to_heads(vt)
    dq, dk, dv = torch.autograd.grad((out * to_heads(torch.tensor(d_o, dtype=torch.float64))).sum(), (qt, kt, vt))
    ot = torch.zeros(q.shape, dtype=torch.float64, requires_grad=True)       # the output back in pixel rows: through the same (linear) rearrangement
    o_rows, = torch.autograd.grad((to_heads(ot) * out.detach()).sum(), ot)
    return o_rows.numpy(), dq.numpy(), dk.numpy(), dv.numpy()


def lft_ang_attn_ref(q, k, v, d_o, B, A, h, w):
    """LFT's angular attention (LFT.py:233-246): dense over the A^2 views of each pixel, 8 heads of 8; rows (b, u, v, y, x) x 64"""
    E = q.shape[1]
    return _attn_autograd(q, k, v, d_o, lambda t: t.reshape(B, A * A, h * w, LFT_NH, E // LFT_NH).permute(0, 2, 3, 1, 4), None)


def lft_spa_attn_ref(q, k, v, d_o, n, h, w):
    """LFT's spatial attention (LFT.py:161-199) in the reference's own dense form: O.lft_gen_mask(h, w, 5) added to the (h w, h w) scores; 8 heads of 16"""
    import torch
    from oracle import lfsr_oracle as O
    E = q.shape[1]
    mask = torch.from_numpy(O.lft_gen_mask(h, w, 5, np.float64))
    return _attn_autograd(q, k, v, d_o, lambda t: t.reshape(n, h * w, LFT_NH, E // LFT_NH).permute(0, 2, 1, 3), mask)
