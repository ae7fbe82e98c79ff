#!/usr/bin/env python3
"""Bit comparison of two builds of DistgSSR's branch operators (lfsr_angconv_fwd, lfsr_epiconv_fwd, lfsr_epiconv_hv_fwd, lfsr_distg_branch_tail_fwd) inside ONE
process: outputs, stage-1 buffers and return codes under every lab selection, every buffer pre-filled with 7.0, torch.equal on the int32 view.
usage: LFSR_LAB=1 python tools/branch_ab.py ref=lib.so new=lib.so      (the selectors are parsed per call, so one process switches them; they need LFSR_LAB)"""
import ctypes as C, os, sys
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lfsr_amd import capi

c_p, c_i, c_f = C.c_void_p, C.c_int, C.c_float
GEOMS = [(1, 5, 8, 8), (2, 5, 6, 7), (1, 5, 8, 16), (1, 3, 8, 8), (2, 1, 9, 7), (1, 7, 5, 6), (1, 5, 33, 8)]       # the last two: gather-GEMM only
SELECTORS = ("LFSR_EPI", "LFSR_EPI_ORDER", "LFSR_ANG")
SELECTIONS = [("none", {}, 0, 0), ("LFSR_EPI=wino", {"LFSR_EPI": "wino"}, 0, 0), ("LFSR_EPI=direct", {"LFSR_EPI": "direct"}, 0, 0),
              ("LFSR_EPI=gather", {"LFSR_EPI": "gather"}, 0, 0), ("LFSR_EPI_ORDER=pass", {"LFSR_EPI_ORDER": "pass"}, 0, 0),
              ("LFSR_EPI_ORDER=item", {"LFSR_EPI_ORDER": "item"}, 0, 0), ("LFSR_EPI=wino LFSR_EPI_ORDER=pass", {"LFSR_EPI": "wino", "LFSR_EPI_ORDER": "pass"}, 0, 0),
              ("LFSR_EPI=wino LFSR_EPI_ORDER=item", {"LFSR_EPI": "wino", "LFSR_EPI_ORDER": "item"}, 0, 0), ("LFSR_ANG=gather", {"LFSR_ANG": "gather"}, 0, 0),
              ("lfsr_set_arithmetic(F32)", {}, 1, 0), ("lfsr_set_branch_arithmetic(BF16)", {}, 0, 1)]


def bind(path):
    lib = C.CDLL(os.path.abspath(path))
    lib.lfsr_angconv_fwd.argtypes = [c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p]
    lib.lfsr_epiconv_fwd.argtypes = [c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p]
    lib.lfsr_epiconv_hv_fwd.argtypes = [c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p]
    lib.lfsr_distg_branch_tail_fwd.argtypes = [c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p]
    lib.lfsr_set_arithmetic.argtypes = lib.lfsr_set_branch_arithmetic.argtypes = [c_i]
    return lib


def calls(lib, geom, st):
    """every call of the comparison on one geometry: name -> (rc, the buffers it may have written)"""
    B, A, h, w = geom
    npix, nlr, nepi = B * A * A * h * w, B * h * w, B * A * h * w
    g = torch.Generator(device="cuda").manual_seed(17)
    x = torch.randn(npix, 64, device="cuda", generator=g)
    spa = torch.randn(npix, 64, device="cuda", generator=g)
    wa0 = capi.pack_conv_weight(torch.randn(16, 64, A, A, device="cuda", generator=g) * 0.03)
    wa2 = capi.pack_conv_weight(torch.randn(16 * A * A, 16, 1, 1, device="cuda", generator=g) * 0.2, perm=1, ch=16)
    we0 = capi.pack_conv_weight(torch.randn(32, 64, 1, A * A, device="cuda", generator=g) * 0.03)
    we2 = capi.pack_conv_weight(torch.randn(32 * A, 32, 1, 1, device="cuda", generator=g) * 0.15)
    wf = capi.pack_conv_weight(torch.randn(64, 144, 1, 1, device="cuda", generator=g) * 0.08)
    L, P = 0.1, (lambda t: t.data_ptr() if t is not None else None)
    new = lambda rows, cols: torch.full((rows, cols), 7.0, device="cuda")
    out = {}
    y, t = new(npix, 144), new(nlr, 16)
    out["angconv"] = (lib.lfsr_angconv_fwd(P(x), 64, 0, P(wa0), P(wa2), P(t), P(y), 144, 64, B, A, h, w, L, st), y, t)
    for v in (0, 1):
        for tag, choff, tmp in (("", 80 + 32 * v, True), (" choff 82", 82, True), (" tmp=NULL", 80 + 32 * v, False)):
            y, t = new(npix, 144), new(nepi, 32)
            out[f"epiconv v={v}{tag}"] = (lib.lfsr_epiconv_fwd(P(x), 64, 0, P(we0), P(we2), P(t) if tmp else None, P(y), 144, choff, B, A, h, w, v, L, st), y, t)
    for tag, ch, cv, tmp in (("", 80, 112, True), (" choff 46 / 82", 46, 82, True), (" tmp=NULL", 80, 112, False)):
        y, t = new(npix, 144), new(nepi, 32)
        out[f"epiconv_hv{tag}"] = (lib.lfsr_epiconv_hv_fwd(P(x), 64, 0, P(we0), P(we2), P(t) if tmp else None, P(y), 144, ch, cv, B, A, h, w, L, st), y, t)
    if A == 5 and h <= 32 and w <= 32:
        y, ta, th, tv = new(npix, 64), new(nlr, 16), new(nepi, 32), new(nepi, 32)
        out["distg_branch_tail"] = (lib.lfsr_distg_branch_tail_fwd(P(x), 64, 0, P(spa), 64, 0, P(wa0), P(wa2), P(we0), P(we2), P(wf), P(ta), P(th), P(tv), P(y), 64, 0,
                                                                   B, A, h, w, L, st), y, ta, th, tv)
    torch.cuda.synchronize()
    return out


def main():
    assert os.environ.get("LFSR_LAB"), "the selectors are read only under LFSR_LAB"
    (rt, ref), (nt, new) = [(t, bind(p)) for t, p in (a.split("=", 1) for a in sys.argv[1:3])]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = 0
    print(f"| selection | calls compared ({rt} vs {nt}) | return codes | buffers |\n|---|---|---|---|")
    for name, env, arith, branch in SELECTIONS:
        for k in SELECTORS:
            os.environ.pop(k, None)
        os.environ.update(env)
        n = nrc = nbuf = 0
        codes = set()
        for geom in GEOMS:
            res = []
            for lib in (ref, new):
                assert lib.lfsr_set_arithmetic(arith) == 0 and lib.lfsr_set_branch_arithmetic(branch) == 0
                res.append(calls(lib, geom, st))
                assert lib.lfsr_set_arithmetic(0) == 0 and lib.lfsr_set_branch_arithmetic(0) == 0
            for key, (rc, *bufs) in res[0].items():
                rc2, *bufs2 = res[1][key]
                same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(bufs, bufs2))
                n += 1; nrc += rc == rc2; nbuf += same; codes.add(rc)
                if rc != rc2 or not same:
                    bad += 1
                    print(f"DIFFERS: {name} {geom} {key}: rc {rc} vs {rc2}, buffers {'equal' if same else 'differ'}", flush=True)
        print(f"| {name} | {n} over {len(GEOMS)} geometries | equal, {nrc} of {n} (values seen: {sorted(codes)}) | equal, {nbuf} of {n} |", flush=True)
    print("ALL EQUAL" if not bad else f"{bad} DIFFERENCES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
