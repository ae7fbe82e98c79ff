#!/usr/bin/env python3
"""Bit comparison of two builds of the weight-gradient operators (lfsr_conv3x3_wgrad, lfsr_pointwise_wgrad, lfsr_linear_wgrad, lfsr_conv3x3_wide_wgrad, lfsr_angconv_bwd,
lfsr_epiconv_hv_bwd) inside ONE process: return codes, every buffer a call may write (pre-filled with 7.0, torch.equal on the int32 view) and every value of the six
*_workspace_floats functions, under every lab selection of the family and each of the four gradient arithmetics.
usage: LFSR_LAB=1 python tools/wgrad_ab.py ref=lib.so new=lib.so [--sizes-only]     (--sizes-only: the workspace functions alone, host code, no GPU needed)"""
import ctypes as C, itertools, os, sys
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lfsr_amd import capi

c_p, c_i, c_f, c_sz, c_ll = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_longlong
GEOMS = [(1, 5, 8, 8), (2, 5, 6, 7), (1, 5, 33, 8), (1, 3, 8, 8), (1, 7, 5, 6)]       # (1, 5, 33, 8): lines above 32 pixels, the merged EPI form declines
CONV3 = [(25, 8, 8), (50, 6, 7), (300, 6, 6), (3, 33, 8), (2, 5, 33)]                 # (300, 6, 6): more tiles than the 256 persistent blocks
LINEAR = [(300, 64, 64), (300, 256, 128), (70001, 64, 64), (4097, 576, 64), (1000, 1024, 256), (2500, 128, 256)]
POINTWISE = [(1600, 64, 144), (5000, 64, 144), (1600, 16, 64), (777, 64, 16), (3000, 32, 32)]
WIDE = [(128, 2, 5, 33), (320, 3, 4, 32), (128, 300, 6, 6), (320, 25, 8, 8)]
SELECTORS = ("LFSR_WGRAD3", "LFSR_WGRAD_EPI", "LFSR_WGRAD_PW")
MODES = ("lfsr_set_grad_arithmetic", "lfsr_set_lin_grad_arithmetic", "lfsr_set_wide_train_arithmetic", "lfsr_set_branch_grad_arithmetic")
SELECTIONS = [("none", {}, {}), ("LFSR_WGRAD3=direct", {"LFSR_WGRAD3": "direct"}, {}), ("LFSR_WGRAD_EPI=gather", {"LFSR_WGRAD_EPI": "gather"}, {}),
              ("LFSR_WGRAD_PW=gather", {"LFSR_WGRAD_PW": "gather"}, {})] + [(f"{m}(1)", {}, {m: 1}) for m in MODES] + \
             [("lfsr_set_wide_train_arithmetic(2)", {}, {"lfsr_set_wide_train_arithmetic": 2}),
              ("lfsr_set_grad_arithmetic(1) LFSR_WGRAD3=direct", {"LFSR_WGRAD3": "direct"}, {"lfsr_set_grad_arithmetic": 1})]
SIZES = {"lfsr_conv3x3_wgrad_workspace_floats": ([c_i] * 3, itertools.product((0, 1, 2, 25, 50, 300, 1000, 1 << 20), (1, 2, 5, 6, 32, 33, 64), (1, 7, 8, 32, 33, 100))),
         "lfsr_pointwise_wgrad_workspace_floats": ([c_ll, c_i, c_i], itertools.product((0, 1, 255, 300, 4097, 70001, 1 << 20, (1 << 31) - 1, 1 << 31), (16, 32, 64), (16, 64, 128, 144, 256))),
         "lfsr_linear_wgrad_workspace_floats": ([c_ll, c_i, c_i], itertools.product((0, 1, 63, 300, 4097, 70001, 1 << 20, (1 << 31) - 129, (1 << 31) - 128), (64, 128, 256, 576, 1024, 96), (64, 128, 256, 32))),
         "lfsr_conv3x3_wide_wgrad_workspace_floats": ([c_i] * 4, itertools.product((128, 320, 64), (0, 1, 2, 3, 25, 300, 1000), (1, 4, 5, 8, 33), (1, 6, 32, 33, 65))),
         "lfsr_angconv_bwd_workspace_floats": ([c_i] * 4, itertools.product((0, 1, 2, 8), (1, 3, 5, 7, 9, 15, 16), (1, 5, 8, 32, 33), (1, 6, 8, 32, 64))),
         "lfsr_epiconv_hv_bwd_workspace_floats": ([c_i] * 4, itertools.product((0, 1, 2, 8), (1, 3, 5, 7, 9, 15, 16), (1, 5, 8, 32, 33), (1, 6, 8, 32, 64)))}
SIZES = {k: (a, list(v)) for k, (a, v) in SIZES.items()}


def bind(path):
    lib = C.CDLL(os.path.abspath(path))
    lib.lfsr_conv3x3_wgrad.argtypes = [c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_sz, c_i, c_i, c_i, c_i, c_p]
    lib.lfsr_pointwise_wgrad.argtypes = [c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_sz, c_ll, c_i, c_p]
    lib.lfsr_linear_wgrad.argtypes = [c_p, c_i, c_p, c_i, c_p, c_p, c_sz, c_ll, c_i, c_i, c_i, c_p]
    lib.lfsr_conv3x3_wide_wgrad.argtypes = [c_p, c_i, c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_sz, c_i, c_i, c_i, c_i, c_p]
    lib.lfsr_angconv_bwd.argtypes = [c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_i, c_i, c_i, c_i, c_f, c_p]
    lib.lfsr_epiconv_hv_bwd.argtypes = [c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_i, c_i, c_i, c_i, c_f, c_p]
    for name, (args, _) in SIZES.items():
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, c_sz
    for m in MODES:
        getattr(lib, m).argtypes = [c_i]
    return lib


def sizes(ref, new):
    """every value of the six workspace functions, under every selection; returns the number of differences"""
    bad = 0
    print("| selection | workspace values compared | equal |\n|---|---|---|")
    for name, env, modes in SELECTIONS:
        for k in SELECTORS:
            os.environ.pop(k, None)
        os.environ.update(env)
        n = same = 0
        for lib in (ref, new):
            for m, v in modes.items():
                assert getattr(lib, m)(v) == 0
        for fn, (_, inputs) in SIZES.items():
            for args in inputs:
                a, b = getattr(ref, fn)(*args), getattr(new, fn)(*args)
                n += 1; same += a == b
                if a != b:
                    bad += 1
                    print(f"DIFFERS: {name} {fn}{args}: {a} vs {b}", flush=True)
        for lib in (ref, new):
            for m in modes:
                assert getattr(lib, m)(0) == 0
        print(f"| {name} | {n} | {same} |", flush=True)
    return bad


def calls(lib, st):
    """every call of the comparison: name -> (rc, the buffers it may have written)"""
    P = lambda t: t.data_ptr() if t is not None else None
    g = torch.Generator(device="cuda").manual_seed(23)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    full = lambda *s: torch.full(s, 7.0, device="cuda")
    out = {}

    def run(key, n_ws, call, *written):
        for acc in (0, 1):
            bufs = [full(*b.shape) for b in written]
            ws = full(n_ws + 64)
            out[f"{key} acc={acc}"] = (call(ws, acc, *bufs), ws, *bufs)

    for n_img, h, w in CONV3:
        dy, x = rnd(n_img * h * w, 72), rnd(n_img * h * w, 68)
        n_ws = lib.lfsr_conv3x3_wgrad_workspace_floats(n_img, h, w)
        run(f"conv3x3_wgrad {(n_img, h, w)}", n_ws,
            lambda ws, acc, dw: lib.lfsr_conv3x3_wgrad(P(dy), 72, 8, P(x), 68, 4, P(dw), P(ws), n_ws, n_img, h, w, acc, st), torch.empty(64, 64, 3, 3))
    for M, cout, cin in POINTWISE:
        dy, x = rnd(M, cout + 8), rnd(M, cin + 4)
        n_ws = lib.lfsr_pointwise_wgrad_workspace_floats(M, cout, cin)
        run(f"pointwise_wgrad {(M, cout, cin)}", n_ws,
            lambda ws, acc, dw: lib.lfsr_pointwise_wgrad(P(dy), cout + 8, 4, cout, P(x), cin + 4, 4, cin, P(dw), P(ws), n_ws, M, acc, st), torch.empty(cout, cin))
    for M, cout, cin in LINEAR:
        dy, x = rnd(M, cout), rnd(M, cin + 4)
        n_ws = lib.lfsr_linear_wgrad_workspace_floats(M, cout, cin)
        run(f"linear_wgrad {(M, cout, cin)}", n_ws,
            lambda ws, acc, dw: lib.lfsr_linear_wgrad(P(dy), cout, P(x), cin + 4, P(dw), P(ws), n_ws, M, cout, cin, acc, st), torch.empty(cout, cin))
        run(f"linear_wgrad {(M, cout, cin)} ws - 1", n_ws,
            lambda ws, acc, dw: lib.lfsr_linear_wgrad(P(dy), cout, P(x), cin + 4, P(dw), P(ws), n_ws - 1, M, cout, cin, acc, st), torch.empty(cout, cin))
    for cin, n_img, h, w in WIDE:
        dy, x = rnd(n_img * h * w, 72), rnd(n_img * h * w, cin + 4)
        n_ws = lib.lfsr_conv3x3_wide_wgrad_workspace_floats(cin, n_img, h, w)
        run(f"conv3x3_wide_wgrad {(cin, n_img, h, w)}", n_ws,
            lambda ws, acc, dw: lib.lfsr_conv3x3_wide_wgrad(P(dy), 72, 8, P(x), cin + 4, 4, cin, P(dw), P(ws), n_ws, n_img, h, w, acc, st), torch.empty(64, cin, 3, 3))
    for B, A, h, w in GEOMS:
        npix, nlr, nepi, L = B * A * A * h * w, B * h * w, B * A * h * w, 0.1
        x, dy, y = rnd(npix, 64), rnd(npix, 144), rnd(npix, 144)
        a16, eh, ev = rnd(nlr, 16), rnd(nepi, 32), rnd(nepi, 32)
        wa0, wa2 = rnd(16, 64, A, A) * 0.03, rnd(16 * A * A, 16, 1, 1) * 0.2
        we0, we2 = rnd(32, 64, 1, A * A) * 0.03, rnd(32 * A, 32, 1, 1) * 0.15
        for tag, yy in (("", y), (" y=NULL", None)):
            n_ws = lib.lfsr_angconv_bwd_workspace_floats(B, A, h, w)
            ws, dx, dw0, dw2 = full(n_ws + 64), full(npix, 64), full(16, 64, A, A), full(16 * A * A, 16)
            out[f"angconv_bwd {(B, A, h, w)}{tag}"] = (lib.lfsr_angconv_bwd(P(dy), 144, 64, P(yy), 144, 64, P(x), P(a16), P(wa0), P(wa2), P(dx), P(dw0), P(dw2), P(ws), n_ws,
                                                                             B, A, h, w, L, st), ws, dx, dw0, dw2)
            n_ws = lib.lfsr_epiconv_hv_bwd_workspace_floats(B, A, h, w)
            ws, dx, dw0, dw2 = full(n_ws + 64), full(npix, 64), full(32, 64, 1, A * A), full(32 * A, 32)
            out[f"epiconv_hv_bwd {(B, A, h, w)}{tag}"] = (lib.lfsr_epiconv_hv_bwd(P(dy), 144, 80, 112, P(yy), 144, 80, 112, P(x), P(eh), P(ev), P(we0), P(we2), P(dx), P(dw0),
                                                                                   P(dw2), P(ws), n_ws, B, A, h, w, L, st), ws, dx, dw0, dw2)
    torch.cuda.synchronize()
    return out


def main():
    assert os.environ.get("LFSR_LAB"), "the selectors are read only under LFSR_LAB"
    (rt, ref), (nt, new) = [(t, bind(p)) for t, p in (a.split("=", 1) for a in sys.argv[1:3])]
    bad = sizes(ref, new)
    if "--sizes-only" in sys.argv:
        print("ALL EQUAL" if not bad else f"{bad} DIFFERENCES")
        return 1 if bad else 0
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    print(f"\n| selection | calls compared ({rt} vs {nt}) | return codes | buffers (workspace, dW, dx) |\n|---|---|---|---|")
    for name, env, modes in SELECTIONS:
        for k in SELECTORS:
            os.environ.pop(k, None)
        os.environ.update(env)
        res = []
        for lib in (ref, new):
            for m, v in modes.items():
                assert getattr(lib, m)(v) == 0
            res.append(calls(lib, st))
            for m in modes:
                assert getattr(lib, m)(0) == 0
        n = nrc = nbuf = 0
        codes = set()
        for key, (rc, ws, *bufs) in res[0].items():
            rc2, ws2, *bufs2 = res[1][key]
            # of the workspace (its size may differ: the table above) the guard of 64 floats behind it
            eq = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
            same = all(eq(a, b) for a, b in zip(bufs, bufs2)) and eq(ws[-64:], ws2[-64:]) and bool((ws[-64:] == 7.0).all())
            n += 1; nrc += rc == rc2; nbuf += same; codes.add(rc)
            if rc != rc2 or not same:
                bad += 1
                print(f"DIFFERS: {name} {key}: rc {rc} vs {rc2}, buffers {'equal' if same else 'differ'}", flush=True)
        print(f"| {name} | {n} | equal, {nrc} of {n} (values seen: {sorted(codes)}) | equal, {nbuf} of {n} |", flush=True)
    print("ALL EQUAL" if not bad else f"{bad} DIFFERENCES")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
