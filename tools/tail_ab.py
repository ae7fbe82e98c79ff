#!/usr/bin/env python3
"""A/B timing of builds of the DistgSSR block tail (lfsr_distg_branch_tail_fwd: k_ang_fused<false> + k_epi_b3<false> + k_distg_tail) inside ONE process,
variants interleaved round-robin as tools/conv_ab.py does.  The builds differ in one kernel, so the difference of two figures is that kernel's.
usage: python tools/tail_ab.py tag=lib.so [tag=lib.so ...]      (the first one is the reference for the bit comparison; DT_ABL builds give wrong results)
env: AB_ROUNDS (default 8), AB_REPS (default 20), AB_B (default 32)"""
import ctypes as C, os, sys, statistics
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lfsr_amd import capi

c_p, c_i, c_f = C.c_void_p, C.c_int, C.c_float


def bind(path):
    lib = C.CDLL(os.path.abspath(path))
    lib.lfsr_distg_branch_tail_fwd.restype = c_i
    lib.lfsr_distg_branch_tail_fwd.argtypes = [c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p]
    return lib


def main():
    libs = [(t, bind(p)) for t, p in (a.split("=", 1) for a in sys.argv[1:])]
    rounds, reps = int(os.environ.get("AB_ROUNDS", "8")), int(os.environ.get("AB_REPS", "20"))
    B, A, h, w = int(os.environ.get("AB_B", "32")), 5, 32, 32
    npix = B * A * A * h * w
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(npix, 64, device="cuda", generator=g)
    spa = torch.randn(npix, 64, device="cuda", generator=g)
    wp = (capi.pack_conv_weight(torch.randn(16, 64, A, A, device="cuda", generator=g) * 0.03),
          capi.pack_conv_weight(torch.randn(16 * A * A, 16, 1, 1, device="cuda", generator=g) * 0.2, perm=1, ch=16),
          capi.pack_conv_weight(torch.randn(32, 64, 1, A * A, device="cuda", generator=g) * 0.03),
          capi.pack_conv_weight(torch.randn(32 * A, 32, 1, 1, device="cuda", generator=g) * 0.15),
          capi.pack_conv_weight(torch.randn(64, 144, 1, 1, device="cuda", generator=g) * 0.08))
    y = torch.empty(npix, 64, device="cuda")
    ta = torch.empty(B * h * w, 16, device="cuda")
    th, tv = torch.empty(B * A * h * w, 32, device="cuda"), torch.empty(B * A * h * w, 32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(lib):
        rc = lib.lfsr_distg_branch_tail_fwd(x.data_ptr(), 64, 0, spa.data_ptr(), 64, 0, *[t.data_ptr() for t in wp], ta.data_ptr(), th.data_ptr(), tv.data_ptr(),
                                            y.data_ptr(), 64, 0, B, A, h, w, 0.1, st)
        assert rc == 0, rc

    ref = None
    for t, lib in libs:
        y.zero_(); run(lib); torch.cuda.synchronize()
        if ref is None: ref = y.clone()
        else: print(f"check {t:10s} {'bit-equal to ' + libs[0][0] if torch.equal(y, ref) else 'DIFFERS: max|d| = %.3e' % float((y - ref).abs().max())}", flush=True)
    for _ in range(3):      # warm-up: clocks settle only after ~20 ms of work
        for t, lib in libs:
            for _ in range(20): run(lib)
    torch.cuda.synchronize()
    times = {t: [] for t, _ in libs}
    for rd in range(rounds):
        for t, lib in (libs if rd % 2 == 0 else libs[::-1]):
            for _ in range(3): run(lib)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps): run(lib)
            e1.record(); torch.cuda.synchronize()
            times[t].append(e0.elapsed_time(e1) * 1e3 / reps)
    print(f"B = {B}: us per call of the three launches, median (min..max) over {rounds} rounds of {reps}")
    for t, _ in libs:
        v = times[t]
        print(f"{t:10s} {statistics.median(v):7.1f} ({min(v):6.1f}..{max(v):6.1f})   vs {libs[0][0]}: {statistics.median(v) - statistics.median(times[libs[0][0]]):+6.1f}", flush=True)


if __name__ == "__main__":
    main()
