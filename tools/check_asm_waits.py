"""The streaming loops of k_distg_tail (distg_tail.hip) and k_epi_b3<false> (epi_b3.hip) request a step's rows first and wait only for loads older than the
row they are about to use, so the rows just requested stay in flight under the step's MFMAs.  The compiler places those waits; a load behind a run-time branch,
or a register copied right after its load, makes it drain the memory counter instead.  This reads the gfx950 ISA the Makefile's flags give and checks
  distg_tail.hip  k_distg_tail: in the view loop (the innermost loop holding bf16 MFMAs) no s_waitcnt has a vmcnt below the number of loads a body issues for
                  the next view (never below 6: four SpaConv.2 row loads and two t_V row loads); ScratchSize 0; at most 256 VGPRs
  epi_b3.hip      k_epi_b3<false>: in the step loop every wait in front of the weights' ds_write_b128 leaves at least the four X loads outstanding; ScratchSize 0
usage: python tools/check_asm_waits.py [--only tail|epi] [file.hip]      (a file argument replaces the source of the one kernel checked, e.g. an older revision)"""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, [d for d in sorted(os.listdir(ROOT)) if d.endswith("_amd") and os.path.isdir(os.path.join(ROOT, d, "csrc"))][0], "csrc")


def kernel_isa(src, symbol_part):
    """(instructions-and-labels of the kernel whose mangled name holds symbol_part, its metadata comment lines)"""
    with tempfile.NamedTemporaryFile(suffix=".s") as t:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "-I", CSRC, "-S", "--cuda-device-only", "-o", t.name, src],
                              stderr=subprocess.DEVNULL)
        text = open(t.name).read().split("\n")
    start = [i for i, l in enumerate(text) if re.match(r"^_Z\w*" + symbol_part + r"\w*:", l)]
    assert len(start) == 1, (symbol_part, start)
    end = next(i for i in range(start[0], len(text)) if text[i].strip().startswith(".Lfunc_end"))
    meta = next(i for i in range(end, len(text)) if "ScratchSize" in text[i])
    body = [l.split(";")[0].strip() if not l.startswith(".LBB") else l.split(":")[0] + ":" for l in text[start[0] + 1:end]]
    return [l for l in body if l and not l.startswith("//") and (not l.startswith(".") or l.startswith(".LBB"))], "\n".join(text[meta - 8:meta + 12])


def innermost_loop(ins, holds):
    """the shortest backward-branch span [label .. branch] that contains an instruction starting with `holds`"""
    at = {l[:-1]: i for i, l in enumerate(ins) if l.endswith(":")}
    best = None
    for i, l in enumerate(ins):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\w+)", l)
        if m and m.group(1) in at and at[m.group(1)] < i:
            a = at[m.group(1)]
            if any(x.startswith(holds) for x in ins[a:i]) and (best is None or i - a < best[1] - best[0]): best = (a, i)
    assert best, "no loop holding " + holds
    return ins[best[0]:best[1] + 1]


def vmcnt(l):
    m = re.search(r"vmcnt\((\d+)\)", l)
    return int(m.group(1)) if m else None


def meta_int(meta, key):
    return int(re.search(key + r":\s*(\d+)", meta).group(1))


def check_tail(src):
    ins, meta = kernel_isa(src, "k_distg_tail")
    loop = innermost_loop(ins, "v_mfma_f32_16x16x32_bf16")
    n_mfma = sum(l.startswith("v_mfma_f32_16x16x32_bf16") for l in loop)
    n_load = sum(l.startswith("buffer_load_dwordx4") for l in loop)
    assert n_mfma == 2 * 144, n_mfma                       # two bodies
    per_body = n_load // 2
    need = max(6, per_body)
    waits = [vmcnt(l) for l in loop if l.startswith("s_waitcnt") and vmcnt(l) is not None]
    print(f"k_distg_tail: view loop of {len(loop)} instructions, {per_body} loads per body, vmcnt waits {waits}; NumVgprs {meta_int(meta, 'NumVgprs')}, "
          f"ScratchSize {meta_int(meta, 'ScratchSize')}")
    bad = [w for w in waits if w < need]
    if bad: print(f"k_distg_tail: waits below the {need} loads a body keeps in flight: {bad}")
    if not waits: print("k_distg_tail: no vmcnt wait in the view loop"); bad = [None]
    ok = not bad and meta_int(meta, "ScratchSize") == 0 and meta_int(meta, "NumVgprs") <= 256
    return ok


def check_epi(src):
    ins, meta = kernel_isa(src, "k_epi_b3ILb0E")
    loop = innermost_loop(ins, "v_mfma_f32_16x16x32_bf16")
    # the waits between the last MFMA of a step and the last of its weight stores
    left, last_mfma = [], None
    for i, l in enumerate(loop):
        if l.startswith("v_mfma"): last_mfma = i
        if l.startswith("ds_write_b128") and last_mfma is not None:
            left += [vmcnt(x) for x in loop[last_mfma:i] if x.startswith("s_waitcnt") and vmcnt(x) is not None]
            last_mfma = i
    print(f"k_epi_b3<false>: step loop of {len(loop)} instructions, vmcnt waits in front of the weight stores {left}; NumVgprs {meta_int(meta, 'NumVgprs')}, "
          f"ScratchSize {meta_int(meta, 'ScratchSize')}")
    bad = [w for w in left if w < 4]
    if bad: print(f"k_epi_b3<false>: waits that drain the X loads: {bad}")
    if not left: print("k_epi_b3<false>: no wait found in front of the weight stores"); bad = [None]
    return not bad and meta_int(meta, "ScratchSize") == 0


if __name__ == "__main__":
    args = sys.argv[1:]
    only = None
    if args[:1] == ["--only"]: only, args = args[1], args[2:]
    ok = True
    if only in (None, "tail"): ok &= check_tail(args[0] if args and only == "tail" else os.path.join(CSRC, "distg_tail.hip"))
    if only in (None, "epi"): ok &= check_epi(args[0] if args and only == "epi" else os.path.join(CSRC, "epi_b3.hip"))
    sys.exit(0 if ok else 1)
