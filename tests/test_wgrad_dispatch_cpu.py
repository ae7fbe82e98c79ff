"""CPU: the weight-gradient family keeps one reader of its selectors and one place that knows which kernel wrote how many slabs.  Reads the sources of csrc/ as
text: the lab selectors LFSR_WGRAD3, LFSR_WGRAD_EPI and LFSR_WGRAD_PW are arguments of lfsr_sel( in wgrad.cpp (lfsr_wgrad_sel) and nowhere else; the slab counts
(lfsr_wgrad_splits and the _blocks functions) are called from wgrad.cpp and the launcher files alone; lfsr_wgrad_reduce is called from wgrad.cpp alone."""
import glob
import os
import re

import lfsr_amd

CSRC = os.path.join(lfsr_amd.PKG_DIR, "csrc")
SELECTORS = ("LFSR_WGRAD3", "LFSR_WGRAD_EPI", "LFSR_WGRAD_PW")
LAUNCHER_FILES = ("wgrad.hip", "wgrad_bf16.hip", "wgrad_wide_bf16.hip", "lin_wgrad_bf16.hip", "epi0_grad_bf16.hip")
COUNTS = ("lfsr_wgrad_splits", "lfsr_wgrad_conv3_blocks", "lfsr_wgrad_pw144_blocks", "lfsr_wgrad_epi0_blocks", "lfsr_lin_wgrad_bf16_blocks",
          "lfsr_lin_wgrad_bf16_slabs_per_block", "lfsr_wgrad_wide_bf16_blocks")


def sources():
    files = sorted(f for ext in ("hip", "cpp", "h") for f in glob.glob(os.path.join(CSRC, "*." + ext)))
    assert len(files) > 60 and any(f.endswith("wgrad.cpp") for f in files), len(files)
    return {os.path.basename(f): open(f).read() for f in files}


def code(text):
    """the text without its // comments"""
    return re.sub(r"//[^\n]*", "", text)


def test_the_weight_gradient_selectors_have_one_reader():
    src = sources()
    for name in SELECTORS:
        quoted = '"' + name + '"'
        users = sorted(f for f, text in src.items() if quoted in text)
        assert users == ["wgrad.cpp"], (name, users)
        text = src["wgrad.cpp"]
        assert text.count(quoted) == len(re.findall(r"lfsr_sel\(\s*" + re.escape(quoted) + r"\s*\)", text)) == 1, name


def test_the_slab_counts_are_called_from_the_dispatcher_and_the_launchers_only():
    src = sources()
    for fn in COUNTS:
        users = sorted(f for f, text in src.items() if f != "lfsr_internal.h" and re.search(r"\b" + fn + r"\s*\(", code(text)))
        assert "wgrad.cpp" in users, fn
        assert set(users) <= set(LAUNCHER_FILES) | {"wgrad.cpp"}, (fn, users)
    # ... and no other function of that family of names has appeared beside them
    named = set(re.findall(r"\b(lfsr_\w*wgrad\w*_(?:blocks|splits|slabs_per_block))\s*\(", "\n".join(code(t) for t in src.values())))
    assert named == set(COUNTS), named ^ set(COUNTS)


def test_the_reduce_is_called_from_the_dispatcher_only():
    src = sources()
    users = sorted(f for f, text in src.items() if f != "lfsr_internal.h" and re.search(r"\blfsr_wgrad_reduce\s*\(", code(text)))
    assert users == ["wgrad.cpp", "wgrad.hip"], users
    assert len(re.findall(r"\blfsr_wgrad_reduce\s*\(", code(src["wgrad.hip"]))) == 1      # its definition
    assert re.search(r"^int lfsr_wgrad_reduce\(const LfsrWgrad& g,", src["wgrad.hip"], re.M)


def test_no_positional_launcher_is_left():
    src = sources()
    for gone in ("lfsr_wgrad_launch", "lfsr_wgrad_conv3_launch", "lfsr_linear_wgrad_run", "lfsr_wide_wgrad_run", "epi_merged"):
        users = sorted(f for f, text in src.items() if re.search(r"\b" + gone + r"\b", text))
        assert not users, (gone, users)
    head = code(src["lfsr_internal.h"])
    for launcher in re.findall(r"\bint (lfsr_\w*wgrad\w*_launch)\(([^)]*)\)", head):
        assert launcher[1].strip() == "const LfsrWgrad& g, hipStream_t st", launcher
