"""CPU: the DistgSSR branch family keeps one reader of its selectors and one spelling of its pack layout.  Reads the sources of csrc/ as text: the lab selectors
LFSR_EPI, LFSR_EPI_ORDER, LFSR_ANG and LFSR_DISTG_TAIL are arguments of lfsr_sel( in distg_branch.cpp (lfsr_branch_sel) and nowhere else, and the sums that place
the copies inside the EPIConv.0 / EPIConv.2 packs are written out in lfsr_internal.h only (LFSR_EPI0_*_OFF, LFSR_EPI2_PLANES_OFF)."""
import glob
import os
import re

import lfsr_amd

CSRC = os.path.join(lfsr_amd.PKG_DIR, "csrc")
SELECTORS = ("LFSR_EPI", "LFSR_EPI_ORDER", "LFSR_ANG", "LFSR_DISTG_TAIL")
LAYOUT_SUMS = ("25 * 32 * 64 +", "+ 160 * 32")


def sources():
    files = sorted(f for ext in ("hip", "cpp", "h") for f in glob.glob(os.path.join(CSRC, "*." + ext)))
    assert len(files) > 60 and any(f.endswith("distg_branch.cpp") for f in files), len(files)
    return {os.path.basename(f): open(f).read() for f in files}


def test_the_branch_selectors_have_one_reader():
    src = sources()
    for name in SELECTORS:
        quoted = '"' + name + '"'
        users = sorted(f for f, text in src.items() if quoted in text)
        assert users == ["distg_branch.cpp"], (name, users)
        text = src["distg_branch.cpp"]
        assert text.count(quoted) == len(re.findall(r"lfsr_sel\(\s*" + re.escape(quoted) + r"\s*\)", text)) >= 1, name


def test_the_epi_pack_layout_is_spelled_once():
    src = sources()
    for s in LAYOUT_SUMS:
        users = sorted(f for f, text in src.items() if s in text and f != "lfsr_internal.h")
        assert not users, (s, users)
    head = src["lfsr_internal.h"]
    for macro in ("LFSR_EPI0_WINO_OFF", "LFSR_EPI0_PLANES_OFF", "LFSR_EPI2_PLANES_OFF"):
        assert re.search(r"#define\s+" + macro + r"\b", head), macro
