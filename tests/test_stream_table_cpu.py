"""CPU: the operator table of tests/test_gpu_streams.py covers the header.  Every entry point of include/lfsr_hip.h whose last parameter is the caller's stream is in
tests/stream_ops.py:OPS, is driven by a whole-model case (MODEL_COVERED) or is in EXEMPT with a reason -- so a new entry point cannot arrive untested off the
default stream."""
import os
import re

from tests import stream_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_entry_points():
    src = open(os.path.join(ROOT, "include", "lfsr_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    decls = re.findall(r"\b(lfsr_[a-z0-9_]+)\s*\(([^;{()]*)\)\s*;", src)
    return [name for name, args in decls if re.search(r"\bvoid\s*\*\s*stream$", args.strip())]


def test_every_stream_entry_point_is_tabled_covered_or_exempt():
    names = stream_entry_points()
    assert len(names) == len(set(names)) and len(names) >= 80, len(names)
    tabled, covered, exempt = set(stream_ops.OPS), stream_ops.MODEL_COVERED, set(stream_ops.EXEMPT)
    missing = [n for n in names if n not in tabled | covered | exempt]
    assert not missing, missing
    # nothing stale, nothing twice
    assert not (tabled | covered | exempt) - set(names), sorted((tabled | covered | exempt) - set(names))
    assert not tabled & covered and not tabled & exempt and not covered & exempt


def test_whole_model_coverage_names_only_life_cycle_calls():
    for n in stream_ops.MODEL_COVERED:
        assert re.fullmatch(r"lfsr_(distgssr|epit|lft|internet|lfssr)_(forward|forward_train|backward|load_param|finalize)", n), n
    assert not [n for n in stream_ops.MODEL_COVERED if n.startswith("lfsr_lfssr_") and n.endswith(("forward_train", "backward"))]


def test_exemptions_are_the_two_allowed_kinds():
    for n, reason in stream_ops.EXEMPT.items():
        assert n == "lfsr_allreduce" or n.endswith("_forward_taps"), n
        assert reason and "\n" not in reason


def test_the_multi_launch_operators_are_in_the_table():
    for n in ("conv3x3_wgrad", "pointwise_wgrad", "linear_wgrad", "conv3x3_wide_wgrad", "angconv_bwd", "epiconv_hv_bwd", "up_tail_bwd", "window_attn_bwd",
              "conv3x3_ps2_fwd", "lfssr_tail_fwd", "view_metrics", "lf_divide", "lf_integrate", "pack_conv_weight", "pack_conv_weight_tr", "pack_up0_weight_tr"):
        assert "lfsr_" + n in stream_ops.OPS, n
