"""CPU: the host-only parts of DistgSSR's training C ABI -- the gradient bucket follows the state_dict order of the golden specs."""
import ctypes as C

from lfsr_amd import capi
from tests.helpers import model_case

TAGS = ("a5h8s4", "a3h6w8s2")


def test_bucket_layout_follows_state_dict():
    lib = capi.load()
    for tag in TAGS:
        case, sd, _, _ = model_case("DistgSSR", tag)
        ctx = C.c_void_p()
        capi.check(lib.lfsr_distgssr_create(C.byref(ctx), case["A"], case["s"], 4, 4, 64), "distgssr_create")
        try:
            n = lib.lfsr_distgssr_num_params(ctx)
            assert n == case["n_params"] == sum(v.size for v in sd.values())
            o = 0
            for k, _ in case["spec"]:
                off, numel = capi.c_sz(0), capi.c_sz(0)
                capi.check(lib.lfsr_distgssr_param_offset(ctx, k.encode(), C.byref(off), C.byref(numel)), k)
                assert (off.value, numel.value) == (o, sd[k].size), k
                o += numel.value
            assert o == n
            for k in (b"no.such.weight", b"", b"init_conv.weight#T"):
                assert lib.lfsr_distgssr_param_offset(ctx, k, None, None) != 0, k
        finally:
            lib.lfsr_distgssr_destroy(ctx)
