"""ctypes binding of liblfsr_hip.so (the C ABI declared in include/lfsr_hip.h).

This is the ONLY bridge between the Python host code and the HIP path.  There is no CPU fallback: if
the shared library is missing, or a tensor is not a contiguous CUDA(ROCm) tensor, the call raises.
PyTorch is used for device memory and streams only.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LFSR_HIP_LIB") or os.path.join(_HERE, "liblfsr_hip.so")   # (LFSR_HIP_LIB: a diagnostic / A-B build of the same library)

c_p = C.c_void_p
c_i = C.c_int
c_f = C.c_float
c_sz = C.c_size_t

# name -> (restype, argtypes): mirrors include/lfsr_hip.h (the model life cycles are added below, from _MODELS)
SIGNATURES = {
    "lfsr_version": (C.c_char_p, []),
    "lfsr_sai2macpi": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_macpi2sai": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_pixel_shuffle2d": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_pixel_shuffle1d": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_image_extend": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_lf_divide": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, C.POINTER(c_i), C.POINTER(c_i), c_p]),
    "lfsr_lf_integrate": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_lf_crop_tiles": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_lf_place_tiles": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_nchw_to_vcl": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_vcl_to_nchw": (c_i, [c_p, c_i, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_pack_conv_weight": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_packed_weight_floats": (c_sz, [c_i, c_i, c_i]),
    "lfsr_conv3x3_fwd": (c_i, [c_p, c_i, c_i, c_p, c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_pointwise_fwd": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_angconv_fwd": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_epiconv_fwd": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_epiconv_hv_fwd": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_distg_branch_tail_fwd": (c_i, [c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_initconv_fwd": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_fold_head": (c_i, [c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_p]),
    "lfsr_upsample_head_fwd": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_distgssr_begin_batched_load": (c_i, [c_p]),
    "lfsr_distgssr_forward_taps": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_sz, C.POINTER(c_p), c_p]),
    "lfsr_layernorm_fwd": (c_i, [c_p, c_i, c_i, c_p, c_i, C.c_longlong, C.c_longlong, c_p, c_p, c_p, c_i, c_i, C.c_longlong, c_i, c_f, c_p]),
    "lfsr_conv3x3_n_fwd": (c_i, [c_p, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_angconv3x3_fwd": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_lfssr_conv0_fwd": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_conv3x3_ps2_fwd": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_lfssr_tail_fwd": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_lft_position_fwd": (c_i, [c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_view_metrics": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_mask_views": (c_i, [c_p, c_p, c_p, c_f, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_mask_views_fill": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_linear_fwd": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_i, c_i, c_p, c_i, c_i, C.c_longlong, c_i, c_f, c_p]),
    "lfsr_ycbcr2rgb_views": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, C.POINTER(C.c_double), C.POINTER(C.c_double), c_p]),
    "lfsr_ffn_fwd": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p, c_i, c_i, c_p, c_i, c_i, C.c_longlong, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_ffn_ln_fwd": (c_i, [c_p, c_i, c_i, c_p, c_p, c_f, c_p, c_p, c_p, c_i, c_i, c_p, c_i, c_i, C.c_longlong, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_linear_ln_fwd": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_f, c_i, c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_p, c_i, c_i, c_i, C.c_longlong, c_i, c_p]),
    "lfsr_window_attn_fwd": (c_i, [c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_i, c_i,
                                   C.c_longlong, C.c_longlong, C.c_longlong, c_i, c_i, C.c_longlong, C.c_longlong, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_window_attn_bwd": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_i, c_i, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i,
                                   C.c_longlong, C.c_longlong, C.c_longlong, c_i, c_i, C.c_longlong, C.c_longlong, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_layernorm_bwd_workspace_floats": (c_sz, [c_i]),
    "lfsr_layernorm_bwd": (c_i, [c_p, c_p, C.c_longlong, C.c_longlong, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, C.c_longlong, c_i, c_p]),
    "lfsr_linear_dgrad": (c_i, [c_p, c_i, c_p, c_p, c_i, c_p, c_i, c_p, c_i, C.c_longlong, c_i, c_p]),
    "lfsr_up_tail_bwd_workspace_floats": (c_sz, []),
    "lfsr_up_tail_bwd": (c_i, [c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_pack_up0_weight_tr": (c_i, [c_p, c_p, c_i, c_p]),
    "lfsr_upsample_ps_fwd": (c_i, [c_p, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_up_tail_fwd": (c_i, [c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_hr_tail_fwd": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_packed_weight_tr_floats": (c_sz, [c_i, c_i, c_i]),
    "lfsr_pack_conv_weight_tr": (c_i, [c_p, c_p, c_i, c_i, c_i, c_p]),
    "lfsr_conv3x3_dgrad": (c_i, [c_p, c_i, c_i, c_p, c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_i, c_i, c_f, c_i, c_i, c_i, c_p]),
    "lfsr_conv3x3_wgrad_workspace_floats": (c_sz, [c_i, c_i, c_i]),
    "lfsr_conv3x3_wgrad": (c_i, [c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_sz, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_pointwise_dgrad": (c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_f, C.c_longlong, c_p]),
    "lfsr_pointwise_wgrad_workspace_floats": (c_sz, [C.c_longlong, c_i, c_i]),
    "lfsr_pointwise_wgrad": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_sz, C.c_longlong, c_i, c_p]),
    "lfsr_upsample_head_dgrad": (c_i, [c_p, c_p, c_p, c_p, c_i, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_comm_available": (c_i, []),
    "lfsr_comm_unique_id": (c_i, [c_p]),
    "lfsr_comm_init": (c_i, [C.POINTER(c_p), c_i, c_i, c_p]),
    "lfsr_comm_destroy": (c_i, [c_p]),
    "lfsr_allreduce": (c_i, [c_p, c_sz, c_p, c_p]),
    "lfsr_angconv_bwd_workspace_floats": (c_sz, [c_i, c_i, c_i, c_i]),
    "lfsr_angconv_bwd": (c_i, [c_p, c_i, c_i, c_p, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_i, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_epiconv_hv_bwd_workspace_floats": (c_sz, [c_i, c_i, c_i, c_i]),
    "lfsr_epiconv_hv_bwd": (c_i, [c_p, c_i, c_i, c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz, c_i, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_set_arithmetic": (c_i, [c_i]),
    "lfsr_get_arithmetic": (c_i, []),
    "lfsr_set_grad_arithmetic": (c_i, [c_i]),
    "lfsr_get_grad_arithmetic": (c_i, []),
    "lfsr_set_gemm_arithmetic": (c_i, [c_i]),
    "lfsr_get_gemm_arithmetic": (c_i, []),
    "lfsr_set_branch_arithmetic": (c_i, [c_i]),
    "lfsr_get_branch_arithmetic": (c_i, []),
    "lfsr_set_ang_arithmetic": (c_i, [c_i]),
    "lfsr_get_ang_arithmetic": (c_i, []),
    "lfsr_set_wide_arithmetic": (c_i, [c_i]),
    "lfsr_get_wide_arithmetic": (c_i, []),
    "lfsr_set_lin_grad_arithmetic": (c_i, [c_i]),
    "lfsr_get_lin_grad_arithmetic": (c_i, []),
    "lfsr_linear_wgrad_workspace_floats": (c_sz, [C.c_longlong, c_i, c_i]),
    "lfsr_linear_wgrad": (c_i, [c_p, c_i, c_p, c_i, c_p, c_p, c_sz, C.c_longlong, c_i, c_i, c_i, c_p]),
    "lfsr_set_wide_train_arithmetic": (c_i, [c_i]),
    "lfsr_get_wide_train_arithmetic": (c_i, []),
    "lfsr_set_branch_grad_arithmetic": (c_i, [c_i]),
    "lfsr_get_branch_grad_arithmetic": (c_i, []),
    "lfsr_conv3x3_wide_wgrad_workspace_floats": (c_sz, [c_i, c_i, c_i, c_i]),
    "lfsr_conv3x3_wide_wgrad": (c_i, [c_p, c_i, c_i, c_p, c_i, c_i, c_i, c_p, c_p, c_sz, c_i, c_i, c_i, c_i, c_p]),
    "lfsr_conv3x3_wide_fwd":(c_i, [c_p, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_p, c_i, c_i, c_i, c_i, c_i, c_f, c_p]),
    "lfsr_op_profile": (c_i, [c_i]),
    "lfsr_op_profile_read": (C.c_longlong, [C.c_char_p, c_sz]),
    "lfsr_distgssr_profile": (c_i, [c_p, c_i]),
    "lfsr_distgssr_profile_read": (c_i, [c_p, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]),
}


def _model_signatures(name, n_create_ints, trainable):
    """the C life cycle of one model (what ModelRuntime drives): lfsr_<name>_create (ctx**, A, scale and n_create_ints more ints), destroy,
    packed_bytes, set_packed, load_param, finalize, workspace_bytes, forward; the trainable ones add num_params, param_offset,
    train_workspace_bytes, forward_train, train_saved, backward"""
    fwd = [c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_sz, c_p]          # ctx, x, out, B, h, w, workspace, workspace_bytes, stream
    sig = {"create": (c_i, [C.POINTER(c_p), c_i, c_i] + [c_i] * n_create_ints),
           "destroy": (None, [c_p]),
           "packed_bytes": (c_sz, [c_p]),
           "set_packed": (c_i, [c_p, c_p, c_sz]),
           "load_param": (c_i, [c_p, C.c_char_p, c_p, c_sz, c_p]),
           "finalize": (c_i, [c_p, c_p]),
           "workspace_bytes": (c_sz, [c_p, c_i, c_i, c_i]),
           "forward": (c_i, fwd)}
    if trainable:
        sig.update({"num_params": (c_sz, [c_p]),
                    "param_offset": (c_i, [c_p, C.c_char_p, C.POINTER(c_sz), C.POINTER(c_sz)]),
                    "train_workspace_bytes": (c_sz, [c_p, c_i, c_i, c_i]),
                    "forward_train": (c_i, list(fwd)),
                    "train_saved": (c_i, [c_p, c_i, c_i, c_i, c_i, c_i, C.POINTER(c_sz), C.POINTER(c_sz)]),
                    "backward": (c_i, [c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_sz, c_p, c_sz, c_p])})
    return {f"lfsr_{name}_{fn}": s for fn, s in sig.items()}


# (model, ints lfsr_<model>_create takes after A and scale, trainable)
_MODELS = (("distgssr", 3, True), ("internet", 2, True), ("lft", 2, True), ("epit", 2, True), ("lfssr", 1, False))
for _m in _MODELS:
    SIGNATURES.update(_model_signatures(*_m))

_lib = None


class LfsrError(RuntimeError):
    pass


def load():
    """dlopen the C-ABI library (no GPU needed) and bind every declared symbol; raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LfsrError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(there is no CPU fallback for the HIP path)")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)   # AttributeError if the .so does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc, what):
    if rc != 0:
        if rc == -1:
            msg = "bad argument"
        elif rc == -2:
            msg = "workspace too small"
        else:
            msg = f"HIP error {-rc - 1000}"
        raise LfsrError(f"{what}: {msg} (rc={rc})")


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_ptr(t, what="tensor"):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise LfsrError(f"{what} must be a CUDA/ROCm tensor: the HIP path has no CPU fallback")
    if not t.is_contiguous():
        raise LfsrError(f"{what} must be contiguous")
    return C.c_void_p(t.data_ptr())


def _elem(t):
    eb = t.element_size()
    if eb not in (2, 4):
        raise LfsrError(f"unsupported element size {eb}")
    return eb


ARITH_DEFAULT, ARITH_F32, ARITH_BF16 = 0, 1, 2


def set_arithmetic(mode):
    """lfsr_set_arithmetic: ARITH_DEFAULT (three exact bf16 terms on the bf16 MFMA pipe where a kernel has that form), ARITH_F32 (every GEMM on fp32 MFMA) or
    ARITH_BF16 (the default, but the 64 -> 64 per-view 3x3 forward conv rounds its activations and weights to bf16, fp32 accumulation); process-wide"""
    check(load().lfsr_set_arithmetic(int(mode)), "set_arithmetic")


def get_arithmetic():
    """lfsr_get_arithmetic: the mode the next launch runs in"""
    return int(load().lfsr_get_arithmetic())


GRAD_ARITH_DEFAULT, GRAD_ARITH_BF16 = 0, 1


def set_grad_arithmetic(mode):
    """lfsr_set_grad_arithmetic: GRAD_ARITH_DEFAULT (every gradient kernel as it is) or GRAD_ARITH_BF16 (the 64 -> 64 per-view 3x3 conv's data and weight
    gradients round their operands to bf16, fp32 accumulation); process-wide, independent of set_arithmetic"""
    check(load().lfsr_set_grad_arithmetic(int(mode)), "set_grad_arithmetic")


def get_grad_arithmetic():
    """lfsr_get_grad_arithmetic: the mode the next gradient launch runs in"""
    return int(load().lfsr_get_grad_arithmetic())


GEMM_ARITH_DEFAULT, GEMM_ARITH_BF16 = 0, 1


def set_gemm_arithmetic(mode):
    """lfsr_set_gemm_arithmetic: GEMM_ARITH_DEFAULT (the transformer GEMMs as they are) or GEMM_ARITH_BF16 (the K = 64 / 128 bias-free linears, the LayerNorm + q | k | v
    projections and the feed-forward blocks round their operands to bf16, fp32 accumulation); process-wide, independent of set_arithmetic and set_grad_arithmetic"""
    check(load().lfsr_set_gemm_arithmetic(int(mode)), "set_gemm_arithmetic")


def get_gemm_arithmetic():
    """lfsr_get_gemm_arithmetic: the mode the next linear / feed-forward launch runs in"""
    return int(load().lfsr_get_gemm_arithmetic())


BRANCH_ARITH_DEFAULT, BRANCH_ARITH_BF16 = 0, 1


def set_branch_arithmetic(mode):
    """lfsr_set_branch_arithmetic: BRANCH_ARITH_DEFAULT (DistgSSR's branches and block tail as they are) or BRANCH_ARITH_BF16 (EPIConv.0, EPIConv.2 and fuse.0 of the
    fused block tail at angRes 5 round their operands to bf16, fp32 accumulation); process-wide, independent of the other three switches"""
    check(load().lfsr_set_branch_arithmetic(int(mode)), "set_branch_arithmetic")


def get_branch_arithmetic():
    """lfsr_get_branch_arithmetic: the mode the next DistgSSR branch / block-tail launch runs in"""
    return int(load().lfsr_get_branch_arithmetic())


ANG_ARITH_DEFAULT, ANG_ARITH_BF16 = 0, 1


def set_ang_arithmetic(mode):
    """lfsr_set_ang_arithmetic: ANG_ARITH_DEFAULT (LFSSR's angular 3x3 conv as it is) or ANG_ARITH_BF16 (lfsr_angconv3x3_fwd rounds its operands to bf16, fp32
    accumulation); process-wide, independent of the other four switches"""
    check(load().lfsr_set_ang_arithmetic(int(mode)), "set_ang_arithmetic")


def get_ang_arithmetic():
    """lfsr_get_ang_arithmetic: the mode the next lfsr_angconv3x3_fwd launch runs in"""
    return int(load().lfsr_get_ang_arithmetic())


WIDE_ARITH_DEFAULT, WIDE_ARITH_BF16 = 0, 1


def set_wide_arithmetic(mode):
    """lfsr_set_wide_arithmetic: WIDE_ARITH_DEFAULT (LF_InterNet's wide per-view 3x3 convs as they are) or WIDE_ARITH_BF16 (lfsr_conv3x3_wide_fwd, and with it the
    SpaConvSq and SpaBottle of the inference forward, rounds its operands to bf16, fp32 accumulation); process-wide, independent of the other five switches"""
    check(load().lfsr_set_wide_arithmetic(int(mode)), "set_wide_arithmetic")


def get_wide_arithmetic():
    """lfsr_get_wide_arithmetic: the mode the next lfsr_conv3x3_wide_fwd launch runs in"""
    return int(load().lfsr_get_wide_arithmetic())


LIN_GRAD_ARITH_DEFAULT, LIN_GRAD_ARITH_BF16 = 0, 1


def set_lin_grad_arithmetic(mode):
    """lfsr_set_lin_grad_arithmetic: LIN_GRAD_ARITH_DEFAULT (the linears' weight and data gradients as they are) or LIN_GRAD_ARITH_BF16 (lfsr_linear_wgrad and
    lfsr_linear_dgrad, and with them every linear of the EPIT and LFT backward, round their operands to bf16, fp32 accumulation); process-wide, independent of the
    other six switches"""
    check(load().lfsr_set_lin_grad_arithmetic(int(mode)), "set_lin_grad_arithmetic")


def get_lin_grad_arithmetic():
    """lfsr_get_lin_grad_arithmetic: the mode the next lfsr_linear_wgrad / lfsr_linear_dgrad launch runs in"""
    return int(load().lfsr_get_lin_grad_arithmetic())


WIDE_TRAIN_ARITH_DEFAULT, WIDE_TRAIN_ARITH_BF16_WGRAD, WIDE_TRAIN_ARITH_BF16 = 0, 1, 2


def set_wide_train_arithmetic(mode):
    """lfsr_set_wide_train_arithmetic: WIDE_TRAIN_ARITH_DEFAULT (LF_InterNet's wide per-view 3x3 convs in training as they are), WIDE_TRAIN_ARITH_BF16_WGRAD
    (lfsr_conv3x3_wide_wgrad, and with it the seventeen wide weight gradients of the backward, rounds its operands to bf16, fp32 accumulation) or
    WIDE_TRAIN_ARITH_BF16 (that, and forward_train's wide convs on bf16 operands); process-wide, independent of the other seven switches"""
    check(load().lfsr_set_wide_train_arithmetic(int(mode)), "set_wide_train_arithmetic")


def get_wide_train_arithmetic():
    """lfsr_get_wide_train_arithmetic: the mode the next lfsr_conv3x3_wide_wgrad / lfsr_internet_forward_train / lfsr_internet_backward launch runs in"""
    return int(load().lfsr_get_wide_train_arithmetic())


BRANCH_GRAD_ARITH_DEFAULT, BRANCH_GRAD_ARITH_BF16 = 0, 1


def set_branch_grad_arithmetic(mode):
    """lfsr_set_branch_grad_arithmetic: BRANCH_GRAD_ARITH_DEFAULT (EPIConv.0's gradients as they are) or BRANCH_GRAD_ARITH_BF16 (the EPI-line weight and data
    gradients of EPIConv.0 behind epiconv_hv_bwd and the DistgSSR backward round their operands to bf16, fp32 accumulation); process-wide, independent of the
    other eight switches"""
    check(load().lfsr_set_branch_grad_arithmetic(int(mode)), "set_branch_grad_arithmetic")


def get_branch_grad_arithmetic():
    """lfsr_get_branch_grad_arithmetic: the mode the next lfsr_epiconv_hv_bwd / lfsr_distgssr_backward launch runs in"""
    return int(load().lfsr_get_branch_grad_arithmetic())


def op_profile(enable):
    """switch the library's operator-level timing hooks on (dropping earlier records) or off (lfsr_op_profile)"""
    check(load().lfsr_op_profile(int(bool(enable))), "op_profile")


def op_profile_read():
    """-> {(op, a, b): (total_ms, launches)} of the hooks recorded since op_profile(True) / the last read; waits for the events"""
    lib = load()
    cap = 1 << 18
    buf = C.create_string_buffer(cap)
    need = lib.lfsr_op_profile_read(buf, cap)
    if need < 0:
        check(int(need), "op_profile_read")
    if need > cap:
        raise LfsrError(f"op_profile_read: table of {need} bytes truncated")
    out = {}
    for line in buf.value.decode().splitlines():
        op, a, b, ms, n = line.split()
        out[(op, int(a), int(b))] = (float(ms), int(n))
    return out


# ---------------------------------------------------------------------------------------------------
# a1-a7 on torch tensors
# ---------------------------------------------------------------------------------------------------

def sai2macpi(x, A):
    """SAI2MacPI, DistgSSR.py:145-155."""
    lib = load()
    B, Cc, Hh, Ww = x.shape
    out = torch.empty_like(x)
    check(lib.lfsr_sai2macpi(dev_ptr(x), dev_ptr(out), B, Cc, A, Hh // A, Ww // A, _elem(x), stream_ptr()), "sai2macpi")
    return out


def macpi2sai(x, A):
    """MacPI2SAI, DistgSSR.py:134-142."""
    lib = load()
    B, Cc, Hh, Ww = x.shape
    out = torch.empty_like(x)
    check(lib.lfsr_macpi2sai(dev_ptr(x), dev_ptr(out), B, Cc, A, Hh // A, Ww // A, _elem(x), stream_ptr()), "macpi2sai")
    return out


def pixel_shuffle2d(x, r):
    lib = load()
    B, Crr, H, W = x.shape
    Cc = Crr // (r * r)
    out = torch.empty((B, Cc, H * r, W * r), dtype=x.dtype, device=x.device)
    check(lib.lfsr_pixel_shuffle2d(dev_ptr(x), dev_ptr(out), B, Cc, r, H, W, _elem(x), stream_ptr()), "pixel_shuffle2d")
    return out


def pixel_shuffle1d(x, f):
    """PixelShuffle1D, DistgSSR.py:114-131."""
    lib = load()
    B, fC, H, W = x.shape
    Cc = fC // f
    out = torch.empty((B, Cc, H, W * f), dtype=x.dtype, device=x.device)
    check(lib.lfsr_pixel_shuffle1d(dev_ptr(x), dev_ptr(out), B, Cc, f, H, W, _elem(x), stream_ptr()), "pixel_shuffle1d")
    return out


def image_extend(im, bdr):
    """ImageExtend, utils/utils.py:137-149.  im (..., h, w), bdr = [top, bottom, left, right]."""
    lib = load()
    h, w = im.shape[-2:]
    N = im.numel() // (h * w) if h * w else 0
    out = torch.empty(tuple(im.shape[:-2]) + (h + bdr[0] + bdr[1], w + bdr[2] + bdr[3]), dtype=im.dtype, device=im.device)
    check(lib.lfsr_image_extend(dev_ptr(im), dev_ptr(out), N, h, w, bdr[0], bdr[1], bdr[2], bdr[3], _elem(im), stream_ptr()), "image_extend")
    return out


def lf_divide(data, A, P, S):
    """LFdivide, utils/utils.py:152-166.  data (A*h0, A*w0) -> (numU, numV, A*P, A*P)."""
    lib = load()
    if data.dim() != 2:
        raise LfsrError("LFdivide expects a 2-D (A*h0, A*w0) mosaic")
    h0, w0 = data.shape[0] // A, data.shape[1] // A
    nu, nv = c_i(0), c_i(0)
    check(lib.lfsr_lf_divide(None, None, A, h0, w0, P, S, _elem(data), C.byref(nu), C.byref(nv), None), "lf_divide(count)")
    out = torch.empty((nu.value, nv.value, A * P, A * P), dtype=data.dtype, device=data.device)
    check(lib.lfsr_lf_divide(dev_ptr(data), dev_ptr(out), A, h0, w0, P, S, _elem(data), None, None, stream_ptr()), "lf_divide")
    return out


def lf_integrate(sub, A, pz, stride, h, w):
    """LFintegrate, utils/utils.py:169-178.  sub (numU,numV,A*pz,A*pz) [or 6-D n1 n2 a1 a2 h w] -> (A,A,h,w)."""
    lib = load()
    if sub.dim() == 6:   # the reference accepts the already-split form too (utils.py:170-172)
        n1, n2 = sub.shape[:2]
        sub = sub.permute(0, 1, 2, 4, 3, 5).reshape(n1, n2, A * pz, A * pz).contiguous()
    n1, n2 = sub.shape[:2]
    out = torch.empty((A, A, h, w), dtype=sub.dtype, device=sub.device)
    check(lib.lfsr_lf_integrate(dev_ptr(sub), dev_ptr(out), A, n1, n2, pz, stride, h, w, _elem(sub), stream_ptr()), "lf_integrate")
    return out


def lf_crop_tiles(sub, A, pz, stride):
    """(n,1,A*pz,A*pz) or (n,A*pz,A*pz) SR patches -> (n,A,A,stride,stride): what LFintegrate keeps of each patch (utils/utils.py:169-178)"""
    lib = load()
    n = sub.shape[0]
    if sub.shape[-1] != A * pz or sub.shape[-2] != A * pz or sub.numel() != n * A * pz * A * pz:
        raise LfsrError(f"lf_crop_tiles: bad patch tensor {tuple(sub.shape)} for A={A} pz={pz}")
    sub = sub.contiguous()
    out = torch.empty((n, A, A, stride, stride), dtype=sub.dtype, device=sub.device)
    check(lib.lfsr_lf_crop_tiles(dev_ptr(sub), dev_ptr(out), A, n, pz, stride, _elem(sub), stream_ptr()), "lf_crop_tiles")
    return out


def lf_place_tiles(tiles, out, A, numU, numV, first, stride):
    """tiles (count,A,A,stride,stride) of patches [first, first+count) -> their places in out (A,A,h,w), in place"""
    lib = load()
    tiles = tiles.contiguous()
    if not out.is_contiguous() or out.dtype != tiles.dtype or out.shape[0] != A or out.shape[1] != A:
        raise LfsrError("lf_place_tiles: bad output tensor")
    check(lib.lfsr_lf_place_tiles(dev_ptr(tiles), dev_ptr(out), A, numU, numV, first, tiles.shape[0], stride, out.shape[2], out.shape[3], _elem(tiles), stream_ptr()),
          "lf_place_tiles")
    return out


def nchw_to_vcl(x, A, layout, out=None, choff=0):
    """(B,C,A*h,A*w) NCHW [layout 0 = SAI mosaic, 1 = MacPI] -> VCL (B*A*A*h*w, stride) fp32."""
    lib = load()
    B, Cc, Hh, Ww = x.shape
    h, w = Hh // A, Ww // A
    if out is None:
        out = torch.empty((B * A * A * h * w, Cc), dtype=torch.float32, device=x.device)
    check(lib.lfsr_nchw_to_vcl(dev_ptr(x), dev_ptr(out), out.shape[1], choff, B, Cc, A, h, w, layout, stream_ptr()), "nchw_to_vcl")
    return out


def vcl_to_nchw(v, B, Cc, A, h, w, layout, choff=0):
    lib = load()
    out = torch.empty((B, Cc, A * h, A * w), dtype=torch.float32, device=v.device)
    check(lib.lfsr_vcl_to_nchw(dev_ptr(v), v.shape[1], choff, dev_ptr(out), B, Cc, A, h, w, layout, stream_ptr()), "vcl_to_nchw")
    return out


def pack_conv_weight(w, perm=0, ch=0):
    """(O,C,kh,kw) -> packed [kh*kw][Npad][C] (see include/lfsr_hip.h)."""
    lib = load()
    O, Cc = w.shape[:2]
    taps = w.numel() // (O * Cc)
    n = lib.lfsr_packed_weight_floats(O, Cc, taps)
    out = torch.empty(n, dtype=torch.float32, device=w.device)
    check(lib.lfsr_pack_conv_weight(dev_ptr(w), dev_ptr(out), O, Cc, taps, perm, ch, stream_ptr()), "pack_conv_weight")
    return out


# ---------------------------------------------------------------------------------------------------
# batch limit of one launch sequence
# ---------------------------------------------------------------------------------------------------

def max_patches_per_launch(A, h, w, widest_row_floats, limit=1 << 31):
    """The kernels address their operands with 32-bit BYTE offsets (buffer descriptors: an out-of-range offset is a dropped access), so every activation tensor of one
    forward must stay below 2 GiB -- 1 GiB for DistgSSR, whose F(4x4,3x3) conv kernel keeps one more bit for its "outside the image" offsets: B * A^2 * h * w pixels x the
    widest row (DistgSSR: the 144-channel concat buffer, counted as 160; EPIT / LFT: the 256-float q | k rows).
    LF_InterNet is the exception: its batches are split by 256-float rows too, but its widest tensor is the 320-float concat of the spatial group outputs, which
    therefore passes 2 GiB in one launch sequence (5x5 x 32x32: B = 66..81).  Every kernel that touches it addresses with 64 bits there (the gather-GEMM's
    non-descriptor loads, long-long row indices in the slice copies), and lfsr_internet_forward bounds it at 2^31 FLOATS; checked against fp64 at B = 66 in
    tests/test_gpu_internet_geometries.py::test_forward_batch_66_concat_past_2_gib.
    The C entry points return LFSR_E_ARG beyond that; the runtimes below split a larger batch into equal launches instead (patches are independent and the path is
    batch-invariant bit for bit -- tests/test_gpu_distgssr.py::test_batch32_equals_single_patches -- so the split changes no value)."""
    per_patch = A * A * h * w * widest_row_floats * 4
    return max(1, (limit - 1) // per_patch)


def _forward_in_chunks(fwd, x, nmax):
    return torch.cat([fwd(x[i:i + nmax]) for i in range(0, x.shape[0], nmax)], 0)


class GraphedForward:
    """A model runtime's forward captured into a HIP graph per input shape and replayed (torch.cuda.CUDAGraph = hipGraph on ROCm).

    A forward is one C call that issues ~100-250 kernel launches from the host; at small batches (EPIT / LFT at B = 1: kernels of a few microseconds) the host's
    launch rate is what the step waits for, and a graph replay removes it.  At the headline batch the GPU is the bound and the graph changes nothing.
    The captured launches are exactly the eager ones (same kernels, same arguments, same workspace), so the result is bit-equal (tests/test_gpu_graph.py).
    The returned tensor is the graph's static output: it is overwritten by the next call with the same shape -- clone it to keep it."""

    def __init__(self, rt):
        self.rt = rt
        self.graphs = {}

    def __call__(self, x):
        key = (tuple(x.shape), x.device, x.dtype, get_arithmetic(), get_gemm_arithmetic(), get_branch_arithmetic(), get_ang_arithmetic(), get_wide_arithmetic())      # all are read at launch: a graph holds the kernels of the modes it was captured in
        g = self.graphs.get(key)
        if g is None:
            static_x = x.clone()
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                    # warm-up off the capture: first-launch attribute calls, workspace allocation
                for _ in range(2):
                    self.rt.forward(static_x)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_y = self.rt.forward(static_x)
            # The captured launches hold the raw pointer of the workspace the warm-up left in rt.ws.  The runtime keeps one workspace and drops it when the
            # geometry changes (ModelRuntime._workspace), so the entry owns that tensor: a forward at another shape, here or eager, must not hand the
            # memory a live graph writes to back to the allocator.
            g = self.graphs[key] = (graph, static_x, static_y, tuple(self.rt.ws.values()))
        graph, static_x, static_y = g[:3]
        static_x.copy_(x)
        graph.replay()
        return static_y


# ---------------------------------------------------------------------------------------------------
# whole-model runtimes: every model drives one C-ABI life cycle, lfsr_<name>_create / packed_bytes / set_packed / load_param /
# finalize / workspace_bytes / forward; every one of them trainable: num_params / param_offset /
# train_workspace_bytes / forward_train / train_saved / backward
# ---------------------------------------------------------------------------------------------------

class ModelRuntime:
    """ctx = lfsr_<name>_create(A, scale, *create_args); packed weights and workspaces are torch allocations owned here.
    The training workspace is kept apart from the inference one: a no-grad forward between a training forward and its backward
    leaves the activations that backward reads in place."""

    widest_row_floats, offset_limit = 256, 1 << 31    # max_patches_per_launch: the 256-float q | k rows of EPIT / LFT

    def __init__(self, name, A, scale, *create_args):
        self.lib = load()
        self.name, self.A, self.scale = name, A, scale
        ctx = c_p()
        check(self._f("create")(C.byref(ctx), A, scale, *create_args), f"{name}_create")
        self.ctx = ctx
        self.packed = None
        self.ws = {}                  # the inference workspace
        self.tws = {}                 # the training workspace
        self.train_generation = 0     # bumped by every forward_train: identifies whose activations the training workspace holds

    def _f(self, fn):
        sym = f"lfsr_{self.name}_{fn}"
        if sym not in SIGNATURES:
            raise LfsrError(f"{self.name}: the C ABI has no {sym}")
        return getattr(self.lib, sym)

    def __del__(self):
        try:
            if getattr(self, "ctx", None):
                self._f("destroy")(self.ctx)
                self.ctx = None
        except Exception:
            pass

    def load_state(self, named_tensors, device):
        """named_tensors: iterable of (key, CUDA tensor) with the reference's state_dict names."""
        nbytes = self._f("packed_bytes")(self.ctx)
        if self.packed is None or self.packed.device != device:
            self.packed = torch.empty(nbytes, dtype=torch.uint8, device=device)
        check(self._f("set_packed")(self.ctx, dev_ptr(self.packed), nbytes), f"{self.name}_set_packed")
        st = stream_ptr()
        keep = []     # a batched load (DistgSSRRuntime) reads the tensors at finalize
        for k, t in named_tensors:
            t = t.detach().float().contiguous()
            keep.append(t)
            check(self._f("load_param")(self.ctx, k.encode(), dev_ptr(t, k), t.numel(), st), f"{self.name}_load_param({k})")
        check(self._f("finalize")(self.ctx, st), f"{self.name}_finalize")

    def _geometry(self, x):
        B, c1, Hh, Ww = x.shape
        if c1 != 1 or Hh % self.A or Ww % self.A:
            raise LfsrError(f"bad input shape {tuple(x.shape)} for angRes {self.A}")
        if x.dtype != torch.float32:
            raise LfsrError(f"{self.name} HIP path computes in fp32; got {x.dtype}")
        return B, Hh // self.A, Ww // self.A

    def _output(self, x):
        return torch.empty((x.shape[0], 1, x.shape[2] * self.scale, x.shape[3] * self.scale), dtype=torch.float32, device=x.device)

    def _workspace(self, B, h, w, device, train=False):
        """one live workspace of each kind per runtime"""
        cache = self.tws if train else self.ws
        key = (B, h, w, device)
        if key not in cache:
            n = self.train_workspace_bytes(B, h, w) if train else self._f("workspace_bytes")(self.ctx, B, h, w)
            if train and n == 0:     # refused before anything is allocated
                raise LfsrError(f"{self.name} training: geometry B={B} h={h} w={w} is outside what the training path covers")
            cache.clear()
            cache[key] = torch.empty(n, dtype=torch.uint8, device=device)
        return cache[key]

    def forward(self, x):
        """x (B,1,A*h,A*w) fp32 CUDA -> (B,1,A*h*s,A*w*s)"""
        B, h, w = self._geometry(x)
        x = x.contiguous()
        nmax = max_patches_per_launch(self.A, h, w, self.widest_row_floats, self.offset_limit)
        if B > nmax:
            return _forward_in_chunks(self.forward, x, nmax)
        out = self._output(x)
        ws = self._workspace(B, h, w, x.device)
        check(self._f("forward")(self.ctx, dev_ptr(x), dev_ptr(out), B, h, w, dev_ptr(ws), ws.numel(), stream_ptr()), f"{self.name}_forward")
        return out

    # ---- training: gradients into one flat fp32 bucket in state_dict order ---------------------------
    def num_params(self):
        return self._f("num_params")(self.ctx)

    def param_span(self, key):
        off, n = c_sz(0), c_sz(0)
        check(self._f("param_offset")(self.ctx, key.encode(), C.byref(off), C.byref(n)), f"param_offset({key})")
        return off.value, n.value

    def train_workspace_bytes(self, B, h, w):
        return self._f("train_workspace_bytes")(self.ctx, B, h, w)

    def forward_train(self, x):
        B, h, w = self._geometry(x)
        x = x.contiguous()
        ws = self._workspace(B, h, w, x.device, train=True)
        out = self._output(x)
        check(self._f("forward_train")(self.ctx, dev_ptr(x), dev_ptr(out), B, h, w, dev_ptr(ws), ws.numel(), stream_ptr()),
              f"{self.name}_forward_train")
        self.train_generation += 1
        return out

    def backward(self, x, dout, grads=None):
        """dLoss/dOut -> flat fp32 gradient bucket (state_dict order).  Must follow forward_train(x) of the same x."""
        B, h, w = self._geometry(x)
        n = self.num_params()
        if grads is None:
            grads = torch.empty(n, dtype=torch.float32, device=x.device)
        ws = self._workspace(B, h, w, x.device, train=True)
        dout = dout.contiguous()
        if dout.dtype != torch.float32:
            dout = dout.float()
        check(self._f("backward")(self.ctx, dev_ptr(x.contiguous()), dev_ptr(dout), B, h, w, dev_ptr(ws), ws.numel(),
                                  dev_ptr(grads), n, stream_ptr()), f"{self.name}_backward")
        return grads

    def train_saved(self, x, which, index):
        """the activation forward_train(x) saved for the backward, as a flat fp32 view of the training workspace (lfsr_<name>_train_saved)"""
        B, h, w = self._geometry(x)
        off, n = c_sz(0), c_sz(0)
        check(self._f("train_saved")(self.ctx, B, h, w, which, index, C.byref(off), C.byref(n)), "train_saved")
        ws = self._workspace(B, h, w, x.device, train=True).view(torch.float32)
        return ws[off.value:off.value + n.value]


class LFSSRRuntime(ModelRuntime):
    """lfsr_lfssr: inference only (the C ABI has no training symbols for it).  Its widest tensor is the 256-wide result of the last up-sampling conv: 256 floats
    per LR pixel at scale 2, and 4 x 256 = 16 x 64 at scale 4, where fup2 runs on the (2h, 2w) views and writes 64 channels at (4h, 4w)."""

    def __init__(self, A, scale, n_layer=10):
        super().__init__("lfssr", A, scale, n_layer)
        self.widest_row_floats = 1024 if scale == 4 else 256


class DistgSSRRuntime(ModelRuntime):
    """lfsr_distgssr: the batched weight load, the tapped forward and the per-class profile on top of the shared life cycle."""

    widest_row_floats, offset_limit = 160, 1 << 30    # the 144-channel concat buffer (counted as 160); 1 GiB: see max_patches_per_launch
    PROFILE_CLASSES = ("conv3x3", "angconv", "epiconv", "pointwise", "init_conv", "upsample_head")

    def __init__(self, A, scale, n_group=4, n_block=4, channels=64):
        super().__init__("distgssr", A, scale, n_group, n_block, channels)

    def load_state(self, named_tensors, device, batched=False):
        """batched: the packs are recorded into a device-side descriptor table (re-uploaded only when an address changed) and run at
        finalize as one launch per pack kind instead of ~280 small launches (lfsr_distgssr_begin_batched_load)."""
        if batched:
            check(self.lib.lfsr_distgssr_begin_batched_load(self.ctx), "distgssr_begin_batched_load")
        super().load_state(named_tensors, device)

    def forward(self, x, taps=None):
        """x (B,1,A*h,A*w) fp32 CUDA -> (B,1,A*h*s,A*w*s).  taps: optional list of 5 bools -> (out, the 5 tapped activations or None)."""
        if taps is None:
            return super().forward(x)
        B, h, w = self._geometry(x)
        x = x.contiguous()
        out = self._output(x)
        ws = self._workspace(B, h, w, x.device)
        bufs = []
        arr = (c_p * 5)()
        for i in range(5):
            if taps[i]:
                t = torch.empty((B, 144 if i == 4 else 64, x.shape[2], x.shape[3]), dtype=torch.float32, device=x.device)
                arr[i] = t.data_ptr()
            else:
                t = None
                arr[i] = None
            bufs.append(t)
        check(self.lib.lfsr_distgssr_forward_taps(self.ctx, dev_ptr(x), dev_ptr(out), B, h, w, dev_ptr(ws), ws.numel(), arr, stream_ptr()),
              "distgssr_forward_taps")
        return out, bufs

    def profile(self, enable):
        check(self.lib.lfsr_distgssr_profile(self.ctx, int(enable)), "distgssr_profile")

    def profile_read(self):
        """-> {class: (total_ms, launches)} from hipEvents recorded on the launch stream; resets."""
        ms = (C.c_double * 6)()
        n = (C.c_longlong * 6)()
        check(self.lib.lfsr_distgssr_profile_read(self.ctx, ms, n), "distgssr_profile_read")
        return {k: (ms[i], n[i]) for i, k in enumerate(self.PROFILE_CLASSES)}

# ---------------------------------------------------------------------------------------------------
# d1-d9 operator-level wrappers on VCL tensors (2-D torch tensors: (pixels, stride))
# ---------------------------------------------------------------------------------------------------

def _opt(t):
    return dev_ptr(t) if t is not None else None


def conv3x3(x, w_packed, n_img, h, w, slope=1.0, res1=None, res2=None, out=None, out_choff=0, x_choff=0):
    lib = load()
    if out is None:
        out = torch.empty((n_img * h * w, 64), dtype=torch.float32, device=x.device)
    check(lib.lfsr_conv3x3_fwd(dev_ptr(x), x.shape[1], x_choff, dev_ptr(w_packed), dev_ptr(out), out.shape[1], out_choff,
                               _opt(res1), res1.shape[1] if res1 is not None else 0, 0,
                               _opt(res2), res2.shape[1] if res2 is not None else 0, 0,
                               n_img, h, w, slope, stream_ptr()), "conv3x3_fwd")
    return out


def conv3x3_wide(x, cin, w_packed, n_img, h, w, slope=0.0, res1=None, res1_choff=0, out=None, out_choff=0, x_choff=0):
    """lfsr_conv3x3_wide_fwd: lrelu(per-view 3x3 conv, cin in {128, 320} -> 64, slope) (+ res1's 64 channels from res1_choff on; res1 may be x itself) on VCL
    rows; w_packed: pack_conv_weight of the (64, cin, 3, 3) weight.  Follows set_wide_arithmetic."""
    lib = load()
    if out is None:
        out = torch.empty((n_img * h * w, 64), dtype=torch.float32, device=x.device)
    check(lib.lfsr_conv3x3_wide_fwd(dev_ptr(x), x.shape[1], x_choff, cin, dev_ptr(w_packed), dev_ptr(out), out.shape[1], out_choff,
                                    _opt(res1), res1.shape[1] if res1 is not None else 0, res1_choff if res1 is not None else 0,
                                    n_img, h, w, slope, stream_ptr()), "conv3x3_wide_fwd")
    return out


def pointwise(x, cin, w_packed, N, slope=1.0, bias=None, out=None, out_choff=0, x_choff=0):
    lib = load()
    M = x.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    check(lib.lfsr_pointwise_fwd(dev_ptr(x), x.shape[1], x_choff, cin, dev_ptr(w_packed), _opt(bias), dev_ptr(out), out.shape[1], out_choff,
                                 M, N, slope, stream_ptr()), "pointwise_fwd")
    return out


def angconv(x, w1p, w2p, B, A, h, w, slope, out, out_choff, tmp=None):
    """tmp: optional (B*h*w, 16) tensor that receives the stage-1 activation lrelu(AngConv.0(x)) (what lfsr_angconv_bwd reads)"""
    lib = load()
    if tmp is None:
        tmp = torch.empty((B * h * w, 16), dtype=torch.float32, device=x.device)
    check(lib.lfsr_angconv_fwd(dev_ptr(x), x.shape[1], 0, dev_ptr(w1p), dev_ptr(w2p), dev_ptr(tmp), dev_ptr(out), out.shape[1], out_choff,
                               B, A, h, w, slope, stream_ptr()), "angconv_fwd")
    return out


def epiconv(x, w1p, w2p, B, A, h, w, vertical, slope, out, out_choff, tmp=None):
    """tmp: optional (B*A*h*w, 32) tensor that receives the stage-1 activation lrelu(EPIConv.0(.)) of this pass (what lfsr_epiconv_hv_bwd reads)"""
    lib = load()
    if tmp is None:
        tmp = torch.empty((B * A * h * w, 32), dtype=torch.float32, device=x.device)
    check(lib.lfsr_epiconv_fwd(dev_ptr(x), x.shape[1], 0, dev_ptr(w1p), dev_ptr(w2p), dev_ptr(tmp), dev_ptr(out), out.shape[1], out_choff,
                               B, A, h, w, int(vertical), slope, stream_ptr()), "epiconv_fwd")
    return out


def epiconv_hv(x, w1p, w2p, B, A, h, w, slope, out, choff_h, choff_v):
    lib = load()
    tmp = torch.empty((B * A * h * w, 32), dtype=torch.float32, device=x.device)
    check(lib.lfsr_epiconv_hv_fwd(dev_ptr(x), x.shape[1], 0, dev_ptr(w1p), dev_ptr(w2p), dev_ptr(tmp), dev_ptr(out), out.shape[1], choff_h, choff_v,
                                  B, A, h, w, slope, stream_ptr()), "epiconv_hv_fwd")
    return out


def distg_branch_tail(x, spa, w_ang0, w_ang2, w_epi0, w_epi2, w_fuse0, B, A, h, w, slope, out=None):
    """DisentgBlock tail (lfsr_distg_branch_tail_fwd): lrelu(fuse.0(spa | ang | epiH | epiV)) of the block input x and the SpaConv.2 output spa, both VCL 64-ch.
    Weights packed as angconv / epiconv_hv / pointwise take them.  Returns (y (B*A*A*h*w, 64), t_a, t_h, t_v); out = those four, preallocated (contiguous)."""
    lib = load()
    shapes = ((x.shape[0], 64), (B * h * w, 16), (B * A * h * w, 32), (B * A * h * w, 32))
    if out is None:
        out = tuple(torch.empty(s, dtype=torch.float32, device=x.device) for s in shapes)
    if len(out) != 4 or any(tuple(o.shape) != s or o.dtype != torch.float32 for o, s in zip(out, shapes)):
        raise LfsrError("distg_branch_tail: out must be four float32 tensors of shapes %r" % (shapes,))
    y, t_a, t_h, t_v = out
    check(lib.lfsr_distg_branch_tail_fwd(dev_ptr(x), x.shape[1], 0, dev_ptr(spa), spa.shape[1], 0, dev_ptr(w_ang0), dev_ptr(w_ang2), dev_ptr(w_epi0),
                                         dev_ptr(w_epi2), dev_ptr(w_fuse0), dev_ptr(t_a), dev_ptr(t_h), dev_ptr(t_v), dev_ptr(y), 64, 0, B, A, h, w, slope,
                                         stream_ptr()), "distg_branch_tail_fwd")
    return y, t_a, t_h, t_v


def initconv(x, w, A):
    lib = load()
    B, _, Hh, Ww = x.shape
    h, wd = Hh // A, Ww // A
    out = torch.empty((B * A * A * h * wd, 64), dtype=torch.float32, device=x.device)
    check(lib.lfsr_initconv_fwd(dev_ptr(x), dev_ptr(w), dev_ptr(out), 64, 0, B, A, h, wd, stream_ptr()), "initconv_fwd")
    return out


def upsample_head(f, w0, b0, w2, x_lr, A, s):
    lib = load()
    B, _, Hh, Ww = x_lr.shape
    h, w = Hh // A, Ww // A
    wf = torch.empty(s * s * 64, dtype=torch.float32, device=f.device)
    bf = torch.empty(s * s, dtype=torch.float32, device=f.device)
    check(lib.lfsr_fold_head(dev_ptr(w0), _opt(b0), dev_ptr(w2), dev_ptr(wf), dev_ptr(bf), 64, s, stream_ptr()), "fold_head")
    out = torch.empty((B, 1, Hh * s, Ww * s), dtype=torch.float32, device=f.device)
    check(lib.lfsr_upsample_head_fwd(dev_ptr(f), f.shape[1], 0, dev_ptr(wf), dev_ptr(bf), dev_ptr(x_lr), dev_ptr(out), B, A, h, w, s, stream_ptr()),
          "upsample_head_fwd")
    return out


# ---------------------------------------------------------------------------------------------------
# LFSSR's operators (inference only)
# ---------------------------------------------------------------------------------------------------

def angconv3x3(x, w_packed, bias, B, A, npix, in_bias=None, out=None, x_choff=0, out_choff=0):
    """lfsr_angconv3x3_fwd: relu(3x3 conv over the A x A grid of views + bias) at every pixel of VCL rows; in_bias: the bias of a conv + ReLU in front, applied as
    the operand is staged.  w_packed: pack_conv_weight of the (64,64,3,3) weight."""
    lib = load()
    if out is None:
        out = torch.empty((B * A * A * npix, 64), dtype=torch.float32, device=x.device)
    check(lib.lfsr_angconv3x3_fwd(dev_ptr(x), x.shape[1], x_choff, dev_ptr(w_packed), dev_ptr(bias), _opt(in_bias), dev_ptr(out), out.shape[1], out_choff,
                                  B, A, npix, stream_ptr()), "angconv3x3_fwd")
    return out


def lfssr_conv0(x, w, bias, A, out=None, out_choff=0):
    """lfsr_lfssr_conv0_fwd: SAI mosaic (B,1,A*h,A*w) -> VCL 64 channels, relu(per-view 3x3 conv + bias); w (64,1,3,3), bias (64) raw"""
    lib = load()
    B, _, Hh, Ww = x.shape
    h, wd = Hh // A, Ww // A
    if out is None:
        out = torch.empty((B * A * A * h * wd, 64), dtype=torch.float32, device=x.device)
    check(lib.lfsr_lfssr_conv0_fwd(dev_ptr(x), dev_ptr(w), dev_ptr(bias), dev_ptr(out), out.shape[1], out_choff, B, A, h, wd, stream_ptr()), "lfssr_conv0_fwd")
    return out


def pack_ps2_weight(w):
    """(256,64,3,3) -> the four consecutive 64 -> 64 packs lfsr_conv3x3_ps2_fwd reads: pack 2i + j from rows 4c + 2i + j"""
    return torch.cat([pack_conv_weight(w[ij::4].contiguous()) for ij in range(4)])


def conv3x3_ps2(x, w_packed4, bias, n_img, h, w, out=None, out_choff=0, x_choff=0):
    """lfsr_conv3x3_ps2_fwd: per-view 3x3 conv 64 -> 256 + bias, PixelShuffle(2), ReLU -> VCL rows of the (2h, 2w) views"""
    lib = load()
    if out is None:
        out = torch.empty((n_img * h * w * 4, 64), dtype=torch.float32, device=x.device)
    tmp = torch.empty((n_img * h * w, 256), dtype=torch.float32, device=x.device)
    check(lib.lfsr_conv3x3_ps2_fwd(dev_ptr(x), x.shape[1], x_choff, dev_ptr(w_packed4), dev_ptr(bias), dev_ptr(tmp), dev_ptr(out), out.shape[1], out_choff,
                                   n_img, h, w, stream_ptr()), "conv3x3_ps2_fwd")
    return out


def lfssr_tail(f, w_res, b_res, lo, w_iup, b_iup, B, A, h, w, mosaic, f_choff=0):
    """lfsr_lfssr_tail_fwd: conv3x3_{64->1}(f) + b_res + PixelShuffle2(conv3x3_{1->4}(lo) + b_iup); f VCL rows of the (2h, 2w) views, lo (B*A*A, h, w) planes
    -> (B*A*A, 2h, 2w) planes, or with mosaic the SAI mosaic (B,1,A*2h,A*2w)"""
    lib = load()
    out = torch.empty((B, 1, A * 2 * h, A * 2 * w) if mosaic else (B * A * A, 2 * h, 2 * w), dtype=torch.float32, device=f.device)
    check(lib.lfsr_lfssr_tail_fwd(dev_ptr(f), f.shape[1], f_choff, dev_ptr(w_res), dev_ptr(b_res), dev_ptr(lo), dev_ptr(w_iup), dev_ptr(b_iup), dev_ptr(out),
                                  B, A, h, w, int(bool(mosaic)), stream_ptr()), "lfssr_tail_fwd")
    return out


# ---------------------------------------------------------------------------------------------------
# operator-level backward wrappers (d11) and the RCCL exchange step at the C ABI
# ---------------------------------------------------------------------------------------------------

def pack_conv_weight_T(w):
    """(O,C,kh,kw) -> the transposed pack the data gradients read (3x3: taps flipped)."""
    lib = load()
    O, Cc = w.shape[:2]
    taps = w.numel() // (O * Cc)
    out = torch.empty(lib.lfsr_packed_weight_tr_floats(O, Cc, taps), dtype=torch.float32, device=w.device)
    check(lib.lfsr_pack_conv_weight_tr(dev_ptr(w), dev_ptr(out), O, Cc, taps, stream_ptr()), "pack_conv_weight_T")
    return out


def conv3x3_dgrad(dy, wT_packed, n_img, h, w, res1=None, act=None, act_slope=1.0):
    lib = load()
    dx = torch.empty((n_img * h * w, 64), dtype=torch.float32, device=dy.device)
    check(lib.lfsr_conv3x3_dgrad(dev_ptr(dy), dy.shape[1], 0, dev_ptr(wT_packed), dev_ptr(dx), 64, 0,
                                 _opt(res1), res1.shape[1] if res1 is not None else 0, 0,
                                 _opt(act), act.shape[1] if act is not None else 0, 0, act_slope, n_img, h, w, stream_ptr()), "conv3x3_dgrad")
    return dx


def conv3x3_wgrad(dy, x, n_img, h, w, dw=None):
    lib = load()
    acc = dw is not None
    if dw is None:
        dw = torch.empty((64, 64, 3, 3), dtype=torch.float32, device=dy.device)
    ws = torch.empty(lib.lfsr_conv3x3_wgrad_workspace_floats(n_img, h, w), dtype=torch.float32, device=dy.device)
    check(lib.lfsr_conv3x3_wgrad(dev_ptr(dy), dy.shape[1], 0, dev_ptr(x), x.shape[1], 0, dev_ptr(dw), dev_ptr(ws), ws.numel(), n_img, h, w, int(acc),
                                 stream_ptr()), "conv3x3_wgrad")
    return dw


def pointwise_dgrad(dy, wT_packed, cin, act=None, act_slope=1.0):
    lib = load()
    M = dy.shape[0]
    dx = torch.empty((M, cin), dtype=torch.float32, device=dy.device)
    check(lib.lfsr_pointwise_dgrad(dev_ptr(dy), dy.shape[1], 0, 64, dev_ptr(wT_packed), dev_ptr(dx), cin, 0, cin,
                                   _opt(act), act.shape[1] if act is not None else 0, 0, act_slope, M, stream_ptr()), "pointwise_dgrad")
    return dx


def pointwise_wgrad(dy, x, cout, cin):
    lib = load()
    M = dy.shape[0]
    dw = torch.empty((cout, cin), dtype=torch.float32, device=dy.device)
    ws = torch.empty(lib.lfsr_pointwise_wgrad_workspace_floats(M, cout, cin), dtype=torch.float32, device=dy.device)
    check(lib.lfsr_pointwise_wgrad(dev_ptr(dy), dy.shape[1], 0, cout, dev_ptr(x), x.shape[1], 0, cin, dev_ptr(dw), dev_ptr(ws), ws.numel(), M, 0,
                                   stream_ptr()), "pointwise_wgrad")
    return dw


def linear_wgrad(dy, x, cout, cin, dw=None):
    """lfsr_linear_wgrad: dw (cout, cin) = dy^T x over the rows of dy (M, >= cout) and x (M, >= cin); dw given: accumulated into.  Follows set_lin_grad_arithmetic."""
    lib = load()
    M = dy.shape[0]
    acc = dw is not None
    if dw is None:
        dw = torch.empty((cout, cin), dtype=torch.float32, device=dy.device)
    ws = torch.empty(lib.lfsr_linear_wgrad_workspace_floats(M, cout, cin), dtype=torch.float32, device=dy.device)
    check(lib.lfsr_linear_wgrad(dev_ptr(dy), dy.shape[1], dev_ptr(x), x.shape[1], dev_ptr(dw), dev_ptr(ws), ws.numel(), M, cout, cin, int(acc), stream_ptr()),
          "linear_wgrad")
    return dw


def conv3x3_wide_wgrad(dy, x, cin, n_img, h, w, dw=None, dy_choff=0, x_choff=0):
    """lfsr_conv3x3_wide_wgrad: dw (64, cin, 3, 3) = the weight gradient of the per-view 3x3 conv cin in {128, 320} -> 64 from VCL rows dy (n_img h w, >= dy_choff + 64)
    and x (n_img h w, >= x_choff + cin); dw given: accumulated into.  Follows set_wide_train_arithmetic."""
    lib = load()
    acc = dw is not None
    if dw is None:
        dw = torch.empty((64, cin, 3, 3), dtype=torch.float32, device=dy.device)
    ws = torch.empty(lib.lfsr_conv3x3_wide_wgrad_workspace_floats(cin, n_img, h, w), dtype=torch.float32, device=dy.device)
    check(lib.lfsr_conv3x3_wide_wgrad(dev_ptr(dy), dy.shape[1], dy_choff, dev_ptr(x), x.shape[1], x_choff, cin, dev_ptr(dw), dev_ptr(ws), ws.numel(),
                                      n_img, h, w, int(acc), stream_ptr()), "conv3x3_wide_wgrad")
    return dw


def linear_dgrad(dy, wT_packed, cin, r1=None, act=None, dx=None):
    """lfsr_linear_dgrad: dx (M, cin) = (dy W) * (act > 0) + r1 from dense rows dy (M, cout) and wT_packed = pack_conv_weight_T of the (cout, cin, 1, 1) weight;
    r1 / act: optional (M, >= cin) rows; dx given: columns [0, cin) of its rows are written (r1 may be dx).  Follows set_lin_grad_arithmetic."""
    lib = load()
    M, cout = dy.shape
    if dx is None:
        dx = torch.empty((M, cin), dtype=torch.float32, device=dy.device)
    check(lib.lfsr_linear_dgrad(dev_ptr(dy), cout, dev_ptr(wT_packed), dev_ptr(dx), dx.shape[1], _opt(r1), r1.shape[1] if r1 is not None else 0,
                                _opt(act), act.shape[1] if act is not None else 0, M, cin, stream_ptr()), "linear_dgrad")
    return dx


class RcclComm:
    """ncclComm_t created through the C ABI (lfsr_comm_*).  The 128-byte unique id comes from rank 0 and is shipped by the caller
    (``exchange``: a callable rank-0-bytes -> bytes-on-every-rank, e.g. a torch.distributed broadcast over gloo, or a Store)."""

    def __init__(self, world, rank, exchange=None):
        self.lib = load()
        if not self.lib.lfsr_comm_available():
            raise LfsrError("RCCL not found (librccl.so): lfsr_allreduce is unavailable on this host")
        buf = C.create_string_buffer(128)
        if rank == 0:
            check(self.lib.lfsr_comm_unique_id(buf), "comm_unique_id")
        raw = bytes(buf.raw)
        if world > 1:
            if exchange is None:
                raise LfsrError("world > 1 needs an `exchange` callable to ship rank 0's unique id")
            raw = exchange(raw)
        comm = c_p()
        check(self.lib.lfsr_comm_init(C.byref(comm), world, rank, C.create_string_buffer(raw, 128)), "comm_init")
        self.comm, self.world = comm, world

    def allreduce_(self, t):
        """in-place SUM over the communicator on the current stream; t: contiguous fp32 CUDA tensor"""
        if t.dtype != torch.float32:
            raise LfsrError("lfsr_allreduce carries fp32 buckets")
        check(self.lib.lfsr_allreduce(dev_ptr(t), t.numel(), self.comm, stream_ptr()), "allreduce")
        return t

    def close(self):
        if getattr(self, "comm", None):
            self.lib.lfsr_comm_destroy(self.comm)
            self.comm = None


def angconv_bwd(dy, dy_choff, y, y_choff, x, a16, w0, w2, dx, B, A, h, w, slope=0.1):
    """lfsr_angconv_bwd: dy / y / x / dx VCL tensors (pixels, stride); y = the forward output (None: dy is already the gradient at the stage-2 pre-activation);
    w0, w2 raw PyTorch layouts.  dx is accumulated into; -> (dw0, dw2)."""
    lib = load()
    ws = torch.empty(lib.lfsr_angconv_bwd_workspace_floats(B, A, h, w), dtype=torch.float32, device=x.device)
    dw0, dw2 = torch.empty_like(w0), torch.empty_like(w2)
    check(lib.lfsr_angconv_bwd(dev_ptr(dy), dy.shape[1], dy_choff, _opt(y), y.shape[1] if y is not None else 0, y_choff, dev_ptr(x), dev_ptr(a16),
                               dev_ptr(w0.contiguous()), dev_ptr(w2.contiguous()), dev_ptr(dx), dev_ptr(dw0), dev_ptr(dw2), dev_ptr(ws), ws.numel(), B, A, h, w, slope,
                               stream_ptr()), "angconv_bwd")
    return dw0, dw2


def epiconv_hv_bwd(dy, choff_h, choff_v, y, y_choff_h, y_choff_v, x, e_h, e_v, w0, w2, dx, B, A, h, w, slope=0.1):
    """lfsr_epiconv_hv_bwd (both passes, shared weights).  dx is accumulated into; -> (dw0, dw2)."""
    lib = load()
    ws = torch.empty(lib.lfsr_epiconv_hv_bwd_workspace_floats(B, A, h, w), dtype=torch.float32, device=x.device)
    dw0, dw2 = torch.empty_like(w0), torch.empty_like(w2)
    check(lib.lfsr_epiconv_hv_bwd(dev_ptr(dy), dy.shape[1], choff_h, choff_v, _opt(y), y.shape[1] if y is not None else 0, y_choff_h, y_choff_v, dev_ptr(x),
                                  dev_ptr(e_h), dev_ptr(e_v), dev_ptr(w0.contiguous()), dev_ptr(w2.contiguous()), dev_ptr(dx), dev_ptr(dw0), dev_ptr(dw2),
                                  dev_ptr(ws), ws.numel(), B, A, h, w, slope, stream_ptr()), "epiconv_hv_bwd")
    return dw0, dw2
