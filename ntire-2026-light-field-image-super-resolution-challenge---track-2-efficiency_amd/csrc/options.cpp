// Library-wide options of liblfsr_hip.so.
//  * lfsr_set_arithmetic: which arithmetic the GEMMs that have two forms run in, or bf16 operands for the 64 -> 64 3x3 forward conv (the product-level choice);
//  * lfsr_set_grad_arithmetic: bf16 operands for the 64 -> 64 3x3 conv's data and weight gradients, independent of the first;
//  * lfsr_set_gemm_arithmetic: bf16 operands for the transformer linears, LayerNorm + q | k | v projections and feed-forward blocks (gemm_bf16.hip), independent of both;
//  * lfsr_set_branch_arithmetic: bf16 operands for DistgSSR's EPI branch and block tail (distg_bf16.hip), independent of the three;
//  * lfsr_set_ang_arithmetic: bf16 operands for LFSSR's angular 3x3 conv (ang3x3_bf16.hip), independent of the four;
//  * lfsr_set_wide_arithmetic: bf16 operands for LF_InterNet's wide per-view 3x3 convs, lfsr_conv3x3_wide_fwd (conv3x3_wide_bf16.hip), independent of the five;
//  * lfsr_set_lin_grad_arithmetic: bf16 operands for the weight and data gradients of the transformers' linears, lfsr_linear_wgrad / lfsr_linear_dgrad (lin_wgrad_bf16.hip,
//    lin_dgrad_bf16.hip), independent of the six;
//  * lfsr_set_wide_train_arithmetic: bf16 operands for LF_InterNet's wide per-view 3x3 convs in training -- their weight gradients, lfsr_conv3x3_wide_wgrad
//    (wgrad_wide_bf16.hip), and optionally forward_train's wide convs (conv3x3_wide_bf16.hip), independent of the seven;
//  * lfsr_set_branch_grad_arithmetic: bf16 operands for the EPI-line weight and data gradients of DistgSSR's EPIConv.0 (epi0_grad_bf16.hip) behind lfsr_epiconv_hv_bwd and
//    lfsr_distgssr_backward, independent of the eight;
//  * lfsr_sel: the A/B selectors of the measurement / parity tooling (LFSR_* environment variables), live only in a process started with LFSR_LAB set.
#include <stdlib.h>

#include "lfsr_internal.h"

namespace {
std::atomic<int> g_arith{LFSR_ARITH_DEFAULT};
std::atomic<int> g_grad_arith{LFSR_GRAD_ARITH_DEFAULT};
std::atomic<int> g_gemm_arith{LFSR_GEMM_ARITH_DEFAULT};
std::atomic<int> g_branch_arith{LFSR_BRANCH_ARITH_DEFAULT};
std::atomic<int> g_ang_arith{LFSR_ANG_ARITH_DEFAULT};
std::atomic<int> g_wide_arith{LFSR_WIDE_ARITH_DEFAULT};
std::atomic<int> g_lin_grad_arith{LFSR_LIN_GRAD_ARITH_DEFAULT};
std::atomic<int> g_wide_train_arith{LFSR_WIDE_TRAIN_ARITH_DEFAULT};
std::atomic<int> g_branch_grad_arith{LFSR_BRANCH_GRAD_ARITH_DEFAULT};
std::atomic<int> g_lab{-1};
}  // namespace

const char* lfsr_sel(const char* name) {
  int lab = g_lab.load(std::memory_order_relaxed);
  if (lab < 0) {
    lab = getenv("LFSR_LAB") != nullptr ? 1 : 0;
    g_lab.store(lab, std::memory_order_relaxed);
  }
  return lab ? getenv(name) : nullptr;
}

bool lfsr_arith_f32() { return g_arith.load(std::memory_order_relaxed) == LFSR_ARITH_F32; }
bool lfsr_arith_bf16() { return g_arith.load(std::memory_order_relaxed) == LFSR_ARITH_BF16; }
bool lfsr_grad_arith_bf16() { return g_grad_arith.load(std::memory_order_relaxed) == LFSR_GRAD_ARITH_BF16; }
bool lfsr_gemm_arith_bf16() { return g_gemm_arith.load(std::memory_order_relaxed) == LFSR_GEMM_ARITH_BF16; }
bool lfsr_branch_arith_bf16() { return g_branch_arith.load(std::memory_order_relaxed) == LFSR_BRANCH_ARITH_BF16; }
bool lfsr_ang_arith_bf16() { return g_ang_arith.load(std::memory_order_relaxed) == LFSR_ANG_ARITH_BF16; }
bool lfsr_wide_arith_bf16() { return g_wide_arith.load(std::memory_order_relaxed) == LFSR_WIDE_ARITH_BF16; }
bool lfsr_lin_grad_arith_bf16() { return g_lin_grad_arith.load(std::memory_order_relaxed) == LFSR_LIN_GRAD_ARITH_BF16; }
bool lfsr_branch_grad_arith_bf16() { return g_branch_grad_arith.load(std::memory_order_relaxed) == LFSR_BRANCH_GRAD_ARITH_BF16; }
int lfsr_wide_train_arith() { return g_wide_train_arith.load(std::memory_order_relaxed); }

extern "C" {

int lfsr_set_arithmetic(int mode) {
  if (mode != LFSR_ARITH_DEFAULT && mode != LFSR_ARITH_F32 && mode != LFSR_ARITH_BF16) return LFSR_E_ARG;
  g_arith.store(mode);
  return LFSR_OK;
}

int lfsr_get_arithmetic(void) { return g_arith.load(); }

int lfsr_set_grad_arithmetic(int mode) {
  if (mode != LFSR_GRAD_ARITH_DEFAULT && mode != LFSR_GRAD_ARITH_BF16) return LFSR_E_ARG;
  g_grad_arith.store(mode);
  return LFSR_OK;
}

int lfsr_get_grad_arithmetic(void) { return g_grad_arith.load(); }

int lfsr_set_gemm_arithmetic(int mode) {
  if (mode != LFSR_GEMM_ARITH_DEFAULT && mode != LFSR_GEMM_ARITH_BF16) return LFSR_E_ARG;
  g_gemm_arith.store(mode);
  return LFSR_OK;
}

int lfsr_get_gemm_arithmetic(void) { return g_gemm_arith.load(); }

int lfsr_set_branch_arithmetic(int mode) {
  if (mode != LFSR_BRANCH_ARITH_DEFAULT && mode != LFSR_BRANCH_ARITH_BF16) return LFSR_E_ARG;
  g_branch_arith.store(mode);
  return LFSR_OK;
}

int lfsr_get_branch_arithmetic(void) { return g_branch_arith.load(); }

int lfsr_set_ang_arithmetic(int mode) {
  if (mode != LFSR_ANG_ARITH_DEFAULT && mode != LFSR_ANG_ARITH_BF16) return LFSR_E_ARG;
  g_ang_arith.store(mode);
  return LFSR_OK;
}

int lfsr_get_ang_arithmetic(void) { return g_ang_arith.load(); }

int lfsr_set_wide_arithmetic(int mode) {
  if (mode != LFSR_WIDE_ARITH_DEFAULT && mode != LFSR_WIDE_ARITH_BF16) return LFSR_E_ARG;
  g_wide_arith.store(mode);
  return LFSR_OK;
}

int lfsr_get_wide_arithmetic(void) { return g_wide_arith.load(); }

int lfsr_set_lin_grad_arithmetic(int mode) {
  if (mode != LFSR_LIN_GRAD_ARITH_DEFAULT && mode != LFSR_LIN_GRAD_ARITH_BF16) return LFSR_E_ARG;
  g_lin_grad_arith.store(mode);
  return LFSR_OK;
}

int lfsr_get_lin_grad_arithmetic(void) { return g_lin_grad_arith.load(); }

int lfsr_set_wide_train_arithmetic(int mode) {
  if (mode != LFSR_WIDE_TRAIN_ARITH_DEFAULT && mode != LFSR_WIDE_TRAIN_ARITH_BF16_WGRAD && mode != LFSR_WIDE_TRAIN_ARITH_BF16) return LFSR_E_ARG;
  g_wide_train_arith.store(mode);
  return LFSR_OK;
}

int lfsr_get_wide_train_arithmetic(void) { return g_wide_train_arith.load(); }

int lfsr_set_branch_grad_arithmetic(int mode) {
  if (mode != LFSR_BRANCH_GRAD_ARITH_DEFAULT && mode != LFSR_BRANCH_GRAD_ARITH_BF16) return LFSR_E_ARG;
  g_branch_grad_arith.store(mode);
  return LFSR_OK;
}

int lfsr_get_branch_grad_arithmetic(void) { return g_branch_grad_arith.load(); }

}  // extern "C"
