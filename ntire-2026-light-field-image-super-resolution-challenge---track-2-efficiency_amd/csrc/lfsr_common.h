// Shared host-side helpers for liblfsr_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "../../include/lfsr_hip.h"

#define LFSR_HIP_ERR(e) (-(1000 + (int)(e)))
#define LFSR_CHECK_LAUNCH()                                   \
  do {                                                        \
    hipError_t e__ = hipGetLastError();                       \
    if (e__ != hipSuccess) return LFSR_HIP_ERR(e__);          \
  } while (0)
// early return of a failed step: LFSR_RC(lfsr_...(...)) returns its nonzero status from the enclosing function
#define LFSR_RC(call)                                         \
  do {                                                        \
    const int rc__ = (call);                                  \
    if (rc__) return rc__;                                    \
  } while (0)

static inline hipStream_t lfsr_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
// A/B ("lab") selectors: LFSR_* environment variables that pick an alternative kernel form of an operator for measurements and parity tests.  They are consulted
// ONLY when the process runs with LFSR_LAB set (read once, at the first selector lookup): the product default is one tested path per operator and no getenv on the
// launch path.  The one selection a product caller may make -- the arithmetic of the GEMMs that have an exact-three-term-bf16 form -- is an API: lfsr_set_arithmetic.
const char* lfsr_sel(const char* name);
bool lfsr_arith_f32();     // lfsr_set_arithmetic(LFSR_ARITH_F32): every GEMM on fp32 MFMA
bool lfsr_arith_bf16();    // lfsr_set_arithmetic(LFSR_ARITH_BF16): the 64 -> 64 3x3 forward conv on bf16 operands (conv3x3_bf16.hip); everything else as the default
bool lfsr_grad_arith_bf16();   // lfsr_set_grad_arithmetic(LFSR_GRAD_ARITH_BF16): that conv's data gradient (conv3x3_bf16_dgrad.hip) and weight gradient (wgrad_bf16.hip) on bf16 operands
bool lfsr_gemm_arith_bf16();   // lfsr_set_gemm_arithmetic(LFSR_GEMM_ARITH_BF16): the K = 64 / 128 linears, LayerNorm + q | k | v projections and feed-forward blocks on bf16 operands (gemm_bf16.hip)
bool lfsr_branch_arith_bf16();   // lfsr_set_branch_arithmetic(LFSR_BRANCH_ARITH_BF16): DistgSSR's EPIConv.0, EPIConv.2 and fuse.0 of the fused block tail on bf16 operands (distg_bf16.hip)
bool lfsr_ang_arith_bf16();   // lfsr_set_ang_arithmetic(LFSR_ANG_ARITH_BF16): LFSSR's angular 3x3 conv, lfsr_angconv3x3_fwd, on bf16 operands (ang3x3_bf16.hip)
bool lfsr_wide_arith_bf16();   // lfsr_set_wide_arithmetic(LFSR_WIDE_ARITH_BF16): LF_InterNet's 128 | 320 -> 64 per-view 3x3 convs, lfsr_conv3x3_wide_fwd, on bf16 operands (conv3x3_wide_bf16.hip)
bool lfsr_lin_grad_arith_bf16();   // lfsr_set_lin_grad_arithmetic(LFSR_LIN_GRAD_ARITH_BF16): the linears' weight and data gradients, lfsr_linear_wgrad / lfsr_linear_dgrad, on bf16 operands (lin_wgrad_bf16.hip, lin_dgrad_bf16.hip)
bool lfsr_branch_grad_arith_bf16();   // lfsr_set_branch_grad_arithmetic(LFSR_BRANCH_GRAD_ARITH_BF16): EPIConv.0's weight and data gradients (the EPI-line forms) on bf16 operands (epi0_grad_bf16.hip)
int lfsr_wide_train_arith();   // lfsr_get_wide_train_arithmetic(): LF_InterNet's wide convs in training -- 1: their weight gradients on bf16 operands (wgrad_wide_bf16.hip); 2: forward_train's wide convs as well
static inline unsigned lfsr_blocks(long long n, int per) {
  long long b = (n + per - 1) / per;
  return (unsigned)(b < 1 ? 1 : b);
}
static inline unsigned lfsr_cap_grid(long long total, unsigned cap = 8192) {   // blocks of 256 for a grid-stride loop over `total`
  unsigned g = lfsr_blocks(total, 256);
  return g > cap ? cap : g;
}

// Host-side layout of a workspace: buffers one after another in 64-float (256-B) granules.  A null base is the sizing pass (every pointer
// null, `floats` exact); offsets() lays out on a stand-in base that is never dereferenced, so that offset(p) tells where a buffer lies.
struct LfsrArena {
  float* base;
  size_t floats = 0;
  explicit LfsrArena(void* b = nullptr) : base(static_cast<float*>(b)) {}
  static LfsrArena offsets() { return LfsrArena(reinterpret_cast<void*>(uintptr_t(256))); }
  static size_t granules(size_t f) { return (f + 63) / 64 * 64; }
  float* take(size_t f) {
    float* p = base ? base + floats : nullptr;
    floats += granules(f);
    return p;
  }
  size_t bytes() const { return floats * sizeof(float); }
  size_t offset(const float* p) const { return (size_t)(p - base); }
};

// Non-temporal hint on result stores.  Measured on one MI355X (two runs each per call): on the 3x3 conv's output stores alone (buffer_store ... nt,
// W4_STPOL in conv3x3_wino4.hip) the DistgSSR forward goes 1678.7 -> 1718 patches/s (profiles/r02_logs/ab_bench_lines.json: bench13_*.json); on the EPI / angular / row-GEMM
// kernels' stores as well (global_store ... nt through lfsr_store_stream) it FALLS to 1444 (EPIT 668 -> 539, LFT 1331 -> 982 patches/s,
// profiles/r02_logs/ab_bench_lines.json: bench14_*.json): those results are re-read by the next kernel while still in the last-level cache.  So only the conv kernel uses the
// hint; lfsr_store_stream stays for A/B builds.  LFSR_NT_STORES=0 at compile time restores plain stores everywhere.
#ifndef LFSR_NT_STORES
#define LFSR_NT_STORES 1
#endif
#if defined(__HIPCC__)
typedef float lfsr_v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void lfsr_store_stream(float4* p, const float4 v) {
#if LFSR_NT_STORES
  lfsr_v4f t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<lfsr_v4f*>(p));
#else
  *p = v;
#endif
}
#endif


