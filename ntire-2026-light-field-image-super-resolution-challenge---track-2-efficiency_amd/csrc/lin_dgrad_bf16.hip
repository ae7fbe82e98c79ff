// Data gradient of a linear with bf16 OPERANDS: the kernel of lfsr_set_lin_grad_arithmetic(LFSR_LIN_GRAD_ARITH_BF16) behind lfsr_linear_dgrad and LfsrTransBwd::dgemm.
//   dx[m][n] = (sum over k < cout of dy[m][k] W[k][n]) * (act[m][n] > 0 ? 1 : 0) + r1[m][n]        cout in {64, 128, 256, 576, 1024}, n < cin in {64, 128, 256}
// dy and the transposed weight are rounded to bf16 once (v_cvt_pk_bf16_f32: nearest even), the products are exact and run on v_mfma_f32_16x16x32_bf16; accumulation,
// the mask and the residual add are fp32, after the accumulation.  Gradients stay fp32 in memory: the mode changes arithmetic, not storage.
//
// The structure is k_gemm_bf16's (gemm_bf16.hip; that file's header: the LDS image and why its reads are conflict-free) with K = cout: the weight is read from the fp32
// transposed pack the drivers already build ([cin rows][cout], k contiguous) and converted while it is staged into LDS, once per block, so the row loop has no barrier;
// a wave owns 16 rows of dy at a time, loads them straight from global memory in B-operand order and ends up with channels 16 t + 4 g .. + 3 of its row: 16-B loads of
// act and r1, 16-B stores of dx.  What differs: K reaches 1024, so a wave's rows do not fit its registers -- it walks them in K chunks of at most 192, the next chunk
// (or the next rows' first one) in flight over this chunk's MFMAs, the accumulators living across the chunks; and where the whole image would not fit LDS
// ((576, 256), (1024, 128 | 256): no driver runs them) the blocks of blockIdx.y take panels of 128 or 64 of the cin columns and dy is read once per panel.  Rows are
// addressed with 64-bit pointers (M < 2^31 - 128 rows of any stride, as the default): a row past M is loaded as row M - 1 and never stored.
// r1 may be dx itself: each lane reads its r1 elements before it stores the same ones.  Only columns [0, cin) of dx are written.
// Determinism: no atomics, one wave and one summation chain (k ascending in K steps of 32) per output element: two runs give the same bits, and a row's result does
// not depend on M or on the grid.
#include <stdlib.h>

#include "lfsr_internal.h"

namespace {

typedef float f32x4d __attribute__((ext_vector_type(4)));
typedef unsigned u32x4d __attribute__((ext_vector_type(4)));

struct LinDgradArgs {
  const float* X;        // dy: M dense rows of K
  const float* Wp;       // [cin rows][K] fp32, k contiguous
  const float* R1; int r1_stride;
  const float* Mk; int mk_stride;
  float* Y; int y_stride;
  long long M;
};

__device__ __forceinline__ unsigned d_cvt_pk(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ u32x4d d_cvt8(const float4 lo, const float4 hi) {
  return u32x4d{d_cvt_pk(lo.x, lo.y), d_cvt_pk(lo.z, lo.w), d_cvt_pk(hi.x, hi.y), d_cvt_pk(hi.z, hi.w)};
}
// asm MFMA, accumulator tied (rowgemm_b3.hip, b3_mfma: why not the builtin); the waits around the groups as in gemm_bf16.hip (q_tie / q_ready / q_settle)
__device__ __forceinline__ void d_mfma(f32x4d& c, const u32x4d a, const u32x4d b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
template <typename T> __device__ __forceinline__ void d_tie(T& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void d_ready() { asm volatile("s_nop 4"); }
__device__ __forceinline__ void d_settle() { asm volatile("s_nop 15\n\ts_nop 15"); }

// K: cout; NP: the block's panel of the cin columns; KC: the K chunk a wave holds in registers
template <int K, int NP, int KC, int NTH>
__global__ __launch_bounds__(NTH) void k_lin_dgrad_bf16(LinDgradArgs p) {
  constexpr int NW = NTH / 64, KSC = KC / 32, NCH = K / KC, NT = NP / 16, G = 4, NG = NT / G;
  static_assert(K % KC == 0 && KC % 32 == 0 && NT % G == 0, "whole chunks, K steps and groups of sub-tiles");
  extern __shared__ __attribute__((aligned(16))) unsigned short sd[];      // [K / 8][NP][8] bf16
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.y * NP;
  const long long ngroups = (p.M + 15) / 16, gstride = (long long)gridDim.x * NW;

  // the panel's rows of the fp32 pack -> their bf16 image; consecutive threads take consecutive rows of one k-group (conflict-free 16-B writes)
  {
    const float* W = p.Wp + (long long)n0 * K;
    for (int i = tid; i < NP * (K / 8); i += NTH) {
      const int c = i / NP, r = i - c * NP;
      const float* src = W + (long long)r * K + c * 8;
      *reinterpret_cast<u32x4d*>(sd + (c * NP + r) * 8) = d_cvt8(*reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4));
    }
  }
  __syncthreads();

  const unsigned short* const wl = sd + (g * NP + l15) * 8;      // this lane's A-operand slot: k-group g, weight row l15 (+ 16 rows per sub-tile, + 4 NP slots per K step)
  float4 xr[KSC][2];
  auto load_chunk = [&](long long grp, int ch) {      // the lane's 8-float groups of chunk ch of its row
    long long row = grp * 16 + l15;
    if (row >= p.M) row = p.M - 1;
    const float* src = p.X + row * K + ch * KC + 8 * g;
#pragma unroll
    for (int s = 0; s < KSC; ++s) { xr[s][0] = *reinterpret_cast<const float4*>(src + 32 * s); xr[s][1] = *reinterpret_cast<const float4*>(src + 32 * s + 4); }
  };

  long long grp = blockIdx.x + (long long)gridDim.x * wave;      // (wave-uniform: the loop has no barrier)
  if (grp < ngroups) load_chunk(grp, 0);
  for (; grp < ngroups; grp += gstride) {
    const long long row = grp * 16 + l15;
    const bool live = row < p.M;
    const long long rr = live ? row : p.M - 1;
    f32x4d acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { acc[t] = f32x4d{0.f, 0.f, 0.f, 0.f}; d_tie(acc[t]); }
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      u32x4d xb[KSC];
#pragma unroll
      for (int s = 0; s < KSC; ++s) { xb[s] = d_cvt8(xr[s][0], xr[s][1]); d_tie(xb[s]); }
      // the next chunk, or the next rows' first one: in flight over this chunk's MFMAs
      if (ch + 1 < NCH) load_chunk(grp, ch + 1);
      else load_chunk(grp + gstride < ngroups ? grp + gstride : grp, 0);
      __builtin_amdgcn_sched_barrier(0);
      d_ready();
      const unsigned short* wc = wl + ch * KSC * 4 * NP * 8;
      // groups of G sub-tiles: the A operands of the next group are read from LDS while this group's MFMAs run; a chain's k ascends
      u32x4d w[2][G];
      auto read = [&](int i, u32x4d (&wd)[G]) {
        const int ks = i / NG, tg = i - ks * NG;
#pragma unroll
        for (int t = 0; t < G; ++t) wd[t] = *reinterpret_cast<const u32x4d*>(wc + (4 * ks * NP + 16 * (tg * G + t)) * 8);
      };
      read(0, w[0]);
#pragma unroll
      for (int i = 0; i < KSC * NG; ++i) {
        if (i + 1 < KSC * NG) read(i + 1, w[(i + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        const int ks = i / NG, tg = i - ks * NG;
#pragma unroll
        for (int t = 0; t < G; ++t) d_mfma(acc[tg * G + t], w[i & 1][t], xb[ks]);
      }
      d_settle();      // (the next chunk's cvt may reuse xb's registers, the epilogue reads acc)
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) d_tie(acc[t]);
    // the lane's mask and residual elements, 64 columns at a time; r1 may be dx: an element is read and then written by the same lane, and by no other
    const int col = n0 + 4 * g;
#pragma unroll
    for (int tg = 0; tg < NG; ++tg) {
      f32x4d mv[G], rv[G];
#pragma unroll
      for (int t = 0; t < G; ++t) {
        const int c = col + 16 * (tg * G + t);
        mv[t] = p.Mk ? *reinterpret_cast<const f32x4d*>(p.Mk + rr * p.mk_stride + c) : f32x4d{1.f, 1.f, 1.f, 1.f};
        rv[t] = p.R1 ? *reinterpret_cast<const f32x4d*>(p.R1 + rr * p.r1_stride + c) : f32x4d{-0.f, -0.f, -0.f, -0.f};      // (v + -0 = v for every v)
      }
      if (live) {
#pragma unroll
        for (int t = 0; t < G; ++t) {
          f32x4d v;
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = (mv[t][k] > 0.f ? acc[tg * G + t][k] : acc[tg * G + t][k] * 0.0f) + rv[t][k];      // (the default's mask: * mk_slope = 0)
          *reinterpret_cast<f32x4d*>(p.Y + row * p.y_stride + col + 16 * (tg * G + t)) = v;
        }
      }
    }
  }
}

int d_device() {
  int dev = 0;
  return (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) ? dev : -1;
}

template <int K, int NP, int KC>
int launch_lin_dgrad(const LinDgradArgs& p, int cin, hipStream_t st) {
  constexpr int smem = NP * K * 2, NTH = smem > 65536 ? 512 : 256;
  static_assert(smem <= 160 * 1024, "the panel's whole weight stays in LDS");
  static std::atomic<bool> attr_set[64];
  static std::atomic<int> resident[64];
  const int dev = d_device();
  if (dev < 0) return LFSR_E_ARG;
  const void* kern = reinterpret_cast<const void*>(k_lin_dgrad_bf16<K, NP, KC, NTH>);
  if (!attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return LFSR_HIP_ERR(e);
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, NTH, (size_t)smem) != hipSuccess || per_cu < 1) per_cu = 1;
    if (per_cu > 2) per_cu = 2;      // (as gemm_bf16.hip: more blocks only stage the weights more often)
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    resident[dev] = per_cu * cus;
    attr_set[dev] = true;
  }
  const int ny = cin / NP;
  const long long ntiles = (p.M + NTH / 4 - 1) / (NTH / 4);
  long long gx = resident[dev] / ny;
  if (gx > ntiles) gx = ntiles;
  if (gx < 1) gx = 1;
  hipLaunchKernelGGL((k_lin_dgrad_bf16<K, NP, KC, NTH>), dim3((unsigned)gx, (unsigned)ny), dim3(NTH), smem, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

}  // namespace

// The caller has made the default's argument checks.  LFSR_E_ARG: not covered (a pointer off the 16-byte grid), nothing written: the caller runs the default kernel
int lfsr_lin_dgrad_bf16_launch(const float* dy, int cout, const float* wT_packed, float* dx, int dx_stride, const float* r1, int r1_stride, const float* act,
                               int act_stride, long long M, int cin, hipStream_t st) {
  if (!dy || !wT_packed || !dx || M <= 0) return LFSR_E_ARG;
  if (((uintptr_t)dy | (uintptr_t)wT_packed | (uintptr_t)dx | (uintptr_t)r1 | (uintptr_t)act) & 15) return LFSR_E_ARG;
  if ((dx_stride & 3) || (r1 && (r1_stride & 3)) || (act && (act_stride & 3))) return LFSR_E_ARG;
  LinDgradArgs p{};
  p.X = dy; p.Wp = wT_packed; p.R1 = r1; p.r1_stride = r1_stride; p.Mk = act; p.mk_stride = act_stride; p.Y = dx; p.y_stride = dx_stride; p.M = M;
  switch (cout * 1000 + cin) {
    case 64064: return launch_lin_dgrad<64, 64, 64>(p, cin, st);
    case 64128: return launch_lin_dgrad<64, 128, 64>(p, cin, st);
    case 64256: return launch_lin_dgrad<64, 256, 64>(p, cin, st);
    case 128064: return launch_lin_dgrad<128, 64, 128>(p, cin, st);
    case 128128: return launch_lin_dgrad<128, 128, 128>(p, cin, st);
    case 128256: return launch_lin_dgrad<128, 256, 128>(p, cin, st);
    case 256064: return launch_lin_dgrad<256, 64, 128>(p, cin, st);
    case 256128: return launch_lin_dgrad<256, 128, 128>(p, cin, st);
    case 256256: return launch_lin_dgrad<256, 256, 128>(p, cin, st);
    case 576064: return launch_lin_dgrad<576, 64, 192>(p, cin, st);
    case 576128: return launch_lin_dgrad<576, 128, 192>(p, cin, st);
    case 576256: return launch_lin_dgrad<576, 128, 192>(p, cin, st);
    case 1024064: return launch_lin_dgrad<1024, 64, 128>(p, cin, st);
    case 1024128: return launch_lin_dgrad<1024, 64, 128>(p, cin, st);
    case 1024256: return launch_lin_dgrad<1024, 64, 128>(p, cin, st);
    default: return LFSR_E_ARG;
  }
}
