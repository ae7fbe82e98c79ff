// The transformer GEMMs of lfsr_set_gemm_arithmetic(LFSR_GEMM_ARITH_BF16): bias-free linear, LayerNorm + q | k | v projection and the feed-forward block with bf16
// OPERANDS.  Activations and weights are rounded to bf16 once (v_cvt_pk_bf16_f32: nearest even), the products are exact and run on v_mfma_f32_16x16x32_bf16; accumulation,
// LayerNorm, ReLU / slope, residual add and stores are fp32.  Activations stay fp32 in memory: the mode changes arithmetic, not storage.  One product per K step where
// the three-term kernels (rowgemm_b3.hip, lnlin_b3.hip, ffn_b3.hip) issue six, and no split VALU.
//
// Structure (all three kernels): the block's WHOLE weight is converted from the fp32 pack while it is staged into LDS, once per block, so the tile loop has no barrier
// and no restaging.  The LDS image is rowgemm_b3.hip's, one plane of it: [k-group c = k / 8][weight row n][8 bf16] -- consecutive rows 16 B apart, the k-groups a
// multiple of 256 B apart, so each of ds_read_b128's four lane groups covers the 16 slots of a bank row exactly once (that file: why padded rows did worse there).
// A wave owns 16 token rows at a time and loads them straight from global memory in B-operand order (lane = row l15, k-group g: eight consecutive k per K step), so
// X is streamed ONCE per launch, whatever N is (the panel kernels read it once per 64 or 128 output columns).  D[channel][row]: A = the weight rows, B = the token
// rows; lane (l15, g) ends up with channels 16 t + 4 g .. + 3 of its row, i.e. 16-B stores.
// Feed-forward: GEMM 1 computed this way leaves lane (l15, g) with hidden units 16 t + 4 g .. + 3 of its row -- after ReLU and cvt_pk the accumulators of sub-tiles
// 2 s and 2 s + 1 ARE a B operand of GEMM 2's K step s, with the k order {32 s + 4 g + i, 32 s + 16 + 4 g + i}; W2's LDS image is stored in that order.
// Memory schedule: the wave's next rows are requested before this tile's MFMAs; every residual load of a tile is issued before its first store; loads and stores go
// through buffer descriptors whose extent ends at row M, so rows past M are neither read (they arrive as zeros, without traffic) nor written, and the tile loop is
// straight-line code in which the compiler counts its waits.
// Determinism: no atomics, one wave and one summation chain (k ascending in K steps of 32) per output element: two runs give the same bits, and a row's result does
// not depend on M or on the grid.
#include <stdlib.h>

#include "lfsr_internal.h"

namespace {

typedef float f32x4q __attribute__((ext_vector_type(4)));
typedef unsigned u32x4q __attribute__((ext_vector_type(4)));

struct GemmB16Args {
  const float* X; int x_stride; int x_choff;
  const float* Wp;       // [N rows][K] fp32 (packed, k contiguous)
  const float* R1; int r1_stride; int r1_choff;
  float* Y; int y_stride; int y_choff;
  long long M;
  float slope;
  // LN form (as RowGemmArgs in rowgemm.hip): columns n < ln_cols see LayerNorm(x (+ pe)), the others the raw rows; columns n >= split_n go to Y2
  const float* ln_g; const float* ln_b; float ln_eps; int ln_cols;
  const float* pe; int pe_stride; int pe_rows; int pe_div;
  float* Y2; int y2_stride; int y2_choff; int split_n;
};

struct FfnB16Args {
  const float* X; int x_stride; int x_choff;
  const float* W1;       // [H][E]
  const float* W2;       // [E][H]
  const float* R; int r_stride; int r_choff;
  float* Y; int y_stride; int y_choff;
  long long M;
  float slope;
  const float* ln_g; const float* ln_b; float ln_eps;
};

// two fp32 -> one register of two bf16, round to nearest even, element 0 in the low half (MFMA operand order)
__device__ __forceinline__ unsigned q_cvt_pk(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ u32x4q q_cvt8(const float4 lo, const float4 hi) {
  return u32x4q{q_cvt_pk(lo.x, lo.y), q_cvt_pk(lo.z, lo.w), q_cvt_pk(hi.x, hi.y), q_cvt_pk(hi.z, hi.w)};
}
// asm MFMA, accumulator tied (rowgemm_b3.hip, b3_mfma: why not the builtin)
__device__ __forceinline__ void q_mfma(f32x4q& c, const u32x4q a, const u32x4q b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
// The compiler sees no MFMA in those statements and pads no wait states around them.  q_tie pins a register set to a point of the (ordered) volatile-asm stream:
// what produced it is scheduled in front of that point, what reads it behind.  In front of an MFMA group: tie every source, then q_ready; behind one: q_settle, then
// tie every accumulator (tools/check_asm_mfma_hazards.py checks the result).
template <typename T> __device__ __forceinline__ void q_tie(T& v) { asm volatile("" : "+v"(v)); }
__device__ __forceinline__ void q_ready() { asm volatile("s_nop 4"); }
__device__ __forceinline__ void q_settle() { asm volatile("s_nop 15\n\ts_nop 15"); }

// the fp32 pack [rows][K] -> its bf16 LDS image [K / 8][rows][8]; consecutive threads take consecutive rows of one k-group (conflict-free 16-B writes)
template <int K, int NTH>
__device__ __forceinline__ void q_stage(const float* __restrict__ W, int rows, unsigned short* sw, int tid) {
  for (int i = tid; i < rows * (K / 8); i += NTH) {
    const int c = i / rows, r = i - c * rows;
    const float* src = W + (long long)r * K + c * 8;
    *reinterpret_cast<u32x4q*>(sw + (c * rows + r) * 8) = q_cvt8(*reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 4));
  }
}

// nn.LayerNorm(K) of the lane's row, in place (rowgemm_b3.hip's arithmetic, operation for operation): the row's K values sit in the four lanes (row l15, g = 0..3)
template <int K>
__device__ __forceinline__ void q_layernorm(float4 (&xr)[K / 32][2], const float* sgb, float eps, int g) {
  constexpr int KS = K / 32;
  float sm = 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int e = 0; e < 2; ++e) sm += (xr[s][e].x + xr[s][e].y) + (xr[s][e].z + xr[s][e].w);
  sm += __shfl_xor(sm, 16);
  sm += __shfl_xor(sm, 32);
  const float mu = sm * (1.0f / K);
  float q2 = 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      xr[s][e].x -= mu; xr[s][e].y -= mu; xr[s][e].z -= mu; xr[s][e].w -= mu;
      q2 += (xr[s][e].x * xr[s][e].x + xr[s][e].y * xr[s][e].y) + (xr[s][e].z * xr[s][e].z + xr[s][e].w * xr[s][e].w);
    }
  q2 += __shfl_xor(q2, 16);
  q2 += __shfl_xor(q2, 32);
  const float rstd = 1.0f / sqrtf(q2 * (1.0f / K) + eps);
#pragma unroll
  for (int s = 0; s < KS; ++s)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float4 gv = *reinterpret_cast<const float4*>(sgb + 32 * s + 8 * g + 4 * e);
      const float4 bv = *reinterpret_cast<const float4*>(sgb + K + 32 * s + 8 * g + 4 * e);
      xr[s][e] = make_float4(xr[s][e].x * rstd * gv.x + bv.x, xr[s][e].y * rstd * gv.y + bv.y, xr[s][e].z * rstd * gv.z + bv.z, xr[s][e].w * rstd * gv.w + bv.w);
    }
}

constexpr int Q_RSRC = 0x00020000;

// acc[t] += W[16 t + ., k] x[., k] over NT sub-tiles and KS K steps of one LDS weight image of ROWS rows (wl: the lane's slot of row l15, k-group g), in groups of
// G sub-tiles: the A operands of the next group are read from LDS while this group's MFMAs run.  A chain's k ascends (the K step is the outer index).
template <int KS, int NT, int G, int ROWS>
__device__ __forceinline__ void q_gemm(f32x4q (&acc)[NT], const unsigned short* wl, const u32x4q (&xo)[KS]) {
  constexpr int NG = NT / G, STEPS = KS * NG;
  static_assert(NT % G == 0, "whole groups");
  u32x4q w[2][G];
  auto read = [&](int i, u32x4q (&wd)[G]) {
    const int ks = i / NG, tg = i - ks * NG;
#pragma unroll
    for (int t = 0; t < G; ++t) wd[t] = *reinterpret_cast<const u32x4q*>(wl + (4 * ks * ROWS + 16 * (tg * G + t)) * 8);
  };
  read(0, w[0]);
#pragma unroll
  for (int i = 0; i < STEPS; ++i) {
    if (i + 1 < STEPS) read(i + 1, w[(i + 1) & 1]);
    __builtin_amdgcn_sched_barrier(0);
    const int ks = i / NG, tg = i - ks * NG;
#pragma unroll
    for (int t = 0; t < G; ++t) q_mfma(acc[tg * G + t], w[i & 1][t], xo[ks]);
  }
}

// the lane's 8-float groups of its token row: the row (and k-group) in the VGPR offset, which the descriptor's bounds check covers; the channel offset in the
// scalar offset, which it does not (a row below M is inside the extent with all of its channels, x_stride >= x_choff + K)
template <int K>
__device__ __forceinline__ void q_load_rows(float4 (&xr)[K / 32][2], const __amdgpu_buffer_rsrc_t rsX, unsigned vo, int x_choff) {
#pragma unroll
  for (int s = 0; s < K / 32; ++s)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const f32x4q v = __builtin_bit_cast(f32x4q, __builtin_amdgcn_raw_buffer_load_b128(rsX, vo, (x_choff + 32 * s + 4 * e) * 4, 0));
      xr[s][e] = make_float4(v.x, v.y, v.z, v.w);
    }
}

// Linear (LN = false: act(x W^T) (+ res)) and LayerNorm + projections (LN = true), all N columns.  The 16-row groups are dealt to the waves wave-major (group = block +
// blocks x (wave + waves x round)), so a last, partial round is spread over every CU instead of filling a few of them (1600 128-row tiles on 256 blocks: 7 rounds for 6.25).
template <int K, int N, bool LN, int NTH>
__global__ __launch_bounds__(NTH) void k_gemm_bf16(GemmB16Args p) {
  constexpr int NW = NTH / 64, KS = K / 32, NP = N / 64, NT = N / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned short sq[];      // [K / 8][N][8] bf16, then (LN) gamma[K], beta[K] as fp32
  float* const sgb = reinterpret_cast<float*>(sq + N * K);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const long long ngroups = (p.M + 15) / 16, gstride = (long long)gridDim.x * NW;

  q_stage<K, NTH>(p.Wp, N, sq, tid);
  if constexpr (LN) for (int i = tid; i < 2 * K; i += NTH) sgb[i] = i < K ? p.ln_g[i] : p.ln_b[i - K];
  __syncthreads();

  const int rowl = l15;
  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), 0, (int)(p.M * p.x_stride * 4), Q_RSRC);
  const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc(p.Y, 0, (int)(p.M * p.y_stride * 4), Q_RSRC);
  const __amdgpu_buffer_rsrc_t rsY2 = __builtin_amdgcn_make_buffer_rsrc(p.Y2 ? p.Y2 : p.Y, 0, p.Y2 ? (int)(p.M * p.y2_stride * 4) : 0, Q_RSRC);
  const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.R1 ? p.R1 : p.X), 0, p.R1 ? (int)(p.M * p.r1_stride * 4) : 0, Q_RSRC);
  const unsigned voX = (unsigned)((rowl * p.x_stride + 8 * g) * 4);
  const unsigned voY = (unsigned)((rowl * p.y_stride + 4 * g) * 4), voY2 = (unsigned)((rowl * p.y2_stride + 4 * g) * 4), voR = (unsigned)((rowl * p.r1_stride + 4 * g) * 4);
  const bool has_res = !LN && p.R1 != nullptr;
  const unsigned short* const wl = sq + (g * N + l15) * 8;      // this lane's A-operand slot: k-group g, weight row l15 (+ 16 rows per sub-tile, + 4 N slots per K step)

  float4 xr[KS][2];
  float4 pr[LN ? KS : 1][2];
  auto prefetch = [&](long long grp) {      // (past the last group: rows >= M, zeros without traffic)
    const int so = (int)(grp * 16);
    q_load_rows<K>(xr, rsX, voX + (unsigned)(so * p.x_stride * 4), p.x_choff);
    if constexpr (LN) if (p.pe) {
      const float* pp = p.pe + (long long)(((so + rowl) / p.pe_div) % p.pe_rows) * p.pe_stride + 8 * g;
#pragma unroll
      for (int s = 0; s < KS; ++s) { pr[s][0] = *reinterpret_cast<const float4*>(pp + 32 * s); pr[s][1] = *reinterpret_cast<const float4*>(pp + 32 * s + 4); }
    }
  };
  long long grp = blockIdx.x + (long long)gridDim.x * wave;      // (wave-uniform: the loop has no barrier)
  prefetch(grp < ngroups ? grp : ngroups);
  for (; grp < ngroups; grp += gstride) {
    const int so = (int)(grp * 16);
    // this group's residual rows, all of them in front of its first store
    f32x4q rv[LN ? 1 : NT];
    if constexpr (!LN) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const f32x4q v = __builtin_bit_cast(f32x4q, __builtin_amdgcn_raw_buffer_load_b128(rsR, voR + (unsigned)(so * p.r1_stride * 4), (p.r1_choff + 16 * t) * 4, 0));
        rv[t] = has_res ? v : f32x4q{-0.f, -0.f, -0.f, -0.f};      // (v + -0 = v for every v, the sign of a zero included)
      }
    }
    // operands: the raw rows, and (LN) their LayerNorm, rounded once
    u32x4q xb[KS], xl[LN ? KS : 1];
#pragma unroll
    for (int s = 0; s < KS; ++s) xb[s] = q_cvt8(xr[s][0], xr[s][1]);
    if constexpr (LN) {
      if (p.pe) {
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
          for (int e = 0; e < 2; ++e) { xr[s][e].x += pr[s][e].x; xr[s][e].y += pr[s][e].y; xr[s][e].z += pr[s][e].z; xr[s][e].w += pr[s][e].w; }
      }
      q_layernorm<K>(xr, sgb, p.ln_eps, g);
#pragma unroll
      for (int s = 0; s < KS; ++s) xl[s] = q_cvt8(xr[s][0], xr[s][1]);
    }
    // the next tile's rows: in flight over this tile's MFMAs and stores
    prefetch(grp + gstride < ngroups ? grp + gstride : ngroups);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int pn = 0; pn < NP; ++pn) {
      f32x4q acc[4];
      u32x4q xo[KS];
      const bool ln = LN && 64 * pn < p.ln_cols;      // (block-uniform: one code path, the operand chosen by a select)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        if constexpr (LN) {
#pragma unroll
          for (int j = 0; j < 4; ++j) xo[s][j] = ln ? xl[s][j] : xb[s][j];
        } else xo[s] = xb[s];
        q_tie(xo[s]);
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) { acc[t] = f32x4q{0.f, 0.f, 0.f, 0.f}; q_tie(acc[t]); }
      q_ready();
      q_gemm<KS, 4, 4, N>(acc, wl + 64 * pn * 8, xo);
      q_settle();
#pragma unroll
      for (int t = 0; t < 4; ++t) q_tie(acc[t]);
      const bool second = LN && p.Y2 && 64 * pn >= p.split_n;      // (block-uniform)
      const __amdgpu_buffer_rsrc_t rs = second ? rsY2 : rsY;
      // (the channel offset goes into the VGPR / immediate offset, which the descriptor's bounds check covers, and the scalar offset stays 0 -- as the sibling
      //  kernels' stores; what was measured with the offset in an SGPR instead: DESIGN.md section 6g)
      const unsigned vo = (second ? voY2 + (unsigned)((so * p.y2_stride + p.y2_choff - p.split_n) * 4) : voY + (unsigned)((so * p.y_stride + p.y_choff) * 4)) + 256u * pn;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float v[4] = {acc[t][0], acc[t][1], acc[t][2], acc[t][3]};
        if constexpr (!LN) {
#pragma unroll
          for (int k = 0; k < 4; ++k) { v[k] = v[k] >= 0.f ? v[k] : v[k] * p.slope; v[k] += rv[4 * pn + t][k]; }
        }
        __builtin_amdgcn_raw_buffer_store_b128(u32x4q{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])}, rs, vo + 64u * t, 0, 0);
      }
    }
  }
}

// y = res + W2 . act(W1 . LN(x)), E -> 2 E -> E, 512 threads: 128 token rows per tile.  has_ln false: x is taken as it is.
template <int E>
__global__ __launch_bounds__(512) void k_ffn_bf16(FfnB16Args p) {
  constexpr int NTH = 512, BMR = 128, H = 2 * E, KS1 = E / 32, NT1 = H / 16, KS2 = H / 32, NT2 = E / 16, G = NT2;
  extern __shared__ __attribute__((aligned(16))) unsigned short sq[];      // W1 [E / 8][H][8] | W2 [H / 8][E][8] (GEMM-2 k order) | gamma[E], beta[E] as fp32
  unsigned short* const sw1 = sq;
  unsigned short* const sw2 = sq + H * E;
  float* const sgb = reinterpret_cast<float*>(sq + 2 * H * E);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const long long ntiles = (p.M + BMR - 1) / BMR;
  const bool has_ln = p.ln_g != nullptr;

  q_stage<E, NTH>(p.W1, H, sw1, tid);
  // W2: slot (c = 4 s + g, row n) <- hidden units 32 s + 4 g + {0..3}, 32 s + 16 + 4 g + {0..3}: what lane (., g) holds of GEMM 1's sub-tiles 2 s and 2 s + 1
  for (int i = tid; i < E * (H / 8); i += NTH) {
    const int c = i / E, n = i - c * E;
    const float* src = p.W2 + (long long)n * H + 32 * (c >> 2) + 4 * (c & 3);
    *reinterpret_cast<u32x4q*>(sw2 + (c * E + n) * 8) = q_cvt8(*reinterpret_cast<const float4*>(src), *reinterpret_cast<const float4*>(src + 16));
  }
  if (has_ln) for (int i = tid; i < 2 * E; i += NTH) sgb[i] = i < E ? p.ln_g[i] : p.ln_b[i - E];
  __syncthreads();

  const int rowl = wave * 16 + l15;
  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), 0, (int)(p.M * p.x_stride * 4), Q_RSRC);
  const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc(p.Y, 0, (int)(p.M * p.y_stride * 4), Q_RSRC);
  const __amdgpu_buffer_rsrc_t rsR = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.R ? p.R : p.X), 0, p.R ? (int)(p.M * p.r_stride * 4) : 0, Q_RSRC);
  const unsigned voX = (unsigned)((rowl * p.x_stride + 8 * g) * 4), voY = (unsigned)((rowl * p.y_stride + 4 * g) * 4), voR = (unsigned)((rowl * p.r_stride + 4 * g) * 4);
  const bool has_res = p.R != nullptr;
  const unsigned short* const wl1 = sw1 + (g * H + l15) * 8;
  const unsigned short* const wl2 = sw2 + (g * E + l15) * 8;

  float4 xr[KS1][2];
  long long tile = blockIdx.x;
  q_load_rows<E>(xr, rsX, voX + (unsigned)((int)((tile < ntiles ? tile : ntiles) * BMR) * p.x_stride * 4), p.x_choff);
  for (; tile < ntiles; tile += gridDim.x) {
    const int so = (int)(tile * BMR);
    if (has_ln) q_layernorm<E>(xr, sgb, p.ln_eps, g);      // (block-uniform)
    u32x4q xb[KS1];
#pragma unroll
    for (int s = 0; s < KS1; ++s) { xb[s] = q_cvt8(xr[s][0], xr[s][1]); q_tie(xb[s]); }
    // this tile's residual rows (in front of its first store), then the next tile's rows: both in flight over the MFMAs
    f32x4q rv[NT2];
#pragma unroll
    for (int t = 0; t < NT2; ++t) {
      const f32x4q v = __builtin_bit_cast(f32x4q, __builtin_amdgcn_raw_buffer_load_b128(rsR, voR + (unsigned)(so * p.r_stride * 4), (p.r_choff + 16 * t) * 4, 0));
      rv[t] = has_res ? v : f32x4q{-0.f, -0.f, -0.f, -0.f};
    }
    {
      const long long nx = tile + gridDim.x < ntiles ? tile + gridDim.x : ntiles;
      q_load_rows<E>(xr, rsX, voX + (unsigned)((int)(nx * BMR) * p.x_stride * 4), p.x_choff);
    }
    __builtin_amdgcn_sched_barrier(0);
    // GEMM 1 (transposed): h[hidden][row]
    f32x4q a1[NT1];
#pragma unroll
    for (int t = 0; t < NT1; ++t) { a1[t] = f32x4q{0.f, 0.f, 0.f, 0.f}; q_tie(a1[t]); }
    q_ready();
    q_gemm<KS1, NT1, G, H>(a1, wl1, xb);
    q_settle();
#pragma unroll
    for (int t = 0; t < NT1; ++t) q_tie(a1[t]);
    // activation, rounded once: sub-tiles 2 s, 2 s + 1 -> the B operand of GEMM 2's K step s
    u32x4q hb[KS2];
#pragma unroll
    for (int s = 0; s < KS2; ++s) {
      float h[8];
#pragma unroll
      for (int k = 0; k < 4; ++k) { h[k] = a1[2 * s][k]; h[4 + k] = a1[2 * s + 1][k]; }
#pragma unroll
      for (int k = 0; k < 8; ++k) h[k] = h[k] >= 0.f ? h[k] : h[k] * p.slope;
      hb[s] = u32x4q{q_cvt_pk(h[0], h[1]), q_cvt_pk(h[2], h[3]), q_cvt_pk(h[4], h[5]), q_cvt_pk(h[6], h[7])};
      q_tie(hb[s]);
    }
    // GEMM 2 (transposed): y[n][row]
    f32x4q a2[NT2];
#pragma unroll
    for (int t = 0; t < NT2; ++t) { a2[t] = f32x4q{0.f, 0.f, 0.f, 0.f}; q_tie(a2[t]); }
    q_ready();
    q_gemm<KS2, NT2, G, E>(a2, wl2, hb);
    q_settle();
#pragma unroll
    for (int t = 0; t < NT2; ++t) q_tie(a2[t]);
    const unsigned vo = voY + (unsigned)((so * p.y_stride + p.y_choff) * 4);      // (the channel offset in the VGPR offset, as k_gemm_bf16's stores)
#pragma unroll
    for (int t = 0; t < NT2; ++t) {
      const f32x4q v = a2[t] + rv[t];
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4q, v), rsY, vo + 64u * t, 0, 0);
    }
  }
}

int q_device() {
  int dev = 0;
  return (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) ? dev : -1;
}
// the blocks of `kernel` the device holds at once (LDS and registers as compiled): the grid of a persistent launch
int q_resident_blocks(const void* kernel, int nth, int smem, int dev) {
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, nth, (size_t)smem) != hipSuccess || per_cu < 1) per_cu = 1;
  if (per_cu > 2) per_cu = 2;      // (eight waves per CU keep HBM busy; more blocks only stage the weights more often)
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
  return per_cu * cus;
}

template <int K, int N, bool LN, int NTH>
int launch_gemm_bf16(const GemmB16Args& p, hipStream_t st) {
  constexpr int smem = N * K * 2 + (LN ? 2 * K * 4 : 0);
  static_assert(smem <= 160 * 1024, "the whole weight stays in LDS");
  static std::atomic<bool> attr_set[64];
  static std::atomic<int> resident[64];
  const int dev = q_device();
  if (dev < 0) return LFSR_E_ARG;
  if (!attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_gemm_bf16<K, N, LN, NTH>), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return LFSR_HIP_ERR(e);
    resident[dev] = q_resident_blocks(reinterpret_cast<const void*>(k_gemm_bf16<K, N, LN, NTH>), NTH, smem, dev);
    attr_set[dev] = true;
  }
  const long long ntiles = (p.M + NTH / 4 - 1) / (NTH / 4);
  long long gx = resident[dev];
  if (gx > ntiles) gx = ntiles;
  hipLaunchKernelGGL((k_gemm_bf16<K, N, LN, NTH>), dim3((unsigned)gx), dim3(NTH), smem, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

template <int E>
int launch_ffn_bf16(const FfnB16Args& p, hipStream_t st) {
  constexpr int smem = 2 * (2 * E) * E * 2 + 2 * E * 4;
  static_assert(smem <= 160 * 1024, "the whole weight stays in LDS");
  static std::atomic<bool> attr_set[64];
  static std::atomic<int> resident[64];
  const int dev = q_device();
  if (dev < 0) return LFSR_E_ARG;
  if (!attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_ffn_bf16<E>), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return LFSR_HIP_ERR(e);
    resident[dev] = q_resident_blocks(reinterpret_cast<const void*>(k_ffn_bf16<E>), 512, smem, dev);
    attr_set[dev] = true;
  }
  const long long ntiles = (p.M + 127) / 128;
  long long gx = resident[dev];
  if (gx > ntiles) gx = ntiles;
  hipLaunchKernelGGL((k_ffn_bf16<E>), dim3((unsigned)gx), dim3(512), smem, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

// 32-bit buffer offsets: a last partial tile and the tile past the end included
bool q_span_ok(long long M, int stride) { return (M + 256) * (long long)stride * 4 < (1LL << 31); }

}  // namespace

// LFSR_E_ARG = shape or operands not covered; nothing is written then
int lfsr_gemm_bf16_launch(const LfsrLin& c, hipStream_t st) {
  if (!c.x || !c.w_packed || !c.y || c.M <= 0 || (c.K != 64 && c.K != 128) || (c.N != 64 && c.N != 128 && c.N != 256)) return LFSR_E_ARG;
  if ((c.x_stride | c.x_choff | c.y_stride | c.y_choff) & 3 || (c.res && ((c.res_stride | c.res_choff) & 3))) return LFSR_E_ARG;
  if (c.x_choff < 0 || c.y_choff < 0 || (c.res && c.res_choff < 0) || c.x_stride < c.x_choff + c.K || c.y_stride < c.y_choff + c.N || (c.res && c.res_stride < c.res_choff + c.N)) return LFSR_E_ARG;
  if (((uintptr_t)c.y | (uintptr_t)c.x | (uintptr_t)c.res | (uintptr_t)c.w_packed) & 15) return LFSR_E_ARG;
  if (!q_span_ok(c.M, c.x_stride) || !q_span_ok(c.M, c.y_stride) || (c.res && !q_span_ok(c.M, c.res_stride))) return LFSR_E_ARG;
  GemmB16Args p{};
  p.X = c.x; p.x_stride = c.x_stride; p.x_choff = c.x_choff; p.Wp = c.w_packed; p.R1 = c.res; p.r1_stride = c.res_stride; p.r1_choff = c.res_choff;
  p.Y = c.y; p.y_stride = c.y_stride; p.y_choff = c.y_choff; p.M = c.M; p.slope = c.slope;
  switch (c.K * 1000 + c.N) {
    case 64064: return launch_gemm_bf16<64, 64, false, 256>(p, st);
    case 64128: return launch_gemm_bf16<64, 128, false, 256>(p, st);
    case 64256: return launch_gemm_bf16<64, 256, false, 256>(p, st);
    case 128064: return launch_gemm_bf16<128, 64, false, 256>(p, st);
    case 128128: return launch_gemm_bf16<128, 128, false, 256>(p, st);
    case 128256: return launch_gemm_bf16<128, 256, false, 256>(p, st);
    default: return LFSR_E_ARG;
  }
}

// LayerNorm + q | k | v projection (the LN form of LfsrLin); (K, N) = (128, 384) or (64, 192)
int lfsr_gemm_bf16_ln_launch(const LfsrLin& c, hipStream_t st) {
  if (!((c.K == 128 && c.N == 384) || (c.K == 64 && c.N == 192)) || !c.x || !c.w_packed || !c.ln_g || !c.ln_b || !c.y || c.M <= 0 || c.ln_cols < 0 || c.ln_cols > c.N || c.ln_cols % 64) return LFSR_E_ARG;
  if (c.y2 && (c.split_n % 64 || c.split_n <= 0 || c.split_n >= c.N)) return LFSR_E_ARG;
  if ((c.x_stride | c.x_choff | c.y_stride | c.y_choff) & 3 || (c.y2 && ((c.y2_stride | c.y2_choff) & 3)) || (c.pe && ((c.pe_stride & 3) || c.pe_stride < c.K || c.pe_rows <= 0 || c.pe_div <= 0))) return LFSR_E_ARG;
  if (c.x_choff < 0 || c.y_choff < 0 || (c.y2 && c.y2_choff < 0)) return LFSR_E_ARG;
  if (c.x_stride < c.x_choff + c.K || c.y_stride < c.y_choff + (c.y2 ? c.split_n : c.N) || (c.y2 && c.y2_stride < c.y2_choff + c.N - c.split_n)) return LFSR_E_ARG;
  if (((uintptr_t)c.y | (uintptr_t)c.y2 | (uintptr_t)c.x | (uintptr_t)c.pe | (uintptr_t)c.ln_g | (uintptr_t)c.ln_b | (uintptr_t)c.w_packed) & 15) return LFSR_E_ARG;
  if (!q_span_ok(c.M, c.x_stride) || !q_span_ok(c.M, c.y_stride) || (c.y2 && !q_span_ok(c.M, c.y2_stride))) return LFSR_E_ARG;
  GemmB16Args p{};
  p.X = c.x; p.x_stride = c.x_stride; p.x_choff = c.x_choff; p.Wp = c.w_packed; p.Y = c.y; p.y_stride = c.y_stride; p.y_choff = c.y_choff; p.M = c.M; p.slope = 1.0f;
  p.ln_g = c.ln_g; p.ln_b = c.ln_b; p.ln_eps = c.ln_eps; p.ln_cols = c.ln_cols; p.pe = c.pe; p.pe_stride = c.pe_stride; p.pe_rows = c.pe_rows; p.pe_div = c.pe_div;
  p.Y2 = c.y2; p.y2_stride = c.y2_stride; p.y2_choff = c.y2_choff; p.split_n = c.split_n;
  return c.K == 128 ? launch_gemm_bf16<128, 384, true, 512>(p, st) : launch_gemm_bf16<64, 192, true, 512>(p, st);
}

// feed-forward block, (K1, H, N2) = (128, 256, 128) or (64, 128, 64); ln_g / ln_b null: x is already normalised
int lfsr_ffn_bf16_launch(const LfsrFfn& f, hipStream_t st) {
  if (!((f.K1 == 128 && f.H == 256 && f.N2 == 128) || (f.K1 == 64 && f.H == 128 && f.N2 == 64)) || !f.x || !f.w1_packed || !f.w2_packed || !f.y || f.M <= 0) return LFSR_E_ARG;
  if ((f.ln_g != nullptr) != (f.ln_b != nullptr)) return LFSR_E_ARG;
  if ((f.x_stride | f.x_choff | f.y_stride | f.y_choff) & 3 || (f.res && ((f.res_stride | f.res_choff) & 3))) return LFSR_E_ARG;
  if (f.x_choff < 0 || f.y_choff < 0 || (f.res && f.res_choff < 0) || f.x_stride < f.x_choff + f.K1 || f.y_stride < f.y_choff + f.N2 || (f.res && f.res_stride < f.res_choff + f.N2)) return LFSR_E_ARG;
  if (((uintptr_t)f.x | (uintptr_t)f.y | (uintptr_t)f.res | (uintptr_t)f.w1_packed | (uintptr_t)f.w2_packed | (uintptr_t)f.ln_g | (uintptr_t)f.ln_b) & 15) return LFSR_E_ARG;
  if (!q_span_ok(f.M, f.x_stride) || !q_span_ok(f.M, f.y_stride) || (f.res && !q_span_ok(f.M, f.res_stride))) return LFSR_E_ARG;
  FfnB16Args p{};
  p.X = f.x; p.x_stride = f.x_stride; p.x_choff = f.x_choff; p.W1 = f.w1_packed; p.W2 = f.w2_packed;
  p.R = f.res; p.r_stride = f.res_stride; p.r_choff = f.res_choff; p.Y = f.y; p.y_stride = f.y_stride; p.y_choff = f.y_choff;
  p.M = f.M; p.slope = f.slope; p.ln_g = f.ln_g; p.ln_b = f.ln_b; p.ln_eps = f.ln_eps;
  return f.K1 == 128 ? launch_ffn_bf16<128>(p, st) : launch_ffn_bf16<64>(p, st);
}
