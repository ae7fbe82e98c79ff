// Per-view 3x3 conv, zero pad 1, 64 -> 64 channels, VCL layout, with bf16 OPERANDS: the kernel body shared by the forward of lfsr_set_arithmetic(LFSR_ARITH_BF16)
// (conv3x3_bf16.hip, MASK = false) and the data gradient of lfsr_set_grad_arithmetic(LFSR_GRAD_ARITH_BF16) (conv3x3_bf16_dgrad.hip: the same conv on the transposed,
// tap-flipped pack; MASK = true multiplies by the LeakyReLU derivative at the saved activation mk before the residual adds).
// Activations and weights are rounded to bf16 (v_cvt_pk_bf16_f32: nearest even), the products are exact and run on v_mfma_f32_32x32x16_bf16, accumulation, LeakyReLU,
// residual adds and stores are fp32.  Activations stay fp32 in memory: the mode changes arithmetic, not storage.
//
// The structure is conv3x3_halo.hip's: one persistent 512-thread block (8 waves) per CU walks 8-row x 32-column tiles of view images; a tile's (8+2) x (32+2) input
// halo is staged into LDS once (zero-filled outside the image = the conv's padding), converted to bf16 on the way, and all 9 taps read it at shifted addresses.  Wave w
// owns image row w of the tile (32 pixels = the 32 A-rows of the MFMA) x all 64 output channels (2 column tiles, 32 accumulator registers): 9 taps x 4 K steps of 16
// channels x 2 = 72 MFMAs per tile and wave.  Unlike the fp32 kernel the WHOLE weight (the direct pack [9][64][64], converted once per block) stays in LDS, so a tile's
// MFMA stream has no barrier in it.  The next tile's halo is fetched into registers while this tile computes (the kernel is bound by HBM, not by the matrix pipe:
// 60.4 GFLOP per launch at 800 images of 32x32 are ~24 us of bf16 matrix time against 63 us of operand traffic at 8 TB/s).
// LDS: rows of 64 bf16 padded to 144 B (conflict-free ds_read_b128: 8 consecutive rows start in 8 distinct 16-B slots of a 128-B bank line pair) --
// 340 x 144 B (halo) + 576 x 144 B (weights) = 131 904 B, one block per CU, 2 waves per SIMD.  The epilogue transposes the accumulators through the (then dead) halo
// region, 32 channels at a time, so that stores / residual loads are 16 B per lane and 128 B contiguous per pixel.
// No atomics and a fixed summation order (tap 0..8, channels ascending inside a tap) for every pixel, whatever the launch: two runs give the same bits and an image's
// result does not depend on how many images the launch has.
#pragma once
#include <stdlib.h>

#include "lfsr_internal.h"

typedef float f32x16h __attribute__((ext_vector_type(16)));
typedef unsigned u32x4h __attribute__((ext_vector_type(4)));

namespace {

constexpr int TR = 8, TC = 32;
constexpr int ROWB = 144;                                     // LDS bytes per row of 64 bf16
constexpr int HALO_PIX = (TR + 2) * (TC + 2);                 // 340
constexpr int SA_BYTES = HALO_PIX * ROWB;                     // 48960
constexpr int SW_BYTES = 9 * 64 * ROWB;                       // 82944
constexpr int SMEM_BYTES = SA_BYTES + SW_BYTES;               // 131904
constexpr int OROW = 36;                                      // floats per pixel row of the epilogue's transposition region (32 channels + 4)
static_assert(8 * 32 * OROW * 4 <= SA_BYTES, "the transposition region lives inside the halo");

struct ConvB16Args {
  const float* X; int x_stride; int x_choff;
  const float* Wp;  // [9][64][64] fp32 (tap, n, k)
  float* Y; int y_stride; int y_choff;
  const float* R1; int r1_stride; int r1_choff;
  const float* R2; int r2_stride; int r2_choff;
  int n_img, H, W, tiles_y, tiles_x, ntiles;
  float slope;
  const float* Mk; int mk_stride; int mk_choff; float mk_slope;   // MASK only: y = conv * (mk > 0 ? 1 : mk_slope) + r1 + r2
};

// two fp32 -> one register of two bf16, round to nearest even, element 0 in the low half (MFMA operand order)
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ uint2 cvt4(const float4 v) { return make_uint2(cvt_pk_bf16(v.x, v.y), cvt_pk_bf16(v.z, v.w)); }
// asm MFMA, accumulator tied (rowgemm_b3.hip, b3_mfma: why not the builtin)
__device__ __forceinline__ void h_mfma(f32x16h& c, const u32x4h a, const u32x4h b) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
// MFMA results -> VALU reads: the wait the compiler would insert for a builtin (tied to the accumulator so it stays between the two)
__device__ __forceinline__ void h_settle(f32x16h& c) { asm volatile("s_nop 15\n\ts_nop 15" : "+v"(c)); }

template <bool MASK>
__global__ __launch_bounds__(512) void k_conv3x3_bf16(ConvB16Args p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_b16[];
  unsigned char* sA = smem_b16;                 // halo [340][ROWB]
  unsigned char* sW = smem_b16 + SA_BYTES;      // weights [9 * 64][ROWB]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c16 = tid & 15;
  const int half = lane >> 5, l31 = lane & 31;

  // per-thread halo slots: slot i covers (pixel, 4-channel chunk) = (tid + 512 i) >> 4, tid & 15
  int hoff[11];
#pragma unroll
  for (int i = 0; i < 11; ++i) {
    int pix = (tid + i * 512) >> 4;
    hoff[i] = pix < HALO_PIX ? pix : -1;
  }
  auto tile_origin = [&](int t, int& img, int& y0, int& x0) {
    int tx = t % p.tiles_x; int q = t / p.tiles_x;
    int ty = q % p.tiles_y; img = q / p.tiles_y;
    y0 = ty * TR; x0 = tx * TC;
  };
  auto halo_load = [&](int i, int img, int y0, int x0) -> float4 {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    int pix = hoff[i];
    if (pix >= 0) {
      int r = pix / (TC + 2), c = pix - r * (TC + 2);
      int yy = y0 + r - 1, xx = x0 + c - 1;
      if (yy >= 0 && yy < p.H && xx >= 0 && xx < p.W)
        v = *reinterpret_cast<const float4*>(p.X + ((long long)img * p.H * p.W + (long long)yy * p.W + xx) * p.x_stride + p.x_choff + c16 * 4);
    }
    return v;
  };

  int tile = (int)blockIdx.x;
  int img, y0, x0;
  tile_origin(tile, img, y0, x0);
  float4 hv[11];   // a tile's halo as loaded ...
  uint2 hb[11];    // ... and as bf16, converted BEFORE the previous tile's output stores are issued: the write to LDS at the top of the loop then waits for no
                   // memory counter, and those stores stay in flight over the seam (a wait for hv there would be a wait for every older store as well)
#pragma unroll
  for (int i = 0; i < 11; ++i) hv[i] = halo_load(i, img, y0, x0);
#pragma unroll
  for (int i = 0; i < 11; ++i) hb[i] = cvt4(hv[i]);

  // the whole weight, fp32 [576][64] -> bf16 rows in LDS, once per block: 9216 chunks of 4 floats, 18 per thread
#pragma unroll
  for (int i = 0; i < 18; ++i) {
    const int idx = tid + i * 512;
    const float4 wv = *reinterpret_cast<const float4*>(p.Wp + (long long)idx * 4);
    *reinterpret_cast<uint2*>(sW + (idx >> 4) * ROWB + (idx & 15) * 8) = cvt4(wv);
  }

  // fragment addresses: lane (r = l31, h = half) holds A[pixel r][k = 8h + j] and B[k = 8h + j][channel r] of a 16-channel K step: 16 B at chunk 2 s + h of a row
  const unsigned char* aBase = sA + ((wave + 1) * (TC + 2) + (l31 + 1)) * ROWB + 16 * half;   // tap (0,0) position
  const unsigned char* bBase = sW + l31 * ROWB + 16 * half;
  float* sO = reinterpret_cast<float*>(sA) + wave * 32 * OROW;   // epilogue transposition region (wave-private, inside the dead halo)
  const int ech = lane & 7, epx = lane >> 3;                    // epilogue: 4-channel chunk inside a 32-channel half, pixel inside a group of 8

  while (true) {
    // ---- registers -> LDS: this tile's halo as bf16 ---------------------------------------------------
#pragma unroll
    for (int i = 0; i < 11; ++i)
      if (hoff[i] >= 0) *reinterpret_cast<uint2*>(sA + hoff[i] * ROWB + c16 * 8) = hb[i];
    // LDS-only barrier: the previous tile's output stores stay in flight (a __syncthreads would drain vmcnt)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    const int next = tile + (int)gridDim.x;
    const bool has_next = next < p.ntiles;
    int nimg = 0, ny0 = 0, nx0 = 0;
    if (has_next) {   // the next tile's halo: in flight during the whole MFMA stream
      tile_origin(next, nimg, ny0, nx0);
#pragma unroll
      for (int i = 0; i < 11; ++i) hv[i] = halo_load(i, nimg, ny0, nx0);
    }
    const int yy = y0 + wave;
    const long long row_base = (long long)img * p.H * p.W + (long long)yy * p.W + x0;
    float4 res[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {   // i >> 2: 32-channel half, i & 3: pixel group
      const int pc = epx + 8 * (i & 3);
      res[i] = (p.R1 && yy < p.H && x0 + pc < p.W) ? *reinterpret_cast<const float4*>(p.R1 + (row_base + pc) * p.r1_stride + p.r1_choff + (i >> 2) * 32 + ech * 4)
                                                   : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float4 msk[MASK ? 8 : 1];   // the saved activation at the output positions, with the residual's access; turned into the factor before the first store
    if constexpr (MASK) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int pc = epx + 8 * (i & 3);
        msk[i] = (yy < p.H && x0 + pc < p.W) ? *reinterpret_cast<const float4*>(p.Mk + (row_base + pc) * p.mk_stride + p.mk_choff + (i >> 2) * 32 + ech * 4)
                                             : make_float4(1.f, 1.f, 1.f, 1.f);
      }
    }

    f32x16h acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    asm volatile("s_nop 1" : "+v"(acc0), "+v"(acc1));   // VALU writes of the accumulators -> the first MFMAs' SrcC: the wait states the compiler pads for a builtin
    // MFMA stream: 36 steps (tap, s) of one A fragment, two B fragments and two MFMAs; the fragments of step n + 1 are requested before the MFMAs of step n issue
    u32x4h fa = *reinterpret_cast<const u32x4h*>(aBase + (-(TC + 2) - 1) * ROWB);
    u32x4h fb0 = *reinterpret_cast<const u32x4h*>(bBase);
    u32x4h fb1 = *reinterpret_cast<const u32x4h*>(bBase + 32 * ROWB);
#pragma unroll
    for (int n = 0; n < 36; ++n) {
      u32x4h na = fa, nb0 = fb0, nb1 = fb1;
      if (n < 35) {
        const int tap = (n + 1) >> 2, s = (n + 1) & 3;
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const unsigned char* aT = aBase + (dy * (TC + 2) + dx) * ROWB + s * 32;
        const unsigned char* bT = bBase + tap * 64 * ROWB + s * 32;
        na = *reinterpret_cast<const u32x4h*>(aT);
        nb0 = *reinterpret_cast<const u32x4h*>(bT);
        nb1 = *reinterpret_cast<const u32x4h*>(bT + 32 * ROWB);
      }
      h_mfma(acc0, fa, fb0);
      h_mfma(acc1, fa, fb1);
      fa = na; fb0 = nb0; fb1 = nb1;
    }
    h_settle(acc0);
    h_settle(acc1);
    // all waves are done reading the halo before the epilogue reuses the region (LDS-only: the halo prefetch stays in flight)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // every load of this iteration is consumed here, before the first output store: no wait behind a store in the epilogue or at the seam
    if (has_next) {
#pragma unroll
      for (int i = 0; i < 11; ++i) hb[i] = cvt4(hv[i]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(res[i].x), "+v"(res[i].y), "+v"(res[i].z), "+v"(res[i].w));
    if constexpr (MASK) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        msk[i].x = msk[i].x > 0.f ? 1.f : p.mk_slope; msk[i].y = msk[i].y > 0.f ? 1.f : p.mk_slope;
        msk[i].z = msk[i].z > 0.f ? 1.f : p.mk_slope; msk[i].w = msk[i].w > 0.f ? 1.f : p.mk_slope;
        asm volatile("" : "+v"(msk[i].x), "+v"(msk[i].y), "+v"(msk[i].z), "+v"(msk[i].w));
      }
    }

    // ---- epilogue: accumulators -> LDS [pixel][32 channels] -> 16-B stores (128 B contiguous per pixel), one 32-channel half at a time ----
    // C/D layout: channel n = lane & 31 (+32 for acc1), pixel column = (reg & 3) + 8 * (reg >> 2) + 4 * half
#pragma unroll
    for (int nh = 0; nh < 2; ++nh) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int pc = (r & 3) + 8 * (r >> 2) + 4 * half;
        float v = nh ? acc1[r] : acc0[r];
        v = v >= 0.f ? v : v * p.slope;
        sO[pc * OROW + l31] = v;
      }
      __builtin_amdgcn_wave_barrier();
      if (yy < p.H) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int pc = epx + 8 * i;
          if (x0 + pc < p.W) {
            float4 v = *reinterpret_cast<const float4*>(sO + pc * OROW + ech * 4);
            const long long pix = row_base + pc;
            const int ch = nh * 32 + ech * 4;
            if constexpr (MASK) { const float4 m = msk[nh * 4 + i]; v.x *= m.x; v.y *= m.y; v.z *= m.z; v.w *= m.w; }
            if (p.R1) { const float4 r = res[nh * 4 + i]; v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w; }
            if (p.R2) {
              const float4 r = *reinterpret_cast<const float4*>(p.R2 + pix * p.r2_stride + p.r2_choff + ch);
              v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
            }
            *reinterpret_cast<float4*>(p.Y + pix * p.y_stride + p.y_choff + ch) = v;
          }
        }
      }
      __builtin_amdgcn_wave_barrier();   // the region is rewritten by the second half
    }
    if (!has_next) break;
    // every wave is done with its sO reads before the halo region is overwritten (LDS-only barrier, stores keep flying)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    tile = next; img = nimg; y0 = ny0; x0 = nx0;
  }
}

template <bool MASK>
int conv3x3_bf16_launch_t(const LfsrConv3& c, hipStream_t st) {
  if (MASK != (c.mk != nullptr)) return LFSR_E_ARG;
  static std::atomic<bool> attr_set[64];   // per device: the >64 KB dynamic-LDS opt-in is a per-device function attribute
  static std::atomic<int> cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return LFSR_E_ARG;
  if (!attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_conv3x3_bf16<MASK>), hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_BYTES);
    if (e != hipSuccess) return LFSR_HIP_ERR(e);
    attr_set[dev] = true;
  }
  if (!cus[dev]) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus[dev] = v; else cus[dev] = 256;
  }
  ConvB16Args p{};
  p.X = c.x; p.x_stride = c.x_stride; p.x_choff = c.x_choff; p.Wp = c.w_direct();
  p.Y = c.y; p.y_stride = c.y_stride; p.y_choff = c.y_choff;
  p.R1 = c.r1; p.r1_stride = c.r1_stride; p.r1_choff = c.r1_choff; p.R2 = c.r2; p.r2_stride = c.r2_stride; p.r2_choff = c.r2_choff;
  if (!p.R1 && p.R2) { p.R1 = p.R2; p.r1_stride = p.r2_stride; p.r1_choff = p.r2_choff; p.R2 = nullptr; }   // a lone residual is the first (prefetched) operand
  p.Mk = c.mk; p.mk_stride = c.mk_stride; p.mk_choff = c.mk_choff; p.mk_slope = c.mk_slope;
  p.n_img = c.n_img; p.H = c.h; p.W = c.w; p.tiles_y = (c.h + TR - 1) / TR; p.tiles_x = (c.w + TC - 1) / TC; p.slope = c.slope;
  const long long ntiles = (long long)c.n_img * p.tiles_y * p.tiles_x;
  if (ntiles <= 0 || ntiles > 0x7fffffffLL - 65536) return LFSR_E_ARG;   // (tile + grid stays an int)
  p.ntiles = (int)ntiles;
  // persistent: one block per CU walks tiles blockIdx.x, + grid, ... (uniform cost, no queue needed)
  const int ncu = cus[dev];
  const unsigned grid = (unsigned)(ntiles < ncu ? ntiles : ncu);
  hipLaunchKernelGGL(k_conv3x3_bf16<MASK>, dim3(grid), dim3(512), SMEM_BYTES, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

}  // namespace
