// lfsr_conv3x3_wide_fwd under lfsr_set_wide_arithmetic(LFSR_WIDE_ARITH_BF16): LF_InterNet's wide per-view 3x3 convs (SpaConvSq 128 -> 64, SpaBottle 320 -> 64;
// zero pad 1, VCL rows) on bf16 OPERANDS.  Activations and weights are rounded to bf16 once (v_cvt_pk_bf16_f32: nearest even), the products are exact and run on
// v_mfma_f32_32x32x16_bf16; accumulation, LeakyReLU, the residual add and the stores are fp32; tensors stay fp32 in memory and the weight is the fp32 gather-GEMM
// pack [9][64][CIN] (no new pack, no workspace).
//
// The structure is conv3x3_bf16_kernel.h's (copied, not shared: k_conv3x3_bf16 is untouched): one persistent 512-thread block per CU walks 8-row x 32-column tiles;
// wave w owns image row w of the tile x all 64 output channels (two 32 x 32 accumulators); the halo is staged as bf16 rows padded to 144 B and the nine taps read
// it at shifted addresses; the epilogue is transposed through the dead halo so that stores and residual loads are 16 B a lane.
// What differs: 128 or 320 input channels do not fit LDS at once (48 960 B of halo and 82 944 B of weight per 64 channels), so a tile runs CIN / 64 STEPS, one per
// 64-channel chunk, with the accumulators kept in registers across them.  A step stages its chunk of the halo AND its chunk [9][64][64] of the weight (131 904 B
// together, one block a CU), runs the 72 MFMAs of conv3x3_bf16_kernel.h between two LDS-only barriers, and meanwhile holds the NEXT step's halo and weight chunk in
// flight in registers (116 VGPRs of a 256-register budget at two waves a SIMD), weight first.  The weight chunk is therefore re-read from L2 once per tile and chunk
// (147 KB against 87 KB of halo): the price of keeping the pack as it is.  Every prefetch address is a uniform 64-bit base plus a 32-bit lane offset recomputed at its
// use: the compiler spills around the MFMA stream, and a spilled address comes back through the same counter as the loads in flight (profiles/wide_bf16_time.md).
// Summation order, fixed for every output whatever n_img and the tile: chunk 0 .. CIN / 64 - 1, inside a chunk tap 0 .. 8, inside a tap channels ascending.  No
// atomics: two runs give the same bits and an image's result does not depend on the batch.
#include <stdlib.h>

#include "lfsr_internal.h"

typedef float f32x16w __attribute__((ext_vector_type(16)));
typedef unsigned u32x4w __attribute__((ext_vector_type(4)));

namespace {

constexpr int TR = 8, TC = 32;
constexpr int ROWB = 144;                                     // LDS bytes per row of 64 bf16
constexpr int HALO_PIX = (TR + 2) * (TC + 2);                 // 340
constexpr int SA_BYTES = HALO_PIX * ROWB;                     // 48960
constexpr int SW_BYTES = 9 * 64 * ROWB;                       // 82944
constexpr int SMEM_BYTES = SA_BYTES + SW_BYTES;               // 131904 (<= 160 KiB)
constexpr int OROW = 36;                                      // floats per pixel row of the epilogue's transposition region (32 channels + 4)
static_assert(8 * 32 * OROW * 4 <= SA_BYTES, "the transposition region lives inside the halo");
static_assert(SMEM_BYTES <= 160 * 1024, "one CU's LDS");

struct WideArgs {
  const float* X; int x_stride; int x_choff;
  const float* Wp;  // [9][64][CIN] fp32 (tap, n, k)
  float* Y; int y_stride; int y_choff;
  const float* R1; int r1_stride; int r1_choff;
  int n_img, H, W, tiles_y, tiles_x, ntiles;
  float slope;
};

// two fp32 -> one register of two bf16, round to nearest even, element 0 in the low half (MFMA operand order)
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ uint2 cvt4(const float4 v) { return make_uint2(cvt_pk_bf16(v.x, v.y), cvt_pk_bf16(v.z, v.w)); }
// asm MFMA, accumulator tied (rowgemm_b3.hip, b3_mfma: why not the builtin)
__device__ __forceinline__ void w_mfma(f32x16w& c, const u32x4w a, const u32x4w b) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
// MFMA results -> VALU reads: the wait the compiler would insert for a builtin (tied to the accumulator so it stays between the two)
__device__ __forceinline__ void w_settle(f32x16w& c) { asm volatile("s_nop 15\n\ts_nop 15" : "+v"(c)); }

template <int CIN>
__global__ __launch_bounds__(512) void k_conv3x3_wide_bf16(WideArgs p) {
  constexpr int NCH = CIN / 64;
  static_assert(CIN % 64 == 0, "whole 64-channel chunks");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_wide[];
  unsigned char* sA = smem_wide;                 // halo chunk [340][ROWB]
  unsigned char* sW = smem_wide + SA_BYTES;      // weight chunk [9 * 64][ROWB]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c16 = tid & 15;
  const int half = lane >> 5, l31 = lane & 31;

  // per-thread halo slots: slot i covers (pixel, 4-channel group) = (tid + 512 i) >> 4, tid & 15; the last slot reaches past the 340 pixels.  A slot's row and
  // column are recomputed at every use from `t`, the thread index behind an empty asm the compiler cannot hoist across: hoisted, the eleven slots' invariants
  // spilled, and a spilled value is reloaded through the counter the loads in flight return on -- every prefetch load then waited for the one before it
  auto tile_origin = [&](int t, int& img, int& y0, int& x0) {
    int tx = t % p.tiles_x; int q = t / p.tiles_x;
    int ty = q % p.tiles_y; img = q / p.tiles_y;
    y0 = ty * TR; x0 = tx * TC;
  };
  auto halo_load = [&](int i, int t, int img, int y0, int x0, int ch) -> float4 {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    const int pix = (t >> 4) + 32 * i;
    if (pix < HALO_PIX) {
      int r = pix / (TC + 2), c = pix - r * (TC + 2);
      int yy = y0 + r - 1, xx = x0 + c - 1;
      if (yy >= 0 && yy < p.H && xx >= 0 && xx < p.W) {
        // a uniform 64-bit base (scalar registers) + a 32-bit lane offset (the launcher's operand span is below 2 GiB): one address register a slot, where
        // 64-bit lane addresses spilled, and a spilled address is reloaded through the counter the loads in flight return on
        const char* base = reinterpret_cast<const char*>(p.X) + ((long long)img * p.H * p.W * p.x_stride + p.x_choff + ch * 64) * 4;
        const unsigned off = (unsigned)((yy * p.W + xx) * p.x_stride + (t & 15) * 4) * 4u;
        v = *reinterpret_cast<const float4*>(base + off);
      }
    }
    return v;
  };
  // weight slot i covers (row = tap * 64 + n, 4-channel group) = (tid + 512 i) >> 4, tid & 15 of chunk ch: 9216 groups, 18 per thread
  auto weight_load = [&](int i, int t, int ch) -> float4 {
    const char* base = reinterpret_cast<const char*>(p.Wp) + (long long)(i * 32 * CIN + ch * 64) * 4;   // uniform
    return *reinterpret_cast<const float4*>(base + (unsigned)((t >> 4) * CIN + (t & 15) * 4) * 4u);
  };

  int tile = (int)blockIdx.x, ch = 0;
  int img, y0, x0;
  tile_origin(tile, img, y0, x0);
  float4 hv[11], wv[18];   // a step's halo and weight chunk as loaded ...
  uint2 hb[11], wb[18];    // ... and as bf16, converted BEFORE the previous tile's output stores are issued (conv3x3_bf16_kernel.h: the write to LDS at the top of
                           // the loop then waits for no memory counter)
#pragma unroll
  for (int i = 0; i < 11; ++i) hv[i] = halo_load(i, tid, img, y0, x0, 0);
#pragma unroll
  for (int i = 0; i < 18; ++i) wv[i] = weight_load(i, tid, 0);
#pragma unroll
  for (int i = 0; i < 11; ++i) hb[i] = cvt4(hv[i]);
#pragma unroll
  for (int i = 0; i < 18; ++i) wb[i] = cvt4(wv[i]);

  // fragment addresses: lane (r = l31, h = half) holds A[pixel r][k = 8h + j] and B[k = 8h + j][channel r] of a 16-channel K step: 16 B at chunk 2 s + h of a row
  const unsigned char* aBase = sA + ((wave + 1) * (TC + 2) + (l31 + 1)) * ROWB + 16 * half;   // tap (0,0) position
  const unsigned char* bBase = sW + l31 * ROWB + 16 * half;
  float* sO = reinterpret_cast<float*>(sA) + wave * 32 * OROW;   // epilogue transposition region (wave-private, inside the dead halo)
  const int ech = lane & 7, epx = lane >> 3;                    // epilogue: 4-channel group inside a 32-channel half, pixel inside a group of 8

  f32x16w acc0, acc1;
  while (true) {
    // ---- registers -> LDS: this step's halo and weight chunks as bf16 ----------------------------------
#pragma unroll
    for (int i = 0; i < 11; ++i)
      if ((tid >> 4) + 32 * i < HALO_PIX) *reinterpret_cast<uint2*>(sA + ((tid >> 4) + 32 * i) * ROWB + c16 * 8) = hb[i];
#pragma unroll
    for (int i = 0; i < 18; ++i) *reinterpret_cast<uint2*>(sW + ((tid >> 4) + 32 * i) * ROWB + c16 * 8) = wb[i];
    // LDS-only barrier: the previous tile's output stores stay in flight (a __syncthreads would drain vmcnt)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // the next step: the next chunk of this tile, or chunk 0 of the block's next tile
    const bool last_ch = ch == NCH - 1;
    const int ntile = last_ch ? tile + (int)gridDim.x : tile, nch = last_ch ? 0 : ch + 1;
    const bool has_next = ntile < p.ntiles;
    int nimg = img, ny0 = y0, nx0 = x0;
    if (has_next) {   // its halo and weight chunks: in flight during the whole MFMA stream
      if (last_ch) tile_origin(ntile, nimg, ny0, nx0);
      int t = tid;
      asm volatile("" : "+v"(t));
#pragma unroll
      for (int i = 0; i < 18; ++i) wv[i] = weight_load(i, t, nch);
#pragma unroll
      for (int i = 0; i < 11; ++i) hv[i] = halo_load(i, t, nimg, ny0, nx0, nch);
    }
    const int yy = y0 + wave;
    const long long row_base = (long long)img * p.H * p.W + (long long)yy * p.W + x0;

    if (ch == 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    }
    asm volatile("s_nop 1" : "+v"(acc0), "+v"(acc1));   // VALU writes of the accumulators -> the first MFMAs' SrcC: the wait states the compiler pads for a builtin
    // MFMA stream: 36 steps (tap, s) of one A fragment, two B fragments and two MFMAs; the fragments of step n + 1 are requested before the MFMAs of step n issue
    u32x4w fa = *reinterpret_cast<const u32x4w*>(aBase + (-(TC + 2) - 1) * ROWB);
    u32x4w fb0 = *reinterpret_cast<const u32x4w*>(bBase);
    u32x4w fb1 = *reinterpret_cast<const u32x4w*>(bBase + 32 * ROWB);
#pragma unroll
    for (int n = 0; n < 36; ++n) {
      u32x4w na = fa, nb0 = fb0, nb1 = fb1;
      if (n < 35) {
        const int tap = (n + 1) >> 2, s = (n + 1) & 3;
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const unsigned char* aT = aBase + (dy * (TC + 2) + dx) * ROWB + s * 32;
        const unsigned char* bT = bBase + tap * 64 * ROWB + s * 32;
        na = *reinterpret_cast<const u32x4w*>(aT);
        nb0 = *reinterpret_cast<const u32x4w*>(bT);
        nb1 = *reinterpret_cast<const u32x4w*>(bT + 32 * ROWB);
      }
      w_mfma(acc0, fa, fb0);
      w_mfma(acc1, fa, fb1);
      fa = na; fb0 = nb0; fb1 = nb1;
    }
    w_settle(acc0);
    w_settle(acc1);
    // all waves are done reading both chunks before either region is rewritten (LDS-only: the prefetch stays in flight)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // the prefetch is consumed here, before the first output store (no wait behind a store at the seam), and before the residual is requested: its 116
    // registers are free again by then
    if (has_next) {
#pragma unroll
      for (int i = 0; i < 11; ++i) hb[i] = cvt4(hv[i]);
#pragma unroll
      for (int i = 0; i < 18; ++i) wb[i] = cvt4(wv[i]);
    }
    __builtin_amdgcn_sched_barrier(0);
    // the residual is requested only now, not across the MFMA stream; in the model it is the chunk-0 half of rows this block staged a step ago, an L2 hit whose
    // latency the first transposition covers
    float4 res[8];
    if (last_ch) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {   // i >> 2: 32-channel half, i & 3: pixel group
        const int pc = epx + 8 * (i & 3);
        res[i] = (p.R1 && yy < p.H && x0 + pc < p.W) ? *reinterpret_cast<const float4*>(p.R1 + (row_base + pc) * p.r1_stride + p.r1_choff + (i >> 2) * 32 + ech * 4)
                                                     : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }

    if (last_ch) {
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
              if (p.R1) { const float4 r = res[nh * 4 + i]; v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w; }
              *reinterpret_cast<float4*>(p.Y + (row_base + pc) * p.y_stride + p.y_choff + nh * 32 + ech * 4) = v;
            }
          }
        }
        __builtin_amdgcn_wave_barrier();   // the region is rewritten by the second half
      }
      if (!has_next) break;
      // every wave is done with its sO reads before the halo region is overwritten (LDS-only barrier, stores keep flying)
      asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    tile = ntile; ch = nch; img = nimg; y0 = ny0; x0 = nx0;
  }
}

template <int CIN>
int wide_launch_t(const float* x, int x_stride, int x_choff, const float* w_packed, float* y, int y_stride, int y_choff, const float* r1, int r1_stride,
                  int r1_choff, int n_img, int h, int w, float slope, hipStream_t st) {
  static std::atomic<bool> attr_set[64];   // per device: the >64 KB dynamic-LDS opt-in is a per-device function attribute
  static std::atomic<int> cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return LFSR_E_ARG;
  if (!attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_conv3x3_wide_bf16<CIN>), hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_BYTES);
    if (e != hipSuccess) return LFSR_HIP_ERR(e);
    attr_set[dev] = true;
  }
  if (!cus[dev]) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus[dev] = v; else cus[dev] = 256;
  }
  WideArgs p{};
  p.X = x; p.x_stride = x_stride; p.x_choff = x_choff; p.Wp = w_packed;
  p.Y = y; p.y_stride = y_stride; p.y_choff = y_choff;
  p.R1 = r1; p.r1_stride = r1_stride; p.r1_choff = r1_choff;
  p.n_img = n_img; p.H = h; p.W = w; p.tiles_y = (h + TR - 1) / TR; p.tiles_x = (w + TC - 1) / TC; p.slope = slope;
  const long long ntiles = (long long)n_img * p.tiles_y * p.tiles_x;
  if (ntiles <= 0 || ntiles > 0x7fffffffLL - 65536) return LFSR_E_ARG;   // (tile + grid stays an int)
  p.ntiles = (int)ntiles;
  // persistent: one block per CU walks tiles blockIdx.x, + grid, ... (uniform cost, no queue needed)
  const int ncu = cus[dev];
  const unsigned grid = (unsigned)(ntiles < ncu ? ntiles : ncu);
  hipLaunchKernelGGL(k_conv3x3_wide_bf16<CIN>, dim3(grid), dim3(512), SMEM_BYTES, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

}  // namespace

int lfsr_conv3x3_wide_bf16_launch(const float* x, int x_stride, int x_choff, int cin, const float* w_packed, float* y, int y_stride, int y_choff,
                                  const float* r1, int r1_stride, int r1_choff, int n_img, int h, int w, float slope, hipStream_t st) {
  if (cin == 128) return wide_launch_t<128>(x, x_stride, x_choff, w_packed, y, y_stride, y_choff, r1, r1_stride, r1_choff, n_img, h, w, slope, st);
  if (cin == 320) return wide_launch_t<320>(x, x_stride, x_choff, w_packed, y, y_stride, y_choff, r1, r1_stride, r1_choff, n_img, h, w, slope, st);
  return LFSR_E_ARG;
}
