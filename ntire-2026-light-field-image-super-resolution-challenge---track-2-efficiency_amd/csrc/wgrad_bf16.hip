// Weight gradient of the per-view 3x3 conv 64 -> 64 with bf16 OPERANDS: the kernel of lfsr_set_grad_arithmetic(LFSR_GRAD_ARITH_BF16) behind the CONV3 form of lfsr_wgrad_run (wgrad.cpp).
//   dW[tap][n][k] = sum over pixels p of dY[p][n] * X[p + shift(tap)][k]   (zero outside the view)
// dY and X are rounded to bf16 (v_cvt_pk_bf16_f32: nearest even) on their way into LDS, the products are exact and run on v_mfma_f32_32x32x16_bf16 with the PIXEL index
// as the MFMA's K, accumulation and the partial slabs are fp32.  Gradients and activations stay fp32 in memory: the mode changes arithmetic, not storage.
//
// The structure is k_wgrad_conv3_halo's (wgrad.hip): a persistent 512-thread block walks 4-row x 32-column tiles; the dY tile and the (4+2) x (32+2) X halo are staged
// once, zero-filled outside the image and on ragged edges (buffer loads with an out-of-range offset), and all 9 taps read X at shifted addresses.  Wave w owns the
// (n, k) quadrant w & 3 for taps 0-4 (w < 4) or 5-8 (w >= 4): at most 5 x 16 accumulator registers that persist across ALL tiles of the block, so each block writes ONE
// partial slab [9][64][64] at the end; lfsr_wgrad_reduce sums the slabs.  The launcher starts exactly the block count the caller sized the slabs for
// (lfsr_wgrad_conv3_blocks, never below this kernel's tile count capped the same way); a block without a tile writes a slab of zeros.  No atomics, a fixed order of
// summation: two runs give the same bits.
//
// Both MFMA operands need K = pixel contiguous per lane, the images are [pixel][64 channels] rows: ds_read_b64_tr_b16 reads, per 16-lane group, 4 pixel rows x 16
// channels and hands each lane ONE channel of the 4 pixels.  Lane (l31 = lane & 31, h = lane >> 5) of a 16-pixel K step takes pixels 8h .. 8h+3 and 8h+4 .. 8h+7 of
// channel 32 q + l31 with two such reads; lane 4q + p of a group supplies the address of pixel row q, channels 4p .. 4p+3.  A tap's shift is a different row address
// only, so the dY fragments are read once per K step and serve all taps of the wave: 2 + 2 x 5 reads per 5 MFMAs.
//   * every lane of every wave takes part in every such read (no divergent control flow around them), every address is inside the staged images (the halo is the
//     padding) and 8-B aligned;
//   * rows are padded to 192 B = 48 dwords: the 32 lanes of a half read 4 rows x 64 B, and 48 q mod 64 = 0, 48, 32, 16 tiles the 64 banks exactly, whatever the
//     common base -- conflict-free.  (The forward kernel's 144-B rows would put rows q and q + 2 of a block 8 banks apart: 2-way on half of the banks.)
// LDS: (204 + 128) x 192 B = 63 744 B.
#include <stdlib.h>

#include "lfsr_internal.h"

typedef float f32x16w __attribute__((ext_vector_type(16)));
typedef unsigned u32x4w __attribute__((ext_vector_type(4)));
typedef short s16x4w __attribute__((ext_vector_type(4)));

namespace {

constexpr int TR = 4, TC = 32;
constexpr int ROWB = 192;                          // LDS bytes per row of 64 bf16
constexpr int X_PIX = (TR + 2) * (TC + 2);         // 204
constexpr int G_PIX = TR * TC;                     // 128
constexpr int SX_BYTES = X_PIX * ROWB;
constexpr int SMEM_BYTES = (X_PIX + G_PIX) * ROWB; // 63744
static_assert(SMEM_BYTES <= 65536, "no dynamic-LDS opt-in needed");

struct WgradB16Args {
  const float* G; int g_stride; int g_choff;
  const float* X; int x_stride; int x_choff;
  float* P;               // [gridDim.x][9][64][64]
  int g_bytes, x_bytes;   // true byte spans (descriptor extents)
  int n_img, H, W, tiles_y, tiles_x, ntiles;
};

__device__ __forceinline__ unsigned w_cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ uint2 w_cvt4(const float4 v) { return make_uint2(w_cvt_pk_bf16(v.x, v.y), w_cvt_pk_bf16(v.z, v.w)); }
// asm MFMA, accumulator tied (rowgemm_b3.hip, b3_mfma: why not the builtin)
__device__ __forceinline__ void w_mfma(f32x16w& c, const u32x4w a, const u32x4w b) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
// MFMA results -> VALU / store reads: the wait the compiler would insert for a builtin
__device__ __forceinline__ void w_settle(f32x16w& c) { asm volatile("s_nop 15\n\ts_nop 15" : "+v"(c)); }
// 8 pixels x 1 channel of a [pixel][channel] image: two transposed reads, 4 pixel rows apart
__device__ __forceinline__ u32x4w tr_frag(const unsigned char* p) {
  typedef __attribute__((address_space(3))) s16x4w* lds_ptr;
  const s16x4w lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p));
  const s16x4w hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p + 4 * ROWB));
  const uint2 l = __builtin_bit_cast(uint2, lo), h = __builtin_bit_cast(uint2, hi);
  return u32x4w{l.x, l.y, h.x, h.y};
}

template <int T0, int NTAP>   // the wave's taps T0 .. T0 + NTAP - 1
__device__ __forceinline__ void wgrad_b16_body(const WgradB16Args& p, unsigned char* smem, const int q) {
  unsigned char* sX = smem;                 // halo [204][ROWB]
  unsigned char* sG = smem + SX_BYTES;      // dY tile [128][ROWB]
  const int tid = threadIdx.x, lane = tid & 63;
  const int c16 = tid & 15, r16 = tid >> 4;
  const int half = lane >> 5, l31 = lane & 31;
  const int nq = q >> 1, kq = q & 1;

  f32x16w acc[NTAP];
#pragma unroll
  for (int t = 0; t < NTAP; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll
  for (int t = 0; t < NTAP; ++t) asm volatile("s_nop 1" : "+v"(acc[t]));   // VALU writes of the accumulators -> the first MFMAs' SrcC

  // tile loads through buffer descriptors with 32-bit offsets (the caller checks the spans): image borders and ragged edges are out-of-range offsets that read as zero
  typedef float f32x4w __attribute__((ext_vector_type(4)));
  constexpr int WOOB = (int)0x80000000u;
  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.G), 0, p.g_bytes, 0x00020000);
  float4 hx[7], hg[4];
  auto load_tile = [&](int tile) {
    int tx = tile % p.tiles_x; int qq = tile / p.tiles_x;
    int ty = qq % p.tiles_y; int img = qq / p.tiles_y;
    const int y0 = ty * TR, x0 = tx * TC;
    const int ib = img * p.H * p.W;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const int pix = r16 + 32 * i;
      const int r = pix / (TC + 2), c = pix - r * (TC + 2);
      const int yy = y0 + r - 1, xx = x0 + c - 1;
      const bool ok = pix < X_PIX && (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W;
      const f32x4w v = __builtin_bit_cast(f32x4w, __builtin_amdgcn_raw_buffer_load_b128(rsX, ok ? ((ib + yy * p.W + xx) * p.x_stride + p.x_choff + c16 * 4) * 4 : WOOB, 0, 0));
      hx[i] = make_float4(v.x, v.y, v.z, v.w);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pix = r16 + 32 * i;
      const int r = pix / TC, c = pix - r * TC;
      const int yy = y0 + r, xx = x0 + c;
      const bool ok = yy < p.H && xx < p.W;
      const f32x4w v = __builtin_bit_cast(f32x4w, __builtin_amdgcn_raw_buffer_load_b128(rsG, ok ? ((ib + yy * p.W + xx) * p.g_stride + p.g_choff + c16 * 4) * 4 : WOOB, 0, 0));
      hg[i] = make_float4(v.x, v.y, v.z, v.w);
    }
  };

  // fragment addresses (see the head of the file): row 8h + q4 of a K step's 16 pixels, channels 32 quadrant + 16 group + 4 p4
  const int q4 = (lane & 15) >> 2, p4 = lane & 3, g16 = (lane >> 4) & 1;
  const unsigned char* gBase = sG + (8 * half + q4) * ROWB + (32 * nq + 16 * g16 + 4 * p4) * 2;
  const unsigned char* xBase = sX + ((TC + 2) + 1 + 8 * half + q4) * ROWB + (32 * kq + 16 * g16 + 4 * p4) * 2;   // tap (0,0) position of tile pixel (0,0)
  constexpr int KSTEPS = G_PIX / 16;   // 8: K step s covers tile row s >> 1, columns 16 (s & 1) ..
  auto frags = [&](int s, u32x4w& fa, u32x4w (&fb)[NTAP]) {
    const int r = s >> 1, cb = (s & 1) * 16;
    fa = tr_frag(gBase + (r * TC + cb) * ROWB);
#pragma unroll
    for (int t = 0; t < NTAP; ++t) {
      const int tap = T0 + t, dy = tap / 3 - 1, dx = tap % 3 - 1;
      fb[t] = tr_frag(xBase + ((r + dy) * (TC + 2) + cb + dx) * ROWB);
    }
  };

  int tile = blockIdx.x;
  if (tile < p.ntiles) load_tile(tile);
  for (; tile < p.ntiles; tile += gridDim.x) {
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const int pix = r16 + 32 * i;
      if (pix < X_PIX) *reinterpret_cast<uint2*>(sX + pix * ROWB + c16 * 8) = w_cvt4(hx[i]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<uint2*>(sG + (r16 + 32 * i) * ROWB + c16 * 8) = w_cvt4(hg[i]);
    __syncthreads();
    if (tile + (int)gridDim.x < p.ntiles) load_tile(tile + gridDim.x);     // next tile flies under this tile's MFMAs
    // the fragments of K step s + 1 are requested before the MFMAs of step s issue
    u32x4w fa, fb[NTAP];
    frags(0, fa, fb);
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      u32x4w na = fa, nb[NTAP];
#pragma unroll
      for (int t = 0; t < NTAP; ++t) nb[t] = fb[t];
      if (s + 1 < KSTEPS) frags(s + 1, na, nb);
#pragma unroll
      for (int t = 0; t < NTAP; ++t) w_mfma(acc[t], fa, fb[t]);
      fa = na;
#pragma unroll
      for (int t = 0; t < NTAP; ++t) fb[t] = nb[t];
    }
    __syncthreads();   // every wave is done reading before the images are overwritten
  }
  // D[row = n][col = k]: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
  for (int t = 0; t < NTAP; ++t) w_settle(acc[t]);
  float* out = p.P + (long long)blockIdx.x * 9 * 64 * 64;
#pragma unroll
  for (int t = 0; t < NTAP; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = nq * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
      out[((long long)(T0 + t) * 64 + n) * 64 + kq * 32 + l31] = acc[t][r];
    }
  }
}

__global__ __launch_bounds__(512) void k_wgrad_conv3_bf16(WgradB16Args p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_wb16[];
  const int wave = threadIdx.x >> 6;
  const int q = __builtin_amdgcn_readfirstlane(wave & 3), hi = __builtin_amdgcn_readfirstlane(wave >> 2);
  if (hi == 0) wgrad_b16_body<0, 5>(p, smem_wb16, q);
  else wgrad_b16_body<5, 4>(p, smem_wb16, q);
}

}  // namespace

int lfsr_wgrad_conv3_bf16_launch(const LfsrWgrad& g, hipStream_t st) {
  const int n_img = g.n_img(), h = g.h, w = g.w;
  if (!g.G || !g.X || !g.part || n_img <= 0 || h <= 0 || w <= 0 || ((g.g_stride | g.g_choff | g.x_stride | g.x_choff) & 3)) return LFSR_E_ARG;
  if (g.g_stride < g.g_choff + 64 || g.x_stride < g.x_choff + 64) return LFSR_E_ARG;
  if ((long long)n_img * h * w * (g.x_stride > g.g_stride ? g.x_stride : g.g_stride) * 4 >= (1LL << 31)) return LFSR_E_ARG;   // 32-bit byte offsets
  WgradB16Args p{};
  p.G = g.G; p.g_stride = g.g_stride; p.g_choff = g.g_choff; p.X = g.X; p.x_stride = g.x_stride; p.x_choff = g.x_choff; p.P = g.part;
  p.g_bytes = (int)((long long)n_img * h * w * g.g_stride * 4); p.x_bytes = (int)((long long)n_img * h * w * g.x_stride * 4);
  p.n_img = n_img; p.H = h; p.W = w; p.tiles_y = (h + TR - 1) / TR; p.tiles_x = (w + TC - 1) / TC;
  p.ntiles = n_img * p.tiles_y * p.tiles_x;
  hipLaunchKernelGGL(k_wgrad_conv3_bf16, dim3((unsigned)lfsr_wgrad_conv3_blocks(n_img, h, w, false)), dim3(512), SMEM_BYTES, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}
