// Weight gradient of LF_InterNet's wide per-view 3x3 convs (SpaConvSq 128 -> 64, BottleNeck.SpaBottle 320 -> 64) with bf16 OPERANDS: the kernel of
// lfsr_set_wide_train_arithmetic(LFSR_WIDE_TRAIN_ARITH_BF16_WGRAD | LFSR_WIDE_TRAIN_ARITH_BF16) behind the WIDE3 form of lfsr_wgrad_run (wgrad.cpp).
//   dW[tap][n][k] = sum over pixels p of dY[p][n] * X[p + shift(tap)][k]   (zero outside the view),  n < 64, k < cin
// dY and X are rounded to bf16 (v_cvt_pk_bf16_f32: nearest even) on their way into LDS, the products are exact and run on v_mfma_f32_32x32x16_bf16 with the PIXEL index
// as the MFMA's K, accumulation and the partial slabs are fp32.  Gradients and activations stay fp32 in memory: the mode changes arithmetic, not storage.
//
// The structure is wgrad_bf16.hip's (read its head first: the tile walk, the transposed fragment reads and why the 192-B row pitch is conflict-free for them are the
// same here, address for address); what is new is the wide K side.  A block owns up to TWO 64-channel chunks of X: it stages the dY tile ONCE and both chunks'
// (4+2) x (32+2) halos, and every dY fragment serves the taps of both chunks (2 + 2 x 2 x 5 transposed reads per 10 MFMAs, where a 64 -> 64 call per chunk reads
// 2 + 2 x 5 per 5 and stages dY per chunk).  Wave w owns the (n, k) quadrant w & 3 of each chunk for taps 0-4 (w < 4) or 5-8 (w >= 4): at most 2 x 5 x 16 = 160
// accumulator registers that persist across ALL tiles of the block -- 8 waves a block, two a SIMD, 256 registers each, one block a CU.
// The grid is (pixel blocks, chunk pairs): one pair for cin 128, three (2 + 2 + 1 chunks) for cin 320, at most 256 / pairs pixel blocks, so at most 256 blocks.
// Block (b, g) walks tiles b, b + gridDim.x, ... and at the end writes columns [128 g, 128 g + 64 nch) of slab b of [gridDim.x][9][64][cin]: the layout
// lfsr_wgrad_reduce sums with nsplit = gridDim.x.  Every block has a tile (the grid never exceeds the tile count), every slab element is written by exactly one
// block, the block count depends on the geometry alone and there are no atomics: two runs give the same bits.
// LDS: (128 + 2 x 204) x 192 B = 102 912 B, above 64 KB: the launcher sets the dynamic-LDS attribute once per device.
// The next tile's global loads are NOT kept in flight under the MFMAs as in wgrad_bf16.hip: 2 x 7 + 4 float4 a thread beside 160 accumulators do not fit 256 registers.
#include <stdlib.h>

#include "lfsr_internal.h"

typedef float f32x16ww __attribute__((ext_vector_type(16)));
typedef unsigned u32x4ww __attribute__((ext_vector_type(4)));
typedef short s16x4ww __attribute__((ext_vector_type(4)));

namespace {

constexpr int TR = 4, TC = 32;
constexpr int ROWB = 192;                          // LDS bytes per row of 64 bf16
constexpr int X_PIX = (TR + 2) * (TC + 2);         // 204
constexpr int G_PIX = TR * TC;                     // 128
constexpr int SG_BYTES = G_PIX * ROWB;
constexpr int SX_BYTES = X_PIX * ROWB;
constexpr int MAXCH = 2;                           // 64-channel chunks of X a block owns
constexpr int SMEM_BYTES = SG_BYTES + MAXCH * SX_BYTES;   // 102912
static_assert(SMEM_BYTES <= 160 * 1024, "one block a CU");

struct WgradWideArgs {
  const float* G; int g_stride; int g_choff;
  const float* X; int x_stride; int x_choff;
  float* P;               // [gridDim.x][9][64][cin]
  int g_bytes, x_bytes;   // true byte spans (descriptor extents)
  int cin, n_img, H, W, tiles_y, tiles_x, ntiles;
};

__device__ __forceinline__ unsigned ww_cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ uint2 ww_cvt4(const float4 v) { return make_uint2(ww_cvt_pk_bf16(v.x, v.y), ww_cvt_pk_bf16(v.z, v.w)); }
// asm MFMA, accumulator tied (rowgemm_b3.hip, b3_mfma: why not the builtin)
__device__ __forceinline__ void ww_mfma(f32x16ww& c, const u32x4ww a, const u32x4ww b) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
// MFMA results -> VALU / store reads: the wait the compiler would insert for a builtin
__device__ __forceinline__ void ww_settle(f32x16ww& c) { asm volatile("s_nop 15\n\ts_nop 15" : "+v"(c)); }
// 8 pixels x 1 channel of a [pixel][channel] image: two transposed reads, 4 pixel rows apart
__device__ __forceinline__ u32x4ww ww_tr_frag(const unsigned char* p) {
  typedef __attribute__((address_space(3))) s16x4ww* lds_ptr;
  const s16x4ww lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p));
  const s16x4ww hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p + 4 * ROWB));
  const uint2 l = __builtin_bit_cast(uint2, lo), h = __builtin_bit_cast(uint2, hi);
  return u32x4ww{l.x, l.y, h.x, h.y};
}

template <int T0, int NTAP, int NCH>   // the wave's taps T0 .. T0 + NTAP - 1, the block's NCH chunks from channel ch0 on
__device__ __forceinline__ void wgrad_wide_body(const WgradWideArgs& p, unsigned char* smem, const int q, const int ch0) {
  unsigned char* sG = smem;                 // dY tile [128][ROWB]
  unsigned char* sX = smem + SG_BYTES;      // halos [NCH][204][ROWB]
  const int tid = threadIdx.x, lane = tid & 63;
  const int c16 = tid & 15, r16 = tid >> 4;
  const int half = lane >> 5, l31 = lane & 31;
  const int nq = q >> 1, kq = q & 1;

  f32x16ww acc[NCH][NTAP];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int t = 0; t < NTAP; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[c][t][r] = 0.f;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int t = 0; t < NTAP; ++t) asm volatile("s_nop 1" : "+v"(acc[c][t]));   // VALU writes of the accumulators -> the first MFMAs' SrcC

  // tile loads through buffer descriptors with 32-bit offsets (the launcher checks the spans): image borders and ragged edges are out-of-range offsets that read as zero
  typedef float f32x4ww __attribute__((ext_vector_type(4)));
  constexpr int WOOB = (int)0x80000000u;
  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.G), 0, p.g_bytes, 0x00020000);
  // global -> bf16 -> LDS, the dY tile and then the halo of every chunk (the rows are written before the barrier, the registers are free after it)
  auto stage_tile = [&](int tile) {
    const int tx = tile % p.tiles_x; const int qq = tile / p.tiles_x;
    const int ty = qq % p.tiles_y; const int img = qq / p.tiles_y;
    const int y0 = ty * TR, x0 = tx * TC;
    const int ib = img * p.H * p.W;
    float4 hg[4], hx[NCH][7];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int pix = r16 + 32 * i;
      const int r = pix / TC, c = pix - r * TC;
      const int yy = y0 + r, xx = x0 + c;
      const bool ok = yy < p.H && xx < p.W;
      const f32x4ww v = __builtin_bit_cast(f32x4ww, __builtin_amdgcn_raw_buffer_load_b128(rsG, ok ? ((ib + yy * p.W + xx) * p.g_stride + p.g_choff + c16 * 4) * 4 : WOOB, 0, 0));
      hg[i] = make_float4(v.x, v.y, v.z, v.w);
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      const int pix = r16 + 32 * i;
      const int r = pix / (TC + 2), c = pix - r * (TC + 2);
      const int yy = y0 + r - 1, xx = x0 + c - 1;
      const bool ok = pix < X_PIX && (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W;
      const int off = ok ? ((ib + yy * p.W + xx) * p.x_stride + p.x_choff + ch0 + c16 * 4) * 4 : WOOB;
#pragma unroll
      for (int c2 = 0; c2 < NCH; ++c2) {
        const f32x4ww v = __builtin_bit_cast(f32x4ww, __builtin_amdgcn_raw_buffer_load_b128(rsX, ok ? off + c2 * 256 : WOOB, 0, 0));
        hx[c2][i] = make_float4(v.x, v.y, v.z, v.w);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<uint2*>(sG + (r16 + 32 * i) * ROWB + c16 * 8) = ww_cvt4(hg[i]);
#pragma unroll
    for (int c2 = 0; c2 < NCH; ++c2)
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        const int pix = r16 + 32 * i;
        if (pix < X_PIX) *reinterpret_cast<uint2*>(sX + c2 * SX_BYTES + pix * ROWB + c16 * 8) = ww_cvt4(hx[c2][i]);
      }
  };

  // fragment addresses (wgrad_bf16.hip): row 8h + q4 of a K step's 16 pixels, channels 32 quadrant + 16 group + 4 p4
  const int q4 = (lane & 15) >> 2, p4 = lane & 3, g16 = (lane >> 4) & 1;
  const unsigned char* gBase = sG + (8 * half + q4) * ROWB + (32 * nq + 16 * g16 + 4 * p4) * 2;
  const unsigned char* xBase = sX + ((TC + 2) + 1 + 8 * half + q4) * ROWB + (32 * kq + 16 * g16 + 4 * p4) * 2;   // tap (0,0) position of tile pixel (0,0), chunk 0
  constexpr int KSTEPS = G_PIX / 16;   // 8: K step s covers tile row s >> 1, columns 16 (s & 1) ..
  constexpr int UNITS = KSTEPS * NCH;  // unit u = (K step u / NCH, chunk u % NCH): NTAP MFMAs on one dY fragment
  auto gfrag = [&](int s) { return ww_tr_frag(gBase + ((s >> 1) * TC + (s & 1) * 16) * ROWB); };
  auto xfrags = [&](int u, u32x4ww (&fb)[NTAP]) {
    const int s = u / NCH, c = u % NCH;
    const int r = s >> 1, cb = (s & 1) * 16;
#pragma unroll
    for (int t = 0; t < NTAP; ++t) {
      const int tap = T0 + t, dy = tap / 3 - 1, dx = tap % 3 - 1;
      fb[t] = ww_tr_frag(xBase + c * SX_BYTES + ((r + dy) * (TC + 2) + cb + dx) * ROWB);
    }
  };

  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    stage_tile(tile);
    __syncthreads();
    // the fragments of unit u + 1 are requested before the MFMAs of unit u issue
    u32x4ww fa = gfrag(0), fb[NTAP];
    xfrags(0, fb);
#pragma unroll
    for (int u = 0; u < UNITS; ++u) {
      u32x4ww na = fa, nb[NTAP];
#pragma unroll
      for (int t = 0; t < NTAP; ++t) nb[t] = fb[t];
      if (u + 1 < UNITS) {
        if ((u + 1) % NCH == 0) na = gfrag((u + 1) / NCH);
        xfrags(u + 1, nb);
      }
#pragma unroll
      for (int t = 0; t < NTAP; ++t) ww_mfma(acc[u % NCH][t], fa, fb[t]);
      fa = na;
#pragma unroll
      for (int t = 0; t < NTAP; ++t) fb[t] = nb[t];
    }
    __syncthreads();   // every wave is done reading before the images are overwritten
  }
  // D[row = n][col = k]: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int t = 0; t < NTAP; ++t) ww_settle(acc[c][t]);
  float* out = p.P + (long long)blockIdx.x * 9 * 64 * p.cin + ch0 + kq * 32 + l31;
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int t = 0; t < NTAP; ++t) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = nq * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
        out[((long long)(T0 + t) * 64 + n) * p.cin + c * 64] = acc[c][t][r];
      }
    }
}

__global__ __launch_bounds__(512) void k_wgrad_wide_bf16(WgradWideArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_ww16[];
  const int wave = threadIdx.x >> 6;
  const int q = __builtin_amdgcn_readfirstlane(wave & 3), hi = __builtin_amdgcn_readfirstlane(wave >> 2);
  const int ch0 = blockIdx.y * (MAXCH * 64);
  if (p.cin - ch0 >= MAXCH * 64) {
    if (hi == 0) wgrad_wide_body<0, 5, 2>(p, smem_ww16, q, ch0);
    else wgrad_wide_body<5, 4, 2>(p, smem_ww16, q, ch0);
  } else {
    if (hi == 0) wgrad_wide_body<0, 5, 1>(p, smem_ww16, q, ch0);
    else wgrad_wide_body<5, 4, 1>(p, smem_ww16, q, ch0);
  }
}

inline int chunk_pairs(int cin) { return (cin / 64 + MAXCH - 1) / MAXCH; }

}  // namespace

int lfsr_wgrad_wide_bf16_blocks(int cin, int n_img, int h, int w) {
  if ((cin != 128 && cin != 320) || n_img <= 0 || h <= 0 || w <= 0) return 0;
  const long long tiles = (long long)n_img * ((h + TR - 1) / TR) * ((w + TC - 1) / TC);
  const int cap = 256 / chunk_pairs(cin);
  return (int)(tiles < cap ? tiles : cap);
}

int lfsr_wgrad_wide_bf16_launch(const LfsrWgrad& g, hipStream_t st) {
  const int cin = g.K, n_img = g.n_img(), h = g.h, w = g.w;
  const int blocks = lfsr_wgrad_wide_bf16_blocks(cin, n_img, h, w);
  if (!g.G || !g.X || !g.part || blocks <= 0 || g.g_choff < 0 || g.x_choff < 0 || ((g.g_stride | g.g_choff | g.x_stride | g.x_choff) & 3)) return LFSR_E_ARG;
  if (g.g_stride < g.g_choff + 64 || g.x_stride < g.x_choff + cin) return LFSR_E_ARG;
  if ((long long)n_img * h * w * (g.x_stride > g.g_stride ? g.x_stride : g.g_stride) * 4 >= (1LL << 31)) return LFSR_E_ARG;   // 32-bit byte offsets
  static std::atomic<bool> attr_set[64];   // per device: the >64 KB dynamic-LDS opt-in is a per-device function attribute
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return LFSR_HIP_ERR(hipErrorInvalidDevice);
  if (!attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_wgrad_wide_bf16), hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_BYTES);
    if (e != hipSuccess) return LFSR_HIP_ERR(e);
    attr_set[dev] = true;
  }
  WgradWideArgs p{};
  p.G = g.G; p.g_stride = g.g_stride; p.g_choff = g.g_choff; p.X = g.X; p.x_stride = g.x_stride; p.x_choff = g.x_choff; p.P = g.part;
  p.g_bytes = (int)((long long)n_img * h * w * g.g_stride * 4); p.x_bytes = (int)((long long)n_img * h * w * g.x_stride * 4);
  p.cin = cin; p.n_img = n_img; p.H = h; p.W = w; p.tiles_y = (h + TR - 1) / TR; p.tiles_x = (w + TC - 1) / TC;
  p.ntiles = n_img * p.tiles_y * p.tiles_x;
  hipLaunchKernelGGL(k_wgrad_wide_bf16, dim3((unsigned)blocks, (unsigned)chunk_pairs(cin)), dim3(512), SMEM_BYTES, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}
