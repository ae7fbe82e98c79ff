// Weight gradient of a linear with bf16 OPERANDS: the kernel of lfsr_set_lin_grad_arithmetic(LFSR_LIN_GRAD_ARITH_BF16) behind the LINEAR form of lfsr_wgrad_run (wgrad.cpp).
//   dW[n][k] = sum over rows m of dY[m][n] * X[m][k]        n < cout in {64, 128, 256, 576, 1024}, k < cin in {64, 128, 256}
// dY and X are rounded to bf16 (v_cvt_pk_bf16_f32: nearest even) on their way into LDS, the products are exact and run on v_mfma_f32_32x32x16_bf16 with the ROW index m
// as the MFMA's K, accumulation and the partial slabs are fp32.  Gradients and activations stay fp32 in memory: the mode changes arithmetic, not storage.
//
// The structure is k_wgrad_conv3_bf16's (wgrad_bf16.hip) without the taps: a persistent 512-thread block walks tiles of MT rows (64, or 32 where dY and X together are
// wider than 384 columns); the dY tile [MT][CT] and the X tile [MT][cin] are staged once per tile, rows past M and dY columns past cout as zeros; the next tile's global
// loads are in flight across this tile's MFMAs.  The CT x cin outputs of a block are 32 x 32 MFMA tiles dealt to the waves as TN x TK rectangles (a wave reads TN + TK
// fragments for TN TK MFMAs): at most 8 x 16 accumulator registers that persist across ALL tiles of the block, so each block writes its rows of ONE partial slab
// [cout][cin] at the end (two where four waves already cover the outputs, (64, 64): the two wave groups take alternate K steps and each writes a slab of its own);
// lfsr_wgrad_reduce sums the slabs.  The launcher starts exactly the block count the caller sized the slabs for; a block without rows writes zeros.  No atomics, a fixed
// order of summation: two runs give the same bits.
//
// Reads of dY and X per launch.  One launch covers all cout rows.  For every shape the drivers run, and every cin = 64 shape but one, CT covers cout (576 as 640: the 64
// columns of padding are zeros in LDS, never loaded and never stored), so each row of dY and of X is read from HBM ONCE.  Register pressure (a wave holds at most eight
// tiles) tiles the rest over cout on blockIdx.y: (1024, 64) as 2 x 512, (576, 128 | 256) as 3 x 192, (1024, 128 | 256) as 4 x 256 -- dY is still read once, X once per
// cout tile.
//
// Both MFMA operands need K = row contiguous per lane, memory holds [row][channel]: ds_read_b64_tr_b16 as in wgrad_bf16.hip (that file's header: which lane supplies
// which address).  Every lane of every wave takes part in every such read (the only control flow around them is block- or wave-uniform), every address is inside the
// staged tiles and 8-B aligned.  Rows of W channels are padded to 2 W + 64 bytes: W is a multiple of 64, so the pitch is 16 or 48 dwords mod 64 and the four rows a
// 32-lane half reads (64 B each) tile the 64 banks exactly, whatever the common base -- that file's bank argument for every width here.
// LDS: MT x (2 CT + 2 cin + 128) B <= 57 344 B.
#include <stdlib.h>

#include "lfsr_internal.h"

typedef float f32x16l __attribute__((ext_vector_type(16)));
typedef unsigned u32x4l __attribute__((ext_vector_type(4)));
typedef short s16x4l __attribute__((ext_vector_type(4)));

namespace {

struct LinWgradArgs {
  const float* G; int g_stride;
  const float* X; int x_stride;
  float* P;               // [slabs][cout][cin]
  long long M;
  int cout, ntiles;
};

constexpr int lw_mt(int ct, int cin) { return ct + cin > 384 ? 32 : 64; }

__device__ __forceinline__ unsigned l_cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ uint2 l_cvt4(const float4 v) { return make_uint2(l_cvt_pk_bf16(v.x, v.y), l_cvt_pk_bf16(v.z, v.w)); }
// asm MFMA, accumulator tied (rowgemm_b3.hip, b3_mfma: why not the builtin)
__device__ __forceinline__ void l_mfma(f32x16l& c, const u32x4l a, const u32x4l b) {
  asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
// MFMA results -> VALU / store reads: the wait the compiler would insert for a builtin
__device__ __forceinline__ void l_settle(f32x16l& c) { asm volatile("s_nop 15\n\ts_nop 15" : "+v"(c)); }
// 8 rows x 1 channel of a [row][channel] tile of row pitch PITCH: two transposed reads, 4 rows apart
template <int PITCH>
__device__ __forceinline__ u32x4l l_tr_frag(const unsigned char* p) {
  typedef __attribute__((address_space(3))) s16x4l* lds_ptr;
  const s16x4l lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p));
  const s16x4l hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p + 4 * PITCH));
  const uint2 l = __builtin_bit_cast(uint2, lo), h = __builtin_bit_cast(uint2, hi);
  return u32x4l{l.x, l.y, h.x, h.y};
}

// CT: the block's dY columns (blockIdx.y * CT ..), padded to whole wave rectangles; a wave owns TN x TK tiles of 32 x 32
template <int CT, int CIN, int TN, int TK>
__global__ __launch_bounds__(512) void k_lin_wgrad_bf16(LinWgradArgs p) {
  constexpr int MT = lw_mt(CT, CIN), PG = 2 * CT + 64, PX = 2 * CIN + 64;
  constexpr int NNW = CT / 32 / TN, NKW = CIN / 32 / TK, WPG = NNW * NKW, MSPLIT = 8 / WPG, KSTEPS = MT / 16, MYSTEPS = KSTEPS / MSPLIT;
  constexpr int G4 = CT / 4, X4 = CIN / 4, NLG = MT * G4 / 512, NLX = MT * X4 / 512;
  static_assert(CT % (32 * TN) == 0 && CIN % (32 * TK) == 0 && WPG * MSPLIT == 8 && MYSTEPS * MSPLIT == KSTEPS, "the waves cover the outputs and the K steps exactly");
  static_assert(NLG * 512 == MT * G4 && NLX * 512 == MT * X4, "whole float4 rounds of the block");
  static_assert(CT % 64 == 0 && CIN % 64 == 0, "the bank argument of the row pitch");
  static_assert(MT * (PG + PX) <= 65536, "no dynamic-LDS opt-in needed");
  __shared__ __attribute__((aligned(16))) unsigned char smem[MT * (PG + PX)];
  unsigned char* sG = smem;                 // dY tile [MT][PG]
  unsigned char* sX = smem + MT * PG;       // X tile [MT][PX]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ms = wave / WPG, wi = wave % WPG, nw = wi / NKW, kw = wi % NKW;
  const int half = lane >> 5, l31 = lane & 31;
  const int n0 = blockIdx.y * CT;

  f32x16l acc[TN][TK];
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int b = 0; b < TK; ++b) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    }
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int b = 0; b < TK; ++b) asm volatile("s_nop 1" : "+v"(acc[a][b]));   // VALU writes of the accumulators -> the first MFMAs' SrcC

  // a tile's rows through plain 64-bit addresses (M rows of any stride); what lies past M or past cout is loaded from element 0 instead and replaced by zero
  float4 hg[NLG], hx[NLX];
  auto load_tile = [&](int tile) {
    const long long m0 = (long long)tile * MT;
#pragma unroll
    for (int j = 0; j < NLG; ++j) {
      const int i = tid + 512 * j, r = i / G4, c = (i - r * G4) * 4;
      const bool ok = m0 + r < p.M && n0 + c < p.cout;
      const float4 v = *reinterpret_cast<const float4*>(p.G + (ok ? (m0 + r) * p.g_stride + n0 + c : 0));
      hg[j] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int j = 0; j < NLX; ++j) {
      const int i = tid + 512 * j, r = i / X4, c = (i - r * X4) * 4;
      const bool ok = m0 + r < p.M;
      const float4 v = *reinterpret_cast<const float4*>(p.X + (ok ? (m0 + r) * p.x_stride + c : 0));
      hx[j] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };

  // fragment addresses (wgrad_bf16.hip, the head of the file): row 8 half + q4 of a K step's 16 rows, channels 32 tile + 16 group + 4 p4
  const int q4 = (lane & 15) >> 2, p4 = lane & 3, g16 = (lane >> 4) & 1;
  const unsigned char* gBase = sG + (16 * ms + 8 * half + q4) * PG + (32 * nw * TN + 16 * g16 + 4 * p4) * 2;
  const unsigned char* xBase = sX + (16 * ms + 8 * half + q4) * PX + (32 * kw * TK + 16 * g16 + 4 * p4) * 2;
  auto frags = [&](int si, u32x4l (&fa)[TN], u32x4l (&fb)[TK]) {      // the wave's K step si: rows 16 (ms + MSPLIT si) .. of the tile
#pragma unroll
    for (int a = 0; a < TN; ++a) fa[a] = l_tr_frag<PG>(gBase + 16 * MSPLIT * si * PG + 64 * a);
#pragma unroll
    for (int b = 0; b < TK; ++b) fb[b] = l_tr_frag<PX>(xBase + 16 * MSPLIT * si * PX + 64 * b);
  };

  int tile = blockIdx.x;
  if (tile < p.ntiles) load_tile(tile);
  for (; tile < p.ntiles; tile += gridDim.x) {
#pragma unroll
    for (int j = 0; j < NLG; ++j) {
      const int i = tid + 512 * j, r = i / G4, c4 = i - r * G4;
      *reinterpret_cast<uint2*>(sG + r * PG + c4 * 8) = l_cvt4(hg[j]);
    }
#pragma unroll
    for (int j = 0; j < NLX; ++j) {
      const int i = tid + 512 * j, r = i / X4, c4 = i - r * X4;
      *reinterpret_cast<uint2*>(sX + r * PX + c4 * 8) = l_cvt4(hx[j]);
    }
    __syncthreads();
    if (tile + (int)gridDim.x < p.ntiles) load_tile(tile + gridDim.x);     // the next tile flies under this tile's MFMAs
    // the fragments of K step si + 1 are requested before the MFMAs of step si issue
    u32x4l fa[TN], fb[TK];
    frags(0, fa, fb);
#pragma unroll
    for (int si = 0; si < MYSTEPS; ++si) {
      u32x4l na[TN], nb[TK];
#pragma unroll
      for (int a = 0; a < TN; ++a) na[a] = fa[a];
#pragma unroll
      for (int b = 0; b < TK; ++b) nb[b] = fb[b];
      if (si + 1 < MYSTEPS) frags(si + 1, na, nb);
#pragma unroll
      for (int a = 0; a < TN; ++a)
#pragma unroll
        for (int b = 0; b < TK; ++b) l_mfma(acc[a][b], fa[a], fb[b]);
#pragma unroll
      for (int a = 0; a < TN; ++a) fa[a] = na[a];
#pragma unroll
      for (int b = 0; b < TK; ++b) fb[b] = nb[b];
    }
    __syncthreads();   // every wave is done reading before the tiles are overwritten
  }
  // D[row = n][col = k]: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 half
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int b = 0; b < TK; ++b) l_settle(acc[a][b]);
  float* out = p.P + ((long long)blockIdx.x * MSPLIT + ms) * p.cout * CIN;
#pragma unroll
  for (int a = 0; a < TN; ++a)
#pragma unroll
    for (int b = 0; b < TK; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + 32 * (nw * TN + a) + (r & 3) + 8 * (r >> 2) + 4 * half;
        if (n < p.cout) out[(long long)n * CIN + 32 * (kw * TK + b) + l31] = acc[a][b][r];
      }
}

template <int CT, int CIN, int TN, int TK>
void launch_lin_wgrad(const LinWgradArgs& p, int bx, int ny, hipStream_t st) {
  hipLaunchKernelGGL((k_lin_wgrad_bf16<CT, CIN, TN, TK>), dim3((unsigned)bx, (unsigned)ny), dim3(512), 0, st, p);
}

// how a (cout, cin) runs: the cout tile of a block and the wave rectangle; the rest follows from them as in the kernel
struct LwShape { int cout, cin, ct, tn, tk; void (*launch)(const LinWgradArgs&, int, int, hipStream_t); };
#define LW(COUT, CIN, CT, TN, TK) {COUT, CIN, CT, TN, TK, launch_lin_wgrad<CT, CIN, TN, TK>}
const LwShape kShapes[] = {
    LW(64, 64, 64, 1, 1),  LW(128, 64, 128, 1, 1),  LW(256, 64, 256, 2, 1),  LW(576, 64, 640, 5, 1),  LW(1024, 64, 512, 2, 2),
    LW(64, 128, 64, 1, 1), LW(128, 128, 128, 2, 1), LW(256, 128, 256, 2, 2), LW(576, 128, 192, 3, 1), LW(1024, 128, 256, 2, 2),
    LW(64, 256, 64, 1, 2), LW(128, 256, 128, 2, 2), LW(256, 256, 256, 4, 2), LW(576, 256, 192, 3, 2), LW(1024, 256, 256, 4, 2)};
#undef LW

const LwShape* lw_shape(int cout, int cin) {
  for (const LwShape& s : kShapes)
    if (s.cout == cout && s.cin == cin) return &s;
  return nullptr;
}
int lw_ny(const LwShape& s) { return (s.cout + s.ct - 1) / s.ct; }
int lw_msplit(const LwShape& s) { return 8 / ((s.ct / 32 / s.tn) * (s.cin / 32 / s.tk)); }

}  // namespace

int lfsr_lin_wgrad_bf16_slabs_per_block(int cout, int cin) {
  const LwShape* s = lw_shape(cout, cin);
  return s ? lw_msplit(*s) : 0;
}

// blocks along x (each writes lfsr_lin_wgrad_bf16_slabs_per_block slabs of cout cin floats): one per row tile up to 256 blocks in all, and no more than cap_floats holds
int lfsr_lin_wgrad_bf16_blocks(long long M, int cout, int cin, size_t cap_floats) {
  const LwShape* s = lw_shape(cout, cin);
  if (!s || M <= 0) return 0;
  const long long ntiles = (M + lw_mt(s->ct, cin) - 1) / lw_mt(s->ct, cin);
  long long bx = 256 / lw_ny(*s);
  if (bx > ntiles) bx = ntiles;
  const long long fit = (long long)(cap_floats / ((size_t)lw_msplit(*s) * cout * cin));
  return (int)(bx < fit ? bx : fit);
}

// the caller has checked the operands (pointers 16-B aligned, strides multiples of 4 and at least the row width, 0 < M < 2^31 - 128); the grid is what g.part_floats
// holds.  LFSR_E_ARG: shape not covered or not one block's slabs fit, nothing written
int lfsr_lin_wgrad_bf16_launch(const LfsrWgrad& g, hipStream_t st) {
  const LwShape* s = lw_shape(g.N, g.K);
  const int blocks = lfsr_lin_wgrad_bf16_blocks(g.M, g.N, g.K, g.part_floats);
  if (!s || !g.G || !g.X || !g.part || g.M <= 0 || blocks <= 0) return LFSR_E_ARG;
  LinWgradArgs p{};
  p.G = g.G; p.g_stride = g.g_stride; p.X = g.X; p.x_stride = g.x_stride; p.P = g.part; p.M = g.M; p.cout = g.N;
  p.ntiles = (int)((g.M + lw_mt(s->ct, g.K) - 1) / lw_mt(s->ct, g.K));
  s->launch(p, blocks, lw_ny(*s), st);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}
