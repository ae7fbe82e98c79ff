// EPIConv.0's weight and data gradients with bf16 OPERANDS: the kernels of lfsr_set_branch_grad_arithmetic(LFSR_BRANCH_GRAD_ARITH_BF16) behind
// lfsr_wgrad_epi0_launch (wgrad.hip) and lfsr_epi0_dgrad_launch (bwd_ops.hip), taken exactly where those launchers take their fp32 EPI-line kernels (A = 5, lines of
// <= 32 pixels).  dE, the input slab and the weights are rounded to bf16 (v_cvt_pk_bf16_f32: nearest even) on their way into LDS, the products are exact and run on
// v_mfma_f32_16x16x32_bf16, accumulation, the partial slabs and the read-modify-write of dx are fp32.  Tensors stay fp32 in memory: the mode changes arithmetic, not
// storage.
//
// ---- weight gradient: k_wgrad_epi0_lines' structure (wgrad.hip) with wgrad_bf16.hip's operand handling
//   dW[tap = 5 dx + v'][n][c] = sum over the EPI lines and their pixels x of dE[line, x][n] * X[view v', x + dx - 2][c]
// A persistent 512-thread block walks EPI lines, horizontal then vertical in one launch; the line's dE (32 px x 32) and its 5 x 36 x 64 input slab (two pixels of zero
// halo, zeros behind a short line: buffer loads with an out-of-range offset) are staged double-buffered, one barrier per line.  The PIXEL index is the MFMA's K: a line
// is ONE K step of 32.  Wave (nh, cq) owns the 16 x 16 block (n half, channel quarter) of all 25 taps: 100 accumulator registers alive across ALL lines of the block,
// one [25][32][64] fp32 slab per block at the end, summed by lfsr_wgrad_reduce.  The launcher starts exactly the block count the caller sized the slabs for; a block
// without a line writes zeros.  No atomics, a fixed order of summation.
//
// Both operands need K = pixel contiguous per lane while the images are [pixel][channel] rows: ds_read_b64_tr_b16 reads, per 16-lane group, 4 pixel rows x 16 channels
// and hands each lane ONE channel of the 4 pixels; lane 4q + p of a group supplies the address of row q, channels 4p .. 4p+3.  K is a summation index, so the pixel it
// stands for is free as long as both operands agree: element 8g + j of lane group g is pixel 4g + j (j < 4) or 16 + 4g + (j - 4).  A 32-lane half (groups g, g + 1)
// then reads 8 CONSECUTIVE rows x 32 B with each of a fragment's two reads, and a tap's shift dx moves all 8 by the same amount.
//   * every lane of every wave takes part in every such read (the line and phase loops are block-uniform), every address is inside the staged images (the halo is the
//     padding) and 8-B aligned (rows are multiples of 8 B, channel blocks of 32 B, p of 8 B; the dynamic LDS base is 16-B aligned, no static LDS);
//   * row pitches 160 B (64 channels) and 96 B (32 channels) = 40 and 24 dwords: 8 consecutive rows start at 0,40,16,56,32,8,48,24 / 0,24,48,8,32,56,16,40 (mod 64)
//     and tile the 64 banks exactly, whatever the common base -- conflict-free.
// LDS: 2 x (180 x 160 + 32 x 96) B = 63 744 B.
//
// ---- data gradient: k_epi0_dgrad_lines' structure (bwd_ops.hip)
//   dX[line, view v', x'][c] += sum_{dx, n} dE[line, x' + 2 - dx][n] * W[tap = 5 dx + v'][n][c]
// A persistent 512-thread block takes chunks of 5 EPI lines; the lines' dE (36 x 32 with the zero halo) are staged once per chunk, then one phase per destination view
// v': its 5 x 32 x 64 weights are rounded from the fp32 direct pack while staged (double-buffered) and wave (pb, cb) computes D[c 16][x' 16] of every line (A = W^t,
// B = dE, K = n = 32: ONE MFMA per (tap, line) where the fp32 kernel issues eight): a lane holds four consecutive CHANNELS of one pixel, so the epilogue is one 16-B
// load + one 16-B store per line.  The weights lie as [dx][n][c] rows of 160 B and are read with the transposed read above (rows = n); the dE rows (80 B pitch: sixteen
// consecutive pixels x 16 B tile the 64 banks) hold n in the same K order -- n = 4g + j at bf16 position 8g + j, n = 16 + 4g + j at 8g + 4 + j -- so a B operand is
// one ds_read_b128.
// LDS: 2 x 5 x 32 x 160 + 5 x 36 x 80 = 65 600 B (dynamic-LDS opt-in).
#include <stdlib.h>

#include "lfsr_internal.h"

typedef float f32x4e __attribute__((ext_vector_type(4)));
typedef unsigned u32x4e __attribute__((ext_vector_type(4)));
typedef short s16x4e __attribute__((ext_vector_type(4)));

namespace {

constexpr int EA = 5;                              // angular resolution both kernels are built for
constexpr int PX = 36;                             // staged pixels of a line: 32 + two of halo on each side
constexpr int XROWB = 160, EROWB = 96;             // weight gradient: LDS bytes per row of 64 / 32 bf16
constexpr int WG_X_BYTES = EA * PX * XROWB;        // 28800
constexpr int WG_BUF_BYTES = WG_X_BYTES + 32 * EROWB;   // 31872
constexpr int WG_SMEM = 2 * WG_BUF_BYTES;          // 63744
static_assert(WG_SMEM <= 65536, "no dynamic-LDS opt-in needed");
constexpr int DG_L = 5;                            // lines of a data-gradient chunk
constexpr int DG_WROWB = 160, DG_EROWB = 80;
constexpr int DG_WBUF_BYTES = EA * 32 * DG_WROWB;  // 25600
constexpr int DG_SMEM = 2 * DG_WBUF_BYTES + DG_L * PX * DG_EROWB;   // 65600
constexpr int OOB = (int)0x80000000u;

struct WgradEpiB16Args {
  const float* G;            // dE rows ((q h + y) w + x), 32 channels: the horizontal pass's (vert != 1) or the only pass's
  const float* G2;           // vert == 2: the vertical pass's dE; lines [0, nH) are horizontal (G), the rest vertical (G2)
  const float* X; int x_stride; int x_choff;
  float* P;                  // [gridDim.x][25][32][64]
  int g_bytes, x_bytes;
  int B, H, W, vert;
};

struct EpiDgradB16Args {
  const float* G;            // dE rows, 32 channels
  const float* Wd;           // fp32 direct pack [25 taps][32][64]
  float* Y; int y_stride; int y_choff;     // dX (read-modify-write)
  int g_bytes, y_bytes;
  int B, H, W, vert;
};

__device__ __forceinline__ unsigned e_cvt_pk_bf16(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}
__device__ __forceinline__ uint2 e_cvt4(const f32x4e v) { return make_uint2(e_cvt_pk_bf16(v.x, v.y), e_cvt_pk_bf16(v.z, v.w)); }
// asm MFMA, accumulator tied (rowgemm_b3.hip, b3_mfma: why not the builtin)
__device__ __forceinline__ void e_mfma(f32x4e& c, const u32x4e a, const u32x4e b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "v"(b));
}
// 8 K elements x 1 column of a [row][column] image: two transposed reads, 16 rows apart (the K order of the head of the file)
template <int ROWB>
__device__ __forceinline__ u32x4e e_tr_frag(const unsigned char* p) {
  typedef __attribute__((address_space(3))) s16x4e* lds_ptr;
  const s16x4e lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p));
  const s16x4e hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p + 16 * ROWB));
  const uint2 l = __builtin_bit_cast(uint2, lo), h = __builtin_bit_cast(uint2, hi);
  return u32x4e{l.x, l.y, h.x, h.y};
}

__global__ __launch_bounds__(512) void k_wgrad_epi0_bf16(WgradEpiB16Args p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm_we[];
  constexpr int NIN = (EA * PX * 16 + 511) / 512;   // 6 float4 of the slab per thread (the last partly)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int nh = wave >> 2, cq = wave & 3;
  const int HW = p.H * p.W;
  const int nH = p.vert == 1 ? 0 : p.B * EA * p.H, nV = p.vert == 0 ? 0 : p.B * EA * p.W;   // horizontal lines (b, u, y), vertical lines (b, v, x)
  const int nlines = nH + nV;
  const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.X), 0, p.x_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.G), 0, p.g_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsG2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.vert == 2 ? p.G2 : p.G), 0, p.g_bytes, 0x00020000);
  f32x4e acc[EA * EA];
#pragma unroll
  for (int t = 0; t < EA * EA; ++t) acc[t] = f32x4e{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < EA * EA; ++t) asm volatile("s_nop 1" : "+v"(acc[t]));   // VALU writes of the accumulators -> the first MFMAs' SrcC
  f32x4e hin[NIN], he;
  auto load_line = [&](int line) {
    const bool vert = line >= nH;                     // block-uniform
    const int ln = vert ? line - nH : line;
    const int len = vert ? p.H : p.W, across = vert ? p.W : p.H;
    const int vstride = vert ? EA * HW : HW, pstride = vert ? p.W : 1;
    const int q = ln / across, o = ln - q * across;
    int base, mbase;   // first pixel of the line in X (view 0); first dE row of the line
    if (!vert) { base = q * EA * HW + o * p.W; mbase = (q * p.H + o) * p.W; }
    else { const int b = q / EA, v = q - b * EA; base = (b * EA * EA + v) * HW + o; mbase = q * HW + o; }
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
      const int idx = tid + 512 * i, c16 = idx & 15, pv = idx >> 4;
      const int vv = pv / PX, t = pv - vv * PX - 2;
      const bool ok = pv < EA * PX && t >= 0 && t < len;
      hin[i] = __builtin_bit_cast(f32x4e, __builtin_amdgcn_raw_buffer_load_b128(rsX, ok ? ((base + vv * vstride + t * pstride) * p.x_stride + p.x_choff + c16 * 4) * 4 : OOB, 0, 0));
    }
    {
      const int px = tid >> 3, c8 = tid & 7;
      const bool ok = tid < 256 && px < len;
      const int off = ok ? ((mbase + px * pstride) * 32 + c8 * 4) * 4 : OOB;
      he = vert ? __builtin_bit_cast(f32x4e, __builtin_amdgcn_raw_buffer_load_b128(rsG2, off, 0, 0))
                : __builtin_bit_cast(f32x4e, __builtin_amdgcn_raw_buffer_load_b128(rsG, off, 0, 0));
    }
  };
  // fragment addresses (see the head of the file): row 4g + q4 (+ 16) of the line's pixels, channels 16 block + 4 p4
  const int q4 = l15 >> 2, p4 = lane & 3;
  const int eOff = WG_X_BYTES + (4 * g + q4) * EROWB + (16 * nh + 4 * p4) * 2;
  const int xOff = (4 * g + q4) * XROWB + (16 * cq + 4 * p4) * 2;
  int line = blockIdx.x, it = 0;
  if (line < nlines) load_line(line);
  for (; line < nlines; line += gridDim.x, ++it) {
    unsigned char* const sIn = sm_we + (it & 1) * WG_BUF_BYTES;
    unsigned char* const sE = sIn + WG_X_BYTES;
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
      const int idx = tid + 512 * i, c16 = idx & 15, pv = idx >> 4;
      if (pv < EA * PX) *reinterpret_cast<uint2*>(sIn + pv * XROWB + c16 * 8) = e_cvt4(hin[i]);
    }
    if (tid < 256) *reinterpret_cast<uint2*>(sE + (tid >> 3) * EROWB + (tid & 7) * 8) = e_cvt4(he);
    __syncthreads();   // (the only barrier of a line: the other buffer was last read before the previous line's barrier)
    if (line + (int)gridDim.x < nlines) load_line(line + gridDim.x);
    const u32x4e fa = e_tr_frag<EROWB>(sIn + eOff);   // read once for all 25 taps
#pragma unroll
    for (int dx = 0; dx < EA; ++dx) {
      u32x4e fb[EA];
#pragma unroll
      for (int vv = 0; vv < EA; ++vv) fb[vv] = e_tr_frag<XROWB>(sIn + xOff + (vv * PX + dx) * XROWB);
#pragma unroll
      for (int vv = 0; vv < EA; ++vv) e_mfma(acc[dx * EA + vv], fa, fb[vv]);
    }
  }
  // D of block (nh, cq): lane holds column c = cq 16 + l15, rows n = nh 16 + 4 g + r
#pragma unroll
  for (int t = 0; t < EA * EA; ++t) asm volatile("s_nop 15\n\ts_nop 15" : "+v"(acc[t]));   // MFMA results -> the stores' reads
  float* out = p.P + (long long)blockIdx.x * EA * EA * 32 * 64;
#pragma unroll
  for (int t = 0; t < EA * EA; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) out[((long long)t * 32 + nh * 16 + 4 * g + r) * 64 + cq * 16 + l15] = acc[t][r];
}

__global__ __launch_bounds__(512) void k_epi0_dgrad_bf16(EpiDgradB16Args p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm_de[];
  unsigned char* const sE = sm_de + 2 * DG_WBUF_BYTES;   // [DG_L][36][DG_EROWB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g = lane >> 4;
  const int pb = wave >> 2, cb = wave & 3;
  const int HW = p.H * p.W;
  const int len = p.vert ? p.H : p.W, across = p.vert ? p.W : p.H;
  const int nlines = p.B * EA * across;
  const int vstride = p.vert ? EA * HW : HW, pstride = p.vert ? p.W : 1;
  const __amdgpu_buffer_rsrc_t rsG = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.G), 0, p.g_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc(p.Y, 0, p.y_bytes, 0x00020000);
  const int nchunks = (nlines + DG_L - 1) / DG_L;
  f32x4e wr[EA];
  auto load_w = [&](int vv) {
#pragma unroll
    for (int i = 0; i < EA; ++i)   // (dx, n, c4): dx = i, n = tid >> 4, c4 = tid & 15
      wr[i] = *reinterpret_cast<const f32x4e*>(p.Wd + ((long long)(i * EA + vv) * 32 + (tid >> 4)) * 64 + (tid & 15) * 4);
  };
  auto store_w = [&](unsigned char* buf) {
#pragma unroll
    for (int i = 0; i < EA; ++i) *reinterpret_cast<uint2*>(buf + (i * 32 + (tid >> 4)) * DG_WROWB + (tid & 15) * 8) = e_cvt4(wr[i]);
  };
  const int q4 = l15 >> 2, p4 = lane & 3;
  const int wOff = (4 * g + q4) * DG_WROWB + (16 * cb + 4 * p4) * 2;   // A fragment: rows n = 4g + q4 (+ 16), channels 16 cb + 4 p4
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int line0 = chunk * DG_L;
    __syncthreads();                               // the previous chunk's phases are done with sE and the weight buffers
    // ---- the chunk's dE lines -> sE (halo pixels and missing lines zero), n in the K order of the head of the file
    for (int idx = tid; idx < DG_L * PX * 8; idx += 512) {
      const int n4 = idx & 7, px = (idx >> 3) % PX, ln = idx / (PX * 8);
      const int line = line0 + ln, t = px - 2;
      int off = OOB;
      if (line < nlines && t >= 0 && t < len) {
        const int q = line / across, o = line - q * across;
        const int mbase = p.vert ? q * HW + o : (q * p.H + o) * p.W;
        off = ((mbase + t * pstride) * 32 + n4 * 4) * 4;
      }
      const f32x4e v = __builtin_bit_cast(f32x4e, __builtin_amdgcn_raw_buffer_load_b128(rsG, off, 0, 0));
      *reinterpret_cast<uint2*>(sE + (ln * PX + px) * DG_EROWB + (n4 & 3) * 16 + (n4 >> 2) * 8) = e_cvt4(v);
    }
    load_w(0);
    store_w(sm_de);
    // this lane's pixel of each line of the chunk (x' = pb 16 + l15) in dX: byte offset of its 4 channels, or out of range
    int yoff[DG_L];
#pragma unroll
    for (int ln = 0; ln < DG_L; ++ln) {
      const int line = line0 + ln, xq = pb * 16 + l15;
      yoff[ln] = OOB;
      if (line < nlines && xq < len) {
        const int q = line / across, o = line - q * across;
        int base;
        if (!p.vert) base = q * EA * HW + o * p.W;
        else { const int b = q / EA, v = q - b * EA; base = (b * EA * EA + v) * HW + o; }
        yoff[ln] = ((base + xq * pstride) * p.y_stride + p.y_choff + cb * 16 + 4 * g) * 4;
      }
    }
#pragma unroll 1
    for (int vv = 0; vv < EA; ++vv) {
      __syncthreads();                             // weights of view vv (and, for vv = 0, the dE lines) are staged; the other buffer is free
      if (vv + 1 < EA) load_w(vv + 1);
      const unsigned char* sW = sm_de + (vv & 1) * DG_WBUF_BYTES;
      const int vbytes = vv * vstride * p.y_stride * 4;   // wave-uniform
      f32x4e old[DG_L];
#pragma unroll
      for (int ln = 0; ln < DG_L; ++ln) old[ln] = __builtin_bit_cast(f32x4e, __builtin_amdgcn_raw_buffer_load_b128(rsY, yoff[ln], vbytes, 0));
      f32x4e acc[DG_L];
#pragma unroll
      for (int ln = 0; ln < DG_L; ++ln) acc[ln] = f32x4e{0.f, 0.f, 0.f, 0.f};
      asm volatile("s_nop 1" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]));   // VALU writes -> the first MFMAs' SrcC
#pragma unroll
      for (int dx = 0; dx < EA; ++dx) {
        const u32x4e a = e_tr_frag<DG_WROWB>(sW + wOff + dx * 32 * DG_WROWB);
#pragma unroll
        for (int ln = 0; ln < DG_L; ++ln) {
          const u32x4e b = *reinterpret_cast<const u32x4e*>(sE + (ln * PX + pb * 16 + l15 + 4 - dx) * DG_EROWB + g * 16);
          e_mfma(acc[ln], a, b);
        }
      }
      asm volatile("s_nop 15\n\ts_nop 15" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]));   // MFMA results -> the adds' reads
#pragma unroll
      for (int ln = 0; ln < DG_L; ++ln)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4e, old[ln] + acc[ln]), rsY, yoff[ln], vbytes, 0);
      if (vv + 1 < EA) store_w(sm_de + ((vv + 1) & 1) * DG_WBUF_BYTES);   // (the other buffer: last read in phase vv - 1, which every wave left before this phase's barrier)
    }
  }
}

}  // namespace

// Both passes in one launch (G / G2), the geometry lfsr_wgrad_epi0_launch covers; lfsr_epi0_dgrad_launch has checked the data gradient's coverage and selector.
int lfsr_wgrad_epi0_bf16_launch(const LfsrWgrad& g, hipStream_t st) {
  const int B = g.B, h = g.h, w = g.w;
  if (!g.G || !g.G2 || !g.X || !g.part || B <= 0 || h <= 0 || w <= 0 || g.A != EA || h > 32 || w > 32) return LFSR_E_ARG;
  if (((g.x_stride | g.x_choff) & 3) || g.x_stride < g.x_choff + 64) return LFSR_E_ARG;
  if ((long long)B * EA * EA * h * w * g.x_stride * 4 >= (1LL << 31)) return LFSR_E_ARG;
  LfsrOpTimer op_t("epi0_wgrad", B, h * w, st);
  WgradEpiB16Args p{};
  p.G = g.G; p.G2 = g.G2; p.X = g.X; p.x_stride = g.x_stride; p.x_choff = g.x_choff; p.P = g.part;
  p.g_bytes = (int)((long long)B * EA * h * w * 32 * 4); p.x_bytes = (int)((long long)B * EA * EA * h * w * g.x_stride * 4);
  p.B = B; p.H = h; p.W = w; p.vert = 2;
  hipLaunchKernelGGL(k_wgrad_epi0_bf16, dim3((unsigned)lfsr_wgrad_epi0_blocks(B, EA, h, w)), dim3(512), WG_SMEM, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

int lfsr_epi0_dgrad_bf16_launch(const float* dE, const float* w_direct, float* dx, int dx_stride, int dx_choff, int B, int h, int w, int vert, hipStream_t st) {
  if (!dE || !w_direct || !dx || B <= 0 || h <= 0 || w <= 0 || ((dx_stride | dx_choff) & 3) || dx_stride < dx_choff + 64 || (vert ? h : w) > 32) return LFSR_E_ARG;
  if ((long long)B * EA * EA * h * w * dx_stride * 4 >= (1LL << 31)) return LFSR_E_ARG;
  static std::atomic<bool> attr_set[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return LFSR_HIP_ERR(hipErrorInvalidDevice);
  if (!attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_epi0_dgrad_bf16), hipFuncAttributeMaxDynamicSharedMemorySize, DG_SMEM);
    if (e != hipSuccess) return LFSR_HIP_ERR(e);
    attr_set[dev] = true;
  }
  EpiDgradB16Args p{};
  p.G = dE; p.Wd = w_direct; p.Y = dx; p.y_stride = dx_stride; p.y_choff = dx_choff;
  p.g_bytes = (int)((long long)B * EA * h * w * 32 * 4); p.y_bytes = (int)((long long)B * EA * EA * h * w * dx_stride * 4);
  p.B = B; p.H = h; p.W = w; p.vert = vert;
  const long long nchunks = ((long long)B * EA * (vert ? w : h) + DG_L - 1) / DG_L;
  hipLaunchKernelGGL(k_epi0_dgrad_bf16, dim3((unsigned)(nchunks < 256 ? nchunks : 256)), dim3(512), DG_SMEM, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}
