// lfsr_ang3x3_bf16_launch: lfsr_angconv3x3_fwd (ang3x3.hip) on bf16 operands, lfsr_set_ang_arithmetic(LFSR_ANG_ARITH_BF16).  The same operation at every pixel q of
// every sample:
//   y[b,u,v,q,o] = relu(bias[o] + sum_{taps (du,dv) whose view (u+du,v+dv) is in the A x A grid} sum_c r(W[o,c,du+1,dv+1]) * r(pre(x[b,u+du,v+dv,q,c])))
//   pre(t) = in_bias ? max(t + in_bias[c], 0) : t     (one fp32 add, one max, as k_ang3x3)          r(t) = round to bf16, nearest even, once (v_cvt_pk_bf16_f32)
// Products are exact on v_mfma_f32_16x16x32_bf16; accumulation, bias, ReLU and the stores are fp32; x and y stay fp32 in memory; w is the fp32 direct pack
// [tap][o][c], rounded while a wave loads it.  An off-grid tap is skipped, not multiplied by zero.
//
// Tiling.  As k_ang3x3 a block takes 16 consecutive pixels of one sample and a band of R view rows (the whole grid up to angRes 5; 4 / 3 / 2 / 2 rows at angRes
// 6 / 7 / 8 / 9) and stages the band's views and the view row on either side, prologue applied and rounded, into LDS: [view][16 pixels][144 B] -- 64 bf16 channels
// and 16 B of padding, so that the 16 pixels of a ds_read_b128 fragment read start 4 banks apart and cover all 64 banks once.  25 views x 2304 B = 56.25 KiB at
// angRes 5 (two blocks a CU), at most 36 views = 81 KiB.  A thread keeps eight 16-byte loads in flight while it stages.
// GEMM.  M = 16 output channels (A operand: the weight), N = the 16 pixels (B operand), K = 32 channels per instruction, two instructions per (view, tap).  With the
// weight on the A side a lane's four results are four consecutive output channels of one pixel: one 16-byte store.  The block is four waves, one per 16 output
// channels; a wave holds ALL NINE taps of its weight slice in 72 registers (each weight element is fetched from L2 once per block) and one accumulator per view
// of the band (at most 25).  The loop runs over the STAGED views: a view's two operand fragments are read from LDS once and feed the up to nine outputs
// (u - du, v - dv) they belong to, so a wave reads each staged byte once instead of up to nine times -- with tap-major loops the four waves' LDS reads
// (200 KiB a tap at angRes 5: 800 clocks of the array's 256 B/clk) would take as long as a SIMD's MFMAs of the tap (50 x 16 clocks).
// An output meets its taps in the order of the staged views, which is tap 0 .. 8, and the channels in the order 0 .. 63, for every output, whatever B, the grid
// or the band: two runs give the same bits and a sample's rows do not depend on the batch.  No atomics.
#include "lfsr_internal.h"

namespace {

constexpr int AB_P = 16;          // pixels per block
constexpr int AB_PITCH = 144;     // bytes per staged pixel row: 64 bf16 + 16
constexpr int AB_THREADS = 256;   // four waves: one per 16 output channels
constexpr int AB_LOADS = 8;       // 16-byte loads a thread has in flight while staging

typedef float ab_v4f __attribute__((ext_vector_type(4)));
typedef __bf16 ab_v8h __attribute__((ext_vector_type(8)));

struct AngBfArgs {
  const float* x; int xs, xo;
  const float *w, *bias, *in_bias;
  float* y; int ys, yo;
  int npix, tiles;
};

// rows per band, as k_ang3x3: R * A <= 25 accumulators, (R + 2) * A <= 36 staged views
constexpr int ab_band_rows(int A) { return A <= 5 ? A : A == 6 ? 4 : A == 7 ? 3 : 2; }
constexpr int ab_staged_rows(int A) { return ab_band_rows(A) < A ? ab_band_rows(A) + 2 : A; }

__device__ __forceinline__ unsigned ab_cvt(float lo, float hi) {
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

template <int A>
__global__ __launch_bounds__(AB_THREADS, 2) void k_ang3x3_bf16(AngBfArgs p) {
  constexpr int R = ab_band_rows(A), T = ab_staged_rows(A), AA = A * A;
  constexpr bool BANDED = R < A;
  constexpr int OFF = BANDED ? 1 : 0;        // staged row t is view row r0 - OFF + t
  extern __shared__ uint4 ab_smem[];         // [T * A staged views][AB_P][AB_PITCH bytes]
  char* const sx = reinterpret_cast<char*>(ab_smem);
  const int npix = p.npix;
  const int tile = blockIdx.x % p.tiles, b = blockIdx.x / p.tiles;
  const int r0 = BANDED ? (int)blockIdx.y * R : 0;
  const int q0 = tile * AB_P;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int li = lane & 15, kq = lane >> 4;
  const int n0 = wave * 16;

  // the wave's weight slice, all nine taps: lane (li, kq) holds W[tap][n0 + li][32 s + 8 kq .. + 7] as fragment s
  uint4 wf[9][2];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const float* wp = p.w + ((size_t)tap * 64 + n0 + li) * 64 + 32 * s + 8 * kq;
      const float4 a = *reinterpret_cast<const float4*>(wp), c = *reinterpret_cast<const float4*>(wp + 4);
      wf[tap][s] = make_uint4(ab_cvt(a.x, a.y), ab_cvt(a.z, a.w), ab_cvt(c.x, c.y), ab_cvt(c.z, c.w));
    }

  {  // stage: thread (px, c4) takes four channels of one pixel of every staged view
    const int px = threadIdx.x >> 4, c4 = (threadIdx.x & 15) * 4;
    const bool pin = q0 + px < npix;
    const bool pre = p.in_bias != nullptr;
    float4 ib = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pre) ib = *reinterpret_cast<const float4*>(p.in_bias + c4);
    const float* xb = p.x + p.xo + c4;
    char* const dst = sx + px * AB_PITCH + c4 * 2;
#pragma unroll
    for (int t0 = 0; t0 < T * A; t0 += AB_LOADS) {
      float4 v[AB_LOADS];
#pragma unroll
      for (int k = 0; k < AB_LOADS; ++k) {
        const int sv = t0 + k;
        if (sv >= T * A) continue;
        const int su = r0 - OFF + sv / A;
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pin && su >= 0 && su < A) {
          const long long row = ((long long)b * AA + su * A + sv % A) * npix + q0 + px;
          v[k] = *reinterpret_cast<const float4*>(xb + row * p.xs);
        }
      }
#pragma unroll
      for (int k = 0; k < AB_LOADS; ++k) {
        const int sv = t0 + k;
        if (sv >= T * A) continue;
        float4 t = v[k];
        if (pre && pin) {
          t.x = fmaxf(t.x + ib.x, 0.f); t.y = fmaxf(t.y + ib.y, 0.f); t.z = fmaxf(t.z + ib.z, 0.f); t.w = fmaxf(t.w + ib.w, 0.f);
        }
        *reinterpret_cast<uint2*>(dst + sv * (AB_P * AB_PITCH)) = make_uint2(ab_cvt(t.x, t.y), ab_cvt(t.z, t.w));
      }
    }
  }
  __syncthreads();

  ab_v4f acc[R * A];
#pragma unroll
  for (int j = 0; j < R * A; ++j) acc[j] = ab_v4f{0.f, 0.f, 0.f, 0.f};
  const char* const frag = sx + li * AB_PITCH + kq * 16;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int su = r0 - OFF + t;
    if (BANDED && (su < 0 || su >= A)) continue;                    // a staged row outside the grid: its taps are skipped
#pragma unroll
    for (int sv = 0; sv < A; ++sv) {
      const char* a = frag + (t * A + sv) * (AB_P * AB_PITCH);
      const uint4 x0 = *reinterpret_cast<const uint4*>(a), x1 = *reinterpret_cast<const uint4*>(a + 64);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int orow = t - OFF - (tap / 3 - 1), ov = sv - (tap % 3 - 1);   // the output view this staged view reaches through the tap
          if (orow < 0 || orow >= R || ov < 0 || ov >= A) continue;
          if (BANDED && r0 + orow >= A) continue;                              // the last band may be short
          acc[orow * A + ov] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ab_v8h, wf[tap][s]), __builtin_bit_cast(ab_v8h, s ? x1 : x0),
                                                                        acc[orow * A + ov], 0, 0, 0);
        }
    }
  }

  // D[i][j]: lane (li, kq) holds output channels n0 + 4 kq .. + 3 of pixel li
  const int n = n0 + 4 * kq;
  const float b0 = p.bias[n], b1 = p.bias[n + 1], b2 = p.bias[n + 2], b3 = p.bias[n + 3];
  if (q0 + li < npix) {
    float* const yb = p.y + p.yo + n;
#pragma unroll
    for (int j = 0; j < R * A; ++j) {
      if (BANDED && r0 + j / A >= A) continue;
      const long long row = ((long long)b * AA + r0 * A + j) * npix + q0 + li;
      *reinterpret_cast<float4*>(yb + row * p.ys) =
          make_float4(fmaxf(acc[j][0] + b0, 0.f), fmaxf(acc[j][1] + b1, 0.f), fmaxf(acc[j][2] + b2, 0.f), fmaxf(acc[j][3] + b3, 0.f));
    }
  }
}

template <int A>
int ab_launch(const AngBfArgs& p, int B, int dev, hipStream_t st) {
  constexpr int R = ab_band_rows(A), smem = ab_staged_rows(A) * A * AB_P * AB_PITCH;
  static std::atomic<bool> attr_set[64];
  if (!attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_ang3x3_bf16<A>), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return LFSR_HIP_ERR(e);
    attr_set[dev] = true;
  }
  hipLaunchKernelGGL(k_ang3x3_bf16<A>, dim3((unsigned)(B * p.tiles), (unsigned)((A + R - 1) / R)), dim3(AB_THREADS), smem, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

}  // namespace

// the caller (lfsr_angconv3x3_fwd) has checked the operands
int lfsr_ang3x3_bf16_launch(const float* x, int x_stride, int x_choff, const float* w_packed, const float* bias, const float* in_bias, float* y, int y_stride,
                            int y_choff, int B, int A, int npix, hipStream_t st) {
  const int tiles = (npix + AB_P - 1) / AB_P;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return LFSR_E_ARG;
  const AngBfArgs p{x, x_stride, x_choff, w_packed, bias, in_bias, y, y_stride, y_choff, npix, tiles};
  switch (A) {
    case 2: return ab_launch<2>(p, B, dev, st);
    case 3: return ab_launch<3>(p, B, dev, st);
    case 4: return ab_launch<4>(p, B, dev, st);
    case 5: return ab_launch<5>(p, B, dev, st);
    case 6: return ab_launch<6>(p, B, dev, st);
    case 7: return ab_launch<7>(p, B, dev, st);
    case 8: return ab_launch<8>(p, B, dev, st);
    case 9: return ab_launch<9>(p, B, dev, st);
  }
  return LFSR_E_ARG;
}
