// lfsr_angconv3x3_fwd: the angular half of LFSSR's AltFilter (model/SR/LFSSR.py:194-216) on VCL rows -- at every pixel q of every sample, a 3x3 conv 64 -> 64 with
// zero padding over the A x A grid of views:
//   y[b,u,v,q,o] = relu(bias[o] + sum_{du,dv in {-1,0,1}, 0 <= u+du < A, 0 <= v+dv < A} sum_c W[o,c,du+1,dv+1] * pre(x[b,u+du,v+dv,q,c]))
//   pre(t) = in_bias ? max(t + in_bias[c], 0) : t          (the bias and ReLU of the spatial conv in front of it, applied while the operand is staged)
// A view outside the grid contributes zero AFTER the prologue: it is neither loaded nor multiplied (its tap is skipped).
//
// Tiling.  A block takes 16 consecutive pixels of one sample and a band of R view rows (R = A up to angRes 5: the whole grid, every input byte read once; 4 / 3 / 2 / 2
// rows at angRes 6 / 7 / 8 / 9).  It stages the band's views and the view row on either side, prologue applied, into LDS: [view][16 pixels][68 floats] (64 channels,
// padded by 4 so that the 16 pixels of an operand fragment start 4 banks apart), at most 36 views x 4352 B = 153 KiB; 106.25 KiB at angRes 5, one block per CU.
// GEMM.  v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation): M = the 16 pixels, N = 16 output channels, K = 4 input channels per instruction.  The sixteen
// waves are 4 output-channel tiles x 4 groups that take the band's views round-robin; a wave keeps one 16 x 16 accumulator per view of its group (at most 7) and, per
// tap, its 16 x 64 slice of W[tap] in 16 registers.  (Four waves a SIMD: 8 waves with 13 accumulators each ran 5 % slower at 32 x 32 views and 10 % at 64 x 64,
// profiles/lfssr_time.md.)  Lane (i, kq) holds the 16 CONTIGUOUS channels 16 kq .. 16 kq + 15 of pixel i / of output channel i, four 16-byte reads each;
// instruction ks of the 16 multiplies channels {16 kq + ks}: any split of K is a valid GEMM as long as both operands use the same one.
// Taps run 0 .. 8 and channels in that fixed order for every output, whatever B, the grid or the band: two runs give the same bits, and a sample's result does not
// depend on the batch.  At angRes 5 the executed taps are 169 of 225.
// k_ang3x3 has one arithmetic.  The entry point reads lfsr_set_ang_arithmetic at every launch: under LFSR_ANG_ARITH_BF16 (and not LFSR_ARITH_F32, which wins) the
// same operation runs on bf16-rounded operands in ang3x3_bf16.hip, after the same argument checks.  It reads none of the other switches.
#include "lfsr_internal.h"

namespace {

constexpr int A3_P = 16;        // pixels per block
constexpr int A3_PITCH = 68;    // floats per staged pixel row
constexpr int A3_SPLIT = 4;     // the band's views go round-robin over this many groups of four waves
constexpr int A3_THREADS = 64 * 4 * A3_SPLIT;
constexpr int A3_J = 7;         // accumulators per wave: its share of the largest band (25 views at angRes 5)
static_assert(A3_J * A3_SPLIT >= 25, "a wave group's accumulators cover its share of a band");

typedef float a3_v4f __attribute__((ext_vector_type(4)));

struct Ang3Args {
  const float* x; int xs, xo;
  const float *w, *bias, *in_bias;
  float* y; int ys, yo;
  int B, A, npix, R, tiles;
};

// rows per band: R * A <= 25 accumulators over the four wave groups, (R + 2) * A <= 36 staged views
__host__ __device__ constexpr int a3_band_rows(int A) { return A <= 5 ? A : A == 6 ? 4 : A == 7 ? 3 : 2; }

__global__ __launch_bounds__(A3_THREADS) void k_ang3x3(Ang3Args p) {
  extern __shared__ float sx[];   // [staged view][A3_P][A3_PITCH]
  const int A = p.A, AA = A * A, npix = p.npix;
  const int tile = blockIdx.x % p.tiles, b = blockIdx.x / p.tiles;
  const int r0 = blockIdx.y * p.R, r1 = min(A, r0 + p.R);        // the band's view rows
  const int s0 = max(0, r0 - 1), s1 = min(A, r1 + 1);            // the staged view rows
  const int q0 = tile * A3_P;
  const int nst = (s1 - s0) * A;
  for (int i = threadIdx.x; i < nst * (A3_P * 16); i += A3_THREADS) {
    const int c4 = (i & 15) * 4, px = (i >> 4) & 15, sv = i >> 8;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q0 + px < npix) {
      const long long row = ((long long)b * AA + s0 * A + sv) * npix + q0 + px;
      t = *reinterpret_cast<const float4*>(p.x + row * p.xs + p.xo + c4);
      if (p.in_bias) {
        const float4 ib = *reinterpret_cast<const float4*>(p.in_bias + c4);
        t.x = fmaxf(t.x + ib.x, 0.f); t.y = fmaxf(t.y + ib.y, 0.f); t.z = fmaxf(t.z + ib.z, 0.f); t.w = fmaxf(t.w + ib.w, 0.f);
      }
    }
    *reinterpret_cast<float4*>(sx + (sv * A3_P + px) * A3_PITCH + c4) = t;
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int nt = wave & 3, part = wave >> 2;
  const int li = lane & 15, kq = lane >> 4;
  const int n = nt * 16 + li;
  const int nout = (r1 - r0) * A;
  a3_v4f acc[A3_J];
#pragma unroll
  for (int j = 0; j < A3_J; ++j) acc[j] = a3_v4f{0.f, 0.f, 0.f, 0.f};
  for (int tap = 0; tap < 9; ++tap) {
    const int du = tap / 3 - 1, dv = tap % 3 - 1;
    float4 wr[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) wr[g] = *reinterpret_cast<const float4*>(p.w + ((size_t)tap * 64 + n) * 64 + kq * 16 + g * 4);
#pragma unroll
    for (int j = 0; j < A3_J; ++j) {
      const int idx = A3_SPLIT * j + part;
      if (idx >= nout) continue;
      const int uu = r0 + idx / A + du, vv = idx % A + dv;
      if (uu < 0 || uu >= A || vv < 0 || vv >= A) continue;      // outside the grid: skipped, not multiplied by zero
      const float* a = sx + (((uu - s0) * A + vv) * A3_P + li) * A3_PITCH + kq * 16;
      float4 ar[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) ar[g] = *reinterpret_cast<const float4*>(a + g * 4);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[g].x, wr[g].x, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[g].y, wr[g].y, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[g].z, wr[g].z, acc[j], 0, 0, 0);
        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[g].w, wr[g].w, acc[j], 0, 0, 0);
      }
    }
  }
  // D[i][j]: lane (li, kq) holds output channel n of pixels 4 kq .. 4 kq + 3
  const float bn = p.bias[n];
#pragma unroll
  for (int j = 0; j < A3_J; ++j) {
    const int idx = A3_SPLIT * j + part;
    if (idx >= nout) continue;
    const long long row0 = ((long long)b * AA + r0 * A + idx) * npix + q0 + 4 * kq;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (q0 + 4 * kq + r < npix) p.y[(row0 + r) * p.ys + p.yo + n] = fmaxf(acc[j][r] + bn, 0.f);
  }
}

}  // namespace

extern "C" int lfsr_angconv3x3_fwd(const float* x, int x_stride, int x_choff, const float* w_packed, const float* bias, const float* in_bias,
                                   float* y, int y_stride, int y_choff, int B, int A, int npix, void* stream) {
  LfsrOpTimer op_t("angconv3x3", A, npix, lfsr_stream(stream));
  if (!x || !w_packed || !bias || !y || B <= 0 || npix <= 0 || A < 2 || A > 9) return LFSR_E_ARG;
  if (x_stride < x_choff + 64 || y_stride < y_choff + 64 || x_choff < 0 || y_choff < 0 || ((x_stride | x_choff | y_stride | y_choff) & 3)) return LFSR_E_ARG;
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)w_packed | (uintptr_t)in_bias) & 15 || ((uintptr_t)bias & 3)) return LFSR_E_ARG;
  const long long rows = (long long)B * A * A * npix;
  if (rows * x_stride >= (1LL << 31) / 4 || rows * y_stride >= (1LL << 31) / 4) return LFSR_E_ARG;   // an operand span of 2 GiB or more
  const int R = a3_band_rows(A), tiles = (npix + A3_P - 1) / A3_P, bands = (A + R - 1) / R;
  if ((long long)B * tiles > 0x7fffffffLL) return LFSR_E_ARG;
  if (lfsr_ang_arith_bf16() && !lfsr_arith_f32())
    return lfsr_ang3x3_bf16_launch(x, x_stride, x_choff, w_packed, bias, in_bias, y, y_stride, y_choff, B, A, npix, lfsr_stream(stream));
  const int staged = (R + 2 < A ? R + 2 : A) * A;
  const size_t smem = (size_t)staged * A3_P * A3_PITCH * sizeof(float);
  static std::atomic<bool> attr_set[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return LFSR_E_ARG;
  if (!attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_ang3x3), hipFuncAttributeMaxDynamicSharedMemorySize, 36 * A3_P * A3_PITCH * (int)sizeof(float));
    if (e != hipSuccess) return LFSR_HIP_ERR(e);
    attr_set[dev] = true;
  }
  Ang3Args p{x, x_stride, x_choff, w_packed, bias, in_bias, y, y_stride, y_choff, B, A, npix, R, tiles};
  hipLaunchKernelGGL(k_ang3x3, dim3((unsigned)(B * tiles), (unsigned)bands), dim3(A3_THREADS), smem, lfsr_stream(stream), p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}
