// Backward of the epipolar-plane self-attention on the matrix pipe: the counterpart of attn_mfma.hip (same geometry, same token order, same
// operand layouts; read its header first).  Given q | k, v, O and dO it writes dQ | dK and dV; the softmax is recomputed (base 2, raw v_exp_f32),
// nothing but the forward's inputs and output is read, and there are no float atomics: every output element is written by one lane in a
// fixed summation order, so two runs give the same bits.
//
// One block per (sequence, head), 256 threads = 4 waves, fp32 v_mfma_f32_16x16x4_f32 throughout (D[i][j]: lane holds j = lane & 15, rows
// i = 4 g + r; A reads [i = lane & 15][k = g], B reads [k = g][j = lane & 15]; g = lane >> 4).  Staged once per block, zero beyond L:
//   row-major  K, V, Q, dO   [token][16]              the K image of attn_mfma.hip, chunk c of token t at (c + ((t >> 2) & 2)) & 3
//   transposed K^T, Q^T, dO^T [tile][d][16 tokens]    the V^T image of attn_mfma.hip, chunk j of row d at j ^ ((-(d >> 2)) & 3)
// 70 KB + the per-query statistics (5 x 160 words): 74 880 B, two blocks per CU.
//
// Phase 1, a wave per query tile (query on the lane, as the forward):
//   S^T  = K Q^T (Q scaled by log2 e / sqrt(hd)), masked, its maximum m and P^T = exp2(S^T - m) over registers and two shuffles
//   D    = sum_d dO O                             lane partial + two shuffles
//   dP^T = V dO^T                                 A = V row-major, B = dO (Q and dO: the lane's chunk of the staged rows)
//   dS^T = P^T o (dP^T - D)                       (the division by the denominator is applied once, to dQ)
//   dQ^T += K^T_tile dS^T                         B = the dS^T registers AS THEY STAND (the forward's O^T += V^T P^T)
//   m, 1 / den, D and the band [lo, lo + width) of the query go to LDS.
// Phase 2, a wave per key tile (key on the lane), over the query tiles whose bands touch it:
//   S  = Q K^T (K scaled), P = exp2(S - m_q) / den_q under the band predicate of the register's query; dP = dO V^T; dS = P o (dP - D_q)
//   dV^T += dO^T_tile P and dK^T += Q^T_tile dS   B = the registers as they stand
// dS carries 1 / sqrt(hd) only (applied to dQ and dK at the store), not log2 e.
#include <math.h>

#include "lfsr_internal.h"

typedef float f32x4a __attribute__((ext_vector_type(4)));
typedef int i32x4a __attribute__((ext_vector_type(4)));

namespace {

struct EpiAttnBwdArgs {
  const float* QK; int qk_stride, q_choff, k_choff;
  const float* V; int v_stride;
  const float* O; const float* dO; int o_stride;
  float* dQK; float* dV;
  int nheads;
  int ns1, ns2; long long bs0, bs1, bs2;
  int n1, n2; long long st1, st2;
  int l2, r2, clip2;
  float scale2;    // 1 / sqrt(hd) * log2(e)
  float scale;     // 1 / sqrt(hd)
  int L;           // n1 * n2
};

__device__ __forceinline__ f32x4a mfma4(const f32x4a a, const f32x4a b, f32x4a acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
  return acc;
}
// A-operand reads: row-major image [token][16] (lane's row, chunk g) and transposed tile [d = lane & 15][16 tokens] (chunk g)
__device__ __forceinline__ f32x4a rd_row(const float* img, int row, int g) {
  return *reinterpret_cast<const f32x4a*>(img + row * 16 + (((g + ((row >> 2) & 2)) & 3) << 2));
}
__device__ __forceinline__ f32x4a rd_tr(const float* img, int tile, int l15, int g) {
  return *reinterpret_cast<const f32x4a*>(img + tile * 256 + l15 * 16 + ((g ^ ((4 - (l15 >> 2)) & 3)) << 2));
}
__device__ __forceinline__ void st_row(float* img, int tok, int c, const f32x4a v) {
  *reinterpret_cast<f32x4a*>(img + tok * 16 + (((c + ((tok >> 2) & 2)) & 3) << 2)) = v;
}
__device__ __forceinline__ void st_tr(float* img, int tok, int c, const f32x4a v) {
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) img[(tok >> 4) * 256 + (4 * c + jj) * 16 + (((((tok >> 2) & 3) ^ ((4 - c) & 3))) << 2) + (tok & 3)] = v[jj];
}

constexpr int NW = 4;     // waves per block

template <int NT, int N1>      // N1: the angular resolution when known at compile time (5), 0: read from the arguments
__global__ __launch_bounds__(64 * NW) void k_epi_attn_bwd_mfma(EpiAttnBwdArgs p) {
  const int n1 = N1 ? N1 : p.n1;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LR = NT * 16, IMG = LR * 16;
  float* const sK = smem;
  float* const sV = sK + IMG;
  float* const sQ = sV + IMG;
  float* const sdO = sQ + IMG;
  float* const sKt = sdO + IMG;
  float* const sQt = sKt + IMG;
  float* const sdOt = sQt + IMG;
  float* const sM = sdOt + IMG;      // statistics of phase 1, per query token
  float* const sInv = sM + LR;
  float* const sD = sInv + LR;
  int* const sLo = reinterpret_cast<int*>(sD + LR);
  int* const sW = sLo + LR;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const int head = blockIdx.x % p.nheads;
  int t = blockIdx.x / p.nheads;
  const int s2 = t % p.ns2; t /= p.ns2;
  const int s1 = t % p.ns1;
  const int s0 = t / p.ns1;
  const long long base = s0 * p.bs0 + s1 * p.bs1 + s2 * p.bs2;
  const int hq = p.q_choff + head * 16, hk = p.k_choff + head * 16, hc = head * 16;

  // ---- stage (item = (token, 16-B chunk c of its 64-B head slice); every load of a thread is issued before its first LDS store) ----
  {
    constexpr int NIT = (LR * 4 + 64 * NW - 1) / (64 * NW);
    f32x4a kv[NIT], vv[NIT], qv[NIT], dv[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = tid + 64 * NW * it;
      const int tok = idx >> 2, c = idx & 3;
      kv[it] = f32x4a{0.f, 0.f, 0.f, 0.f}; vv[it] = kv[it]; qv[it] = kv[it]; dv[it] = kv[it];
      if (idx < LR * 4 && tok < p.L) {
        const int t2 = tok / n1, t1 = tok - t2 * n1;
        const long long pix = base + t1 * p.st1 + t2 * p.st2;
        kv[it] = *reinterpret_cast<const f32x4a*>(p.QK + pix * p.qk_stride + hk + 4 * c);
        qv[it] = *reinterpret_cast<const f32x4a*>(p.QK + pix * p.qk_stride + hq + 4 * c);
        vv[it] = *reinterpret_cast<const f32x4a*>(p.V + pix * p.v_stride + hc + 4 * c);
        dv[it] = *reinterpret_cast<const f32x4a*>(p.dO + pix * p.o_stride + hc + 4 * c);
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = tid + 64 * NW * it;
      if (idx < LR * 4) {
        const int tok = idx >> 2, c = idx & 3;
        st_row(sK, tok, c, kv[it]); st_row(sV, tok, c, vv[it]); st_row(sQ, tok, c, qv[it]); st_row(sdO, tok, c, dv[it]);
        st_tr(sKt, tok, c, kv[it]); st_tr(sQt, tok, c, qv[it]); st_tr(sdOt, tok, c, dv[it]);
      }
    }
  }
  __syncthreads();

  const int kmax = min(p.n2, p.clip2);
  const int ntl = (p.L + 15) >> 4;       // tiles that hold a token
  // ---- phase 1: query tiles wave, wave + NW, ... ----
#pragma unroll
  for (int qi = 0; qi < (NT + NW - 1) / NW; ++qi) {
    const int qt = wave + NW * qi;
    if (qt >= ntl) break;
    const int qtok = qt * 16 + l15;
    const bool qok = qtok < p.L;
    const int qc = qok ? qtok : p.L - 1;
    const int t2q = qc / n1, t1q = qc - t2q * n1;
    const long long qpix = base + t1q * p.st1 + t2q * p.st2;
    const f32x4a qb = rd_row(sQ, qtok, g) * p.scale2;      // the B operand [d = 4 g + r][q = lane & 15] is the lane's own chunk g of the row-major image
    const f32x4a dob = rd_row(sdO, qtok, g);
    const f32x4a ob = *reinterpret_cast<const f32x4a*>(p.O + qpix * p.o_stride + hc + 4 * g);
    float D = dob.x * ob.x + dob.y * ob.y + dob.z * ob.z + dob.w * ob.w;
    D += __shfl_xor(D, 16);
    D += __shfl_xor(D, 32);
    const int lo = max(0, t2q - p.l2) * n1, hi = min(kmax, t2q + p.r2) * n1;
    const int kbase = 4 * g - lo;
    const unsigned kwidth = (unsigned)(hi > lo ? hi - lo : 0);
    const int q2lo = (qt * 16) / n1, q2hi = min(p.L - 1, qt * 16 + 15) / n1;
    const int klo = max(0, q2lo - p.l2) * n1, khi = min(kmax, q2hi + p.r2) * n1;
    const int ktlo = klo >> 4, kthi = (khi - 1) >> 4;

    f32x4a S[NT];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      if (kt >= ktlo && kt <= kthi) {
        const f32x4a acc = mfma4(rd_row(sK, kt * 16 + l15, g), qb, f32x4a{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float s = (unsigned)(kbase + (kt * 16 + r)) < kwidth ? acc[r] : -INFINITY;
          S[kt][r] = s;
          m = fmaxf(m, s);
        }
      }
    }
    m = fmaxf(m, __shfl_xor(m, 16));
    m = fmaxf(m, __shfl_xor(m, 32));
    float den = 0.f;
    f32x4a dq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      if (kt >= ktlo && kt <= kthi) {
        const f32x4a dp = mfma4(rd_row(sV, kt * 16 + l15, g), dob, f32x4a{0.f, 0.f, 0.f, 0.f});
        f32x4a ds;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pw = __builtin_amdgcn_exp2f(S[kt][r] - m);     // 0 on masked keys
          den += pw;
          ds[r] = pw * (dp[r] - D);
        }
        dq = mfma4(rd_tr(sKt, kt, l15, g), ds, dq);
      }
    }
    den += __shfl_xor(den, 16);
    den += __shfl_xor(den, 32);
    const float inv = 1.0f / den;
    if (qok) *reinterpret_cast<f32x4a*>(p.dQK + qpix * p.qk_stride + hq + 4 * g) = dq * (inv * p.scale);
    if (g == 0) {      // a query beyond L has an empty band: phase 2 never reads its m, 1 / den, D
      sM[qtok] = m; sInv[qtok] = inv; sD[qtok] = D; sLo[qtok] = lo; sW[qtok] = qok ? (int)kwidth : 0;
    }
  }
  __syncthreads();

  // ---- phase 2: key tiles wave, wave + NW, ... ----
  for (int kt = wave; kt < ntl; kt += NW) {
    const int krow = kt * 16 + l15;
    const f32x4a kb = rd_row(sK, krow, g) * p.scale2;
    const f32x4a vb = rd_row(sV, krow, g);
    // the queries that can see a key of this tile: t2q in [t2k - r2 + 1, t2k + l2]
    const int k2lo = (kt * 16) / n1, k2hi = min(p.L - 1, kt * 16 + 15) / n1;
    const int q2lo = max(0, k2lo - p.r2 + 1), q2hi = min(p.n2 - 1, k2hi + p.l2);
    const int qtlo = (q2lo * n1) >> 4, qthi = min(ntl - 1, ((q2hi + 1) * n1 - 1) >> 4);
    f32x4a dk = {0.f, 0.f, 0.f, 0.f}, dvv = {0.f, 0.f, 0.f, 0.f};
    for (int qt = qtlo; qt <= qthi; ++qt) {
      const int qrow = qt * 16 + l15;
      const f32x4a s = mfma4(rd_row(sQ, qrow, g), kb, f32x4a{0.f, 0.f, 0.f, 0.f});
      const f32x4a dp = mfma4(rd_row(sdO, qrow, g), vb, f32x4a{0.f, 0.f, 0.f, 0.f});
      const int q4 = qt * 16 + 4 * g;
      const f32x4a m4 = *reinterpret_cast<const f32x4a*>(sM + q4), i4 = *reinterpret_cast<const f32x4a*>(sInv + q4), d4 = *reinterpret_cast<const f32x4a*>(sD + q4);
      const i32x4a lo4 = *reinterpret_cast<const i32x4a*>(sLo + q4), w4 = *reinterpret_cast<const i32x4a*>(sW + q4);
      f32x4a pr, ds;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = (unsigned)(krow - lo4[r]) < (unsigned)w4[r];
        const float pv = __builtin_amdgcn_exp2f(s[r] - m4[r]) * i4[r];
        pr[r] = ok ? pv : 0.f;
        ds[r] = ok ? pv * (dp[r] - d4[r]) : 0.f;
      }
      dvv = mfma4(rd_tr(sdOt, qt, l15, g), pr, dvv);
      dk = mfma4(rd_tr(sQt, qt, l15, g), ds, dk);
    }
    if (krow < p.L) {
      const int t2 = krow / n1, t1 = krow - t2 * n1;
      const long long kpix = base + t1 * p.st1 + t2 * p.st2;
      *reinterpret_cast<f32x4a*>(p.dQK + kpix * p.qk_stride + hk + 4 * g) = dk * p.scale;
      *reinterpret_cast<f32x4a*>(p.dV + kpix * p.v_stride + hc + 4 * g) = dvv;
    }
  }
}

}  // namespace

// LFSR_E_ARG = geometry not covered (the dispatcher runs the VALU pair): the coverage of lfsr_epi_attn_mfma_launch
int lfsr_epi_attn_bwd_mfma_launch(const LfsrAttnGrad& a, hipStream_t st) {
  const LfsrAttnGeom& g = a.g;
  const long long Lll = g.tokens();
  // every angular position visible; <= 10 tiles of 16 tokens.  A one-token sequence goes to the VALU pair: the softmax over a single key is constant, dQ = dK = 0
  // and dV = dO exactly, which the pair returns, while dP - D here (two differently ordered sums of the same products) leaves rounding residue in their place
  if (a.hd != 16 || a.nheads % 4 || Lll > 160 || Lll < 2 || g.l1 < g.n1 - 1 || g.r1 < g.n1) return LFSR_E_ARG;
  EpiAttnBwdArgs p{};
  p.QK = a.qk; p.qk_stride = a.qk_stride; p.q_choff = a.q_choff; p.k_choff = a.k_choff; p.V = a.v; p.v_stride = a.v_stride; p.O = a.o; p.dO = a.d_o; p.o_stride = a.o_stride;
  p.dQK = a.dqk; p.dV = a.dv; p.nheads = a.nheads; p.ns1 = g.ns1; p.ns2 = g.ns2; p.bs0 = g.bs0; p.bs1 = g.bs1; p.bs2 = g.bs2;
  p.n1 = g.n1; p.n2 = g.n2; p.st1 = g.st1; p.st2 = g.st2; p.l2 = g.l2 < g.n2 ? g.l2 : g.n2; p.r2 = g.r2 < g.n2 ? g.r2 : g.n2; p.clip2 = g.clip2;     // (a window wider than the sequence is the sequence)
  p.scale = 1.0f / sqrtf(16.0f);
  p.scale2 = p.scale * 1.44269504088896340736f;
  p.L = (int)Lll;
  const long long nblk = g.nseq() * a.nheads;
  if (nblk <= 0 || nblk > 0x7fffffffLL) return LFSR_E_ARG;
  constexpr int NT = 10;
  const int smem = (7 * NT * 16 * 16 + 5 * NT * 16) * 4;   // 74880
  static std::atomic<bool> attr_set[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return LFSR_HIP_ERR(hipErrorInvalidDevice);
  if (!attr_set[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_epi_attn_bwd_mfma<NT, 5>), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_epi_attn_bwd_mfma<NT, 0>), hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    if (e != hipSuccess) return LFSR_HIP_ERR(e);
    attr_set[dev] = true;
  }
  if (g.n1 == 5) hipLaunchKernelGGL((k_epi_attn_bwd_mfma<NT, 5>), dim3((unsigned)nblk), dim3(64 * NW), smem, st, p);
  else hipLaunchKernelGGL((k_epi_attn_bwd_mfma<NT, 0>), dim3((unsigned)nblk), dim3(64 * NW), smem, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}
