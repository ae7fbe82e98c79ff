// What the backward drivers of LFT (lft_train.hip) and EPIT (epit_train.hip) share beyond the gather-GEMMs and wgrad.hip: the elementwise
// add / mask, the LayerNorm backward, the up-sampling tail's backward, and the windowed attention backward's VALU pair, which every
// geometry can run on (LFT's angular and spatial attention; EPIT's EPI attention outside the coverage of attn_bwd_mfma.hip; attn.cpp
// picks).  Every reduction runs in a fixed order: gradient buckets are bitwise reproducible.  After the kernels
// and their launchers comes the drivers' shared host code: the context the two drivers are written in (LfsrTransBwd) and the three stages that
// are the same graph in both models, the mirror of transformer.hip's lfsr_trans_head / _qkv / _ffn / _tail.
#include <math.h>

#include <algorithm>

#include "gemm_gather_kernel.h"
#include "param_table.h"

namespace {

// d = (a (+ b)) * (mk > 0 ? 1 : slope)  over C columns (C % 4 == 0); b, mk optional; a and d may alias
__global__ __launch_bounds__(256) void k_ew(const float* a, int as, const float* __restrict__ b, int bs, const float* __restrict__ mk, int ms, float slope,
                                            float* d, int ds, int C, long long M) {
  const int c4n = C / 4;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < M * c4n; g += (long long)gridDim.x * 256) {
    const long long r = g / c4n;
    const int c = (int)(g - r * c4n) * 4;
    float4 v = *reinterpret_cast<const float4*>(a + r * as + c);
    if (b) {
      const float4 u = *reinterpret_cast<const float4*>(b + r * bs + c);
      v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    if (mk) {
      const float4 m = *reinterpret_cast<const float4*>(mk + r * ms + c);
      v.x = m.x > 0.f ? v.x : v.x * slope; v.y = m.y > 0.f ? v.y : v.y * slope; v.z = m.z > 0.f ? v.z : v.z * slope; v.w = m.w > 0.f ? v.w : v.w * slope;
    }
    *reinterpret_cast<float4*>(d + r * ds + c) = v;
  }
}

// out[j] = sum over blocks b < nb of part[b * stride + j] (j < ncol): 32 columns per block, eight groups of threads each summing every
// eighth block in order (fp64), then the eight group sums in order -- a fixed order for a given nb
__global__ __launch_bounds__(256) void k_colsum(const float* __restrict__ part, int nb, int stride, int ncol, float* __restrict__ out) {
  __shared__ double red[8][32];
  const int jl = threadIdx.x & 31, g = threadIdx.x >> 5, j = blockIdx.x * 32 + jl;
  double s = 0.0;
  if (j < ncol)
    for (int b = g; b < nb; b += 8) s += (double)part[(long long)b * stride + j];
  red[g][jl] = s;
  __syncthreads();
  if (g == 0 && j < ncol) {
    for (int q = 1; q < 8; ++q) s += red[q][jl];
    out[j] = (float)s;
  }
}

// LayerNorm backward, y = LN(x + pe) * g + beta (pe row = (row / pe_div) % pe_rows, as k_layernorm reads it):
//   dx = rstd (dy g - mean(dy g) - xhat mean(dy g xhat)) (+ r)      r may alias dx
// and per-block partials part[block][0:C] = sum dy xhat (dgamma), part[block][C:2C] = sum dy (dbeta) over the block's rows.
template <int C>
__global__ __launch_bounds__(256) void k_ln_bwd(const float* __restrict__ x, int x_stride, const float* __restrict__ pe, int pe_stride, long long pe_rows,
                                                long long pe_div, const float* __restrict__ g, const float* __restrict__ dy, int dy_stride,
                                                const float* r, int r_stride, float* dx, int dx_stride, float* __restrict__ part, long long M, float eps) {
  constexpr int LPR = C / 4, RPB = 256 / LPR;
  __shared__ float red[RPB][2 * C];
  const int lr = threadIdx.x % LPR, rr = threadIdx.x / LPR;
  const float4 gv = *reinterpret_cast<const float4*>(g + lr * 4);
  float4 dg = make_float4(0.f, 0.f, 0.f, 0.f), db = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long long row = (long long)blockIdx.x * RPB + rr; row < M; row += (long long)gridDim.x * RPB) {
    float4 v = *reinterpret_cast<const float4*>(x + row * x_stride + lr * 4);
    if (pe) {
      const float4 q = *reinterpret_cast<const float4*>(pe + ((row / pe_div) % pe_rows) * pe_stride + lr * 4);
      v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    float s = v.x + v.y + v.z + v.w;
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, LPR);
    const float mu = s * (1.0f / C);
    const float ex = v.x - mu, ey = v.y - mu, ez = v.z - mu, ew = v.w - mu;
    float q2 = ex * ex + ey * ey + ez * ez + ew * ew;
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) q2 += __shfl_xor(q2, o, LPR);
    const float rstd = 1.0f / sqrtf(q2 * (1.0f / C) + eps);
    const float hx = ex * rstd, hy = ey * rstd, hz = ez * rstd, hw = ew * rstd;
    const float4 d = *reinterpret_cast<const float4*>(dy + row * dy_stride + lr * 4);
    dg.x += d.x * hx; dg.y += d.y * hy; dg.z += d.z * hz; dg.w += d.w * hw;
    db.x += d.x; db.y += d.y; db.z += d.z; db.w += d.w;
    const float gx = d.x * gv.x, gy = d.y * gv.y, gz = d.z * gv.z, gw = d.w * gv.w;
    float sg = gx + gy + gz + gw, sgx = gx * hx + gy * hy + gz * hz + gw * hw;
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) { sg += __shfl_xor(sg, o, LPR); sgx += __shfl_xor(sgx, o, LPR); }
    const float mg = sg * (1.0f / C), mgx = sgx * (1.0f / C);
    float4 o4 = make_float4(rstd * (gx - mg - hx * mgx), rstd * (gy - mg - hy * mgx), rstd * (gz - mg - hz * mgx), rstd * (gw - mg - hw * mgx));
    if (r) {
      const float4 rv = *reinterpret_cast<const float4*>(r + row * r_stride + lr * 4);
      o4.x += rv.x; o4.y += rv.y; o4.z += rv.z; o4.w += rv.w;
    }
    *reinterpret_cast<float4*>(dx + row * dx_stride + lr * 4) = o4;
  }
  red[rr][lr * 4] = dg.x; red[rr][lr * 4 + 1] = dg.y; red[rr][lr * 4 + 2] = dg.z; red[rr][lr * 4 + 3] = dg.w;
  red[rr][C + lr * 4] = db.x; red[rr][C + lr * 4 + 1] = db.y; red[rr][C + lr * 4 + 2] = db.z; red[rr][C + lr * 4 + 3] = db.w;
  __syncthreads();
  for (int j = threadIdx.x; j < 2 * C; j += 256) {
    float s = 0.f;
    for (int q = 0; q < RPB; ++q) s += red[q][j];
    part[(long long)blockIdx.x * 2 * C + j] = s;
  }
}

// dgrad pack of upsampling.0 with the rows in PyTorch order: out[k][c s2 + ij] = Wp[ij * 64 + c][k] (Wp: the forward's perm-1 pack, 64 s2 rows of 64)
__global__ __launch_bounds__(256) void k_pack_up0_T(const float* __restrict__ Wp, float* __restrict__ out, int s2) {
  const int i = blockIdx.x * 256 + threadIdx.x;   // over 64 * 64 s2
  const int N = 64 * s2;
  if (i >= 64 * N) return;
  const int n = i % N, k = i / N, c = n / s2, ij = n - c * s2;
  out[i] = Wp[(ij * 64 + c) * 64 + k];
}

// Tail backward: out = conv3x3(lrelu(HR), w3) + skip on the HR mosaic, HR = PixelShuffle(upsampling.0(f)) channel-last (B, A h s, A w s, 64).
// One thread per (LR VCL pixel p, channel c), walking the s^2 HR pixels of p:
//   dU[p][c s2 + ij] = (sum_t dout[P - off_t] w3[c][t]) * lrelu'(HR[P][c])       (the un-shuffled gradient of upsampling.0's output)
//   dw3[c][t] += lrelu(HR[P][c]) * dout[P - off_t]                               (per-block partials part[block][c * 9 + t])
__global__ __launch_bounds__(256) void k_tail_bwd(const float* __restrict__ dout, const float* __restrict__ w3, const float* __restrict__ hr,
                                                  float* __restrict__ du, float* __restrict__ part, int B, int A, int h, int w, int S, float slope) {
  __shared__ float red[4][9 * 64];
  const int c = threadIdx.x & 63, pl = threadIdx.x >> 6;
  float wc[9], acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) { wc[t] = w3[c * 9 + t]; acc[t] = 0.f; }
  const int s2 = S * S, AA = A * A;
  const long long npix = (long long)B * AA * h * w;
  const int Hs = A * h * S, Ws = A * w * S;
  for (long long p = (long long)blockIdx.x * 4 + pl; p < npix; p += (long long)gridDim.x * 4) {
    const int x = (int)(p % w);
    long long t = p / w;
    const int y = (int)(t % h);
    t /= h;
    const int view = (int)(t % AA);
    const long long b = t / AA;
    const int u = view / A, v = view - u * A;
    float dv[16];                                      // s^2 <= 16: the thread's s^2 outputs, stored together
#pragma unroll
    for (int ij = 0; ij < 16; ++ij) {
      if (ij >= s2) continue;
      const int i = ij / S, j = ij - i * S;
      const int Y = (u * h + y) * S + i, X = (v * w + x) * S + j;
      const float* dplane = dout + b * Hs * Ws;
      float d[9];
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) {
        const int yy = Y - (tp / 3 - 1), xx = X - (tp % 3 - 1);
        d[tp] = (yy >= 0 && yy < Hs && xx >= 0 && xx < Ws) ? dplane[(long long)yy * Ws + xx] : 0.f;
      }
      const float z = hr[((b * Hs + Y) * Ws + X) * 64 + c];
      const float act = z >= 0.f ? z : z * slope;      // as k_hr_tail forms it
      float da = 0.f;
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) { da = fmaf(d[tp], wc[tp], da); acc[tp] = fmaf(act, d[tp], acc[tp]); }
      dv[ij] = z > 0.f ? da : da * slope;
    }
    float* dst = du + p * 64 * s2 + c * s2;
    if ((s2 & 3) == 0) {
#pragma unroll
      for (int q = 0; q < 16; q += 4)
        if (q < s2) *reinterpret_cast<float4*>(dst + q) = make_float4(dv[q], dv[q + 1], dv[q + 2], dv[q + 3]);
    } else {
#pragma unroll
      for (int q = 0; q < 16; ++q)
        if (q < s2) dst[q] = dv[q];
    }
  }
#pragma unroll
  for (int tp = 0; tp < 9; ++tp) red[pl][c * 9 + tp] = acc[tp];
  __syncthreads();
  for (int jj = threadIdx.x; jj < 9 * 64; jj += 256) part[(long long)blockIdx.x * 9 * 64 + jj] = ((red[0][jj] + red[1][jj]) + red[2][jj]) + red[3][jj];
}

// ---- windowed attention backward ---------------------------------------------------------------------------------------------------
// The stride / window parametrisation of lfsr_window_attn_fwd: sequences (s0,s1,s2) start at pixel s0 bs0 + s1 bs1 + s2 bs2, token (t1,t2)
// sits at + t1 st1 + t2 st2 and attends keys [t1-l1, t1+r1) x [t2-l2, min(t2+r2, clip2, n2)).  P is recomputed from the saved q | k.
struct AttnBwdArgs {
  const float* Q; const float* K; int qk_stride, q_choff, k_choff;     // q and k in one buffer (the forward's q | k rows)
  const float* V; int v_stride;
  const float* O; const float* dO; int o_stride;                       // O and dO share a row stride
  float* dQK; float* dV;                                               // dQK: the layout of q | k; dV: the layout of V
  float4* stats;                                                       // per (query pixel, head): row max, 1 / denominator, rowsum(dO o O)
  int nheads;
  int ns1, ns2; long long bs0, bs1, bs2;
  int n1, n2; long long st1, st2;
  int l1, r1, l2, r2, clip2;
  float scale;
  long long total;
};

struct TokenPos { long long base; int t1, t2, head; };

__device__ __forceinline__ TokenPos attn_token(long long idx, const AttnBwdArgs& p) {
  TokenPos r;
  r.head = (int)(idx % p.nheads);
  long long t = idx / p.nheads;
  r.t2 = (int)(t % p.n2); t /= p.n2;
  r.t1 = (int)(t % p.n1); t /= p.n1;
  const int s2 = (int)(t % p.ns2); t /= p.ns2;
  const int s1 = (int)(t % p.ns1);
  const long long s0 = t / p.ns1;
  r.base = s0 * p.bs0 + s1 * p.bs1 + s2 * p.bs2;
  return r;
}

template <int HD>
__device__ __forceinline__ void load_row(const float* src, float (&v)[HD], float mul = 1.0f) {
  const float4* q = reinterpret_cast<const float4*>(src);
#pragma unroll
  for (int i = 0; i < HD / 4; ++i) {
    const float4 a = q[i];
    v[4 * i] = a.x * mul; v[4 * i + 1] = a.y * mul; v[4 * i + 2] = a.z * mul; v[4 * i + 3] = a.w * mul;
  }
}

template <int HD>
__device__ __forceinline__ float dot(const float (&a)[HD], const float* b) {
  const float4* q = reinterpret_cast<const float4*>(b);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < HD / 4; ++i) {
    const float4 v = q[i];
    s = fmaf(a[4 * i], v.x, s); s = fmaf(a[4 * i + 1], v.y, s); s = fmaf(a[4 * i + 2], v.z, s); s = fmaf(a[4 * i + 3], v.w, s);
  }
  return s;
}

// pass 1, one thread per (query, head): the softmax statistics, D = rowsum(dO o O) and dQ = scale sum_k P (dP - D) k
template <int HD>
__global__ __launch_bounds__(256) void k_attn_bwd_q(AttnBwdArgs p) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  const TokenPos tp = attn_token(idx, p);
  const long long qpix = tp.base + tp.t1 * p.st1 + tp.t2 * p.st2;
  const int hc = tp.head * HD;
  float q[HD], dO[HD], o[HD], dq[HD];
  load_row<HD>(p.Q + qpix * p.qk_stride + p.q_choff + hc, q, p.scale);
  load_row<HD>(p.dO + qpix * p.o_stride + hc, dO);
  load_row<HD>(p.O + qpix * p.o_stride + hc, o);
  float D = 0.f;
#pragma unroll
  for (int i = 0; i < HD; ++i) { D = fmaf(dO[i], o[i], D); dq[i] = 0.f; }
  const int a0 = max(0, tp.t1 - p.l1), a1 = min(p.n1, tp.t1 + p.r1);
  const int b0 = max(0, tp.t2 - p.l2), b1 = min(min(p.n2, p.clip2), tp.t2 + p.r2);
  float mx = -INFINITY, den = 0.f;     // the softmax statistics in one pass, as the forward forms them
  for (int k1 = a0; k1 < a1; ++k1)
    for (int k2 = b0; k2 < b1; ++k2) {
      const float sc = dot<HD>(q, p.K + (tp.base + k1 * p.st1 + k2 * p.st2) * p.qk_stride + p.k_choff + hc);
      const float mn = fmaxf(mx, sc);
      den = den * expf(mx - mn) + expf(sc - mn);
      mx = mn;
    }
  const float inv = 1.0f / den;
  for (int k1 = a0; k1 < a1; ++k1)
    for (int k2 = b0; k2 < b1; ++k2) {
      const long long kpix = tp.base + k1 * p.st1 + k2 * p.st2;
      const float* kr = p.K + kpix * p.qk_stride + p.k_choff + hc;
      const float pr = expf(dot<HD>(q, kr) - mx) * inv;
      const float ds = pr * (dot<HD>(dO, p.V + kpix * p.v_stride + hc) - D);
      float kv[HD];
      load_row<HD>(kr, kv);
#pragma unroll
      for (int i = 0; i < HD; ++i) dq[i] = fmaf(ds, kv[i], dq[i]);
    }
  float4* dst = reinterpret_cast<float4*>(p.dQK + qpix * p.qk_stride + p.q_choff + hc);
#pragma unroll
  for (int i = 0; i < HD / 4; ++i) dst[i] = make_float4(dq[4 * i] * p.scale, dq[4 * i + 1] * p.scale, dq[4 * i + 2] * p.scale, dq[4 * i + 3] * p.scale);
  p.stats[qpix * p.nheads + tp.head] = make_float4(mx, inv, D, 0.f);
}

// pass 2, one thread per (key, head): gathers over the queries whose window holds the key
//   dK = scale sum_q P (dP - D) q,   dV = sum_q P dO
template <int HD>
__global__ __launch_bounds__(256) void k_attn_bwd_kv(AttnBwdArgs p) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.total) return;
  const TokenPos tp = attn_token(idx, p);
  const long long kpix = tp.base + tp.t1 * p.st1 + tp.t2 * p.st2;
  const int hc = tp.head * HD;
  float k[HD], v[HD], dk[HD], dv[HD];
  load_row<HD>(p.K + kpix * p.qk_stride + p.k_choff + hc, k);
  load_row<HD>(p.V + kpix * p.v_stride + hc, v);
#pragma unroll
  for (int i = 0; i < HD; ++i) { dk[i] = 0.f; dv[i] = 0.f; }
  const int c1 = min(p.n1, tp.t1 + p.l1 + 1), c2 = min(p.n2, tp.t2 + p.l2 + 1);
  for (int q1 = max(0, tp.t1 - p.r1 + 1); q1 < c1; ++q1) {
    if (tp.t1 < q1 - p.l1 || tp.t1 >= min(p.n1, q1 + p.r1)) continue;
    for (int q2 = max(0, tp.t2 - p.r2 + 1); q2 < c2; ++q2) {
      if (tp.t2 < q2 - p.l2 || tp.t2 >= min(min(p.n2, p.clip2), q2 + p.r2)) continue;
      const long long qpix = tp.base + q1 * p.st1 + q2 * p.st2;
      float q[HD], dO[HD];
      load_row<HD>(p.Q + qpix * p.qk_stride + p.q_choff + hc, q, p.scale);
      load_row<HD>(p.dO + qpix * p.o_stride + hc, dO);
      const float4 sv = p.stats[qpix * p.nheads + tp.head];
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int i = 0; i < HD; ++i) { s = fmaf(q[i], k[i], s); dp = fmaf(dO[i], v[i], dp); }
      const float pr = expf(s - sv.x) * sv.y;
      const float ds = pr * (dp - sv.z);
#pragma unroll
      for (int i = 0; i < HD; ++i) { dk[i] = fmaf(ds, q[i], dk[i]); dv[i] = fmaf(pr, dO[i], dv[i]); }
    }
  }
  float4* dkp = reinterpret_cast<float4*>(p.dQK + kpix * p.qk_stride + p.k_choff + hc);
  float4* dvp = reinterpret_cast<float4*>(p.dV + kpix * p.v_stride + hc);
#pragma unroll
  for (int i = 0; i < HD / 4; ++i) {
    dkp[i] = make_float4(dk[4 * i], dk[4 * i + 1], dk[4 * i + 2], dk[4 * i + 3]);     // q was scaled on load
    dvp[i] = make_float4(dv[4 * i], dv[4 * i + 1], dv[4 * i + 2], dv[4 * i + 3]);
  }
}

}  // namespace

int lfsr_ew_launch(const float* a, int as, const float* b, int bs, const float* mk, int ms, float slope, float* d, int ds, int C, long long M, hipStream_t st) {
  hipLaunchKernelGGL(k_ew, dim3(lfsr_cap_grid(M * C / 4)), dim3(256), 0, st, a, as, b, bs, mk, ms, slope, d, ds, C, M);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

int lfsr_ln_bwd_launch(int C, const float* x, const float* pe, long long pe_rows, long long pe_div, const float* gamma, const float* dy, const float* r,
                       float* dx, float* part, long long M, float* dgamma, float* dbeta, hipStream_t st) {
  const int rpb = 256 / (C / 4);
  unsigned nb = lfsr_blocks(M, rpb);
  if (nb > LFSR_RED_BLOCKS) nb = LFSR_RED_BLOCKS;
  if (C == 64)
    hipLaunchKernelGGL(k_ln_bwd<64>, dim3(nb), dim3(256), 0, st, x, 64, pe, 64, pe_rows, pe_div, gamma, dy, 64, r, 64, dx, 64, part, M, 1e-5f);
  else
    hipLaunchKernelGGL(k_ln_bwd<128>, dim3(nb), dim3(256), 0, st, x, 128, pe, 128, pe_rows, pe_div, gamma, dy, 128, r, 128, dx, 128, part, M, 1e-5f);
  LFSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_colsum, dim3(C / 32), dim3(256), 0, st, part, (int)nb, 2 * C, C, dgamma);
  LFSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_colsum, dim3(C / 32), dim3(256), 0, st, part + C, (int)nb, 2 * C, C, dbeta);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

int lfsr_tail_bwd_launch(const float* dout, const float* w3, const float* hr, float* du, float* part, float* dw3, int B, int A, int h, int w, int S, float slope,
                         hipStream_t st) {
  const long long npix = (long long)B * A * A * h * w;
  unsigned nb = lfsr_blocks(npix, 4);
  if (nb > LFSR_RED_BLOCKS) nb = LFSR_RED_BLOCKS;
  hipLaunchKernelGGL(k_tail_bwd, dim3(nb), dim3(256), 0, st, dout, w3, hr, du, part, B, A, h, w, S, slope);
  LFSR_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_colsum, dim3(9 * 64 / 32), dim3(256), 0, st, part, (int)nb, 9 * 64, 9 * 64, dw3);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

int lfsr_pack_up0_T_launch(const float* Wp, float* out, int s2, hipStream_t st) {
  hipLaunchKernelGGL(k_pack_up0_T, dim3((64 * 64 * s2 + 255) / 256), dim3(256), 0, st, Wp, out, s2);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

int lfsr_attn_bwd_valu_launch(const LfsrAttnGrad& a, hipStream_t st) {
  const LfsrAttnGeom& g = a.g;
  if (a.hd != 8 && a.hd != 16) return LFSR_E_ARG;
  AttnBwdArgs p{};
  p.Q = a.qk; p.K = a.qk; p.qk_stride = a.qk_stride; p.q_choff = a.q_choff; p.k_choff = a.k_choff; p.V = a.v; p.v_stride = a.v_stride; p.O = a.o; p.dO = a.d_o;
  p.o_stride = a.o_stride; p.dQK = a.dqk; p.dV = a.dv; p.stats = reinterpret_cast<float4*>(a.stats); p.nheads = a.nheads;
  p.ns1 = g.ns1; p.ns2 = g.ns2; p.bs0 = g.bs0; p.bs1 = g.bs1; p.bs2 = g.bs2; p.n1 = g.n1; p.n2 = g.n2; p.st1 = g.st1; p.st2 = g.st2;
  p.l1 = g.l1; p.r1 = g.r1; p.l2 = g.l2; p.r2 = g.r2; p.clip2 = g.clip2;
  p.scale = 1.0f / sqrtf((float)a.hd);
  p.total = g.nseq() * g.tokens() * a.nheads;
  const unsigned grid = lfsr_blocks(p.total, 256);
  if (a.hd == 8) hipLaunchKernelGGL(k_attn_bwd_q<8>, dim3(grid), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(k_attn_bwd_q<16>, dim3(grid), dim3(256), 0, st, p);
  LFSR_CHECK_LAUNCH();
  if (a.hd == 8) hipLaunchKernelGGL(k_attn_bwd_kv<8>, dim3(grid), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(k_attn_bwd_kv<16>, dim3(grid), dim3(256), 0, st, p);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

namespace {
// Y (N columns) = X (M dense rows of cin) . WT, then * (Mk > 0 ? 1 : 0), then + R1: the 1x1 data gradient of the drivers and of lfsr_linear_dgrad.  Under
// lfsr_set_lin_grad_arithmetic(LFSR_LIN_GRAD_ARITH_BF16): lin_dgrad_bf16.hip where it covers the call (N in {64, 128, 256}, 16-B aligned operands)
int dgemm_launch(const float* X, int cin, const float* WT, float* Y, int ys, const float* R1, int r1s, const float* Mk, int mks, int M, int N, int A, int h, int w,
                 int S, hipStream_t st) {
  if (lfsr_lin_grad_arith_bf16()) {
    const int rc = lfsr_lin_dgrad_bf16_launch(X, cin, WT, Y, ys, R1, r1s, Mk, mks, M, N, st);
    if (rc != LFSR_E_ARG) return rc;
  }
  GemmArgs p{};
  p.X = X; p.x_stride = cin; p.Wp = WT; p.Y = Y; p.y_stride = ys; p.R1 = R1; p.r1_stride = r1s; p.Mk = Mk; p.mk_stride = mks; p.mk_slope = 0.0f;
  p.M = M; p.N = N; p.Npad = npad32(N); p.A = A; p.H = h; p.W = w; p.ntaps = 1; p.CH = N; p.slope = 1.0f; p.S = S;
  switch (cin) {
    case 64: return launch_gemm<IN_SAME, OUT_SAME, 64, 2>(p, st);
    case 128: return launch_gemm<IN_SAME, OUT_SAME, 128, 2>(p, st);
    case 256: return launch_gemm<IN_SAME, OUT_SAME, 256, 2>(p, st);
    case 576: return launch_gemm<IN_SAME, OUT_SAME, 576, 2>(p, st);
    case 1024: return launch_gemm<IN_SAME, OUT_SAME, 1024, 2>(p, st);
  }
  return LFSR_E_ARG;
}
}  // namespace

// ---- operator-level entry points over the launchers above (what the drivers call; tests/test_gpu_trans_bwd_ops.py) -------------------------
extern "C" size_t lfsr_layernorm_bwd_workspace_floats(int C) { return (C == 64 || C == 128) ? (size_t)LFSR_RED_BLOCKS * 2 * C : 0; }

extern "C" int lfsr_layernorm_bwd(const float* x, const float* pe, long long pe_rows, long long pe_div, const float* gamma, const float* dy, const float* r, float* dx,
                                  float* dgamma, float* dbeta, float* workspace, size_t workspace_floats, long long M, int C, void* stream) {
  if (!x || !gamma || !dy || !dx || !dgamma || !dbeta || !workspace || M <= 0 || (C != 64 && C != 128)) return LFSR_E_ARG;
  if (pe && (pe_rows <= 0 || pe_div <= 0)) return LFSR_E_ARG;
  if (workspace_floats < lfsr_layernorm_bwd_workspace_floats(C)) return LFSR_E_WS;
  return lfsr_ln_bwd_launch(C, x, pe, pe ? pe_rows : 1, pe ? pe_div : 1, gamma, dy, r, dx, workspace, M, dgamma, dbeta, lfsr_stream(stream));
}

extern "C" int lfsr_linear_dgrad(const float* dy, int cout, const float* wT_packed, float* dx, int dx_stride, const float* r1, int r1_stride, const float* act,
                                 int act_stride, long long M, int cin, void* stream) {
  if (!dy || !wT_packed || !dx || M <= 0 || M > 0x7fffffffLL - BM) return LFSR_E_ARG;      // the gather-GEMM counts rows, padded to its 128-row tile, in an int
  if (cout != 64 && cout != 128 && cout != 256 && cout != 576 && cout != 1024) return LFSR_E_ARG;
  if (cin != 64 && cin != 128 && cin != 256) return LFSR_E_ARG;
  if (dx_stride < cin || (dx_stride & 3) || (r1 && (r1_stride < cin || (r1_stride & 3))) || (act && (act_stride < cin || (act_stride & 3)))) return LFSR_E_ARG;
  return dgemm_launch(dy, cout, wT_packed, dx, dx_stride, r1, r1 ? r1_stride : 0, act, act ? act_stride : 0, (int)M, cin, 1, 1, 1, 1, lfsr_stream(stream));
}

// ---- a linear's weight gradient: the LINEAR form, as the operator and the drivers submit it --------------------------------------------------
static LfsrWgrad linear_wgrad(const float* dy, int dy_stride, const float* x, int x_stride, float* dw, long long M, int cout, int cin, int A, int h, int w) {
  LfsrWgrad g{};
  g.form = LFSR_WG_LINEAR; g.G = dy; g.g_stride = dy_stride; g.X = x; g.x_stride = x_stride; g.M = M; g.N = cout; g.K = cin; g.A = A; g.h = h; g.w = w; g.dW = dw;
  return g;
}

// one size for both modes: the default's slabs, or the bf16 form's full grid where that is more
extern "C" size_t lfsr_linear_wgrad_workspace_floats(long long M, int cout, int cin) {
  return lfsr_wgrad_part_floats(linear_wgrad(nullptr, 0, nullptr, 0, nullptr, M, cout, cin, 1, 1, 1), true);
}

extern "C" int lfsr_linear_wgrad(const float* dy, int dy_stride, const float* x, int x_stride, float* dw, float* workspace, size_t workspace_floats, long long M,
                                 int cout, int cin, int accumulate, void* stream) {
  const size_t need = lfsr_linear_wgrad_workspace_floats(M, cout, cin);      // 0: rows or shape not covered
  if (!dy || !x || !dw || !workspace || !need) return LFSR_E_ARG;
  if (dy_stride < cout || x_stride < cin || ((dy_stride | x_stride) & 3)) return LFSR_E_ARG;
  if (((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dw | (uintptr_t)workspace) & 15) return LFSR_E_ARG;
  if (workspace_floats < need) return LFSR_E_WS;
  LfsrWgrad g = linear_wgrad(dy, dy_stride, x, x_stride, dw, M, cout, cin, 1, 1, 1);
  g.accumulate = accumulate ? 1 : 0; g.part = workspace; g.part_floats = workspace_floats;
  return lfsr_wgrad_run(g, lfsr_stream(stream));
}

extern "C" size_t lfsr_up_tail_bwd_workspace_floats(void) { return (size_t)LFSR_RED_BLOCKS * 9 * 64; }

extern "C" int lfsr_up_tail_bwd(const float* dout, const float* w3, const float* hr, float* du, float* dw3, float* workspace, size_t workspace_floats, int B, int A,
                                int h, int w, int s, float slope, void* stream) {
  if (!dout || !w3 || !hr || !du || !dw3 || !workspace || B <= 0 || A <= 0 || h <= 0 || w <= 0 || s < 2 || s > 4) return LFSR_E_ARG;
  if ((long long)A * h * s > 0x7fffffffLL || (long long)A * w * s > 0x7fffffffLL || (long long)A * A > 0x7fffffffLL) return LFSR_E_ARG;   // k_tail_bwd keeps the mosaic's sides in ints
  if (workspace_floats < lfsr_up_tail_bwd_workspace_floats()) return LFSR_E_WS;
  return lfsr_tail_bwd_launch(dout, w3, hr, du, workspace, dw3, B, A, h, w, s, slope, lfsr_stream(stream));
}

extern "C" int lfsr_pack_up0_weight_tr(const float* w_packed, float* out, int s, void* stream) {
  if (!w_packed || !out || s < 2 || s > 4) return LFSR_E_ARG;
  return lfsr_pack_up0_T_launch(w_packed, out, s * s, lfsr_stream(stream));
}

// ---- the drivers' shared host code ---------------------------------------------------------------------------------------------------
bool lfsr_trans_train_geometry_ok(int A, int s, int B, int h, int w) {
  if (B <= 0 || h <= 0 || w <= 0 || s < 2 || s > 4) return false;
  const long long npix = (long long)B * A * A * h * w;
  const long long widest = 64LL * s * s > 256 ? 64LL * s * s : 256;
  return npix * widest * 4 < (1LL << 31);
}

size_t lfsr_trans_wgrad_partial_max(int B, int A, int h, int w) {
  const long long npix = (long long)B * A * A * h * w;
  // the 64 -> 64 3x3 convs as EPIT / LFT submit them: the GATHER form, not CONV3 -- the Winograd kernel would change bits and speed; conv_init0 on its 9 gathered taps
  size_t m = std::max(lfsr_wgrad_part_floats(lfsr_wgrad_gather(LFSR_IN_SAME, LFSR_IN_CONV3, npix, 64, 64, 9, A, h, w)),
                      lfsr_wgrad_part_floats(lfsr_wgrad_gather(LFSR_IN_SAME, LFSR_IN_SAME, npix, 64, 16, 1, A, h, w)));
  auto lin = [&](int O, int K) { m = std::max(m, lfsr_wgrad_part_floats(linear_wgrad(nullptr, 0, nullptr, 0, nullptr, npix, O, K, A, h, w))); };
  for (int E : {64, 128}) { lin(E, 2 * E); lin(2 * E, E); lin(E, E); }      // the sublayers' and the drivers' own linears
  for (int s : {2, 3, 4}) lin(64 * s * s, 64);                               // upsampling.0
  return m;
}

float* LfsrTransBwd::G(const std::string& k) const { return gbase + P.grad_off(k); }

int LfsrTransBwd::dgemm(const float* X, int cin, const float* WT, float* Y, int ys, const float* R1, int r1s, const float* Mk, int mks, int N) const {
  return dgemm_launch(X, cin, WT, Y, ys, R1, r1s, Mk, mks, npix, N, A, h, w, S, st);
}

int LfsrTransBwd::wgrad(int xm, const float* Gr, int gs, int go, const float* X, int xs, int M, int N, int K, int ntaps, float* dW, int accumulate,
                        int c_valid) const {
  LfsrWgrad g = lfsr_wgrad_gather(LFSR_IN_SAME, xm, M, N, K, ntaps, A, h, w);
  g.G = Gr; g.g_stride = gs; g.g_choff = go; g.X = X; g.x_stride = xs;
  g.dW = dW; g.accumulate = accumulate; g.c_valid = c_valid; g.part = ws.part; g.part_floats = ws.part_floats;
  return lfsr_wgrad_run(g, st);
}

int LfsrTransBwd::wgrad_lin(const float* Gr, int gs, int O, const float* X, int xs, int K, float* dW) const {
  LfsrWgrad g = linear_wgrad(Gr, gs, X, xs, dW, npix, O, K, A, h, w);
  g.part = ws.part; g.part_floats = ws.part_floats;
  return lfsr_wgrad_run(g, st);
}

int LfsrTransBwd::ew(int C, const float* a, const float* b, const float* mk, float slope, float* d) const {
  return lfsr_ew_launch(a, C, b, C, mk, C, slope, d, C, C, npix, st);
}

int LfsrTransBwd::ln_bwd(int C, const float* X, const float* pe, long long pe_rows, long long pe_div, const std::string& gkey, const std::string& bkey,
                         const float* dy, const float* r, float* dxo) const {
  return lfsr_ln_bwd_launch(C, X, pe, pe_rows, pe_div, P.w(gkey), dy, r, dxo, ws.pln, npix, G(gkey), G(bkey), st);
}

int LfsrTransBwd::dgrad3(const float* dy, int dys, int dyo, const float* wT, float* dxo, const float* r1, const float* mk) const {
  return lfsr_conv3x3_bwd_data(dy, dys, dyo, wT, dxo, 64, 0, r1, 64, 0, mk, 64, 0, L, nimg, h, w, st);
}

int LfsrTransBwd::packT(const float* Wp, int n0, int C, int O, float* o) const { return lfsr_pack_T_from_fwd(Wp + (size_t)n0 * C, o, 1, O, C, O, 0, C, 0, st); }

int LfsrTransBwd::pack3T(const std::string& key, float* o) const {
  LFSR_RC(lfsr_pack_T_from_fwd(P.w(key), o, 9, 64, 64, 64, 0, 64, 1, st));
  return lfsr_pack_wino_m(o, o + LFSR_CONV3_WINO2_OFF, LFSR_W_ALL, st);   // the 64 -> 64 3x3 data gradient's Winograd copies
}

// upsampling.0 (1x1 64 -> 64 s^2), PixelShuffle(s), LeakyReLU 0.2, 3x3 conv 64 -> 1, + bicubic skip (no parameters)
int lfsr_trans_tail_bwd(const LfsrTransBwd& k, const float* dout, const float* xin, float* dX) {
  const LfsrTransBwdWs& s = k.ws;
  const int s2 = k.S * k.S;
  LFSR_RC(lfsr_upsample_ps_fwd(xin, 64, 0, k.P.w("upsampling.0.weight"), s.hr, k.B, k.A, k.h, k.w, k.S, k.st));   // the HR pre-activation, rebuilt
  LFSR_RC(lfsr_tail_bwd_launch(dout, k.P.w("upsampling.3.weight"), s.hr, s.du, s.ptail, k.G("upsampling.3.weight"), k.B, k.A, k.h, k.w, k.S, k.L, k.st));
  LFSR_RC(lfsr_pack_up0_T_launch(k.P.w("upsampling.0.weight"), s.up0T, s2, k.st));
  LFSR_RC(k.dgemm(s.du, 64 * s2, s.up0T, dX, 64, nullptr, 0, nullptr, 0, 64));
  return k.wgrad_lin(s.du, 64 * s2, 64 * s2, xin, 64, 64, k.G("upsampling.0.weight"));
}

// buf0 = lrelu(conv_init.4(c2)) + f0, c2 = lrelu(conv_init.2(c1)), c1 = lrelu(conv_init.0(f0)), f0 = conv_init0(x)
int lfsr_trans_head_bwd(const LfsrTransBwd& k, const float* x, const float* f0, const float* c1, const float* c2, const float* dbuf0) {
  const LfsrTransBwdWs& s = k.ws;
  LFSR_RC(k.pack3T("conv_init.0.weight", s.initT[0]));
  LFSR_RC(k.pack3T("conv_init.2.weight", s.initT[1]));
  LFSR_RC(k.pack3T("conv_init.4.weight", s.initT[2]));
  // conv_init.4's LeakyReLU output without the residual, for its mask (the forward's launch minus r1)
  LFSR_RC(lfsr_conv3x3_fwd(c2, 64, 0, k.P.w("conv_init.4.weight"), s.r4, 64, 0, nullptr, 0, 0, nullptr, 0, 0, k.nimg, k.h, k.w, k.L, k.st));
  LFSR_RC(k.ew(64, dbuf0, nullptr, s.r4, k.L, s.d64));
  LFSR_RC(k.wgrad(LFSR_IN_CONV3, s.d64, 64, 0, c2, 64, k.npix, 64, 64, 9, k.G("conv_init.4.weight"), 0));
  LFSR_RC(k.dgrad3(s.d64, 64, 0, s.initT[2], s.t64, nullptr, c2));
  LFSR_RC(k.wgrad(LFSR_IN_CONV3, s.t64, 64, 0, c1, 64, k.npix, 64, 64, 9, k.G("conv_init.2.weight"), 0));
  LFSR_RC(k.dgrad3(s.t64, 64, 0, s.initT[1], s.d64, nullptr, c1));
  LFSR_RC(k.wgrad(LFSR_IN_CONV3, s.d64, 64, 0, f0, 64, k.npix, 64, 64, 9, k.G("conv_init.0.weight"), 0));
  LFSR_RC(k.dgrad3(s.d64, 64, 0, s.initT[0], s.t64, dbuf0, nullptr));
  LFSR_RC(lfsr_init_gather9(x, s.xg9, k.B, k.A, k.h, k.w, k.st));
  return k.wgrad(LFSR_IN_SAME, s.t64, 64, 0, s.xg9, 16, k.npix, 64, 16, 1, k.G("conv_init0.0.weight"), 0, 9);
}

int lfsr_trans_sublayer_packs(const LfsrTransBwd& k, const std::string& pre, int E, float* const* lin) {
  LFSR_RC(k.packT(k.P.w(pre + "feed_forward.4.weight"), 0, 2 * E, E, lin[0]));
  LFSR_RC(k.packT(k.P.w(pre + "feed_forward.1.weight"), 0, E, 2 * E, lin[1]));
  LFSR_RC(k.packT(k.P.w(pre + "attention.out_proj.weight"), 0, E, E, lin[2]));
  LFSR_RC(k.packT(k.P.w(pre + "attention.in_proj_weight"), 0, E, 2 * E, lin[3]));
  return k.packT(k.P.w(pre + "attention.in_proj_weight"), 2 * E, E, E, lin[4]);
}

int lfsr_trans_sublayer_bwd(const LfsrTransBwd& k, const std::string& pre, int E, const float* dy, const float* x2, const float* ao, const float* qk,
                            const float* v, const float* tok, const float* pe, long long pe_rows, long long pe_div, float* hid, float* const* lin,
                            const LfsrAttnBwdCallback& attn, float* dtok, const float* ln_r, float* ln_dx) {
  const LfsrParamTable& P = k.P;
  const LfsrTransBwdWs& s = k.ws;
  // the feed-forward: its LayerNorm (into lnt) and hidden rows are recomputed
  LFSR_RC(lfsr_layernorm_fwd(x2, E, 0, nullptr, 0, 0, 1, P.w(pre + "feed_forward.0.weight"), P.w(pre + "feed_forward.0.bias"), s.lnt, E, 0, k.npix, E, 1e-5f, k.st));
  LFSR_RC(lfsr_linear_fwd(s.lnt, E, 0, E, P.w(pre + "feed_forward.1.weight"), nullptr, nullptr, 0, 0, hid, 2 * E, 0, k.npix, 2 * E, 0.0f, k.st));   // ReLU(hidden)
  LFSR_RC(k.wgrad_lin(dy, E, E, hid, 2 * E, 2 * E, k.G(pre + "feed_forward.4.weight")));
  LFSR_RC(k.dgemm(dy, E, lin[0], s.dh, 2 * E, nullptr, 0, hid, 2 * E, 2 * E));
  LFSR_RC(k.wgrad_lin(s.dh, 2 * E, 2 * E, s.lnt, E, E, k.G(pre + "feed_forward.1.weight")));
  LFSR_RC(k.dgemm(s.dh, 2 * E, lin[1], s.dln, E, nullptr, 0, nullptr, 0, E));
  LFSR_RC(k.ln_bwd(E, x2, nullptr, 1, 1, pre + "feed_forward.0.weight", pre + "feed_forward.0.bias", s.dln, dy, s.dsm));   // dsm = dL/d x2
  LFSR_RC(k.dgemm(s.dsm, E, lin[2], s.dso, E, nullptr, 0, nullptr, 0, E));
  LFSR_RC(k.wgrad_lin(s.dsm, E, E, ao, E, E, k.G(pre + "attention.out_proj.weight")));
  LFSR_RC(attn(qk, v, ao, s.dso, s.dqk, s.dv));
  // the in-projection: its LayerNorm is recomputed
  LFSR_RC(lfsr_layernorm_fwd(tok, E, 0, pe, pe ? E : 0, pe ? pe_rows : 0, pe_div, P.w(pre + "norm.weight"), P.w(pre + "norm.bias"), s.lnt, E, 0, k.npix, E, 1e-5f, k.st));
  float* dWin = k.G(pre + "attention.in_proj_weight");
  LFSR_RC(k.wgrad_lin(s.dqk, 2 * E, 2 * E, s.lnt, E, E, dWin));
  LFSR_RC(k.wgrad_lin(s.dv, E, E, tok, E, E, dWin + 2 * E * E));
  LFSR_RC(k.dgemm(s.dqk, 2 * E, lin[3], s.dln, E, nullptr, 0, nullptr, 0, E));
  LFSR_RC(k.dgemm(s.dv, E, lin[4], dtok, E, s.dsm, E, nullptr, 0, E));
  return k.ln_bwd(E, tok, pe, pe_rows, pe_div, pre + "norm.weight", pre + "norm.bias", s.dln, ln_r, ln_dx);
}
