// LFT training: the forward that keeps what the backward reads, and the backward (autograd of model/SR/LFT.py:67-98 as driven by
// train.py:256-264, fp32; the graph of oracle/lfsr_torch_port.py::lft_forward is the spec).  Rows are VCL pixels as in the forward (lft.cpp).
//
// forward_train runs lfsr_lft_forward_body, the inference forward's launches, on buffers of its own per layer: the AltFilter inputs, the
// attention's q | k, v and output, the feed-forward inputs and outputs and the spatial tokens.  The fused launches keep no LayerNorm
// statistics, feed-forward hidden rows or HR map: the backward recomputes those from the saved sublayer inputs with the unfused kernels.
//
// Backward: data gradients are gather-GEMMs over transposed packs (gemm_gather_kernel.h) and the 64 -> 64 3x3 data-gradient kernel;
// weight gradients are the two-pass partial-slab reduction of wgrad.hip.  New kernels: the windowed attention backward (two gathers, one
// per query and one per key: no float atomics), the LayerNorm backward with the position embedding added to its input, the tail's
// LeakyReLU / 3x3 conv backward with the HR -> LR un-shuffle, and small fixed-order reductions.  Buckets are bitwise reproducible.
#include <string>
#include <vector>

#include "gemm_gather_kernel.h"
#include "lft_ctx.h"

namespace {

inline unsigned cap_grid(long long total, unsigned cap = 8192) {
  unsigned g = lfsr_blocks(total, 256);
  return g > cap ? cap : g;
}

constexpr int RED_BLOCKS = 1024;   // fixed grid of the kernels that write per-block partials (a fixed order for every geometry)

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

// dspe[p][c] = sum over the n_img images of dln[img * HW + p][c] (128 channels), in image order
__global__ __launch_bounds__(256) void k_pe_reduce(const float* __restrict__ dln, float* __restrict__ dspe, int n_img, int HW) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)HW * 128) return;
  float s = 0.f;
  for (int i = 0; i < n_img; ++i) s += dln[(long long)i * HW * 128 + e];
  dspe[e] = s;
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

// ---- workspace ------------------------------------------------------------------------------------------------------------------
inline size_t tr3_floats() { return lfsr_packed_weight_tr_floats(64, 64, 9); }

struct LftTrainWs {
  LftFwdBufs f;                       // saved by forward_train (the scratch members point into the backward scratch below)
  // backward scratch
  float *hr, *du, *dx[2], *dbuf0, *dsf, *dh, *dln, *dln2, *dsm, *dso, *dqk, *dv, *dst, *lnt, *hid, *d64, *t64, *dspe, *xg9, *r4;
  std::vector<float*> hid_a, hid_s;   // the feed-forward hidden rows (after the ReLU) the backward rebuilt, per layer: its ReLU decisions
  float4* stats;
  float *part, *pln, *ptail;
  // transposed packs, rebuilt from the current packed weights by every backward
  float *up0T, *initT[3];
  std::vector<float*> mloT, mhiT;
  float* lin[11];                     // one layer's 1x1 dgrad packs (rebuilt for every layer): see the backward
};

size_t wgrad_partial_max(int B, int A, int h, int w) {
  const size_t npix = (size_t)B * A * A * h * w;
  size_t m = 0;
  auto up = [&](size_t v) { if (v > m) m = v; };
  for (int K : {16, 64, 128, 256}) up(lfsr_wgrad_partial_floats((int)npix, 1, 64, K));
  up(lfsr_wgrad_partial_floats((int)npix, 9, 64, 64));
  up(lfsr_wgrad_partial_floats(h * w, 9, 64, 64));
  return m;
}

// geometry the training path covers: every activation below 2 GiB (the forward's bound on the 256-float q | k rows, and the HR map of 64 s^2
// floats per LR pixel that the backward rebuilds)
bool train_geometry_ok(const lfsr_lft* c, int B, int h, int w) {
  if (!c || B <= 0 || h <= 0 || w <= 0 || c->s < 2 || c->s > 4) return false;
  const long long npix = (long long)B * c->A * c->A * h * w;
  const long long widest = 64LL * c->s * c->s > 256 ? 64LL * c->s * c->s : 256;
  return npix * widest * 4 < (1LL << 31);
}

void train_layout(const lfsr_lft* c, int B, int h, int w, LfsrArena& ws, LftTrainWs& t) {
  const int nl = c->nlayer, s2 = c->s * c->s;
  const size_t npix = (size_t)B * c->A * c->A * h * w, HW = (size_t)h * w;
  LftFwdBufs& f = t.f;
  f.f0 = ws.take(npix * 64); f.c1 = ws.take(npix * 64); f.c2 = ws.take(npix * 64); f.buf0 = ws.take(npix * 64);
  f.spos = ws.take(HW * 64); f.ape = ws.take((size_t)c->A * c->A * 64);
  f.x.assign(nl + 1, nullptr);
  f.x[0] = f.buf0;
  for (int b = 0; b < nl; ++b) {
    f.aqk.push_back(ws.take(npix * 128)); f.av.push_back(ws.take(npix * 64)); f.ao.push_back(ws.take(npix * 64)); f.am.push_back(ws.take(npix * 64));
    f.ay.push_back(ws.take(npix * 64));
    f.st.push_back(ws.take(npix * 128)); f.spe.push_back(ws.take(HW * 128)); f.sqk.push_back(ws.take(npix * 256)); f.sv.push_back(ws.take(npix * 128));
    f.so.push_back(ws.take(npix * 128)); f.sm.push_back(ws.take(npix * 128)); f.sf.push_back(ws.take(npix * 128));
    f.x[b + 1] = ws.take(npix * 64);
  }
  t.hr = ws.take(npix * 64 * s2); t.du = ws.take(npix * 64 * s2);
  t.dx[0] = ws.take(npix * 64); t.dx[1] = ws.take(npix * 64); t.dbuf0 = ws.take(npix * 64);
  t.dsf = ws.take(npix * 128); t.dh = ws.take(npix * 256); t.dln = ws.take(npix * 128); t.dln2 = ws.take(npix * 128); t.dsm = ws.take(npix * 128);
  t.dso = ws.take(npix * 128); t.dqk = ws.take(npix * 256); t.dv = ws.take(npix * 128); t.dst = ws.take(npix * 128); t.lnt = ws.take(npix * 128);
  t.hid = ws.take(npix * 256); t.r4 = ws.take(npix * 64); t.d64 = ws.take(npix * 64); t.t64 = ws.take(npix * 64); t.dspe = ws.take(HW * 128); t.xg9 = ws.take(npix * 16);
  t.stats = reinterpret_cast<float4*>(ws.take(npix * 8 * 4));
  t.hid_a.clear(); t.hid_s.clear();
  for (int b = 0; b < nl; ++b) { t.hid_a.push_back(ws.take(npix * 128)); t.hid_s.push_back(ws.take(npix * 256)); }
  t.part = ws.take(wgrad_partial_max(B, c->A, h, w)); t.pln = ws.take((size_t)RED_BLOCKS * 256); t.ptail = ws.take((size_t)RED_BLOCKS * 9 * 64);
  // the forward body's scratch (unfused LayerNorm outputs, two-launch feed-forward hidden rows, the unfused tail's HR map)
  f.n64 = t.t64; f.tn = t.lnt; f.lnf = t.dln2; f.ha = t.dh; f.hs = t.hid; f.hr = t.hr;
  t.up0T = ws.take((size_t)64 * 64 * s2);
  for (int i = 0; i < 3; ++i) t.initT[i] = ws.take(tr3_floats());
  t.mloT.clear(); t.mhiT.clear();
  for (int b = 0; b < nl; ++b) { t.mloT.push_back(ws.take(tr3_floats())); t.mhiT.push_back(ws.take(tr3_floats())); }
  for (float*& l : t.lin) l = ws.take(256 * 128);       // the largest: [128][256]
}

}  // namespace

extern "C" {

// the gradient bucket: state_dict order (LFT.py module creation order; AltFilter creates spa_trans before ang_trans); MLP.weight#lo / #hi are internal
size_t lfsr_lft_num_params(const lfsr_lft* c) { return c ? c->P.num_params() : 0; }

int lfsr_lft_param_offset(const lfsr_lft* c, const char* key, size_t* off, size_t* numel) { return c ? c->P.param_offset(key, off, numel) : LFSR_E_ARG; }

size_t lfsr_lft_train_workspace_bytes(const lfsr_lft* c, int B, int h, int w) {
  if (!train_geometry_ok(c, B, h, w)) return 0;
  LfsrArena ws;
  LftTrainWs t;
  train_layout(c, B, h, w, ws, t);
  return ws.bytes();
}

// which: 0 the input of AltFilter `index` (index = n_layer: the altblock output plus its skip, the tail's input), 1 the angular feed-forward
// input of layer `index` (out_proj + token), 2 the spatial feed-forward input, 3 the spatial tokens (the MLP output), 4 the spatial
// feed-forward output (linear.0's input): VCL rows of 64 (0, 1) or 128 (2 - 4) floats; 5 conv_init's LeakyReLU outputs (index 0: stage
// conv_init.0, 1: conv_init.2; 64).  After a backward, what it rebuilt and took its ReLU / LeakyReLU decisions from: 6 the angular (128)
// and 7 the spatial (256) feed-forward hidden rows after the ReLU of layer `index`, 8 conv_init.4's LeakyReLU output without the residual
// (64; index 0), 9 the HR pre-activation (the channel-last mosaic (B, A h s, A w s, 64); index 0).
int lfsr_lft_train_saved(const lfsr_lft* c, int B, int h, int w, int which, int index, size_t* offset_floats, size_t* numel) {
  if (!train_geometry_ok(c, B, h, w) || !offset_floats || !numel || index < 0) return LFSR_E_ARG;
  const int nl = c->nlayer;
  if (index >= (which == 0 ? nl + 1 : which == 5 ? 2 : which >= 8 ? 1 : nl)) return LFSR_E_ARG;
  LfsrArena ws = LfsrArena::offsets();
  LftTrainWs t;
  train_layout(c, B, h, w, ws, t);
  const size_t npix = (size_t)B * c->A * c->A * h * w;
  const float* p = nullptr;
  size_t n = npix * 128;
  switch (which) {
    case 0: p = t.f.x[index]; n = npix * 64; break;
    case 1: p = t.f.am[index]; n = npix * 64; break;
    case 2: p = t.f.sm[index]; break;
    case 3: p = t.f.st[index]; break;
    case 4: p = t.f.sf[index]; break;
    case 5: p = index ? t.f.c2 : t.f.c1; n = npix * 64; break;
    case 6: p = t.hid_a[index]; break;
    case 7: p = t.hid_s[index]; n = npix * 256; break;
    case 8: p = t.r4; n = npix * 64; break;
    case 9: p = t.hr; n = npix * 64 * c->s * c->s; break;
    default: return LFSR_E_ARG;
  }
  *offset_floats = ws.offset(p);
  *numel = n;
  return LFSR_OK;
}

int lfsr_lft_forward_train(lfsr_lft* c, const float* x, float* out, int B, int h, int w, void* workspace, size_t workspace_bytes, void* stream) {
  if (!c || !c->run_args_ok(x, out, B, h, w, workspace) || !train_geometry_ok(c, B, h, w)) return LFSR_E_ARG;
  LfsrArena ws(workspace);
  LftTrainWs t;
  train_layout(c, B, h, w, ws, t);
  if (workspace_bytes < ws.bytes()) return LFSR_E_WS;
  return lfsr_lft_forward_body(c, x, out, B, h, w, t.f, stream);
}

int lfsr_lft_backward(lfsr_lft* c, const float* x, const float* dout, int B, int h, int w, void* workspace, size_t workspace_bytes,
                      float* grads, size_t n_grads, void* stream) {
  if (!c || !c->run_args_ok(x, dout, B, h, w, workspace) || !grads || !train_geometry_ok(c, B, h, w) || n_grads != c->P.num_params()) return LFSR_E_ARG;
  LfsrArena ws(workspace);
  LftTrainWs t;
  train_layout(c, B, h, w, ws, t);
  if (workspace_bytes < ws.bytes()) return LFSR_E_WS;
  const int A = c->A, AA = A * A, S = c->s, s2 = S * S, nimg = B * AA, HW = h * w, nl = c->nlayer;
  const int npix = nimg * HW;
  const float L = 0.2f;
  const LfsrParamTable& P = c->P;
  const LftFwdBufs& f = t.f;
  hipStream_t st = lfsr_stream(stream);
  auto G = [&](const std::string& k) -> float* { return grads + P.grad_off(k); };
  auto launched = [&]() -> int { LFSR_CHECK_LAUNCH(); return LFSR_OK; };
  // 1x1 data gradient Y (N columns) = X (CIN columns) . WT, then * (Mk > 0 ? 1 : 0) (ReLU'), then + R1 (may alias Y)
  auto dgemm = [&](auto launcher, const float* X, int xs, const float* WT, float* Y, int ys, const float* R1, int r1s, const float* Mk, int mks, int N) -> int {
    GemmArgs p{};
    p.X = X; p.x_stride = xs; p.Wp = WT; p.Y = Y; p.y_stride = ys; p.R1 = R1; p.r1_stride = r1s; p.Mk = Mk; p.mk_stride = mks; p.mk_slope = 0.0f;
    p.M = npix; p.N = N; p.Npad = npad32(N); p.A = A; p.H = h; p.W = w; p.ntaps = 1; p.CH = N; p.slope = 1.0f; p.S = S;
    return launcher(p, st);
  };
  // weight gradient of output rows [n0, n0 + N) (N <= 64) of a raw (O, C, T) weight: partial slabs, then the fixed-order reduce
  auto wgrad = [&](int xm, const float* Gr, int gs, int go, const float* X, int xs, int M, int N, int K, int ntaps, float* dW, int accumulate,
                   int c_valid = 0) -> int {
    int r = lfsr_wgrad_launch(LFSR_IN_SAME, xm, Gr, gs, go, X, xs, 0, t.part, M, N, K, A, h, w, ntaps, st);
    if (!r) r = lfsr_wgrad_reduce(t.part, lfsr_wgrad_splits(M, ntaps, K), nullptr, 0, dW, N, K, ntaps, 0, 0, accumulate, c_valid, 0, st);
    return r;
  };
  // every 64-row slice of a (O, K) linear weight's gradient: G (O columns, stride gs) against X (K columns)
  auto wgrad_lin = [&](const float* Gr, int gs, int O, const float* X, int xs, int K, float* dW) -> int {
    for (int n0 = 0; n0 < O; n0 += 64) {
      const int r = wgrad(LFSR_IN_SAME, Gr, gs, n0, X, xs, npix, 64, K, 1, dW + (size_t)n0 * K, 0);
      if (r) return r;
    }
    return LFSR_OK;
  };
  auto ew = [&](const float* a, int as, const float* b, int bs, const float* mk, int ms, float slope, float* d, int ds, int C, long long M) -> int {
    hipLaunchKernelGGL(k_ew, dim3(cap_grid(M * C / 4)), dim3(256), 0, st, a, as, b, bs, mk, ms, slope, d, ds, C, M);
    return launched();
  };
  // LayerNorm backward with the gradients of its affine parameters written to dg / dbeta
  auto ln_bwd = [&](int C, const float* X, const float* pe, long long pe_rows, long long pe_div, const std::string& gkey, const std::string& bkey,
                    const float* dy, const float* r, float* dxo) -> int {
    const int rpb = 256 / (C / 4);
    unsigned nb = lfsr_blocks(npix, rpb);
    if (nb > RED_BLOCKS) nb = RED_BLOCKS;
    if (C == 64)
      hipLaunchKernelGGL(k_ln_bwd<64>, dim3(nb), dim3(256), 0, st, X, 64, pe, 64, pe_rows, pe_div, P.w(gkey), dy, 64, r, 64, dxo, 64, t.pln, (long long)npix, 1e-5f);
    else
      hipLaunchKernelGGL(k_ln_bwd<128>, dim3(nb), dim3(256), 0, st, X, 128, pe, 128, pe_rows, pe_div, P.w(gkey), dy, 128, r, 128, dxo, 128, t.pln, (long long)npix, 1e-5f);
    LFSR_RC(launched());
    hipLaunchKernelGGL(k_colsum, dim3(C / 32), dim3(256), 0, st, t.pln, (int)nb, 2 * C, C, G(gkey));
    LFSR_RC(launched());
    hipLaunchKernelGGL(k_colsum, dim3(C / 32), dim3(256), 0, st, t.pln + C, (int)nb, 2 * C, C, G(bkey));
    return launched();
  };
  auto attn_bwd = [&](int hd, const float* qk, int qks, int kchoff, const float* V, int vs, const float* O, const float* dO, int os, float* dqk, float* dv,
                      int ns0, int ns1, int ns2, long long bs0, long long bs1, long long bs2, int n1, int n2, long long st1, long long st2,
                      int l1, int r1, int l2, int r2, int clip2) -> int {
    AttnBwdArgs p{};
    p.Q = qk; p.K = qk; p.qk_stride = qks; p.q_choff = 0; p.k_choff = kchoff; p.V = V; p.v_stride = vs; p.O = O; p.dO = dO; p.o_stride = os;
    p.dQK = dqk; p.dV = dv; p.stats = t.stats; p.nheads = 8;
    p.ns1 = ns1; p.ns2 = ns2; p.bs0 = bs0; p.bs1 = bs1; p.bs2 = bs2; p.n1 = n1; p.n2 = n2; p.st1 = st1; p.st2 = st2;
    p.l1 = l1; p.r1 = r1; p.l2 = l2; p.r2 = r2; p.clip2 = clip2 > 0 ? clip2 : n2;
    p.scale = 1.0f / sqrtf((float)hd);
    p.total = (long long)ns0 * ns1 * ns2 * n1 * n2 * 8;
    const unsigned grid = lfsr_blocks(p.total, 256);
    if (hd == 8) hipLaunchKernelGGL(k_attn_bwd_q<8>, dim3(grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_attn_bwd_q<16>, dim3(grid), dim3(256), 0, st, p);
    LFSR_RC(launched());
    if (hd == 8) hipLaunchKernelGGL(k_attn_bwd_kv<8>, dim3(grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(k_attn_bwd_kv<16>, dim3(grid), dim3(256), 0, st, p);
    return launched();
  };
  auto dgrad3 = [&](const float* dy, int dys, int dyo, const float* wT, float* dxo, const float* r1, const float* mk) -> int {
    return lfsr_conv3x3_bwd_data(dy, dys, dyo, wT, dxo, 64, 0, r1, 64, 0, mk, 64, 0, L, nimg, h, w, st);
  };
  // 1x1 dgrad pack of rows [n0, n0 + O) of a (Npad_in, C) forward pack: [C][O]
  auto packT = [&](const float* Wp, int n0, int C, int O, float* o) -> int { return lfsr_pack_T_from_fwd(Wp + (size_t)n0 * C, o, 1, O, C, O, 0, C, 0, st); };
  auto pack3T = [&](const std::string& key, float* o) -> int {
    LFSR_RC(lfsr_pack_T_from_fwd(P.w(key), o, 9, 64, 64, 64, 0, 64, 1, st));
    return lfsr_pack_wino_m(o, o + LFSR_CONV3_WINO2_OFF, LFSR_W_ALL, st);   // the 64 -> 64 3x3 data gradient's Winograd copies
  };

  // ---- tail: upsampling.0 (1x1 64 -> 64 s^2), PixelShuffle(s), LeakyReLU 0.2, 3x3 conv 64 -> 1, + bicubic skip (no parameters) ----------
  LFSR_RC(lfsr_upsample_ps_fwd(f.x[nl], 64, 0, P.w("upsampling.0.weight"), t.hr, B, A, h, w, S, stream));   // the HR pre-activation, rebuilt
  {
    unsigned nb = lfsr_blocks(npix, 4);
    if (nb > RED_BLOCKS) nb = RED_BLOCKS;
    hipLaunchKernelGGL(k_tail_bwd, dim3(nb), dim3(256), 0, st, dout, P.w("upsampling.3.weight"), t.hr, t.du, t.ptail, B, A, h, w, S, L);
    LFSR_RC(launched());
    hipLaunchKernelGGL(k_colsum, dim3(9 * 64 / 32), dim3(256), 0, st, t.ptail, (int)nb, 9 * 64, 9 * 64, G("upsampling.3.weight"));
    LFSR_RC(launched());
  }
  hipLaunchKernelGGL(k_pack_up0_T, dim3((64 * 64 * s2 + 255) / 256), dim3(256), 0, st, P.w("upsampling.0.weight"), t.up0T, s2);
  LFSR_RC(launched());
  float* dX = t.dx[0];   // the gradient at the altblock output (+ its skip): dL/d x[nl]
  if (s2 == 4) LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 256, 2>, t.du, 256, t.up0T, dX, 64, nullptr, 0, nullptr, 0, 64));
  else if (s2 == 9) LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 576, 2>, t.du, 576, t.up0T, dX, 64, nullptr, 0, nullptr, 0, 64));
  else LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 1024, 2>, t.du, 1024, t.up0T, dX, 64, nullptr, 0, nullptr, 0, 64));
  LFSR_RC(wgrad_lin(t.du, 64 * s2, 64 * s2, f.x[nl], 64, 64, G("upsampling.0.weight")));

  // ---- altblock, reversed.  LFT.py:91 buffer = altblock(buffer) + buffer: dX also reaches buf0 directly ----------------------------------
  LFSR_RC(ew(dX, 64, nullptr, 0, nullptr, 0, 1.0f, t.dbuf0, 64, 64, npix));
  for (int b = nl - 1; b >= 0; --b) {
    const std::string sp = "altblock." + std::to_string(b) + ".spa_trans.", an = "altblock." + std::to_string(b) + ".ang_trans.";
    float** lin = t.lin;
    // the layer's 1x1 dgrad packs: [C_in][O] of every linear weight (q | k and v as separate row ranges of in_proj)
    LFSR_RC(packT(P.w(sp + "linear.0.weight"), 0, 128, 64, lin[0]));
    LFSR_RC(packT(P.w(sp + "feed_forward.4.weight"), 0, 256, 128, lin[1]));
    LFSR_RC(packT(P.w(sp + "feed_forward.1.weight"), 0, 128, 256, lin[2]));
    LFSR_RC(packT(P.w(sp + "attention.out_proj.weight"), 0, 128, 128, lin[3]));
    LFSR_RC(packT(P.w(sp + "attention.in_proj_weight"), 0, 128, 256, lin[4]));
    LFSR_RC(packT(P.w(sp + "attention.in_proj_weight"), 256, 128, 128, lin[5]));
    LFSR_RC(packT(P.w(an + "feed_forward.4.weight"), 0, 128, 64, lin[6]));
    LFSR_RC(packT(P.w(an + "feed_forward.1.weight"), 0, 64, 128, lin[7]));
    LFSR_RC(packT(P.w(an + "attention.out_proj.weight"), 0, 64, 64, lin[8]));
    LFSR_RC(packT(P.w(an + "attention.in_proj_weight"), 0, 64, 128, lin[9]));
    LFSR_RC(packT(P.w(an + "attention.in_proj_weight"), 128, 64, 64, lin[10]));
    LFSR_RC(pack3T(sp + "MLP.weight#lo", t.mloT[b]));
    LFSR_RC(pack3T(sp + "MLP.weight#hi", t.mhiT[b]));

    // ---- SpaTrans (LFT.py:188-203): x[b+1] = linear.0(sf), sf = sm + FFN(LN(sm)), sm = out_proj(attn) + st ----------------------
    LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 64, 2>, dX, 64, lin[0], t.dsf, 128, nullptr, 0, nullptr, 0, 128));
    LFSR_RC(wgrad_lin(dX, 64, 64, f.sf[b], 128, 128, G(sp + "linear.0.weight")));
    LFSR_RC(lfsr_layernorm_fwd(f.sm[b], 128, 0, nullptr, 0, 0, 1, P.w(sp + "feed_forward.0.weight"), P.w(sp + "feed_forward.0.bias"), t.lnt, 128, 0, npix, 128, 1e-5f, stream));
    LFSR_RC(lfsr_linear_fwd(t.lnt, 128, 0, 128, P.w(sp + "feed_forward.1.weight"), nullptr, nullptr, 0, 0, t.hid_s[b], 256, 0, npix, 256, 0.0f, stream));   // ReLU(hidden)
    LFSR_RC(wgrad_lin(t.dsf, 128, 128, t.hid_s[b], 256, 256, G(sp + "feed_forward.4.weight")));
    LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 128, 2>, t.dsf, 128, lin[1], t.dh, 256, nullptr, 0, t.hid_s[b], 256, 256));
    LFSR_RC(wgrad_lin(t.dh, 256, 256, t.lnt, 128, 128, G(sp + "feed_forward.1.weight")));
    LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 256, 2>, t.dh, 256, lin[2], t.dln, 128, nullptr, 0, nullptr, 0, 128));
    LFSR_RC(ln_bwd(128, f.sm[b], nullptr, 1, 1, sp + "feed_forward.0.weight", sp + "feed_forward.0.bias", t.dln, t.dsf, t.dsm));
    LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 128, 2>, t.dsm, 128, lin[3], t.dso, 128, nullptr, 0, nullptr, 0, 128));
    LFSR_RC(wgrad_lin(t.dsm, 128, 128, f.so[b], 128, 128, G(sp + "attention.out_proj.weight")));
    // window [i-2, i+3) x [j-2, min(h, j+3)): the column clamp uses h (LFT.py:168), as the forward
    LFSR_RC(attn_bwd(16, f.sqk[b], 256, 128, f.sv[b], 128, f.so[b], t.dso, 128, t.dqk, t.dv, nimg, 1, 1, HW, 0, 0, h, w, w, 1, 2, 3, 2, 3, h));
    // q | k = LN(st + spe) W[0:256]^T, v = st W[256:384]^T
    LFSR_RC(lfsr_layernorm_fwd(f.st[b], 128, 0, f.spe[b], 128, HW, 1, P.w(sp + "norm.weight"), P.w(sp + "norm.bias"), t.lnt, 128, 0, npix, 128, 1e-5f, stream));
    float* dWin = G(sp + "attention.in_proj_weight");
    LFSR_RC(wgrad_lin(t.dqk, 256, 256, t.lnt, 128, 128, dWin));
    LFSR_RC(wgrad_lin(t.dv, 128, 128, f.st[b], 128, 128, dWin + 256 * 128));
    LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 256, 2>, t.dqk, 256, lin[4], t.dln, 128, nullptr, 0, nullptr, 0, 128));
    LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 128, 2>, t.dv, 128, lin[5], t.dst, 128, t.dsm, 128, nullptr, 0, 128));
    LFSR_RC(ln_bwd(128, f.st[b], f.spe[b], HW, 1, sp + "norm.weight", sp + "norm.bias", t.dln, nullptr, t.dln2));
    LFSR_RC(ew(t.dst, 128, t.dln2, 128, nullptr, 0, 1.0f, t.dst, 128, 128, npix));
    // st = MLP(unfold(ay)), spe = MLP(unfold(spa_position)): MLP.weight also gets the LayerNorm-input gradient summed over the images
    hipLaunchKernelGGL(k_pe_reduce, dim3(lfsr_blocks((long long)HW * 128, 256)), dim3(256), 0, st, t.dln2, t.dspe, nimg, HW);
    LFSR_RC(launched());
    float* dWm = G(sp + "MLP.weight");
    for (int half = 0; half < 2; ++half) {
      LFSR_RC(wgrad(LFSR_IN_CONV3, t.dst, 128, 64 * half, f.ay[b], 64, npix, 64, 64, 9, dWm + half * 64 * 576, 0));
      LFSR_RC(lfsr_wgrad_launch(LFSR_IN_SAME, LFSR_IN_CONV3, t.dspe, 128, 64 * half, f.spos, 64, 0, t.part, HW, 64, 64, 1, h, w, 9, st));
      LFSR_RC(lfsr_wgrad_reduce(t.part, lfsr_wgrad_splits(HW, 9, 64), nullptr, 0, dWm + half * 64 * 576, 64, 64, 9, 0, 0, 1, 0, 0, st));
    }
    LFSR_RC(dgrad3(t.dst, 128, 0, t.mloT[b], t.d64, nullptr, nullptr));
    LFSR_RC(dgrad3(t.dst, 128, 64, t.mhiT[b], t.t64, t.d64, nullptr));   // t64 = dL/d ay

    // ---- AngTrans (LFT.py:233-246): ay = am + FFN(LN(am)), am = out_proj(attn) + x[b] ---------------------------------------------
    LFSR_RC(lfsr_layernorm_fwd(f.am[b], 64, 0, nullptr, 0, 0, 1, P.w(an + "feed_forward.0.weight"), P.w(an + "feed_forward.0.bias"), t.lnt, 64, 0, npix, 64, 1e-5f, stream));
    LFSR_RC(lfsr_linear_fwd(t.lnt, 64, 0, 64, P.w(an + "feed_forward.1.weight"), nullptr, nullptr, 0, 0, t.hid_a[b], 128, 0, npix, 128, 0.0f, stream));
    LFSR_RC(wgrad_lin(t.t64, 64, 64, t.hid_a[b], 128, 128, G(an + "feed_forward.4.weight")));
    LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 64, 2>, t.t64, 64, lin[6], t.dh, 128, nullptr, 0, t.hid_a[b], 128, 128));
    LFSR_RC(wgrad_lin(t.dh, 128, 128, t.lnt, 64, 64, G(an + "feed_forward.1.weight")));
    LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 128, 2>, t.dh, 128, lin[7], t.dln, 64, nullptr, 0, nullptr, 0, 64));
    LFSR_RC(ln_bwd(64, f.am[b], nullptr, 1, 1, an + "feed_forward.0.weight", an + "feed_forward.0.bias", t.dln, t.t64, t.dsm));   // dsm: dL/d am (64)
    LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 64, 2>, t.dsm, 64, lin[8], t.dso, 64, nullptr, 0, nullptr, 0, 64));
    LFSR_RC(wgrad_lin(t.dsm, 64, 64, f.ao[b], 64, 64, G(an + "attention.out_proj.weight")));
    LFSR_RC(attn_bwd(8, f.aqk[b], 128, 64, f.av[b], 64, f.ao[b], t.dso, 64, t.dqk, t.dv, B, h, w, (long long)AA * HW, w, 1, AA, 1, HW, 0, AA, AA, 0, 1, 0));
    LFSR_RC(lfsr_layernorm_fwd(f.x[b], 64, 0, f.ape, 64, AA, HW, P.w(an + "norm.weight"), P.w(an + "norm.bias"), t.lnt, 64, 0, npix, 64, 1e-5f, stream));
    dWin = G(an + "attention.in_proj_weight");
    LFSR_RC(wgrad_lin(t.dqk, 128, 128, t.lnt, 64, 64, dWin));
    LFSR_RC(wgrad_lin(t.dv, 64, 64, f.x[b], 64, 64, dWin + 128 * 64));
    LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 128, 2>, t.dqk, 128, lin[9], t.dln, 64, nullptr, 0, nullptr, 0, 64));
    float* dXp = t.dx[(nl - b) & 1];
    LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 64, 2>, t.dv, 64, lin[10], dXp, 64, t.dsm, 64, nullptr, 0, 64));
    LFSR_RC(ln_bwd(64, f.x[b], f.ape, AA, HW, an + "norm.weight", an + "norm.bias", t.dln, dXp, dXp));
    dX = dXp;
  }

  // ---- init: buf0 = lrelu(conv_init.4(c2)) + f0, c2 = lrelu(conv_init.2(c1)), c1 = lrelu(conv_init.0(f0)), f0 = conv_init0(x) ------------
  LFSR_RC(ew(t.dbuf0, 64, dX, 64, nullptr, 0, 1.0f, t.dbuf0, 64, 64, npix));
  LFSR_RC(pack3T("conv_init.0.weight", t.initT[0]));
  LFSR_RC(pack3T("conv_init.2.weight", t.initT[1]));
  LFSR_RC(pack3T("conv_init.4.weight", t.initT[2]));
  // conv_init.4's LeakyReLU output without the residual, for its mask (the forward's launch minus r1)
  LFSR_RC(lfsr_conv3x3_fwd(f.c2, 64, 0, P.w("conv_init.4.weight"), t.r4, 64, 0, nullptr, 0, 0, nullptr, 0, 0, nimg, h, w, L, stream));
  LFSR_RC(ew(t.dbuf0, 64, nullptr, 0, t.r4, 64, L, t.d64, 64, 64, npix));
  LFSR_RC(wgrad(LFSR_IN_CONV3, t.d64, 64, 0, f.c2, 64, npix, 64, 64, 9, G("conv_init.4.weight"), 0));
  LFSR_RC(dgrad3(t.d64, 64, 0, t.initT[2], t.t64, nullptr, f.c2));
  LFSR_RC(wgrad(LFSR_IN_CONV3, t.t64, 64, 0, f.c1, 64, npix, 64, 64, 9, G("conv_init.2.weight"), 0));
  LFSR_RC(dgrad3(t.t64, 64, 0, t.initT[1], t.d64, nullptr, f.c1));
  LFSR_RC(wgrad(LFSR_IN_CONV3, t.d64, 64, 0, f.f0, 64, npix, 64, 64, 9, G("conv_init.0.weight"), 0));
  LFSR_RC(dgrad3(t.d64, 64, 0, t.initT[0], t.t64, t.dbuf0, nullptr));
  LFSR_RC(lfsr_init_gather9(x, t.xg9, B, A, h, w, st));
  LFSR_RC(wgrad(LFSR_IN_SAME, t.t64, 64, 0, t.xg9, 16, npix, 64, 16, 1, G("conv_init0.0.weight"), 0, 9));
  return LFSR_OK;
}

}  // extern "C"
