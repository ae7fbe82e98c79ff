// Backward of DistgSSR's angular and epipolar branches as operators (disentg_branches_bwd; reference layers DistgSSR.py:84-97,108; what
// autograd derives for them in train.py:256-264, fp32).  lfsr_distgssr_backward calls the two internal functions; the C-ABI entry points
// lfsr_angconv_bwd / lfsr_epiconv_hv_bwd wrap them for callers that hold raw PyTorch-layout weights (they pack what the kernels read into the
// caller's workspace first).
#include <stdlib.h>

#include <algorithm>

#include "lfsr_internal.h"

namespace {
inline int pad32(int v) { return (v + 31) / 32 * 32; }

// out[row][c] = dy[row][c] * LeakyReLU'(y[row][c]) for C channels (a multiple of 4) of strided VCL operands: the gradient at a branch's stage-2 pre-activation
__global__ __launch_bounds__(256) void k_mask_lrelu(const float* __restrict__ dy, int dy_stride, int dy_choff, const float* __restrict__ y, int y_stride, int y_choff,
                                                   float* __restrict__ out, int out_stride, int out_choff, long long rows, int C, float slope) {
  const int c4 = C >> 2;
  const long long total = rows * c4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long r = i / c4;
    const int c = (int)(i - r * c4) * 4;
    const float4 g = *reinterpret_cast<const float4*>(dy + r * dy_stride + dy_choff + c);
    const float4 a = *reinterpret_cast<const float4*>(y + r * y_stride + y_choff + c);
    *reinterpret_cast<float4*>(out + r * out_stride + out_choff + c) =
        make_float4(a.x > 0.f ? g.x : g.x * slope, a.y > 0.f ? g.y : g.y * slope, a.z > 0.f ? g.z : g.z * slope, a.w > 0.f ? g.w : g.w * slope);
  }
}

int mask_lrelu(const float* dy, int dy_stride, int dy_choff, const float* y, int y_stride, int y_choff, float* out, int out_stride, int out_choff, long long rows, int C,
               float slope, hipStream_t st) {
  if ((dy_stride | dy_choff | y_stride | y_choff | out_stride | out_choff | C) & 3 || (((uintptr_t)dy | (uintptr_t)y | (uintptr_t)out) & 15)) return LFSR_E_ARG;
  unsigned grid = lfsr_blocks(rows * (C >> 2), 256);
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(k_mask_lrelu, dim3(grid), dim3(256), 0, st, dy, dy_stride, dy_choff, y, y_stride, y_choff, out, out_stride, out_choff, rows, C, slope);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

// the four weight gradients of the branches, pointers apart: what the backward submits and what lfsr_branch_bwd_partial_floats sizes
LfsrWgrad ang2_wgrad(int B, int A, int h, int w) {      // AngConv.2 (16 A A, 16): G gathered from the A A views, the taps are the pixel shuffle's chunks
  LfsrWgrad g = lfsr_wgrad_gather(LFSR_IN_ANG, LFSR_IN_SAME, B * h * w, 16, 16, A * A, A, h, w);
  g.O = 16 * A * A; g.C = 16; g.T = A * A; g.perm = 1; g.ch = 16; g.chunk_mode = 1;
  return g;
}
LfsrWgrad ang0_wgrad(int B, int A, int h, int w) { return lfsr_wgrad_gather(LFSR_IN_SAME, LFSR_IN_ANG, B * h * w, 16, 64, A * A, A, h, w); }      // AngConv.0 (16, 64, A, A)
LfsrWgrad epi2_wgrad(int B, int A, int h, int w) {      // EPIConv.2 (32 A, 32), one pass (gmode: LFSR_IN_CHK_H / _V)
  LfsrWgrad g = lfsr_wgrad_gather(LFSR_IN_CHK_H, LFSR_IN_SAME, B * A * h * w, 32, 32, A, A, h, w);
  g.O = 32 * A; g.C = 32; g.T = A; g.ch = 32; g.chunk_mode = 1;
  return g;
}
LfsrWgrad epi0_wgrad(int B, int A, int h, int w) {      // EPIConv.0 (32, 64, 1, A A)
  LfsrWgrad g{};
  g.form = LFSR_WG_EPI0; g.g_stride = 32; g.x_stride = 64; g.B = B; g.A = A; g.h = h; g.w = w;
  return g;
}
}  // namespace

// AngConv: y = PixelShuffle_A(lrelu(W2 . a16)), a16 = lrelu(W0 (*) x) (A x A, stride A).  dcat: dLoss/dy inside a VCL buffer (16 channels at dc_choff).
// dx += ; dw0 (16,64,A,A), dw2 (16 A^2,16,1,1) overwritten.  dA16: (B h w, 16) scratch; P: partial-slab scratch of >= lfsr_branch_bwd_partial_floats.
// Two parts so that a caller may run part 1 (everything up to dA16 and both weight gradients) on another stream than part 2 (the read-modify-write of dx).
int lfsr_ang_branch_bwd_p1(const float* dcat, int dc_stride, int dc_choff, const float* xin, const float* a16, const float* w2T_packed, float* dw0, float* dw2,
                           float* dA16, float* P, int B, int A, int h, int w, float slope, hipStream_t st) {
  const int AA = A * A, nlr = B * h * w;
  LfsrWgrad g2 = ang2_wgrad(B, A, h, w), g0 = ang0_wgrad(B, A, h, w);
  g2.G = dcat; g2.g_stride = dc_stride; g2.g_choff = dc_choff; g2.X = a16; g2.dW = dw2; g2.part = P; g2.part_floats = lfsr_branch_bwd_partial_floats(B, A, h, w);
  g0.G = dA16; g0.X = xin; g0.dW = dw0; g0.part = P; g0.part_floats = g2.part_floats;
  LFSR_RC(lfsr_wgrad_run(g2, st));
  {
    LfsrGemm q{};
    q.in_mode = LFSR_IN_ANG; q.out_mode = LFSR_OUT_SAME; q.cin = 16; q.X = dcat; q.x_stride = dc_stride; q.x_choff = dc_choff; q.Wp = w2T_packed;
    q.Y = dA16; q.y_stride = 16; q.Mk = a16; q.mk_stride = 16; q.mk_slope = slope;
    q.M = nlr; q.N = 16; q.A = A; q.h = h; q.w = w; q.ntaps = AA; q.CH = 16;
    LFSR_RC(lfsr_bwd_gemm(q, st));
  }
  return lfsr_wgrad_run(g0, st);
}

int lfsr_ang_branch_bwd_p2(const float* dA16, const float* w0_packed, const float* w0T_packed, float* dx, int B, int A, int h, int w, hipStream_t st) {
  const int AA = A * A, nlr = B * h * w;
  LfsrGemm q{};
  q.in_mode = LFSR_IN_SAME; q.out_mode = LFSR_OUT_VIEWS; q.cin = 16; q.X = dA16; q.x_stride = 16; q.Wp = w0T_packed;
  q.Y = dx; q.y_stride = 64; q.R1 = dx; q.r1_stride = 64;
  q.M = nlr; q.N = AA * 64; q.A = A; q.h = h; q.w = w; q.ntaps = 1; q.CH = 64;
  int rc4 = lfsr_ang0_dgrad_launch(dA16, w0_packed, dx, 64, 0, B, A, h, w, st);   // streaming read-modify-write form; else the gather-GEMM
  if (rc4 == LFSR_E_ARG) rc4 = lfsr_bwd_gemm(q, st);
  return rc4;
}

int lfsr_ang_branch_bwd(const float* dcat, int dc_stride, int dc_choff, const float* xin, const float* a16, const float* w0_packed, const float* w0T_packed,
                        const float* w2T_packed, float* dx, float* dw0, float* dw2, float* dA16, float* P, int B, int A, int h, int w, float slope, hipStream_t st) {
  const int rc = lfsr_ang_branch_bwd_p1(dcat, dc_stride, dc_choff, xin, a16, w2T_packed, dw0, dw2, dA16, P, B, A, h, w, slope, st);
  return rc ? rc : lfsr_ang_branch_bwd_p2(dA16, w0_packed, w0T_packed, dx, B, A, h, w, st);
}

// EPIConv on the tensor (horizontal) and on its transpose (vertical), shared weights: y_h / y_v = PixelShuffle1D_A(lrelu(W2 . e)), e = lrelu(W0 (*) x)
// (1 x A^2, stride A along the EPI line).  dcat: dLoss/dy_h at choff_h, dLoss/dy_v at choff_v (32 channels each) of one VCL buffer.
// dx += ; dw0 (32,64,1,A^2), dw2 (32 A,32,1,1) overwritten (both passes summed).  dEh, dEv: (B A h w, 32) scratch; P[4]: partial-slab scratch.
// Three parts: p1 = stage 2 of both passes (dEh, dEv, dw2), p2d = the read-modify-write of dx, p2w = EPIConv.0's weight gradient (reads dEh, dEv and x only).
int lfsr_epi_branch_bwd_p1(const float* dcat, int dc_stride, int choff_h, int choff_v, const float* eh, const float* ev, const float* w2T_packed, float* dw2,
                           float* dEh, float* dEv, float* const P[4], int B, int A, int h, int w, float slope, hipStream_t st) {
  const int nepi = B * A * h * w;
  LfsrWgrad g = epi2_wgrad(B, A, h, w);      // the passes share EPIConv.2's weights: two slab sets, one reduce
  g.G = dcat; g.g_stride = dc_stride; g.dW = dw2; g.part_floats = lfsr_branch_bwd_partial_floats(B, A, h, w);
  int slabs[2] = {0, 0};
  for (int vert = 0; vert < 2; ++vert) {
    const float* E = vert ? ev : eh;
    float* dE = vert ? dEv : dEh;
    const int choff = vert ? choff_v : choff_h;
    g.gmode = vert ? LFSR_IN_CHK_V : LFSR_IN_CHK_H; g.g_choff = choff; g.X = E; g.part = P[vert ? 2 : 0];
    LFSR_RC(lfsr_wgrad_partials(g, &slabs[vert], st));
    LfsrGemm q{};
    q.in_mode = vert ? LFSR_IN_CHK_V : LFSR_IN_CHK_H; q.out_mode = LFSR_OUT_SAME; q.cin = 32; q.X = dcat; q.x_stride = dc_stride; q.x_choff = choff;
    q.Wp = w2T_packed; q.Y = dE; q.y_stride = 32; q.Mk = E; q.mk_stride = 32; q.mk_slope = slope;
    q.M = nepi; q.N = 32; q.A = A; q.h = h; q.w = w; q.ntaps = A; q.CH = 32;
    LFSR_RC(lfsr_bwd_gemm(q, st));
  }
  g.part = P[0];
  return lfsr_wgrad_sum(g, slabs[0], P[2], slabs[1], st);
}

int lfsr_epi_branch_bwd_p2d(const float* dEh, const float* dEv, const float* w0_packed, const float* w0T_packed, float* dx, int B, int A, int h, int w, hipStream_t st) {
  const int nepi = B * A * h * w;
  for (int vert = 0; vert < 2; ++vert) {
    const float* dE = vert ? dEv : dEh;
    LfsrGemm r{};
    r.in_mode = vert ? LFSR_IN_LINE_V : LFSR_IN_LINE_H; r.out_mode = vert ? LFSR_OUT_EPIV : LFSR_OUT_EPIH; r.cin = 32; r.X = dE; r.x_stride = 32;
    r.Wp = w0T_packed; r.Y = dx; r.y_stride = 64; r.R1 = dx; r.r1_stride = 64;
    r.M = nepi; r.N = A * 64; r.A = A; r.h = h; r.w = w; r.ntaps = A; r.CH = 64;
    // EPIConv.0 data gradient (accumulates into dx): EPI-line kernel where it applies, else the gather-GEMM
    int rc3 = lfsr_epi0_dgrad_launch(dE, w0_packed, dx, 64, 0, B, A, h, w, vert, st);
    if (rc3 == LFSR_E_ARG) rc3 = lfsr_bwd_gemm(r, st);
    if (rc3) return rc3;
  }
  return LFSR_OK;
}

int lfsr_epi_branch_bwd_p2w(const float* dEh, const float* dEv, const float* xin, float* dw0, float* const P[4], int B, int A, int h, int w, hipStream_t st) {
  // the two passes share EPIConv.0's weights: where the EPI-line kernel applies, ONE weight-gradient launch covers both (one slab per block instead of
  // two sets); else the gather form per pass
  LfsrWgrad g = epi0_wgrad(B, A, h, w);
  g.G = dEh; g.G2 = dEv; g.X = xin; g.dW = dw0; g.part = P[1]; g.part_floats = lfsr_branch_bwd_partial_floats(B, A, h, w);
  int slabs[2] = {0, 0};
  int rc = lfsr_wgrad_partials(g, &slabs[0], st);
  if (rc == LFSR_E_ARG) {
    g.G2 = nullptr; g.xmode = LFSR_IN_EPIH;
    LFSR_RC(lfsr_wgrad_partials(g, &slabs[0], st));
    g.G = dEv; g.xmode = LFSR_IN_EPIV; g.part = P[3];
    rc = lfsr_wgrad_partials(g, &slabs[1], st);
    g.part = P[1];
  }
  return rc ? rc : lfsr_wgrad_sum(g, slabs[0], slabs[1] ? P[3] : nullptr, slabs[1], st);
}

int lfsr_epi_branch_bwd(const float* dcat, int dc_stride, int choff_h, int choff_v, const float* xin, const float* eh, const float* ev,
                        const float* w0_packed, const float* w0T_packed, const float* w2T_packed, float* dx, float* dw0, float* dw2,
                        float* dEh, float* dEv, float* const P[4], int B, int A, int h, int w, float slope, hipStream_t st) {
  int rc = lfsr_epi_branch_bwd_p1(dcat, dc_stride, choff_h, choff_v, eh, ev, w2T_packed, dw2, dEh, dEv, P, B, A, h, w, slope, st);
  if (!rc) rc = lfsr_epi_branch_bwd_p2d(dEh, dEv, w0_packed, w0T_packed, dx, B, A, h, w, st);
  if (!rc) rc = lfsr_epi_branch_bwd_p2w(dEh, dEv, xin, dw0, P, B, A, h, w, st);
  return rc;
}

size_t lfsr_branch_bwd_partial_floats(int B, int A, int h, int w) {
  size_t m = 0;
  for (const LfsrWgrad& g : {ang2_wgrad(B, A, h, w), ang0_wgrad(B, A, h, w), epi2_wgrad(B, A, h, w), epi0_wgrad(B, A, h, w)}) m = std::max(m, lfsr_wgrad_part_floats(g));
  return m;
}

namespace {
struct AngWs { float *w0p, *w0T, *w2T, *dA16, *P, *dym; };
void ang_layout(int B, int A, int h, int w, LfsrArena& ws, AngWs& t) {
  const int AA = A * A;
  t.w0p = ws.take(lfsr_packed_weight_floats(16, 64, AA));
  t.w0T = ws.take((size_t)AA * pad32(64) * 16);
  t.w2T = ws.take((size_t)AA * pad32(16) * 16);
  t.dA16 = ws.take((size_t)B * h * w * 16);
  t.P = ws.take(lfsr_branch_bwd_partial_floats(B, A, h, w));
  t.dym = ws.take((size_t)B * AA * h * w * 16);
}
struct EpiWs { float *w0p, *w0T, *w2T, *dEh, *dEv, *P[4], *dym; };
void epi_layout(int B, int A, int h, int w, LfsrArena& ws, EpiWs& t) {
  const int AA = A * A;
  t.w0p = ws.take(lfsr_packed_weight_floats(32, 64, AA));
  t.w0T = ws.take((size_t)AA * pad32(64) * 32);
  t.w2T = ws.take((size_t)A * pad32(32) * 32);
  t.dEh = ws.take((size_t)B * A * h * w * 32);
  t.dEv = ws.take((size_t)B * A * h * w * 32);
  for (int i = 0; i < 4; ++i) t.P[i] = ws.take(lfsr_branch_bwd_partial_floats(B, A, h, w));
  t.dym = ws.take((size_t)B * AA * h * w * 64);
}
}  // namespace

extern "C" {

size_t lfsr_angconv_bwd_workspace_floats(int B, int A, int h, int w) {
  if (B <= 0 || A <= 0 || A > 15 || h <= 0 || w <= 0) return 0;
  LfsrArena ws;
  AngWs t;
  ang_layout(B, A, h, w, ws, t);
  return ws.floats;
}

int lfsr_angconv_bwd(const float* dy, int dy_stride, int dy_choff, const float* y, int y_stride, int y_choff, const float* x, const float* a16, const float* w0, const float* w2,
                     float* dx, float* dw0, float* dw2, float* workspace, size_t workspace_floats, int B, int A, int h, int w, float slope, void* stream) {
  if (!dy || !x || !a16 || !w0 || !w2 || !dx || !dw0 || !dw2 || !workspace || B <= 0 || A <= 0 || A > 15 || !(A & 1) || h <= 0 || w <= 0) return LFSR_E_ARG;
  if (dy_stride < dy_choff + 16 || (y && y_stride < y_choff + 16) || ((uintptr_t)workspace & 15)) return LFSR_E_ARG;
  if ((long long)B * A * A * h * w >= (1LL << 31) / 144) return LFSR_E_ARG;
  LfsrArena ws(workspace);
  AngWs t;
  ang_layout(B, A, h, w, ws, t);
  if (workspace_floats < ws.floats) return LFSR_E_WS;
  hipStream_t st = lfsr_stream(stream);
  const int AA = A * A;
  int rc = lfsr_pack_conv_weight_m(w0, t.w0p, 16, 64, AA, 0, 0, 0, stream);
  if (!rc) rc = lfsr_pack_weight_T(w0, t.w0T, 16, 64, AA, 0, st);
  if (!rc) rc = lfsr_pack_weight_chunkT(w2, t.w2T, 16 * AA, 16, 16, 1, st);
  if (rc) return rc;
  if (y) {   // dLoss/dy -> the gradient at the stage-2 pre-activation (inside the model the fuse.0 data gradient's LeakyReLU' epilogue has done this already)
    rc = mask_lrelu(dy, dy_stride, dy_choff, y, y_stride, y_choff, t.dym, 16, 0, (long long)B * AA * h * w, 16, slope, st);
    if (rc) return rc;
    dy = t.dym; dy_stride = 16; dy_choff = 0;
  }
  return lfsr_ang_branch_bwd(dy, dy_stride, dy_choff, x, a16, t.w0p, t.w0T, t.w2T, dx, dw0, dw2, t.dA16, t.P, B, A, h, w, slope, st);
}

size_t lfsr_epiconv_hv_bwd_workspace_floats(int B, int A, int h, int w) {
  if (B <= 0 || A <= 0 || A > 15 || h <= 0 || w <= 0) return 0;
  LfsrArena ws;
  EpiWs t;
  epi_layout(B, A, h, w, ws, t);
  return ws.floats;
}

int lfsr_epiconv_hv_bwd(const float* dy, int dy_stride, int choff_h, int choff_v, const float* y, int y_stride, int y_choff_h, int y_choff_v,
                        const float* x, const float* e_h, const float* e_v, const float* w0, const float* w2,
                        float* dx, float* dw0, float* dw2, float* workspace, size_t workspace_floats, int B, int A, int h, int w, float slope, void* stream) {
  if (!dy || !x || !e_h || !e_v || !w0 || !w2 || !dx || !dw0 || !dw2 || !workspace || B <= 0 || A <= 0 || A > 15 || !(A & 1) || h <= 0 || w <= 0) return LFSR_E_ARG;
  if (dy_stride < choff_h + 32 || dy_stride < choff_v + 32 || (y && (y_stride < y_choff_h + 32 || y_stride < y_choff_v + 32)) || ((uintptr_t)workspace & 15)) return LFSR_E_ARG;
  if ((long long)B * A * A * h * w >= (1LL << 31) / 144) return LFSR_E_ARG;
  LfsrArena ws(workspace);
  EpiWs t;
  epi_layout(B, A, h, w, ws, t);
  if (workspace_floats < ws.floats) return LFSR_E_WS;
  hipStream_t st = lfsr_stream(stream);
  const int AA = A * A;
  int rc = lfsr_pack_conv_weight_m(w0, t.w0p, 32, 64, AA, 0, 0, 0, stream);
  if (!rc) rc = lfsr_pack_weight_T(w0, t.w0T, 32, 64, AA, 0, st);
  if (!rc) rc = lfsr_pack_weight_chunkT(w2, t.w2T, 32 * A, 32, 32, 0, st);
  if (rc) return rc;
  if (y) {
    const long long npix = (long long)B * AA * h * w;
    rc = mask_lrelu(dy, dy_stride, choff_h, y, y_stride, y_choff_h, t.dym, 64, 0, npix, 32, slope, st);
    if (!rc) rc = mask_lrelu(dy, dy_stride, choff_v, y, y_stride, y_choff_v, t.dym, 64, 32, npix, 32, slope, st);
    if (rc) return rc;
    dy = t.dym; dy_stride = 64; choff_h = 0; choff_v = 32;
  }
  return lfsr_epi_branch_bwd(dy, dy_stride, choff_h, choff_v, x, e_h, e_v, t.w0p, t.w0T, t.w2T, dx, dw0, dw2, t.dEh, t.dEv, t.P, B, A, h, w, slope, st);
}

}  // extern "C"
