// LF_InterNet training: the forward that keeps what the backward reads, and the backward (autograd of model/SR/LF_InterNet.py:33-141
// as driven by train.py:256-264, fp32).  Layouts are the forward's (internet.hip): spatial rows are VCL pixels, angular rows are LR
// pixels (b,y,x); every chain layer keeps its own 128-wide rows [xs | spa2] and [xa | ang2] instead of the forward's ping-pong.
//
// ReLU' masks: out_a, out_s and BottleNeck's output are ReLU(z) + residual, and the sum can absorb a tiny positive z, so the mask is
// never rebuilt from the sum.  The training forward writes ReLU(z) to a saved buffer and adds the residual in a separate launch: the
// same two fp32 operations as the forward's epilogue (v = relu(acc); v += r), so the output is bit-identical to the inference forward.
// AngConvSq runs twice instead (once exactly as the forward does, once without the residual into the saved buffer): it is small.
//
// Backward: every data gradient is a gather-GEMM over transposed packs (gemm_gather_kernel.h) or the 64 -> 64 3x3 data-gradient kernel
// (on the 64-channel input slices of SpaConvSq / SpaBottle); every weight gradient is the two-pass partial-slab reduction of wgrad.hip
// (no float atomics: bitwise reproducible).  ReconBlock's folded conv is differentiated through the fold (k_fold_bwd).
//
// lfsr_set_wide_train_arithmetic (read at every launch) reaches the wide per-view 3x3 convs, the sixteen SpaConvSq (128 -> 64) and SpaBottle (320 -> 64), and nothing
// else: in modes 1 and 2 their weight gradients run wgrad_wide_bf16.hip through the WIDE3 form of lfsr_wgrad_run, which lfsr_conv3x3_wide_wgrad shares; in mode 2 the
// training forward computes ReLU(SpaConvSq) and ReLU(SpaBottle) with conv3x3_wide_bf16.hip (unless LFSR_ARITH_F32 is set) and keeps the separate residual add,
// because the backward reads the ReLU results as masks.  lfsr_set_wide_arithmetic is not read here.
#include <algorithm>
#include <string>
#include <vector>

#include "gemm_gather_kernel.h"
#include "internet_ctx.h"

namespace {

// d[r][c] = (a[r][c] (+ b[r][c])) * [mk[r][c] > 0]   for 64 channels; b, mk optional.  The forward's residual add (a = ReLU(z), b = residual)
// and the backward's ReLU' masks and gradient sums.
__global__ __launch_bounds__(256) void k_ew64(const float* a, int as, int ao, const float* __restrict__ b, int bs, int bo,
                                              const float* __restrict__ mk, int ms, int mo, float* d, int ds, int dof, long long M) {   // (a and d may alias: in-place sums)
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < M * 16; g += (long long)gridDim.x * 256) {
    const long long r = g >> 4;
    const int c4 = (int)(g & 15) * 4;
    float4 v = *reinterpret_cast<const float4*>(a + r * as + ao + c4);
    if (b) {
      const float4 u = *reinterpret_cast<const float4*>(b + r * bs + bo + c4);
      v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    if (mk) {
      const float4 m = *reinterpret_cast<const float4*>(mk + r * ms + mo + c4);
      v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f; v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
    }
    *reinterpret_cast<float4*>(d + r * ds + dof + c4) = v;
  }
}

// dOut (B,1,A*h*s,A*w*s) HR mosaic -> g[p][ij] (p = VCL pixel, ij = i*s+j < s^2, zero up to 16): the transpose of the OUT_PS_HR scatter
__global__ __launch_bounds__(256) void k_unshuffle_hr(const float* __restrict__ dout, float* __restrict__ g, int B, int A, int h, int w, int s) {
  const long long npix = (long long)B * A * A * h * w;
  const long long Wo = (long long)A * w * s;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < npix * 16; e += (long long)gridDim.x * 256) {
    const long long pix = e >> 4;
    const int ij = (int)(e & 15);
    float v = 0.f;
    if (ij < s * s) {
      const int x = (int)(pix % w);
      long long t = pix / w;
      const int y = (int)(t % h);
      t /= h;
      const int view = (int)(t % (A * A));
      const long long b = t / (A * A);
      const int u = view / A, vv = view - u * A, i = ij / s, j = ij - i * s;
      v = dout[(b * A * h * s + (long long)(u * h + y) * s + i) * Wo + (long long)(vv * w + x) * s + j];
    }
    g[e] = v;
  }
}

// x (B,1,A*h,A*w) -> xg[r][view] (r = LR pixel, zero up to kpad): AngFE's input as rows, for its weight gradient
__global__ __launch_bounds__(256) void k_angfe_gather(const float* __restrict__ x, float* __restrict__ xg, int B, int A, int h, int w, int kpad) {
  const long long nlr = (long long)B * h * w;
  const int AA = A * A;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nlr * kpad; e += (long long)gridDim.x * 256) {
    const long long r = e / kpad;
    const int k = (int)(e - r * kpad);
    float v = 0.f;
    if (k < AA) {
      const int xx = (int)(r % w);
      const long long t = r / w;
      const int yy = (int)(t % h);
      const long long b = t / h;
      const int u = k / A, vv = k - u * A;
      v = x[b * (long long)A * h * A * w + (long long)(u * h + yy) * A * w + vv * w + xx];
    }
    xg[e] = v;
  }
}

// dgrad pack of the folded ReconBlock conv: out[t'][k (64)][ij (16)] = wf[8 - t'][ij][k] (ij < s^2, else 0); wf = the forward's [9][32][64] fold
__global__ void k_pack_fold_T(const float* __restrict__ wf, float* __restrict__ out, int s2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;   // over 9*64*16
  if (i >= 9 * 64 * 16) return;
  const int ij = i & 15, k = (i >> 4) & 63, tp = i >> 10;
  out[i] = ij < s2 ? wf[((8 - tp) * 32 + ij) * 64 + k] : 0.f;
}

// dgrad pack from the forward's pack Wp[T][Npad_in][C] (Wp[t][n][k] = W[n][k][t]): out[t'][k'][n] = Wp[flip ? T-1-t' : t'][n][k0 + k'] for n < O,
// k' < Kc -- the transposed (3x3: flipped) pack of the input-channel slice [k0, k0 + Kc).  The forward's perm-1 pack of a 1x1 conv + PixelShuffle
// (row n = view*64 + c) read with T = A^2 blocks of Npad_in = 64 rows is the chunked transposed pack [view][k][c] of the Ang2Spa data gradient.
__global__ __launch_bounds__(256) void k_pack_T_from_fwd(const float* __restrict__ Wp, float* __restrict__ out, int T, int Npad_in, int C, int O, int k0, int Kc, int flip) {
  const long long total = (long long)T * Kc * O;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int n = (int)(i % O);
    const long long r = i / O;
    const int k = (int)(r % Kc), tp = (int)(r / Kc);
    const int t = flip ? T - 1 - tp : tp;
    out[i] = Wp[((long long)t * Npad_in + n) * C + k0 + k];
  }
}

// Backward of the ReconBlock fold wf[tap][ij][k] = sum_c wfin[c] wpre[c s2 + ij][k][tap] (linear in each factor), dWf raw (16, 64, 9):
//   dPreConv[c s2 + ij][k][tap] = wfin[c] dWf[ij][k][tap],   dFinalConv[c] = sum_{ij,k,tap} wpre[c s2 + ij][k][tap] dWf[ij][k][tap]
// One block per c: its dPreConv rows, then dFinalConv[c] as a fixed-order fp64 tree sum (deterministic).
__global__ __launch_bounds__(256) void k_fold_bwd(const float* __restrict__ dWf, const float* __restrict__ wpre, const float* __restrict__ wfin,
                                                  float* __restrict__ dpre, float* __restrict__ dfin, int s2) {
  __shared__ double red[256];
  const int c = blockIdx.x, n = s2 * 64 * 9;
  const float wc = wfin[c];
  const float* wp = wpre + (long long)c * n;
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float g = dWf[i];      // (ij, k, tap) of dWf == (ij, k, tap) of PreConv row c s2 + ij
    dpre[(long long)c * n + i] = wc * g;
    a += (double)wp[i] * (double)g;
  }
  red[threadIdx.x] = a;
  __syncthreads();
  for (int sft = 128; sft > 0; sft >>= 1) {
    if ((int)threadIdx.x < sft) red[threadIdx.x] += red[threadIdx.x + sft];
    __syncthreads();
  }
  if (threadIdx.x == 0) dfin[c] = (float)red[0];
}

int ew64(const float* a, int as, int ao, const float* b, int bs, int bo, const float* mk, int ms, int mo, float* d, int ds, int dof, long long M, hipStream_t st) {
  hipLaunchKernelGGL(k_ew64, dim3(lfsr_cap_grid(M * 16)), dim3(256), 0, st, a, as, ao, b, bs, bo, mk, ms, mo, d, ds, dof, M);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

// ---- workspace --------------------------------------------------------------------------------------------------------------
constexpr int NG = 4, NL = 4, NLAYER = NG * NL;
inline int angfe_kpad(int A) { return (A * A + 3) / 4 * 4; }

struct InterTrainWs {
  // saved by forward_train
  float *S[NLAYER + 1], *Ar[NLAYER + 1];   // layer l's input rows [xs | spa2] (VCL, 128) and [xa | ang2] (LR, 128); index 16: the cascade's output
  float *RS[NLAYER], *RA[NLAYER];         // ReLU(SpaConvSq), ReLU(AngConvSq) of layer l (64)
  float *CS, *CA, *BA, *RB, *BO;           // concat of the spatial group outputs + BottleNeck's Ang2Spa (VCL, 320), of the angular ones (LR, 256),
                                           // ReLU(AngBottle) (LR, 64), ReLU(SpaBottle) (VCL, 64), BottleNeck output (VCL, 64)
  // transposed packs (built by forward_train)
  float *ScLo[NLAYER], *ScHi[NLAYER], *AcT[NLAYER], *A2sT[NLAYER], *S2aT[NLAYER];
  float *SbT[NG + 1], *AbT, *BA2sT, *FoldT;
  // backward scratch
  float *G16, *dBO, *dZ, *dCS, *dOs[2], *dSP, *dOa[2], *dzA, *dG2, *dCA, *dZa, *XG9, *XA, *P, *dWf;
};

// the backward's weight gradients, pointers apart: what lfsr_internet_backward submits and what partial_floats sizes
LfsrWgrad wide_wgrad(int cin, int B, int A, int h, int w) {      // SpaConvSq (128) / SpaBottle (320): follows lfsr_set_wide_train_arithmetic
  LfsrWgrad g{};
  g.form = LFSR_WG_WIDE3; g.g_stride = 64; g.K = cin; g.B = B; g.A = A; g.h = h; g.w = w;
  return g;
}

size_t partial_floats(int A, int B, int h, int w) {
  const int AA = A * A, npix = B * AA * h * w, nlr = B * h * w;
  const int S = LFSR_IN_SAME;
  size_t m = 0;
  for (const LfsrWgrad& g : {lfsr_wgrad_gather(S, LFSR_IN_CONV3, npix, 16, 64, 9, A, h, w),      // ReconBlock fold
                             wide_wgrad(64 * (NG + 1), B, A, h, w), wide_wgrad(128, B, A, h, w),   // SpaBottle, SpaConvSq
                             lfsr_wgrad_gather(S, LFSR_IN_ANG, nlr, 64, 64, AA, A, h, w),         // Ang2Spa / Spa2Ang
                             lfsr_wgrad_gather(S, S, nlr, 64, 64 * NG, 1, A, h, w),               // AngBottle
                             lfsr_wgrad_gather(S, S, nlr, 64, 128, 1, A, h, w),                   // AngConvSq
                             lfsr_wgrad_gather(S, S, npix, 64, 16, 1, A, h, w),                   // SpaFE
                             lfsr_wgrad_gather(S, S, nlr, 64, angfe_kpad(A), 1, A, h, w)})        // AngFE
    m = std::max(m, lfsr_wgrad_part_floats(g));
  return m;
}

void train_layout(const lfsr_internet* c, int B, int h, int w, LfsrArena& ws, InterTrainWs& t) {
  const int A = c->A, AA = A * A;
  const size_t npix = (size_t)B * AA * h * w, nlr = (size_t)B * h * w;
  for (int l = 0; l <= NLAYER; ++l) { t.S[l] = ws.take(npix * 128); t.Ar[l] = ws.take(nlr * 128); }
  for (int l = 0; l < NLAYER; ++l) { t.RS[l] = ws.take(npix * 64); t.RA[l] = ws.take(nlr * 64); }
  t.CS = ws.take(npix * 64 * (NG + 1)); t.CA = ws.take(nlr * 64 * NG); t.BA = ws.take(nlr * 64); t.RB = ws.take(npix * 64); t.BO = ws.take(npix * 64);
  for (int l = 0; l < NLAYER; ++l) {
    t.ScLo[l] = ws.take(lfsr_tr3_floats()); t.ScHi[l] = ws.take(lfsr_tr3_floats()); t.AcT[l] = ws.take(128 * 64);
    t.A2sT[l] = ws.take((size_t)AA * 64 * 64); t.S2aT[l] = ws.take((size_t)AA * 64 * 64);
  }
  for (int j = 0; j <= NG; ++j) t.SbT[j] = ws.take(lfsr_tr3_floats());
  t.AbT = ws.take(64 * NG * 64); t.BA2sT = ws.take((size_t)AA * 64 * 64); t.FoldT = ws.take(9 * 64 * 16);
  t.G16 = ws.take(npix * 16); t.dBO = ws.take(npix * 64); t.dZ = ws.take(npix * 64); t.dCS = ws.take(npix * 64 * (NG + 1));
  t.dOs[0] = ws.take(npix * 64); t.dOs[1] = ws.take(npix * 64); t.dSP = ws.take(npix * 64);
  t.dOa[0] = ws.take(nlr * 64); t.dOa[1] = ws.take(nlr * 64); t.dzA = ws.take(nlr * 64); t.dG2 = ws.take(nlr * 64); t.dCA = ws.take(nlr * 64 * NG); t.dZa = ws.take(nlr * 64);
  t.XG9 = ws.take(npix * 16); t.XA = ws.take(nlr * angfe_kpad(A));
  t.P = ws.take(partial_floats(A, B, h, w)); t.dWf = ws.take(16 * 64 * 9);
}

// geometry the training path covers: the forward's per-tensor bound (the widest tensor, the 320-channel concat, below 2^31 floats), the
// upstream configuration n_groups = n_layers = 4.
// The bound is in floats, not bytes: CS / dCS may span 2 GiB and more, and every launch that touches them then addresses with 64 bits --
// the gather-GEMM takes its non-descriptor loads (launch_gemm's addr32), the 3x3 data gradients into dCS leave the Winograd kernels
// (F(4x4) declines from 1 GiB, F(2x2) from 2 GiB) for the direct halo kernel, whose addresses are long long, as are those of the generic
// weight gradient (k_wgrad: an int pixel index times a long long stride) and of k_ew64 / k_copy64.  Only the pixel COUNT has to fit an int.
bool train_geometry_ok(const lfsr_internet* c, int B, int h, int w) {
  if (!c || B <= 0 || h <= 0 || w <= 0 || c->ngroups != NG || c->nlayers != NL) return false;
  const long long npix = (long long)B * c->A * c->A * h * w;
  return npix < (1LL << 31) / (64 * (NG + 1));
}

std::string chain_key(int g, int l, const char* leaf) {
  return "CascadeInterBlock.body." + std::to_string(g) + ".chained_layers." + std::to_string(l) + "." + leaf;
}

}  // namespace

int lfsr_pack_T_from_fwd(const float* Wp, float* out, int T, int Npad_in, int C, int O, int k0, int Kc, int flip, hipStream_t st) {
  hipLaunchKernelGGL(k_pack_T_from_fwd, dim3(lfsr_cap_grid((long long)T * Kc * O)), dim3(256), 0, st, Wp, out, T, Npad_in, C, O, k0, Kc, flip);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

extern "C" {

size_t lfsr_conv3x3_wide_wgrad_workspace_floats(int cin, int n_img, int h, int w) { return lfsr_wgrad_part_floats(wide_wgrad(cin, n_img, 1, h, w)); }

int lfsr_conv3x3_wide_wgrad(const float* dy, int dy_stride, int dy_choff, const float* x, int x_stride, int x_choff, int cin, float* dw, float* workspace,
                            size_t workspace_floats, int n_img, int h, int w, int accumulate, void* stream) {
  LfsrOpTimer op_t("conv3x3_wide_wgrad", cin, h * w, lfsr_stream(stream));
  if (!dy || !x || !dw || !workspace || (cin != 128 && cin != 320) || n_img <= 0 || h <= 0 || w <= 0) return LFSR_E_ARG;
  if (x_choff < 0 || dy_choff < 0 || x_stride < x_choff + cin || dy_stride < dy_choff + 64 || ((x_stride | x_choff | dy_stride | dy_choff) & 3)) return LFSR_E_ARG;
  if (((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dw | (uintptr_t)workspace) & 15) return LFSR_E_ARG;
  const long long rows = (long long)n_img * h * w, lim = (1LL << 31) / 4;   // an operand span of 2 GiB or more
  if (rows * x_stride >= lim || rows * dy_stride >= lim) return LFSR_E_ARG;
  const size_t need = lfsr_conv3x3_wide_wgrad_workspace_floats(cin, n_img, h, w);
  if (!need) return LFSR_E_ARG;
  if (workspace_floats < need) return LFSR_E_WS;
  LfsrWgrad g = wide_wgrad(cin, n_img, 1, h, w);
  g.G = dy; g.g_stride = dy_stride; g.g_choff = dy_choff; g.X = x; g.x_stride = x_stride; g.x_choff = x_choff;
  g.dW = dw; g.accumulate = accumulate ? 1 : 0; g.part = workspace; g.part_floats = workspace_floats;
  return lfsr_wgrad_run(g, lfsr_stream(stream));
}

size_t lfsr_internet_num_params(const lfsr_internet* c) { return c ? c->P.num_params() : 0; }

int lfsr_internet_param_offset(const lfsr_internet* c, const char* key, size_t* off, size_t* numel) {
  return c ? c->P.param_offset(key, off, numel) : LFSR_E_ARG;
}

size_t lfsr_internet_train_workspace_bytes(const lfsr_internet* c, int B, int h, int w) {
  if (!train_geometry_ok(c, B, h, w)) return 0;
  LfsrArena ws;
  InterTrainWs t;
  train_layout(c, B, h, w, ws, t);
  return ws.bytes();
}

// which: 0 S (layer input rows [xs | spa2], VCL, 128), 1 Ar (layer input rows [xa | ang2], LR, 128), 2 ReLU(SpaConvSq) (VCL, 64),
// 3 ReLU(AngConvSq) (LR, 64), 4 ReLU(SpaBottle) (VCL, 64), 5 ReLU(AngBottle) (LR, 64); index = chain layer g * n_layers + l (0 for 4 / 5)
int lfsr_internet_train_saved(const lfsr_internet* c, int B, int h, int w, int which, int index, size_t* offset_floats, size_t* numel) {
  if (!train_geometry_ok(c, B, h, w) || !offset_floats || !numel || index < 0 || index >= (which <= 3 ? NLAYER : 1)) return LFSR_E_ARG;
  LfsrArena ws = LfsrArena::offsets();
  InterTrainWs t;
  train_layout(c, B, h, w, ws, t);
  const size_t npix = (size_t)B * c->A * c->A * h * w, nlr = (size_t)B * h * w;
  const float* p = nullptr;
  size_t n = 0;
  switch (which) {
    case 0: p = t.S[index]; n = npix * 128; break;
    case 1: p = t.Ar[index]; n = nlr * 128; break;
    case 2: p = t.RS[index]; n = npix * 64; break;
    case 3: p = t.RA[index]; n = nlr * 64; break;
    case 4: p = t.RB; n = npix * 64; break;
    case 5: p = t.BA; n = nlr * 64; break;
    default: return LFSR_E_ARG;
  }
  *offset_floats = ws.offset(p);
  *numel = n;
  return LFSR_OK;
}

int lfsr_internet_forward_train(lfsr_internet* c, const float* x, float* out, int B, int h, int w, void* workspace, size_t workspace_bytes, void* stream) {
  if (!c || !c->run_args_ok(x, out, B, h, w, workspace) || !train_geometry_ok(c, B, h, w)) return LFSR_E_ARG;
  LfsrArena ws(workspace);
  InterTrainWs t;
  train_layout(c, B, h, w, ws, t);
  if (workspace_bytes < ws.bytes()) return LFSR_E_WS;
  const int A = c->A, AA = A * A;
  const long long npix = (long long)B * AA * h * w, nlr = (long long)B * h * w;
  const LfsrParamTable& P = c->P;
  hipStream_t st = lfsr_stream(stream);
  const int cs_stride = 64 * (NG + 1), ca_stride = 64 * NG;
  auto gemm = [&](auto launcher, const float* X, int xs, int xo, const float* Wp, float* Y, int ys, int yo, const float* R1, int r1s, int r1o,
                  int M, int N, int ntaps, int CH, float slope) -> int {
    GemmArgs p{};
    p.X = X; p.x_stride = xs; p.x_choff = xo; p.Wp = Wp; p.Y = Y; p.y_stride = ys; p.y_choff = yo; p.R1 = R1; p.r1_stride = r1s; p.r1_choff = r1o;
    p.M = M; p.N = N; p.Npad = npad32(N); p.A = A; p.AA = AA; p.H = h; p.W = w; p.ntaps = ntaps; p.CH = CH; p.slope = slope; p.S = c->s;
    return launcher(p, st);
  };
  // ---- the packs only the backward reads, transposed from the forward's packs (which the runtime refreshes before every training forward)
  auto packT = [&](const std::string& key, float* o, int T, int Npad_in, int C, int O, int k0, int Kc, int flip) -> int {
    hipLaunchKernelGGL(k_pack_T_from_fwd, dim3(lfsr_cap_grid((long long)T * Kc * O)), dim3(256), 0, st, P.w(key), o, T, Npad_in, C, O, k0, Kc, flip);
    LFSR_CHECK_LAUNCH();
    if (T == 9 && O == 64 && Kc == 64) return lfsr_pack_wino_m(o, o + LFSR_CONV3_WINO2_OFF, LFSR_W_ALL, st);   // the 64 -> 64 3x3 data gradient's Winograd copies
    return LFSR_OK;
  };
  for (int g = 0; g < NG; ++g)
    for (int l = 0; l < NL; ++l) {
      const int i = g * NL + l;
      LFSR_RC(packT(chain_key(g, l, "SpaConvSq.weight"), t.ScLo[i], 9, 64, 128, 64, 0, 64, 1));
      LFSR_RC(packT(chain_key(g, l, "SpaConvSq.weight"), t.ScHi[i], 9, 64, 128, 64, 64, 64, 1));
      LFSR_RC(packT(chain_key(g, l, "AngConvSq.weight"), t.AcT[i], 1, 64, 128, 64, 0, 128, 0));
      LFSR_RC(packT(chain_key(g, l, "Ang2Spa.0.weight"), t.A2sT[i], AA, 64, 64, 64, 0, 64, 0));
      LFSR_RC(packT(chain_key(g, l, "Spa2Ang.weight"), t.S2aT[i], AA, 64, 64, 64, 0, 64, 0));
    }
  for (int j = 0; j <= NG; ++j) LFSR_RC(packT("BottleNeck.SpaBottle.weight", t.SbT[j], 9, 64, 64 * (NG + 1), 64, 64 * j, 64, 1));
  LFSR_RC(packT("BottleNeck.AngBottle.weight", t.AbT, 1, 64, 64 * NG, 64, 0, 64 * NG, 0));
  LFSR_RC(packT("BottleNeck.Ang2Spa.0.weight", t.BA2sT, AA, 64, 64, 64, 0, 64, 0));
  hipLaunchKernelGGL(k_pack_fold_T, dim3((9 * 64 * 16 + 255) / 256), dim3(256), 0, st, P.packed + c->off_wf, t.FoldT, c->s * c->s);
  LFSR_CHECK_LAUNCH();

  // ReLU(wide conv) into its saved buffer: conv3x3_wide_bf16.hip under LFSR_WIDE_TRAIN_ARITH_BF16 (LFSR_ARITH_F32 wins), else the fp32 gather-GEMM as ever
  // (a concat of 2 GiB or more keeps the gather-GEMM and its 64-bit addresses)
  const bool wide_bf16 = lfsr_wide_train_arith() == LFSR_WIDE_TRAIN_ARITH_BF16 && !lfsr_arith_f32() && npix * cs_stride * 4 < (1LL << 31);
  auto wide_relu = [&](const float* X, int xs, int cin, const float* Wp, float* Y) -> int {
    if (wide_bf16) return lfsr_conv3x3_wide_bf16_launch(X, xs, 0, cin, Wp, Y, 64, 0, nullptr, 0, 0, B * AA, h, w, 0.0f, st);
    if (cin == 128) return gemm(launch_gemm<IN_CONV3, OUT_SAME, 128, 2>, X, xs, 0, Wp, Y, 64, 0, nullptr, 0, 0, (int)npix, 64, 9, 64, 0.0f);
    return gemm(launch_gemm<IN_CONV3, OUT_SAME, 320, 2>, X, xs, 0, Wp, Y, 64, 0, nullptr, 0, 0, (int)npix, 64, 9, 64, 0.0f);
  };
  // ---- the forward's launches (internet.hip), every layer into its own buffers
  LFSR_RC(lfsr_internet_angfe(x, P.w("AngFE.0.weight"), t.Ar[0], 128, 0, B, A, h, w, st));
  LFSR_RC(lfsr_initconv_fwd(x, P.w("SpaFE.0.weight"), t.S[0], 128, 0, B, A, h, w, stream));
  for (int g = 0; g < NG; ++g) {
    for (int l = 0; l < NL; ++l) {
      const int i = g * NL + l;
      LFSR_RC(gemm(launch_gemm<IN_ANG, OUT_SAME, 64, 2>, t.S[i], 128, 0, P.w(chain_key(g, l, "Spa2Ang.weight")), t.Ar[i], 128, 64, nullptr, 0, 0, (int)nlr, 64, AA, 64, 0.0f));
      LFSR_RC(gemm(launch_gemm<IN_SAME, OUT_VIEWS, 64, 2>, t.Ar[i], 128, 0, P.w(chain_key(g, l, "Ang2Spa.0.weight")), t.S[i], 128, 64, nullptr, 0, 0, (int)nlr, AA * 64, 1, 64, 1.0f));
      LFSR_RC(lfsr_linear_fwd(t.Ar[i], 128, 0, 128, P.w(chain_key(g, l, "AngConvSq.weight")), nullptr, t.Ar[i], 128, 0, t.Ar[i + 1], 128, 0, nlr, 64, 0.0f, stream));
      LFSR_RC(lfsr_linear_fwd(t.Ar[i], 128, 0, 128, P.w(chain_key(g, l, "AngConvSq.weight")), nullptr, nullptr, 0, 0, t.RA[i], 64, 0, nlr, 64, 0.0f, stream));
      LFSR_RC(wide_relu(t.S[i], 128, 128, P.w(chain_key(g, l, "SpaConvSq.weight")), t.RS[i]));
      LFSR_RC(ew64(t.RS[i], 64, 0, t.S[i], 128, 0, nullptr, 0, 0, t.S[i + 1], 128, 0, npix, st));
    }
    LFSR_RC(lfsr_internet_copy64(t.Ar[(g + 1) * NL], 128, 0, t.CA, ca_stride, 64 * g, nlr, st));
    LFSR_RC(lfsr_internet_copy64(t.S[(g + 1) * NL], 128, 0, t.CS, cs_stride, 64 * g, npix, st));
  }
  LFSR_RC(lfsr_linear_fwd(t.CA, ca_stride, 0, 64 * NG, P.w("BottleNeck.AngBottle.weight"), nullptr, nullptr, 0, 0, t.BA, 64, 0, nlr, 64, 0.0f, stream));
  LFSR_RC(gemm(launch_gemm<IN_SAME, OUT_VIEWS, 64, 2>, t.BA, 64, 0, P.w("BottleNeck.Ang2Spa.0.weight"), t.CS, cs_stride, 64 * NG, nullptr, 0, 0, (int)nlr, AA * 64, 1, 64, 1.0f));
  LFSR_RC(wide_relu(t.CS, cs_stride, cs_stride, P.w("BottleNeck.SpaBottle.weight"), t.RB));
  LFSR_RC(ew64(t.RB, 64, 0, t.S[0], 128, 0, nullptr, 0, 0, t.BO, 64, 0, npix, st));
  LFSR_RC(gemm(launch_gemm<IN_CONV3, OUT_PS_HR, 64, 1>, t.BO, 64, 0, P.packed + c->off_wf, out, 1, 0, nullptr, 0, 0, (int)npix, c->s * c->s, 9, 1, 1.0f));
  return LFSR_OK;
}

int lfsr_internet_backward(lfsr_internet* c, const float* x, const float* dout, int B, int h, int w, void* workspace, size_t workspace_bytes,
                           float* grads, size_t n_grads, void* stream) {
  if (!c || !c->run_args_ok(x, dout, B, h, w, workspace) || !grads || !train_geometry_ok(c, B, h, w) || n_grads != c->P.num_params()) return LFSR_E_ARG;
  LfsrArena ws(workspace);
  InterTrainWs t;
  train_layout(c, B, h, w, ws, t);
  if (workspace_bytes < ws.bytes()) return LFSR_E_WS;
  const int A = c->A, AA = A * A, s2 = c->s * c->s, nimg = B * AA;
  const int npix = nimg * h * w, nlr = B * h * w;
  const int cs_stride = 64 * (NG + 1), ca_stride = 64 * NG;
  const LfsrParamTable& P = c->P;
  hipStream_t st = lfsr_stream(stream);
  auto G = [&](const std::string& k) -> float* { return grads + P.grad_off(k); };
  // gather-GEMM data gradient: identity epilogue, optional R1 (may alias Y: in-place accumulate) and ReLU' mask Mk (> 0 keeps)
  auto gemm = [&](auto launcher, const float* X, int xs, int xo, const float* Wp, float* Y, int ys, int yo, const float* R1, int r1s, int r1o,
                  const float* Mk, int mks, int mko, int M, int N, int ntaps, int CH) -> int {
    GemmArgs p{};
    p.X = X; p.x_stride = xs; p.x_choff = xo; p.Wp = Wp; p.Y = Y; p.y_stride = ys; p.y_choff = yo; p.R1 = R1; p.r1_stride = r1s; p.r1_choff = r1o;
    p.Mk = Mk; p.mk_stride = mks; p.mk_choff = mko; p.mk_slope = 0.0f;
    p.M = M; p.N = N; p.Npad = npad32(N); p.A = A; p.AA = AA; p.H = h; p.W = w; p.ntaps = ntaps; p.CH = CH; p.slope = 1.0f; p.S = c->s;
    return launcher(p, st);
  };
  // weight gradient: partial slabs, then the fixed-order reduce into the bucket (raw PyTorch layout); (O, C, T) = 0: (N, K, ntaps)
  const size_t pfloats = partial_floats(A, B, h, w);
  auto wgrad = [&](int gm, int xm, const float* Gr, int gs, int go, const float* X, int xs, int xo, int M, int N, int K, int ntaps, float* dW,
                   int O, int C, int T, int perm, int ch, int c_valid, int chunk) -> int {
    LfsrWgrad g = lfsr_wgrad_gather(gm, xm, M, N, K, ntaps, A, h, w);
    g.G = Gr; g.g_stride = gs; g.g_choff = go; g.X = X; g.x_stride = xs; g.x_choff = xo;
    g.dW = dW; g.O = O; g.C = C; g.T = T; g.perm = perm; g.ch = ch; g.c_valid = c_valid; g.chunk_mode = chunk; g.part = t.P; g.part_floats = pfloats;
    return lfsr_wgrad_run(g, st);
  };
  auto wgrad_wide = [&](const float* X, int xs, int cin, float* dW) -> int {
    LfsrWgrad g = wide_wgrad(cin, B, A, h, w);
    g.G = t.dZ; g.X = X; g.x_stride = xs; g.dW = dW; g.part = t.P; g.part_floats = pfloats;
    return lfsr_wgrad_run(g, st);
  };
  auto dgrad3 = [&](const float* dy, const float* wT, float* dx, int dxs, int dxo, const float* r1) -> int {
    return lfsr_conv3x3_bwd_data(dy, 64, 0, wT, dx, dxs, dxo, r1, 64, 0, nullptr, 0, 0, 1.0f, nimg, h, w, st);
  };

  // ---- ReconBlock (folded 3x3 conv 64 -> s^2 + MacPI2SAI + PixelShuffle(s)) ----------------------------------------------------------
  hipLaunchKernelGGL(k_unshuffle_hr, dim3(lfsr_cap_grid((long long)npix * 16)), dim3(256), 0, st, dout, t.G16, B, A, h, w, c->s);
  LFSR_CHECK_LAUNCH();
  LFSR_RC(gemm(launch_gemm<IN_CONV3, OUT_SAME, 16, 2>, t.G16, 16, 0, t.FoldT, t.dBO, 64, 0, nullptr, 0, 0, nullptr, 0, 0, npix, 64, 9, 64));
  LFSR_RC(wgrad(LFSR_IN_SAME, LFSR_IN_CONV3, t.G16, 16, 0, t.BO, 64, 0, npix, 16, 64, 9, t.dWf, 16, 64, 9, 0, 0, 0, 0));
  hipLaunchKernelGGL(k_fold_bwd, dim3(64), dim3(256), 0, st, t.dWf, P.w("ReconBlock.PreConv.weight"), P.w("ReconBlock.FinalConv.weight"),
                     G("ReconBlock.PreConv.weight"), G("ReconBlock.FinalConv.weight"), s2);
  LFSR_CHECK_LAUNCH();

  // ---- BottleNeck: BO = ReLU(SpaBottle(CS)) + xs, CS[:, 256:320] = PS(Ang2Spa(a)), a = ReLU(AngBottle(CA)) --------------------------------
  LFSR_RC(ew64(t.dBO, 64, 0, nullptr, 0, 0, t.RB, 64, 0, t.dZ, 64, 0, npix, st));
  LFSR_RC(wgrad_wide(t.CS, cs_stride, cs_stride, G("BottleNeck.SpaBottle.weight")));
  for (int j = 0; j <= NG; ++j) LFSR_RC(dgrad3(t.dZ, t.SbT[j], t.dCS, cs_stride, 64 * j, nullptr));
  LFSR_RC(gemm(launch_gemm<IN_ANG, OUT_SAME, 64, 2>, t.dCS, cs_stride, 64 * NG, t.BA2sT, t.dZa, 64, 0, nullptr, 0, 0, t.BA, 64, 0, nlr, 64, AA, 64));
  LFSR_RC(wgrad(LFSR_IN_ANG, LFSR_IN_SAME, t.dCS, cs_stride, 64 * NG, t.BA, 64, 0, nlr, 64, 64, AA, G("BottleNeck.Ang2Spa.0.weight"), AA * 64, 64, AA, 1, 64, 0, 1));
  LFSR_RC(gemm(launch_gemm<IN_SAME, OUT_SAME, 64, 2>, t.dZa, 64, 0, t.AbT, t.dCA, ca_stride, 0, nullptr, 0, 0, nullptr, 0, 0, nlr, ca_stride, 1, ca_stride));
  LFSR_RC(wgrad(LFSR_IN_SAME, LFSR_IN_SAME, t.dZa, 64, 0, t.CA, ca_stride, 0, nlr, 64, ca_stride, 1, G("BottleNeck.AngBottle.weight"), 64, ca_stride, 1, 0, 0, 0, 0));

  // ---- cascade, reversed.  dOs / dOa: the gradient at the current layer's outputs out_s (VCL, 64) and out_a (LR, 64) ------------------------
  int cur = 0;
  for (int g = NG - 1; g >= 0; --g) {
    // the group's output also went into the concat buffers
    if (g == NG - 1) {
      LFSR_RC(ew64(t.dCS, cs_stride, 64 * g, nullptr, 0, 0, nullptr, 0, 0, t.dOs[cur], 64, 0, npix, st));
      LFSR_RC(ew64(t.dCA, ca_stride, 64 * g, nullptr, 0, 0, nullptr, 0, 0, t.dOa[cur], 64, 0, nlr, st));
    } else {
      LFSR_RC(ew64(t.dOs[cur], 64, 0, t.dCS, cs_stride, 64 * g, nullptr, 0, 0, t.dOs[cur], 64, 0, npix, st));
      LFSR_RC(ew64(t.dOa[cur], 64, 0, t.dCA, ca_stride, 64 * g, nullptr, 0, 0, t.dOa[cur], 64, 0, nlr, st));
    }
    for (int l = NL - 1; l >= 0; --l) {
      const int i = g * NL + l, nxt = cur ^ 1;
      float *dOs = t.dOs[cur], *dOa = t.dOa[cur], *dxs = t.dOs[nxt], *dxa = t.dOa[nxt];
      // out_s = ReLU(SpaConvSq([xs | spa2])) + xs ; out_a = ReLU(AngConvSq([xa | ang2])) + xa
      LFSR_RC(ew64(dOs, 64, 0, nullptr, 0, 0, t.RS[i], 64, 0, t.dZ, 64, 0, npix, st));
      LFSR_RC(ew64(dOa, 64, 0, nullptr, 0, 0, t.RA[i], 64, 0, t.dzA, 64, 0, nlr, st));
      // AngConvSq: dxa = dzA W[:, :64]^T + dOa ; dang2 = (dzA W[:, 64:]^T) * [ang2 > 0]
      LFSR_RC(wgrad(LFSR_IN_SAME, LFSR_IN_SAME, t.dzA, 64, 0, t.Ar[i], 128, 0, nlr, 64, 128, 1, G(chain_key(g, l, "AngConvSq.weight")), 64, 128, 1, 0, 0, 0, 0));
      LFSR_RC(gemm(launch_gemm<IN_SAME, OUT_SAME, 64, 2>, t.dzA, 64, 0, t.AcT[i], dxa, 64, 0, dOa, 64, 0, nullptr, 0, 0, nlr, 64, 1, 64));
      LFSR_RC(gemm(launch_gemm<IN_SAME, OUT_SAME, 64, 2>, t.dzA, 64, 0, t.AcT[i] + 64 * 64, t.dG2, 64, 0, nullptr, 0, 0, t.Ar[i], 128, 64, nlr, 64, 1, 64));
      // SpaConvSq: dxs = conv3^T(dzS; W[:, :64]) + dOs ; dspa2 = conv3^T(dzS; W[:, 64:])
      LFSR_RC(wgrad_wide(t.S[i], 128, 128, G(chain_key(g, l, "SpaConvSq.weight"))));
      LFSR_RC(dgrad3(t.dZ, t.ScLo[i], dxs, 64, 0, dOs));
      LFSR_RC(dgrad3(t.dZ, t.ScHi[i], t.dSP, 64, 0, nullptr));
      // Ang2Spa: spa2 = PS(W xa) -> dxa += sum over the views (IN_ANG gather of dspa2)
      LFSR_RC(gemm(launch_gemm<IN_ANG, OUT_SAME, 64, 2>, t.dSP, 64, 0, t.A2sT[i], dxa, 64, 0, dxa, 64, 0, nullptr, 0, 0, nlr, 64, AA, 64));
      LFSR_RC(wgrad(LFSR_IN_ANG, LFSR_IN_SAME, t.dSP, 64, 0, t.Ar[i], 128, 0, nlr, 64, 64, AA, G(chain_key(g, l, "Ang2Spa.0.weight")), AA * 64, 64, AA, 1, 64, 0, 1));
      // Spa2Ang: ang2 = ReLU(convAxA(xs)) -> dxs += the OUT_VIEWS scatter of the masked dang2 (each view pixel has one LR pixel: no atomics)
      LFSR_RC(gemm(launch_gemm<IN_SAME, OUT_VIEWS, 64, 2>, t.dG2, 64, 0, t.S2aT[i], dxs, 64, 0, dxs, 64, 0, nullptr, 0, 0, nlr, AA * 64, 1, 64));
      LFSR_RC(wgrad(LFSR_IN_SAME, LFSR_IN_ANG, t.dG2, 64, 0, t.S[i], 128, 0, nlr, 64, 64, AA, G(chain_key(g, l, "Spa2Ang.weight")), 64, 64, AA, 0, 0, 0, 0));
      cur = nxt;
    }
  }

  // ---- feature extraction: xs = SpaFE(x) (also the BottleNeck skip), xa = AngFE(x) ----------------------------------------------------
  LFSR_RC(ew64(t.dOs[cur], 64, 0, t.dBO, 64, 0, nullptr, 0, 0, t.dOs[cur], 64, 0, npix, st));
  LFSR_RC(lfsr_init_gather9(x, t.XG9, B, A, h, w, st));
  LFSR_RC(wgrad(LFSR_IN_SAME, LFSR_IN_SAME, t.dOs[cur], 64, 0, t.XG9, 16, 0, npix, 64, 16, 1, G("SpaFE.0.weight"), 64, 16, 1, 0, 0, 9, 0));
  const int kp = angfe_kpad(A);
  hipLaunchKernelGGL(k_angfe_gather, dim3(lfsr_cap_grid((long long)nlr * kp)), dim3(256), 0, st, x, t.XA, B, A, h, w, kp);
  LFSR_CHECK_LAUNCH();
  LFSR_RC(wgrad(LFSR_IN_SAME, LFSR_IN_SAME, t.dOa[cur], 64, 0, t.XA, kp, 0, nlr, 64, kp, 1, G("AngFE.0.weight"), 64, kp, 1, 0, 0, AA, 0));
  return LFSR_OK;
}

}  // extern "C"
