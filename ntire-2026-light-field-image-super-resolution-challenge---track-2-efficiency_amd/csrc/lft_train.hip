// LFT training: the forward that keeps what the backward reads, and the backward (autograd of model/SR/LFT.py:67-98 as driven by
// train.py:256-264, fp32; the graph of oracle/lfsr_torch_port.py::lft_forward is the spec).  Rows are VCL pixels as in the forward (lft.cpp).
//
// forward_train runs lfsr_lft_forward_body, the inference forward's launches, on buffers of its own per layer: the AltFilter inputs, the
// attention's q | k, v and output, the feed-forward inputs and outputs and the spatial tokens.  The fused launches keep no LayerNorm
// statistics, feed-forward hidden rows or HR map: the backward recomputes those from the saved sublayer inputs with the unfused kernels.
//
// Backward: data gradients are gather-GEMMs over transposed packs (gemm_gather_kernel.h) and the 64 -> 64 3x3 data-gradient kernel;
// weight gradients are the two-pass partial-slab reduction of wgrad.hip.  The windowed attention backward (two gathers, one per query and one
// per key: no float atomics), the LayerNorm backward with the position embedding added to its input, the tail's LeakyReLU / 3x3 conv backward
// with the HR -> LR un-shuffle and the small fixed-order reductions are the kernels of trans_bwd.hip, which EPIT's backward shares.  Buckets
// are bitwise reproducible.
#include <string>
#include <vector>

#include "gemm_gather_kernel.h"
#include "lft_ctx.h"

namespace {

// dspe[p][c] = sum over the n_img images of dln[img * HW + p][c] (128 channels), in image order
__global__ __launch_bounds__(256) void k_pe_reduce(const float* __restrict__ dln, float* __restrict__ dspe, int n_img, int HW) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)HW * 128) return;
  float s = 0.f;
  for (int i = 0; i < n_img; ++i) s += dln[(long long)i * HW * 128 + e];
  dspe[e] = s;
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
  t.part = ws.take(wgrad_partial_max(B, c->A, h, w)); t.pln = ws.take((size_t)LFSR_RED_BLOCKS * 256); t.ptail = ws.take((size_t)LFSR_RED_BLOCKS * 9 * 64);
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
    return lfsr_ew_launch(a, as, b, bs, mk, ms, slope, d, ds, C, M, st);
  };
  // LayerNorm backward with the gradients of its affine parameters written to dg / dbeta
  auto ln_bwd = [&](int C, const float* X, const float* pe, long long pe_rows, long long pe_div, const std::string& gkey, const std::string& bkey,
                    const float* dy, const float* r, float* dxo) -> int {
    return lfsr_ln_bwd_launch(C, X, pe, pe_rows, pe_div, P.w(gkey), dy, r, dxo, t.pln, npix, G(gkey), G(bkey), st);
  };
  auto attn_bwd = [&](int hd, const float* qk, int qks, int kchoff, const float* V, int vs, const float* O, const float* dO, int os, float* dqk, float* dv,
                      int ns0, int ns1, int ns2, long long bs0, long long bs1, long long bs2, int n1, int n2, long long st1, long long st2,
                      int l1, int r1, int l2, int r2, int clip2) -> int {
    return lfsr_attn_bwd_valu_launch(hd, qk, qks, 0, kchoff, V, vs, O, dO, os, dqk, dv, reinterpret_cast<float*>(t.stats), 8, ns0, ns1, ns2, bs0, bs1, bs2,
                                     n1, n2, st1, st2, l1, r1, l2, r2, clip2, st);
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
  LFSR_RC(lfsr_tail_bwd_launch(dout, P.w("upsampling.3.weight"), t.hr, t.du, t.ptail, G("upsampling.3.weight"), B, A, h, w, S, L, st));
  LFSR_RC(lfsr_pack_up0_T_launch(P.w("upsampling.0.weight"), t.up0T, s2, st));
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
