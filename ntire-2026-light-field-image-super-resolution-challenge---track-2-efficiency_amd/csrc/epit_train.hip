// EPIT training: the forward that keeps what the backward reads, and the backward (autograd of model/SR/EPIT.py:51-71, AltFilter :144-161,
// BasicTrans :110-128, fp32; the graph of oracle/lfsr_torch_port.py::epit_forward is the spec).  Rows are VCL pixels as in the forward (epit.cpp).
//
// forward_train runs lfsr_epit_forward_body, the inference forward's launches, on buffers of its own per (block, pass): every sublayer's
// input.  The fused launches keep no LayerNorm statistics, feed-forward hidden rows or HR map: the backward recomputes those from the saved
// sublayer inputs with the unfused kernels, as LFT's does (lft_train.hip), and shares its kernels (trans_bwd.hip, wgrad.hip, the gather-GEMMs).
//
// An AltFilter runs ONE epi_trans and ONE conv stack in both passes: each of its 13 weights gets the sum of two contributions.  The vertical
// pass (the later one in the forward) writes the bucket, the horizontal pass writes a scratch image of the block's span of the bucket, and one
// elementwise add joins them: a fixed order, so buckets are bitwise reproducible.  The block input is added after BOTH passes
// (t1 = conv(trans_H(x)) + x, x' = conv(trans_V(t1)) + x): dx = dx' + dt1 + trans_H's input gradient, dt1 = trans_V's input gradient.
#include <string>
#include <vector>

#include "epit_ctx.h"
#include "gemm_gather_kernel.h"

namespace {

inline size_t tr3_floats() { return lfsr_packed_weight_tr_floats(64, 64, 9); }

struct EpitTrainWs {
  EpitFwdBufs f;                      // saved by forward_train (the scratch members point into the backward scratch below)
  // backward scratch
  float *hr, *du, *dx[2], *dbuf0, *dsf, *dh, *dln, *dsm, *dso, *dqk, *dv, *dst, *lnt, *d64, *t64, *r4, *xg9, *stats, *gtmp;
  std::vector<float*> hid;            // the feed-forward hidden rows (after the ReLU) the backward rebuilt, per (block, pass): its ReLU decisions
  float *part, *pln, *ptail;
  // transposed packs, rebuilt from the current packed weights by every backward
  float *up0T, *initT[3], *convT[3];  // convT: one block's conv stack (rebuilt for every block)
  float* lin[7];                      // one block's 1x1 dgrad packs
};

size_t wgrad_partial_max(int B, int A, int h, int w) {
  const size_t npix = (size_t)B * A * A * h * w;
  size_t m = 0;
  auto up = [&](size_t v) { if (v > m) m = v; };
  for (int K : {16, 64, 128, 256}) up(lfsr_wgrad_partial_floats((int)npix, 1, 64, K));
  up(lfsr_wgrad_partial_floats((int)npix, 9, 64, 64));
  return m;
}

// geometry the training path covers: every activation below 2 GiB (the widest rows: the 256-float q | k, and the HR map of 64 s^2 floats per LR pixel)
bool train_geometry_ok(const lfsr_epit* c, int B, int h, int w) {
  if (!c || B <= 0 || h <= 0 || w <= 0 || c->s < 2 || c->s > 4) return false;
  const long long npix = (long long)B * c->A * c->A * h * w;
  const long long widest = 64LL * c->s * c->s > 256 ? 64LL * c->s * c->s : 256;
  return npix * widest * 4 < (1LL << 31);
}

size_t block_grad_floats(const lfsr_epit* c) {
  return c->P.grad_off("altblock.0.conv.4.weight") + (size_t)64 * 64 * 9 - c->P.grad_off("altblock.0.epi_trans.linear_in.weight");
}

void train_layout(const lfsr_epit* c, int B, int h, int w, LfsrArena& ws, EpitTrainWs& t) {
  const int nb = c->nblk, s2 = c->s * c->s;
  const size_t npix = (size_t)B * c->A * c->A * h * w;
  EpitFwdBufs& f = t.f;
  f.f0 = ws.take(npix * 64); f.c1i = ws.take(npix * 64); f.c2i = ws.take(npix * 64); f.buf0 = ws.take(npix * 64);
  f.x.assign(nb + 1, nullptr);
  f.x[0] = f.buf0;
  for (int b = 0; b < nb; ++b) {
    f.mid.push_back(ws.take(npix * 64));
    f.x[b + 1] = ws.take(npix * 64);
    for (int v = 0; v < 2; ++v) {
      f.t.push_back(ws.take(npix * 128)); f.qk.push_back(ws.take(npix * 256)); f.v.push_back(ws.take(npix * 128)); f.ao.push_back(ws.take(npix * 128));
      f.t2.push_back(ws.take(npix * 128)); f.tf.push_back(ws.take(npix * 128)); f.y.push_back(ws.take(npix * 64)); f.c1.push_back(ws.take(npix * 64));
      f.c2.push_back(ws.take(npix * 64));
    }
  }
  t.hr = ws.take(npix * 64 * s2); t.du = ws.take(npix * 64 * s2);
  t.dx[0] = ws.take(npix * 64); t.dx[1] = ws.take(npix * 64); t.dbuf0 = ws.take(npix * 64);
  t.dsf = ws.take(npix * 128); t.dh = ws.take(npix * 256); t.dln = ws.take(npix * 128); t.dsm = ws.take(npix * 128); t.dso = ws.take(npix * 128);
  t.dqk = ws.take(npix * 256); t.dv = ws.take(npix * 128); t.dst = ws.take(npix * 128); t.lnt = ws.take(npix * 128);
  t.d64 = ws.take(npix * 64); t.t64 = ws.take(npix * 64); t.r4 = ws.take(npix * 64); t.xg9 = ws.take(npix * 16);
  t.stats = ws.take(npix * 8 * 4);
  t.gtmp = ws.take(block_grad_floats(c));
  t.hid.clear();
  for (int j = 0; j < 2 * nb; ++j) t.hid.push_back(ws.take(npix * 256));
  t.part = ws.take(wgrad_partial_max(B, c->A, h, w)); t.pln = ws.take((size_t)LFSR_RED_BLOCKS * 256); t.ptail = ws.take((size_t)LFSR_RED_BLOCKS * 9 * 64);
  // the forward body's scratch (unfused LayerNorm outputs, two-launch feed-forward hidden rows, the unfused tail's HR map)
  f.tn = t.lnt; f.lnx = t.dln; f.hid = t.dh; f.hr = t.hr;
  t.up0T = ws.take((size_t)64 * 64 * s2);
  for (int i = 0; i < 3; ++i) t.initT[i] = ws.take(tr3_floats());
  for (int i = 0; i < 3; ++i) t.convT[i] = ws.take(tr3_floats());
  for (float*& l : t.lin) l = ws.take(256 * 128);       // the largest: [128][256]
}

}  // namespace

extern "C" {

// the gradient bucket: state_dict order (EPIT.py module creation order); the feed-forward weights' pre-split image is no entry
size_t lfsr_epit_num_params(const lfsr_epit* c) { return c ? c->P.num_params() : 0; }

int lfsr_epit_param_offset(const lfsr_epit* c, const char* key, size_t* off, size_t* numel) { return c ? c->P.param_offset(key, off, numel) : LFSR_E_ARG; }

size_t lfsr_epit_train_workspace_bytes(const lfsr_epit* c, int B, int h, int w) {
  if (!train_geometry_ok(c, B, h, w)) return 0;
  LfsrArena ws;
  EpitTrainWs t;
  train_layout(c, B, h, w, ws, t);
  return ws.bytes();
}

// which (pass index j = 2 block + vertical): 0 the input of AltFilter `index` (index = n_block: the altblock output plus the network skip, the
// tail's input), 1 conv_init's LeakyReLU outputs (index 0: conv_init.0, 1: conv_init.2), 2 / 3 the LeakyReLU outputs of conv.0 / conv.2 of pass
// `index`: VCL rows of 64 floats.  After a backward, what it rebuilt and took its ReLU / LeakyReLU decisions from: 4 the feed-forward hidden rows
// after the ReLU of pass `index` (256), 5 conv_init.4's LeakyReLU output without the residual (64; index 0), 6 the HR pre-activation (the
// channel-last mosaic (B, A h s, A w s, 64); index 0).
int lfsr_epit_train_saved(const lfsr_epit* c, int B, int h, int w, int which, int index, size_t* offset_floats, size_t* numel) {
  if (!train_geometry_ok(c, B, h, w) || !offset_floats || !numel || index < 0) return LFSR_E_ARG;
  const int nb = c->nblk;
  if (index >= (which == 0 ? nb + 1 : which == 1 ? 2 : which >= 5 ? 1 : 2 * nb)) return LFSR_E_ARG;
  LfsrArena ws = LfsrArena::offsets();
  EpitTrainWs t;
  train_layout(c, B, h, w, ws, t);
  const size_t npix = (size_t)B * c->A * c->A * h * w;
  const float* p = nullptr;
  size_t n = npix * 64;
  switch (which) {
    case 0: p = t.f.x[index]; break;
    case 1: p = index ? t.f.c2i : t.f.c1i; break;
    case 2: p = t.f.c1[index]; break;
    case 3: p = t.f.c2[index]; break;
    case 4: p = t.hid[index]; n = npix * 256; break;
    case 5: p = t.r4; break;
    case 6: p = t.hr; n = npix * 64 * c->s * c->s; break;
    default: return LFSR_E_ARG;
  }
  *offset_floats = ws.offset(p);
  *numel = n;
  return LFSR_OK;
}

int lfsr_epit_forward_train(lfsr_epit* c, const float* x, float* out, int B, int h, int w, void* workspace, size_t workspace_bytes, void* stream) {
  if (!c || !c->run_args_ok(x, out, B, h, w, workspace) || !train_geometry_ok(c, B, h, w)) return LFSR_E_ARG;
  LfsrArena ws(workspace);
  EpitTrainWs t;
  train_layout(c, B, h, w, ws, t);
  if (workspace_bytes < ws.bytes()) return LFSR_E_WS;
  return lfsr_epit_forward_body(c, x, out, B, h, w, t.f, stream);
}

int lfsr_epit_backward(lfsr_epit* c, const float* x, const float* dout, int B, int h, int w, void* workspace, size_t workspace_bytes,
                       float* grads, size_t n_grads, void* stream) {
  if (!c || !c->run_args_ok(x, dout, B, h, w, workspace) || !grads || !train_geometry_ok(c, B, h, w) || n_grads != c->P.num_params()) return LFSR_E_ARG;
  LfsrArena ws(workspace);
  EpitTrainWs t;
  train_layout(c, B, h, w, ws, t);
  if (workspace_bytes < ws.bytes()) return LFSR_E_WS;
  const int A = c->A, AA = A * A, S = c->s, s2 = S * S, nimg = B * AA, HW = h * w, nb = c->nblk;
  const int npix = nimg * HW;
  const float L = 0.2f;
  const LfsrParamTable& P = c->P;
  const EpitFwdBufs& f = t.f;
  hipStream_t st = lfsr_stream(stream);
  float* gbase = grads;     // where G() points: the bucket, or (horizontal pass) the scratch image of the block's span of it
  auto G = [&](const std::string& k) -> float* { return gbase + P.grad_off(k); };
  // 1x1 data gradient Y (N columns) = X (CIN columns) . WT, then * (Mk > 0 ? 1 : 0) (ReLU'), then + R1 (may alias Y)
  auto dgemm = [&](auto launcher, const float* X, int xs, const float* WT, float* Y, int ys, const float* R1, int r1s, const float* Mk, int mks, int N) -> int {
    GemmArgs p{};
    p.X = X; p.x_stride = xs; p.Wp = WT; p.Y = Y; p.y_stride = ys; p.R1 = R1; p.r1_stride = r1s; p.Mk = Mk; p.mk_stride = mks; p.mk_slope = 0.0f;
    p.M = npix; p.N = N; p.Npad = npad32(N); p.A = A; p.H = h; p.W = w; p.ntaps = 1; p.CH = N; p.slope = 1.0f; p.S = S;
    return launcher(p, st);
  };
  // weight gradient of output rows [n0, n0 + N) (N <= 64) of a raw (O, C, T) weight: partial slabs, then the fixed-order reduce
  auto wgrad = [&](int xm, const float* Gr, int gs, int go, const float* X, int xs, int N, int K, int ntaps, float* dW, int c_valid = 0) -> int {
    int r = lfsr_wgrad_launch(LFSR_IN_SAME, xm, Gr, gs, go, X, xs, 0, t.part, npix, N, K, A, h, w, ntaps, st);
    if (!r) r = lfsr_wgrad_reduce(t.part, lfsr_wgrad_splits(npix, ntaps, K), nullptr, 0, dW, N, K, ntaps, 0, 0, 0, c_valid, 0, st);
    return r;
  };
  // every 64-row slice of a (O, K) linear weight's gradient: G (O columns, stride gs) against X (K columns)
  auto wgrad_lin = [&](const float* Gr, int gs, int O, const float* X, int xs, int K, float* dW) -> int {
    for (int n0 = 0; n0 < O; n0 += 64) LFSR_RC(wgrad(LFSR_IN_SAME, Gr, gs, n0, X, xs, 64, K, 1, dW + (size_t)n0 * K));
    return LFSR_OK;
  };
  auto ew = [&](const float* a, const float* b, const float* mk, float slope, float* d) -> int {     // 64-float rows
    return lfsr_ew_launch(a, 64, b, 64, mk, 64, slope, d, 64, 64, npix, st);
  };
  auto ln_bwd = [&](const float* X, const std::string& gkey, const std::string& bkey, const float* dy, const float* r, float* dxo) -> int {
    return lfsr_ln_bwd_launch(128, X, nullptr, 1, 1, P.w(gkey), dy, r, dxo, t.pln, npix, G(gkey), G(bkey), st);
  };
  auto dgrad3 = [&](const float* dy, const float* wT, float* dxo, const float* r1, const float* mk) -> int {
    return lfsr_conv3x3_bwd_data(dy, 64, 0, wT, dxo, 64, 0, r1, 64, 0, mk, 64, 0, L, nimg, h, w, st);
  };
  // 1x1 dgrad pack of rows [n0, n0 + O) of a (Npad_in, C) forward pack: [C][O]
  auto packT = [&](const float* Wp, int n0, int C, int O, float* o) -> int { return lfsr_pack_T_from_fwd(Wp + (size_t)n0 * C, o, 1, O, C, O, 0, C, 0, st); };
  auto pack3T = [&](const std::string& key, float* o) -> int {
    LFSR_RC(lfsr_pack_T_from_fwd(P.w(key), o, 9, 64, 64, 64, 0, 64, 1, st));
    return lfsr_pack_wino_m(o, o + LFSR_CONV3_WINO2_OFF, LFSR_W_ALL, st);   // the 64 -> 64 3x3 data gradient's Winograd copies
  };

  // ---- tail: upsampling.0 (1x1 64 -> 64 s^2), PixelShuffle(s), LeakyReLU 0.2, 3x3 conv 64 -> 1, + bicubic skip (no parameters) ----------
  LFSR_RC(lfsr_upsample_ps_fwd(f.x[nb], 64, 0, P.w("upsampling.0.weight"), t.hr, B, A, h, w, S, stream));   // the HR pre-activation, rebuilt
  LFSR_RC(lfsr_tail_bwd_launch(dout, P.w("upsampling.3.weight"), t.hr, t.du, t.ptail, G("upsampling.3.weight"), B, A, h, w, S, L, st));
  LFSR_RC(lfsr_pack_up0_T_launch(P.w("upsampling.0.weight"), t.up0T, s2, st));
  float* dX = t.dx[0];   // the gradient at the altblock output (+ the network skip): dL/d x[nb]
  if (s2 == 4) LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 256, 2>, t.du, 256, t.up0T, dX, 64, nullptr, 0, nullptr, 0, 64));
  else if (s2 == 9) LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 576, 2>, t.du, 576, t.up0T, dX, 64, nullptr, 0, nullptr, 0, 64));
  else LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 1024, 2>, t.du, 1024, t.up0T, dX, 64, nullptr, 0, nullptr, 0, 64));
  for (int n0 = 0; n0 < 64 * s2; n0 += 64) LFSR_RC(wgrad(LFSR_IN_SAME, t.du, 64 * s2, n0, f.x[nb], 64, 64, 64, 1, G("upsampling.0.weight") + (size_t)n0 * 64));

  // ---- altblock, reversed.  EPIT.py:66 buffer = altblock(buffer) + buffer: dX also reaches buf0 directly ----------------------------------
  LFSR_RC(ew(dX, nullptr, nullptr, 1.0f, t.dbuf0));
  float* dT1 = t.dx[1];
  for (int b = nb - 1; b >= 0; --b) {
    const std::string bp = "altblock." + std::to_string(b) + ".", e = bp + "epi_trans.";
    float** lin = t.lin;
    // the block's dgrad packs, shared by both passes: [C_in][O] of every linear weight (q | k and v as separate row ranges of in_proj)
    LFSR_RC(packT(P.w(e + "linear_out.weight"), 0, 128, 64, lin[0]));
    LFSR_RC(packT(P.w(e + "feed_forward.4.weight"), 0, 256, 128, lin[1]));
    LFSR_RC(packT(P.w(e + "feed_forward.1.weight"), 0, 128, 256, lin[2]));
    LFSR_RC(packT(P.w(e + "attention.out_proj.weight"), 0, 128, 128, lin[3]));
    LFSR_RC(packT(P.w(e + "attention.in_proj_weight"), 0, 128, 256, lin[4]));
    LFSR_RC(packT(P.w(e + "attention.in_proj_weight"), 256, 128, 128, lin[5]));
    LFSR_RC(packT(P.w(e + "linear_in.weight"), 0, 64, 128, lin[6]));
    for (int i = 0; i < 3; ++i) LFSR_RC(pack3T(bp + "conv." + std::to_string(2 * i) + ".weight", t.convT[i]));
    const size_t blk_off = P.grad_off(e + "linear_in.weight"), blk_n = block_grad_floats(c);

    for (int vert = 1; vert >= 0; --vert) {
      const int j = 2 * b + vert;
      const float* Xin = vert ? f.mid[b] : f.x[b];        // the transformer's input
      const float* dOut = vert ? dX : dT1;                // the gradient at conv.4's output (the shortcut takes it to x[b] as it stands)
      gbase = vert ? grads : t.gtmp - blk_off;
      // ---- conv stack (EPIT.py:136-141): conv.4(lrelu(conv.2(lrelu(conv.0(y))))) ----
      LFSR_RC(wgrad(LFSR_IN_CONV3, dOut, 64, 0, f.c2[j], 64, 64, 64, 9, G(bp + "conv.4.weight")));
      LFSR_RC(dgrad3(dOut, t.convT[2], t.d64, nullptr, f.c2[j]));
      LFSR_RC(wgrad(LFSR_IN_CONV3, t.d64, 64, 0, f.c1[j], 64, 64, 64, 9, G(bp + "conv.2.weight")));
      LFSR_RC(dgrad3(t.d64, t.convT[1], t.t64, nullptr, f.c1[j]));
      LFSR_RC(wgrad(LFSR_IN_CONV3, t.t64, 64, 0, f.y[j], 64, 64, 64, 9, G(bp + "conv.0.weight")));
      LFSR_RC(dgrad3(t.t64, t.convT[0], t.d64, nullptr, nullptr));     // d64 = dL/d y
      // ---- BasicTrans (EPIT.py:110-128): y = linear_out(tf), tf = t2 + FFN(LN(t2)), t2 = out_proj(attn) + t, t = linear_in(x) ----
      LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 64, 2>, t.d64, 64, lin[0], t.dsf, 128, nullptr, 0, nullptr, 0, 128));
      LFSR_RC(wgrad_lin(t.d64, 64, 64, f.tf[j], 128, 128, G(e + "linear_out.weight")));
      LFSR_RC(lfsr_layernorm_fwd(f.t2[j], 128, 0, nullptr, 0, 0, 1, P.w(e + "feed_forward.0.weight"), P.w(e + "feed_forward.0.bias"), t.lnt, 128, 0, npix, 128, 1e-5f, stream));
      LFSR_RC(lfsr_linear_fwd(t.lnt, 128, 0, 128, P.w(e + "feed_forward.1.weight"), nullptr, nullptr, 0, 0, t.hid[j], 256, 0, npix, 256, 0.0f, stream));   // ReLU(hidden)
      LFSR_RC(wgrad_lin(t.dsf, 128, 128, t.hid[j], 256, 256, G(e + "feed_forward.4.weight")));
      LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 128, 2>, t.dsf, 128, lin[1], t.dh, 256, nullptr, 0, t.hid[j], 256, 256));
      LFSR_RC(wgrad_lin(t.dh, 256, 256, t.lnt, 128, 128, G(e + "feed_forward.1.weight")));
      LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 256, 2>, t.dh, 256, lin[2], t.dln, 128, nullptr, 0, nullptr, 0, 128));
      LFSR_RC(ln_bwd(f.t2[j], e + "feed_forward.0.weight", e + "feed_forward.0.bias", t.dln, t.dsf, t.dsm));     // dsm = dL/d t2
      LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 128, 2>, t.dsm, 128, lin[3], t.dso, 128, nullptr, 0, nullptr, 0, 128));
      LFSR_RC(wgrad_lin(t.dsm, 128, 128, f.ao[j], 128, 128, G(e + "attention.out_proj.weight")));
      // mask_field = [2A, 11]: the geometry of the forward's launch
      if (!vert) LFSR_RC(lfsr_window_attn_bwd(f.qk[j], 256, 0, 128, f.v[j], 128, 0, f.ao[j], t.dso, 128, 0, t.dqk, t.dv, t.stats, 8, 16, B, A, w, (long long)AA * HW, HW, 1,
                                              A, h, (long long)A * HW, w, A, A, 5, 6, 0, stream));
      else LFSR_RC(lfsr_window_attn_bwd(f.qk[j], 256, 0, 128, f.v[j], 128, 0, f.ao[j], t.dso, 128, 0, t.dqk, t.dv, t.stats, 8, 16, B, A, h, (long long)AA * HW,
                                        (long long)A * HW, w, A, w, HW, 1, A, A, 5, 6, 0, stream));
      // q | k = LN(t) W[0:256]^T, v = t W[256:384]^T
      LFSR_RC(lfsr_layernorm_fwd(f.t[j], 128, 0, nullptr, 0, 0, 1, P.w(e + "norm.weight"), P.w(e + "norm.bias"), t.lnt, 128, 0, npix, 128, 1e-5f, stream));
      float* dWin = G(e + "attention.in_proj_weight");
      LFSR_RC(wgrad_lin(t.dqk, 256, 256, t.lnt, 128, 128, dWin));
      LFSR_RC(wgrad_lin(t.dv, 128, 128, f.t[j], 128, 128, dWin + 256 * 128));
      LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 256, 2>, t.dqk, 256, lin[4], t.dln, 128, nullptr, 0, nullptr, 0, 128));
      LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 128, 2>, t.dv, 128, lin[5], t.dst, 128, t.dsm, 128, nullptr, 0, 128));
      LFSR_RC(ln_bwd(f.t[j], e + "norm.weight", e + "norm.bias", t.dln, t.dst, t.dst));                          // dst = dL/d t
      LFSR_RC(wgrad_lin(t.dst, 128, 128, Xin, 64, 64, G(e + "linear_in.weight")));
      if (vert) {
        LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 128, 2>, t.dst, 128, lin[6], dT1, 64, nullptr, 0, nullptr, 0, 64));      // dL/d t1: mid feeds trans_V only
        LFSR_RC(ew(dX, dT1, nullptr, 1.0f, dX));                                                                             // both shortcuts' share of dL/d x[b]
      } else {
        LFSR_RC(dgemm(launch_gemm<IN_SAME, OUT_SAME, 128, 2>, t.dst, 128, lin[6], dX, 64, dX, 64, nullptr, 0, 64));          // + trans_H's input gradient
      }
    }
    gbase = grads;
    LFSR_RC(lfsr_add_inplace(grads + blk_off, t.gtmp, (long long)blk_n, st));
  }

  // ---- init: buf0 = lrelu(conv_init.4(c2)) + f0, c2 = lrelu(conv_init.2(c1)), c1 = lrelu(conv_init.0(f0)), f0 = conv_init0(x) ------------
  LFSR_RC(ew(t.dbuf0, dX, nullptr, 1.0f, t.dbuf0));
  LFSR_RC(pack3T("conv_init.0.weight", t.initT[0]));
  LFSR_RC(pack3T("conv_init.2.weight", t.initT[1]));
  LFSR_RC(pack3T("conv_init.4.weight", t.initT[2]));
  // conv_init.4's LeakyReLU output without the residual, for its mask (the forward's launch minus r1)
  LFSR_RC(lfsr_conv3x3_fwd(f.c2i, 64, 0, P.w("conv_init.4.weight"), t.r4, 64, 0, nullptr, 0, 0, nullptr, 0, 0, nimg, h, w, L, stream));
  LFSR_RC(ew(t.dbuf0, nullptr, t.r4, L, t.d64));
  LFSR_RC(wgrad(LFSR_IN_CONV3, t.d64, 64, 0, f.c2i, 64, 64, 64, 9, G("conv_init.4.weight")));
  LFSR_RC(dgrad3(t.d64, t.initT[2], t.t64, nullptr, f.c2i));
  LFSR_RC(wgrad(LFSR_IN_CONV3, t.t64, 64, 0, f.c1i, 64, 64, 64, 9, G("conv_init.2.weight")));
  LFSR_RC(dgrad3(t.t64, t.initT[1], t.d64, nullptr, f.c1i));
  LFSR_RC(wgrad(LFSR_IN_CONV3, t.d64, 64, 0, f.f0, 64, 64, 64, 9, G("conv_init.0.weight")));
  LFSR_RC(dgrad3(t.d64, t.initT[0], t.t64, t.dbuf0, nullptr));
  LFSR_RC(lfsr_init_gather9(x, t.xg9, B, A, h, w, st));
  LFSR_RC(wgrad(LFSR_IN_SAME, t.t64, 64, 0, t.xg9, 16, 64, 16, 1, G("conv_init0.0.weight"), 9));
  return LFSR_OK;
}

}  // extern "C"
