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
// with the HR -> LR un-shuffle and the small fixed-order reductions are the kernels of trans_bwd.hip, which EPIT's backward shares, as it does
// the launch helpers (LfsrTransBwd) and the tail, head and sublayer stages the driver below is written in.  Buckets are bitwise reproducible.
#include <algorithm>
#include <string>
#include <vector>

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
struct LftTrainWs : LfsrTransBwdWs {  // the base: the scratch of the stages EPIT shares
  LftFwdBufs f;                       // saved by forward_train (the scratch members point into the backward scratch below)
  // backward scratch of the driver's own
  float *dx[2], *dbuf0, *dsf, *dln2, *dst, *hid, *dspe;
  std::vector<float*> hid_a, hid_s;   // the feed-forward hidden rows (after the ReLU) the backward rebuilt, per layer: its ReLU decisions
  float4* stats;
  std::vector<float*> mloT, mhiT;     // transposed packs, rebuilt from the current packed weights by every backward
  float* lin[11];                     // one layer's 1x1 dgrad packs (rebuilt for every layer): see the backward
};

bool train_geometry_ok(const lfsr_lft* c, int B, int h, int w) { return c && lfsr_trans_train_geometry_ok(c->A, c->s, B, h, w); }

// the position map's share of MLP.weight (one 64-column half): a 3x3 conv over the h w pixels of ONE view; the GATHER form like the other 3x3 weight gradients of
// EPIT / LFT, not CONV3 -- the Winograd kernel would change bits and speed
LfsrWgrad spe_wgrad(int h, int w) {
  LfsrWgrad g = lfsr_wgrad_gather(LFSR_IN_SAME, LFSR_IN_CONV3, h * w, 64, 64, 9, 1, h, w);
  g.g_stride = 128;
  return g;
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
  // part: the position map's share of MLP.weight runs over the h w pixels of one view; part_floats: what the shared stages use of it
  t.part_floats = lfsr_trans_wgrad_partial_max(B, c->A, h, w);
  t.part = ws.take(std::max(t.part_floats, lfsr_wgrad_part_floats(spe_wgrad(h, w))));
  t.pln = ws.take((size_t)LFSR_RED_BLOCKS * 256); t.ptail = ws.take((size_t)LFSR_RED_BLOCKS * 9 * 64);
  // the forward body's scratch (unfused LayerNorm outputs, two-launch feed-forward hidden rows, the unfused tail's HR map)
  f.n64 = t.t64; f.tn = t.lnt; f.lnf = t.dln2; f.ha = t.dh; f.hs = t.hid; f.hr = t.hr;
  t.up0T = ws.take((size_t)64 * 64 * s2);
  for (int i = 0; i < 3; ++i) t.initT[i] = ws.take(lfsr_tr3_floats());
  t.mloT.clear(); t.mhiT.clear();
  for (int b = 0; b < nl; ++b) { t.mloT.push_back(ws.take(lfsr_tr3_floats())); t.mhiT.push_back(ws.take(lfsr_tr3_floats())); }
  for (float*& l : t.lin) l = ws.take(256 * 128);       // the largest: [128][256]
}

// a sublayer's attention backward on rows of width E (q | k in rows of 2 E, 8 heads of hd floats), with the sequence / window geometry of the forward's
// launch.  The VALU pair directly, not lfsr_attn_grad_run: the dispatcher would hand the spatial geometry to k_epi_attn_bwd_mfma whenever h <= 3
// (every row visible, <= 160 tokens) and change those gradients' bits
LfsrAttnBwdCallback attn_bwd(int E, int hd, float4* stats, hipStream_t st, const LfsrAttnGeom& g) {
  return [=](const float* qk, const float* v, const float* o, const float* d_o, float* dqk, float* dv) {
    return lfsr_attn_bwd_valu_launch(LfsrAttnGrad{qk, 2 * E, 0, E, v, E, o, d_o, E, dqk, dv, reinterpret_cast<float*>(stats), 8, hd, g}, st);
  };
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
  const int A = c->A, AA = A * A, HW = h * w, nl = c->nlayer;
  const LfsrParamTable& P = c->P;
  const LftFwdBufs& f = t.f;
  hipStream_t st = lfsr_stream(stream);
  const LfsrTransBwd k(P, grads, t, B, A, h, w, c->s, st);
  const int nimg = k.nimg, npix = k.npix;

  // ---- tail ---------------------------------------------------------------------------------------------------------------------------
  float* dX = t.dx[0];   // the gradient at the altblock output (+ its skip): dL/d x[nl]
  LFSR_RC(lfsr_trans_tail_bwd(k, dout, f.x[nl], dX));

  // ---- altblock, reversed.  LFT.py:91 buffer = altblock(buffer) + buffer: dX also reaches buf0 directly ----------------------------------
  LFSR_RC(k.ew(64, dX, nullptr, nullptr, 1.0f, t.dbuf0));
  for (int b = nl - 1; b >= 0; --b) {
    const std::string sp = "altblock." + std::to_string(b) + ".spa_trans.", an = "altblock." + std::to_string(b) + ".ang_trans.";
    float** lin = t.lin;
    // the layer's 1x1 dgrad packs: linear.0, then the five of either sublayer
    LFSR_RC(k.packT(P.w(sp + "linear.0.weight"), 0, 128, 64, lin[0]));
    LFSR_RC(lfsr_trans_sublayer_packs(k, sp, 128, lin + 1));
    LFSR_RC(lfsr_trans_sublayer_packs(k, an, 64, lin + 6));
    LFSR_RC(k.pack3T(sp + "MLP.weight#lo", t.mloT[b]));
    LFSR_RC(k.pack3T(sp + "MLP.weight#hi", t.mhiT[b]));

    // ---- SpaTrans (LFT.py:188-203): x[b+1] = linear.0(sf), sf = sm + FFN(LN(sm)), sm = out_proj(attn) + st ----------------------
    LFSR_RC(k.dgemm(dX, 64, lin[0], t.dsf, 128, nullptr, 0, nullptr, 0, 128));
    LFSR_RC(k.wgrad_lin(dX, 64, 64, f.sf[b], 128, 128, k.G(sp + "linear.0.weight")));
    // the forward's window (lfsr_attn_geom_lft_spa).  q | k = LN(st + spe) W[0:256]^T: the LayerNorm's input gradient goes to dln2, dst = the rest of dL/d st
    LFSR_RC(lfsr_trans_sublayer_bwd(k, sp, 128, t.dsf, f.sm[b], f.so[b], f.sqk[b], f.sv[b], f.st[b], f.spe[b], HW, 1, t.hid_s[b], lin + 1,
                                    attn_bwd(128, 16, t.stats, st, lfsr_attn_geom_lft_spa(nimg, h, w)), t.dst, nullptr, t.dln2));
    LFSR_RC(k.ew(128, t.dst, t.dln2, nullptr, 1.0f, t.dst));
    // st = MLP(unfold(ay)), spe = MLP(unfold(spa_position)): MLP.weight also gets the LayerNorm-input gradient summed over the images
    hipLaunchKernelGGL(k_pe_reduce, dim3(lfsr_blocks((long long)HW * 128, 256)), dim3(256), 0, st, t.dln2, t.dspe, nimg, HW);
    LFSR_CHECK_LAUNCH();
    float* dWm = k.G(sp + "MLP.weight");
    for (int half = 0; half < 2; ++half) {
      LFSR_RC(k.wgrad(LFSR_IN_CONV3, t.dst, 128, 64 * half, f.ay[b], 64, npix, 64, 64, 9, dWm + half * 64 * 576, 0));
      LfsrWgrad g = spe_wgrad(h, w);
      g.G = t.dspe; g.g_choff = 64 * half; g.X = f.spos; g.dW = dWm + half * 64 * 576; g.accumulate = 1; g.part = t.part; g.part_floats = lfsr_wgrad_part_floats(g);
      LFSR_RC(lfsr_wgrad_run(g, st));
    }
    LFSR_RC(k.dgrad3(t.dst, 128, 0, t.mloT[b], t.d64, nullptr, nullptr));
    LFSR_RC(k.dgrad3(t.dst, 128, 64, t.mhiT[b], t.t64, t.d64, nullptr));   // t64 = dL/d ay

    // ---- AngTrans (LFT.py:233-246): ay = am + FFN(LN(am)), am = out_proj(attn) + x[b], q | k = LN(x[b] + ape) W[0:128]^T ------------------
    float* dXp = t.dx[(nl - b) & 1];
    LFSR_RC(lfsr_trans_sublayer_bwd(k, an, 64, t.t64, f.am[b], f.ao[b], f.aqk[b], f.av[b], f.x[b], f.ape, AA, HW, t.hid_a[b], lin + 6,
                                    attn_bwd(64, 8, t.stats, st, lfsr_attn_geom_lft_ang(B, A, h, w)), dXp, dXp, dXp));
    dX = dXp;
  }

  // ---- init -----------------------------------------------------------------------------------------------------------------------------
  LFSR_RC(k.ew(64, t.dbuf0, dX, nullptr, 1.0f, t.dbuf0));
  return lfsr_trans_head_bwd(k, x, f.f0, f.c1, f.c2, t.dbuf0);
}

}  // extern "C"
