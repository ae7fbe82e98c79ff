// EPIT training: the forward that keeps what the backward reads, and the backward (autograd of model/SR/EPIT.py:51-71, AltFilter :144-161,
// BasicTrans :110-128, fp32; the graph of oracle/lfsr_torch_port.py::epit_forward is the spec).  Rows are VCL pixels as in the forward (epit.cpp).
//
// forward_train runs lfsr_epit_forward_body, the inference forward's launches, on buffers of its own per (block, pass): every sublayer's
// input.  The fused launches keep no LayerNorm statistics, feed-forward hidden rows or HR map: the backward recomputes those from the saved
// sublayer inputs with the unfused kernels, as LFT's does (lft_train.hip), and shares its kernels (trans_bwd.hip, wgrad.hip, the gather-GEMMs),
// its launch helpers (LfsrTransBwd) and the tail, head and sublayer stages: a BasicTrans is LFT's SpaTrans sublayer without the position embedding.
//
// An AltFilter runs ONE epi_trans and ONE conv stack in both passes: each of its 13 weights gets the sum of two contributions.  The vertical
// pass (the later one in the forward) writes the bucket, the horizontal pass writes a scratch image of the block's span of the bucket, and one
// elementwise add joins them: a fixed order, so buckets are bitwise reproducible.  The block input is added after BOTH passes
// (t1 = conv(trans_H(x)) + x, x' = conv(trans_V(t1)) + x): dx = dx' + dt1 + trans_H's input gradient, dt1 = trans_V's input gradient.
#include <string>
#include <vector>

#include "epit_ctx.h"

namespace {

struct EpitTrainWs : LfsrTransBwdWs {  // the base: the scratch of the stages LFT shares
  EpitFwdBufs f;                      // saved by forward_train (the scratch members point into the backward scratch below)
  // backward scratch of the driver's own
  float *dx[2], *dbuf0, *dsf, *dst, *stats, *gtmp;
  std::vector<float*> hid;            // the feed-forward hidden rows (after the ReLU) the backward rebuilt, per (block, pass): its ReLU decisions
  float* convT[3];                    // one block's conv stack, transposed packs (rebuilt for every block)
  float* lin[7];                      // one block's 1x1 dgrad packs
};

bool train_geometry_ok(const lfsr_epit* c, int B, int h, int w) { return c && lfsr_trans_train_geometry_ok(c->A, c->s, B, h, w); }

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
  t.part_floats = lfsr_trans_wgrad_partial_max(B, c->A, h, w); t.part = ws.take(t.part_floats); t.pln = ws.take((size_t)LFSR_RED_BLOCKS * 256); t.ptail = ws.take((size_t)LFSR_RED_BLOCKS * 9 * 64);
  // the forward body's scratch (unfused LayerNorm outputs, two-launch feed-forward hidden rows, the unfused tail's HR map)
  f.tn = t.lnt; f.lnx = t.dln; f.hid = t.dh; f.hr = t.hr;
  t.up0T = ws.take((size_t)64 * 64 * s2);
  for (int i = 0; i < 3; ++i) t.initT[i] = ws.take(lfsr_tr3_floats());
  for (int i = 0; i < 3; ++i) t.convT[i] = ws.take(lfsr_tr3_floats());
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
  const int A = c->A, nb = c->nblk;
  const LfsrParamTable& P = c->P;
  const EpitFwdBufs& f = t.f;
  hipStream_t st = lfsr_stream(stream);
  LfsrTransBwd k(P, grads, t, B, A, h, w, c->s, st);
  const int npix = k.npix;

  // ---- tail ---------------------------------------------------------------------------------------------------------------------------
  float* dX = t.dx[0];   // the gradient at the altblock output (+ the network skip): dL/d x[nb]
  LFSR_RC(lfsr_trans_tail_bwd(k, dout, f.x[nb], dX));

  // ---- altblock, reversed.  EPIT.py:66 buffer = altblock(buffer) + buffer: dX also reaches buf0 directly ----------------------------------
  LFSR_RC(k.ew(64, dX, nullptr, nullptr, 1.0f, t.dbuf0));
  float* dT1 = t.dx[1];
  for (int b = nb - 1; b >= 0; --b) {
    const std::string bp = "altblock." + std::to_string(b) + ".", e = bp + "epi_trans.";
    float** lin = t.lin;
    // the block's dgrad packs, shared by both passes: linear_out, the sublayer's five, linear_in
    LFSR_RC(k.packT(P.w(e + "linear_out.weight"), 0, 128, 64, lin[0]));
    LFSR_RC(lfsr_trans_sublayer_packs(k, e, 128, lin + 1));
    LFSR_RC(k.packT(P.w(e + "linear_in.weight"), 0, 64, 128, lin[6]));
    for (int i = 0; i < 3; ++i) LFSR_RC(k.pack3T(bp + "conv." + std::to_string(2 * i) + ".weight", t.convT[i]));
    const size_t blk_off = P.grad_off(e + "linear_in.weight"), blk_n = block_grad_floats(c);

    for (int vert = 1; vert >= 0; --vert) {
      const int j = 2 * b + vert;
      const float* Xin = vert ? f.mid[b] : f.x[b];        // the transformer's input
      const float* dOut = vert ? dX : dT1;                // the gradient at conv.4's output (the shortcut takes it to x[b] as it stands)
      k.gbase = vert ? grads : t.gtmp - blk_off;          // the horizontal pass writes the scratch image of the block's span of the bucket
      // ---- conv stack (EPIT.py:136-141): conv.4(lrelu(conv.2(lrelu(conv.0(y))))) ----
      LFSR_RC(k.wgrad(LFSR_IN_CONV3, dOut, 64, 0, f.c2[j], 64, npix, 64, 64, 9, k.G(bp + "conv.4.weight"), 0));
      LFSR_RC(k.dgrad3(dOut, 64, 0, t.convT[2], t.d64, nullptr, f.c2[j]));
      LFSR_RC(k.wgrad(LFSR_IN_CONV3, t.d64, 64, 0, f.c1[j], 64, npix, 64, 64, 9, k.G(bp + "conv.2.weight"), 0));
      LFSR_RC(k.dgrad3(t.d64, 64, 0, t.convT[1], t.t64, nullptr, f.c1[j]));
      LFSR_RC(k.wgrad(LFSR_IN_CONV3, t.t64, 64, 0, f.y[j], 64, npix, 64, 64, 9, k.G(bp + "conv.0.weight"), 0));
      LFSR_RC(k.dgrad3(t.t64, 64, 0, t.convT[0], t.d64, nullptr, nullptr));     // d64 = dL/d y
      // ---- BasicTrans (EPIT.py:110-128): y = linear_out(tf), tf = t2 + FFN(LN(t2)), t2 = out_proj(attn) + t, t = linear_in(x) ----
      LFSR_RC(k.dgemm(t.d64, 64, lin[0], t.dsf, 128, nullptr, 0, nullptr, 0, 128));
      LFSR_RC(k.wgrad_lin(t.d64, 64, 64, f.tf[j], 128, 128, k.G(e + "linear_out.weight")));
      // the geometry of the forward's launch; the kernel is the dispatcher's choice (the matrix pipe up to 160 tokens, else the VALU pair)
      const LfsrAttnBwdCallback attn = [&](const float* qk, const float* v, const float* o, const float* d_o, float* dqk, float* dv) {
        return lfsr_attn_grad_run(LfsrAttnGrad{qk, 256, 0, 128, v, 128, o, d_o, 128, dqk, dv, t.stats, 8, 16,
                                               vert ? lfsr_attn_geom_epit_v(B, A, h, w) : lfsr_attn_geom_epit_h(B, A, h, w)}, st);
      };
      LFSR_RC(lfsr_trans_sublayer_bwd(k, e, 128, t.dsf, f.t2[j], f.ao[j], f.qk[j], f.v[j], f.t[j], nullptr, 1, 1, t.hid[j], lin + 1, attn, t.dst, t.dst,
                                      t.dst));                                                                             // dst = dL/d t
      LFSR_RC(k.wgrad_lin(t.dst, 128, 128, Xin, 64, 64, k.G(e + "linear_in.weight")));
      if (vert) {
        LFSR_RC(k.dgemm(t.dst, 128, lin[6], dT1, 64, nullptr, 0, nullptr, 0, 64));      // dL/d t1: mid feeds trans_V only
        LFSR_RC(k.ew(64, dX, dT1, nullptr, 1.0f, dX));                                 // both shortcuts' share of dL/d x[b]
      } else {
        LFSR_RC(k.dgemm(t.dst, 128, lin[6], dX, 64, dX, 64, nullptr, 0, 64));           // + trans_H's input gradient
      }
    }
    k.gbase = grads;
    LFSR_RC(lfsr_add_inplace(grads + blk_off, t.gtmp, (long long)blk_n, st));
  }

  // ---- init -----------------------------------------------------------------------------------------------------------------------------
  LFSR_RC(k.ew(64, t.dbuf0, dX, nullptr, 1.0f, t.dbuf0));
  return lfsr_trans_head_bwd(k, x, f.f0, f.c1i, f.c2i, t.dbuf0);
}

}  // extern "C"
