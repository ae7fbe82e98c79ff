// Host driver for the EPIT forward (get_model.forward, model/SR/EPIT.py:51-71; AltFilter :144-161; BasicTrans :110-128)
// on VCL buffers.  Tokens are VCL pixels; the horizontal / vertical EPI passes differ only in the strides handed to the
// attention kernel, so none of the reference's six `rearrange` copies per AltFilter exists here.
#include "epit_ctx.h"

extern "C" {

int lfsr_epit_create(lfsr_epit** out, int A, int scale, int n_block, int channels) {
  if (!out || A <= 0 || A > 15 || scale < 2 || scale > 4 || n_block <= 0 || channels != 64) return LFSR_E_ARG;
  lfsr_epit* c = new lfsr_epit();
  c->A = A; c->s = scale; c->nblk = n_block;
  LfsrParamTable& P = c->P;
  P.add("conv_init0.0.weight", 64, 1, 9, 0, 0, true);
  for (int i : {0, 2, 4}) P.add("conv_init." + std::to_string(i) + ".weight", 64, 64, 9);
  for (int b = 0; b < n_block; ++b) {
    std::string p = "altblock." + std::to_string(b) + ".";
    std::string e = p + "epi_trans.";
    P.add(e + "linear_in.weight", 128, 64, 1);
    P.add(e + "norm.weight", 128, 1, 1, 0, 0, true);
    P.add(e + "norm.bias", 128, 1, 1, 0, 0, true);
    P.add(e + "attention.in_proj_weight", 384, 128, 1);
    P.add(e + "attention.out_proj.weight", 128, 128, 1);
    P.add(e + "feed_forward.0.weight", 128, 1, 1, 0, 0, true);
    P.add(e + "feed_forward.0.bias", 128, 1, 1, 0, 0, true);
    P.add(e + "feed_forward.1.weight", 256, 128, 1);
    P.add(e + "feed_forward.4.weight", 128, 256, 1);
    P.add(e + "linear_out.weight", 64, 128, 1);
    for (int i : {0, 2, 4}) P.add(p + "conv." + std::to_string(i) + ".weight", 64, 64, 9);
    c->ffn_split.push_back(lfsr_trans_ffn_reserve(P, 128));
  }
  P.add("upsampling.0.weight", 64 * scale * scale, 64, 1, 1, 64);   // PixelShuffle order folded into the packing
  P.add("upsampling.3.weight", 1, 64, 9, 0, 0, true);
  *out = c;
  return LFSR_OK;
}

void lfsr_epit_destroy(lfsr_epit* c) { delete c; }
size_t lfsr_epit_packed_bytes(const lfsr_epit* c) { return c ? c->packed_bytes() : 0; }
int lfsr_epit_set_packed(lfsr_epit* c, void* packed, size_t bytes) { return c ? c->set_packed(packed, bytes) : LFSR_E_ARG; }
int lfsr_epit_load_param(lfsr_epit* c, const char* key, const float* data, size_t numel, void* stream) {
  return c ? c->load_param(key, data, numel, stream) : LFSR_E_ARG;
}
int lfsr_epit_finalize(lfsr_epit* c, void* stream) {
  if (!c || !c->all_loaded()) return LFSR_E_ARG;
  for (int b = 0; b < c->nblk; ++b) LFSR_RC(lfsr_trans_ffn_presplit(c->P, "altblock." + std::to_string(b) + ".epi_trans.", 128, c->ffn_split[b], stream));
  c->finalized = true;
  return LFSR_OK;
}

static void epit_layout(const lfsr_epit* c, int B, int h, int w, LfsrArena& ws, float* buf[14]) {
  const size_t npix = (size_t)B * c->A * c->A * h * w;
  for (int i = 0; i < 8; ++i) buf[i] = ws.take(npix * 64);       // F0, BUF0, P, Q, MID, Y, C1, C2
  for (int i = 8; i < 12; ++i) buf[i] = ws.take(npix * 128);     // T, TN/O, V/FN, T2
  buf[12] = ws.take(npix * 256);                                  // QK / FF
  buf[13] = ws.take(npix * 64 * c->s * c->s);                     // HR mosaic, channel-last
}

size_t lfsr_epit_workspace_bytes(const lfsr_epit* c, int B, int h, int w) {
  if (!c || B <= 0 || h <= 0 || w <= 0) return 0;
  LfsrArena ws;
  float* buf[14];
  epit_layout(c, B, h, w, ws, buf);
  return ws.bytes();
}

int lfsr_epit_forward(lfsr_epit* c, const float* x, float* out, int B, int h, int w, void* workspace, size_t workspace_bytes, void* stream) {
  if (!c || !c->run_args_ok(x, out, B, h, w, workspace)) return LFSR_E_ARG;
  LfsrArena ws(workspace);
  float* buf[14];
  epit_layout(c, B, h, w, ws, buf);
  if (workspace_bytes < ws.bytes()) return LFSR_E_WS;
  const long long npix = (long long)B * c->A * c->A * h * w;
  if (npix * 256 * 4 >= (1LL << 31)) return LFSR_E_ARG;   // every activation tensor < 2 GiB (the q | k rows are the widest): the kernels' 32-bit byte offsets; callers split the batch (capi.py)
  float *F0 = buf[0], *BUF0 = buf[1], *Pb = buf[2], *Qb = buf[3], *MID = buf[4], *Y = buf[5], *C1 = buf[6], *C2 = buf[7];
  float *T = buf[8], *TN = buf[9], *V = buf[10], *T2 = buf[11], *QK = buf[12], *HR = buf[13];
  // the aliasing of the buffers: the blocks ping-pong between Pb and Qb, every pass runs on the same token buffers
  EpitFwdBufs bf;
  bf.f0 = F0; bf.c1i = C1; bf.c2i = C2; bf.buf0 = BUF0; bf.tn = TN; bf.lnx = V; bf.hid = QK; bf.hr = HR;
  bf.x.push_back(BUF0);
  for (int b = 0; b < c->nblk; ++b) {
    bf.mid.push_back(MID);
    bf.x.push_back((bf.x[b] == Pb) ? Qb : Pb);
    for (int vert = 0; vert < 2; ++vert) {
      bf.t.push_back(T); bf.qk.push_back(QK); bf.v.push_back(V); bf.ao.push_back(TN); bf.t2.push_back(T2); bf.tf.push_back(T);
      bf.y.push_back(Y); bf.c1.push_back(C1); bf.c2.push_back(C2);
    }
  }
  return lfsr_epit_forward_body(c, x, out, B, h, w, bf, stream);
}

}  // extern "C"

int lfsr_epit_forward_body(const lfsr_epit* c, const float* x, float* out, int B, int h, int w, const EpitFwdBufs& bf, void* stream) {
  const int A = c->A, AA = A * A, nimg = B * AA, HW = h * w;
  const long long npix = (long long)nimg * HW;
  const LfsrParamTable& P = c->P;
  const LfsrTransSel sel = lfsr_trans_sel();
  const float L = 0.2f;   // LeakyReLU(0.2), EPIT.py:27-31,138-140
  auto conv = [&](const float* in, const std::string& key, float* o, const float* r1, const float* r2, float slope) -> int {
    return lfsr_conv3x3_fwd(in, 64, 0, P.w(key), o, 64, 0, r1, 64, 0, r2, 64, 0, nimg, h, w, slope, stream);
  };
  // BasicTrans.forward (EPIT.py:110-128) over all sequences of one pass
  auto trans = [&](const float* X, const std::string& e, int vertical, int blk) -> int {
    const int j = 2 * blk + vertical;
    float *T = bf.t[j], *QK = bf.qk[j], *V = bf.v[j], *AO = bf.ao[j], *T2 = bf.t2[j], *TF = bf.tf[j];
    LFSR_RC(lfsr_linear_fwd(X, 64, 0, 64, P.w(e + "linear_in.weight"), nullptr, nullptr, 0, 0, T, 128, 0, npix, 128, 1.0f, stream));
    LFSR_RC(lfsr_trans_qkv(sel, P, e, T, 128, nullptr, 1, 1, QK, V, bf.tn, npix, stream));     // q | k from LayerNorm(t), v from t
    LFSR_RC(lfsr_attn_run(LfsrAttn{QK, 256, 0, QK, 256, 128, V, 128, 0, AO, 128, 0, 8, 16, vertical ? lfsr_attn_geom_epit_v(B, A, h, w) : lfsr_attn_geom_epit_h(B, A, h, w)},
                          lfsr_stream(stream)));
    LFSR_RC(lfsr_linear_fwd(AO, 128, 0, 128, P.w(e + "attention.out_proj.weight"), nullptr, T, 128, 0, T2, 128, 0, npix, 128, 1.0f, stream));
    LFSR_RC(lfsr_trans_ffn(sel, P, e, T2, 128, c->ffn_split[blk], TF, bf.lnx, bf.hid, npix, stream));
    return lfsr_linear_fwd(TF, 128, 0, 128, P.w(e + "linear_out.weight"), nullptr, nullptr, 0, 0, bf.y[j], 64, 0, npix, 64, 1.0f, stream);
  };

  LFSR_RC(lfsr_trans_head(P, x, bf.f0, bf.c1i, bf.c2i, bf.buf0, B, A, h, w, stream));       // lrelu(conv) + buffer   (EPIT.py:63)
  for (int b = 0; b < c->nblk; ++b) {
    std::string p = "altblock." + std::to_string(b) + ".";
    const float* cur = bf.x[b];
    const bool last = b == c->nblk - 1;
    for (int vert = 0; vert < 2; ++vert) {
      const int j = 2 * b + vert;
      LFSR_RC(trans(vert ? bf.mid[b] : cur, p + "epi_trans.", vert, b));
      LFSR_RC(conv(bf.y[j], p + "conv.0.weight", bf.c1[j], nullptr, nullptr, L));
      LFSR_RC(conv(bf.c1[j], p + "conv.2.weight", bf.c2[j], nullptr, nullptr, L));
      // + shortcut (the block INPUT both times, EPIT.py:153,159); the network-level skip (:66) rides on the very last conv
      LFSR_RC(conv(bf.c2[j], p + "conv.4.weight", vert ? bf.x[b + 1] : bf.mid[b], cur, (vert && last) ? bf.buf0 : nullptr, 1.0f));
    }
  }
  return lfsr_trans_tail(sel, P, bf.x[c->nblk], x, out, bf.hr, B, A, h, w, c->s, stream);
}
