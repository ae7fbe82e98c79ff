// Host driver for the LFT forward (get_model.forward, model/SR/LFT.py:67-98; AngTrans :206-246; SpaTrans :133-203).
// Tokens are VCL pixels: the angular transformer's sequences (25 views at one (y,x)) and the spatial transformer's
// (32x32 positions of one view) are just two stride sets for the same attention kernel; the 5x5 window mask
// (LFT.py:161-174, rebuilt on the CPU per call upstream) is a predicate, so 25 keys per query are visited, not 1024.
#include "lft_ctx.h"

extern "C" {

int lfsr_lft_create(lfsr_lft** out, int A, int scale, int n_layer, int channels) {
  if (!out || A <= 0 || A > 15 || scale < 2 || scale > 4 || n_layer <= 0 || channels != 64) return LFSR_E_ARG;
  lfsr_lft* c = new lfsr_lft();
  c->A = A; c->s = scale; c->nlayer = n_layer;
  LfsrParamTable& P = c->P;
  P.add("conv_init0.0.weight", 64, 1, 9, 0, 0, true);
  for (int i : {0, 2, 4}) P.add("conv_init." + std::to_string(i) + ".weight", 64, 64, 9);
  for (int b = 0; b < n_layer; ++b) {
    std::string sp = "altblock." + std::to_string(b) + ".spa_trans.";
    P.add(sp + "MLP.weight", 128, 64, 9);                       // (128, 576) == (128, 64, 3, 3): unfold order is c*9 + tap
    P.add(sp + "MLP.weight#lo", 64, 64, 9, 0, 0, false, false);   // the same weights as two 64-output 3x3 convs for the halo-tile kernel
    P.add(sp + "MLP.weight#hi", 64, 64, 9, 0, 0, false, false);   // (internal entries: not in the gradient bucket)
    P.add(sp + "norm.weight", 128, 1, 1, 0, 0, true);
    P.add(sp + "norm.bias", 128, 1, 1, 0, 0, true);
    P.add(sp + "attention.in_proj_weight", 384, 128, 1);
    P.add(sp + "attention.out_proj.weight", 128, 128, 1);
    P.add(sp + "feed_forward.0.weight", 128, 1, 1, 0, 0, true);
    P.add(sp + "feed_forward.0.bias", 128, 1, 1, 0, 0, true);
    P.add(sp + "feed_forward.1.weight", 256, 128, 1);
    P.add(sp + "feed_forward.4.weight", 128, 256, 1);
    P.add(sp + "linear.0.weight", 64, 128, 1);
    std::string an = "altblock." + std::to_string(b) + ".ang_trans.";
    P.add(an + "norm.weight", 64, 1, 1, 0, 0, true);
    P.add(an + "norm.bias", 64, 1, 1, 0, 0, true);
    P.add(an + "attention.in_proj_weight", 192, 64, 1);
    P.add(an + "attention.out_proj.weight", 64, 64, 1);
    P.add(an + "feed_forward.0.weight", 64, 1, 1, 0, 0, true);
    P.add(an + "feed_forward.0.bias", 64, 1, 1, 0, 0, true);
    P.add(an + "feed_forward.1.weight", 128, 64, 1);
    P.add(an + "feed_forward.4.weight", 64, 128, 1);
    c->ffn_split_spa.push_back(lfsr_trans_ffn_reserve(P, 128));
    c->ffn_split_ang.push_back(lfsr_trans_ffn_reserve(P, 64));
  }
  P.add("upsampling.0.weight", 64 * scale * scale, 64, 1, 1, 64);
  P.add("upsampling.3.weight", 1, 64, 9, 0, 0, true);
  *out = c;
  return LFSR_OK;
}

void lfsr_lft_destroy(lfsr_lft* c) { delete c; }
size_t lfsr_lft_packed_bytes(const lfsr_lft* c) { return c ? c->packed_bytes() : 0; }
int lfsr_lft_set_packed(lfsr_lft* c, void* packed, size_t bytes) { return c ? c->set_packed(packed, bytes) : LFSR_E_ARG; }
int lfsr_lft_load_param(lfsr_lft* c, const char* key, const float* data, size_t numel, void* stream) {
  if (!c) return LFSR_E_ARG;
  int rc = c->load_param(key, data, numel, stream);
  std::string k(key ? key : "");
  if (!rc && k.size() > 10 && k.compare(k.size() - 10, 10, "MLP.weight") == 0) {
    rc = c->P.load((k + "#lo").c_str(), data, (size_t)64 * 576, stream);
    if (!rc) rc = c->P.load((k + "#hi").c_str(), data + 64 * 576, (size_t)64 * 576, stream);
  }
  return rc;
}
int lfsr_lft_finalize(lfsr_lft* c, void* stream) {
  if (!c || !c->all_loaded()) return LFSR_E_ARG;
  for (int b = 0; b < c->nlayer; ++b) {      // feed-forward weights split once into the fused kernel's bf16 chunk images
    const std::string a = "altblock." + std::to_string(b);
    LFSR_RC(lfsr_trans_ffn_presplit(c->P, a + ".spa_trans.", 128, c->ffn_split_spa[b], stream));
    LFSR_RC(lfsr_trans_ffn_presplit(c->P, a + ".ang_trans.", 64, c->ffn_split_ang[b], stream));
  }
  c->finalized = true;
  return LFSR_OK;
}

static void lft_layout(const lfsr_lft* c, int B, int h, int w, LfsrArena& ws, float* buf[16]) {
  const size_t npix = (size_t)B * c->A * c->A * h * w;
  for (int i = 0; i < 7; ++i) buf[i] = ws.take(npix * 64);          // F0, BUF0, P, Q, C1, C2, N64
  for (int i = 7; i < 11; ++i) buf[i] = ws.take(npix * 128);        // T, TN, V, T2
  buf[11] = ws.take(npix * 256);                                    // QK / FF
  buf[12] = ws.take(npix * 64 * c->s * c->s);                       // HR mosaic
  buf[13] = ws.take((size_t)h * w * 64);                            // spa position map (h*w, 64)
  buf[14] = ws.take((size_t)c->A * c->A * 64);                      // ang PE
  buf[15] = ws.take((size_t)h * w * 128);                           // embedded spa PE (h*w, 128)
}

size_t lfsr_lft_workspace_bytes(const lfsr_lft* c, int B, int h, int w) {
  if (!c || B <= 0 || h <= 0 || w <= 0) return 0;
  LfsrArena ws;
  float* buf[16];
  lft_layout(c, B, h, w, ws, buf);
  return ws.bytes();
}

int lfsr_lft_forward(lfsr_lft* c, const float* x, float* out, int B, int h, int w, void* workspace, size_t workspace_bytes, void* stream) {
  if (!c || !c->run_args_ok(x, out, B, h, w, workspace)) return LFSR_E_ARG;
  LfsrArena ws(workspace);
  float* buf[16];
  lft_layout(c, B, h, w, ws, buf);
  if (workspace_bytes < ws.bytes()) return LFSR_E_WS;
  const long long npix = (long long)B * c->A * c->A * h * w;
  if (npix * 256 * 4 >= (1LL << 31)) return LFSR_E_ARG;   // every activation tensor < 2 GiB (the q | k rows are the widest): the kernels' 32-bit byte offsets; callers split the batch (capi.py)
  float *Pb = buf[2], *Qb = buf[3], *C1 = buf[4], *T = buf[7], *TN = buf[8], *V = buf[9], *QK = buf[11];
  // the ping-pong aliasing of the buffers: every layer's AngTrans writes Pb, its SpaTrans Qb
  LftFwdBufs bf;
  bf.f0 = buf[0]; bf.buf0 = buf[1]; bf.c1 = C1; bf.c2 = buf[5]; bf.spos = buf[13]; bf.ape = buf[14];
  bf.n64 = buf[6]; bf.tn = TN; bf.lnf = V; bf.ha = T; bf.hs = QK; bf.hr = buf[12];
  bf.x.push_back(bf.buf0);
  for (int b = 0; b < c->nlayer; ++b) {
    float* a_out = (bf.x[b] == Pb) ? Qb : Pb;
    bf.aqk.push_back(T); bf.av.push_back(C1); bf.ao.push_back(bf.c2); bf.am.push_back(C1); bf.ay.push_back(a_out);
    bf.st.push_back(T); bf.spe.push_back(buf[15]); bf.sqk.push_back(QK); bf.sv.push_back(V); bf.so.push_back(TN); bf.sm.push_back(buf[10]);
    bf.sf.push_back(T);
    bf.x.push_back((a_out == Pb) ? Qb : Pb);
  }
  return lfsr_lft_forward_body(c, x, out, B, h, w, bf, stream);
}

}  // extern "C"

int lfsr_lft_forward_body(const lfsr_lft* c, const float* x, float* out, int B, int h, int w, const LftFwdBufs& bf, void* stream) {
  const int A = c->A, AA = A * A, nimg = B * AA, HW = h * w;
  const long long npix = (long long)nimg * HW;
  float *N64 = bf.n64, *SPOS = bf.spos, *APE = bf.ape;
  const LfsrParamTable& P = c->P;
  const LfsrTransSel sel = lfsr_trans_sel();
  LFSR_RC(lfsr_trans_head(P, x, bf.f0, bf.c1, bf.c2, bf.buf0, B, A, h, w, stream));   // LFT.py:80-81
  LFSR_RC(lfsr_lft_position_fwd(SPOS, APE, A, h, w, 64, stream));                    // LFT.py:84-85
  for (int b = 0; b < c->nlayer; ++b) {
    const float* cur = bf.x[b];
    float *AQK = bf.aqk[b], *AV = bf.av[b], *AO = bf.ao[b], *AM = bf.am[b], *AY = bf.ay[b], *HA = bf.ha;
    float *ST = bf.st[b], *SPE = bf.spe[b], *SQK = bf.sqk[b], *SV = bf.sv[b], *SO = bf.so[b], *SM = bf.sm[b], *SF = bf.sf[b];
    float *TN = bf.tn, *LNF = bf.lnf, *HS = bf.hs;
    // ---- AngTrans (LFT.py:233-246): tokens = the A*A views at one (y, x); E = 64, 8 heads of 8, no mask -----------
    std::string an = "altblock." + std::to_string(b) + ".ang_trans.";
    LFSR_RC(lfsr_trans_qkv(sel, P, an, cur, 64, APE, AA, HW, AQK, AV, N64, npix, stream));    // q | k from LayerNorm(token + PE), v from the raw token
    LFSR_RC(lfsr_attn_run(LfsrAttn{AQK, 128, 0, AQK, 128, 64, AV, 64, 0, AO, 64, 0, 8, 8, lfsr_attn_geom_lft_ang(B, A, h, w)}, lfsr_stream(stream)));
    LFSR_RC(lfsr_linear_fwd(AO, 64, 0, 64, P.w(an + "attention.out_proj.weight"), nullptr, cur, 64, 0, AM, 64, 0, npix, 64, 1.0f, stream));     // + token
    LFSR_RC(lfsr_trans_ffn(sel, P, an, AM, 64, c->ffn_split_ang[b], AY, N64, HA, npix, stream));
    // ---- SpaTrans (LFT.py:188-203): tokens = the h*w positions of one view; E = 128, 8 heads of 16, 5x5 window --------
    std::string sp = "altblock." + std::to_string(b) + ".spa_trans.";
    LFSR_RC(lfsr_conv3x3_fwd(AY, 64, 0, P.w(sp + "MLP.weight#lo"), ST, 128, 0, nullptr, 0, 0, nullptr, 0, 0, nimg, h, w, 1.0f, stream));   // unfold + MLP (tokens),
    LFSR_RC(lfsr_conv3x3_fwd(AY, 64, 0, P.w(sp + "MLP.weight#hi"), ST, 128, 64, nullptr, 0, 0, nullptr, 0, 0, nimg, h, w, 1.0f, stream));  // as two 64-output convs
    LFSR_RC(lfsr_conv3x3_n_fwd(SPOS, 64, 0, P.w(sp + "MLP.weight"), SPE, 128, 0, 1, h, w, 128, 1.0f, stream));              // same embedding of the PE map
    LFSR_RC(lfsr_trans_qkv(sel, P, sp, ST, 128, SPE, HW, 1, SQK, SV, TN, npix, stream));
    LFSR_RC(lfsr_attn_run(LfsrAttn{SQK, 256, 0, SQK, 256, 128, SV, 128, 0, SO, 128, 0, 8, 16, lfsr_attn_geom_lft_spa(nimg, h, w)}, lfsr_stream(stream)));
    LFSR_RC(lfsr_linear_fwd(SO, 128, 0, 128, P.w(sp + "attention.out_proj.weight"), nullptr, ST, 128, 0, SM, 128, 0, npix, 128, 1.0f, stream));
    LFSR_RC(lfsr_trans_ffn(sel, P, sp, SM, 128, c->ffn_split_spa[b], SF, LNF, HS, npix, stream));
    // Conv3d 1x1x1 128 -> 64 (LFT.py:183-186); the network-level skip (LFT.py:91) rides on the last layer's projection
    const bool last = b == c->nlayer - 1;
    LFSR_RC(lfsr_linear_fwd(SF, 128, 0, 128, P.w(sp + "linear.0.weight"), nullptr, last ? bf.buf0 : nullptr, 64, 0, bf.x[b + 1], 64, 0, npix, 64, 1.0f, stream));
  }
  return lfsr_trans_tail(sel, P, bf.x[c->nlayer], x, out, bf.hr, B, A, h, w, c->s, stream);
}
