// LFSSR forward (get_model.forward, model/SR/LFSSR.py:30-46; net2x :87-100, net4x :154-176) on VCL buffers: host driver, inference only.
//   conv0 -> n_layer AltFilters -> fup (64 -> 256, PixelShuffle(2), ReLU) -> res (64 -> 1) + iup (1 -> 4, PixelShuffle(2)) of the LR view, once at scale 2 and
//   a second time on the 2h x 2w views at scale 4 (iup2 reads the level-1 result).
// An AltFilter is two launches: the per-view 3x3 conv on the dispatcher with no activation (lfsr_conv3x3_run, slope 1: it follows lfsr_set_arithmetic), then
// lfsr_angconv3x3_fwd, whose prologue applies spaconv's bias and ReLU while it stages its operand.
#include "lfssr_ctx.h"

namespace {

std::string lvl(const char* what, int level) { return std::string("net.") + what + std::to_string(level + 1); }

struct LfssrBufs {
  float *F[2], *F2;      // the AltFilters' ping-pong at level 1; level 2 runs between U[0] and F2
  float *T[2], *U[2];    // per level: the 256-wide result of the up-sampling conv, and the up-sampled features
  float *lo0, *lo;       // iup's operand as per-view planes: the LR views, and the level-1 result
};

void lfssr_layout(const lfsr_lfssr* c, int B, int h, int w, LfsrArena& ws, LfssrBufs& b) {
  const size_t npix = (size_t)B * c->A * c->A * h * w;
  b.F[0] = ws.take(npix * 64); b.F[1] = ws.take(npix * 64);
  b.T[0] = ws.take(npix * 256);
  b.U[0] = ws.take(npix * 4 * 64);
  b.lo0 = ws.take(npix);
  b.F2 = b.T[1] = b.U[1] = b.lo = nullptr;
  if (c->s == 4) {
    b.lo = ws.take(npix * 4);
    b.F2 = ws.take(npix * 4 * 64);
    b.T[1] = ws.take(npix * 4 * 256);
    b.U[1] = ws.take(npix * 16 * 64);
  }
}

// the widest tensor of one forward, in floats per LR pixel: the 256-wide conv result of the last level
int lfssr_widest(int s) { return s == 4 ? 1024 : 256; }

}  // namespace

extern "C" {

int lfsr_lfssr_create(lfsr_lfssr** out, int A, int scale, int n_layer) {
  if (!out || A < 2 || A > 9 || (scale != 2 && scale != 4) || n_layer < 1) return LFSR_E_ARG;
  lfsr_lfssr* c = new lfsr_lfssr();
  c->A = A; c->s = scale; c->nlayers = n_layer;
  LfsrParamTable& P = c->P;
  P.add("net.conv0.weight", 64, 1, 9, 0, 0, true);
  P.add("net.conv0.bias", 64, 1, 1, 0, 0, true);
  for (int level = 0; level < (scale == 4 ? 2 : 1); ++level) {
    for (int i = 0; i < n_layer; ++i) {
      const std::string p = lvl("altblock", level) + "." + std::to_string(i) + ".";
      P.add(p + "spaconv.weight", 64, 64, 9);
      P.add(p + "spaconv.bias", 64, 1, 1, 0, 0, true);
      P.add(p + "angconv.weight", 64, 64, 9);
      P.add(p + "angconv.bias", 64, 1, 1, 0, 0, true);
    }
    const std::string f = lvl("fup", level) + ".0.";
    P.add(f + "weight", 256, 64, 9, 0, 0, true);
    P.add(f + "bias", 256, 1, 1, 0, 0, true);
    P.add(lvl("res", level) + ".weight", 1, 64, 9, 0, 0, true);
    P.add(lvl("res", level) + ".bias", 1, 1, 1, 0, 0, true);
    P.add(lvl("iup", level) + ".0.weight", 4, 1, 9, 0, 0, true);
    P.add(lvl("iup", level) + ".0.bias", 4, 1, 1, 0, 0, true);
    // internal: the four sub-pixel convs of fup as consecutive 64 -> 64 packs, and the de-interleaved weight they are packed from
    for (int ij = 0; ij < 4; ++ij) P.add(f + "weight#" + std::to_string(ij), 64, 64, 9, 0, 0, false, false);
    c->off_split[level] = P.reserve(4 * 64 * 576);
  }
  *out = c;
  return LFSR_OK;
}

void lfsr_lfssr_destroy(lfsr_lfssr* c) { delete c; }
size_t lfsr_lfssr_packed_bytes(const lfsr_lfssr* c) { return c ? c->packed_bytes() : 0; }
int lfsr_lfssr_set_packed(lfsr_lfssr* c, void* packed, size_t bytes) { return c ? c->set_packed(packed, bytes) : LFSR_E_ARG; }

int lfsr_lfssr_load_param(lfsr_lfssr* c, const char* key, const float* data, size_t numel, void* stream) {
  if (!c || !key) return LFSR_E_ARG;
  if (std::string(key).find('#') != std::string::npos) return LFSR_E_ARG;   // the internal entries are no state_dict keys
  LFSR_RC(c->load_param(key, data, numel, stream));
  for (int level = 0; level < (c->s == 4 ? 2 : 1); ++level) {
    const std::string f = lvl("fup", level) + ".0.weight";
    if (f != key) continue;
    LfsrParamTable& P = c->P;
    float* split = P.packed + c->off_split[level];
    LFSR_RC(lfsr_lfssr_split4(P.w(f), split, lfsr_stream(stream)));
    for (int ij = 0; ij < 4; ++ij) {
      LfsrParamTable::Slot& s = P.slots.at(f + "#" + std::to_string(ij));
      LFSR_RC(lfsr_pack_conv_weight(split + (size_t)ij * 64 * 576, P.packed + s.off, 64, 64, 9, 0, 0, stream));
      s.loaded = true;
    }
  }
  return LFSR_OK;
}

int lfsr_lfssr_finalize(lfsr_lfssr* c, void* stream) {
  (void)stream;
  if (!c || !c->all_loaded()) return LFSR_E_ARG;
  c->finalized = true;
  return LFSR_OK;
}

size_t lfsr_lfssr_workspace_bytes(const lfsr_lfssr* c, int B, int h, int w) {
  if (!c || B <= 0 || h <= 0 || w <= 0) return 0;
  LfsrArena ws;
  LfssrBufs b;
  lfssr_layout(c, B, h, w, ws, b);
  return ws.bytes();
}

int lfsr_lfssr_forward(lfsr_lfssr* c, const float* x, float* out, int B, int h, int w, void* workspace, size_t workspace_bytes, void* stream) {
  if (!c || !c->run_args_ok(x, out, B, h, w, workspace)) return LFSR_E_ARG;
  const int A = c->A, nimg = B * A * A;
  if ((long long)nimg * h * w * lfssr_widest(c->s) >= (1LL << 31) / 4) return LFSR_E_ARG;   // every tensor of the forward below 2 GiB
  LfsrArena ws(workspace);
  LfssrBufs b;
  lfssr_layout(c, B, h, w, ws, b);
  if (workspace_bytes < ws.bytes()) return LFSR_E_WS;
  const LfsrParamTable& P = c->P;
  hipStream_t st = lfsr_stream(stream);
  LFSR_RC(lfsr_lfssr_conv0_fwd(x, P.w("net.conv0.weight"), P.w("net.conv0.bias"), b.F[0], 64, 0, B, A, h, w, stream));
  float *cur = b.F[0], *tmp = b.F[1];
  LFSR_RC(lfsr_nchw_to_vcl(x, b.lo0, 1, 0, B, 1, A, h, w, 0, stream));   // the mosaic un-tiled: rows (b, u, v, y, x) of one channel = per-view planes
  const float* lo = b.lo0;
  int H = h, W = w;
  for (int level = 0; level < (c->s == 4 ? 2 : 1); ++level, H *= 2, W *= 2) {
    for (int i = 0; i < c->nlayers; ++i) {
      const std::string p = lvl("altblock", level) + "." + std::to_string(i) + ".";
      LfsrConv3 cv{};
      cv.x = cur; cv.x_stride = 64; cv.w_packed = P.w(p + "spaconv.weight"); cv.y = tmp; cv.y_stride = 64;
      cv.mk_slope = 1.0f; cv.n_img = nimg; cv.h = H; cv.w = W; cv.slope = 1.0f;
      LFSR_RC(lfsr_conv3x3_run(cv, false, st));
      LFSR_RC(lfsr_angconv3x3_fwd(tmp, 64, 0, P.w(p + "angconv.weight"), P.w(p + "angconv.bias"), P.w(p + "spaconv.bias"), cur, 64, 0, B, A, H * W, stream));
    }
    const std::string f = lvl("fup", level) + ".0.";
    LFSR_RC(lfsr_conv3x3_ps2_fwd(cur, 64, 0, P.w(f + "weight#0"), P.w(f + "bias"), b.T[level], b.U[level], 64, 0, nimg, H, W, stream));
    const bool last = level == (c->s == 4 ? 1 : 0);
    LFSR_RC(lfsr_lfssr_tail_fwd(b.U[level], 64, 0, P.w(lvl("res", level) + ".weight"), P.w(lvl("res", level) + ".bias"), lo, P.w(lvl("iup", level) + ".0.weight"),
                                P.w(lvl("iup", level) + ".0.bias"), last ? out : b.lo, B, A, H, W, last ? 1 : 0, stream));
    lo = b.lo;
    cur = b.U[level];
    tmp = b.F2;
  }
  return LFSR_OK;
}

}  // extern "C"
