// The LFT context and its forward body (shared by the inference forward, lft.cpp, and the training path, lft_train.hip).
#pragma once
#include "param_table.h"

struct lfsr_lft : LfsrModel {
  int nlayer = 0;
  std::vector<size_t> ffn_split_spa, ffn_split_ang;   // per layer: offsets (floats) of the feed-forward weights' pre-split bf16 images (ffn_b3.hip)
};

// Where the forward body reads and writes.  The inference forward aliases these onto a few ping-pong buffers (lft.cpp); the training
// forward gives every tensor the backward reads a buffer of its own.  Per layer b (rows = VCL pixels):
//   x[b] (64) the AltFilter's input (x[0] = buf0), aqk (128) the angular q | k, av (64) v, ao (64) the attention output, am (64)
//   out_proj + token (the feed-forward input), ay (64) the AngTrans output; st (128) the spatial tokens, spe (h*w, 128) the embedded
//   position map, sqk (256), sv (128), so (128), sm (128), sf (128) the feed-forward output (the input of linear.0); x[b + 1] (64).
// Scratch the backward does not read: n64 (64) and tn (128) LayerNorm outputs of the unfused paths, lnf (128) the spatial feed-forward's
// LayerNorm output and ha (128) / hs (256) the hidden rows of the two-launch feed-forward (LFSR_NO_FFN_FUSED), hr the HR mosaic of the
// unfused tail.
struct LftFwdBufs {
  float *f0, *c1, *c2, *buf0, *spos, *ape;
  std::vector<float*> x;                                               // nlayer + 1 entries
  std::vector<float*> aqk, av, ao, am, ay, st, spe, sqk, sv, so, sm, sf;    // nlayer entries each
  float *n64, *tn, *lnf, *ha, *hs, *hr;
};

// lft.cpp: the launches of lfsr_lft_forward on the buffers of `bf` (arguments already checked)
int lfsr_lft_forward_body(const lfsr_lft* c, const float* x, float* out, int B, int h, int w, const LftFwdBufs& bf, void* stream);
