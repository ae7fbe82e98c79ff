// The EPIT context and its forward body (shared by the inference forward, epit.cpp, and the training path, epit_train.hip).
#pragma once
#include "param_table.h"

struct lfsr_epit : LfsrModel {
  int nblk = 0;
  std::vector<size_t> ffn_split;      // per block: offset (floats) of the feed-forward weights' pre-split bf16 image in the packed buffer (ffn_b3.hip)
};

// Where the forward body reads and writes.  The inference forward aliases these onto a few buffers (epit.cpp); the training forward gives
// every tensor the backward reads a buffer of its own.  Rows = VCL pixels.  x[b] (64) is the input of AltFilter b (x[0] = buf0, x[nblk] the
// tail's input) and mid[b] (64) the result of its horizontal pass; per pass j = 2 b + vertical: t (128) the tokens (linear_in), qk (256) and
// v (128) the in-projection, ao (128) the attention output, t2 (128) out_proj + tokens (the feed-forward input), tf (128) the feed-forward
// output (the input of linear_out), y (64) the transformer output and c1, c2 (64) the LeakyReLU outputs of conv.0 / conv.2.
// Scratch the backward does not read: tn (128) the LayerNorm output of the unfused in-projection, lnx (128) / hid (256) the LayerNorm output and
// hidden rows of the unfused feed-forward, hr the HR mosaic of the unfused tail.
struct EpitFwdBufs {
  float *f0, *c1i, *c2i, *buf0;
  std::vector<float*> x, mid;                            // nblk + 1, nblk entries
  std::vector<float*> t, qk, v, ao, t2, tf, y, c1, c2;   // 2 nblk entries each
  float *tn, *lnx, *hid, *hr;
};

// epit.cpp: the launches of lfsr_epit_forward on the buffers of `bf` (arguments already checked)
int lfsr_epit_forward_body(const lfsr_epit* c, const float* x, float* out, int B, int h, int w, const EpitFwdBufs& bf, void* stream);
