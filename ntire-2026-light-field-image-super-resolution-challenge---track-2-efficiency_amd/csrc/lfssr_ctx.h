// The LFSSR context (lfssr.cpp: the driver; lfssr_ops.hip: its small operators).  Inference only.
#pragma once
#include "param_table.h"

struct lfsr_lfssr : LfsrModel {
  int nlayers = 0;
  size_t off_split[2] = {0, 0};   // per up-sampling conv: its weight as four contiguous (64, 64, 3, 3) slices, what the packs of its sub-pixel convs are made from
};

// lfssr_ops.hip: rows c * 4 + ij of a raw (256, 64, 3, 3) weight -> out [ij][c][64][9]
int lfsr_lfssr_split4(const float* w_raw, float* out, hipStream_t st);
