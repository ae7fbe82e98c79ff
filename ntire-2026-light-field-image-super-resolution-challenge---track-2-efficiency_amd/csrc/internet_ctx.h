// The LF_InterNet context (shared by the forward, internet.hip, and the training path, internet_train.hip).
#pragma once
#include "param_table.h"

struct lfsr_internet : LfsrModel {
  int ngroups = 0, nlayers = 0;
  size_t off_wf = 0;
};

// internet.hip: the forward's AngFE and 64-channel slice copy as host launches
int lfsr_internet_angfe(const float* x, const float* w, float* y, int y_stride, int y_choff, int B, int A, int h, int wd, hipStream_t st);
int lfsr_internet_copy64(const float* src, int s_stride, int s_choff, float* dst, int d_stride, int d_choff, long long M, hipStream_t st);
