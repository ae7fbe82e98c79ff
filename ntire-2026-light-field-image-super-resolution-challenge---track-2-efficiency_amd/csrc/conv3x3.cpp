// The 64 -> 64 3x3 conv as one operator: which of its kernels runs a given call (forward: lfsr_conv3x3_fwd; data gradient: lfsr_conv3x3_bwd_data / _bwd_data_r2).
// The kernels and their launchers are conv3x3_wino4.hip (F(4x4,3x3), the product path), conv3x3_wino.hip (F(2x2,3x3)), conv3x3_halo.hip (direct 9-tap), the
// gather-GEMM of gemm_gather.hip, and conv3x3_bf16.hip / conv3x3_bf16_dgrad.hip (direct 9-tap on bf16 operands: the forward under LFSR_ARITH_BF16, the data gradient
// under LFSR_GRAD_ARITH_BF16).  Host code only.
#include "lfsr_internal.h"

namespace {

// the vocabulary of LFSR_CONV3X3 / LFSR_DGRAD3: halo | gather | wino2 | anything else (wino4, ...) = the default kernel, selected by name
LfsrConv3Sel parse_sel(const char* s) {
  if (!s) return LFSR_C3_DEFAULT;
  if (s[0] == 'h') return LFSR_C3_HALO;
  if (s[0] == 'g') return LFSR_C3_GATHER;
  if (s[0] == 'w' && s[1] == 'i' && s[2] == 'n' && s[3] == 'o' && s[4] == '2') return LFSR_C3_WINO2;
  return LFSR_C3_WINO4;
}

enum Kernel { END = 0, WINO4, WINO2, HALO, GATHER };

// direction x selection -> the kernels to try, in order: a launcher that returns LFSR_E_ARG does not cover the geometry and the next one runs.
//   WINO4   operand spans below 1 GiB            WINO2   spans below 2 GiB, h * w < 2^24            HALO, GATHER   everything the entry points admit
// The tile kernels (all but GATHER) need 16-B aligned channel vectors on y / r1 / r2 / mk (x: checked by the entry points); other operands run on GATHER whatever is
// selected.  Row 2 is lfsr_conv3x3_bwd_data_r2 (both residuals at once): the F(4x4) kernel with nothing selected, else LFSR_E_ARG and the caller adds r2 itself.
// LFSR_DGRAD3=gather has always run the halo kernel on aligned operands (LFSR_CONV3X3=gather: the gather-GEMM); kept as it is.
const Kernel kChain[3][5][2] = {
  //  DEFAULT          WINO4            WINO2            HALO     GATHER
  {{WINO4, HALO}, {WINO4, HALO}, {WINO2, HALO}, {HALO}, {GATHER}},   // forward
  {{WINO4, HALO}, {WINO4, HALO}, {WINO2, HALO}, {HALO}, {HALO}},     // data gradient
  {{WINO4}, {END}, {END}, {END}, {END}},                             // data gradient, two residuals
};

int sel_mask(LfsrConv3Sel s) { return s == LFSR_C3_WINO2 ? LFSR_W_WINO2 : (s == LFSR_C3_HALO || s == LFSR_C3_GATHER) ? 0 : LFSR_W_WINO4; }

bool al4(const float* p, int stride, int choff) { return !p || !((stride | choff) & 3); }

}  // namespace

// read at every call, never cached (lfsr_sel: live only in a lab process)
LfsrConv3Sel lfsr_conv3_fwd_sel() { return parse_sel(lfsr_sel("LFSR_CONV3X3")); }
LfsrConv3Sel lfsr_conv3_dgrad_sel() { const char* d = lfsr_sel("LFSR_DGRAD3"); return parse_sel(d ? d : lfsr_sel("LFSR_CONV3X3")); }

int lfsr_conv3_variant_mask() { return sel_mask(lfsr_conv3_fwd_sel()) | sel_mask(lfsr_conv3_dgrad_sel()); }

int lfsr_conv3x3_run(const LfsrConv3& c, bool dgrad, hipStream_t st) {
  if (!(al4(c.y, c.y_stride, c.y_choff) && al4(c.r1, c.r1_stride, c.r1_choff) && al4(c.r2, c.r2_stride, c.r2_choff) && al4(c.mk, c.mk_stride, c.mk_choff) &&
        al4(c.x, c.x_stride, c.x_choff)))
    return lfsr_conv3x3_gather_launch(c, st);
  const Kernel* chain = kChain[dgrad ? (c.r2 ? 2 : 1) : 0][dgrad ? lfsr_conv3_dgrad_sel() : lfsr_conv3_fwd_sel()];
  int rc = LFSR_E_ARG;
  // lfsr_set_arithmetic(LFSR_ARITH_BF16): a forward call with nothing selected runs on bf16 operands; what that launcher does not cover goes down the chain in fp32
  if (!dgrad && lfsr_arith_bf16() && lfsr_conv3_fwd_sel() == LFSR_C3_DEFAULT) rc = lfsr_conv3x3_bf16_launch(c, st);
  // lfsr_set_grad_arithmetic(LFSR_GRAD_ARITH_BF16): likewise a data gradient (with one or two residuals) with nothing selected
  if (dgrad && lfsr_grad_arith_bf16() && lfsr_conv3_dgrad_sel() == LFSR_C3_DEFAULT) rc = lfsr_conv3x3_bf16_dgrad_launch(c, st);
  for (int i = 0; i < 2 && chain[i] != END && rc == LFSR_E_ARG; ++i)
    rc = chain[i] == WINO4 ? lfsr_conv3x3_wino4_launch(c, st) : chain[i] == WINO2 ? lfsr_conv3x3_wino2_launch(c, st)
       : chain[i] == HALO ? lfsr_conv3x3_halo_launch(c, st) : lfsr_conv3x3_gather_launch(c, st);
  return rc;
}
