// The transformer GEMM family as four operators: which kernel runs a dense linear (lfsr_linear_fwd, lfsr_pointwise_fwd), a LayerNorm + projection (lfsr_linear_ln_fwd),
// a feed-forward block (lfsr_ffn_fwd, lfsr_ffn_ln_fwd) and fuse.0's data gradient (lfsr_bwd_gemm).  The kernels and their launchers are rowgemm.hip / ffn_fused.hip (fp32
// MFMA), rowgemm_b3.hip / lnlin_b3.hip / ffn_b3.hip (the exact three-term bf16 split, the product path) and gemm_bf16.hip (LFSR_GEMM_ARITH_BF16).  Host code only.
#include "lfsr_internal.h"

// The chains: a launcher that returns LFSR_E_ARG does not cover the call and the next one runs.  [..]: only with the fp32 form not selected.
//   linear      [ bf16 (the mode set, K != 144) -> b3 ]  (no bias, K in {64, 128, 144})  -> fp32 (LFSR_ROWGEMM=128: wide tiles)  -> the caller's gather-GEMM
//   LN-linear   [ bf16 (the mode set) -> lnlin_b3 (unless LFSR_LNLIN=0) -> b3 ]                                                   -> fp32
//   FFN         [ bf16 (the mode set) -> b3 (the one that reads wsplit) ]                                                         -> fp32
//   dgrad144    [ b3 (mk given, not LFSR_DGRAD_PW=f32) ]                                                                          -> fp32, one 192-column panel
// What the last kernel of the (LN-)linear chain refuses (lfsr_rowgemm_ok / _ln_ok) leaves the family whatever is selected; lnlin_b3 takes only what b3 would (_b3_ln_ok).
LfsrGemmSel lfsr_gemm_sel() {
  const char *rsel = lfsr_sel("LFSR_ROWGEMM"), *fsel = lfsr_sel("LFSR_FFN"), *lsel = lfsr_sel("LFSR_LNLIN"), *dsel = lfsr_sel("LFSR_DGRAD_PW");
  LfsrGemmSel s;
  s.wide = rsel && rsel[0] == '1';                                   // LFSR_ROWGEMM=128
  s.f32 = (rsel && rsel[0] == 'f') || s.wide || lfsr_arith_f32();    // LFSR_ROWGEMM=f32 | 128, lfsr_set_arithmetic(LFSR_ARITH_F32)
  s.ffn_f32 = (fsel && fsel[0] == 'f') || lfsr_arith_f32();          // LFSR_FFN=f32
  s.ffn_chunks = fsel && fsel[0] == 'c';                             // LFSR_FFN=chunks (ffn_b3.hip)
  s.lnlin = !(lsel && lsel[0] == '0');
  s.dgrad_f32 = s.f32 || (dsel && dsel[0] == 'f');                   // LFSR_DGRAD_PW=f32: the fp32-MFMA kernel for this data gradient only (A/B runs)
  s.dgrad_gather = dsel && dsel[0] == 'g';                           // LFSR_DGRAD_PW=gather: the gather-GEMM for it (bwd_ops.hip)
  return s;
}

bool lfsr_rowgemm_enabled() { return !lfsr_sel("LFSR_NO_ROWGEMM"); }

int lfsr_linear_run(const LfsrLin& c, hipStream_t st) {
  if (c.M < LFSR_ROWGEMM_MIN_ROWS || !lfsr_rowgemm_enabled() || !lfsr_rowgemm_ok(c)) return LFSR_E_ARG;
  int rc = LFSR_E_ARG;
  if (!lfsr_gemm_sel().f32 && !c.bias && (c.K == 64 || c.K == 128 || c.K == 144)) {
    if (lfsr_gemm_arith_bf16() && c.K != 144) rc = lfsr_gemm_bf16_launch(c, st);      // K = 144 (DistgSSR's fuse.0) keeps the default
    if (rc == LFSR_E_ARG) rc = lfsr_rowgemm_b3_launch(c, st);
  }
  return rc == LFSR_E_ARG ? lfsr_rowgemm_launch(c, st) : rc;
}

int lfsr_linear_ln_run(const LfsrLin& c, hipStream_t st) {
  LfsrOpTimer op_t("linear_ln", c.K, c.N, st);
  if (!lfsr_rowgemm_ln_ok(c)) return LFSR_E_ARG;
  const LfsrGemmSel sel = lfsr_gemm_sel();
  int rc = LFSR_E_ARG;
  if (!sel.f32) {
    if (lfsr_gemm_arith_bf16()) rc = lfsr_gemm_bf16_ln_launch(c, st);
    if (rc == LFSR_E_ARG && sel.lnlin && lfsr_rowgemm_b3_ln_ok(c)) rc = lfsr_lnlin_b3_launch(c, st);
    if (rc == LFSR_E_ARG) rc = lfsr_rowgemm_b3_ln_launch(c, st);
  }
  return rc == LFSR_E_ARG ? lfsr_rowgemm_ln_launch(c, st) : rc;
}

int lfsr_ffn_run(const LfsrFfn& f, hipStream_t st) {
  LfsrOpTimer op_t("ffn", f.K1, f.H, st);
  if ((f.ln_g != nullptr) != (f.ln_b != nullptr)) return LFSR_E_ARG;      // half a LayerNorm: no kernel's call
  int rc = LFSR_E_ARG;
  if (!lfsr_gemm_sel().ffn_f32) {
    if (lfsr_gemm_arith_bf16()) rc = lfsr_ffn_bf16_launch(f, st);
    if (rc == LFSR_E_ARG) rc = lfsr_ffn_b3_launch(f, st);
  }
  return rc == LFSR_E_ARG ? lfsr_ffn_launch(f, st) : rc;
}

int lfsr_dgrad144_run(const LfsrLin& c, hipStream_t st) {
  const int rc = c.mk && !lfsr_gemm_sel().dgrad_f32 ? lfsr_rowgemm_b3_dgrad_launch(c, st) : LFSR_E_ARG;
  return rc == LFSR_E_ARG ? lfsr_rowgemm_dgrad144_launch(c, st) : rc;
}

extern "C" int lfsr_linear_ln_fwd(const float* x, int x_stride, int x_choff, int K, const float* w_packed, const float* gamma, const float* beta, float eps, int ln_cols,
                                  const float* pe, int pe_stride, int pe_rows, int pe_div, float* y, int y_stride, int y_choff,
                                  float* y2, int y2_stride, int y2_choff, int split_n, long long M, int N, void* stream) {
  LfsrLin c{};
  c.x = x; c.x_stride = x_stride; c.x_choff = x_choff; c.K = K; c.w_packed = w_packed; c.ln_g = gamma; c.ln_b = beta; c.ln_eps = eps; c.ln_cols = ln_cols; c.pe = pe;
  c.pe_stride = pe_stride; c.pe_rows = pe_rows; c.pe_div = pe_div; c.y = y; c.y_stride = y_stride; c.y_choff = y_choff; c.y2 = y2; c.y2_stride = y2_stride;
  c.y2_choff = y2_choff; c.split_n = split_n; c.M = M; c.N = N; c.slope = 1.0f;
  return lfsr_linear_ln_run(c, lfsr_stream(stream));
}

extern "C" int lfsr_ffn_fwd(const float* x, int x_stride, int x_choff, const float* w1_packed, const float* w2_packed, const float* res, int res_stride, int res_choff,
                            float* y, int y_stride, int y_choff, long long M, int K1, int H, int N2, float slope, void* stream) {
  LfsrFfn f{};
  f.x = x; f.x_stride = x_stride; f.x_choff = x_choff; f.w1_packed = w1_packed; f.w2_packed = w2_packed; f.res = res; f.res_stride = res_stride; f.res_choff = res_choff;
  f.y = y; f.y_stride = y_stride; f.y_choff = y_choff; f.M = M; f.K1 = K1; f.H = H; f.N2 = N2; f.slope = slope;
  return lfsr_ffn_run(f, lfsr_stream(stream));
}

extern "C" int lfsr_ffn_ln_fwd(const float* x, int x_stride, int x_choff, const float* gamma, const float* beta, float eps, const float* w1_packed, const float* w2_packed,
                               const float* res, int res_stride, int res_choff, float* y, int y_stride, int y_choff, long long M, int K1, int H, int N2, float slope, void* stream) {
  if (!gamma || !beta) return LFSR_E_ARG;
  LfsrFfn f{};
  f.x = x; f.x_stride = x_stride; f.x_choff = x_choff; f.w1_packed = w1_packed; f.w2_packed = w2_packed; f.res = res; f.res_stride = res_stride; f.res_choff = res_choff;
  f.y = y; f.y_stride = y_stride; f.y_choff = y_choff; f.M = M; f.K1 = K1; f.H = H; f.N2 = N2; f.slope = slope; f.ln_g = gamma; f.ln_b = beta; f.ln_eps = eps;
  return lfsr_ffn_run(f, lfsr_stream(stream));
}
