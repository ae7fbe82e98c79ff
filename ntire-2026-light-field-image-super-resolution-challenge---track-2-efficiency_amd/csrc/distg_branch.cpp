// DistgSSR's angular and epipolar branches and the fused block tail as operators: which kernel runs lfsr_angconv_fwd, lfsr_epiconv_fwd / _hv_fwd and
// lfsr_distg_branch_tail_fwd, and the same chains for the inference and training drivers (distgssr.cpp).  The kernels and their launchers are ang_fused.hip,
// epi_b3.hip (the exact three-term bf16 split, the product path at angRes 5), epi_fused.hip (fp32 MFMA), distg_tail.hip, distg_bf16.hip (LFSR_BRANCH_ARITH_BF16)
// and gemm_gather.hip (the gather-GEMM pairs).  Host code only.
#include "lfsr_internal.h"

// The chains: a launcher that returns LFSR_E_ARG does not cover the call and the next one runs.  [..]: only at angRes 5 with no fp32 form selected (epi_f32).
//   ang         fused (A <= 5, 16-B y, not LFSR_ANG=gather)                                                                     | the gather pair
//   epi         not LFSR_EPI=gather, A odd and <= 5, h, w <= 32, 16-B outputs, x span below 2 GiB:
//                 [ b3 ] -> fp32: F(2,5) (A = 5) | direct<5> (LFSR_EPI=direct) | direct (A < 5)                                 | the gather pair per pass
//   block tail  ang stage 1 (fused, y = null); EPI stage 1: { bf16 } -> b3 (y = null); tail: { bf16 } -> distg_tail
//               {..}: only under lfsr_set_branch_arithmetic(bf16) without lfsr_set_arithmetic(f32)
// `|` is a choice made before any launch, not a fallback: what the chosen side refuses is the call's answer.  The gather pair of a pass needs its stage-1 buffer.
// The block tail is taken only where lfsr_distg_tail_covers holds: it has no other form, the three operators above are its alternative.
LfsrBranchSel lfsr_branch_sel() {
  const char *esel = lfsr_sel("LFSR_EPI"), *osel = lfsr_sel("LFSR_EPI_ORDER"), *asel = lfsr_sel("LFSR_ANG"), *tsel = lfsr_sel("LFSR_DISTG_TAIL");
  LfsrBranchSel s;
  s.epi_gather = esel && esel[0] == 'g';                             // LFSR_EPI=gather: the two-launch gather-GEMM path (A/B runs)
  s.epi_direct = esel && esel[0] == 'd';                             // LFSR_EPI=direct: stage 1 in direct form at angRes 5 (else Winograd F(2,5))
  s.epi_f32 = s.epi_gather || s.epi_direct || (esel && (esel[0] == 'w' || esel[0] == 'f')) || lfsr_arith_f32();   // LFSR_EPI=wino | direct | f32 | gather
  s.ang_gather = asel && asel[0] == 'g';                             // LFSR_ANG=gather
  s.tail_off = tsel && tsel[0] == '0';                               // LFSR_DISTG_TAIL=0: the drivers keep the three operators (same-process A/B)
  s.order_pass = osel && osel[0] == 'p';                             // LFSR_EPI_ORDER=pass: pass-major blocks in the fp32 two-pass launch
  s.order_item = osel && osel[0] == 'i';                             // LFSR_EPI_ORDER=item: item-major without the XCD swizzle
  return s;
}

int lfsr_ang_run(const LfsrAng& a, hipStream_t st) {
  LfsrOpTimer op_t("angconv", a.B, a.h * a.w, st);
  if (!lfsr_branch_sel().ang_gather && lfsr_ang_fused_ok(a.A) && !((a.y_stride | a.y_choff) & 3)) return lfsr_ang_fused_launch(a, st);
  return lfsr_ang_gather_launch(a, st);
}

int lfsr_epi_run(const LfsrEpi& e, float* scratch, hipStream_t st) {
  LfsrOpTimer op_t(e.which == 3 ? "epiconv_hv" : "epiconv", e.B, e.h * e.w, st);
  const LfsrBranchSel sel = lfsr_branch_sel();
  if (!sel.epi_gather && lfsr_epi_fused_ok(e.A, e.h, e.w) && !((e.y_stride | e.choff_h | e.choff_v) & 3) &&
      (long long)e.B * e.A * e.A * e.h * e.w * e.x_stride * 4 < (1LL << 31)) {      // (16-B output vectors, 32-bit byte offsets into x)
    LfsrOpTimer fused_t("epi_fused", e.B, e.h * e.w, st);
    const int rc = e.A == 5 && !sel.epi_f32 ? lfsr_epi_b3_launch(e, st) : LFSR_E_ARG;
    return rc == LFSR_E_ARG ? lfsr_epi_f32_launch(e, sel, st) : rc;
  }
  LfsrEpi g = e;
  if (!g.t_h) g.t_h = scratch;
  if (!g.t_v) g.t_v = scratch;
  return lfsr_epi_gather_launch(g, st);
}

bool lfsr_distg_tail_covers(const LfsrEpi& e) {
  if (e.A != 5 || e.h <= 0 || e.w <= 0 || e.h > 32 || e.w > 32 || !lfsr_ang_fused_ok(e.A)) return false;
  const LfsrBranchSel sel = lfsr_branch_sel();
  if (sel.epi_f32 || sel.ang_gather || lfsr_gemm_sel().f32 || !lfsr_rowgemm_enabled()) return false;      // fuse.0 would not run the three-term row GEMM
  if ((e.x_stride | e.x_choff) & 3 || e.x_stride < e.x_choff + 64 || (((uintptr_t)e.x | (uintptr_t)e.t_h | (uintptr_t)e.t_v) & 15)) return false;
  return true;
}

int lfsr_distg_ang1_run(const LfsrAng& a, hipStream_t st) { return lfsr_ang_fused_launch(a, st); }

// the bf16 kernels and the default ones are independent: either tail is valid on the other form's t_h / t_v, which are fp32 in memory
int lfsr_distg_epi1_run(const LfsrEpi& e, hipStream_t st) {
  const int rc = lfsr_branch_arith_bf16() && !lfsr_arith_f32() ? lfsr_epi_bf16_launch(e, st) : LFSR_E_ARG;
  return rc == LFSR_E_ARG ? lfsr_epi_b3_launch(e, st) : rc;
}

int lfsr_distg_tail2_run(const LfsrDistgTail& t, hipStream_t st) {
  const int rc = lfsr_branch_arith_bf16() && !lfsr_arith_f32() ? lfsr_distg_tail_bf16_launch(t, st) : LFSR_E_ARG;
  return rc == LFSR_E_ARG ? lfsr_distg_tail_launch(t, st) : rc;
}

int lfsr_distg_block_tail_run(const LfsrAng& a, const LfsrEpi& e, const LfsrDistgTail& t, hipStream_t st) {
  LfsrOpTimer op_t("distg_tail", t.B, t.h * t.w, st);
  int rc = lfsr_distg_ang1_run(a, st);
  if (!rc) rc = lfsr_distg_epi1_run(e, st);
  if (!rc) rc = lfsr_distg_tail2_run(t, st);
  return rc;
}

// ---- the C ABI: argument checks, then the chains above ----
extern "C" int lfsr_angconv_fwd(const float* x, int x_stride, int x_choff, const float* w1_packed, const float* w2_packed,
                                float* tmp, float* y, int y_stride, int y_choff, int B, int A, int h, int w, float slope, void* stream) {
  if (!x || !w1_packed || !w2_packed || !tmp || !y || B <= 0 || A <= 0 || h <= 0 || w <= 0) return LFSR_E_ARG;
  if (x_stride < x_choff + 64 || y_stride < y_choff + 16 || (x_stride | x_choff) & 3) return LFSR_E_ARG;
  return lfsr_ang_run(LfsrAng{x, x_stride, x_choff, w1_packed, w2_packed, tmp, y, y_stride, y_choff, B, A, h, w, slope}, lfsr_stream(stream));
}

// tmp (may be NULL where a fused kernel runs): receives the pass's stage-1 activation, as the gather path leaves it
extern "C" int lfsr_epiconv_fwd(const float* x, int x_stride, int x_choff, const float* w1_packed, const float* w2_packed,
                                float* tmp, float* y, int y_stride, int y_choff, int B, int A, int h, int w, int vertical, float slope, void* stream) {
  if (!x || !w1_packed || !w2_packed || !y || B <= 0 || A <= 0 || h <= 0 || w <= 0) return LFSR_E_ARG;
  if (x_stride < x_choff + 64 || y_stride < y_choff + 32 || (x_stride | x_choff) & 3) return LFSR_E_ARG;
  const LfsrEpi e{x, x_stride, x_choff, w1_packed, w2_packed, y, y_stride, y_choff, y_choff, vertical ? nullptr : tmp, vertical ? tmp : nullptr,
                  B, A, h, w, vertical ? 2 : 1, slope};
  return lfsr_epi_run(e, nullptr, lfsr_stream(stream));
}

// tmp (may be NULL where a fused kernel runs): the gather pairs' scratch, untouched by the fused kernels
extern "C" int lfsr_epiconv_hv_fwd(const float* x, int x_stride, int x_choff, const float* w1_packed, const float* w2_packed,
                                   float* tmp, float* y, int y_stride, int choff_h, int choff_v, int B, int A, int h, int w, float slope, void* stream) {
  if (!x || !w1_packed || !w2_packed || !y || B <= 0 || A <= 0 || h <= 0 || w <= 0) return LFSR_E_ARG;
  if (x_stride < x_choff + 64 || y_stride < choff_h + 32 || y_stride < choff_v + 32 || (x_stride | x_choff) & 3) return LFSR_E_ARG;
  const LfsrEpi e{x, x_stride, x_choff, w1_packed, w2_packed, y, y_stride, choff_h, choff_v, nullptr, nullptr, B, A, h, w, 3, slope};
  return lfsr_epi_run(e, tmp, lfsr_stream(stream));
}

extern "C" int lfsr_distg_branch_tail_fwd(const float* x, int x_stride, int x_choff, const float* spa, int spa_stride, int spa_choff,
                                          const float* w_ang0, const float* w_ang2, const float* w_epi0, const float* w_epi2, const float* w_fuse0,
                                          float* t_a, float* t_h, float* t_v, float* y, int y_stride, int y_choff, int B, int A, int h, int w, float slope,
                                          void* stream) {
  if (!x || !spa || !w_ang0 || !w_ang2 || !w_epi0 || !w_epi2 || !w_fuse0 || !t_a || !t_h || !t_v || !y || B <= 0) return LFSR_E_ARG;
  const LfsrAng a{x, x_stride, x_choff, w_ang0, nullptr, t_a, nullptr, 0, 0, B, A, h, w, slope};
  const LfsrEpi e{x, x_stride, x_choff, w_epi0, nullptr, nullptr, 0, 0, 0, t_h, t_v, B, A, h, w, 3, slope};
  const LfsrDistgTail t{spa, spa_stride, spa_choff, t_a, t_h, t_v, w_ang2, w_epi2, w_fuse0, y, y_stride, y_choff, B, A, h, w, slope};
  if (!lfsr_distg_tail_covers(e)) return LFSR_E_ARG;
  if ((spa_stride | spa_choff | y_stride | y_choff) & 3 || spa_stride < spa_choff + 64 || y_stride < y_choff + 64) return LFSR_E_ARG;
  if (((uintptr_t)spa | (uintptr_t)t_a | (uintptr_t)w_ang2 | (uintptr_t)w_epi0 | (uintptr_t)w_epi2 | (uintptr_t)w_fuse0 | (uintptr_t)y) & 15) return LFSR_E_ARG;
  if (!(slope >= 0.f && slope <= 1.f)) return LFSR_E_ARG;
  const long long npix = (long long)B * A * A * h * w;
  if (npix * x_stride * 4 >= (1LL << 31) || npix * spa_stride * 4 >= (1LL << 31) || npix * y_stride * 4 >= (1LL << 31)) return LFSR_E_ARG;   // 32-bit byte offsets
  return lfsr_distg_block_tail_run(a, e, t, lfsr_stream(stream));
}
