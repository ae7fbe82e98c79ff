// The windowed attention as two operators: which kernel runs a forward (lfsr_window_attn_fwd, the EPIT and LFT forwards) and a backward (lfsr_window_attn_bwd, the
// EPIT training driver), and the four sequence / window geometries the models run them on.  The kernels and their launchers are attn_mfma.hip / win_attn_mfma.hip /
// attn_bwd_mfma.hip (the matrix pipe) and transformer.hip / trans_bwd.hip (the VALU).  Host code only.
#include "lfsr_internal.h"

// The chains: a launcher that returns LFSR_E_ARG does not cover the call and the next one runs.  [..]: only with LFSR_ATTN=valu not set; {..}: only with LFSR_ATTN_L1 not set.
//   forward   { [ epi_mfma (hd 16, every angular position visible, <= 160 tokens) -> win_mfma (hd 16, the 5 x 5 window, n2 <= 32) ]
//               -> lds16 (hd 16, heads in pairs, the staged tile fits) -> ang8 (eight heads of 8, full attention over <= 64 tokens) }      -> valu (k_window_attn)
//                  ang8: k_ang_attn_pair at 25 tokens; LFSR_ATTN_ANG=lds | loop: k_window_attn_lds<8, 8> (loop: its plain staging loop), as at every other length; =l1: not covered
//   backward  [ epi_bwd_mfma (hd 16, the coverage of epi_mfma, at least two tokens) ]                                                     -> the VALU pair
// LFSR_ATTN_L1 is a forward selector: the backward does not read it.
LfsrAttnSel lfsr_attn_sel() {
  const char *asel = lfsr_sel("LFSR_ATTN"), *gsel = lfsr_sel("LFSR_ATTN_ANG");
  LfsrAttnSel s;
  s.valu = asel && asel[0] == 'v';                                  // LFSR_ATTN=valu
  s.l1 = lfsr_sel("LFSR_ATTN_L1") != nullptr;
  s.ang_set = gsel != nullptr;
  s.ang_loop = gsel && gsel[0] == 'l' && gsel[1] == 'o';            // LFSR_ATTN_ANG=loop
  s.ang_l1 = gsel && gsel[0] == 'l' && gsel[1] == '1';              // LFSR_ATTN_ANG=l1
  return s;
}

int lfsr_attn_run(const LfsrAttn& a, hipStream_t st) {
  LfsrOpTimer op_t("window_attn", a.hd, a.g.n1 * a.g.n2, st);
  const LfsrAttnSel sel = lfsr_attn_sel();
  int rc = LFSR_E_ARG;
  if (!sel.l1) {
    if (a.hd == 16 && !sel.valu) {
      rc = lfsr_epi_attn_mfma_launch(a, st);
      if (rc == LFSR_E_ARG) rc = lfsr_win_attn_mfma_launch(a, st);
    }
    if (rc == LFSR_E_ARG) rc = lfsr_attn_lds16_launch(a, st);
    if (rc == LFSR_E_ARG) rc = lfsr_attn_ang8_launch(a, st);
  }
  return rc == LFSR_E_ARG ? lfsr_attn_valu_launch(a, st) : rc;
}

int lfsr_attn_grad_run(const LfsrAttnGrad& a, hipStream_t st) {
  LfsrOpTimer op_t("window_attn_bwd", a.hd, a.g.n1 * a.g.n2, st);
  const int rc = a.hd == 16 && !lfsr_attn_sel().valu ? lfsr_epi_attn_bwd_mfma_launch(a, st) : LFSR_E_ARG;
  return rc == LFSR_E_ARG ? lfsr_attn_bwd_valu_launch(a, st) : rc;
}

// ---- the models' geometries (HW = h w pixels per view, AA = A A views; a pixel of the VCL layout is ((b AA + u A + v) h + y) w + x) ----
// LFT's AngTrans (LFT.py:233-246): one sequence per (b, y, x), its tokens the AA views of that pixel, no mask
LfsrAttnGeom lfsr_attn_geom_lft_ang(int B, int A, int h, int w) {
  const int AA = A * A, HW = h * w;
  return LfsrAttnGeom{B, h, w, (long long)AA * HW, w, 1, AA, 1, HW, 0, AA, AA, 0, 1, 0}.normalised();
}
// LFT's SpaTrans (LFT.py:161-203): one sequence per view image, window [i-2, i+3) x [j-2, min(h, j+3)): the column clamp uses h (LFT.py:168)
LfsrAttnGeom lfsr_attn_geom_lft_spa(int nimg, int h, int w) { return LfsrAttnGeom{nimg, 1, 1, (long long)h * w, 0, 0, h, w, w, 1, 2, 3, 2, 3, h}.normalised(); }
// EPIT's BasicTrans, mask_field = [2A, 11] (EPIT.py:147): all angular positions, spatial window [j-5, j+6).  Horizontal: sequence (b, v, x), tokens (u, y); vertical: (b, u, y), (v, x)
LfsrAttnGeom lfsr_attn_geom_epit_h(int B, int A, int h, int w) {
  const int AA = A * A, HW = h * w;
  return LfsrAttnGeom{B, A, w, (long long)AA * HW, HW, 1, A, h, (long long)A * HW, w, A, A, 5, 6, 0}.normalised();
}
LfsrAttnGeom lfsr_attn_geom_epit_v(int B, int A, int h, int w) {
  const int AA = A * A, HW = h * w;
  return LfsrAttnGeom{B, A, h, (long long)AA * HW, (long long)A * HW, w, A, w, HW, 1, A, A, 5, 6, 0}.normalised();
}

// ---- the C ABI: argument checks, then the chains above ----
extern "C" int lfsr_window_attn_fwd(const float* q, int q_stride, int q_choff, const float* k, int k_stride, int k_choff, const float* v, int v_stride, int v_choff,
                                    float* o, int o_stride, int o_choff, int nheads, int hd,
                                    int ns0, int ns1, int ns2, long long bs0, long long bs1, long long bs2,
                                    int n1, int n2, long long st1, long long st2, int l1, int r1, int l2, int r2, int clip2, void* stream) {
  if (!q || !k || !v || !o || nheads <= 0 || (hd != 8 && hd != 16) || ns0 <= 0 || ns1 <= 0 || ns2 <= 0 || n1 <= 0 || n2 <= 0) return LFSR_E_ARG;
  if ((q_stride | q_choff | k_stride | k_choff | v_stride | v_choff | o_stride | o_choff) & 3) return LFSR_E_ARG;
  const LfsrAttn a{q, q_stride, q_choff, k, k_stride, k_choff, v, v_stride, v_choff, o, o_stride, o_choff, nheads, hd,
                   LfsrAttnGeom{ns0, ns1, ns2, bs0, bs1, bs2, n1, n2, st1, st2, l1, r1, l2, r2, clip2}.normalised()};
  return lfsr_attn_run(a, lfsr_stream(stream));
}

extern "C" int lfsr_window_attn_bwd(const float* qk, int qk_stride, int q_choff, int k_choff, const float* v, int v_stride, int v_choff, const float* o,
                                    const float* d_o, int o_stride, int o_choff, float* dqk, float* dv, float* stats, int nheads, int hd,
                                    int ns0, int ns1, int ns2, long long bs0, long long bs1, long long bs2,
                                    int n1, int n2, long long st1, long long st2, int l1, int r1, int l2, int r2, int clip2, void* stream) {
  if (!qk || !v || !o || !d_o || !dqk || !dv || !stats || nheads <= 0 || (hd != 8 && hd != 16) || ns0 <= 0 || ns1 <= 0 || ns2 <= 0 || n1 <= 0 || n2 <= 0) return LFSR_E_ARG;
  if ((qk_stride | q_choff | k_choff | v_stride | v_choff | o_stride | o_choff) & 3) return LFSR_E_ARG;
  const LfsrAttnGeom g = LfsrAttnGeom{ns0, ns1, ns2, bs0, bs1, bs2, n1, n2, st1, st2, l1, r1, l2, r2, clip2}.normalised();
  if (g.nseq() * g.tokens() * nheads > 0x7fffffffLL * 256) return LFSR_E_ARG;
  const LfsrAttnGrad a{qk, qk_stride, q_choff, k_choff, v + v_choff, v_stride, o + o_choff, d_o + o_choff, o_stride, dqk, dv + v_choff, stats, nheads, hd, g};
  return lfsr_attn_grad_run(a, lfsr_stream(stream));
}
