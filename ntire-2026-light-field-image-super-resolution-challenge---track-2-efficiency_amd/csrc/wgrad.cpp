// The weight gradients as one operator family: which kernel writes the partial slabs of an LfsrWgrad, how many, and the reduce behind it.  Every training driver
// and lfsr_conv3x3_wgrad, lfsr_pointwise_wgrad, lfsr_linear_wgrad, lfsr_conv3x3_wide_wgrad, lfsr_angconv_bwd and lfsr_epiconv_hv_bwd come through here.  The kernels and
// their launchers are wgrad.hip (fp32 MFMA), wgrad_bf16.hip, wgrad_wide_bf16.hip, lin_wgrad_bf16.hip and epi0_grad_bf16.hip (bf16-rounded operands).  Host code only.
#include <algorithm>

#include "lfsr_internal.h"

// The chains: a launcher that returns LFSR_E_ARG does not cover the call and the next one runs.  {..}: only under the named arithmetic.
//   GATHER   the generic split-K gather kernel
//   CONV3    { bf16: lfsr_set_grad_arithmetic, with LFSR_WGRAD3 unset } -> Winograd | halo (LFSR_WGRAD3=direct)
//   PW144    pw144 (not LFSR_WGRAD_PW=gather) -> generic
//   EPI0     G2 set: the EPI lines of both passes, { bf16: lfsr_set_branch_grad_arithmetic } | fp32 (not LFSR_WGRAD_EPI=gather; A = 5, lines <= 32 pixels, x span
//            below 2 GiB); what they decline is the call's answer: the caller submits the passes one by one (G2 = null), which run the generic kernel
//   LINEAR   bf16 (lfsr_set_lin_grad_arithmetic) | the generic kernel on every 64-row slice of the weight, each with its own reduce (lfsr_wgrad_run only)
//   WIDE3    { bf16: lfsr_set_wide_train_arithmetic 1 | 2 } -> generic
// `|` is a choice made before any launch, not a fallback.
LfsrWgradSel lfsr_wgrad_sel() {
  const char *s3 = lfsr_sel("LFSR_WGRAD3"), *se = lfsr_sel("LFSR_WGRAD_EPI"), *sp = lfsr_sel("LFSR_WGRAD_PW");
  LfsrWgradSel s;
  s.conv3_direct = s3 && s3[0] == 'd';                               // LFSR_WGRAD3=direct keeps the direct-form kernel (A/B runs); the Winograd form is the default
  s.conv3_bf16 = lfsr_grad_arith_bf16() && !s3;                      // bf16 operands with nothing selected
  s.epi_gather = se && se[0] == 'g';                                 // LFSR_WGRAD_EPI=gather: the gather form per pass
  s.epi_bf16 = lfsr_branch_grad_arith_bf16();
  s.pw_gather = sp && sp[0] == 'g';                                  // LFSR_WGRAD_PW=gather keeps the generic kernel
  s.lin_bf16 = lfsr_lin_grad_arith_bf16();
  s.wide_bf16 = lfsr_wide_train_arith() != LFSR_WIDE_TRAIN_ARITH_DEFAULT;
  return s;
}

namespace {
// what the form fixes: the GEMM the generic kernel would run (M, N, K, ntaps, the gathers) and dW's shape where the caller left it open
LfsrWgrad shaped(const LfsrWgrad& g0) {
  LfsrWgrad g = g0;
  switch (g.form) {
    case LFSR_WG_CONV3: g.gmode = LFSR_IN_SAME; g.xmode = LFSR_IN_CONV3; g.M = (long long)g.n_img() * g.h * g.w; g.N = 64; g.K = 64; g.ntaps = 9; break;
    case LFSR_WG_WIDE3: g.gmode = LFSR_IN_SAME; g.xmode = LFSR_IN_CONV3; g.M = (long long)g.n_img() * g.h * g.w; g.N = 64; g.ntaps = 9; break;
    case LFSR_WG_PW144: g.gmode = g.xmode = LFSR_IN_SAME; g.N = 64; g.K = 144; g.ntaps = 1; break;
    case LFSR_WG_EPI0: g.gmode = LFSR_IN_SAME; g.M = (long long)g.B * g.A * g.h * g.w; g.N = 32; g.K = 64; g.ntaps = g.A * g.A; break;
    case LFSR_WG_LINEAR: g.gmode = g.xmode = LFSR_IN_SAME; g.ntaps = 1; break;
  }
  if (!g.O) { g.O = g.N; g.C = g.K; g.T = g.ntaps; }
  return g;
}

size_t slab(const LfsrWgrad& g) { return (size_t)g.ntaps * g.N * g.K; }      // of the forms' own kernels (N a multiple of 32 there)

size_t part_floats(const LfsrWgrad& g, bool full) {
  if (g.form == LFSR_WG_CONV3)      // one slab per block, whatever the row count (the Winograd form's 2-row tiles are never fewer than the direct form's)
    return (size_t)std::max(lfsr_wgrad_conv3_blocks(g.n_img(), g.h, g.w, false), lfsr_wgrad_conv3_blocks(g.n_img(), g.h, g.w, true)) * slab(g);
  if (g.M <= 0 || g.M > 0x7fffffffLL || g.N <= 0 || g.K <= 0 || g.ntaps <= 0) return 0;
  const int M = (int)g.M;
  const size_t generic = lfsr_wgrad_partial_floats(M, g.ntaps, g.N, g.K);
  switch (g.form) {
    case LFSR_WG_PW144: return std::max(generic, (size_t)lfsr_wgrad_pw144_blocks(g.M) * slab(g));
    case LFSR_WG_EPI0: return std::max(generic, (size_t)LFSR_WGRAD_MAX_BLOCKS * slab(g));      // the lines' grid at its cap, whatever the geometry: the operators' workspaces hold it
    case LFSR_WG_LINEAR: {
      const int per = lfsr_lin_wgrad_bf16_slabs_per_block(g.N, g.K);
      if (!per || g.M > 0x7fffffffLL - 128) return 0;
      const int blocks = full ? lfsr_lin_wgrad_bf16_blocks(g.M, g.N, g.K, (size_t)-1) : 1;      // (the bf16 form's smallest grid: it sizes itself to what part holds)
      return std::max(lfsr_wgrad_partial_floats(M, 1, 64, g.K), (size_t)blocks * per * slab(g));
    }
    case LFSR_WG_WIDE3: {
      const int blocks = lfsr_wgrad_wide_bf16_blocks(g.K, g.n_img(), g.h, g.w);
      return blocks > 0 ? std::max(generic, (size_t)blocks * slab(g)) : 0;
    }
  }
  return generic;
}
}  // namespace

size_t lfsr_wgrad_part_floats(const LfsrWgrad& g, bool full_grid) { return part_floats(shaped(g), full_grid); }

int lfsr_wgrad_partials(const LfsrWgrad& g0, int* slabs, hipStream_t st) {
  const LfsrWgrad g = shaped(g0);
  const LfsrWgradSel sel = lfsr_wgrad_sel();
  const size_t need = part_floats(g, false);
  *slabs = 0;
  if (!need) return LFSR_E_ARG;
  if (g.part_floats < need) return LFSR_E_WS;
  int rc = LFSR_E_ARG;
  switch (g.form) {
    case LFSR_WG_CONV3: {
      LfsrOpTimer op_t("conv3x3_wgrad", g.n_img(), g.h * g.w, st);
      if (sel.conv3_bf16) rc = lfsr_wgrad_conv3_bf16_launch(g, st);
      if (rc == LFSR_E_ARG) rc = sel.conv3_direct ? lfsr_wgrad_conv3_halo_launch(g, st) : lfsr_wgrad_conv3_wino_launch(g, st);
      *slabs = lfsr_wgrad_conv3_blocks(g.n_img(), g.h, g.w, sel.conv3_direct);
      return rc;
    }
    case LFSR_WG_PW144:
      if (!sel.pw_gather) rc = lfsr_wgrad_pw144_launch(g, st);
      *slabs = lfsr_wgrad_pw144_blocks(g.M);
      break;
    case LFSR_WG_EPI0:
      if (g.G2) {
        if (sel.epi_gather) return LFSR_E_ARG;
        *slabs = lfsr_wgrad_epi0_blocks(g.B, g.A, g.h, g.w);
        return sel.epi_bf16 ? lfsr_wgrad_epi0_bf16_launch(g, st) : lfsr_wgrad_epi0_launch(g, st);
      }
      break;
    case LFSR_WG_LINEAR:      // (the default's slices are not one launch: lfsr_wgrad_run)
      *slabs = lfsr_lin_wgrad_bf16_blocks(g.M, g.N, g.K, g.part_floats) * lfsr_lin_wgrad_bf16_slabs_per_block(g.N, g.K);
      return sel.lin_bf16 ? lfsr_lin_wgrad_bf16_launch(g, st) : LFSR_E_ARG;
    case LFSR_WG_WIDE3:
      if (sel.wide_bf16) rc = lfsr_wgrad_wide_bf16_launch(g, st);
      *slabs = lfsr_wgrad_wide_bf16_blocks(g.K, g.n_img(), g.h, g.w);
      break;
  }
  if (rc != LFSR_E_ARG) return rc;
  *slabs = lfsr_wgrad_splits((int)g.M, g.ntaps, g.K);
  return lfsr_wgrad_gather_launch(g, st);
}

int lfsr_wgrad_sum(const LfsrWgrad& g, int slabs, const float* part2, int slabs2, hipStream_t st) { return lfsr_wgrad_reduce(shaped(g), slabs, part2, slabs2, st); }

// LINEAR without the bf16 mode: the generic kernel on the rows [n0, n0 + 64) of the weight, slice by slice through the same slabs, each with its own reduce
static int linear_slices(const LfsrWgrad& g, hipStream_t st) {
  LfsrWgrad s = shaped(g);
  const size_t need = part_floats(s, false);
  if (!need) return LFSR_E_ARG;
  if (s.part_floats < need) return LFSR_E_WS;
  s.N = s.O = 64;
  for (int n0 = 0; n0 < g.N; n0 += 64) {
    s.g_choff = g.g_choff + n0; s.dW = g.dW + (size_t)n0 * g.K;
    LFSR_RC(lfsr_wgrad_gather_launch(s, st));
    LFSR_RC(lfsr_wgrad_reduce(s, lfsr_wgrad_splits((int)s.M, 1, s.K), nullptr, 0, st));
  }
  return LFSR_OK;
}

int lfsr_wgrad_run(const LfsrWgrad& g, hipStream_t st) {
  if (g.form == LFSR_WG_LINEAR && !lfsr_wgrad_sel().lin_bf16) return linear_slices(g, st);
  int slabs = 0;
  LFSR_RC(lfsr_wgrad_partials(g, &slabs, st));
  return lfsr_wgrad_sum(g, slabs, nullptr, 0, st);
}
