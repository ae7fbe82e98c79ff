// Internal (non-ABI) entry points shared between the translation units of liblfsr_hip.so.
#pragma once
#include <functional>
#include <string>

#include "lfsr_common.h"

// gather modes (values match gemm_gather_kernel.h)
enum { LFSR_IN_SAME = 0, LFSR_IN_CONV3 = 1, LFSR_IN_ANG = 2, LFSR_IN_EPIH = 3, LFSR_IN_EPIV = 4,
       LFSR_IN_CHK_H = 5, LFSR_IN_CHK_V = 6, LFSR_IN_LINE_H = 7, LFSR_IN_LINE_V = 8 };
enum { LFSR_OUT_SAME = 0, LFSR_OUT_VIEWS = 1, LFSR_OUT_EPIH = 2, LFSR_OUT_EPIV = 3 };

#if defined(__HIPCC__)
// The exact three-term bf16 split of one PAIR of fp32 values (x = x0 + x1 + x2 by truncation), planes in MFMA operand order (element 0 in the low half).
//   p0 = (top 16 bits of a1, top 16 bits of a0), r = a - trunc(a) (exact), p1 likewise from r, p2 from q = r - trunc(r).
// LFSR_SPLIT_DOT2 (default 1): the residuals as ONE v_dot2c_f32_bf16 each on the plane just packed -- r0 = a0 + (-1.0) * p0.lo + 0 * p0.hi, r1 = a1 + 0 * p0.lo
// + (-1.0) * p0.hi: every partial sum is exactly representable, so the instruction's internal order and rounding do not matter (tools/lab/dot2_split.hip: bit-equal
// to the and / sub form on 2^26 random bit patterns over every exponent, denormals included) -- 3.5 VALU per element instead of 5.5.  The builtin (not asm) so that
// the compiler pads the DOT-write -> VALU-read hazard (3 wait states, which inline asm does not get: found as spurious mismatches in the first lab run).
// The selector constants go through an SGPR the compiler cannot see into: given the literal 0x0000BF80 it encodes the INLINE constant -1.0, which the hardware reads
// as the f32 pattern 0xBF800000 for this operand -- the other half (lab: r0 came out as a0 - trunc(a1)).
#ifndef LFSR_SPLIT_DOT2
#define LFSR_SPLIT_DOT2 1
#endif
__device__ __forceinline__ void lfsr_split_pair(float a0, float a1, unsigned& p0, unsigned& p1, unsigned& p2) {
  typedef __bf16 lfsr_bf16x2 __attribute__((ext_vector_type(2)));
  p0 = __builtin_amdgcn_perm(__float_as_uint(a1), __float_as_uint(a0), 0x07060302u);
#if LFSR_SPLIT_DOT2
  unsigned klo, khi;
  asm("s_mov_b32 %0, 0xbf80" : "=s"(klo));
  asm("s_mov_b32 %0, 0xbf800000" : "=s"(khi));
  const float r0 = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(lfsr_bf16x2, p0), __builtin_bit_cast(lfsr_bf16x2, klo), a0, false);
  const float r1 = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(lfsr_bf16x2, p0), __builtin_bit_cast(lfsr_bf16x2, khi), a1, false);
  p1 = __builtin_amdgcn_perm(__float_as_uint(r1), __float_as_uint(r0), 0x07060302u);
  const float q0 = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(lfsr_bf16x2, p1), __builtin_bit_cast(lfsr_bf16x2, klo), r0, false);
  const float q1 = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(lfsr_bf16x2, p1), __builtin_bit_cast(lfsr_bf16x2, khi), r1, false);
#else
  const float r0 = a0 - __uint_as_float(__float_as_uint(a0) & 0xffff0000u), r1 = a1 - __uint_as_float(__float_as_uint(a1) & 0xffff0000u);
  p1 = __builtin_amdgcn_perm(__float_as_uint(r1), __float_as_uint(r0), 0x07060302u);
  const float q0 = r0 - __uint_as_float(__float_as_uint(r0) & 0xffff0000u), q1 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
#endif
  p2 = __builtin_amdgcn_perm(__float_as_uint(q1), __float_as_uint(q0), 0x07060302u);
}
#endif

#ifdef LFSR_CONV_DIAG
// diagnostic builds only (tools/build_diag.sh): buffer that receives the conv kernels' in-kernel s_memtime stamps; its own argument, never an
// operand slot (round 1 passed it as R2, which selected the two-residual kernel variant on a null-based descriptor: DESIGN.md, incident note)
extern float* g_lfsr_diag_buf;
extern "C" int lfsr_diag_set_buffer(float* buf);
#endif

// op_profile.cpp: operator-level timing hook (RAII).  Off (default): one relaxed atomic load.  On (lfsr_op_profile(1)): a hipEvent pair on `st` around
// the scope, aggregated per (op, a, b) by lfsr_op_profile_read.  `op` must be a string literal.
struct LfsrOpTimer {
  LfsrOpTimer(const char* op, int a, int b, hipStream_t st);
  ~LfsrOpTimer();
  LfsrOpTimer(const LfsrOpTimer&) = delete;
  LfsrOpTimer& operator=(const LfsrOpTimer&) = delete;
 private:
  int slot_, gen_;
  hipStream_t st_;
};

// The 64 -> 64 3x3 conv's packed weight: the direct pack [9][64][64] (LFSR_CONV3_DIRECT_FLOATS), then its Winograd-domain copies (LFSR_CONV3_WINO_FLOATS, see
// lfsr_pack_wino): the F(2x2,3x3) pack of conv3x3_wino.hip (LFSR_CONV3_WINO2_FLOATS), then the F(4x4,3x3) pack of conv3x3_wino4.hip.
#define LFSR_CONV3_DIRECT_FLOATS (9 * 64 * 64)
#define LFSR_CONV3_WINO2_FLOATS (16 * 64 * 64)
#define LFSR_CONV3_WINO4_FLOATS (36 * 64 * 64)
#define LFSR_CONV3_WINO_FLOATS (LFSR_CONV3_WINO2_FLOATS + LFSR_CONV3_WINO4_FLOATS)
#define LFSR_CONV3_WINO2_OFF LFSR_CONV3_DIRECT_FLOATS                                  // where the copies begin in a pack: the only place that spells the layout out
#define LFSR_CONV3_WINO4_OFF (LFSR_CONV3_DIRECT_FLOATS + LFSR_CONV3_WINO2_FLOATS)
// One 3x3 conv 64 -> 64 (forward, or a data gradient on the transposed pack): y = lrelu(conv(x), slope) [* (mk > 0 ? 1 : mk_slope)] [+ r1] [+ r2].
// Every kernel launcher of the operator takes this; lfsr_conv3x3_run (conv3x3.cpp) picks the launcher.
struct LfsrConv3 {
  const float* x; int x_stride, x_choff;
  const float* w_packed;                            // base of the whole pack
  float* y; int y_stride, y_choff;
  const float* r1; int r1_stride, r1_choff;         // residuals (may be null)
  const float* r2; int r2_stride, r2_choff;
  const float* mk; int mk_stride, mk_choff; float mk_slope;   // backward: the saved activation behind a LeakyReLU (may be null)
  int n_img, h, w;
  float slope;
  const float* w_direct() const { return w_packed; }
  const float* w_wino2() const { return w_packed + LFSR_CONV3_WINO2_OFF; }
  const float* w_wino4() const { return w_packed + LFSR_CONV3_WINO4_OFF; }
};
// The launchers return LFSR_E_ARG for a geometry they do not cover: the dispatcher then goes on to the next kernel of its chain.
int lfsr_conv3x3_halo_launch(const LfsrConv3& c, hipStream_t st);                                      // conv3x3_halo.hip: direct 9-tap form
int lfsr_conv3x3_halo_tail_launch(const LfsrConv3& c, int tile_begin, int tile_count, hipStream_t st);  // ... its channel-split launch over a tile range only
int lfsr_conv3x3_wino2_launch(const LfsrConv3& c, hipStream_t st);                                     // conv3x3_wino.hip: F(2x2,3x3); operand spans below 2 GiB
int lfsr_conv3x3_wino4_launch(const LfsrConv3& c, hipStream_t st);                                     // conv3x3_wino4.hip: F(4x4,3x3); operand spans below 1 GiB
int lfsr_conv3x3_bf16_launch(const LfsrConv3& c, hipStream_t st);                                      // conv3x3_bf16.hip: direct 9-tap form on bf16 operands, forward only (LFSR_ARITH_BF16)
int lfsr_conv3x3_bf16_dgrad_launch(const LfsrConv3& c, hipStream_t st);                                // conv3x3_bf16_dgrad.hip: ... with the gradient's mask operand (LFSR_GRAD_ARITH_BF16)
int lfsr_conv3x3_gather_launch(const LfsrConv3& c, hipStream_t st);                                    // gemm_gather.hip: gather-GEMM, no alignment demand on y / r1 / r2 / mk
// conv3x3.cpp: which kernel runs.  LFSR_CONV3X3 selects the forward kernel, LFSR_DGRAD3 (same vocabulary) the data-gradient kernel, which otherwise follows
// LFSR_CONV3X3.  The selection is read when weights are packed AND at every launch: set it before loading a model.
enum LfsrConv3Sel { LFSR_C3_DEFAULT = 0, LFSR_C3_WINO4, LFSR_C3_WINO2, LFSR_C3_HALO, LFSR_C3_GATHER };   // DEFAULT: nothing selected (runs as WINO4)
LfsrConv3Sel lfsr_conv3_fwd_sel();
LfsrConv3Sel lfsr_conv3_dgrad_sel();
int lfsr_conv3x3_run(const LfsrConv3& c, bool dgrad, hipStream_t st);
int lfsr_pack_wino(const float* direct_packed, float* out, hipStream_t st);   // every Winograd-domain copy (the operator-level pack)
// ... or only the copies in `mask` (LFSR_W_WINO2 | LFSR_W_WINO4).  The model runtimes repack every weight each
// training step and write only what the selected 3x3 kernels read: lfsr_conv3_variant_mask() (default: wino4).
enum { LFSR_W_WINO2 = 1, LFSR_W_WINO4 = 2, LFSR_W_ALL = 3 };
int lfsr_conv3_variant_mask();          // union of the copies the forward (LFSR_CONV3X3) and the data-gradient (LFSR_DGRAD3) selections read
// Batched repack (training: every weight is repacked every step; one launch per pack KIND with a device-side descriptor table instead of one 4-us
// launch per weight and layout).  kind 0: lfsr_pack_conv_weight's direct pack (perm 0 / 1), 1: lfsr_pack_weight_T (flip = taps reversed), 2: lfsr_pack_weight_chunkT.
struct LfsrPackDesc { const float* src; float* dst; float* dst2; int kind, O, C, T, Npad, perm, ch, flip; };
int lfsr_pack_generic_batch(const LfsrPackDesc* table_dev, int n, hipStream_t st);                    // kinds 0..2 (pack_batch.hip)
int lfsr_pack_conv3_raw_wino4_batch(const LfsrPackDesc* table_dev, int n, hipStream_t st);            // src -> dst (direct) + dst2 (F(4x4) copy); flip = transposed form
int lfsr_pack_epi_wino_batch(const LfsrPackDesc* table_dev, int n, hipStream_t st);                   // src = the direct pack, dst = its F(2,5) copy
int lfsr_pack_conv3_raw_wino4(const float* w_raw, float* direct_out, float* wino4_out, int transposed, hipStream_t st);   // direct + F(4x4) copies in one launch
int lfsr_pack_wino_m(const float* direct_packed, float* out, int mask, hipStream_t st);
int lfsr_pack_conv_weight_m(const float* w, float* packed, int O, int C, int taps, int perm, int ch, int mask, void* stream);
int lfsr_pack_weight_T_m(const float* w, float* out, int O, int C, int T, int flip, int mask, hipStream_t st);
int lfsr_pack_wino4(const float* direct_packed, float* out, hipStream_t st);
// ---- DistgSSR's angular and epipolar branches and the fused block tail: three operand structs, their launchers, one dispatcher (distg_branch.cpp) ----
// The packs of the EPI branch's weights (lfsr_pack_conv_weight).  EPIConv.0 (O = 32, C = 64, taps = 25 = 5 x 5) at angRes 5: the direct pack, its Winograd F(2,5) copy
// (epi_fused.hip), then its three bf16 planes in the order k_epi_b3 stages them (epi_b3.hip).  EPIConv.2 (O = 160, C = 32, taps = 1): the direct pack, then its planes.
// Both plane images are 16-B aligned.  The _OFF names are the only place that spells the layout out.
#define LFSR_EPI0_DIRECT_FLOATS (25 * 32 * 64)
#define LFSR_EPI_WINO_FLOATS (5 * 6 * 32 * 64)
#define LFSR_EPI_B3_W1_FLOATS (25 * 32 * 64 * 3 / 2)
#define LFSR_EPI2_DIRECT_FLOATS (160 * 32)
#define LFSR_EPI_B3_W2_FLOATS (160 * 32 * 3 / 2)
#define LFSR_EPI0_WINO_OFF LFSR_EPI0_DIRECT_FLOATS
#define LFSR_EPI0_PLANES_OFF (LFSR_EPI0_DIRECT_FLOATS + LFSR_EPI_WINO_FLOATS)
#define LFSR_EPI2_PLANES_OFF LFSR_EPI2_DIRECT_FLOATS
int lfsr_pack_epi_wino(const float* w1_direct_packed, float* out, hipStream_t st);
int lfsr_pack_epi_b3(const float* direct_packed, float* out, int kind, hipStream_t st);              // kind 0: EPIConv.0, 1: EPIConv.2
int lfsr_pack_epi_b3_batch(const LfsrPackDesc* table_dev, int n, hipStream_t st);                     // src = the direct pack, dst = its planes, kind as above
// The AngConv branch (DistgSSR.py:84-90): t = lrelu(conv AxA stride A, 64 -> 16) (16 floats per LR pixel, kept for the backward), y = lrelu(1x1 16 -> 16 A A) after
// PixelShuffle(A).  y = null: stage 1 only (w2 unused).
struct LfsrAng {
  const float* x; int x_stride, x_choff;
  const float *w0, *w2;                             // AngConv.0 (perm 0), AngConv.2 (perm 1, ch 16)
  float* t;
  float* y; int y_stride, y_choff;
  int B, A, h, w;
  float slope;
};
// The EPIConv branch (DistgSSR.py:91-97,108), one pass or both: t = lrelu(conv 1 x A A over the lines of a pass, 64 -> 32), y = lrelu(1x1 32 -> 32 A) after the 1-D
// PixelShuffle.  which: 1 = the horizontal pass, 2 = the vertical one, 3 = both; t_h / t_v ((B A h w), 32) receive a pass's stage-1 result, optional for the fused
// kernels; y = null: stage 1 only (w2 unused).  w0 / w2: the bases of the whole packs.
struct LfsrEpi {
  const float* x; int x_stride, x_choff;
  const float *w0, *w2;
  float* y; int y_stride, choff_h, choff_v;
  float *t_h, *t_v;
  int B, A, h, w, which;
  float slope;
  const float* w0_direct() const { return w0; }
  const float* w0_wino() const { return w0 ? w0 + LFSR_EPI0_WINO_OFF : nullptr; }          // (the copies exist at angRes 5 only)
  const float* w0_planes() const { return w0 ? w0 + LFSR_EPI0_PLANES_OFF : nullptr; }
  const float* w2_direct() const { return w2; }
  const float* w2_planes() const { return w2 ? w2 + LFSR_EPI2_PLANES_OFF : nullptr; }
};
// The block tail at angRes 5: the branches' second stages on their stage-1 results t_a / t_h / t_v, the concat with spa (the SpaConv.2 output) and fuse.0 ([64][144])
struct LfsrDistgTail {
  const float* spa; int spa_stride, spa_choff;
  const float *t_a, *t_h, *t_v;
  const float *w_ang2, *w_epi2, *w_fuse0;           // w_epi2: the base of the whole pack
  float* y; int y_stride, y_choff;
  int B, A, h, w;
  float slope;
  const float* w_epi2_direct() const { return w_epi2; }
  const float* w_epi2_planes() const { return w_epi2 ? w_epi2 + LFSR_EPI2_PLANES_OFF : nullptr; }
};
// which kernel runs.  lfsr_branch_sel: LFSR_EPI=wino | direct | f32 | gather, LFSR_EPI_ORDER=pass | item, LFSR_ANG=gather, LFSR_DISTG_TAIL=0 with lfsr_set_arithmetic(f32)
// folded in, parsed at every call, never cached; the only reader of their characters.  epi_f32: an fp32-MFMA form of the EPI branch (any value above, or the arithmetic)
struct LfsrBranchSel { bool epi_gather, epi_direct, epi_f32, ang_gather, tail_off, order_pass, order_item; };
LfsrBranchSel lfsr_branch_sel();
// A launcher launches its own kernel(s) only; LFSR_E_ARG = the call is not covered and nothing was launched or written: the dispatcher goes down its chain.
bool lfsr_ang_fused_ok(int A);
bool lfsr_epi_fused_ok(int A, int h, int w);
int lfsr_ang_fused_launch(const LfsrAng& a, hipStream_t st);                              // ang_fused.hip: the branch in one launch, A <= 5
int lfsr_ang_gather_launch(const LfsrAng& a, hipStream_t st);                             // gemm_gather.hip: the gather-GEMM pair, every A; needs y
int lfsr_epi_b3_launch(const LfsrEpi& e, hipStream_t st);                                 // epi_b3.hip: the exact three-term bf16 split, A = 5; y = null with which = 3
int lfsr_epi_f32_launch(const LfsrEpi& e, const LfsrBranchSel& sel, hipStream_t st);      // epi_fused.hip, fp32 MFMA: F(2,5) (A = 5) | direct<5> (sel.epi_direct) | direct (A < 5); needs y
int lfsr_epi_gather_launch(const LfsrEpi& e, hipStream_t st);                             // gemm_gather.hip: the gather-GEMM pair per pass, every A; needs y and the passes' t
int lfsr_epi_bf16_launch(const LfsrEpi& e, hipStream_t st);                               // distg_bf16.hip, bf16 operands (LFSR_BRANCH_ARITH_BF16): stage 1 of both passes only
int lfsr_distg_tail_launch(const LfsrDistgTail& t, hipStream_t st);                       // distg_tail.hip: reads EPIConv.2's planes
int lfsr_distg_tail_bf16_launch(const LfsrDistgTail& t, hipStream_t st);                  // distg_bf16.hip: reads EPIConv.2's direct pack
// distg_branch.cpp: what lfsr_angconv_fwd, lfsr_epiconv_fwd / _hv_fwd and lfsr_distg_branch_tail_fwd run behind their argument checks, and what the DistgSSR drivers
// call; op timers "angconv", "epiconv" (one pass) / "epiconv_hv" (both), "epi_fused" (around any fused EPI launch) and "distg_tail".
int lfsr_ang_run(const LfsrAng& a, hipStream_t st);
int lfsr_epi_run(const LfsrEpi& e, float* scratch, hipStream_t st);     // scratch ((B A h w), 32; may be null): the gather pair's stage 1 for a pass without t_h / t_v
// The fused tail covers a block when the default arithmetic runs the three kernels it replaces in their three-term bf16 / fp32-MFMA forms at angRes 5 (no lab
// selector moves one of them) and the stage-1 kernels take e's geometry and operands; e.x may be null (not yet known)
bool lfsr_distg_tail_covers(const LfsrEpi& e);
// ... and its three launches, one by one (the inference driver brackets each with its profiling events) and together: the angular stage 1, the EPI stage 1 and the
// tail, the last two on bf16 operands under lfsr_set_branch_arithmetic unless LFSR_ARITH_F32 is set, where those kernels cover the call
int lfsr_distg_ang1_run(const LfsrAng& a, hipStream_t st);
int lfsr_distg_epi1_run(const LfsrEpi& e, hipStream_t st);
int lfsr_distg_tail2_run(const LfsrDistgTail& t, hipStream_t st);
int lfsr_distg_block_tail_run(const LfsrAng& a, const LfsrEpi& e, const LfsrDistgTail& t, hipStream_t st);
// ang3x3_bf16.hip: lfsr_angconv3x3_fwd's kernel on bf16 operands (lfsr_set_ang_arithmetic(LFSR_ANG_ARITH_BF16)); the caller has checked the operands
int lfsr_ang3x3_bf16_launch(const float* x, int x_stride, int x_choff, const float* w_packed, const float* bias, const float* in_bias, float* y, int y_stride,
                            int y_choff, int B, int A, int npix, hipStream_t st);
// internet.hip: lfsr_conv3x3_wide_fwd behind its argument checks -- y = lrelu(conv3x3(x), slope) (+ r1), cin in {128, 320} -> 64, as lfsr_set_wide_arithmetic selects
// it at this launch: the gather-GEMM launch_gemm<IN_CONV3, OUT_SAME, cin, 2> (AA: what lfsr_internet_forward passes as GemmArgs.A * A, 1 from the operator), or
// conv3x3_wide_bf16.hip's kernel under LFSR_WIDE_ARITH_BF16 unless LFSR_ARITH_F32 is set
int lfsr_conv3x3_wide_run(const float* x, int x_stride, int x_choff, int cin, const float* w_packed, float* y, int y_stride, int y_choff, const float* r1,
                          int r1_stride, int r1_choff, int n_img, int h, int w, float slope, int A, hipStream_t st);
int lfsr_conv3x3_wide_bf16_launch(const float* x, int x_stride, int x_choff, int cin, const float* w_packed, float* y, int y_stride, int y_choff,
                                  const float* r1, int r1_stride, int r1_choff, int n_img, int h, int w, float slope, hipStream_t st);
// bwd_ops.hip: one entry for every backward gather-GEMM (dgrad) instantiation
struct LfsrGemm {
  int in_mode, out_mode, cin;
  const float* X; int x_stride, x_choff;
  const float* Wp;
  float* Y; int y_stride, y_choff;
  const float* R1; int r1_stride, r1_choff;        // added after the mask (may alias Y: in-place accumulate)
  const float* Mk; int mk_stride, mk_choff; float mk_slope;
  int M, N, A, h, w, ntaps, CH;
};
int lfsr_bwd_gemm(const LfsrGemm& g, hipStream_t st);
int lfsr_conv3x3_bwd_data_r2(const float* dy, int dy_stride, const float* wT_packed, float* dx, const float* r1, const float* r2, int n_img, int h, int w, hipStream_t st);
int lfsr_conv3x3_bwd_data(const float* dy, int dy_stride, int dy_choff, const float* wT_packed, float* dx, int dx_stride, int dx_choff,
                          const float* r1, int r1_stride, int r1_choff, const float* mk, int mk_stride, int mk_choff, float mk_slope,
                          int n_img, int h, int w, hipStream_t st);
int lfsr_head_bwd_data(const float* dout, const float* wf, float* df, float* g16, int B, int A, int h, int w, int s, hipStream_t st);
int lfsr_colsum(const float* g, int M, int N, float* partial, int* nblk_out, hipStream_t st);
int lfsr_head_fold_bwd(const float* dWf, const float* colsum_partial, int nblk, const float* w0, const float* b0, const float* w2,
                       float* dw0, float* db0, float* dw2, int s, hipStream_t st);
int lfsr_init_gather9(const float* x, float* xg, int B, int A, int h, int w, hipStream_t st);
int lfsr_add_inplace(float* a, const float* b, long long n, hipStream_t st);   // a += b
int lfsr_pack_weight_chunkT(const float* w, float* out, int O, int C, int ch, int perm, hipStream_t st);
// internet_train.hip: dgrad pack from a forward pack Wp[T][Npad_in][C]: out[t'][k'][n] = Wp[flip ? T-1-t' : t'][n][k0 + k'] (n < O, k' < Kc)
int lfsr_pack_T_from_fwd(const float* Wp, float* out, int T, int Npad_in, int C, int O, int k0, int Kc, int flip, hipStream_t st);

// One dense linear of the row-streaming GEMM family in every form it has: y = act(x W^T (+ bias), slope) (+ res), K -> N over M rows; optional fields null / 0 when absent.
// mk: the data gradient of a 1x1 conv, y = (x W) * (mk > 0 ? 1 : mk_slope).  ln_g / ln_b: the weight rows n < ln_cols see LayerNorm(x (+ pe)) (pe row of token m:
// (m / pe_div) % pe_rows), the others x itself.  y2: the columns n >= split_n go to y2 (column n - split_n).
struct LfsrLin {
  const float* x; int x_stride, x_choff;
  const float *w_packed, *bias;
  float* y; int y_stride, y_choff;
  const float* res; int res_stride, res_choff;
  const float* mk; int mk_stride, mk_choff; float mk_slope;
  const float *ln_g, *ln_b, *pe; float ln_eps; int ln_cols, pe_stride, pe_rows, pe_div;
  float* y2; int y2_stride, y2_choff, split_n;
  long long M; int K, N; float slope;
};
// One feed-forward block: y = res + W2 act(W1 LayerNorm(x), slope), K1 -> H -> N2 (ln_g / ln_b null: x is already normalised); wsplit: lfsr_ffn_b3_presplit's image, optional
struct LfsrFfn {
  const float* x; int x_stride, x_choff;
  const float *ln_g, *ln_b, *w1_packed, *w2_packed; float ln_eps; const void* wsplit;
  const float* res; int res_stride, res_choff;
  float* y; int y_stride, y_choff;
  long long M; int K1, H, N2; float slope;
};
// A launcher launches its own kernel only; LFSR_E_ARG = the call is not covered and nothing was written: the dispatcher (rowgemm.cpp) goes down its chain.
using LfsrLinFn = int(const LfsrLin& c, hipStream_t st);
using LfsrFfnFn = int(const LfsrFfn& f, hipStream_t st);
LfsrLinFn lfsr_rowgemm_launch, lfsr_rowgemm_ln_launch, lfsr_rowgemm_dgrad144_launch;            // rowgemm.hip, fp32 MFMA: the linear, its LN form, the 64 -> 144 data gradient
LfsrLinFn lfsr_rowgemm_b3_launch, lfsr_rowgemm_b3_ln_launch, lfsr_rowgemm_b3_dgrad_launch, lfsr_lnlin_b3_launch;   // rowgemm_b3.hip, the exact three-term bf16 split: the same three; lnlin_b3.hip: its LN form with the weights in registers
LfsrLinFn lfsr_gemm_bf16_launch, lfsr_gemm_bf16_ln_launch;                                      // gemm_bf16.hip, bf16 operands (LFSR_GEMM_ARITH_BF16)
LfsrFfnFn lfsr_ffn_launch, lfsr_ffn_b3_launch, lfsr_ffn_bf16_launch;                            // ffn_fused.hip (fp32 MFMA), ffn_b3.hip (the one that reads wsplit), gemm_bf16.hip
bool lfsr_rowgemm_ok(const LfsrLin& c), lfsr_rowgemm_ln_ok(const LfsrLin& c), lfsr_rowgemm_b3_ln_ok(const LfsrLin& c);   // the operands lfsr_rowgemm_launch / _ln_launch / _b3_ln_launch take
// rowgemm.cpp: which kernel runs.  lfsr_gemm_sel: the family's lab selectors (LFSR_ROWGEMM, LFSR_FFN, LFSR_LNLIN, LFSR_DGRAD_PW) with lfsr_set_arithmetic(f32) folded
// in, parsed at every call, never cached; the only reader of their characters.  f32 / ffn_f32 / dgrad_f32: the fp32-MFMA kernels; wide: LFSR_ROWGEMM=128
struct LfsrGemmSel { bool f32, wide, ffn_f32, ffn_chunks, lnlin, dgrad_f32, dgrad_gather; };
LfsrGemmSel lfsr_gemm_sel();
#define LFSR_ROWGEMM_MIN_ROWS 2048      // a linear over fewer rows leaves the family (lfsr_linear_run); what a caller needs to know to tell which kernel its linear runs
bool lfsr_rowgemm_enabled();            // LFSR_NO_ROWGEMM not set (A/B runs: every plain linear on its caller's gather-GEMM)
LfsrLinFn lfsr_linear_run, lfsr_linear_ln_run, lfsr_dgrad144_run; LfsrFfnFn lfsr_ffn_run;   // lfsr_linear_run's LFSR_E_ARG: no row-streaming kernel covers the call, the caller runs its gather-GEMM
size_t lfsr_ffn_b3_presplit_bytes(int K1, int H, int N2);
int lfsr_ffn_b3_presplit(const float* w1_packed, const float* w2_packed, int K1, int H, int N2, void* out, hipStream_t st);

// attn.cpp: the windowed attention.  The sequence / window geometry, the parametrisation documented at lfsr_window_attn_fwd (include/lfsr_hip.h): sequence (s0,s1,s2) starts
// at pixel s0 bs0 + s1 bs1 + s2 bs2, token (t1,t2) sits at + t1 st1 + t2 st2 and attends keys [t1-l1, t1+r1) x [t2-l2, min(t2+r2, clip2, n2)).
struct LfsrAttnGeom {
  int ns0, ns1, ns2; long long bs0, bs1, bs2;
  int n1, n2; long long st1, st2;
  int l1, r1, l2, r2, clip2;         // every launcher takes a normalised() geometry: clip2 is never 0 (the C ABI's "no clip beyond n2")
  long long nseq() const { return (long long)ns0 * ns1 * ns2; }
  long long tokens() const { return (long long)n1 * n2; }
  LfsrAttnGeom normalised() const { LfsrAttnGeom g = *this; g.clip2 = clip2 > 0 ? clip2 : n2; return g; }
};
// the four geometries the models run, a forward and its backward from the same constructor: LFT's AngTrans and SpaTrans, EPIT's horizontal and vertical pass
LfsrAttnGeom lfsr_attn_geom_lft_ang(int B, int A, int h, int w), lfsr_attn_geom_lft_spa(int nimg, int h, int w), lfsr_attn_geom_epit_h(int B, int A, int h, int w),
    lfsr_attn_geom_epit_v(int B, int A, int h, int w);
// One windowed attention o = softmax(q k^T / sqrt(hd) + window mask) v over nheads heads of hd floats; strides and channel offsets in floats, multiples of 4
struct LfsrAttn {
  const float* q; int q_stride, q_choff; const float* k; int k_stride, k_choff;
  const float* v; int v_stride, v_choff; float* o; int o_stride, o_choff;
  int nheads, hd; LfsrAttnGeom g;
};
// ... and its backward: q | k in one buffer (dqk in its layout); O and dO share a row stride; v / o / d_o / dv point at their first channel (dv in v's layout).
// stats: 4 floats per (pixel, head) of the span the sequences cover, the VALU pair's scratch
struct LfsrAttnGrad {
  const float* qk; int qk_stride, q_choff, k_choff; const float* v; int v_stride;
  const float *o, *d_o; int o_stride; float *dqk, *dv, *stats;
  int nheads, hd; LfsrAttnGeom g;
};
// A launcher launches its own kernel(s) only; LFSR_E_ARG = the call is not covered and nothing was launched or written: the dispatcher goes down its chain.
using LfsrAttnFn = int(const LfsrAttn& a, hipStream_t st);
using LfsrAttnGradFn = int(const LfsrAttnGrad& a, hipStream_t st);
LfsrAttnFn lfsr_epi_attn_mfma_launch, lfsr_win_attn_mfma_launch;   // attn_mfma.hip, win_attn_mfma.hip: EPI attention (<= 160 tokens) and LFT's 5 x 5 window on the matrix pipe, heads of 16
LfsrAttnFn lfsr_attn_lds16_launch, lfsr_attn_ang8_launch, lfsr_attn_valu_launch;   // transformer.hip: k_window_attn_lds<16, 2>; k_ang_attn_pair | k_window_attn_lds<8, 8>; k_window_attn (every geometry)
LfsrAttnGradFn lfsr_epi_attn_bwd_mfma_launch, lfsr_attn_bwd_valu_launch;   // attn_bwd_mfma.hip (reads no stats); trans_bwd.hip: the gather pair, one thread per (query, head) and per (key, head), every geometry
// which kernel runs.  lfsr_attn_sel: LFSR_ATTN=valu, LFSR_ATTN_L1, LFSR_ATTN_ANG=lds | loop | l1 (ang_set: any value), parsed at every call, never cached; the only reader of their characters
struct LfsrAttnSel { bool valu, l1, ang_set, ang_loop, ang_l1; };
LfsrAttnSel lfsr_attn_sel();
LfsrAttnFn lfsr_attn_run; LfsrAttnGradFn lfsr_attn_grad_run;   // what lfsr_window_attn_fwd / _bwd run behind their argument checks; op timers "window_attn" / "window_attn_bwd"
// trans_bwd.hip: what the backward drivers of LFT and EPIT share.  LFSR_RED_BLOCKS: the fixed grid of the kernels that write per-block partials (a fixed order for every geometry)
#define LFSR_RED_BLOCKS 1024
// d = (a (+ b)) * (mk > 0 ? 1 : slope) over C columns (C % 4 == 0); b, mk optional; a and d may alias
int lfsr_ew_launch(const float* a, int as, const float* b, int bs, const float* mk, int ms, float slope, float* d, int ds, int C, long long M, hipStream_t st);
// LayerNorm backward of y = LN(x + pe) gamma + beta on dense rows of C in {64, 128}: dx = ... (+ r; r may alias dx), dgamma, dbeta; part: LFSR_RED_BLOCKS * 2 C floats
int lfsr_ln_bwd_launch(int C, const float* x, const float* pe, long long pe_rows, long long pe_div, const float* gamma, const float* dy, const float* r,
                       float* dx, float* part, long long M, float* dgamma, float* dbeta, hipStream_t st);
// the up-sampling tail's LeakyReLU / 3x3 conv 64 -> 1 backward: du = the un-shuffled gradient of upsampling.0's output, dw3; part: LFSR_RED_BLOCKS * 576 floats
int lfsr_tail_bwd_launch(const float* dout, const float* w3, const float* hr, float* du, float* part, float* dw3, int B, int A, int h, int w, int S, float slope,
                         hipStream_t st);
int lfsr_pack_up0_T_launch(const float* Wp, float* out, int s2, hipStream_t st);   // dgrad pack of upsampling.0 from its forward (perm 1) pack

int lfsr_ang0_dgrad_launch(const float* dA16, const float* w_direct, float* dx, int dx_stride, int dx_choff, int B, int A, int h, int w, hipStream_t st);
int lfsr_epi0_dgrad_launch(const float* dE, const float* w_direct, float* dx, int dx_stride, int dx_choff, int B, int A, int h, int w, int vert, hipStream_t st);
// epi0_grad_bf16.hip: lfsr_epi0_dgrad_launch's kernel on bf16-rounded operands (LFSR_BRANCH_GRAD_ARITH_BF16), A = 5, behind that launcher's coverage checks and selector
int lfsr_epi0_dgrad_bf16_launch(const float* dE, const float* w_direct, float* dx, int dx_stride, int dx_choff, int B, int h, int w, int vert, hipStream_t st);
// lin_dgrad_bf16.hip: lfsr_linear_dgrad's kernel on bf16-rounded operands behind the default's argument checks; LFSR_E_ARG = not covered, the default kernel runs
int lfsr_lin_dgrad_bf16_launch(const float* dy, int cout, const float* wT_packed, float* dx, int dx_stride, const float* r1, int r1_stride, const float* act,
                               int act_stride, long long M, int cin, hipStream_t st);
// ---- the weight gradients: one operand struct, its launchers, one dispatcher (wgrad.cpp) ----
// One weight gradient dW[t][n][k] = sum_m G[src_g(m, t)][n] X[src_x(m, t)][k] in two steps: a kernel writes partial slabs [ntaps][pad32(N)][K] into `part`, then
// lfsr_wgrad_reduce sums them in a fixed order and scatters to the PyTorch layout.  form: the operator the caller means; the dispatcher derives what it fixes.
//   GATHER   gmode / xmode (LFSR_IN_*), M rows, N <= 64 columns of G, K of X, ntaps; A, h, w: the gathers' geometry
//   CONV3    the 64 -> 64 3x3 conv over B A A images of h x w                      PW144   fuse.0's shape, 64 x 144 over M rows
//   EPI0     EPIConv.0 (32 x 64 x A A) over the EPI lines: G / G2 = the horizontal / vertical pass's gradient, both in one launch; G2 = null: the one pass xmode names
//   LINEAR   a dense (N, K) linear over M rows, N in {64, 128, 256, 576, 1024}, K in {64, 128, 256}; part_floats also sizes the bf16 form's grid
//   WIDE3    LF_InterNet's wide 3x3 conv, K in {128, 320} -> 64, over B A A images
// Where the result lands: dW as (O, C, T) (0: N, K, ntaps), perm / ch / chunk_mode as lfsr_pack_conv_weight's inverse (chunk_mode = 1: the T 'taps' are the chunks of a
// pixel shuffle: row = perm ? n T + t : t ch + n (n < ch), dW (T ch, C)); c_valid < C: only the first c_valid input channels, with row length c_valid (init_conv's 9 taps)
enum { LFSR_WG_GATHER = 0, LFSR_WG_CONV3, LFSR_WG_PW144, LFSR_WG_EPI0, LFSR_WG_LINEAR, LFSR_WG_WIDE3 };
#define LFSR_WGRAD_MAX_BLOCKS 256      // the persistent weight-gradient kernels run at most this many blocks, one slab each
struct LfsrWgrad {
  int form, gmode, xmode;
  const float* G; int g_stride, g_choff;
  const float* G2;
  const float* X; int x_stride, x_choff;
  long long M; int N, K, ntaps;
  int B, A, h, w;
  float* dW; int O, C, T, perm, ch, c_valid, chunk_mode, accumulate;
  float* part; size_t part_floats;
  int n_img() const { return B * A * A; }
};
// The launchers: each launches its own kernel only and fills all the slabs its count function names; LFSR_E_ARG = the call is not covered, nothing was launched.
// They read the operand as the dispatcher has shaped it (M, N, K, ntaps filled for every form).
int lfsr_wgrad_splits(int M, int ntaps, int K);
size_t lfsr_wgrad_partial_floats(int M, int ntaps, int N, int K);
int lfsr_wgrad_gather_launch(const LfsrWgrad& g, hipStream_t st);                    // wgrad.hip: the generic split-K gather kernel; lfsr_wgrad_splits slabs
int lfsr_wgrad_conv3_blocks(int n_img, int h, int w, bool direct);                   // one slab [9][64][64] per block of ...
int lfsr_wgrad_conv3_wino_launch(const LfsrWgrad& g, hipStream_t st);                // ... the Winograd form (2-row tiles), spans below 2 GiB
int lfsr_wgrad_conv3_halo_launch(const LfsrWgrad& g, hipStream_t st);                // ... the direct form (direct = true: 4-row tiles)
int lfsr_wgrad_conv3_bf16_launch(const LfsrWgrad& g, hipStream_t st);                // wgrad_bf16.hip: bf16-rounded operands, the Winograd form's block count
int lfsr_wgrad_pw144_blocks(long long M);
int lfsr_wgrad_pw144_launch(const LfsrWgrad& g, hipStream_t st);                     // wgrad.hip: streaming, one slab [64][144] per block
int lfsr_wgrad_epi0_blocks(int B, int A, int h, int w);                              // one per line of both passes: one slab set for the shared weights
int lfsr_wgrad_epi0_launch(const LfsrWgrad& g, hipStream_t st);                      // wgrad.hip: both passes' EPI lines (A = 5, lines of <= 32 pixels), one slab [25][32][64] per block
int lfsr_wgrad_epi0_bf16_launch(const LfsrWgrad& g, hipStream_t st);                 // epi0_grad_bf16.hip: the same lines, slabs and block count on bf16-rounded operands
// lin_wgrad_bf16.hip: `blocks` blocks along x, each writing _slabs_per_block slabs [N][K]; _blocks: one per row tile up to 256 blocks in all, and no more than
// cap_floats holds (0: not one)
int lfsr_lin_wgrad_bf16_slabs_per_block(int cout, int cin);                          // 0: shape not covered
int lfsr_lin_wgrad_bf16_blocks(long long M, int cout, int cin, size_t cap_floats);
int lfsr_lin_wgrad_bf16_launch(const LfsrWgrad& g, hipStream_t st);                  // the grid lfsr_lin_wgrad_bf16_blocks(.., g.part_floats) names
int lfsr_wgrad_wide_bf16_blocks(int cin, int n_img, int h, int w);                   // one per 4 x 32 tile up to 256 / ceil(cin / 128) (0: cin not covered); slabs [9][64][cin]
int lfsr_wgrad_wide_bf16_launch(const LfsrWgrad& g, hipStream_t st);                 // wgrad_wide_bf16.hip: spans below 2 GiB
int lfsr_wgrad_reduce(const LfsrWgrad& g, int slabs, const float* part2, int slabs2, hipStream_t st);   // wgrad.hip: g.part's slabs, then part2's (same geometry; may be null)
// wgrad.cpp: which kernel runs (the table stands there).  lfsr_wgrad_sel: LFSR_WGRAD3, LFSR_WGRAD_EPI, LFSR_WGRAD_PW with the four gradient arithmetics folded in, parsed
// at every call, never cached; the only reader of their characters
struct LfsrWgradSel { bool conv3_direct, conv3_bf16, epi_gather, epi_bf16, pw_gather, lin_bf16, wide_bf16; };
LfsrWgradSel lfsr_wgrad_sel();
int lfsr_wgrad_partials(const LfsrWgrad& g, int* slabs, hipStream_t st);             // one kernel of the form's chain; *slabs: how many slabs it wrote
int lfsr_wgrad_sum(const LfsrWgrad& g, int slabs, const float* part2, int slabs2, hipStream_t st);   // the reduce of one or two slab sets (two passes that share weights)
int lfsr_wgrad_run(const LfsrWgrad& g, hipStream_t st);                              // both; LFSR_E_WS: part_floats below lfsr_wgrad_part_floats
// the most any kernel of the chain needs, in any mode; 0: not covered.  LINEAR: at least, and with full_grid what lets its bf16 form run its whole grid (an operator's workspace)
size_t lfsr_wgrad_part_floats(const LfsrWgrad& g, bool full_grid = false);
// the GATHER form on dense operands (g_stride = N, x_stride = K), pointers apart: what the sites fill in and the sizing loops submit as it is
inline LfsrWgrad lfsr_wgrad_gather(int gmode, int xmode, long long M, int N, int K, int ntaps, int A, int h, int w) {
  LfsrWgrad g{};
  g.form = LFSR_WG_GATHER; g.gmode = gmode; g.xmode = xmode; g.g_stride = N; g.x_stride = K; g.M = M; g.N = N; g.K = K; g.ntaps = ntaps; g.A = A; g.h = h; g.w = w;
  return g;
}
int lfsr_pack_weight_T(const float* w, float* out, int O, int C, int T, int flip, hipStream_t st);

// branch_bwd.cpp: backward of the angular / epipolar branches (DistgSSR.py:84-97,108) on packed weights; C-ABI wrappers lfsr_angconv_bwd / lfsr_epiconv_hv_bwd
size_t lfsr_branch_bwd_partial_floats(int B, int A, int h, int w);
int lfsr_ang_branch_bwd(const float* dcat, int dc_stride, int dc_choff, const float* xin, const float* a16, const float* w0_packed, const float* w0T_packed,
                        const float* w2T_packed, float* dx, float* dw0, float* dw2, float* dA16, float* P, int B, int A, int h, int w, float slope, hipStream_t st);
int lfsr_epi_branch_bwd(const float* dcat, int dc_stride, int choff_h, int choff_v, const float* xin, const float* eh, const float* ev,
                        const float* w0_packed, const float* w0T_packed, const float* w2T_packed, float* dx, float* dw0, float* dw2,
                        float* dEh, float* dEv, float* const P[4], int B, int A, int h, int w, float slope, hipStream_t st);
// ... the same in parts, for callers that run independent parts on two streams (lfsr_distgssr_backward): p1 = everything but the read-modify-write of dx
int lfsr_ang_branch_bwd_p1(const float* dcat, int dc_stride, int dc_choff, const float* xin, const float* a16, const float* w2T_packed, float* dw0, float* dw2,
                           float* dA16, float* P, int B, int A, int h, int w, float slope, hipStream_t st);
int lfsr_ang_branch_bwd_p2(const float* dA16, const float* w0_packed, const float* w0T_packed, float* dx, int B, int A, int h, int w, hipStream_t st);
int lfsr_epi_branch_bwd_p1(const float* dcat, int dc_stride, int choff_h, int choff_v, const float* eh, const float* ev, const float* w2T_packed, float* dw2,
                           float* dEh, float* dEv, float* const P[4], int B, int A, int h, int w, float slope, hipStream_t st);
int lfsr_epi_branch_bwd_p2d(const float* dEh, const float* dEv, const float* w0_packed, const float* w0T_packed, float* dx, int B, int A, int h, int w, hipStream_t st);
int lfsr_epi_branch_bwd_p2w(const float* dEh, const float* dEv, const float* xin, float* dw0, float* const P[4], int B, int A, int h, int w, hipStream_t st);

// transformer.hip: what the EPIT and LFT forwards share, on their packed tables (param_table.h; `pre` = the key prefix of a sublayer)
struct LfsrParamTable;
// the lab selectors of those forwards (LFSR_LN_FUSE, LFSR_ROWGEMM, LFSR_NO_FFN_FUSED, LFSR_FFN_PRESPLIT, LFSR_NO_UPTAIL), read once per forward
struct LfsrTransSel {
  bool ln_fuse;       // LayerNorms formed inside the consuming kernel
  bool ln_fuse_qkv;   // ... the attention norm too, inside the q | k | v projection
  bool ffn_fused;     // the one-launch feed-forward (else two linears through HBM)
  bool presplit;      // the fused feed-forward reads the weights' pre-split image
  bool up_tail;       // the fused up-sampling tail at scales 2 and 4
};
LfsrTransSel lfsr_trans_sel();
// conv_init0 and the conv_init stack: buf0 = lrelu(conv_init.4(c2)) + f0
int lfsr_trans_head(const LfsrParamTable& P, const float* x, float* f0, float* c1, float* c2, float* buf0, int B, int A, int h, int w, void* stream);
// q | k = LayerNorm(x + pe) W[0:2E]^T, v = x W[2E:3E]^T (norm.*, attention.in_proj_weight): one launch, else LayerNorm into tn and two linears
int lfsr_trans_qkv(const LfsrTransSel& sel, const LfsrParamTable& P, const std::string& pre, const float* x, int E, const float* pe, long long pe_rows,
                   long long pe_div, float* qk, float* v, float* tn, long long M, void* stream);
// y = x + FFN(LayerNorm(x)), E -> 2E -> E (feed_forward.*): LayerNorm inside the fused feed-forward, else LayerNorm into lnx and the fused
// feed-forward, else two linears through hid; split_off = the pre-split image of the weights (lfsr_trans_ffn_reserve / _presplit)
int lfsr_trans_ffn(const LfsrTransSel& sel, const LfsrParamTable& P, const std::string& pre, const float* x, int E, size_t split_off, float* y, float* lnx,
                   float* hid, long long M, void* stream);
size_t lfsr_trans_ffn_reserve(LfsrParamTable& P, int E);
int lfsr_trans_ffn_presplit(const LfsrParamTable& P, const std::string& pre, int E, size_t split_off, void* stream);
// upsampling.0 / .3 and the bicubic skip: the fused tail at scales 2 and 4, else the HR map in hr and the two-kernel tail
int lfsr_trans_tail(const LfsrTransSel& sel, const LfsrParamTable& P, const float* f, const float* x, float* out, float* hr, int B, int A, int h, int w, int s,
                    void* stream);

// trans_bwd.hip: what the EPIT and LFT backwards share above the kernels, the mirror of the four forward stages above.
inline size_t lfsr_tr3_floats() { return lfsr_packed_weight_tr_floats(64, 64, 9); }   // the 64 -> 64 3x3 data gradient's pack
// geometry the training paths cover: every activation below 2 GiB (the widest rows: the 256-float q | k, and the HR map of 64 s^2 floats per LR pixel)
bool lfsr_trans_train_geometry_ok(int A, int s, int B, int h, int w);
size_t lfsr_trans_wgrad_partial_max(int B, int A, int h, int w);   // the most lfsr_wgrad_part_floats asks for over the weight gradients the shared stages submit (at any scale)
// the scratch of the shared stages (rows = VCL pixels): the tail's hr / du (64 s^2), ptail and up0T; the head's r4 / d64 / t64 (64), xg9 (16) and
// initT; a sublayer's lnt / dln / dsm / dso / dv (128), dh / dqk (256); part / pln: the weight gradients' and the LayerNorm backward's partials
struct LfsrTransBwdWs {
  float *hr, *du, *ptail, *up0T, *r4, *d64, *t64, *xg9, *initT[3], *lnt, *dh, *dln, *dsm, *dso, *dqk, *dv, *part, *pln;
  size_t part_floats;   // what part holds
};
// One backward's context and the launches its driver and the stages below are written in.
struct LfsrTransBwd {
  static constexpr float L = 0.2f;   // every LeakyReLU of both models
  const LfsrParamTable& P;
  float* gbase;                      // where G() points: the gradient bucket (EPIT's horizontal pass redirects it)
  const LfsrTransBwdWs& ws;
  int B, A, h, w, S, nimg, npix;
  hipStream_t st;
  LfsrTransBwd(const LfsrParamTable& P_, float* grads, const LfsrTransBwdWs& ws_, int B_, int A_, int h_, int w_, int S_, hipStream_t st_)
      : P(P_), gbase(grads), ws(ws_), B(B_), A(A_), h(h_), w(w_), S(S_), nimg(B_ * A_ * A_), npix(B_ * A_ * A_ * h_ * w_), st(st_) {}
  float* G(const std::string& k) const;
  // 1x1 data gradient Y (N columns) = X (dense rows of cin in {64, 128, 256, 576, 1024}) . WT, then * (Mk > 0 ? 1 : 0) (ReLU'), then + R1 (may alias Y);
  // follows lfsr_set_lin_grad_arithmetic
  int dgemm(const float* X, int cin, const float* WT, float* Y, int ys, const float* R1, int r1s, const float* Mk, int mks, int N) const;
  // weight gradient of a raw (N <= 64, K, ntaps) weight from the columns [go, go + N) of Gr: the GATHER form (IN_SAME, xm) over M rows into ws.part
  int wgrad(int xm, const float* Gr, int gs, int go, const float* X, int xs, int M, int N, int K, int ntaps, float* dW, int accumulate, int c_valid = 0) const;
  // a (O, K) linear weight's gradient: Gr (O columns, stride gs) against X (K columns), over all pixels: the LINEAR form
  int wgrad_lin(const float* Gr, int gs, int O, const float* X, int xs, int K, float* dW) const;
  int ew(int C, const float* a, const float* b, const float* mk, float slope, float* d) const;   // lfsr_ew_launch on dense rows of C, over all pixels
  // LayerNorm backward with the gradients of its affine parameters written to G(gkey) / G(bkey); no position embedding: pe = nullptr, pe_rows = pe_div = 1
  int ln_bwd(int C, const float* X, const float* pe, long long pe_rows, long long pe_div, const std::string& gkey, const std::string& bkey, const float* dy,
             const float* r, float* dxo) const;
  // 64 -> 64 3x3 data gradient into dense rows of 64: dxo = conv^T(dy) * lrelu'(mk) + r1 (mk, r1 optional)
  int dgrad3(const float* dy, int dys, int dyo, const float* wT, float* dxo, const float* r1, const float* mk) const;
  int packT(const float* Wp, int n0, int C, int O, float* o) const;   // 1x1 dgrad pack of rows [n0, n0 + O) of a (Npad_in, C) forward pack: [C][O]
  int pack3T(const std::string& key, float* o) const;                 // dgrad pack of a 64 -> 64 3x3 weight, with its Winograd copies
};
// lfsr_trans_tail in reverse: from dout and the tail's input xin to dX = dL/d xin; writes the upsampling.3 and upsampling.0 gradients
int lfsr_trans_tail_bwd(const LfsrTransBwd& k, const float* dout, const float* xin, float* dX);
// lfsr_trans_head in reverse: from dbuf0 = dL/d buf0 and the saved f0 / c1 / c2; writes the four conv_init* gradients
int lfsr_trans_head_bwd(const LfsrTransBwd& k, const float* x, const float* f0, const float* c1, const float* c2, const float* dbuf0);
// the attention backward of a sublayer, the driver's choice of kernel and geometry: (q | k, v, o, d_o) -> (dqk, dv)
using LfsrAttnBwdCallback = std::function<int(const float* qk, const float* v, const float* o, const float* d_o, float* dqk, float* dv)>;
// lfsr_trans_ffn and lfsr_trans_qkv in reverse, one attention + feed-forward sublayer of width E (key prefix `pre`), from dy = dL/d y to the token:
//   y = x2 + FFN(LayerNorm(x2)), x2 = out_proj(ao) + tok, ao = attention(q | k, v), q | k = LayerNorm(tok + pe) W[0:2E]^T, v = tok W[2E:3E]^T.
// hid (2E) receives the hidden rows after the ReLU, rebuilt; lin: the five dgrad packs of lfsr_trans_sublayer_packs.  dtok = dL/d x2 + the v path's
// share of dL/d tok; ln_dx = the norm's share (+ ln_r, which may alias it).
int lfsr_trans_sublayer_bwd(const LfsrTransBwd& k, const std::string& pre, int E, const float* dy, const float* x2, const float* ao, const float* qk,
                            const float* v, const float* tok, const float* pe, long long pe_rows, long long pe_div, float* hid, float* const* lin,
                            const LfsrAttnBwdCallback& attn, float* dtok, const float* ln_r, float* ln_dx);
// ... and its 1x1 dgrad packs [C_in][O]: feed_forward.4, feed_forward.1, out_proj and the q | k and v rows of in_proj_weight into lin[0..4]
int lfsr_trans_sublayer_packs(const LfsrTransBwd& k, const std::string& pre, int E, float* const* lin);
