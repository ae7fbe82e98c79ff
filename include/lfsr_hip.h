/*
 * lfsr_hip.h -- C ABI of liblfsr_hip.so: the MI355X (gfx950) light-field SR hot path.
 *
 * Drop-in boundary for the reference's arithmetic layer (stock PyTorch ops called from
 * model/SR/{DistgSSR,EPIT,LFT,LF_InterNet,LFSSR}.py and utils/utils.py of the BasicLFSR fork).  Every entry
 * point cites the reference interface it replaces (file:line relative to the reference root).
 *
 * Conventions
 *   - plain pointers and sizes only; all data pointers are DEVICE pointers borrowed from the caller
 *     (never freed or retained past the call, except packed weights / workspaces the caller hands
 *     to a model context and keeps alive itself);
 *   - outputs are pre-allocated by the caller;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return value: 0 on success, LFSR_E_ARG (-1) for a bad argument, LFSR_E_WS (-2) for a too-small
 *     workspace, -(1000 + hipError_t) for a HIP runtime failure.  No exceptions cross the ABI;
 *   - re-entrant; the only process-wide state is per-device caches of idempotent function attributes / CU counts (atomic flags) and the
 *     lazily resolved RCCL entry points.
 *
 * Tensor layouts
 *   NCHW "SAI mosaic"  (B,C,A*h,A*w)  element [b,c,u*h+y,v*w+x]      -- what the reference passes around
 *   NCHW "MacPI"       (B,C,h*A,w*A)  element [b,c,y*A+u,x*A+v]      -- DistgSSR / LF_InterNet interior
 *   VCL  "view-major channel-last" [B][A*A][h][w][C] fp32             -- this library's interior layout:
 *        one pixel's C channels are contiguous (256 B for C=64), so spatial, angular and epipolar
 *        gathers are all coalesced and SAI<->MacPI rearranges disappear from the network interior.
 *        A VCL operand is described by (ptr, stride, choff): channel c of pixel p lives at
 *        ptr[p*stride + choff + c] (lets a branch write straight into a slice of a concat buffer).
 */
#ifndef LFSR_HIP_H
#define LFSR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFSR_OK 0
#define LFSR_E_ARG (-1)
#define LFSR_E_WS (-2)

/* library / build identification: returns a static NUL-terminated string ("lfsr_hip gfx950 ...") */
const char* lfsr_version(void);

/* ------------------------------------------------------------------------------------------------
 * a1-a7: integer-indexing primitives, bit-exact, reference NCHW layouts.  elem_bytes is 2 or 4.
 * ---------------------------------------------------------------------------------------------- */

/* SAI2MacPI, model/SR/DistgSSR.py:145-155 (dup LF_InterNet.py:155-165).  in/out (B,C,A*h,A*w). */
int lfsr_sai2macpi(const void* in, void* out, int B, int C, int A, int h, int w, int elem_bytes, void* stream);
/* MacPI2SAI, model/SR/DistgSSR.py:134-142 (dup LF_InterNet.py:144-152). */
int lfsr_macpi2sai(const void* in, void* out, int B, int C, int A, int h, int w, int elem_bytes, void* stream);
/* nn.PixelShuffle(r) as called at DistgSSR.py:26,89; EPIT.py:46; LFT.py:54; LF_InterNet.py:51,114,132.
 * in (B,C*r*r,H,W) -> out (B,C,H*r,W*r). */
int lfsr_pixel_shuffle2d(const void* in, void* out, int B, int C, int r, int H, int W, int elem_bytes, void* stream);
/* PixelShuffle1D, model/SR/DistgSSR.py:114-131 (factor-major).  in (B,f*C,H,W) -> out (B,C,H,W*f). */
int lfsr_pixel_shuffle1d(const void* in, void* out, int B, int C, int f, int H, int W, int elem_bytes, void* stream);
/* ImageExtend, utils/utils.py:137-149.  in (N,h,w) -> out (N,h+top+bottom,w+left+right), symmetric. */
int lfsr_image_extend(const void* in, void* out, int N, int h, int w, int top, int bottom, int left, int right,
                      int elem_bytes, void* stream);
/* LFdivide, utils/utils.py:152-166.  in (A*h0,A*w0) -> out (numU,numV,A*P,A*P);
 * numU=(h0+2*bdr-1)/S, numV=(w0+2*bdr-1)/S, bdr=(P-S)/2 (returned through num_u/num_v if non-NULL;
 * with out == NULL only the counts are computed). */
int lfsr_lf_divide(const void* in, void* out, int A, int h0, int w0, int P, int S, int elem_bytes,
                   int* num_u, int* num_v, void* stream);
/* LFintegrate, utils/utils.py:169-178.  in (numU,numV,A*pz,A*pz) -> out (A,A,h,w). */
int lfsr_lf_integrate(const void* in, void* out, int A, int numU, int numV, int pz, int stride, int h, int w,
                      int elem_bytes, void* stream);

/* LFintegrate factored for patch-sharded ranks (utils/utils.py:169-178 keeps only the centre stride x stride of every view of every SR patch):
 * crop: in (count,A*pz,A*pz) SR patches -> tiles (count,A,A,stride,stride), run by the rank that computed the patches (a quarter of the bytes then
 * crosses xGMI); place: the tiles of patches [first, first+count) of the row-major (numU,numV) list -> out (A,A,h,w), pixels beyond (h,w) dropped.
 * place(crop(x)) over all patches == lfsr_lf_integrate(x), bit for bit. */
int lfsr_lf_crop_tiles(const void* in, void* tiles, int A, int count, int pz, int stride, int elem_bytes, void* stream);
int lfsr_lf_place_tiles(const void* tiles, void* out, int A, int numU, int numV, int first, int count, int stride, int h, int w,
                        int elem_bytes, void* stream);

/* NCHW <-> VCL (fp32).  layout: 0 = SAI mosaic, 1 = MacPI.  VCL side described by (stride, choff). */
int lfsr_nchw_to_vcl(const float* in, float* out, int out_stride, int out_choff, int B, int C, int A, int h, int w,
                     int layout, void* stream);
int lfsr_vcl_to_nchw(const float* in, int in_stride, int in_choff, float* out, int B, int C, int A, int h, int w,
                     int layout, void* stream);

/* ------------------------------------------------------------------------------------------------
 * d1-d9: DistgSSR operator classes on VCL tensors (fp32, MFMA v_mfma_f32_32x32x2_f32 = exact fp32).
 * Weights are passed PACKED (see lfsr_pack_*): [tap][Npad][Cin], k contiguous, Npad = N rounded up to 32.
 * ---------------------------------------------------------------------------------------------- */

/* Pack a PyTorch conv weight (O,C,kh,kw) (device, fp32) into [kh*kw][Npad][C].
 * perm = 0: n' = n.   perm = 1 (PixelShuffle(A) feeding VCL views, DistgSSR.py:87-89): the reference's
 * output channel c*r2 + q becomes n' = q*ch + c (r2 = O/ch views, ch channels per view).
 * A 3x3 64->64 weight (O = C = 64, taps = 9, perm = 0) is followed by its Winograd-domain copies U = G g G^t
 * (computed in fp64, rounded once): F(2x2,3x3), 16 x 64 x 64 floats in the fragment order of conv3x3_wino.hip, then
 * F(4x4,3x3), 36 x 64 x 64 floats in the fragment order of conv3x3_wino4.hip (the default kernel);
 * lfsr_packed_weight_floats includes both and lfsr_conv3x3_fwd expects them there. */
int lfsr_pack_conv_weight(const float* w, float* packed, int O, int C, int taps, int perm, int ch, void* stream);
size_t lfsr_packed_weight_floats(int O, int C, int taps);

/* per-view 3x3 conv, zero pad 1 (== the MacPI conv "k3, dilation A, padding A" of DistgSSR.py:22,47,64,
 * 79-83,101; == Conv3d(1,3,3) of EPIT.py:24-32,136-142 / LFT.py:36-46), Cin=Cout=64:
 *   y = act(conv(x)) [+ r1] [+ r2],  act(v) = v >= 0 ? v : slope * v for any slope (1.0f: none, 0.0f: ReLU); a lone residual may be passed as r2.
 * n_img = B*A*A images of h x w.  x_stride and x_choff must be multiples of 4 and every stride at least its offset + 64 (LFSR_E_ARG otherwise, nothing
 * written); y, r1 and r2 may sit at any offset (off the 16-byte grid the gather-GEMM runs). */
int lfsr_conv3x3_fwd(const float* x, int x_stride, int x_choff, const float* w_packed,
                     float* y, int y_stride, int y_choff,
                     const float* r1, int r1_stride, int r1_choff, const float* r2, int r2_stride, int r2_choff,
                     int n_img, int h, int w, float slope, void* stream);

/* pointwise (1x1) conv: y[p, choff + n] = act(sum_k x[p,k] * W[n,k] (+bias[n])), Cin in {16,32,64,144},
 * any N (DistgSSR.py:99 fuse.0).  M pixels. */
int lfsr_pointwise_fwd(const float* x, int x_stride, int x_choff, int cin, const float* w_packed, const float* bias,
                       float* y, int y_stride, int y_choff, int M, int N, float slope, void* stream);

/* AngConv, DistgSSR.py:84-90: t = lrelu(conv AxA stride A 64->16); y = lrelu(1x1 16->16*A*A) scattered
 * by PixelShuffle(A) to the A*A views.  tmp: (B*h*w*16) floats. w1 packed perm 0, w2 packed perm 1 (ch 16). */
int lfsr_angconv_fwd(const float* x, int x_stride, int x_choff, const float* w1_packed, const float* w2_packed,
                     float* tmp, float* y, int y_stride, int y_choff, int B, int A, int h, int w, float slope, void* stream);

/* EPIConv, DistgSSR.py:91-97 (horizontal: vertical = 0) and its transposed application DistgSSR.py:108
 * (vertical = 1, same weights): t = lrelu(conv 1xA^2 stride A pad A(A-1)/2 64->32);
 * y = lrelu(1x1 32->32*A) scattered by PixelShuffle1D(A).  tmp: (B*A*h*w*32) floats; on return it holds the pass's stage-1 activation t, rows ordered
 * (b*A+u, y, x) / (b*A+v, y, x) -- what lfsr_epiconv_hv_bwd takes as e_h / e_v.  tmp may be NULL (nothing saved) where a fused kernel runs: A odd, A <= 5,
 * h, w <= 32, y_stride and y_choff multiples of 4, x below 2^31 bytes (B*A*A*h*w*x_stride*4), and LFSR_EPI=gather not selected in a lab process; the gather-GEMM
 * path everywhere else needs it and answers LFSR_E_ARG without it.  lrelu(v) = v >= 0 ? v :
 * slope * v for any slope (the three-term bf16 kernel of angRes 5 covers 0 <= slope <= 1; outside it the fp32-MFMA kernel runs). */
int lfsr_epiconv_fwd(const float* x, int x_stride, int x_choff, const float* w1_packed, const float* w2_packed,
                     float* tmp, float* y, int y_stride, int y_choff, int B, int A, int h, int w, int vertical,
                     float slope, void* stream);

/* Both EPI passes of a DisentgBlock (DistgSSR.py:107-108) in one launch: horizontal result to channel slice
 * choff_h, vertical (transposed application, same weights) to choff_v of y.  Uses the fused LDS-tile kernel
 * when (A odd, A <= 5, h,w <= 32; y_stride and both offsets multiples of 4; x below 2^31 bytes; LFSR_EPI=gather not selected), else two gather-GEMM launches per pass through tmp (may be NULL if fused:
 * LFSR_E_ARG, nothing written, where the gather-GEMM path would need it).  tmp is scratch here: the fused kernels leave it alone, the gather-GEMM path
 * leaves the vertical pass's stage-1 activation in it. */
int lfsr_epiconv_hv_fwd(const float* x, int x_stride, int x_choff, const float* w1_packed, const float* w2_packed,
                        float* tmp, float* y, int y_stride, int choff_h, int choff_v, int B, int A, int h, int w,
                        float slope, void* stream);

/* DisentgBlock tail, DistgSSR.py:84-99 at A = 5 under the default arithmetic: the angular and both epipolar branches of x, the concat
 * (spa | ang | epiH | epiV, 144 channels) and fuse.0 with its LeakyReLU, without the concat in memory: y (64 channels) = lrelu(fuse.0(concat)).
 * spa: the SpaConv.2 output (64 channels).  Weights packed as lfsr_angconv_fwd (w_ang0, w_ang2), lfsr_epiconv_hv_fwd (w_epi0, w_epi2) and
 * lfsr_pointwise_fwd (w_fuse0, cin 144) take them.  t_a (B*h*w*16), t_h, t_v (B*A*h*w*32 each) receive the stage-1 activations.  The result bits are those
 * of lfsr_angconv_fwd + lfsr_epiconv_hv_fwd + lfsr_pointwise_fwd over a (B*A*A*h*w, 144) concat whenever that pointwise call runs the three-term bf16
 * row-GEMM (M >= 2048).  LFSR_E_ARG: not covered (A != 5, h or w > 32, fp32 arithmetic or an fp32 lab selection, a tensor of 2^31 bytes or more). */
int lfsr_distg_branch_tail_fwd(const float* x, int x_stride, int x_choff, const float* spa, int spa_stride, int spa_choff,
                               const float* w_ang0, const float* w_ang2, const float* w_epi0, const float* w_epi2, const float* w_fuse0,
                               float* t_a, float* t_h, float* t_v, float* y, int y_stride, int y_choff, int B, int A, int h, int w, float slope,
                               void* stream);

/* init_conv, DistgSSR.py:22,32 fused with SAI2MacPI (DistgSSR.py:31): x (B,1,A*h,A*w) SAI mosaic NCHW,
 * w (64,1,3,3) raw PyTorch layout -> y VCL 64 channels. */
int lfsr_initconv_fwd(const float* x, const float* w, float* y, int y_stride, int y_choff, int B, int A, int h, int wd,
                      void* stream);

/* upsample head, DistgSSR.py:24-27,35 fused with MacPI2SAI (:34), PixelShuffle(s) and the bilinear skip
 * (:30): out (B,1,A*h*s,A*w*s) = PS_s(W'f + b') + bilinear_s(x_lr), with the linear chain
 * 1x1(64->64 s^2, bias) -> PixelShuffle -> 1x1(64->1) folded to W' (s^2 x 64), b' (s^2) by lfsr_fold_head. */
int lfsr_fold_head(const float* w0, const float* b0, const float* w2, float* wf, float* bf, int C, int s, void* stream);
int lfsr_upsample_head_fwd(const float* f, int f_stride, int f_choff, const float* wf, const float* bf,
                           const float* x_lr, float* out, int B, int A, int h, int w, int s, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Whole-model driver: DistgSSR forward (get_model.forward, DistgSSR.py:29-36).
 * ---------------------------------------------------------------------------------------------- */
typedef struct lfsr_distgssr lfsr_distgssr;

int lfsr_distgssr_create(lfsr_distgssr** ctx, int A, int scale, int n_group, int n_block, int channels);
void lfsr_distgssr_destroy(lfsr_distgssr* ctx);
/* bytes of device memory the packed weights need; caller allocates and hands over with set_packed */
size_t lfsr_distgssr_packed_bytes(const lfsr_distgssr* ctx);
int lfsr_distgssr_set_packed(lfsr_distgssr* ctx, void* packed, size_t bytes);
/* feed one state_dict entry (reference key names), raw PyTorch layout, device fp32.
 * Returns LFSR_E_ARG for an unknown key or a wrong element count. */
int lfsr_distgssr_load_param(lfsr_distgssr* ctx, const char* key, const float* data, size_t numel, void* stream);
/* after all params are loaded: folds the upsample head; returns LFSR_E_ARG if a parameter is missing */
int lfsr_distgssr_finalize(lfsr_distgssr* ctx, void* stream);
/* optional, before a round of lfsr_distgssr_load_param calls (a training step's repack): the packs are recorded instead of launched one by one and
 * lfsr_distgssr_finalize launches them, one kernel per pack kind (the descriptor table lives in a small device buffer owned by the context and is
 * re-uploaded only when a parameter's address changed).  The data pointers passed to load_param must stay valid until finalize's work has run. */
int lfsr_distgssr_begin_batched_load(lfsr_distgssr* ctx);
size_t lfsr_distgssr_workspace_bytes(const lfsr_distgssr* ctx, int B, int h, int w);
/* x (B,1,A*h,A*w) -> out (B,1,A*h*s,A*w*s), both NCHW SAI mosaics, fp32 */
int lfsr_distgssr_forward(lfsr_distgssr* ctx, const float* x, float* out, int B, int h, int w,
                          void* workspace, size_t workspace_bytes, void* stream);
/* parity variant: additionally writes interior activations as NCHW MacPI (B,64,h*A,w*A) tensors into
 * taps[i] (device pointers, NULL = skip): 0 = init_conv output, 1 = block(0,0) output, 2 = group 0 output,
 * 3 = disentg output; and block(0,0)'s concat buffer (B,144,h*A,w*A) into taps[4]. */
int lfsr_distgssr_forward_taps(lfsr_distgssr* ctx, const float* x, float* out, int B, int h, int w,
                               void* workspace, size_t workspace_bytes, float* const* taps, void* stream);

/* ---- training (config "DistgSSR x4 training, data-parallel"): forward that keeps the activations, and backward ----
 * Gradients are written into ONE flat fp32 bucket in state_dict order (lfsr_distgssr_param_offset gives each
 * parameter's span): exactly the buffer a data-parallel job hands to a single RCCL all-reduce.
 * The workspace must be the same memory for forward_train and the backward that follows it. */
size_t lfsr_distgssr_num_params(const lfsr_distgssr* ctx);
int lfsr_distgssr_param_offset(const lfsr_distgssr* ctx, const char* key, size_t* offset, size_t* numel);
size_t lfsr_distgssr_train_workspace_bytes(const lfsr_distgssr* ctx, int B, int h, int w);
int lfsr_distgssr_forward_train(lfsr_distgssr* ctx, const float* x, float* out, int B, int h, int w,
                                void* workspace, size_t workspace_bytes, void* stream);
/* parity aid: offset (in floats, into the training workspace) and size of an activation forward_train saved for the backward.  which: 0 SpaConv.0
 * output (VCL, 64 ch), 1 the concat buffer (VCL, 144 ch), 2 AngConv.0 output (rows (b,y,x), 16 ch), 3 / 4 EPIConv.0 output of the horizontal /
 * vertical pass (rows (b*A+u,y,x) / (b*A+v,y,x), 32 ch), 5 fuse.0 output (VCL, 64), 6 block output (VCL, 64); index = group * n_block + block.
 * All are post-LeakyReLU values: their signs are the LeakyReLU' masks the data gradients apply (DistgSSR.py:79-101). */
int lfsr_distgssr_train_saved(const lfsr_distgssr* ctx, int B, int h, int w, int which, int index, size_t* offset_floats, size_t* numel);
/* dout (B,1,A*h*s,A*w*s) = dLoss/dOut; grads: n_grads == lfsr_distgssr_num_params(ctx) floats, overwritten */
int lfsr_distgssr_backward(lfsr_distgssr* ctx, const float* x, const float* dout, int B, int h, int w,
                           void* workspace, size_t workspace_bytes, float* grads, size_t n_grads, void* stream);

/* ---- operator-level backward entry points (SURVEY 8b export list: conv3x3 dgrad / wgrad, pointwise bwd, upsample_head bwd).
 * They replace what autograd derives from nn.Conv2d in the reference's training step (train.py:256-264, fp32). ---- */
/* transposed pack used by the data gradients: w (O,C,kh,kw) raw PyTorch layout -> [tap'][Cpad][O] (3x3: taps flipped; O = C = 64, taps = 9
 * is followed by the Winograd-domain copies, as lfsr_pack_conv_weight does) */
size_t lfsr_packed_weight_tr_floats(int O, int C, int taps);
int lfsr_pack_conv_weight_tr(const float* w, float* packed_T, int O, int C, int taps, void* stream);
/* dx = (conv3x3^T(dy)) * LeakyReLU'(act) + r1: `act` = the saved output of the LeakyReLU(act_slope) in front of this conv's input
 * (NULL: none), r1 = a gradient arriving over a skip connection (NULL: none).  64 -> 64, per-view zero pad 1.  dy_stride and dy_choff must be
 * multiples of 4 (LFSR_E_ARG otherwise); dx, r1 and act may sit at any offset (off the 16-byte grid the gather-GEMM runs). */
int lfsr_conv3x3_dgrad(const float* dy, int dy_stride, int dy_choff, const float* wT_packed, float* dx, int dx_stride, int dx_choff,
                       const float* r1, int r1_stride, int r1_choff, const float* act, int act_stride, int act_choff, float act_slope,
                       int n_img, int h, int w, void* stream);
/* dw (64,64,3,3) raw PyTorch layout [= or += if accumulate] sum_pixels dy (x) shifted x; workspace: per-block partial slabs, reduced in a
 * second deterministic pass (no float atomics) */
size_t lfsr_conv3x3_wgrad_workspace_floats(int n_img, int h, int w);
int lfsr_conv3x3_wgrad(const float* dy, int dy_stride, int dy_choff, const float* x, int x_stride, int x_choff, float* dw,
                       float* workspace, size_t workspace_floats, int n_img, int h, int w, int accumulate, void* stream);
/* 1x1 conv y = x W^T, W (cout = 64, cin): dx = (dy W) * LeakyReLU'(act);  dw (cout, cin) = dy^T x  (cout <= 64) */
int lfsr_pointwise_dgrad(const float* dy, int dy_stride, int dy_choff, int cout, const float* wT_packed, float* dx, int dx_stride, int dx_choff, int cin,
                         const float* act, int act_stride, int act_choff, float act_slope, long long M, void* stream);
size_t lfsr_pointwise_wgrad_workspace_floats(long long M, int cout, int cin);
int lfsr_pointwise_wgrad(const float* dy, int dy_stride, int dy_choff, int cout, const float* x, int x_stride, int x_choff, int cin, float* dw,
                         float* workspace, size_t workspace_floats, long long M, int accumulate, void* stream);
/* data gradient of lfsr_upsample_head_fwd w.r.t. f: dout (B,1,A*h*s,A*w*s) -> df (pixels, 64) VCL; g16 (pixels, 16) scratch that receives the
 * un-shuffled output gradient (the operand of the folded matrix' weight gradient) */
int lfsr_upsample_head_dgrad(const float* dout, const float* wf, float* df, float* g16, int B, int A, int h, int w, int s, void* stream);

/* ---- the exchange step of data-parallel training: in-place sum-all-reduce of n fp32 values over RCCL (xGMI) -----------
 * The reference has no gradient exchange (single process; option.py:28 `--local_rank` is vestigial).  `comm` is an ncclComm_t created by
 * lfsr_comm_init (or by the caller with RCCL directly); unique_id = the 128-byte ncclUniqueId obtained on rank 0 and shipped to the others by
 * the host.  RCCL is resolved at run time (dlopen): lfsr_comm_available() is 0 on a host without it, and the calls then return LFSR_E_ARG.
 * Return: 0, LFSR_E_ARG, or -(2000 + ncclResult_t). */
int lfsr_comm_available(void);
int lfsr_comm_unique_id(void* id128);
int lfsr_comm_init(void** comm, int world, int rank, const void* id128);
int lfsr_comm_destroy(void* comm);
int lfsr_allreduce(void* grads, size_t n, void* comm, void* stream);

/* Per-operator-class timing with hipEvents recorded on the launch stream around every launch of the
 * forward (measurement aid for bench.py's roofline line; off by default).
 * classes: 0 conv3x3, 1 angconv, 2 epiconv, 3 pointwise (fuse.0), 4 init_conv, 5 upsample head. */
#define LFSR_DISTG_NCLASS 6
int lfsr_distgssr_profile(lfsr_distgssr* ctx, int enable);   /* 0 off, 1 every class, 2 class 0 (3x3 conv) only, 3 every 4th launch of class 0; drops recorded events */
/* waits for the recorded events, returns summed milliseconds and launch counts per class, then resets */
int lfsr_distgssr_profile_read(lfsr_distgssr* ctx, double* ms, long long* launches);

/* ------------------------------------------------------------------------------------------------
 * e1-e7 / l1-l5: transformer operator classes (EPIT.py:74-128, LFT.py:133-246) on VCL rows (tokens == pixels).
 * ---------------------------------------------------------------------------------------------- */
/* nn.LayerNorm(C) over M rows of (x [+ pe[(row / pe_div) % pe_rows]]); C in {64,128} (EPIT.py:78,83; LFT.py:142,150,211,215) */
int lfsr_layernorm_fwd(const float* x, int x_stride, int x_choff, const float* pe, int pe_stride, long long pe_rows, long long pe_div,
                       const float* gamma, const float* beta, float* y, int y_stride, int y_choff, long long M, int C,
                       float eps, void* stream);
/* nn.Linear (no transposes needed: weight (N,K) packed by lfsr_pack_conv_weight(O=N,C=K,taps=1)); K in {64,128,256};
 * y = act(x W^T + bias) + res;  slope 1 = identity, 0 = ReLU, else LeakyReLU.
 * Arithmetic: fp32 in, fp32 out, fp32 accumulation.  The bias-free K = 64 / 128 case (and lfsr_ffn_*, lfsr_linear_ln_fwd, lfsr_up_tail_fwd's 1x1 conv) runs on the bf16
 * MFMA pipe with every fp32 operand split EXACTLY into three bf16 terms (six products; error against fp64 no larger than the fp32-MFMA kernels': tools/b3_accuracy.py);
 * the environment selectors LFSR_ROWGEMM=f32, LFSR_FFN=f32, LFSR_UPTAIL=v2 choose the fp32-MFMA kernels. */
int lfsr_linear_fwd(const float* x, int x_stride, int x_choff, int cin, const float* w_packed, const float* bias,
                    const float* res, int res_stride, int res_choff, float* y, int y_stride, int y_choff,
                    long long M, int N, float slope, void* stream);
/* Fused feed-forward block of the transformers (EPIT.py:84-90,126; LFT.py:151-156,202,216-221,243):
 *   y = res + W2 . act(W1 . x)      x: (M, K1) LayerNorm'd tokens, W1 (H, K1), W2 (N2, H) packed as for lfsr_linear_fwd, no biases;
 * the (M, H) hidden activations stay on chip.  (K1, N2) in {(128,128), (64,64)}, H a multiple of 32; slope 0 = ReLU. */
int lfsr_ffn_fwd(const float* x, int x_stride, int x_choff, const float* w1_packed, const float* w2_packed,
                 const float* res, int res_stride, int res_choff, float* y, int y_stride, int y_choff,
                 long long M, int K1, int H, int N2, float slope, void* stream);
/* The same block with its leading LayerNorm (feed_forward.0: EPIT.py:85, LFT.py:152,217) formed in registers:
 *   y = res + W2 . act(W1 . LayerNorm(x))      x: (M, K1) RAW tokens, gamma / beta (K1), eps as nn.LayerNorm */
int lfsr_ffn_ln_fwd(const float* x, int x_stride, int x_choff, const float* gamma, const float* beta, float eps,
                    const float* w1_packed, const float* w2_packed, const float* res, int res_stride, int res_choff,
                    float* y, int y_stride, int y_choff, long long M, int K1, int H, int N2, float slope, void* stream);
/* LayerNorm + attention in-projection in one launch (EPIT.py:113-121; LFT.py:190-197,236-241): weight rows n < ln_cols (q | k) see
 * LayerNorm(x [+ pe[(row / pe_div) % pe_rows]]), rows n >= ln_cols (v) see x; columns n >= split_n go to y2 (column n - split_n).
 * K in {64,128}; N, ln_cols, split_n multiples of 64.  Same bits as lfsr_layernorm_fwd + lfsr_linear_fwd. */
int lfsr_linear_ln_fwd(const float* x, int x_stride, int x_choff, int K, const float* w_packed, const float* gamma, const float* beta,
                       float eps, int ln_cols, const float* pe, int pe_stride, int pe_rows, int pe_div,
                       float* y, int y_stride, int y_choff, float* y2, int y2_stride, int y2_choff, int split_n,
                       long long M, int N, void* stream);
/* nn.MultiheadAttention core with the reference's additive window mask evaluated as a predicate (EPIT.py:93-122,
 * LFT.py:161-199,238-241): o = softmax(q k^T / sqrt(hd) + mask) v per head; hd in {8,16}.
 * Sequences (s0,s1,s2) start at pixel s0*bs0+s1*bs1+s2*bs2; token (t1,t2) sits at + t1*st1 + t2*st2; token (t1,t2)
 * attends keys [t1-l1, t1+r1) x [t2-l2, min(t2+r2, clip2 or n2)) clipped to the grid. */
int lfsr_window_attn_fwd(const float* q, int q_stride, int q_choff, const float* k, int k_stride, int k_choff,
                         const float* v, int v_stride, int v_choff, float* o, int o_stride, int o_choff, int nheads, int hd,
                         int ns0, int ns1, int ns2, long long bs0, long long bs1, long long bs2,
                         int n1, int n2, long long st1, long long st2, int l1, int r1, int l2, int r2, int clip2, void* stream);
/* Backward of lfsr_window_attn_fwd, same geometry arguments.  q | k are columns q_choff / k_choff of one buffer of row stride qk_stride (as
 * the in-projection writes them); o is the forward's output and d_o its gradient (one row stride and channel offset for both).  Writes dQ | dK
 * into dqk in the layout of qk and dV into dv in the layout of v; nothing outside those nheads*hd-wide column ranges is touched.
 * stats: scratch of 4 floats per (pixel, head) over the pixel span the sequences cover (the softmax statistics the VALU kernels pass from their
 * query pass to their key pass; the matrix-pipe kernel of the EPI geometry recomputes them and leaves it alone).  No float atomics: two runs
 * give the same bits. */
int lfsr_window_attn_bwd(const float* qk, int qk_stride, int q_choff, int k_choff, const float* v, int v_stride, int v_choff,
                         const float* o, const float* d_o, int o_stride, int o_choff, float* dqk, float* dv, float* stats,
                         int nheads, int hd, int ns0, int ns1, int ns2, long long bs0, long long bs1, long long bs2,
                         int n1, int n2, long long st1, long long st2, int l1, int r1, int l2, int r2, int clip2, void* stream);
/* ---- the backward operators the LFT and EPIT training drivers share (the launchers those drivers call).  No float atomics: two runs give the same bits. ----
 * LayerNorm backward of y = LN(x + pe[(row / pe_div) % pe_rows]) gamma + beta, eps 1e-5, over M rows; C in {64,128}.  x, dy, r, dx: dense rows of C floats;
 * pe (NULL: none; else pe_rows > 0, pe_div > 0): dense rows of C; every pointer 16-byte aligned.  Writes dx = dL/dx (+ r if r is not NULL; r may be dx itself,
 * no other operands may overlap), dgamma (C) and dbeta (C), both overwritten, and the workspace (lfsr_layernorm_bwd_workspace_floats(C) = 1024 * 2 C
 * floats of per-block partials; 0 for an unsupported C).  LFSR_E_ARG / LFSR_E_WS before any launch. */
size_t lfsr_layernorm_bwd_workspace_floats(int C);
int lfsr_layernorm_bwd(const float* x, const float* pe, long long pe_rows, long long pe_div, const float* gamma, const float* dy, const float* r, float* dx,
                       float* dgamma, float* dbeta, float* workspace, size_t workspace_floats, long long M, int C, void* stream);
/* Data gradient of nn.Linear y = x W^T, W (cout, cin), with the extras of the transformer sublayers:  dx = (dy W) * (act > 0 ? 1 : 0) + r1.
 * dy: M dense rows of cout in {64,128,256,576,1024}, 16-byte aligned; wT_packed from lfsr_pack_conv_weight_tr(W, cout, cin, 1); cin in {64,128,256}.
 * dx, r1 (NULL: none), act (NULL: no mask; the saved ReLU output): rows of cin floats at row strides >= cin that are multiples of 4; r1 may be dx itself.
 * Writes columns [0, cin) of the M rows of dx and nothing else.  M < 2^31 - 128.  LFSR_E_ARG before any launch.  Follows lfsr_set_lin_grad_arithmetic (below). */
int lfsr_linear_dgrad(const float* dy, int cout, const float* wT_packed, float* dx, int dx_stride, const float* r1, int r1_stride, const float* act, int act_stride,
                      long long M, int cin, void* stream);
/* Backward of lfsr_hr_tail_fwd's LeakyReLU(slope) + 3x3 conv 64 -> 1 (zero pad 1 over the whole mosaic), s in {2,3,4}:
 * dout (B, 1, A h s, A w s); w3 (1, 64, 3, 3) raw; hr: the channel-last HR pre-activation (B, A h s, A w s, 64) of lfsr_upsample_ps_fwd.
 * Writes du (B A^2 h w, 64 s^2), the gradient of upsampling.0's output un-shuffled to VCL rows p = (b, u, v, y, x) with columns c s^2 + i s + j
 * (= dHR[b][(u h + y) s + i][(v w + x) s + j][c], LeakyReLU' = 1 for hr > 0, slope otherwise), dw3 (1, 64, 3, 3) overwritten, and the workspace
 * (lfsr_up_tail_bwd_workspace_floats() = 1024 * 576 floats).  Every pointer 16-byte aligned; no overlap.  LFSR_E_ARG / LFSR_E_WS before any launch. */
size_t lfsr_up_tail_bwd_workspace_floats(void);
int lfsr_up_tail_bwd(const float* dout, const float* w3, const float* hr, float* du, float* dw3, float* workspace, size_t workspace_floats, int B, int A, int h, int w,
                     int s, float slope, void* stream);
/* the data-gradient pack of upsampling.0 (64 s^2, 64) from its forward pack (lfsr_pack_conv_weight perm 1, ch 64: row ij * 64 + c, 64 floats):
 * out[k][c s^2 + ij] = w_packed[(ij * 64 + c) * 64 + k], 64 rows of 64 s^2 -- what lfsr_linear_dgrad(du, 64 s^2, out, ..., cin = 64) reads; s in {2,3,4} */
int lfsr_pack_up0_weight_tr(const float* w_packed, float* out, int s, void* stream);
/* per-view 3x3 conv 64 -> N for any N (gather-GEMM): LFT's unfold(3x3) + Linear(576 -> 128) token embedding (LFT.py:176-182) */
int lfsr_conv3x3_n_fwd(const float* x, int x_stride, int x_choff, const float* w_packed, float* y, int y_stride, int y_choff,
                       int n_img, int h, int w, int N, float slope, void* stream);
/* PositionEncoding.forward (LFT.py:106-130): spa_pe (h*w, C), ang_pe (A*A, C) */
int lfsr_lft_position_fwd(float* spa_pe, float* ang_pe, int A, int h, int w, int C, void* stream);
/* up-sampling tail shared by EPIT (EPIT.py:44-49) and LFT (LFT.py:52-57):
 * 1x1 64->64 s^2 (no bias) + PixelShuffle(s) into the channel-last HR mosaic (B, A*h*s, A*w*s, 64) [w packed perm 1, ch 64];
 * then LeakyReLU(slope) -> 3x3 conv 64->1 (zero pad 1 over the whole mosaic) + per-view bicubic skip of x_lr. */
int lfsr_upsample_ps_fwd(const float* f, int f_stride, int f_choff, const float* w_packed, float* hr, int B, int A, int h, int w,
                         int s, void* stream);
/* both steps fused (s in {2,4}): the (B,64,A h s,A w s) intermediate never exists.  w0_packed as for lfsr_upsample_ps_fwd. */
int lfsr_up_tail_fwd(const float* f, int f_stride, int f_choff, const float* w0_packed, const float* w3, const float* x_lr, float* out,
                     int B, int A, int h, int w, int s, float slope, void* stream);
int lfsr_hr_tail_fwd(const float* hr, const float* w3, const float* x_lr, float* out, int B, int A, int h, int w, int s,
                     float slope, void* stream);

/* Whole-model driver: EPIT forward (get_model.forward, EPIT.py:51-71).  Same life cycle as lfsr_distgssr_*. */
typedef struct lfsr_epit lfsr_epit;
int lfsr_epit_create(lfsr_epit** ctx, int A, int scale, int n_block, int channels);
void lfsr_epit_destroy(lfsr_epit* ctx);
size_t lfsr_epit_packed_bytes(const lfsr_epit* ctx);
int lfsr_epit_set_packed(lfsr_epit* ctx, void* packed, size_t bytes);
int lfsr_epit_load_param(lfsr_epit* ctx, const char* key, const float* data, size_t numel, void* stream);
int lfsr_epit_finalize(lfsr_epit* ctx, void* stream);
size_t lfsr_epit_workspace_bytes(const lfsr_epit* ctx, int B, int h, int w);
int lfsr_epit_forward(lfsr_epit* ctx, const float* x, float* out, int B, int h, int w, void* workspace, size_t workspace_bytes,
                      void* stream);

/* ---- EPIT training: the same contract as the LFT training ABI below.  Gradients go into ONE flat fp32 bucket in state_dict order (71 tensors at
 * n_block = 5: an AltFilter's epi_trans and conv weights serve both of its passes and receive the sum of both contributions, in a fixed order);
 * the feed-forward weights' pre-split image in the packed buffer is no parameter and lfsr_epit_param_offset refuses any key outside state_dict.
 * forward_train = the inference forward's launches (bit-equal output) on buffers that keep every sublayer's input; a no-grad forward in the
 * inference workspace leaves them in place.  train_workspace_bytes is 0 for a null context and outside the covered geometry (every activation,
 * the 256-float q | k rows and the 64 s^2-float HR rows included, below 2 GiB). */
size_t lfsr_epit_num_params(const lfsr_epit* ctx);
int lfsr_epit_param_offset(const lfsr_epit* ctx, const char* key, size_t* offset, size_t* numel);
size_t lfsr_epit_train_workspace_bytes(const lfsr_epit* ctx, int B, int h, int w);
int lfsr_epit_forward_train(lfsr_epit* ctx, const float* x, float* out, int B, int h, int w, void* workspace, size_t workspace_bytes, void* stream);
/* Where in the training workspace a saved activation lies (floats from its base), VCL rows.  Pass index j = 2 * block + vertical.
 * which: 0 the input of AltFilter `index` (64 floats a row; index = n_block: the tail's input), 1 conv_init's LeakyReLU outputs (index 0:
 * conv_init.0, 1: conv_init.2; 64), 2 / 3 the LeakyReLU outputs of conv.0 / conv.2 of pass `index` (64).  After a backward, what it rebuilt and
 * took its ReLU / LeakyReLU decisions from: 4 the feed-forward hidden rows after the ReLU of pass `index` (256), 5 conv_init.4's LeakyReLU
 * output without the residual (64; index 0), 6 the HR pre-activation ((B, A h s, A w s, 64); index 0). */
int lfsr_epit_train_saved(const lfsr_epit* ctx, int B, int h, int w, int which, int index, size_t* offset_floats, size_t* numel);
/* dout (B,1,A*h*s,A*w*s) = dLoss/dOut; grads: n_grads == lfsr_epit_num_params(ctx) floats, overwritten */
int lfsr_epit_backward(lfsr_epit* ctx, const float* x, const float* dout, int B, int h, int w, void* workspace, size_t workspace_bytes,
                       float* grads, size_t n_grads, void* stream);

/* Whole-model driver: LFT forward (get_model.forward, LFT.py:67-98). */
typedef struct lfsr_lft lfsr_lft;
int lfsr_lft_create(lfsr_lft** ctx, int A, int scale, int n_layer, int channels);
void lfsr_lft_destroy(lfsr_lft* ctx);
size_t lfsr_lft_packed_bytes(const lfsr_lft* ctx);
int lfsr_lft_set_packed(lfsr_lft* ctx, void* packed, size_t bytes);
int lfsr_lft_load_param(lfsr_lft* ctx, const char* key, const float* data, size_t numel, void* stream);
int lfsr_lft_finalize(lfsr_lft* ctx, void* stream);
size_t lfsr_lft_workspace_bytes(const lfsr_lft* ctx, int B, int h, int w);
int lfsr_lft_forward(lfsr_lft* ctx, const float* x, float* out, int B, int h, int w, void* workspace, size_t workspace_bytes,
                     void* stream);
/* ---- LFT training: the same contract as the LF_InterNet training ABI.  Gradients go into ONE flat fp32 bucket in state_dict order (78 tensors
 * at n_layer = 4; the packed table's internal entries MLP.weight#lo / #hi are not parameters and lfsr_lft_param_offset refuses them).
 * forward_train runs the inference forward's launches (bit-identical output in either arithmetic) and keeps the sublayer inputs the backward
 * reads; the backward recomputes LayerNorm statistics, feed-forward hidden rows and the HR map.  The workspace must be the same memory for
 * forward_train and the backward that follows.  train_workspace_bytes returns 0 for a geometry the path refuses (every activation, the
 * 64 s^2-float HR rows included, below 2 GiB). */
size_t lfsr_lft_num_params(const lfsr_lft* ctx);
int lfsr_lft_param_offset(const lfsr_lft* ctx, const char* key, size_t* offset, size_t* numel);
size_t lfsr_lft_train_workspace_bytes(const lfsr_lft* ctx, int B, int h, int w);
int lfsr_lft_forward_train(lfsr_lft* ctx, const float* x, float* out, int B, int h, int w, void* workspace, size_t workspace_bytes, void* stream);
/* parity aid: offset (floats, into the training workspace) and size of an activation forward_train saved (VCL rows).  which: 0 the input of
 * AltFilter `index` (64; index = n_layer: the tail's input), 1 the angular feed-forward input (64), 2 the spatial feed-forward input (128),
 * 3 the spatial tokens (128), 4 the spatial feed-forward output (128) of layer `index`; 5 conv_init's LeakyReLU outputs (64; index 0 / 1).
 * After a backward, what it rebuilt and took its ReLU / LeakyReLU decisions from: 6 / 7 the angular (128) / spatial (256) feed-forward hidden
 * rows after the ReLU of layer `index`, 8 conv_init.4's LeakyReLU output without the residual (64), 9 the HR pre-activation ((B, A h s, A w s, 64)). */
int lfsr_lft_train_saved(const lfsr_lft* ctx, int B, int h, int w, int which, int index, size_t* offset_floats, size_t* numel);
/* dout (B,1,A*h*s,A*w*s) = dLoss/dOut; grads: n_grads == lfsr_lft_num_params(ctx) floats, overwritten */
int lfsr_lft_backward(lfsr_lft* ctx, const float* x, const float* dout, int B, int h, int w, void* workspace, size_t workspace_bytes,
                      float* grads, size_t n_grads, void* stream);

/* ---- "next" rows: the steps either side of the hot path in the training loop, on the device ----
 * N2: cal_metrics (utils/utils.py:91-134): per-view PSNR (and SSIM, skimage semantics with gaussian_weights=True) of two
 * (B,1,A*H,A*W) SAI mosaics, fp64 accumulation; psnr/ssim: B*A*A doubles (ssim may be NULL; SSIM needs views >= 11x11). */
int lfsr_view_metrics(const float* label, const float* out, double* psnr, double* ssim, int B, int A, int H, int W, void* stream);
/* N3: MaskedAngularPretraining.forward, utils/masked_pretraining.py:85-139: y = x with the views flagged in mask[A*A]
 * (device bytes) filled with `fill` ('zero' / 'mean' strategies; the reference applies one mask to the whole batch). */
int lfsr_mask_views(const float* x, float* y, const unsigned char* mask, float fill, int B, int C, int A, int h, int w, void* stream);
/* the same with one fill value per view, fill[A*A] device floats (mask_value 'mean' with several masked views: each view is filled with
 * its OWN mean over batch, channels and pixels, masked_pretraining.py:121-123) */
int lfsr_mask_views_fill(const float* x, float* y, const unsigned char* mask, const float* fill, int B, int C, int A, int h, int w, void* stream);

/* N4, output tail of test() (train.py:329-341, inference.py:205-216; utils/utils.py:191-204 ycbcr2rgb):
 * out[(u, v, y, x, c)] = uint8(clip(M255 . (Y, Cb, Cr) - offset, 0, 1) * 255), evaluated in fp64 like the reference's numpy path.
 * y (A*h, A*w) and cbcr (2, A*h, A*w) fp32 SAI mosaics; minv255 = inv(M) * 255 (row-major 3x3) and offset = inv(M) . (16,128,128),
 * both computed by the caller exactly as the reference does; out: (A, A, h, w, 3) uint8. */
int lfsr_ycbcr2rgb_views(const float* y, const float* cbcr, unsigned char* out, int A, int h, int w, const double* minv255,
                         const double* offset, void* stream);

/* Whole-model driver: LF_InterNet forward (get_model.forward, LF_InterNet.py:33-41); n_groups = n_layers = 4 upstream. */
typedef struct lfsr_internet lfsr_internet;
int lfsr_internet_create(lfsr_internet** ctx, int A, int scale, int n_groups, int n_layers);
void lfsr_internet_destroy(lfsr_internet* ctx);
size_t lfsr_internet_packed_bytes(const lfsr_internet* ctx);
int lfsr_internet_set_packed(lfsr_internet* ctx, void* packed, size_t bytes);
int lfsr_internet_load_param(lfsr_internet* ctx, const char* key, const float* data, size_t numel, void* stream);
int lfsr_internet_finalize(lfsr_internet* ctx, void* stream);
size_t lfsr_internet_workspace_bytes(const lfsr_internet* ctx, int B, int h, int w);
int lfsr_internet_forward(lfsr_internet* ctx, const float* x, float* out, int B, int h, int w, void* workspace,
                          size_t workspace_bytes, void* stream);
/* ---- LF_InterNet training (n_groups = n_layers = 4; other geometries: LFSR_E_ARG): the same contract as the DistgSSR training ABI.
 * Gradients go into ONE flat fp32 bucket in state_dict order (lfsr_internet_param_offset gives each parameter's span).  forward_train runs
 * the inference forward's launches (bit-identical output), keeps every activation the backward reads and builds the transposed weight packs
 * the backward reads from the current packed weights; the workspace must be the same memory for forward_train and the backward that follows.
 * train_workspace_bytes returns 0 for a geometry the path refuses (the forward's per-tensor bound: B*A*A*h*w*320 < 2^31). */
size_t lfsr_internet_num_params(const lfsr_internet* ctx);
int lfsr_internet_param_offset(const lfsr_internet* ctx, const char* key, size_t* offset, size_t* numel);
size_t lfsr_internet_train_workspace_bytes(const lfsr_internet* ctx, int B, int h, int w);
int lfsr_internet_forward_train(lfsr_internet* ctx, const float* x, float* out, int B, int h, int w,
                                void* workspace, size_t workspace_bytes, void* stream);
/* parity aid: offset (floats, into the training workspace) and size of an activation forward_train saved.  which: 0 a chain layer's input
 * rows [xs | spa2] (VCL, 128), 1 its rows [xa | ang2] (rows (b,y,x), 128), 2 ReLU(SpaConvSq) (VCL, 64), 3 ReLU(AngConvSq) ((b,y,x), 64),
 * 4 ReLU(SpaBottle) (VCL, 64), 5 ReLU(AngBottle) ((b,y,x), 64); index = g * n_layers + l (0..15) for 0..3, 0 for 4 / 5. */
int lfsr_internet_train_saved(const lfsr_internet* ctx, int B, int h, int w, int which, int index, size_t* offset_floats, size_t* numel);
/* dout (B,1,A*h*s,A*w*s) = dLoss/dOut; grads: n_grads == lfsr_internet_num_params(ctx) floats, overwritten */
int lfsr_internet_backward(lfsr_internet* ctx, const float* x, const float* dout, int B, int h, int w,
                           void* workspace, size_t workspace_bytes, float* grads, size_t n_grads, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LFSSR (model/SR/LFSSR.py, the spatial-angular separable network): INFERENCE only -- there is no backward and there are no num_params / param_offset / *_train
 * symbols.  Scale 2 (net2x) and 4 (net4x), angRes 2..9, any view size.  All its convs have biases; the activation is ReLU.
 * The four kernels below have one arithmetic each and read none of the four arithmetic switches further down; the per-view 64 -> 64 3x3 convs of the model (the
 * spatial half of every AltFilter, the four sub-pixel convs of lfsr_conv3x3_ps2_fwd) run through the 3x3 dispatcher and so follow lfsr_set_arithmetic; LFSSR is
 * tested under that mode, alone and with lfsr_set_ang_arithmetic, across its geometry matrix (tests/test_gpu_lfssr_geometries.py::test_bf16_modes).
 * ---------------------------------------------------------------------------------------------- */
/* The angular half of an AltFilter (LFSSR.py:201,208-215): at every pixel, a 3x3 conv 64 -> 64 with zero padding over the A x A grid of views, on VCL rows
 * p = ((b A + u) A + v) npix + q (npix = h w):
 *   y[b,u,v,q,o] = relu(bias[o] + sum over du, dv in {-1,0,1} with 0 <= u+du < A and 0 <= v+dv < A, and over c, of
 *                       W[o,c,du+1,dv+1] * pre(x[b,u+du,v+dv,q,c])),      pre(t) = in_bias ? max(t + in_bias[c], 0) : t
 * (in_bias, may be NULL: the bias and ReLU of the conv in front, applied while the operand is staged; a view outside the grid contributes zero AFTER that prologue
 * and is never loaded).  w_packed: lfsr_pack_conv_weight(O = 64, C = 64, taps = 9, perm = 0), of which the direct [9][64][64] part is read.  fp32 MFMA, exact
 * products; no atomics: two runs give the same bits and a sample's result does not depend on B.  LFSR_E_ARG before any launch: A outside 2..9, strides or offsets
 * that are no multiples of 4 or a stride below its offset + 64, x / y / w_packed / in_bias off the 16-byte grid, an operand span (B A^2 npix stride floats) of
 * 2 GiB or more. */
int lfsr_angconv3x3_fwd(const float* x, int x_stride, int x_choff, const float* w_packed, const float* bias, const float* in_bias,
                        float* y, int y_stride, int y_choff, int B, int A, int npix, void* stream);
/* conv0 (LFSSR.py:59,92): x (B,1,A*h,A*w) SAI mosaic NCHW, w (64,1,3,3) and bias (64) raw -> y VCL 64 channels = relu(per-view 3x3 conv, zero pad 1, + bias).
 * y_stride, y_choff multiples of 4. */
int lfsr_lfssr_conv0_fwd(const float* x, const float* w, const float* bias, float* y, int y_stride, int y_choff, int B, int A, int h, int wd, void* stream);
/* fup (LFSSR.py:62-66): per-view 3x3 conv 64 -> 256 + bias, PixelShuffle(2), ReLU, into VCL rows of the n_img views of (2h, 2w): y[(img, 2y+i, 2x+j), c] =
 * relu(conv(x)[img, 4c + 2i + j, y, x] + bias[4c + 2i + j]).  w_packed4: four consecutive lfsr_pack_conv_weight(64, 64, 9) packs, pack 2i + j made from rows
 * 4c + 2i + j (c = 0..63) of the (256,64,3,3) weight; bias (256) raw; tmp: n_img*h*w*256 floats of scratch (the four conv results side by side).  x, y, tmp
 * 16-byte aligned, strides and offsets multiples of 4; every tensor below 2 GiB. */
int lfsr_conv3x3_ps2_fwd(const float* x, int x_stride, int x_choff, const float* w_packed4, const float* bias, float* tmp, float* y, int y_stride, int y_choff,
                         int n_img, int h, int w, void* stream);
/* res + iup (LFSSR.py:67-71,95-98): out = conv3x3_{64->1}(f) + b_res + PixelShuffle2(conv3x3_{1->4}(lo) + b_iup), per view, zero pad 1.  f: VCL rows of the
 * B*A*A views of (2h, 2w); lo: per-view planes (B*A*A, h, w); w_res (1,64,3,3), b_res (1), w_iup (4,1,3,3), b_iup (4) raw.  mosaic = 0: out as per-view planes
 * (B*A*A, 2h, 2w); 1: out as the SAI mosaic (B,1,A*2h,A*2w). */
int lfsr_lfssr_tail_fwd(const float* f, int f_stride, int f_choff, const float* w_res, const float* b_res, const float* lo, const float* w_iup, const float* b_iup,
                        float* out, int B, int A, int h, int w, int mosaic, void* stream);
/* Whole-model driver: LFSSR forward (get_model.forward, LFSSR.py:30-46).  The life cycle and error codes of lfsr_internet_*; state_dict keys net.conv0.*,
 * net.altblock{1,2}.{i}.{spaconv,angconv}.*, net.fup{1,2}.0.*, net.res{1,2}.*, net.iup{1,2}.0.* (48 tensors at scale 2 and 94 at scale 4 with n_layer = 10, the
 * reference's depth; any n_layer >= 1 is accepted).  create: LFSR_E_ARG for a scale other than 2 and 4 or A outside 2..9.  forward: LFSR_E_ARG, nothing written,
 * when a tensor of the forward (the widest: 256 floats per LR pixel at scale 2, 1024 at scale 4) would reach 2 GiB. */
typedef struct lfsr_lfssr lfsr_lfssr;
int lfsr_lfssr_create(lfsr_lfssr** ctx, int A, int scale, int n_layer);
void lfsr_lfssr_destroy(lfsr_lfssr* ctx);
size_t lfsr_lfssr_packed_bytes(const lfsr_lfssr* ctx);
int lfsr_lfssr_set_packed(lfsr_lfssr* ctx, void* packed, size_t bytes);
int lfsr_lfssr_load_param(lfsr_lfssr* ctx, const char* key, const float* data, size_t numel, void* stream);
int lfsr_lfssr_finalize(lfsr_lfssr* ctx, void* stream);
size_t lfsr_lfssr_workspace_bytes(const lfsr_lfssr* ctx, int B, int h, int w);
int lfsr_lfssr_forward(lfsr_lfssr* ctx, const float* x, float* out, int B, int h, int w, void* workspace, size_t workspace_bytes, void* stream);

/* ---- backward of the disentangling branches as operators (disentg_branches_bwd; reference layers DistgSSR.py:84-97,108, differentiated by
 * autograd in train.py:256-264).  Raw PyTorch-layout weights in (the entry points pack what their kernels read into the workspace), raw-layout weight
 * gradients out (overwritten); dx (pixels, 64) VCL is ACCUMULATED into (the block input receives gradients from four branches).
 * AngConv: y = PixelShuffle_A(lrelu(W2 . a16)), a16 = lrelu(W0 (*) x).  dy: dLoss/dy, 16 channels at dy_choff of a VCL buffer of row stride dy_stride;
 * y: the branch output as lfsr_angconv_fwd wrote it (its signs are the LeakyReLU' mask of stage 2), or NULL when dy already is the gradient at the stage-2
 * pre-activation (what lfsr_pointwise_dgrad with act = the concat buffer leaves); x: the block input (pixels, 64) VCL; a16: the stage-1 activation
 * lfsr_angconv_fwd left in its `tmp` argument ((B h w), 16); w0 (16,64,A,A), w2 (16 A^2,16,1,1). */
size_t lfsr_angconv_bwd_workspace_floats(int B, int A, int h, int w);
int lfsr_angconv_bwd(const float* dy, int dy_stride, int dy_choff, const float* y, int y_stride, int y_choff, const float* x, const float* a16,
                     const float* w0, const float* w2, float* dx, float* dw0, float* dw2, float* workspace, size_t workspace_floats,
                     int B, int A, int h, int w, float slope, void* stream);
/* EPIConv on the tensor and on its transpose (shared weights; both passes' weight gradients summed): dy holds dLoss/dy_h at choff_h and dLoss/dy_v at
 * choff_v (32 channels each); y likewise the two outputs (or NULL, as above); e_h / e_v: the stage-1 activations lfsr_epiconv_fwd(vertical = 0 / 1) left
 * in `tmp` ((B A h w), 32); w0 (32,64,1,A^2), w2 (32 A,32,1,1).  Odd angRes only (symmetric padding of the EPI line).
 * EPIConv.0's data gradient (into dx) and weight gradient (dw0) follow lfsr_set_branch_grad_arithmetic (below) where their EPI-line kernels apply: A = 5, a pass's
 * line length <= 32 (the weight gradient: both h and w <= 32); stage 2 (dE, dw2) does not, and the workspace does not depend on the mode. */
size_t lfsr_epiconv_hv_bwd_workspace_floats(int B, int A, int h, int w);
int lfsr_epiconv_hv_bwd(const float* dy, int dy_stride, int choff_h, int choff_v, const float* y, int y_stride, int y_choff_h, int y_choff_v,
                        const float* x, const float* e_h, const float* e_v, const float* w0, const float* w2,
                        float* dx, float* dw0, float* dw2, float* workspace, size_t workspace_floats, int B, int A, int h, int w, float slope, void* stream);

/* ---- arithmetic of the GEMMs that exist in two forms (DistgSSR's EPI branch and fuse.0; the transformers' linears, fused FFN and up-sampling tail) ----
 * LFSR_ARITH_DEFAULT: fp32 operands carried EXACTLY as three bf16 terms on the bf16 MFMA pipe, six products, fp32 accumulation (error against fp64 not above the
 * fp32-MFMA kernels': tests/test_gpu_b3_accuracy.py); LFSR_ARITH_F32: every GEMM on fp32 MFMA.  Process-wide, read at every launch; the 3x3 convs, the angular
 * branch and the attention kernels compute on fp32 MFMA either way.  The reference computes all of these layers with stock fp32 torch ops.
 * LFSR_ARITH_BF16: reduced-precision operands for ONE layer class, opt-in.  Only the 64 -> 64 per-view 3x3 forward conv (lfsr_conv3x3_fwd on 16-B aligned operands,
 * hence every such conv of the four model drivers' forward and forward_train) changes: its activations and weights are rounded to bf16 (nearest even), the products
 * are exact and accumulation, LeakyReLU and residual adds are fp32; activations stay fp32 in memory.  Everything else runs exactly as under LFSR_ARITH_DEFAULT (the
 * GEMMs keep their exact three-term bf16 form, lfsr_distg_branch_tail_fwd covers what it covers there): lfsr_conv3x3_n_fwd, LF_InterNet's 128 -> 64 convs, the
 * angular branch, the attention kernels, unaligned conv operands (fp32 gather-GEMM) and every data- and weight-gradient kernel do not change (the gradients have a
 * switch of their own: lfsr_set_grad_arithmetic below).  A backward after a
 * forward_train in this mode differentiates the fp32 layers at that forward's activations, as autocast does; parity with the reference's gradients is claimed only
 * in the other two modes. */
#define LFSR_ARITH_DEFAULT 0
#define LFSR_ARITH_F32 1
#define LFSR_ARITH_BF16 2
int lfsr_set_arithmetic(int mode);
int lfsr_get_arithmetic(void);

/* ---- arithmetic of the 64 -> 64 per-view 3x3 conv's GRADIENTS: a second process-wide selection, independent of lfsr_set_arithmetic, read at every launch ----
 * LFSR_GRAD_ARITH_DEFAULT: every gradient kernel as it is (fp32 MFMA, Winograd forms), bit for bit.
 * LFSR_GRAD_ARITH_BF16: opt-in, the backward counterpart of LFSR_ARITH_BF16.  Two operators change:
 *  - the data gradient of that conv (lfsr_conv3x3_dgrad, and inside the drivers every call of the 3x3 dispatcher in its gradient direction, both with one and with
 *    two residuals, on 16-B aligned operands: the 64 -> 64 3x3 data gradients of lfsr_distgssr_backward, lfsr_epit_backward, lfsr_lft_backward and
 *    lfsr_internet_backward all follow the mode): dy and the transposed weight are rounded to bf16 (nearest even), the products are exact, accumulation, the
 *    LeakyReLU mask and the residual adds are fp32;
 *  - the weight gradient of that conv where it runs on the tile kernel (lfsr_conv3x3_wgrad and lfsr_distgssr_backward): dy and x are rounded to bf16, products
 *    exact, fp32 accumulation into the same per-block partial slabs, the same reduction.  lfsr_conv3x3_wgrad_workspace_floats does not depend on the mode.
 * What does not change: gradients, activations and slabs stay fp32 in memory; the forward (it does not read this switch); the EPI, angular, fuse.0, 1x1,
 * 128 | 320 -> 64 weight gradients (LF_InterNet's wide convs: they have a switch of their own, lfsr_set_wide_train_arithmetic below; their data gradients are
 * 64 -> 64 calls of the dispatcher and do follow this mode) and up-sampling gradients; the transformers' GEMM gradients (they have a switch of their own: lfsr_set_lin_grad_arithmetic below); unaligned data-gradient operands (fp32 gather-GEMM); strides the bf16 weight-gradient
 * kernel does not cover (the default kernel); and the 3x3 weight gradients of the EPIT, LFT and LF_InterNet drivers, which run through the generic gather
 * weight-gradient kernel.  bf16 keeps fp32's exponent range: no loss scaling is needed.  Both kernels are free of atomics: two runs give the same bits, and an
 * image's data gradient does not depend on how many images the launch has.  Parity with the reference's fp32 gradients is claimed only in the default mode
 * (error against fp64 autograd under the mode: below torch.autocast(bfloat16)'s on every parameter, tests/test_gpu_grad_bf16.py). */
#define LFSR_GRAD_ARITH_DEFAULT 0
#define LFSR_GRAD_ARITH_BF16 1
int lfsr_set_grad_arithmetic(int mode);   /* LFSR_E_ARG for any other value, nothing changed */
int lfsr_get_grad_arithmetic(void);

/* ---- arithmetic of the transformers' GEMMs: a third process-wide selection, independent of the two above, read at every launch ----
 * LFSR_GEMM_ARITH_DEFAULT: every kernel as it is, bit for bit.
 * LFSR_GEMM_ARITH_BF16: opt-in.  Three operators round their activations and weights to bf16 (nearest even) where they run on the three-term form by default; the
 * products are exact, and accumulation, LayerNorm, ReLU / slope, residual adds and stores are fp32 (activations stay fp32 in memory):
 *  - the bias-free linear of lfsr_linear_fwd / lfsr_pointwise_fwd with K in {64, 128}, N in {64, 128, 256} and at least 2048 rows;
 *  - LayerNorm (+ position encoding) + q | k | v projection, lfsr_linear_ln_fwd, at (K, N) = (128, 384) and (64, 192);
 *  - the feed-forward block, lfsr_ffn_fwd / lfsr_ffn_ln_fwd, at (K1, H, N2) = (128, 256, 128) and (64, 128, 64).
 * Every other shape, unaligned operands and spans of 2 GiB or more run exactly as under the default.  LFSR_ARITH_F32 wins over this mode.  What follows: the forward
 * and forward_train of lfsr_epit_* and lfsr_lft_*, LF_InterNet's 128 -> 64 angular squeeze, and the training backward's recomputation of the feed-forward hidden
 * rows (so that it equals what the forward computed).  What does not: K = 144 (DistgSSR's fuse.0, hence all of DistgSSR, which has its own switch: lfsr_set_branch_arithmetic below), linears below 2048 rows, biased linears,
 * the attention kernels, the up-sampling tail, the 3x3 convs and every gradient kernel.  No atomics: two runs give the same bits and a row's result does not depend
 * on the number of rows.  Parity with the reference's fp32 results is claimed only in the default mode (error against fp64 under the mode: below
 * torch.autocast(bfloat16)'s, tests/test_gpu_gemm_bf16.py). */
#define LFSR_GEMM_ARITH_DEFAULT 0
#define LFSR_GEMM_ARITH_BF16 1
int lfsr_set_gemm_arithmetic(int mode);   /* LFSR_E_ARG for any other value, nothing changed */
int lfsr_get_gemm_arithmetic(void);

/* ---- arithmetic of DistgSSR's EPI branch and block tail: a fourth process-wide selection, independent of the three above, read at every launch ----
 * LFSR_BRANCH_ARITH_DEFAULT: every kernel as it is, bit for bit.
 * LFSR_BRANCH_ARITH_BF16: opt-in.  Where the DistgSSR forward at angRes 5 runs its fused block tail (stage 1 of the branches, then AngConv.2, EPIConv.2 of both
 * passes, the concat and fuse.0 in one launch), three GEMMs round their operands to bf16 (nearest even) once instead of carrying them as three bf16 terms:
 *  - EPIConv.0 of both passes: x and the weight;
 *  - EPIConv.2 of both passes: the fp32 post-LeakyReLU stage-1 results as they lie in memory, and the weight;
 *  - fuse.0: all 144 concat channels (the SpaConv.2 rows, the post-LeakyReLU AngConv.2 and EPIConv.2 results) and the weight.
 * The products are exact; accumulation, LeakyReLU and stores are fp32; every intermediate stays fp32 in memory; the weights are rounded from their fp32 packs
 * while a block stages them, so the packs, lfsr_distgssr_packed_bytes and the workspace do not change.  AngConv.0 and AngConv.2 keep their fp32-MFMA
 * arithmetic.  What follows: lfsr_distgssr_forward (and _taps) and the operator lfsr_distg_branch_tail_fwd.  What does not, with its bits unchanged:
 * LFSR_ARITH_F32 (which wins), angRes other than 5, inputs of fewer than 2048 pixels, block (0,0) when the concat tap is requested, the LFSR_LAB selectors,
 * lfsr_distgssr_forward_train and every backward kernel (the training forward keeps the three-kernel sequence whose intermediates the backward reads: training
 * under the mode is not its aim; the branch backward has its own switch, lfsr_set_branch_grad_arithmetic below), and EPIT, LFT and LF_InterNet.  No atomics: two runs give the same bits, and a macro-pixel's result depends neither on B nor on
 * the grid.  Parity with the reference's fp32 results is claimed only in the default mode (error against fp64 under the mode: below
 * torch.autocast(bfloat16)'s, tests/test_gpu_branch_bf16.py). */
#define LFSR_BRANCH_ARITH_DEFAULT 0
#define LFSR_BRANCH_ARITH_BF16 1
int lfsr_set_branch_arithmetic(int mode);   /* LFSR_E_ARG for any other value, nothing changed */
int lfsr_get_branch_arithmetic(void);

/* ---- arithmetic of LFSSR's angular conv: a fifth process-wide selection, independent of the four above, read at every launch ----
 * LFSR_ANG_ARITH_DEFAULT: every kernel as it is, bit for bit.
 * LFSR_ANG_ARITH_BF16: opt-in.  lfsr_angconv3x3_fwd rounds its operands to bf16 (nearest even) once: the activations after the optional in_bias + ReLU prologue
 * (which stays one fp32 add and one max), and the weight from its fp32 pack while a wave loads it, so the pack, lfsr_lfssr_packed_bytes and the workspace do not
 * change.  The products are exact; accumulation, bias, ReLU and stores are fp32; x and y stay fp32 in memory; off-grid taps are skipped as under the default.  The
 * geometries, argument checks and return codes are the default's (angRes 2..9, any npix, strides and channel offsets).  What follows: lfsr_angconv3x3_fwd and,
 * through it, the angular convs of lfsr_lfssr_forward (n_layer per level: twenty at scale 4).  What does not, with its bits unchanged: LFSR_ARITH_F32 (which wins), LFSSR's per-view
 * convs (they follow lfsr_set_arithmetic), the fused up-sampling tail, DistgSSR's AngConv (a different operator), and EPIT, LFT and LF_InterNet.  No atomics: taps
 * and channels run in one fixed order, two runs give the same bits, and a sample's result depends neither on B nor on the grid.  Parity with the reference's fp32
 * results is claimed only in the default mode (error against fp64 under the mode: below torch.autocast(bfloat16)'s, tests/test_gpu_ang_bf16.py). */
#define LFSR_ANG_ARITH_DEFAULT 0
#define LFSR_ANG_ARITH_BF16 1
int lfsr_set_ang_arithmetic(int mode);   /* LFSR_E_ARG for any other value, nothing changed */
int lfsr_get_ang_arithmetic(void);

/* ---- arithmetic of LF_InterNet's wide per-view 3x3 convs: a sixth process-wide selection, independent of the five above, read at every launch ----
 * LFSR_WIDE_ARITH_DEFAULT: every kernel as it is, bit for bit.
 * LFSR_WIDE_ARITH_BF16: opt-in.  lfsr_conv3x3_wide_fwd (below) rounds its activations and its weight to bf16 (nearest even) once, the weight from its fp32 pack
 * while a block stages it, so the pack, lfsr_internet_packed_bytes and the workspace do not change.  The products are exact; accumulation, LeakyReLU, the
 * residual add and stores are fp32; x, r1 and y stay fp32 in memory.  The argument checks and return codes are the default's.  What follows: lfsr_conv3x3_wide_fwd
 * and, through its launcher, the sixteen SpaConvSq (128 -> 64) and the SpaBottle (320 -> 64) of lfsr_internet_forward: 82 % of that forward's arithmetic.  What
 * does not, with its bits unchanged: LFSR_ARITH_F32 (which wins), lfsr_internet_forward_train and lfsr_internet_backward (the training forward does not read
 * this switch: a training step is the same in either mode; training has its own, lfsr_set_wide_train_arithmetic below), LF_InterNet's other operators (its 128 -> 64 angular squeeze follows
 * lfsr_set_gemm_arithmetic), lfsr_conv3x3_fwd, lfsr_conv3x3_n_fwd, lfsr_angconv3x3_fwd, and DistgSSR, EPIT, LFT and LFSSR.  No atomics: chunks, taps and channels
 * run in one fixed order, two runs give the same bits, and an image's result does not depend on n_img.  Parity with the reference's fp32 results is claimed only
 * in the default mode (error against fp64 under the mode: below torch.autocast(bfloat16)'s, tests/test_gpu_wide_bf16.py). */
#define LFSR_WIDE_ARITH_DEFAULT 0
#define LFSR_WIDE_ARITH_BF16 1
int lfsr_set_wide_arithmetic(int mode);   /* LFSR_E_ARG for any other value, nothing changed */
int lfsr_get_wide_arithmetic(void);
/* The wide per-view 3x3 conv of LF_InterNet (SpaConvSq, LF_InterNet.py:64; BottleNeck.SpaBottle, :122): zero pad 1, cin in {128, 320} -> 64 channels, on the VCL
 * rows of n_img view images of h x w:  y = LeakyReLU_slope(conv(x)) + r1   (slope 0: ReLU, 1: identity; r1 may be NULL).
 * w_packed: lfsr_pack_conv_weight(w, packed, 64, cin, 9, 0, 0), [9][64][cin] fp32.  r1 may alias x (the model passes the first 64 channels of the same rows);
 * y must not overlap x.  LFSR_E_ARG before any launch, nothing written, in both arithmetics: NULL x / w_packed / y, cin outside {128, 320}, non-positive n_img /
 * h / w, x_stride < x_choff + cin, y_stride < y_choff + 64 (r1 likewise when given), a negative stride or offset or one that is no multiple of 4, a pointer off
 * the 16-byte grid, an operand span (n_img h w stride floats) of 2 GiB or more.  Then the switch above selects the kernel: the gather-GEMM on the fp32 MFMA
 * pipe (default, and under LFSR_ARITH_F32), or csrc/conv3x3_wide_bf16.hip. */
int lfsr_conv3x3_wide_fwd(const float* x, int x_stride, int x_choff, int cin, const float* w_packed,
                          float* y, int y_stride, int y_choff,
                          const float* r1, int r1_stride, int r1_choff,
                          int n_img, int h, int w, float slope, void* stream);

/* ---- arithmetic of the linears' GRADIENTS (the transformers' GEMM gradients): a seventh process-wide selection, independent of the six above, read at every launch ----
 * LFSR_LIN_GRAD_ARITH_DEFAULT: every gradient kernel as it is, bit for bit.
 * LFSR_LIN_GRAD_ARITH_BF16: opt-in, what LFSR_GRAD_ARITH_BF16 leaves out.  Two operators change:
 *  - the weight gradient of a linear, lfsr_linear_wgrad (below) and LfsrTransBwd::wgrad_lin inside the drivers: dy and x are rounded to bf16 (nearest even) on their
 *    way into LDS, the products are exact (v_mfma_f32_32x32x16_bf16, the row index as the MFMA's K), accumulation is fp32 into per-block partial slabs, and the same
 *    fixed-order reduction sums them -- one launch and one reduction per linear, where the default runs one of each per 64 output rows
 *    (csrc/lin_wgrad_bf16.hip: how often dy and x are read);
 *  - the data gradient of a linear, lfsr_linear_dgrad and LfsrTransBwd::dgemm: dy and the transposed weight (from the fp32 pack, while a block stages it: no new
 *    pack, no new workspace) are rounded to bf16 once, the products are exact, accumulation is fp32, and the act > 0 mask and the r1 add are fp32 after the
 *    accumulation (csrc/lin_dgrad_bf16.hip).  Every shape the entry point accepts, r1 == dx, columns [0, cin) only; the argument checks and return codes are the
 *    default's; an operand pointer off the 16-byte grid runs the default kernel.
 * What follows: lfsr_epit_backward and lfsr_lft_backward, in every linear of their sublayers (feed_forward.1 / .4, out_proj, in_proj), EPIT's linear_in /
 * linear_out, LFT's linear.0 and upsampling.0.  What does not, with its bits unchanged: the forwards and forward_train (they read no gradient switch), the
 * recomputation inside the backward, the attention and LayerNorm backward, every 3x3 conv gradient (the conv_init stack, LFT's position 3x3, the tail's 3x3: the
 * generic weight-gradient kernel and lfsr_set_grad_arithmetic), lfsr_pointwise_dgrad / lfsr_pointwise_wgrad, and DistgSSR, LF_InterNet and LFSSR.  It does not
 * interact with lfsr_set_arithmetic: no "F32 wins" rule, as for the grad switch.  lfsr_linear_wgrad_workspace_floats and lfsr_*_train_workspace_bytes do not depend
 * on the mode.  Gradients, activations and slabs stay fp32 in memory; bf16 keeps fp32's exponent range: no loss scaling is needed.  Both kernels are free of
 * atomics: two runs give the same bits, and a row's data gradient does not depend on M.  Parity with the reference's fp32 gradients is claimed only in the default
 * mode (error against fp64 autograd under the mode: tests/test_gpu_lin_grad_bf16.py). */
#define LFSR_LIN_GRAD_ARITH_DEFAULT 0
#define LFSR_LIN_GRAD_ARITH_BF16 1
int lfsr_set_lin_grad_arithmetic(int mode);   /* LFSR_E_ARG for any other value, nothing changed */
int lfsr_get_lin_grad_arithmetic(void);
/* Weight gradient of nn.Linear y = x W^T, W (cout, cin):  dw[n][k] (=, or += if accumulate) sum over m < M of dy[m][n] x[m][k], dw in the raw (cout, cin) layout.
 * cout in {64,128,256,576,1024}, cin in {64,128,256}; dy / x: rows of cout / cin floats at row strides that are multiples of 4 and at least the row width;
 * dy, x, dw, workspace 16-byte aligned; 0 < M < 2^31 - 128.  workspace: lfsr_linear_wgrad_workspace_floats(M, cout, cin) floats of partial slabs (0 for a
 * refused shape; the same in both modes).  LFSR_E_ARG / LFSR_E_WS before any launch, nothing written.  Then the switch above selects the kernels.  Default: what the
 * drivers run, a loop over the 64-row slices of W through the generic gather weight-gradient kernel and its reduction -- the bits of lfsr_pointwise_wgrad called per
 * slice with dy_choff = n0.  LFSR_LIN_GRAD_ARITH_BF16: csrc/lin_wgrad_bf16.hip and one reduction.  No float atomics in either: two runs give the same bits. */
size_t lfsr_linear_wgrad_workspace_floats(long long M, int cout, int cin);
int lfsr_linear_wgrad(const float* dy, int dy_stride, const float* x, int x_stride, float* dw, float* workspace, size_t workspace_floats, long long M, int cout,
                      int cin, int accumulate, void* stream);

/* ---- arithmetic of LF_InterNet's wide per-view 3x3 convs IN TRAINING: an eighth process-wide selection, independent of the seven above, read at every launch ----
 * LFSR_WIDE_TRAIN_ARITH_DEFAULT: every kernel as it is, bit for bit.
 * LFSR_WIDE_TRAIN_ARITH_BF16_WGRAD: opt-in.  The weight gradient of the wide convs (SpaConvSq 128 -> 64, BottleNeck.SpaBottle 320 -> 64), lfsr_conv3x3_wide_wgrad
 * (below), rounds dy and x to bf16 (nearest even) on their way into LDS; the products are exact (v_mfma_f32_32x32x16_bf16, the pixel index as the MFMA's K),
 * accumulation is fp32 into per-block partial slabs, and the fixed-order reduction of the default sums them (csrc/wgrad_wide_bf16.hip: the dy tile is staged once
 * for every 64-channel chunk of x a block owns).  forward_train as it is.
 * LFSR_WIDE_TRAIN_ARITH_BF16: that, and lfsr_internet_forward_train computes ReLU(SpaConvSq) and ReLU(SpaBottle) with the kernel of LFSR_WIDE_ARITH_BF16
 * (csrc/conv3x3_wide_bf16.hip); the residual add stays the separate fp32 launch, so the output equals lfsr_internet_forward's under LFSR_WIDE_ARITH_BF16 bit for bit.
 * What follows: lfsr_conv3x3_wide_wgrad, the seventeen wide weight gradients of lfsr_internet_backward (modes 1 and 2) and the seventeen wide convs of
 * lfsr_internet_forward_train (mode 2).  What does not, with its bits unchanged: the wide convs' data gradients (64 -> 64 calls that follow
 * lfsr_set_grad_arithmetic alone), every other operator of the LF_InterNet training step, lfsr_internet_forward and lfsr_conv3x3_wide_fwd (they follow
 * lfsr_set_wide_arithmetic, which in turn does not reach training), spans of 2 GiB or more (the default kernel), and DistgSSR, EPIT, LFT and LFSSR (LFT's 64 -> 64
 * position conv runs the same generic weight-gradient kernel and does not read this switch).  LFSR_ARITH_F32 wins for the forward half of mode 2 and has no
 * bearing on the weight gradients, as for the other gradient switches.  lfsr_conv3x3_wide_wgrad_workspace_floats and lfsr_internet_train_workspace_bytes do not
 * depend on the mode.  Gradients, activations and slabs stay fp32 in memory; bf16 keeps fp32's exponent range: no loss scaling is needed.  No atomics: slab order
 * and block count are fixed by the geometry alone, two runs give the same bits.  Parity with the reference's fp32 gradients is claimed only in the default mode
 * (error against fp64 autograd under the modes: below torch.autocast(bfloat16)'s, tests/test_gpu_wide_train_bf16.py). */
#define LFSR_WIDE_TRAIN_ARITH_DEFAULT 0
#define LFSR_WIDE_TRAIN_ARITH_BF16_WGRAD 1
#define LFSR_WIDE_TRAIN_ARITH_BF16 2
int lfsr_set_wide_train_arithmetic(int mode);   /* LFSR_E_ARG for any other value, nothing changed */
int lfsr_get_wide_train_arithmetic(void);
/* Weight gradient of the wide per-view 3x3 conv (zero pad 1, cin in {128, 320} -> 64):  dw[n][k][tap] (=, or += if accumulate) the sum over the pixels p of the
 * n_img views of dy[p][n] x[p + shift(tap)][k], zero outside the view; dw (64, cin, 3, 3) in the raw PyTorch layout, dy and x VCL rows.  workspace:
 * lfsr_conv3x3_wide_wgrad_workspace_floats(cin, n_img, h, w) floats of partial slabs (0 for a refused shape; the same in every mode).  LFSR_E_ARG before any launch,
 * nothing written, in every mode: NULL dy / x / dw / workspace, cin outside {128, 320}, non-positive n_img / h / w, x_stride < x_choff + cin,
 * dy_stride < dy_choff + 64, a negative stride or offset or one that is no multiple of 4, dy, x, dw or workspace off the 16-byte grid, an operand span
 * (n_img h w stride floats) of 2 GiB or more; LFSR_E_WS for a short workspace.  Then the switch above selects the kernel.  Default: what lfsr_internet_backward
 * has always run, the generic gather weight-gradient kernel over (row splits, 9 taps, cin / 64 column tiles) and its reduction.  Modes 1 and 2:
 * csrc/wgrad_wide_bf16.hip and the same reduction.  No float atomics in either: two runs give the same bits. */
size_t lfsr_conv3x3_wide_wgrad_workspace_floats(int cin, int n_img, int h, int w);
int lfsr_conv3x3_wide_wgrad(const float* dy, int dy_stride, int dy_choff, const float* x, int x_stride, int x_choff, int cin,
                            float* dw, float* workspace, size_t workspace_floats, int n_img, int h, int w, int accumulate, void* stream);

/* ---- arithmetic of EPIConv.0's GRADIENTS (DistgSSR's disentangling branch in training): a ninth process-wide selection, independent of the eight above, read at every
 * launch ----
 * LFSR_BRANCH_GRAD_ARITH_DEFAULT: every kernel as it is, bit for bit.
 * LFSR_BRANCH_GRAD_ARITH_BF16: opt-in, the training counterpart of lfsr_set_branch_arithmetic.  The two EPI-line gradient kernels of EPIConv.0 (1 x A^2, stride A,
 * 64 -> 32, shared by the horizontal and the vertical pass) run on bf16 operands (csrc/epi0_grad_bf16.hip):
 *  - the weight gradient: dE and the input slab of an EPI line are rounded to bf16 (nearest even) on their way into LDS, the products are exact
 *    (v_mfma_f32_16x16x32_bf16, the pixel index as the MFMA's K), accumulation is fp32 into one partial slab per block, and the fixed-order reduction of the default
 *    sums the same number of slabs;
 *  - the data gradient: dE and the weights (from the fp32 direct pack, while a block stages them: no new pack, no new workspace) are rounded to bf16, the products are
 *    exact, accumulation is fp32 and the read-modify-write of dx stays fp32.
 * They are taken exactly where the fp32 EPI-line kernels are taken: A = 5, the pass's line length <= 32 (the merged weight gradient: h and w both <= 32), the operand
 * span below 2 GiB.  Everywhere else the call runs what it runs in the default mode, bit for bit.  The LFSR_LAB selectors LFSR_WGRAD_EPI=gather and
 * LFSR_DGRAD_EPI=gather still win.
 * What follows: lfsr_epiconv_hv_bwd and lfsr_distgssr_backward (one-stream and two-stream order alike).  What does not, with its bits unchanged: every forward and
 * forward_train, lfsr_angconv_bwd, stage 2 of the EPI branch (dE, dw2), fuse.0's gradients, the 3x3 convs (lfsr_set_grad_arithmetic), and EPIT, LFT, LF_InterNet and
 * LFSSR.  It does not interact with lfsr_set_arithmetic: no "F32 wins" rule, as for the grad switch.  lfsr_epiconv_hv_bwd_workspace_floats and
 * lfsr_distgssr_train_workspace_bytes do not depend on the mode.  Gradients, activations and slabs stay fp32 in memory; bf16 keeps fp32's exponent range: no loss
 * scaling is needed.  No atomics: two runs give the same bits, and a sample's data gradient does not depend on B.  Parity with the reference's fp32 gradients is
 * claimed only in the default mode (error against fp64 autograd under the mode: below torch.autocast(bfloat16)'s, tests/test_gpu_branch_grad_bf16.py). */
#define LFSR_BRANCH_GRAD_ARITH_DEFAULT 0
#define LFSR_BRANCH_GRAD_ARITH_BF16 1
int lfsr_set_branch_grad_arithmetic(int mode);   /* LFSR_E_ARG for any other value, nothing changed */
int lfsr_get_branch_grad_arithmetic(void);

/* ---- operator-level timing hooks (measurement aid; the reference times whole forwards only: check_efficiency_official.py:306-330) ----
 * lfsr_op_profile(1): from now on every instrumented operator entry point brackets its launches with a hipEvent pair on its launch stream (and any
 * earlier records are dropped); lfsr_op_profile(0): off (the default; a hook then costs one atomic load).  lfsr_op_profile_read waits for the recorded
 * events, writes one text line "op a b total_ms launches" per (operator, tag a, tag b) into buf (NUL-terminated, truncated to cap), clears the records and
 * returns the bytes the full text needs, or a negative LFSR_E_* / HIP code.  Tags: conv3x3 / conv3x3_dgrad / conv3x3_wgrad (n_img, h*w), linear (K, N),
 * window_attn (head dim, tokens per sequence), ffn (K, hidden), up_tail (scale, 0), epiconv / angconv / pointwise (cin, N). */
int lfsr_op_profile(int enable);
long long lfsr_op_profile_read(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LFSR_HIP_H */
