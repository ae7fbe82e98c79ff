// The small operators of the LFSSR forward (model/SR/LFSSR.py:50-176) around its two 64 -> 64 convs: conv0 (1 -> 64 from the SAI mosaic), the up-sampling conv
// 64 -> 256 + PixelShuffle(2) + ReLU (four 64 -> 64 convs on the 3x3 dispatcher, then one scatter), and the tail res + iup (64 -> 1 and 1 -> 4 + PixelShuffle(2)).
// All per view with zero padding 1, all with biases.  The kernels here run on the VALU in one arithmetic and read none of the four arithmetic switches; the four
// convs of lfsr_conv3x3_ps2_fwd go through lfsr_conv3x3_run and follow lfsr_set_arithmetic like every other 64 -> 64 3x3 conv.
#include "lfssr_ctx.h"

namespace {

// conv0 + bias + ReLU: 16 threads per pixel, 4 output channels each; x is the SAI mosaic (B, 1, A h, A w)
__global__ __launch_bounds__(256) void k_lfssr_conv0(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ y,
                                                    int ys, int yo, int B, int A, int h, int wd) {
  __shared__ float sw[9 * 64 + 64];   // [tap][channel], then the bias
  for (int i = threadIdx.x; i < 576; i += 256) sw[(i % 9) * 64 + i / 9] = w[i];
  for (int i = threadIdx.x; i < 64; i += 256) sw[576 + i] = bias[i];
  __syncthreads();
  const long long npix = (long long)B * A * A * h * wd;
  const int Wm = A * wd;
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < npix * 16; g += (long long)gridDim.x * 256) {
    const long long pix = g >> 4;
    const int c4 = (int)(g & 15) * 4;
    const int xx = (int)(pix % wd);
    long long t = pix / wd;
    const int yy = (int)(t % h);
    t /= h;
    const int v = (int)(t % A);
    t /= A;
    const int u = (int)(t % A), b = (int)(t / A);
    const float* img = x + ((long long)b * A * h + (long long)u * h) * Wm + (long long)v * wd;
    float a0 = sw[576 + c4], a1 = sw[577 + c4], a2 = sw[578 + c4], a3 = sw[579 + c4];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int sy = yy + tap / 3 - 1, sx = xx + tap % 3 - 1;
      if (sy < 0 || sy >= h || sx < 0 || sx >= wd) continue;
      const float xv = img[(long long)sy * Wm + sx];
      a0 = fmaf(xv, sw[tap * 64 + c4], a0); a1 = fmaf(xv, sw[tap * 64 + c4 + 1], a1);
      a2 = fmaf(xv, sw[tap * 64 + c4 + 2], a2); a3 = fmaf(xv, sw[tap * 64 + c4 + 3], a3);
    }
    *reinterpret_cast<float4*>(y + pix * ys + yo + c4) = make_float4(fmaxf(a0, 0.f), fmaxf(a1, 0.f), fmaxf(a2, 0.f), fmaxf(a3, 0.f));
  }
}

// PixelShuffle(2) + bias + ReLU: t (rows, 256), column 64 (2 i + j) + c = the reference's conv channel 4 c + 2 i + j  ->  y[(img, 2 yy + i, 2 xx + j), c]
__global__ __launch_bounds__(256) void k_lfssr_ps2(const float* __restrict__ t, const float* __restrict__ bias, float* __restrict__ y, int ys, int yo,
                                                  long long rows, int h, int wd) {
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < rows * 64; g += (long long)gridDim.x * 256) {
    const long long p = g >> 6;
    const int ij = (int)(g >> 4) & 3, c4 = (int)(g & 15) * 4;
    const int xx = (int)(p % wd);
    const long long q = p / wd;
    const int yy = (int)(q % h);
    const long long img = q / h;
    const float4 v = *reinterpret_cast<const float4*>(t + p * 256 + 64 * ij + c4);
    const long long o = (img * 2 * h + 2 * yy + (ij >> 1)) * (2 * wd) + 2 * xx + (ij & 1);
    *reinterpret_cast<float4*>(y + o * ys + yo + c4) =
        make_float4(fmaxf(v.x + bias[4 * c4 + ij], 0.f), fmaxf(v.y + bias[4 * c4 + 4 + ij], 0.f), fmaxf(v.z + bias[4 * c4 + 8 + ij], 0.f),
                    fmaxf(v.w + bias[4 * c4 + 12 + ij], 0.f));
  }
}

// out = conv3x3_{64 -> 1}(f) + b_res + PS2(conv3x3_{1 -> 4}(lo) + b_iup): 16 lanes per output pixel, 4 channels of the 9 taps each, summed over the
// 16 lanes in a fixed butterfly.  H, W: the output view (= the view of f); lo: planes of (H / 2, W / 2).
__global__ __launch_bounds__(256) void k_lfssr_tail(const float* __restrict__ f, int fs, int fo, const float* __restrict__ w_res, const float* __restrict__ b_res,
                                                   const float* __restrict__ lo, const float* __restrict__ w_iup, const float* __restrict__ b_iup,
                                                   float* __restrict__ out, int B, int A, int H, int W, int mosaic) {
  __shared__ float sw[9 * 64 + 36 + 5];   // res [tap][channel]; iup [ij][tap]; b_iup[4], b_res
  for (int i = threadIdx.x; i < 576; i += 256) sw[(i % 9) * 64 + i / 9] = w_res[i];
  for (int i = threadIdx.x; i < 36; i += 256) sw[576 + i] = w_iup[i];
  if (threadIdx.x < 4) sw[612 + threadIdx.x] = b_iup[threadIdx.x];
  if (threadIdx.x == 4) sw[616] = b_res[0];
  __syncthreads();
  const long long npix = (long long)B * A * A * H * W;
  const int h = H / 2, wd = W / 2;
  const long long total = (npix * 16 + 255) / 256 * 256;     // whole groups of 16 lanes take part in the butterfly
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
    const long long pix = g >> 4;
    const bool live = pix < npix;
    const int c4 = (int)(g & 15) * 4;
    const int X = (int)(pix % W);
    const long long t = pix / W;
    const int Y = (int)(t % H);
    const long long img = t / H;
    float s = 0.f;
    if (live) {
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int sy = Y + tap / 3 - 1, sx = X + tap % 3 - 1;
        if (sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
        const float4 v = *reinterpret_cast<const float4*>(f + ((img * H + sy) * W + sx) * fs + fo + c4);
        s = fmaf(v.x, sw[tap * 64 + c4], s); s = fmaf(v.y, sw[tap * 64 + c4 + 1], s);
        s = fmaf(v.z, sw[tap * 64 + c4 + 2], s); s = fmaf(v.w, sw[tap * 64 + c4 + 3], s);
      }
    }
    s += __shfl_xor(s, 1, 16); s += __shfl_xor(s, 2, 16); s += __shfl_xor(s, 4, 16); s += __shfl_xor(s, 8, 16);
    if (!live || (g & 15)) continue;
    const int ij = (Y & 1) * 2 + (X & 1), yy = Y >> 1, xx = X >> 1;
    float up = sw[612 + ij];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int sy = yy + tap / 3 - 1, sx = xx + tap % 3 - 1;
      if (sy < 0 || sy >= h || sx < 0 || sx >= wd) continue;
      up = fmaf(lo[(img * h + sy) * wd + sx], sw[576 + ij * 9 + tap], up);
    }
    const float r = s + sw[616] + up;
    if (!mosaic) {
      out[pix] = r;
    } else {
      const int v = (int)(img % A), u = (int)((img / A) % A);
      const long long b = img / (A * A);
      out[((b * A + u) * H + Y) * ((long long)A * W) + (long long)v * W + X] = r;
    }
  }
}

// rows c * 4 + ij of the reference's (256, 64, 3, 3) weight -> four contiguous (64, 64, 3, 3) weights, one per sub-pixel ij = 2 i + j
__global__ void k_lfssr_split4(const float* __restrict__ w, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 4 * 64 * 576) return;
  const int r = i % 576, c = (i / 576) % 64, ij = i / (576 * 64);
  out[i] = w[(size_t)(c * 4 + ij) * 576 + r];
}

}  // namespace

int lfsr_lfssr_split4(const float* w_raw, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_lfssr_split4, dim3((4 * 64 * 576 + 255) / 256), dim3(256), 0, st, w_raw, out);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

extern "C" {

int lfsr_lfssr_conv0_fwd(const float* x, const float* w, const float* bias, float* y, int y_stride, int y_choff, int B, int A, int h, int wd, void* stream) {
  if (!x || !w || !bias || !y || B <= 0 || A <= 0 || h <= 0 || wd <= 0) return LFSR_E_ARG;
  if (y_choff < 0 || y_stride < y_choff + 64 || ((y_stride | y_choff) & 3) || ((uintptr_t)y & 15)) return LFSR_E_ARG;
  const long long npix = (long long)B * A * A * h * wd;
  if (npix * y_stride >= (1LL << 31) / 4) return LFSR_E_ARG;
  hipLaunchKernelGGL(k_lfssr_conv0, dim3(lfsr_cap_grid(npix * 16)), dim3(256), 0, lfsr_stream(stream), x, w, bias, y, y_stride, y_choff, B, A, h, wd);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

int lfsr_conv3x3_ps2_fwd(const float* x, int x_stride, int x_choff, const float* w_packed4, const float* bias, float* tmp, float* y, int y_stride, int y_choff,
                         int n_img, int h, int w, void* stream) {
  if (!x || !w_packed4 || !bias || !tmp || !y || n_img <= 0 || h <= 0 || w <= 0) return LFSR_E_ARG;
  if (x_choff < 0 || y_choff < 0 || x_stride < x_choff + 64 || y_stride < y_choff + 64 || ((x_stride | x_choff | y_stride | y_choff) & 3)) return LFSR_E_ARG;
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)tmp | (uintptr_t)w_packed4) & 15) return LFSR_E_ARG;
  const long long rows = (long long)n_img * h * w;
  if (rows * 256 >= (1LL << 31) / 4 || rows * x_stride >= (1LL << 31) / 4 || rows * 4 * y_stride >= (1LL << 31) / 4) return LFSR_E_ARG;
  hipStream_t st = lfsr_stream(stream);
  const size_t pack = lfsr_packed_weight_floats(64, 64, 9);
  for (int ij = 0; ij < 4; ++ij) {
    LfsrConv3 c{};
    c.x = x; c.x_stride = x_stride; c.x_choff = x_choff; c.w_packed = w_packed4 + ij * pack; c.y = tmp; c.y_stride = 256; c.y_choff = 64 * ij;
    c.mk_slope = 1.0f; c.n_img = n_img; c.h = h; c.w = w; c.slope = 1.0f;
    LFSR_RC(lfsr_conv3x3_run(c, false, st));
  }
  hipLaunchKernelGGL(k_lfssr_ps2, dim3(lfsr_cap_grid(rows * 64)), dim3(256), 0, st, tmp, bias, y, y_stride, y_choff, rows, h, w);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

int lfsr_lfssr_tail_fwd(const float* f, int f_stride, int f_choff, const float* w_res, const float* b_res, const float* lo, const float* w_iup, const float* b_iup,
                        float* out, int B, int A, int h, int w, int mosaic, void* stream) {
  if (!f || !w_res || !b_res || !lo || !w_iup || !b_iup || !out || B <= 0 || A <= 0 || h <= 0 || w <= 0 || (mosaic != 0 && mosaic != 1)) return LFSR_E_ARG;
  if (f_choff < 0 || f_stride < f_choff + 64 || ((f_stride | f_choff) & 3) || ((uintptr_t)f & 15)) return LFSR_E_ARG;
  const long long npix = (long long)B * A * A * h * w * 4;
  if (npix * f_stride >= (1LL << 31) / 4) return LFSR_E_ARG;
  hipLaunchKernelGGL(k_lfssr_tail, dim3(lfsr_cap_grid(npix * 16)), dim3(256), 0, lfsr_stream(stream), f, f_stride, f_choff, w_res, b_res, lo, w_iup, b_iup, out,
                     B, A, 2 * h, 2 * w, mosaic);
  LFSR_CHECK_LAUNCH();
  return LFSR_OK;
}

}  // extern "C"
