// The data gradient of lfsr_set_grad_arithmetic(LFSR_GRAD_ARITH_BF16): dx = conv^T(dy) * (mk > 0 ? 1 : mk_slope) + r1 + r2 on bf16-rounded dy and weights (the
// transposed, tap-flipped pack), fp32 accumulation.  The kernel is conv3x3_bf16_kernel.h's with the mask operand; a call without a mask is the forward's instantiation.
#include "conv3x3_bf16_kernel.h"

int lfsr_conv3x3_bf16_dgrad_launch(const LfsrConv3& c, hipStream_t st) {
  return c.mk ? conv3x3_bf16_launch_t<true>(c, st) : lfsr_conv3x3_bf16_launch(c, st);
}
