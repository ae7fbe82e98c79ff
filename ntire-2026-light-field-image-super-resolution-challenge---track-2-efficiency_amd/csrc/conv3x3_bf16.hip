// The forward of lfsr_set_arithmetic(LFSR_ARITH_BF16): the 64 -> 64 per-view 3x3 conv on bf16 operands, without the gradient's mask operand.  The kernel and its
// description are in conv3x3_bf16_kernel.h; the gradient form is instantiated in conv3x3_bf16_dgrad.hip.
#include "conv3x3_bf16_kernel.h"

int lfsr_conv3x3_bf16_launch(const LfsrConv3& c, hipStream_t st) { return conv3x3_bf16_launch_t<false>(c, st); }
