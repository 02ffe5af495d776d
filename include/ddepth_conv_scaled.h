/*
 * ddepth_conv_scaled.h -- the two gradients of the training convolutions of ddepth_conv.h with a power-of-two rescale of grad_y (same shared
 * library; kernels in diffusiondepth_amd/csrc/dd_conv.hip).  Opt-in: nothing in ddepth_conv.h changes, and nothing here is called unless asked for.
 *
 * Why: the kernels of ddepth_conv.h turn grad_y into an MFMA operand by rounding it as it arrives, f16(v) (and f16(v - hi) in the split mode).
 * A training step hands these layers gradients of about 3e-7 -- the loss is a mean over millions of pixels -- and f16 goes subnormal below
 * 6.1e-5 and flushes to zero below 6e-8; above 65504 it is Inf.  Here grad_y is multiplied by a power of two s on its way into the operand and
 * the result by 1 / s on its way out, so the rounding happens where f16 has its 11 bits.  bf16 has fp32's exponent range and needs none of this.
 *
 * The rule (the tests compute it themselves):
 *     amax = the largest FINITE |grad_y[i]|
 *     s    = 2^(14 - floor(log2 amax)), built from amax's exponent field; the shift is held to +-126, so s and 1 / s are normal fp32
 *     amax == 0 gives s = 1.  NaN and Inf elements take no part in amax and travel through the kernels as they are.
 * 14 is derived, not measured: the largest exponent with s * amax < 2^15 <= 65504.  One GEMM accumulates in fp32, so nothing behind the
 * operand can overflow, and every bit of headroom not needed at the top is range gained at the bottom: in the split mode the lo half goes
 * subnormal below |s v| = 2^-3, so a lower exponent gives the split up for most of a heavy-tailed gradient.
 * Both factors are powers of two: a gradient 2^k times another gives exactly 2^k times the result (short of fp32's own range).
 *
 * Conventions: those of ddepth_conv.h -- DEVICE pointers, contiguous fp32 NCHW, asynchronous on `stream`, no host synchronisation, allocation or
 * host read of device memory; DD_OK or a dd_status code with the message in dd_conv_last_error().  Bitwise reproducible: the reduction is an
 * integer maximum, the accumulation order of the kernels is that of ddepth_conv.h.
 */
#ifndef DDEPTH_CONV_SCALED_H_
#define DDEPTH_CONV_SCALED_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* scale: a caller-owned device buffer of 4 floats (16 bytes); receives {s, 1 / s, the bits of amax, unused (0)} for the n elements of grad_y.
 * The buffer is zeroed, one pass over grad_y takes the maximum, one single-thread kernel writes the pair.  precision: a dd_precision value of
 * ddepth_conv.h; DD_PREC_BF16 writes {1, 1} and launches no reduction.  n >= 0.  Compute it once per backward and hand it to both functions
 * below: grad_y is then read once for it. */
int dd_conv_grad_scale(const float* grad_y, int64_t n, int precision, float* scale, void* stream);

/* dd_convx_backward_data / dd_convx_backward_weight of ddepth_conv.h (the extended channel contract, a superset: a block-64 shape runs the
 * block-64 tiles; workspace of dd_convx_workspace_bytes, unchanged) on grad_y * s, the result times 1 / s, with {s, 1 / s} = scale[0], scale[1]
 * read on the device.  scale == NULL returns DD_ERR_INVALID_ARG.  DD_PREC_BF16 ignores the pair's values, runs the kernels of
 * dd_convx_backward_* and gives their bits. */
int dd_convx_backward_data_scaled(int op, const float* grad_y, const float* w, float* grad_x, void* workspace, const float* scale, int B, int Cin,
                                  int Cout, int H, int W, int precision, void* stream);
int dd_convx_backward_weight_scaled(int op, const float* x, const float* grad_y, float* grad_w, void* workspace, const float* scale, int B, int Cin,
                                    int Cout, int H, int W, int precision, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDEPTH_CONV_SCALED_H_ */
