/*
 * ddepth_linear.h -- the token Linears of a Swin block (`qkv`, `proj`, the MLP's `fc1` and `fc2`, PatchMerging's reduction) on the MFMA units, with
 * the block's cheap neighbours in the epilogue: bias, exact GELU and the residual add.  Forward only (same shared library as ddepth.h; kernel in
 * diffusiondepth_amd/csrc/dd_linear.hip).  Opt-in: nothing in the other headers changes.
 *
 *     y[m, n] = act(sum_k x[m, k] * w[n, k] + bias[n]) + addend[m, n]
 *
 *     x       fp32 [M, K] row-major: the token tensor as LayerNorm or the attention operator wrote it
 *     w       fp32 [N, K]: nn.Linear.weight as it is (dd_linear_pack reads it; dd_linear_forward reads the packed image `wp`)
 *     bias    N floats, or NULL
 *     addend  fp32 [M, N], or NULL: the block's residual, added AFTER the activation
 *     y       fp32 [M, N]
 *     act     0 = none, 1 = GELU in the exact erf form 0.5 v (1 + erf(v / sqrt 2)): nn.GELU()'s default
 * `precision` chooses the MFMA operand type only: DD_PREC_FP32 (the parity mode, v_mfma_f32_32x32x2_f32), DD_PREC_BF16 or DD_PREC_F16
 * (v_mfma_f32_32x32x16_*), which round x and w once each to the operand type.  Accumulation, bias, GELU and add are fp32 at every precision.
 *
 * Packed weights: dd_linear_pack writes the operand image once -- [N][K] in the operand type (fp32: a copy), dd_linear_packed_bytes bytes -- and
 * the caller may keep it for as long as the weight does not change.  An image is valid for the (K, N, precision) it was packed for.
 *
 * Supported: K and N multiples of 32 in 32 .. 8192, act 0 or 1, those three precisions; M >= 1 takes any value (rows beyond M are read as zeros
 * and never stored).  Anything else is DD_ERR_UNSUPPORTED, answered before anything is launched.
 *
 * Conventions: DEVICE pointers, contiguous; x, w, wp, addend and y 16-byte aligned; asynchronous on `stream`; no workspace, no atomics, no host
 * synchronisation, allocation or host read of device memory (the call can be captured in a graph); two calls give the same bits; y may not alias
 * x, wp, bias or addend (checked for equal pointers: DD_ERR_INVALID_ARG); DD_OK or a dd_status code (ddepth.h) with the message in
 * dd_linear_last_error().  The order in which the K products of an output are summed depends on (K, N, precision) alone -- never on M, the grid
 * or the device: row m of y is a function of row m of x, bit for bit, whatever the other rows are.
 *
 * Not here: the backward, a 16-bit output, LayerNorm, the split-f16 mode.
 */
#ifndef DDEPTH_LINEAR_H_
#define DDEPTH_LINEAR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The message of the last failed call of this header on the calling thread. */
const char* dd_linear_last_error(void);

/* 1 where (K, N, act, precision) runs in this library, else 0.  No side effects, no device. */
int dd_linear_supported(int K, int N, int act, int precision);

/* The size of the packed image of an [N, K] weight at `precision`.  No device. */
int dd_linear_packed_bytes(int K, int N, int precision, int64_t* bytes);

int dd_linear_pack(const float* w, void* wp, int K, int N, int precision, void* stream);

int dd_linear_forward(const float* x, const void* wp, const float* bias, const float* addend, float* y,
                      long long M, int K, int N, int act, int precision, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDEPTH_LINEAR_H_ */
