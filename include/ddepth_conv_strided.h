/*
 * ddepth_conv_strided.h -- the stride-2 3x3 convolution of a ResNet stage opening (conv1 and the biased downsample of a BasicBlock), forward and
 * backward, with an optional bias and its gradient (same shared library as ddepth_conv.h; kernels in diffusiondepth_amd/csrc/dd_conv.hip).
 * Opt-in: nothing in ddepth_conv.h or ddepth_conv_scaled.h changes, and dd_conv_op keeps its three values.
 *
 * What it replaces: nn.Conv2d(Cin, Cout, 3, stride=2, padding=1, bias=True or False) with its autograd in .train().
 *     y[b][co][oy][ox] = bias[co] + sum over ci, ky, kx of w[co][ci][ky][kx] . x[b][ci][2 oy - 1 + ky][2 ox - 1 + kx]      (zero outside the image)
 *     Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1 for every H, W >= 1, odd or even.
 * The forward and the weight gradient are the implicit-GEMM and pixel-contraction kernels of ddepth_conv.h at stride 2.  The data gradient is a
 * kernel of its own: by the parity of an input pixel the nine taps fall into four classes (1, 2, 2 and 4 taps), so a 2 x 2 block of input pixels
 * costs nine tap GEMMs -- not the 36 of a 3x3 convolution over a zero-inserted grad_y.  The bias is added in fp32 where the accumulator is stored.
 * The bias gradient is the weight gradient of an all-ones plane: the sum of grad_y as the weight gradient's operand holds it (rounded to the
 * precision; hi + lo in the split mode), accumulated in fp64 in a fixed order.
 *
 * Channels, one contract: Cout a multiple of 8 in 8 .. 2048; Cin 3 (the RGB planes) or a multiple of 8 in 8 .. 2048.  Counts that are both
 * multiples of 64 in 64 .. 1536 run unguarded kernels; every other pair runs guarded ones that treat the channels beyond the count as zeros with
 * the same accumulation order, so the result equals that of tensors zero-padded to the next multiple of 64.
 * precision: DD_PREC_BF16, DD_PREC_F16 or DD_PREC_F16X3 as in ddepth_conv.h; every other value returns DD_ERR_UNSUPPORTED.
 *
 * Conventions: those of ddepth_conv.h -- DEVICE pointers, contiguous fp32 NCHW, raw parameters, caller-owned 16-byte aligned workspace whose
 * contents on entry do not matter, asynchronous on `stream`, no host synchronisation, allocation or host read of device memory; outputs may not
 * alias inputs; DD_OK or a dd_status code with the message in dd_conv_last_error().  Bitwise reproducible: no floating-point atomics.
 * H, W are the INPUT size of the forward in every function.
 */
#ifndef DDEPTH_CONV_STRIDED_H_
#define DDEPTH_CONV_STRIDED_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 where (Cin, Cout, precision) runs in this library, else 0.  No side effects. */
int dd_conv3x3s2_supported(int Cin, int Cout, int precision);

/* Bytes of device scratch the three directions need at this shape (one size serves all three): the padded 16-bit weight image of the forward or
 * the data gradient (twice in the split mode), or the weight gradient's partial sums. */
int dd_conv3x3s2_workspace_bytes(int B, int Cin, int Cout, int H, int W, int precision, int64_t* bytes);

/* x[B,Cin,H,W], w[Cout,Cin,3,3], bias[Cout] or NULL, y[B,Cout,Ho,Wo] */
int dd_conv3x3s2_forward(const float* x, const float* w, const float* bias, float* y, void* workspace, int B, int Cin, int Cout, int H, int W,
                         int precision, void* stream);

/* grad_y[B,Cout,Ho,Wo] -> grad_x[B,Cin,H,W], every element written.
 * scale: NULL, or the device pair of dd_conv_grad_scale (ddepth_conv_scaled.h): grad_y * s into the operand, the result * 1 / s.  DD_PREC_BF16
 * ignores its values and gives the bits of scale == NULL. */
int dd_conv3x3s2_backward_data(const float* grad_y, const float* w, float* grad_x, void* workspace, const float* scale, int B, int Cin, int Cout,
                               int H, int W, int precision, void* stream);

/* grad_w[Cout,Cin,3,3], and grad_bias[Cout] unless it is NULL.  scale: as above. */
int dd_conv3x3s2_backward_weight(const float* x, const float* grad_y, float* grad_w, float* grad_bias, void* workspace, const float* scale, int B,
                                 int Cin, int Cout, int H, int W, int precision, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDEPTH_CONV_STRIDED_H_ */
