/*
 * ddepth_conv_fused.h -- the eval-mode forward of a ResNet BasicBlock's convolutions: a 3x3 pad-1 convolution of stride 1 or 2 whose epilogue applies
 * a folded BatchNorm, adds the residual and applies the ReLU (same shared library as ddepth_conv.h; kernels in diffusiondepth_amd/csrc/dd_conv.hip).
 * Opt-in: nothing in ddepth_conv.h, ddepth_conv_scaled.h or ddepth_conv_strided.h changes.
 *
 * What it replaces: in .eval(), relu(batch_norm(conv2d(x, w, conv_bias, stride, 1)) + addend) with the BatchNorm's running statistics -- a
 * convolution and up to four elementwise passes over fp32 planes -- by two launches on top of the weight pack:
 *     dd_bn_fold                   scale[c] = weight[c] / sqrt(running_var[c] + eps),  shift[c] = bias[c] + (conv_bias[c] - running_mean[c]) * scale[c]
 *                                  in fp64, each rounded once to fp32, into scale_shift[2][C] (row 0 the scales, row 1 the shifts)
 *     dd_conv3x3_affine_forward    y = act(conv(x, w) * scale + shift + addend): the implicit GEMM of ddepth_conv.h (stride 1) or
 *                                  ddepth_conv_strided.h (stride 2); where an accumulator is stored, in fp32,
 *                                      v = fma(acc, scale[co], shift[co]);  v += addend[...] (unless NULL);  v = v < 0 ? 0 : v (relu != 0)
 *                                  The ReLU keeps a NaN, as torch's does.  At most two fp32 roundings behind the accumulation.
 * With scale = 1 and shift = 0 (or the bias), no addend and relu = 0 the result is that of dd_convx_forward(DD_CONV_3X3) / dd_conv3x3s2_forward.
 *
 * Channels: stride 1 takes what dd_convx_supported(DD_CONV_3X3, ...) takes (multiples of 8 in 8 .. 2048), stride 2 what dd_conv3x3s2_supported takes
 * (Cin = 3 included).  Counts that are both multiples of 64 in 64 .. 1536 run the unguarded kernel; every other pair runs the guarded one, which
 * reads scale_shift for the real rows only and addend inside the output plane only.
 * precision: DD_PREC_BF16, DD_PREC_F16 or DD_PREC_F16X3; every other value returns DD_ERR_UNSUPPORTED.
 *
 * Conventions: those of ddepth_conv_strided.h -- DEVICE pointers, contiguous fp32 NCHW, raw parameters, caller-owned 16-byte aligned workspace whose
 * contents on entry do not matter, asynchronous on `stream`, no host synchronisation, allocation or host read of device memory; y may not alias
 * an input; DD_OK or a dd_status code with the message in dd_conv_last_error().  Bitwise reproducible.  H, W are the INPUT size.
 */
#ifndef DDEPTH_CONV_FUSED_H_
#define DDEPTH_CONV_FUSED_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* scale_shift[2][C] from an eval-mode BatchNorm (weight, bias: its affine parameters; running_mean, running_var, eps) behind a convolution with the
 * bias conv_bias.  weight, bias and conv_bias may each be NULL: read as 1, 0 and 0.  running_mean and running_var may be NULL together: no
 * normalisation (scale = weight, shift = bias + conv_bias * weight) -- with everything else NULL but conv_bias, a bare biased convolution.
 * One thread per channel, no atomics. */
int dd_bn_fold(const float* weight, const float* bias, const float* running_mean, const float* running_var, double eps,
               const float* conv_bias, float* scale_shift /* [2][C] */, int C, void* stream);

/* 1 where (stride, Cin, Cout, precision) runs in this library, else 0.  No side effects. */
int dd_conv3x3_affine_supported(int stride, int Cin, int Cout, int precision);

/* Bytes of device scratch of one forward at this shape: the padded 16-bit weight image (twice in the split mode). */
int dd_conv3x3_affine_workspace_bytes(int stride, int B, int Cin, int Cout, int H, int W, int precision, int64_t* bytes);

/* x[B,Cin,H,W], w[Cout,Cin,3,3], scale_shift[2][Cout], addend[B,Cout,Ho,Wo] or NULL, y[B,Cout,Ho,Wo]; stride 1: Ho = H, Wo = W; stride 2:
 * Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1.  relu: 0 or 1. */
int dd_conv3x3_affine_forward(const float* x, const float* w, const float* scale_shift, const float* addend, float* y, void* workspace,
                              int stride, int relu, int B, int Cin, int Cout, int H, int W, int precision, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDEPTH_CONV_FUSED_H_ */
