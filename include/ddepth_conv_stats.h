/*
 * ddepth_conv_stats.h -- a training 3x3 pad-1 convolution, stride 1 or 2, that also emits the statistics of the BatchNorm behind it (same shared
 * library as ddepth_conv.h; kernels in diffusiondepth_amd/csrc/dd_conv.hip).  Opt-in: nothing in ddepth_conv.h, ddepth_conv_scaled.h,
 * ddepth_conv_strided.h, ddepth_conv_fused.h or ddepth_bn.h changes.
 *
 * What it replaces: in .train() a BatchNorm starts with dd_bn_stats, a full read of the tensor the convolution has just written.  Here the
 * convolution's epilogue, which holds its 4 x 32 pixel x 64 channel output tile in registers, sums the values it stores:
 *     y      exactly what dd_convx_forward(DD_CONV_3X3) (stride 1) or dd_conv3x3s2_forward (stride 2) stores for the same inputs, bit for bit;
 *            a bias (NULL: none) is added in fp32 where the accumulator is stored, at either stride
 *     sums   [2 * Cout + 1] doubles, the layout of dd_bn_stats: sums[c] = sum of y over batch and plane, sums[Cout + c] = sum of y^2,
 *            sums[2 * Cout] = B * Ho * Wo.  Each stored fp32 value is widened to fp64 and then squared (exact); the sums are fp64.
 * It drops in front of dd_bn_finalize (after the all-reduce of `sums` under SyncBN) with nothing else to change.  The ORDER of the additions is
 * that of the convolution's tiles, not dd_bn_stats's: on data whose sums are exact in fp64 the two agree bit for bit, elsewhere within the
 * rounding of an fp64 sum.  No floating-point atomics; the order depends on the shape alone, so two calls give the same bits.  A NaN or Inf in
 * one channel's values stays in that channel's two entries.
 *
 * Channels: those of dd_conv3x3_affine_supported -- stride 1 takes what dd_convx_supported(DD_CONV_3X3, ...) takes, stride 2 what
 * dd_conv3x3s2_supported takes (Cin = 3 included).  precision: DD_PREC_BF16, DD_PREC_F16 or DD_PREC_F16X3.
 *
 * Conventions: those of ddepth_conv_fused.h -- DEVICE pointers, contiguous fp32 NCHW, raw parameters, caller-owned 16-byte aligned workspace whose
 * contents on entry do not matter (the packed weight image, then one fp64 pair per channel, image and tile), asynchronous on `stream`, no host
 * synchronisation, allocation or host read of device memory (the call can be captured in a graph); no output may alias an input; DD_OK or a
 * dd_status code with the message in dd_conv_last_error().  H, W are the INPUT size.
 *
 * Not here: the transpose, pointwise and codec convolutions, and statistics in the backward.
 */
#ifndef DDEPTH_CONV_STATS_H_
#define DDEPTH_CONV_STATS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 where (stride, Cin, Cout, precision) runs in this library, else 0.  No side effects. */
int dd_conv3x3_stats_supported(int stride, int Cin, int Cout, int precision);

/* Bytes of device scratch of one forward at this shape: the padded 16-bit weight image (twice in the split mode) and the partial sums. */
int dd_conv3x3_stats_workspace_bytes(int stride, int B, int Cin, int Cout, int H, int W, int precision, int64_t* bytes);

/* x[B,Cin,H,W], w[Cout,Cin,3,3], bias[Cout] or NULL, y[B,Cout,Ho,Wo], sums[2 * Cout + 1]; stride 1: Ho = H, Wo = W; stride 2:
 * Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1. */
int dd_conv3x3_stats_forward(const float* x, const float* w, const float* bias, float* y, double* sums, void* workspace,
                             int stride, int B, int Cin, int Cout, int H, int W, int precision, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDEPTH_CONV_STATS_H_ */
