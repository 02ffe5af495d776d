/*
 * ddepth_swin_backward.h -- the backward of dd_window_attention_forward (ddepth_swin.h): the gradients with respect to qkv, qkv_pad and rel_bias
 * from qkv, qkv_pad, rel_bias and grad_out alone (same shared library; kernel in diffusiondepth_amd/csrc/dd_swin_bwd.hip).  Opt-in: nothing in
 * ddepth_swin.h changes.
 *
 * Nothing is saved by the forward.  Per task = (image, window, head) the scores, the row maximum and the row sum are computed again exactly as
 * the forward computes them; with P = softmax(S) and S = (scale q) . k^T + bias + mask:
 *     dP = dO . V^T      D_i = sum_j P_ij dP_ij      dS = P o (dP - D)
 *     dV = P^T . dO      dK = dS^T . (scale Q)       dQ = scale (dS . K)      (scale multiplies the finished fp32 sum, once)
 *     grad_rel_bias[head] = sum of dS over images and windows
 *     grad_qkv_pad        = sum of the dq / dk / dv rows of every padded slot over images and windows (also when qkv_pad == NULL)
 * All sums, the softmax, D and grad_rel_bias are fp32 at every precision.  DD_PREC_BF16 / DD_PREC_F16 round scale q, k, v, P (for dV), dO and
 * dS (for dQ and dK) to the operand type once each; DD_PREC_FP32 runs the same data through the fp32 MFMA.
 *
 *     grad_out       fp32 [B, H, W, C], the layout of the forward's `out`
 *     grad_qkv       fp32 [B, H, W, 3 C]: every element is written exactly once (each token is a slot of exactly one window); it need not be
 *                    zeroed.  Padded positions are never stored.
 *     grad_qkv_pad   3 C floats, or NULL
 *     grad_rel_bias  fp32 [heads, 49, 49] dense, or NULL.  (The gradient of the (2 * 7 - 1)^2 table is a fixed gather of it: the caller's.)
 *     workspace      dd_window_attention_backward_workspace_bytes bytes, 16-byte aligned.  It holds one partial of grad_rel_bias and
 *                    grad_qkv_pad per (slice of windows, head); a second kernel sums the slices in ascending order.  How the windows are sliced
 *                    depends on the shape alone, never on the device: the size needs no device and two devices give the same bits.  The
 *                    call writes every workspace byte it reads; the caller does not initialise it.  No floating-point atomics anywhere.
 *     scale          NULL, or the 4-float device buffer {s, 1 / s, ..} that dd_conv_grad_scale (ddepth_conv_scaled.h) writes for grad_out.
 *                    DD_PREC_F16 multiplies grad_out by s before anything is rounded and all three results by 1 / s at the store, so that
 *                    gradients at training scale (about 3e-7) are rounded where f16 has its 11 bits.  The other precisions ignore the values.
 *
 * Supported: what dd_window_attention_supported answers (C == 32 * heads, window == 7, three precisions).
 *
 * Conventions: those of ddepth_swin.h -- DEVICE pointers, contiguous fp32, 16-byte aligned; asynchronous on `stream`; no host synchronisation,
 * allocation or host read of device memory (the call can be captured in a graph); two calls give the same bits; no output may alias an input
 * or another output; DD_ERR_UNSUPPORTED / DD_ERR_INVALID_ARG are answered before anything is launched, with the message in
 * dd_swin_last_error(), and a refused call writes nothing.
 */
#ifndef DDEPTH_SWIN_BACKWARD_H_
#define DDEPTH_SWIN_BACKWARD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 where (C, heads, window, precision) runs in this library, else 0.  No side effects. */
int dd_window_attention_backward_supported(int C, int heads, int window, int precision);

/* The workspace of one call at this shape, in bytes.  Needs no device. */
int dd_window_attention_backward_workspace_bytes(int B, int H, int W, int C, int heads, int window, int precision, int64_t* bytes);

int dd_window_attention_backward(const float* qkv, const float* qkv_pad, const float* rel_bias, const float* grad_out, float* grad_qkv,
                                 float* grad_qkv_pad /* may be NULL */, float* grad_rel_bias /* may be NULL */, void* workspace,
                                 const float* scale /* may be NULL */, int B, int H, int W, int C, int heads, int window, int shift,
                                 int precision, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDEPTH_SWIN_BACKWARD_H_ */
