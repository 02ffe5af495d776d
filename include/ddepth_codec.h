/*
 * ddepth_codec.h -- C ABI of the MI355X-native training convolutions of the latent depth codec, forward and backward, and of its fused decoder
 * tail (same shared library as ddepth.h: diffusiondepth_amd/libddepth_hip.so; kernels in diffusiondepth_amd/csrc/dd_codec.hip).
 *
 * What it replaces: the four convolutions of DeepDepthTransformWithUpsampling (1 -> 16 k3 s2 p1; 16 -> 16 k3 s1 p1; ConvTranspose2d 16 -> 16
 * k4 s2 p1 with bias; 16 -> 1 k3 s1 p1 with bias) with their autograd in .train() -- fp32 MIOpen kernels otherwise -- and the four elementwise
 * launches of 1 / sigmoid(z).clamp(eps) - 1 behind the decoder, by fp32 kernels with the four geometries fixed at compile time.
 *
 * Conventions (those of ddepth_conv.h): DEVICE pointers; every tensor is contiguous fp32 NCHW exactly as torch holds it, the weights are the
 * raw parameters (nothing is cached across calls); inputs are borrowed, outputs are caller-allocated and may not alias an input; work is
 * enqueued on `stream` and is asynchronous: no call here synchronises the host, allocates, or reads device memory on the host.  Every
 * function returns DD_OK (0) or a dd_status code (ddepth.h) and leaves the message in dd_codec_last_error().  Stateless (no handle) and
 * thread-safe, provided concurrent calls use different workspaces.  There is no CPU path.
 *
 * Arithmetic: fp32 operands, fp32 FMA; a tap outside the image contributes an exact zero; NaN and Inf propagate.  H, W >= 1 are arbitrary
 * (4 * H * W must fit an int), B <= 65535.  H, W are always the op's INPUT size of the forward.
 *
 * Results are bitwise reproducible: no floating-point atomics; the weight and bias gradients' partial sums over the pixel dimension are
 * combined in a fixed order, in fp64, by a second launch and rounded to fp32 once.
 */
#ifndef DDEPTH_CODEC_H_
#define DDEPTH_CODEC_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dd_codec_op {
  DD_CODEC_ENC0 = 0, /* Conv2d 1 -> 16, k3 s2 p1, no bias:        x[B,1,H,W],   w[16,1,3,3],  y[B,16,(H-1)/2+1,(W-1)/2+1] */
  DD_CODEC_ENC1 = 1, /* Conv2d 16 -> 16, k3 s1 p1, no bias:       x[B,16,H,W],  w[16,16,3,3], y[B,16,H,W] */
  DD_CODEC_DEC0 = 2, /* ConvTranspose2d 16 -> 16, k4 s2 p1, bias: x[B,16,H,W],  w[16(ci),16(co),4,4], bias[16], y[B,16,2H,2W] */
  DD_CODEC_DEC1 = 3  /* Conv2d 16 -> 1, k3 s1 p1, bias:           x[B,16,H,W],  w[1,16,3,3],  bias[1],  y[B,1,H,W] */
} dd_codec_op;

/* Message of the last failing call of this header on the calling thread.  Never NULL. */
const char* dd_codec_last_error(void);

/* Bytes of device scratch the three directions of `op` need at this shape (one size serves all three: the repacked weights of the forward and
 * the data gradient, the weight gradient's partial sums).
 * The workspace must be 16-byte aligned; its contents on entry do not matter.  One workspace serves one stream at a time. */
int dd_codec_workspace_bytes(int op, int B, int H, int W, int64_t* bytes);

/* y = conv(x, w) + bias.  bias must be NULL for ENC0 / ENC1 and may be NULL (no bias added) for DEC0 / DEC1. */
int dd_codec_conv_forward(int op, const float* x, const float* w, const float* bias, float* y, void* workspace, int B, int H, int W,
                          void* stream);

/* grad_x from grad_y (the forward's output shape) and w.  ENC0's and DEC0's are gathers by parity class: no scatter, no atomics. */
int dd_codec_conv_backward_data(int op, const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int H, int W, void* stream);

/* grad_w (the weight's shape) and, for DEC0 / DEC1, grad_bias = the sum of grad_y per output channel.  grad_bias must be NULL for ENC0 / ENC1
 * and may be NULL for the others (it is then not written). */
int dd_codec_conv_backward_weight(int op, const float* x, const float* grad_y, float* grad_w, float* grad_bias, void* workspace, int B, int H,
                                  int W, void* stream);

/* depth[i] = 1 / max(sigmoid(z[i]), eps) - 1 over n elements: the operation sequence of dd_decode's last stage, bit for bit. */
int dd_codec_tail_forward(const float* z, float* depth, int64_t n, float eps, void* stream);

/* grad_z[i] = -grad_depth[i] * (1 - s) / s where s = sigmoid(z[i]) >= eps, else 0 (torch's clamp(min) rule); the factor is evaluated as
 * exp(-z[i]), which it equals.  A NaN in z gives NaN. */
int dd_codec_tail_backward(const float* z, const float* grad_depth, float* grad_z, int64_t n, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDEPTH_CODEC_H_ */
