/*
 * ddepth_conv.h -- C ABI of the MI355X-native training convolutions of the condition FPN and the HAHI neck, forward and backward (same shared
 * library as ddepth.h: diffusiondepth_amd/libddepth_hip.so; kernels in diffusiondepth_amd/csrc/dd_conv.hip).
 *
 * What it replaces: nn.Conv2d(C_i, C_o, 3, 1, 1, bias=False) (conv_lateral; the neck's conv_fusion / trans_fusion), nn.ConvTranspose2d(256, 256,
 * 2, 2, bias=False) (conv_up) and nn.Conv2d(C_i, C_o, 1, bias=False) (the neck's lateral_convs, conv_proj, trans_proj) with their autograd in
 * .train() -- fp32 MIOpen kernels otherwise -- by GEMM kernels on 16-bit MFMA operands with fp32 accumulation.
 *
 * Conventions (those of ddepth_bn.h): DEVICE pointers; every tensor is contiguous fp32 NCHW exactly as torch holds it, the weights are the
 * raw parameters (nothing is cached across calls); inputs are borrowed, outputs are caller-allocated and may not alias an input; work is
 * enqueued on `stream` and is asynchronous: no call here synchronises the host, allocates, or reads device memory on the host.  Every
 * function returns DD_OK (0) or a dd_status code (ddepth.h) and leaves the message in dd_conv_last_error().  Stateless (no handle) and
 * thread-safe, provided concurrent calls use different workspaces.  There is no CPU path.
 *
 * precision: a dd_precision value (ddepth.h).  DD_PREC_BF16 / DD_PREC_F16 round both operands to 16 bits once and contract them on
 * v_mfma_f32_32x32x16_{bf16,f16}; DD_PREC_F16X3 carries every operand as the f16 pair hi = f16(v), lo = f16(v - hi) and contracts
 * hi.hi + hi.lo + lo.hi (three MFMAs per product).  Every other value returns DD_ERR_UNSUPPORTED.
 * Channels: two contracts.  dd_conv_supported, dd_conv_workspace_bytes and the nine dd_conv3x3_* / dd_deconv2x2_* / dd_conv1x1_* functions take
 * Cin and Cout that are multiples of 64 in 64 .. 1536 (the block-64 contract).  The five dd_convx_* functions take the extended range, a
 * superset: Cin and Cout multiples of 8 in 8 .. 2048 (every width of every registered head).  Through them a block-64 shape runs the same
 * kernels and gives the same bits as through the nine; any other shape runs guarded kernels that treat the channels beyond the count as zeros,
 * with the same accumulation order, so the result equals that of the tensors zero-padded to the next multiple of 64.  Channel counts outside
 * the contract of the function called return DD_ERR_UNSUPPORTED.  H, W >= 1 are arbitrary.
 *
 * Results are bitwise reproducible: no floating-point atomics; the weight gradient's partial sums over the pixel dimension are combined
 * in a fixed order by a second launch.
 */
#ifndef DDEPTH_CONV_H_
#define DDEPTH_CONV_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dd_conv_op {
  DD_CONV_3X3 = 0,        /* Conv2d k3 s1 p1, no bias */
  DD_CONV_DECONV2X2 = 1,  /* ConvTranspose2d k2 s2, no bias */
  DD_CONV_1X1 = 2         /* Conv2d k1 s1 p0 (pointwise), no bias */
} dd_conv_op;

/* Message of the last failing call of this header on the calling thread.  Never NULL. */
const char* dd_conv_last_error(void);

/* 1 where (op, Cin, Cout, precision) runs in this library, else 0.  No side effects (dd_conv_last_error() is left alone). */
int dd_conv_supported(int op, int Cin, int Cout, int precision);

/* Bytes of device scratch the three directions of `op` need at this shape (one size serves all three; H, W are the INPUT size of the
 * forward).  The workspace must be 16-byte aligned; its contents on entry do not matter.  One workspace serves one stream at a time. */
int dd_conv_workspace_bytes(int op, int B, int Cin, int Cout, int H, int W, int precision, int64_t* bytes);

/* 3x3, stride 1, pad 1, no bias:  x[B,Cin,H,W], w[Cout,Cin,3,3], y[B,Cout,H,W] */
int dd_conv3x3_forward(const float* x, const float* w, float* y, void* workspace, int B, int Cin, int Cout, int H, int W, int precision,
                       void* stream);
int dd_conv3x3_backward_data(const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int Cin, int Cout, int H, int W,
                             int precision, void* stream);
int dd_conv3x3_backward_weight(const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H, int W,
                               int precision, void* stream);

/* ConvTranspose2d k2 s2, no bias:  x[B,Cin,H,W], w[Cin,Cout,2,2], y[B,Cout,2H,2W]  (H, W = input size) */
int dd_deconv2x2_forward(const float* x, const float* w, float* y, void* workspace, int B, int Cin, int Cout, int H, int W, int precision,
                         void* stream);
int dd_deconv2x2_backward_data(const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int Cin, int Cout, int H, int W,
                               int precision, void* stream);
int dd_deconv2x2_backward_weight(const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H,
                                 int W, int precision, void* stream);

/* 1x1 (pointwise), stride 1, no padding, no bias:  x[B,Cin,H,W], w[Cout,Cin,1,1], y[B,Cout,H,W].  Kernels of their own: a plane is a flat run of
 * H * W pixels (no halo), tiled 128 consecutive pixels at a time; any H * W, odd ones included (every load of a tensor is a dword load). */
int dd_conv1x1_forward(const float* x, const float* w, float* y, void* workspace, int B, int Cin, int Cout, int H, int W, int precision,
                       void* stream);
int dd_conv1x1_backward_data(const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int Cin, int Cout, int H, int W,
                             int precision, void* stream);
int dd_conv1x1_backward_weight(const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H, int W,
                               int precision, void* stream);

/* ---- the extended channel range: Cin, Cout multiples of 8 in 8 .. 2048; `op` is a dd_conv_op, tensors and H, W as for that operator above ---- */

/* 1 where (op, Cin, Cout, precision) runs through dd_convx_*, else 0.  No side effects. */
int dd_convx_supported(int op, int Cin, int Cout, int precision);

/* As dd_conv_workspace_bytes.  The packed weights are padded to whole tiles (Cout, or Cin in the data gradient, to a multiple of 64; the
 * other count to a multiple of 32) and the size covers that; a workspace of the size dd_conv_workspace_bytes would give for rounded-down
 * counts is too small.  The weight gradient's partials grow with the range: 3x3, 2048 -> 1536, B = 4, 11 x 38 needs about 680 MB. */
int dd_convx_workspace_bytes(int op, int B, int Cin, int Cout, int H, int W, int precision, int64_t* bytes);

int dd_convx_forward(int op, const float* x, const float* w, float* y, void* workspace, int B, int Cin, int Cout, int H, int W, int precision,
                     void* stream);
int dd_convx_backward_data(int op, const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int Cin, int Cout, int H, int W,
                           int precision, void* stream);
int dd_convx_backward_weight(int op, const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H, int W,
                             int precision, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDEPTH_CONV_H_ */
