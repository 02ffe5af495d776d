/*
 * ddepth_bn_add.h -- the batch-statistics BatchNorm of ddepth_bn.h with an ADDEND fused into its apply (same shared library; kernels in
 * diffusiondepth_amd/csrc/dd_bn.hip).
 *
 * What it replaces: the elementwise glue torch runs between a BatchNorm and its neighbours where a residual joins --
 *   DD_BN_ADD_PRE    y = act(z + r)    the tail of a ResNet BasicBlock: relu(bn2(conv2(out)) + identity)
 *   DD_BN_ADD_POST   y = act(z) + r    the top-down add of the FPN: lateral(f) + conv_up(x)
 * with z = (x - mean) * invstd * weight + bias the pre-activation dd_bn_apply forms, by the same arithmetic (one fused multiply-add),
 * followed by ONE fp32 add of r.
 *
 * Statistics are those of x alone: dd_bn_stats and dd_bn_finalize are used as they are, and a SyncBN exchange is unchanged.
 *   forward          dd_bn_stats -> sums [ all-reduce ] -> dd_bn_finalize -> dd_bn_apply_add
 *   backward, PRE    dd_bn_backward_reduce_add -> g (= grad_addend), sums2 [ all-reduce ] -> dd_bn_backward_apply(x, g, act = DD_BN_ACT_NONE)
 *   backward, POST   nothing new: dd_bn_backward_reduce / dd_bn_backward_apply on (x, grad_y) -- the mask recomputed from x is still the
 *                    forward's -- and grad_addend is grad_y itself
 *
 * Conventions are those of ddepth_bn.h: DEVICE pointers, contiguous fp32 NCHW, errors in dd_bn_last_error(), stateless, asynchronous,
 * no allocation, no host read, capturable in a hipGraph, workspace from dd_bn_workspace_bytes (zeroed once by the caller).
 */
#ifndef DDEPTH_BN_ADD_H_
#define DDEPTH_BN_ADD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum dd_bn_add_mode {
  DD_BN_ADD_PRE = 0,      /* y = act(z + r)   BasicBlock tail   */
  DD_BN_ADD_POST = 1      /* y = act(z) + r   FPN top-down add  */
} dd_bn_add_mode;

/* y = act(z + addend) (PRE) or act(z) + addend (POST), fp32; act, slope as in dd_bn_apply.  weight, bias (C) fp32; either may be NULL
 * (= 1, = 0).  addend has x's shape.  y may alias neither x nor addend. */
int dd_bn_apply_add(const float* x, const float* mean_invstd, const float* weight, const float* bias, const float* addend, float* y,
                    int act, float slope, int add_mode, int B, int C, int HW, void* stream);

/* The PRE-mode backward's reduction, in one pass.  y is the forward's OUTPUT and carries the activation's mask:
 *   g = grad_y * act'(y):  ReLU passes nothing at y <= 0 (a NaN y passes grad_y);  LeakyReLU: y > 0 ? grad_y : grad_y * slope;
 *                          DD_BN_ACT_NONE: g = grad_y
 * The sign of y is the sign of z + r for ReLU and for any slope >= 0, so neither the addend nor the affine parameters are read;
 * LeakyReLU with slope < 0 returns DD_ERR_UNSUPPORTED.
 *   g (B, C, HW) fp32 out: the gradient of the addend, and the grad_y of dd_bn_backward_apply(x, g, ..., act = DD_BN_ACT_NONE);
 *     may alias no input
 *   sums2 (2C) fp64 out: [ sum g per channel | sum g * xhat per channel ], xhat = (x - mean) * invstd, accumulated in the order of
 *     dd_bn_backward_reduce: on mutually aligned tensors the bits equal those of dd_bn_backward_reduce(x, g, act = DD_BN_ACT_NONE) */
int dd_bn_backward_reduce_add(const float* x, const float* grad_y, const float* y, const float* mean_invstd, int act, float slope,
                              float* g, double* sums2, void* workspace, int B, int C, int HW, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDEPTH_BN_ADD_H_ */
