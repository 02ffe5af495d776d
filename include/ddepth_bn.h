/*
 * ddepth_bn.h -- C ABI of the MI355X-native batch-statistics BatchNorm, forward and backward (same shared library as ddepth.h:
 * diffusiondepth_amd/libddepth_hip.so; kernels in diffusiondepth_amd/csrc/dd_bn.hip).
 *
 * What it replaces: F.batch_norm(training=True) and the activation behind it, with their autograd, at every BatchNorm2d of the part of a
 * head that runs once per image (condition FPN, latent codec, HAHI neck) -- MIOpenBatchNormFwdTrainSpatial / MIOpenBatchNormBwdSpatial on
 * one rank, the torch composition of dist._SyncBatchNormFn on a data-parallel rank.
 *
 * The family is cut where a SyncBN exchange has to happen:
 *   forward    dd_bn_stats            -> sums   [ all-reduce(sums)  ] -> dd_bn_finalize -> dd_bn_apply
 *   backward   dd_bn_backward_reduce  -> sums2  [ all-reduce(sums2) ] -> dd_bn_backward_apply
 * sums and sums2 are small fp64 device vectors; a caller without ranks simply omits the bracket.  The number of values per channel N
 * travels inside sums and is read ON THE DEVICE by the calls behind the exchange: the host never learns the global count.
 * Backward keeps only x and mean_invstd from the forward; the activation's mask is recomputed from x.
 *
 * Conventions (those of ddepth_eval.h): DEVICE pointers; x, y, grad_y, grad_x are contiguous fp32 NCHW (B, C, H, W) with HW = H * W
 * <= INT_MAX values per plane, n = B * HW values per channel; inputs are borrowed, outputs are caller-allocated; work is enqueued on
 * `stream` and is asynchronous: no call here synchronises the host, allocates, or reads device memory on the host, so every call can be
 * captured in a hipGraph.  Every function returns DD_OK (0) or a dd_status code (ddepth.h) and leaves the message in
 * dd_bn_last_error().  Stateless (no handle) and thread-safe, provided concurrent calls use different workspaces.  There is no CPU path.
 *
 * Numerics: elements are loaded in fp32, sums are accumulated in fp64, mean / variance / the two backward means are formed in fp64 and
 * rounded to fp32 once.  Results are bitwise reproducible: no floating-point atomics, one fp64 partial per workgroup, combined in a
 * fixed order by a second small launch.
 */
#ifndef DDEPTH_BN_H_
#define DDEPTH_BN_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The activation fused behind the normalisation: y = act(z), z = (x - mean) * invstd * weight + bias. */
typedef enum dd_bn_act {
  DD_BN_ACT_NONE = 0,
  DD_BN_ACT_RELU = 1,
  DD_BN_ACT_LEAKY_RELU = 2      /* z > 0 ? z : slope * z */
} dd_bn_act;

/* Message of the last failing call of this header on the calling thread.  Never NULL. */
const char* dd_bn_last_error(void);

/* Bytes of device scratch dd_bn_stats / dd_bn_backward_reduce need for a (B, C, H, W) tensor with HW = H * W (one size serves both).
 * The caller ZEROES the workspace once after allocating it; every call leaves it reusable, call after call and replay after replay of
 * a graph.  One workspace serves one stream at a time. */
int dd_bn_workspace_bytes(int B, int C, int HW, int64_t* bytes);

/* sums (2C + 1) fp64 out: [ sum x per channel | sum x^2 per channel | n = B * HW ].  This is the payload a SyncBN exchange all-reduces
 * (SUM).  A NaN or Inf in one channel stays in that channel's two entries. */
int dd_bn_stats(const float* x, double* sums, void* workspace, int B, int C, int HW, void* stream);

/* From sums (after any exchange), in fp64: N = sums[2C], mean = sum x / N, var = max(sum x^2 / N - mean^2, 0) (biased).
 *   mean_invstd (2C) fp32 out: [ mean | 1 / sqrt(var + eps) ]
 *   running_mean, running_var (C) fp32, updated in place where non-NULL (both or neither):
 *     running_mean = (1 - momentum) * running_mean + momentum * mean
 *     running_var  = (1 - momentum) * running_var  + momentum * var * N / (N - 1)      (N = 1 gives NaN; callers refuse it, as torch does) */
int dd_bn_finalize(const double* sums, float eps, float momentum, float* mean_invstd, float* running_mean, float* running_var, int C,
                   void* stream);

/* y = act((x - mean) * (invstd * weight) + bias), fp32.  weight, bias (C) fp32; either may be NULL (= 1, = 0).  y may not alias x. */
int dd_bn_apply(const float* x, const float* mean_invstd, const float* weight, const float* bias, float* y, int act, float slope, int B,
                int C, int HW, void* stream);

/* With z the pre-activation dd_bn_apply formed (recomputed here from x by the same arithmetic, so its sign is the forward's),
 * g = grad_y * act'(z) and xhat = (x - mean) * invstd:
 *   sums2 (2C) fp64 out: [ sum g per channel | sum g * xhat per channel ]
 * The LOCAL sums2 are the bias and weight gradients; a SyncBN exchange all-reduces (SUM) them before dd_bn_backward_apply.
 * act'(0) = 0 for ReLU, = slope for LeakyReLU, as in torch. */
int dd_bn_backward_reduce(const float* x, const float* grad_y, const float* mean_invstd, const float* weight, const float* bias, int act,
                          float slope, double* sums2, void* workspace, int B, int C, int HW, void* stream);

/* grad_x = weight * invstd * (g - sum g / N - xhat * sum(g * xhat) / N), fp32 out; may not alias x or grad_y.
 *   sums2: what dd_bn_backward_reduce wrote, after any exchange     sums: the forward's (after ITS exchange); only sums[2C] = N is read */
int dd_bn_backward_apply(const float* x, const float* grad_y, const float* mean_invstd, const float* weight, const float* bias,
                         const double* sums2, const double* sums, float* grad_x, int act, float slope, int B, int C, int HW, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDEPTH_BN_H_ */
