/*
 * ddepth_eval.h -- C ABI of the MI355X-native depth metrics and supervised L1 / L2 loss (same shared library as ddepth.h:
 * diffusiondepth_amd/libddepth_hip.so; kernels in diffusiondepth_amd/csrc/dd_eval.hip).
 *
 * These are the two consumers of output['pred'] that every run of the reference's main.py calls:
 *   dd_depth_metric_sums + dd_depth_metrics   <- Diffusion_DCbase_Metric.evaluate   (src/metric/diffusion_dcbase_metric.py:31-93)
 *   dd_sup_loss_forward / dd_sup_loss_backward <- L1Loss.forward + L2Loss.forward    (src/loss/submodule/l1loss.py:22-39, l2loss.py:22-39)
 *                                                 and what torch autograd derives from them for loss.backward() (src/main.py)
 * as used by Diffusion_DCbase_Loss.compute (src/loss/diffusion_dcbase_loss.py:14-49) with the default --loss 1.0*L1+1.0*L2+1.0*DDIM
 * (src/config.py:147).  The reference's metric is about 45 small torch launches with four boolean-mask gathers, each of which makes
 * the host wait for the device; here it is one streaming pass and nothing waits.
 *
 * Conventions (those of ddepth.h / ddepth_dcn.h): DEVICE pointers; pred and gt are contiguous fp32 (B,1,H,W) tensors exactly as
 * output['pred'] and sample['gt'] hold them, n = H*W <= INT_MAX pixels per image; inputs are borrowed, outputs are caller-allocated;
 * work is enqueued on `stream` and is asynchronous: no call here synchronises the host, allocates, or reads device memory on the
 * host, so every call can be captured in a hipGraph.  Every function returns DD_OK (0) or a dd_status code (ddepth.h) and leaves
 * the message in dd_eval_last_error().  Stateless (no handle) and thread-safe, provided concurrent calls use different workspaces.
 * There is no CPU path.
 *
 * Numerics: per-pixel arithmetic is fp32, operation for operation the reference's (no FMA contraction), so n_valid and the three
 * delta counts are the reference's integers; only the ACCUMULATION is wider (fp64; the reference sums in fp32).  Results are bitwise
 * reproducible: no floating-point atomics, workgroup partials are combined in a fixed order.
 */
#ifndef DDEPTH_EVAL_H_
#define DDEPTH_EVAL_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* How the per-workgroup partial sums of one call are combined (both give the same bits). */
typedef enum dd_eval_reduce {
  DD_EVAL_REDUCE_DEFAULT = 0,        /* the faster one as measured on the MI355X */
  DD_EVAL_REDUCE_TWO_LAUNCH = 1,     /* a second small launch reads the partial slab */
  DD_EVAL_REDUCE_TICKET = 2          /* the last workgroup of an image to arrive reads it (integer tickets in the workspace) */
} dd_eval_reduce;

#define DD_METRIC_SUMS 9    /* [n_valid, S|d|, S d^2, S|dinv|, S dinv^2, S|d|/(gt+1e-8), #(ratio<1.25), #(ratio<1.25^2), #(ratio<1.25^3)] */
#define DD_METRICS 8        /* [RMSE, MAE, iRMSE, iMAE, REL, D^1, D^2, D^3]  (metric_name, diffusion_dcbase_metric.py:27-29) */
#define DD_LOSS_SUMS 3      /* [S|p-g| m, S(p-g)^2 m, S m] */

/* Message of the last failing call of this header on the calling thread.  Never NULL. */
const char* dd_eval_last_error(void);

/* Bytes of device scratch dd_depth_metric_sums / dd_sup_loss_forward need for B images of H*W pixels (one size serves both).
 * The first 4096 bytes hold the arrival tickets of DD_EVAL_REDUCE_TICKET (one per image and one over the images; batches of more
 * than 1023 images combine by the second launch whatever was asked): the caller ZEROES the workspace once after allocating it;
 * every call leaves its tickets at zero again, so the buffer is reused call after call (and replay after replay of a graph)
 * without further attention.  One workspace serves one stream at a time. */
int dd_eval_workspace_bytes(int B, int H, int W, int64_t* bytes);

/* Replaces: the per-pixel part and the .sum() calls of Diffusion_DCbase_Metric.evaluate (diffusion_dcbase_metric.py:36-85).
 *   pred, gt (B,1,H,W)     sums (B, DD_METRIC_SUMS) fp64 out, one row per image
 * Per pixel, fp32: valid iff gt > t_valid (:40; a NaN gt is not valid); d = pred - gt (:53); pred_inv = 1 / (pred + 1e-8), 0 where
 * pred <= t_valid (:36,:49); gt_inv likewise (:37,:50); dinv = pred_inv - gt_inv (:63); rel = |d| / (gt + 1e-8) (:73);
 * ratio = max(gt / (pred + 1e-8), pred / (gt + 1e-8)) (:77-79).  A NaN pred at a valid pixel reaches the sums as NaN, as it reaches
 * the reference's metrics; n_valid and the three counts are exact integers (up to 2^53). */
int dd_depth_metric_sums(const float* pred, const float* gt, double* sums, void* workspace, int B, int H, int W, float t_valid,
                         int reduce, void* stream);

/* Replaces: the formulas of evaluate (:57-90): x / (n_valid + 1e-8), sqrt for RMSE and iRMSE.
 *   sums (B, DD_METRIC_SUMS) fp64
 *   batch_metrics (DD_METRICS) fp32 out, or NULL: over ALL valid pixels of the batch -- what the reference returns (its mask gathers
 *                 over the whole (B,1,H,W) tensor); the rows of sums are added in image order first
 *   image_metrics (B, DD_METRICS) fp32 out, or NULL: the same formulas per image
 * The quotients are taken in fp64 and rounded once (the reference divides fp32 by fp32).  No valid pixel gives 0 / 1e-8 = 0. */
int dd_depth_metrics(const double* sums, float* batch_metrics, float* image_metrics, int B, void* stream);

/* Replaces: L1Loss.forward and L2Loss.forward (l1loss.py:22-39, l2loss.py:22-39) in ONE pass:
 *   p = clamp(pred, 0, max_depth), g = clamp(gt, 0, max_depth) (:23-24), m = g > t_valid as 0 / 1 (:26; multiplied in, as the
 *   reference does), per image s1 = S|p-g| m, s2 = S(p-g)^2 m, cnt = S m (:28-31);
 *   loss[0] = L1 = sum_b s1_b / (cnt_b + 1e-8), loss[1] = L2 = sum_b s2_b / (cnt_b + 1e-8) (:33-37)
 *   loss (2) fp32 out     sums (B, DD_LOSS_SUMS) fp64 out: keep it for dd_sup_loss_backward */
int dd_sup_loss_forward(const float* pred, const float* gt, float* loss, double* sums, void* workspace, int B, int H, int W,
                        float max_depth, float t_valid, int reduce, void* stream);

/* Replaces: what torch autograd computes for d(g1 * L1 + g2 * L2) / d pred through the code above; one elementwise pass, fp32:
 *   grad_pred = [0 <= pred <= max_depth] * m * (g1 / (cnt_b + 1e-8) * sign(p - g) + g2 / (cnt_b + 1e-8) * 2 (p - g))
 * with autograd's edge rules: clamp passes gradient at both ends of its range, abs has gradient 0 at 0, masked pixels get 0.
 *   sums: what dd_sup_loss_forward wrote for the same pred / gt
 *   grad_l1, grad_l2: DEVICE pointers to the two upstream gradients (one fp32 each); either may be NULL (= 0).  Never read on the host.
 *   grad_pred (B,1,H,W) fp32 out, overwritten */
int dd_sup_loss_backward(const float* pred, const float* gt, const double* sums, const float* grad_l1, const float* grad_l2,
                         float* grad_pred, int B, int H, int W, float max_depth, float t_valid, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DDEPTH_EVAL_H_ */
