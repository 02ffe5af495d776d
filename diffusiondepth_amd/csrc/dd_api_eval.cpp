// dd_api_eval.cpp -- the C ABI of include/ddepth_eval.h: argument checks and the launch sequence; the kernels are in dd_eval.hip.
#include "../../include/ddepth.h"
#include "../../include/ddepth_eval.h"
#include "dd_eval.h"
#include "dd_status.h"

#include <climits>
#include <cmath>

namespace {

thread_local ddstatus::LastError g_eval_err;

// The combine step both families default to: DESIGN.md section 5 has the measurement behind the choice.
constexpr int kDefaultReduce = DD_EVAL_REDUCE_TICKET;

int check_shape(int B, int H, int W, int* n) {
  if (B < 1 || H < 1 || W < 1) return g_eval_err.fail(DD_ERR_INVALID_ARG, "B, H, W must be positive (got %d, %d, %d)", B, H, W);
  if (B > 65535) return g_eval_err.fail(DD_ERR_INVALID_ARG, "B = %d exceeds 65535 images per call", B);
  if ((long long)H * W > INT_MAX) return g_eval_err.fail(DD_ERR_INVALID_ARG, "H * W = %lld exceeds INT_MAX", (long long)H * W);
  *n = H * W;
  return DD_OK;
}

int check_reduce(int* reduce) {
  if (*reduce == DD_EVAL_REDUCE_DEFAULT) *reduce = kDefaultReduce;
  if (*reduce != DD_EVAL_REDUCE_TWO_LAUNCH && *reduce != DD_EVAL_REDUCE_TICKET)
    return g_eval_err.fail(DD_ERR_INVALID_ARG, "reduce must be a dd_eval_reduce value (got %d)", *reduce);
  return DD_OK;
}

}  // namespace

extern "C" {

const char* dd_eval_last_error(void) { return g_eval_err.text.c_str(); }

int dd_eval_workspace_bytes(int B, int H, int W, int64_t* bytes) {
  if (!bytes) return g_eval_err.fail(DD_ERR_INVALID_ARG, "bytes is NULL");
  int n = 0;
  if (int rc = check_shape(B, H, W, &n)) return rc;
  *bytes = (int64_t)ddeval::workspace_bytes(B, n);
  return DD_OK;
}

int dd_depth_metric_sums(const float* pred, const float* gt, double* sums, void* workspace, int B, int H, int W, float t_valid, int reduce,
                         void* stream) {
  if (!pred || !gt || !sums || !workspace) return g_eval_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  int n = 0;
  if (int rc = check_shape(B, H, W, &n)) return rc;
  if (int rc = check_reduce(&reduce)) return rc;
  DD_STATUS_HIP(g_eval_err, ddeval::launch_metric_sums(pred, gt, sums, workspace, B, n, t_valid, reduce, (hipStream_t)stream));
  return DD_OK;
}

int dd_depth_metrics(const double* sums, float* batch_metrics, float* image_metrics, int B, void* stream) {
  if (!sums || (!batch_metrics && !image_metrics)) return g_eval_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if (B < 1) return g_eval_err.fail(DD_ERR_INVALID_ARG, "B must be positive (got %d)", B);
  DD_STATUS_HIP(g_eval_err, ddeval::launch_metric_finalize(sums, batch_metrics, image_metrics, B, (hipStream_t)stream));
  return DD_OK;
}

int dd_sup_loss_forward(const float* pred, const float* gt, float* loss, double* sums, void* workspace, int B, int H, int W, float max_depth,
                        float t_valid, int reduce, void* stream) {
  if (!pred || !gt || !loss || !sums || !workspace) return g_eval_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  int n = 0;
  if (int rc = check_shape(B, H, W, &n)) return rc;
  if (int rc = check_reduce(&reduce)) return rc;
  if (!(max_depth >= 0.0f)) return g_eval_err.fail(DD_ERR_INVALID_ARG, "max_depth must be >= 0 (got %g)", (double)max_depth);
  DD_STATUS_HIP(g_eval_err, ddeval::launch_loss_forward(pred, gt, loss, sums, workspace, B, n, max_depth, t_valid, reduce, (hipStream_t)stream));
  return DD_OK;
}

int dd_sup_loss_backward(const float* pred, const float* gt, const double* sums, const float* grad_l1, const float* grad_l2, float* grad_pred,
                         int B, int H, int W, float max_depth, float t_valid, void* stream) {
  if (!pred || !gt || !sums || !grad_pred) return g_eval_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  int n = 0;
  if (int rc = check_shape(B, H, W, &n)) return rc;
  if (!(max_depth >= 0.0f)) return g_eval_err.fail(DD_ERR_INVALID_ARG, "max_depth must be >= 0 (got %g)", (double)max_depth);
  DD_STATUS_HIP(g_eval_err, ddeval::launch_loss_backward(pred, gt, sums, grad_l1, grad_l2, grad_pred, B, n, max_depth, t_valid, (hipStream_t)stream));
  return DD_OK;
}

}  // extern "C"
