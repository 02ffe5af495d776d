// dd_api_bn.cpp -- the C ABI of include/ddepth_bn.h and include/ddepth_bn_add.h: argument checks and the launch sequence; the kernels are in dd_bn.hip.
#include "../../include/ddepth.h"
#include "../../include/ddepth_bn.h"
#include "../../include/ddepth_bn_add.h"
#include "dd_bn.h"
#include "dd_status.h"

#include <climits>
#include <cmath>

namespace {

thread_local ddstatus::LastError g_bn_err;

int check_shape(int B, int C, int HW) {
  if (B < 1 || C < 1 || HW < 1) return g_bn_err.fail(DD_ERR_INVALID_ARG, "B, C, HW must be positive (got %d, %d, %d)", B, C, HW);
  if (B > 65535 || C > 65535) return g_bn_err.fail(DD_ERR_INVALID_ARG, "B = %d, C = %d: at most 65535 each per call", B, C);
  return DD_OK;
}

int check_act(int act, float slope) {
  if (act != DD_BN_ACT_NONE && act != DD_BN_ACT_RELU && act != DD_BN_ACT_LEAKY_RELU)
    return g_bn_err.fail(DD_ERR_INVALID_ARG, "act must be a dd_bn_act value (got %d)", act);
  if (act == DD_BN_ACT_LEAKY_RELU && !std::isfinite(slope)) return g_bn_err.fail(DD_ERR_INVALID_ARG, "slope must be finite");
  return DD_OK;
}

}  // namespace

extern "C" {

const char* dd_bn_last_error(void) { return g_bn_err.text.c_str(); }

int dd_bn_workspace_bytes(int B, int C, int HW, int64_t* bytes) {
  if (!bytes) return g_bn_err.fail(DD_ERR_INVALID_ARG, "bytes is NULL");
  if (int rc = check_shape(B, C, HW)) return rc;
  *bytes = (int64_t)ddbn::workspace_bytes(B, C, HW);
  return DD_OK;
}

int dd_bn_stats(const float* x, double* sums, void* workspace, int B, int C, int HW, void* stream) {
  if (!x || !sums || !workspace) return g_bn_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_shape(B, C, HW)) return rc;
  DD_STATUS_HIP(g_bn_err, ddbn::launch_stats(x, sums, workspace, B, C, HW, (hipStream_t)stream));
  return DD_OK;
}

int dd_bn_finalize(const double* sums, float eps, float momentum, float* mean_invstd, float* running_mean, float* running_var, int C,
                   void* stream) {
  if (!sums || !mean_invstd) return g_bn_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if ((running_mean == nullptr) != (running_var == nullptr))
    return g_bn_err.fail(DD_ERR_INVALID_ARG, "running_mean and running_var: both or neither");
  if (C < 1 || C > 65535) return g_bn_err.fail(DD_ERR_INVALID_ARG, "C must be in 1..65535 (got %d)", C);
  if (!(eps >= 0.0f)) return g_bn_err.fail(DD_ERR_INVALID_ARG, "eps must be >= 0 (got %g)", (double)eps);
  DD_STATUS_HIP(g_bn_err, ddbn::launch_finalize(sums, eps, momentum, mean_invstd, running_mean, running_var, C, (hipStream_t)stream));
  return DD_OK;
}

int dd_bn_apply(const float* x, const float* mean_invstd, const float* weight, const float* bias, float* y, int act, float slope, int B,
                int C, int HW, void* stream) {
  if (!x || !mean_invstd || !y) return g_bn_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if (x == y) return g_bn_err.fail(DD_ERR_INVALID_ARG, "y may not alias x (the backward reads x)");
  if (int rc = check_shape(B, C, HW)) return rc;
  if (int rc = check_act(act, slope)) return rc;
  DD_STATUS_HIP(g_bn_err, ddbn::launch_apply(x, mean_invstd, weight, bias, y, act, slope, B, C, HW, (hipStream_t)stream));
  return DD_OK;
}

int dd_bn_backward_reduce(const float* x, const float* grad_y, const float* mean_invstd, const float* weight, const float* bias, int act,
                          float slope, double* sums2, void* workspace, int B, int C, int HW, void* stream) {
  if (!x || !grad_y || !mean_invstd || !sums2 || !workspace) return g_bn_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if (int rc = check_shape(B, C, HW)) return rc;
  if (int rc = check_act(act, slope)) return rc;
  DD_STATUS_HIP(g_bn_err, ddbn::launch_backward_reduce(x, grad_y, mean_invstd, weight, bias, act, slope, sums2, workspace, B, C, HW, (hipStream_t)stream));
  return DD_OK;
}

int dd_bn_backward_apply(const float* x, const float* grad_y, const float* mean_invstd, const float* weight, const float* bias,
                         const double* sums2, const double* sums, float* grad_x, int act, float slope, int B, int C, int HW, void* stream) {
  if (!x || !grad_y || !mean_invstd || !sums2 || !sums || !grad_x) return g_bn_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if (grad_x == x || grad_x == grad_y) return g_bn_err.fail(DD_ERR_INVALID_ARG, "grad_x may not alias x or grad_y");
  if (int rc = check_shape(B, C, HW)) return rc;
  if (int rc = check_act(act, slope)) return rc;
  DD_STATUS_HIP(g_bn_err, ddbn::launch_backward_apply(x, grad_y, mean_invstd, weight, bias, sums2, sums, grad_x, act, slope, B, C, HW, (hipStream_t)stream));
  return DD_OK;
}

// ---- include/ddepth_bn_add.h ---------------------------------------------------------------------------------------------------------------
int dd_bn_apply_add(const float* x, const float* mean_invstd, const float* weight, const float* bias, const float* addend, float* y,
                    int act, float slope, int add_mode, int B, int C, int HW, void* stream) {
  if (!x || !mean_invstd || !addend || !y) return g_bn_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if (y == x || y == addend) return g_bn_err.fail(DD_ERR_INVALID_ARG, "y may not alias x or addend");
  if (add_mode != DD_BN_ADD_PRE && add_mode != DD_BN_ADD_POST)
    return g_bn_err.fail(DD_ERR_INVALID_ARG, "add_mode must be a dd_bn_add_mode value (got %d)", add_mode);
  if (int rc = check_shape(B, C, HW)) return rc;
  if (int rc = check_act(act, slope)) return rc;
  DD_STATUS_HIP(g_bn_err, ddbn::launch_apply_add(x, mean_invstd, weight, bias, addend, y, act, slope, add_mode == DD_BN_ADD_POST, B, C, HW,
                                                 (hipStream_t)stream));
  return DD_OK;
}

int dd_bn_backward_reduce_add(const float* x, const float* grad_y, const float* y, const float* mean_invstd, int act, float slope,
                              float* g, double* sums2, void* workspace, int B, int C, int HW, void* stream) {
  if (!x || !grad_y || !y || !mean_invstd || !g || !sums2 || !workspace) return g_bn_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if (g == x || g == grad_y || g == y) return g_bn_err.fail(DD_ERR_INVALID_ARG, "g may not alias x, grad_y or y");
  if (int rc = check_shape(B, C, HW)) return rc;
  if (int rc = check_act(act, slope)) return rc;
  if (act == DD_BN_ACT_LEAKY_RELU && slope < 0.0f)
    return g_bn_err.fail(DD_ERR_UNSUPPORTED, "LeakyReLU with a negative slope (%g): the sign of y is not the sign of z + r", (double)slope);
  DD_STATUS_HIP(g_bn_err, ddbn::launch_backward_reduce_add(x, grad_y, y, mean_invstd, act, slope, g, sums2, workspace, B, C, HW,
                                                           (hipStream_t)stream));
  return DD_OK;
}

}  // extern "C"
