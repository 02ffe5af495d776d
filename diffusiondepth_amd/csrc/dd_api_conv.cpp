// dd_api_conv.cpp -- the C ABI of include/ddepth_conv.h, include/ddepth_conv_scaled.h, include/ddepth_conv_strided.h, include/ddepth_conv_fused.h and
// include/ddepth_conv_stats.h:
// argument checks and the launch sequence; the kernels are in dd_conv.hip.
#include "../../include/ddepth.h"
#include "../../include/ddepth_conv.h"
#include "../../include/ddepth_conv_scaled.h"
#include "../../include/ddepth_conv_strided.h"
#include "../../include/ddepth_conv_fused.h"
#include "../../include/ddepth_conv_stats.h"
#include "dd_conv.h"
#include "dd_status.h"

#include <climits>

namespace {

thread_local ddstatus::LastError g_conv_err;

// dd_precision -> operand mode of the kernels, or -1
int kernel_prec(int precision) {
  switch (precision) {
    case DD_PREC_BF16: return ddconv::kPrecBf16;
    case DD_PREC_F16: return ddconv::kPrecF16;
    case DD_PREC_F16X3: return ddconv::kPrecF16x3;
    default: return -1;
  }
}

using ddconv::ChannelContract;
using ddconv::kChannelsBlock64;
using ddconv::kChannelsExtended;

bool op_ok(int op) { return op == DD_CONV_3X3 || op == DD_CONV_DECONV2X2 || op == DD_CONV_1X1; }

// everything but the pointers; leaves the kernels' mode in *prec
int check(ChannelContract contract, int op, int B, int Cin, int Cout, int H, int W, int precision, int* prec) {
  if (!op_ok(op)) return g_conv_err.fail(DD_ERR_INVALID_ARG, "op must be a dd_conv_op value (got %d)", op);
  *prec = kernel_prec(precision);
  if (*prec < 0)
    return g_conv_err.fail(DD_ERR_UNSUPPORTED, "precision %d is unsupported: this operator runs DD_PREC_BF16, DD_PREC_F16 and DD_PREC_F16X3", precision);
  if (!ddconv::channels_ok(contract, Cin) || !ddconv::channels_ok(contract, Cout))
    return g_conv_err.fail(DD_ERR_UNSUPPORTED, "Cin = %d, Cout = %d are unsupported: %s", Cin, Cout,
                           contract == kChannelsExtended ? "multiples of 8 in 8..2048" : "multiples of 64 in 64..1536");
  if (B < 1 || H < 1 || W < 1) return g_conv_err.fail(DD_ERR_INVALID_ARG, "B, H, W must be positive (got %d, %d, %d)", B, H, W);
  if (B > 65535) return g_conv_err.fail(DD_ERR_INVALID_ARG, "B = %d: at most 65535 per call", B);
  // the larger side of the transpose convolution is (2H, 2W); a plane and the tile grid stay inside int
  if ((int64_t)H * (int64_t)W > (int64_t)INT_MAX / 4 || H > INT_MAX / 4 || W > INT_MAX / 4)
    return g_conv_err.fail(DD_ERR_INVALID_ARG, "H = %d, W = %d: 4 * H * W must fit an int", H, W);
  return DD_OK;
}

int supported(ChannelContract contract, int op, int Cin, int Cout, int precision) {
  return (op_ok(op) && kernel_prec(precision) >= 0 && ddconv::channels_ok(contract, Cin) && ddconv::channels_ok(contract, Cout)) ? 1 : 0;
}

int workspace_bytes(ChannelContract contract, int op, int B, int Cin, int Cout, int H, int W, int precision, int64_t* bytes) {
  if (!bytes) return g_conv_err.fail(DD_ERR_INVALID_ARG, "bytes is NULL");
  int prec = 0;
  if (int rc = check(contract, op, B, Cin, Cout, H, W, precision, &prec)) return rc;
  *bytes = (int64_t)ddconv::workspace_bytes(op, B, Cin, Cout, H, W, prec);
  return DD_OK;
}

// scale: NULL for the functions of ddepth_conv.h, the device pair of dd_conv_grad_scale for those of ddepth_conv_scaled.h (`scaled`)
int run_conv(ChannelContract contract, int op, int dir, const float* in, const float* w, float* out, void* ws, int B, int Cin, int Cout, int H,
             int W, int precision, void* stream, bool scaled = false, const float* scale = nullptr) {
  int prec = 0;
  if (int rc = check(contract, op, B, Cin, Cout, H, W, precision, &prec)) return rc;
  if (int rc = ddstatus::check_ptrs(g_conv_err, in, w, out, ws)) return rc;
  if (scaled && !scale) return g_conv_err.fail(DD_ERR_INVALID_ARG, "scale is NULL");
  DD_STATUS_HIP(g_conv_err, ddconv::launch_conv(op, dir, in, w, out, ws, B, Cin, Cout, H, W, prec, (hipStream_t)stream, scale));
  return DD_OK;
}

int run_wgrad(ChannelContract contract, int op, const float* x, const float* grad_y, float* grad_w, void* ws, int B, int Cin, int Cout, int H,
              int W, int precision, void* stream, bool scaled = false, const float* scale = nullptr) {
  int prec = 0;
  if (int rc = check(contract, op, B, Cin, Cout, H, W, precision, &prec)) return rc;
  if (int rc = ddstatus::check_ptrs(g_conv_err, x, grad_y, grad_w, ws)) return rc;
  if (scaled && !scale) return g_conv_err.fail(DD_ERR_INVALID_ARG, "scale is NULL");
  DD_STATUS_HIP(g_conv_err, ddconv::launch_wgrad(op, x, grad_y, grad_w, ws, B, Cin, Cout, H, W, prec, (hipStream_t)stream, scale));
  return DD_OK;
}

// include/ddepth_conv_strided.h: everything but the pointers; leaves the kernels' mode in *prec
int check_s2(int B, int Cin, int Cout, int H, int W, int precision, int* prec) {
  *prec = kernel_prec(precision);
  if (*prec < 0)
    return g_conv_err.fail(DD_ERR_UNSUPPORTED, "precision %d is unsupported: this operator runs DD_PREC_BF16, DD_PREC_F16 and DD_PREC_F16X3", precision);
  if (!ddconv::channels_s2_in(Cin) || !ddconv::channels_extended(Cout))
    return g_conv_err.fail(DD_ERR_UNSUPPORTED, "Cin = %d, Cout = %d are unsupported: Cout a multiple of 8 in 8..2048, Cin 3 or a multiple of 8 in 8..2048",
                           Cin, Cout);
  if (B < 1 || H < 1 || W < 1) return g_conv_err.fail(DD_ERR_INVALID_ARG, "B, H, W must be positive (got %d, %d, %d)", B, H, W);
  if (B > 65535) return g_conv_err.fail(DD_ERR_INVALID_ARG, "B = %d: at most 65535 per call", B);
  if ((int64_t)H * (int64_t)W > (int64_t)INT_MAX / 4 || H > INT_MAX / 4 || W > INT_MAX / 4)
    return g_conv_err.fail(DD_ERR_INVALID_ARG, "H = %d, W = %d: 4 * H * W must fit an int", H, W);
  return DD_OK;
}

// include/ddepth_conv_fused.h: the checks of the stride's own operator
int check_affine(int stride, int B, int Cin, int Cout, int H, int W, int precision, int* prec) {
  if (stride == 1) return check(kChannelsExtended, DD_CONV_3X3, B, Cin, Cout, H, W, precision, prec);
  if (stride == 2) return check_s2(B, Cin, Cout, H, W, precision, prec);
  return g_conv_err.fail(DD_ERR_INVALID_ARG, "stride must be 1 or 2 (got %d)", stride);
}

}  // namespace

extern "C" {

const char* dd_conv_last_error(void) { return g_conv_err.text.c_str(); }

int dd_conv_supported(int op, int Cin, int Cout, int precision) { return supported(kChannelsBlock64, op, Cin, Cout, precision); }

int dd_conv_workspace_bytes(int op, int B, int Cin, int Cout, int H, int W, int precision, int64_t* bytes) {
  return workspace_bytes(kChannelsBlock64, op, B, Cin, Cout, H, W, precision, bytes);
}

int dd_conv3x3_forward(const float* x, const float* w, float* y, void* workspace, int B, int Cin, int Cout, int H, int W, int precision,
                       void* stream) {
  return run_conv(kChannelsBlock64, DD_CONV_3X3, 0, x, w, y, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_conv3x3_backward_data(const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int Cin, int Cout, int H, int W,
                             int precision, void* stream) {
  return run_conv(kChannelsBlock64, DD_CONV_3X3, 1, grad_y, w, grad_x, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_conv3x3_backward_weight(const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H, int W,
                               int precision, void* stream) {
  return run_wgrad(kChannelsBlock64, DD_CONV_3X3, x, grad_y, grad_w, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_deconv2x2_forward(const float* x, const float* w, float* y, void* workspace, int B, int Cin, int Cout, int H, int W, int precision,
                         void* stream) {
  return run_conv(kChannelsBlock64, DD_CONV_DECONV2X2, 0, x, w, y, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_deconv2x2_backward_data(const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int Cin, int Cout, int H, int W,
                               int precision, void* stream) {
  return run_conv(kChannelsBlock64, DD_CONV_DECONV2X2, 1, grad_y, w, grad_x, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_deconv2x2_backward_weight(const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H,
                                 int W, int precision, void* stream) {
  return run_wgrad(kChannelsBlock64, DD_CONV_DECONV2X2, x, grad_y, grad_w, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_conv1x1_forward(const float* x, const float* w, float* y, void* workspace, int B, int Cin, int Cout, int H, int W, int precision,
                       void* stream) {
  return run_conv(kChannelsBlock64, DD_CONV_1X1, 0, x, w, y, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_conv1x1_backward_data(const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int Cin, int Cout, int H, int W,
                             int precision, void* stream) {
  return run_conv(kChannelsBlock64, DD_CONV_1X1, 1, grad_y, w, grad_x, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_conv1x1_backward_weight(const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H, int W,
                               int precision, void* stream) {
  return run_wgrad(kChannelsBlock64, DD_CONV_1X1, x, grad_y, grad_w, workspace, B, Cin, Cout, H, W, precision, stream);
}

// ---- the extended channel range: multiples of 8 in 8..2048 (a block-64 shape runs exactly what the functions above run) ----------------------
int dd_convx_supported(int op, int Cin, int Cout, int precision) { return supported(kChannelsExtended, op, Cin, Cout, precision); }

int dd_convx_workspace_bytes(int op, int B, int Cin, int Cout, int H, int W, int precision, int64_t* bytes) {
  return workspace_bytes(kChannelsExtended, op, B, Cin, Cout, H, W, precision, bytes);
}

int dd_convx_forward(int op, const float* x, const float* w, float* y, void* workspace, int B, int Cin, int Cout, int H, int W, int precision,
                     void* stream) {
  return run_conv(kChannelsExtended, op, 0, x, w, y, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_convx_backward_data(int op, const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int Cin, int Cout, int H, int W,
                           int precision, void* stream) {
  return run_conv(kChannelsExtended, op, 1, grad_y, w, grad_x, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_convx_backward_weight(int op, const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H, int W,
                             int precision, void* stream) {
  return run_wgrad(kChannelsExtended, op, x, grad_y, grad_w, workspace, B, Cin, Cout, H, W, precision, stream);
}

// ---- include/ddepth_conv_scaled.h: the two gradients on grad_y rescaled by a power of two ------------------------------------------------------
int dd_conv_grad_scale(const float* grad_y, int64_t n, int precision, float* scale, void* stream) {
  const int prec = kernel_prec(precision);
  if (prec < 0)
    return g_conv_err.fail(DD_ERR_UNSUPPORTED, "precision %d is unsupported: this operator runs DD_PREC_BF16, DD_PREC_F16 and DD_PREC_F16X3", precision);
  if (!scale) return g_conv_err.fail(DD_ERR_INVALID_ARG, "scale is NULL");
  if (n < 0 || (n > 0 && !grad_y)) return g_conv_err.fail(DD_ERR_INVALID_ARG, "grad_y is NULL or n = %lld is negative", (long long)n);
  if ((const void*)grad_y == (const void*)scale) return g_conv_err.fail(DD_ERR_INVALID_ARG, "the output may not alias an input");
  DD_STATUS_HIP(g_conv_err, ddconv::launch_grad_scale(grad_y, n, prec, ddconv::kGradAmaxExp, scale, (hipStream_t)stream));
  return DD_OK;
}

int dd_convx_backward_data_scaled(int op, const float* grad_y, const float* w, float* grad_x, void* workspace, const float* scale, int B, int Cin,
                                  int Cout, int H, int W, int precision, void* stream) {
  return run_conv(kChannelsExtended, op, 1, grad_y, w, grad_x, workspace, B, Cin, Cout, H, W, precision, stream, true, scale);
}

int dd_convx_backward_weight_scaled(int op, const float* x, const float* grad_y, float* grad_w, void* workspace, const float* scale, int B, int Cin,
                                    int Cout, int H, int W, int precision, void* stream) {
  return run_wgrad(kChannelsExtended, op, x, grad_y, grad_w, workspace, B, Cin, Cout, H, W, precision, stream, true, scale);
}

// ---- include/ddepth_conv_strided.h: 3x3 stride 2 pad 1, optional bias ----------------------------------------------------------------------------------
int dd_conv3x3s2_supported(int Cin, int Cout, int precision) {
  return (kernel_prec(precision) >= 0 && ddconv::channels_s2_in(Cin) && ddconv::channels_extended(Cout)) ? 1 : 0;
}

int dd_conv3x3s2_workspace_bytes(int B, int Cin, int Cout, int H, int W, int precision, int64_t* bytes) {
  if (!bytes) return g_conv_err.fail(DD_ERR_INVALID_ARG, "bytes is NULL");
  int prec = 0;
  if (int rc = check_s2(B, Cin, Cout, H, W, precision, &prec)) return rc;
  *bytes = (int64_t)ddconv::workspace_bytes_s2(B, Cin, Cout, H, W, prec);
  return DD_OK;
}

int dd_conv3x3s2_forward(const float* x, const float* w, const float* bias, float* y, void* workspace, int B, int Cin, int Cout, int H, int W,
                         int precision, void* stream) {
  int prec = 0;
  if (int rc = check_s2(B, Cin, Cout, H, W, precision, &prec)) return rc;
  if (int rc = ddstatus::check_ptrs(g_conv_err, x, w, y, workspace)) return rc;
  if (bias && (const void*)bias == (const void*)y) return g_conv_err.fail(DD_ERR_INVALID_ARG, "the output may not alias an input");
  DD_STATUS_HIP(g_conv_err, ddconv::launch_conv_s2_forward(x, w, bias, y, workspace, B, Cin, Cout, H, W, prec, (hipStream_t)stream));
  return DD_OK;
}

int dd_conv3x3s2_backward_data(const float* grad_y, const float* w, float* grad_x, void* workspace, const float* scale, int B, int Cin, int Cout,
                               int H, int W, int precision, void* stream) {
  int prec = 0;
  if (int rc = check_s2(B, Cin, Cout, H, W, precision, &prec)) return rc;
  if (int rc = ddstatus::check_ptrs(g_conv_err, grad_y, w, grad_x, workspace)) return rc;
  DD_STATUS_HIP(g_conv_err, ddconv::launch_conv_s2_dgrad(grad_y, w, grad_x, workspace, B, Cin, Cout, H, W, prec, (hipStream_t)stream, scale));
  return DD_OK;
}

int dd_conv3x3s2_backward_weight(const float* x, const float* grad_y, float* grad_w, float* grad_bias, void* workspace, const float* scale, int B,
                                 int Cin, int Cout, int H, int W, int precision, void* stream) {
  int prec = 0;
  if (int rc = check_s2(B, Cin, Cout, H, W, precision, &prec)) return rc;
  if (int rc = ddstatus::check_ptrs(g_conv_err, x, grad_y, grad_w, workspace)) return rc;
  if (grad_bias && ((const void*)grad_bias == (const void*)x || (const void*)grad_bias == (const void*)grad_y || grad_bias == grad_w))
    return g_conv_err.fail(DD_ERR_INVALID_ARG, "the output may not alias an input");
  DD_STATUS_HIP(g_conv_err,
                ddconv::launch_conv_s2_wgrad(x, grad_y, grad_w, grad_bias, workspace, B, Cin, Cout, H, W, prec, (hipStream_t)stream, scale));
  return DD_OK;
}

// ---- include/ddepth_conv_fused.h: the folded eval-mode forward, 3x3 pad 1, stride 1 or 2 ------------------------------------------------------------
int dd_bn_fold(const float* weight, const float* bias, const float* running_mean, const float* running_var, double eps, const float* conv_bias,
               float* scale_shift, int C, void* stream) {
  if (!scale_shift) return g_conv_err.fail(DD_ERR_INVALID_ARG, "scale_shift is NULL");
  if (C < 1) return g_conv_err.fail(DD_ERR_INVALID_ARG, "C must be positive (got %d)", C);
  if ((running_mean == nullptr) != (running_var == nullptr))
    return g_conv_err.fail(DD_ERR_INVALID_ARG, "running_mean and running_var must both be given, or both be NULL");
  if (!(eps >= 0.0)) return g_conv_err.fail(DD_ERR_INVALID_ARG, "eps must not be negative (got %g)", eps);
  for (const float* p : {weight, bias, running_mean, running_var, conv_bias})
    if (p && p == scale_shift) return g_conv_err.fail(DD_ERR_INVALID_ARG, "the output may not alias an input");
  DD_STATUS_HIP(g_conv_err, ddconv::launch_bn_fold(weight, bias, running_mean, running_var, eps, conv_bias, scale_shift, C, (hipStream_t)stream));
  return DD_OK;
}

int dd_conv3x3_affine_supported(int stride, int Cin, int Cout, int precision) {
  if (stride == 1) return supported(kChannelsExtended, DD_CONV_3X3, Cin, Cout, precision);
  return stride == 2 ? dd_conv3x3s2_supported(Cin, Cout, precision) : 0;
}

int dd_conv3x3_affine_workspace_bytes(int stride, int B, int Cin, int Cout, int H, int W, int precision, int64_t* bytes) {
  if (!bytes) return g_conv_err.fail(DD_ERR_INVALID_ARG, "bytes is NULL");
  int prec = 0;
  if (int rc = check_affine(stride, B, Cin, Cout, H, W, precision, &prec)) return rc;
  *bytes = (int64_t)ddconv::workspace_bytes_affine(stride, Cin, Cout, prec);
  return DD_OK;
}

int dd_conv3x3_affine_forward(const float* x, const float* w, const float* scale_shift, const float* addend, float* y, void* workspace, int stride,
                              int relu, int B, int Cin, int Cout, int H, int W, int precision, void* stream) {
  int prec = 0;
  if (int rc = check_affine(stride, B, Cin, Cout, H, W, precision, &prec)) return rc;
  if (int rc = ddstatus::check_ptrs(g_conv_err, x, w, y, workspace)) return rc;
  if (!scale_shift) return g_conv_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if ((const void*)scale_shift == (const void*)y || (addend && (const void*)addend == (const void*)y))
    return g_conv_err.fail(DD_ERR_INVALID_ARG, "the output may not alias an input");
  if (relu != 0 && relu != 1) return g_conv_err.fail(DD_ERR_INVALID_ARG, "relu must be 0 or 1 (got %d)", relu);
  DD_STATUS_HIP(g_conv_err, ddconv::launch_conv_affine(stride, x, w, scale_shift, addend, y, workspace, relu, B, Cin, Cout, H, W, prec,
                                                       (hipStream_t)stream));
  return DD_OK;
}

// ---- include/ddepth_conv_stats.h: the training forward that emits the BatchNorm statistics, 3x3 pad 1, stride 1 or 2 --------------------------------
int dd_conv3x3_stats_supported(int stride, int Cin, int Cout, int precision) { return dd_conv3x3_affine_supported(stride, Cin, Cout, precision); }

int dd_conv3x3_stats_workspace_bytes(int stride, int B, int Cin, int Cout, int H, int W, int precision, int64_t* bytes) {
  if (!bytes) return g_conv_err.fail(DD_ERR_INVALID_ARG, "bytes is NULL");
  int prec = 0;
  if (int rc = check_affine(stride, B, Cin, Cout, H, W, precision, &prec)) return rc;
  *bytes = (int64_t)ddconv::workspace_bytes_stats(stride, B, Cin, Cout, H, W, prec);
  return DD_OK;
}

int dd_conv3x3_stats_forward(const float* x, const float* w, const float* bias, float* y, double* sums, void* workspace, int stride, int B, int Cin,
                             int Cout, int H, int W, int precision, void* stream) {
  int prec = 0;
  if (int rc = check_affine(stride, B, Cin, Cout, H, W, precision, &prec)) return rc;
  if (int rc = ddstatus::check_ptrs(g_conv_err, x, w, y, workspace)) return rc;
  if (!sums) return g_conv_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  for (const void* p : {(const void*)x, (const void*)w, (const void*)bias})
    if (p && (p == (const void*)y || p == (const void*)sums)) return g_conv_err.fail(DD_ERR_INVALID_ARG, "the output may not alias an input");
  if ((const void*)sums == (const void*)y) return g_conv_err.fail(DD_ERR_INVALID_ARG, "the outputs may not alias each other");
  DD_STATUS_HIP(g_conv_err, ddconv::launch_conv_stats(stride, x, w, bias, y, sums, workspace, B, Cin, Cout, H, W, prec, (hipStream_t)stream));
  return DD_OK;
}

}  // extern "C"
