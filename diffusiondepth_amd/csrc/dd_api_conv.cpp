// dd_api_conv.cpp -- the C ABI of include/ddepth_conv.h: argument checks and the launch sequence; the kernels are in dd_conv.hip.
#include "../../include/ddepth.h"
#include "../../include/ddepth_conv.h"
#include "dd_conv.h"

#include <climits>
#include <cstdarg>
#include <cstdio>
#include <string>

namespace {

thread_local std::string g_conv_err;

int conv_fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_conv_err = buf;
  return code;
}

#define CONV_HIP(expr)                                                                            \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) return conv_fail(DD_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e));   \
  } while (0)

// dd_precision -> operand mode of the kernels, or -1
int kernel_prec(int precision) {
  switch (precision) {
    case DD_PREC_BF16: return ddconv::kPrecBf16;
    case DD_PREC_F16: return ddconv::kPrecF16;
    case DD_PREC_F16X3: return ddconv::kPrecF16x3;
    default: return -1;
  }
}

bool channels_ok(int c) { return c >= 64 && c <= 1536 && c % 64 == 0; }      // the block-64 contract of dd_conv_* / dd_conv3x3_* / ...

bool channels_any_ok(int c) { return c >= 8 && c <= 2048 && c % 8 == 0; }      // the extended contract of dd_convx_*

bool op_ok(int op) { return op == DD_CONV_3X3 || op == DD_CONV_DECONV2X2 || op == DD_CONV_1X1; }

// everything but the pointers; leaves the kernels' mode in *prec.  any: the extended channel contract
int check(int op, int B, int Cin, int Cout, int H, int W, int precision, int* prec, bool any = false) {
  if (!op_ok(op)) return conv_fail(DD_ERR_INVALID_ARG, "op must be a dd_conv_op value (got %d)", op);
  *prec = kernel_prec(precision);
  if (*prec < 0)
    return conv_fail(DD_ERR_UNSUPPORTED, "precision %d is unsupported: this operator runs DD_PREC_BF16, DD_PREC_F16 and DD_PREC_F16X3", precision);
  if (any && (!channels_any_ok(Cin) || !channels_any_ok(Cout)))
    return conv_fail(DD_ERR_UNSUPPORTED, "Cin = %d, Cout = %d are unsupported: multiples of 8 in 8..2048", Cin, Cout);
  if (!any && (!channels_ok(Cin) || !channels_ok(Cout)))
    return conv_fail(DD_ERR_UNSUPPORTED, "Cin = %d, Cout = %d are unsupported: multiples of 64 in 64..1536", Cin, Cout);
  if (B < 1 || H < 1 || W < 1) return conv_fail(DD_ERR_INVALID_ARG, "B, H, W must be positive (got %d, %d, %d)", B, H, W);
  if (B > 65535) return conv_fail(DD_ERR_INVALID_ARG, "B = %d: at most 65535 per call", B);
  // the larger side of the transpose convolution is (2H, 2W); a plane and the tile grid stay inside int
  if ((int64_t)H * (int64_t)W > (int64_t)INT_MAX / 4 || H > INT_MAX / 4 || W > INT_MAX / 4)
    return conv_fail(DD_ERR_INVALID_ARG, "H = %d, W = %d: 4 * H * W must fit an int", H, W);
  return DD_OK;
}

int check_ptrs(const void* a, const void* b, const void* out, const void* ws) {
  if (!a || !b || !out || !ws) return conv_fail(DD_ERR_INVALID_ARG, "null pointer");
  if (out == a || out == b) return conv_fail(DD_ERR_INVALID_ARG, "the output may not alias an input");
  if (((uintptr_t)ws & 15) != 0) return conv_fail(DD_ERR_INVALID_ARG, "the workspace must be 16-byte aligned");
  return DD_OK;
}

int run_conv(int op, int dir, const float* in, const float* w, float* out, void* ws, int B, int Cin, int Cout, int H, int W, int precision,
             void* stream, bool any = false) {
  int prec = 0;
  if (int rc = check(op, B, Cin, Cout, H, W, precision, &prec, any)) return rc;
  if (int rc = check_ptrs(in, w, out, ws)) return rc;
  CONV_HIP(ddconv::launch_conv(op, dir, in, w, out, ws, B, Cin, Cout, H, W, prec, (hipStream_t)stream));
  return DD_OK;
}

int run_wgrad(int op, const float* x, const float* grad_y, float* grad_w, void* ws, int B, int Cin, int Cout, int H, int W, int precision,
              void* stream, bool any = false) {
  int prec = 0;
  if (int rc = check(op, B, Cin, Cout, H, W, precision, &prec, any)) return rc;
  if (int rc = check_ptrs(x, grad_y, grad_w, ws)) return rc;
  CONV_HIP(ddconv::launch_wgrad(op, x, grad_y, grad_w, ws, B, Cin, Cout, H, W, prec, (hipStream_t)stream));
  return DD_OK;
}

}  // namespace

extern "C" {

const char* dd_conv_last_error(void) { return g_conv_err.c_str(); }

int dd_conv_supported(int op, int Cin, int Cout, int precision) {
  return (op_ok(op) && kernel_prec(precision) >= 0 && channels_ok(Cin) && channels_ok(Cout)) ? 1 : 0;
}

int dd_conv_workspace_bytes(int op, int B, int Cin, int Cout, int H, int W, int precision, int64_t* bytes) {
  if (!bytes) return conv_fail(DD_ERR_INVALID_ARG, "bytes is NULL");
  int prec = 0;
  if (int rc = check(op, B, Cin, Cout, H, W, precision, &prec)) return rc;
  *bytes = (int64_t)ddconv::workspace_bytes(op, B, Cin, Cout, H, W, prec);
  return DD_OK;
}

int dd_conv3x3_forward(const float* x, const float* w, float* y, void* workspace, int B, int Cin, int Cout, int H, int W, int precision,
                       void* stream) {
  return run_conv(DD_CONV_3X3, 0, x, w, y, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_conv3x3_backward_data(const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int Cin, int Cout, int H, int W,
                             int precision, void* stream) {
  return run_conv(DD_CONV_3X3, 1, grad_y, w, grad_x, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_conv3x3_backward_weight(const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H, int W,
                               int precision, void* stream) {
  return run_wgrad(DD_CONV_3X3, x, grad_y, grad_w, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_deconv2x2_forward(const float* x, const float* w, float* y, void* workspace, int B, int Cin, int Cout, int H, int W, int precision,
                         void* stream) {
  return run_conv(DD_CONV_DECONV2X2, 0, x, w, y, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_deconv2x2_backward_data(const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int Cin, int Cout, int H, int W,
                               int precision, void* stream) {
  return run_conv(DD_CONV_DECONV2X2, 1, grad_y, w, grad_x, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_deconv2x2_backward_weight(const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H,
                                 int W, int precision, void* stream) {
  return run_wgrad(DD_CONV_DECONV2X2, x, grad_y, grad_w, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_conv1x1_forward(const float* x, const float* w, float* y, void* workspace, int B, int Cin, int Cout, int H, int W, int precision,
                       void* stream) {
  return run_conv(DD_CONV_1X1, 0, x, w, y, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_conv1x1_backward_data(const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int Cin, int Cout, int H, int W,
                             int precision, void* stream) {
  return run_conv(DD_CONV_1X1, 1, grad_y, w, grad_x, workspace, B, Cin, Cout, H, W, precision, stream);
}

int dd_conv1x1_backward_weight(const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H, int W,
                               int precision, void* stream) {
  return run_wgrad(DD_CONV_1X1, x, grad_y, grad_w, workspace, B, Cin, Cout, H, W, precision, stream);
}

// ---- the extended channel range: multiples of 8 in 8..2048 (a block-64 shape runs exactly what the functions above run) ----------------------
int dd_convx_supported(int op, int Cin, int Cout, int precision) {
  return (op_ok(op) && kernel_prec(precision) >= 0 && channels_any_ok(Cin) && channels_any_ok(Cout)) ? 1 : 0;
}

int dd_convx_workspace_bytes(int op, int B, int Cin, int Cout, int H, int W, int precision, int64_t* bytes) {
  if (!bytes) return conv_fail(DD_ERR_INVALID_ARG, "bytes is NULL");
  int prec = 0;
  if (int rc = check(op, B, Cin, Cout, H, W, precision, &prec, true)) return rc;
  *bytes = (int64_t)ddconv::workspace_bytes(op, B, Cin, Cout, H, W, prec);
  return DD_OK;
}

int dd_convx_forward(int op, const float* x, const float* w, float* y, void* workspace, int B, int Cin, int Cout, int H, int W, int precision,
                     void* stream) {
  return run_conv(op, 0, x, w, y, workspace, B, Cin, Cout, H, W, precision, stream, true);
}

int dd_convx_backward_data(int op, const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int Cin, int Cout, int H, int W,
                           int precision, void* stream) {
  return run_conv(op, 1, grad_y, w, grad_x, workspace, B, Cin, Cout, H, W, precision, stream, true);
}

int dd_convx_backward_weight(int op, const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H, int W,
                             int precision, void* stream) {
  return run_wgrad(op, x, grad_y, grad_w, workspace, B, Cin, Cout, H, W, precision, stream, true);
}

}  // extern "C"
