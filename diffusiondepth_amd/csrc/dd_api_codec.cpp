// dd_api_codec.cpp -- the C ABI of include/ddepth_codec.h: argument checks and the launch sequence; the kernels are in dd_codec.hip.
#include "../../include/ddepth.h"
#include "../../include/ddepth_codec.h"
#include "dd_codec.h"
#include "dd_status.h"

#include <climits>

namespace {

thread_local ddstatus::LastError g_codec_err;

bool has_bias(int op) { return op == DD_CODEC_DEC0 || op == DD_CODEC_DEC1; }

int check(int op, int B, int H, int W) {
  if (op < DD_CODEC_ENC0 || op > DD_CODEC_DEC1) return g_codec_err.fail(DD_ERR_INVALID_ARG, "op must be a dd_codec_op value (got %d)", op);
  if (B < 1 || H < 1 || W < 1) return g_codec_err.fail(DD_ERR_INVALID_ARG, "B, H, W must be positive (got %d, %d, %d)", B, H, W);
  if (B > 65535) return g_codec_err.fail(DD_ERR_INVALID_ARG, "B = %d: at most 65535 per call", B);
  // the larger side of the transpose convolution is (2H, 2W); a plane and the tile grid stay inside int
  if ((int64_t)H * (int64_t)W > (int64_t)INT_MAX / 4 || H > INT_MAX / 4 || W > INT_MAX / 4)
    return g_codec_err.fail(DD_ERR_INVALID_ARG, "H = %d, W = %d: 4 * H * W must fit an int", H, W);
  if (op == DD_CODEC_DEC0 && H > 131070) return g_codec_err.fail(DD_ERR_INVALID_ARG, "H = %d: DEC0 takes at most 131070 input rows per call", H);
  return DD_OK;
}

}  // namespace

extern "C" {

const char* dd_codec_last_error(void) { return g_codec_err.text.c_str(); }

int dd_codec_workspace_bytes(int op, int B, int H, int W, int64_t* bytes) {
  if (!bytes) return g_codec_err.fail(DD_ERR_INVALID_ARG, "bytes is NULL");
  if (int rc = check(op, B, H, W)) return rc;
  *bytes = (int64_t)ddcodec::workspace_bytes(op, B, H, W);
  return DD_OK;
}

int dd_codec_conv_forward(int op, const float* x, const float* w, const float* bias, float* y, void* workspace, int B, int H, int W,
                          void* stream) {
  if (int rc = check(op, B, H, W)) return rc;
  if (int rc = ddstatus::check_ptrs(g_codec_err, x, w, y, workspace)) return rc;
  if (bias && !has_bias(op)) return g_codec_err.fail(DD_ERR_INVALID_ARG, "op %d has no bias: bias must be NULL", op);
  if (bias && (const void*)bias == (const void*)y) return g_codec_err.fail(DD_ERR_INVALID_ARG, "the output may not alias an input");
  DD_STATUS_HIP(g_codec_err, ddcodec::launch_conv(op, 0, x, w, bias, y, workspace, B, H, W, (hipStream_t)stream));
  return DD_OK;
}

int dd_codec_conv_backward_data(int op, const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int H, int W, void* stream) {
  if (int rc = check(op, B, H, W)) return rc;
  if (int rc = ddstatus::check_ptrs(g_codec_err, grad_y, w, grad_x, workspace)) return rc;
  DD_STATUS_HIP(g_codec_err, ddcodec::launch_conv(op, 1, grad_y, w, nullptr, grad_x, workspace, B, H, W, (hipStream_t)stream));
  return DD_OK;
}

int dd_codec_conv_backward_weight(int op, const float* x, const float* grad_y, float* grad_w, float* grad_bias, void* workspace, int B, int H,
                                  int W, void* stream) {
  if (int rc = check(op, B, H, W)) return rc;
  if (int rc = ddstatus::check_ptrs(g_codec_err, x, grad_y, grad_w, workspace)) return rc;
  if (grad_bias && !has_bias(op)) return g_codec_err.fail(DD_ERR_INVALID_ARG, "op %d has no bias: grad_bias must be NULL", op);
  if (grad_bias && ((const void*)grad_bias == (const void*)x || (const void*)grad_bias == (const void*)grad_y || grad_bias == grad_w))
    return g_codec_err.fail(DD_ERR_INVALID_ARG, "the output may not alias an input");
  DD_STATUS_HIP(g_codec_err, ddcodec::launch_wgrad(op, x, grad_y, grad_w, grad_bias, workspace, B, H, W, (hipStream_t)stream));
  return DD_OK;
}

int dd_codec_tail_forward(const float* z, float* depth, int64_t n, float eps, void* stream) {
  if (!z || !depth) return g_codec_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if (z == depth) return g_codec_err.fail(DD_ERR_INVALID_ARG, "the output may not alias an input");
  if (n < 1) return g_codec_err.fail(DD_ERR_INVALID_ARG, "n must be positive (got %lld)", (long long)n);
  if (n > (int64_t)1 << 38) return g_codec_err.fail(DD_ERR_INVALID_ARG, "n = %lld: at most 2^38 elements per call", (long long)n);
  DD_STATUS_HIP(g_codec_err, ddcodec::launch_tail_forward(z, depth, n, eps, (hipStream_t)stream));
  return DD_OK;
}

int dd_codec_tail_backward(const float* z, const float* grad_depth, float* grad_z, int64_t n, float eps, void* stream) {
  if (!z || !grad_depth || !grad_z) return g_codec_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if (grad_z == z || grad_z == grad_depth) return g_codec_err.fail(DD_ERR_INVALID_ARG, "the output may not alias an input");
  if (n < 1) return g_codec_err.fail(DD_ERR_INVALID_ARG, "n must be positive (got %lld)", (long long)n);
  if (n > (int64_t)1 << 38) return g_codec_err.fail(DD_ERR_INVALID_ARG, "n = %lld: at most 2^38 elements per call", (long long)n);
  DD_STATUS_HIP(g_codec_err, ddcodec::launch_tail_backward(z, grad_depth, grad_z, n, eps, (hipStream_t)stream));
  return DD_OK;
}

}  // extern "C"
