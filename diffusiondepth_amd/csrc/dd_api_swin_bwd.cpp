// dd_api_swin_bwd.cpp -- the C ABI of include/train/ddepth_swin_backward.h: argument checks and the launch; the kernels are in dd_swin_bwd.hip.
#include "../../include/ddepth.h"
#include "../../include/ddepth_swin.h"
#include "../../include/train/ddepth_swin_backward.h"
#include "dd_status.h"
#include "dd_swin.h"
#include "dd_swin_bwd.h"

#include <cstdint>

namespace ddswin {
extern __attribute__((visibility("hidden"))) thread_local ddstatus::LastError g_swin_err;      // dd_api_swin.cpp: behind dd_swin_last_error()
}

namespace {

using ddswin::g_swin_err;

int mode_of(int precision) { return precision == DD_PREC_FP32 ? 0 : precision == DD_PREC_BF16 ? 1 : precision == DD_PREC_F16 ? 2 : -1; }

// DD_OK, or the refusal of a shape: the checks of dd_window_attention_forward
int check_shape(int B, int H, int W, int C, int heads, int window, int precision) {
  if (B < 1 || H < 1 || W < 1 || C < 1 || heads < 1 || window < 1)
    return g_swin_err.fail(DD_ERR_INVALID_ARG, "B, H, W, C, heads, window must be positive (got %d, %d, %d, %d, %d, %d)", B, H, W, C, heads, window);
  if (mode_of(precision) < 0)
    return g_swin_err.fail(DD_ERR_UNSUPPORTED, "precision %d: DD_PREC_FP32, DD_PREC_BF16 or DD_PREC_F16", precision);
  if (!dd_window_attention_backward_supported(C, heads, window, precision))
    return g_swin_err.fail(DD_ERR_UNSUPPORTED, "C = %d, heads = %d, window = %d: only window 7 and C == 32 * heads", C, heads, window);
  // token indices and the task count are 32-bit in the kernel
  const int64_t tokens = (int64_t)B * H * W;
  const int64_t tasks = (int64_t)B * ((H + 6) / 7) * ((W + 6) / 7) * heads;
  if (tokens > (int64_t)1 << 30 || tasks > (int64_t)1 << 30)
    return g_swin_err.fail(DD_ERR_INVALID_ARG, "B * H * W = %lld tokens, %lld tasks: at most 2^30 each per call", (long long)tokens, (long long)tasks);
  return DD_OK;
}

int64_t windows(int B, int H, int W) { return (int64_t)B * ((H + 6) / 7) * ((W + 6) / 7); }

}  // namespace

extern "C" {

int dd_window_attention_backward_supported(int C, int heads, int window, int precision) {
  return dd_window_attention_supported(C, heads, window, precision);
}

int dd_window_attention_backward_workspace_bytes(int B, int H, int W, int C, int heads, int window, int precision, int64_t* bytes) {
  if (!bytes) return g_swin_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  const int rc = check_shape(B, H, W, C, heads, window, precision);
  if (rc != DD_OK) return rc;
  *bytes = ddswin::backward_workspace_bytes(windows(B, H, W), heads);
  return DD_OK;
}

int dd_window_attention_backward(const float* qkv, const float* qkv_pad, const float* rel_bias, const float* grad_out, float* grad_qkv,
                                 float* grad_qkv_pad, float* grad_rel_bias, void* workspace, const float* scale, int B, int H, int W, int C,
                                 int heads, int window, int shift, int precision, void* stream) {
  if (!qkv || !rel_bias || !grad_out || !grad_qkv || !workspace) return g_swin_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  const void* ins[] = {qkv, qkv_pad, rel_bias, grad_out, scale};
  const void* outs[] = {grad_qkv, grad_qkv_pad, grad_rel_bias, workspace};
  for (int o = 0; o < 4; ++o) {
    if (!outs[o]) continue;
    for (const void* in : ins)
      if (in == outs[o]) return g_swin_err.fail(DD_ERR_INVALID_ARG, "an output may not alias an input");
    for (int p = 0; p < o; ++p)
      if (outs[p] == outs[o]) return g_swin_err.fail(DD_ERR_INVALID_ARG, "an output may not alias another output");
  }
  const int rc = check_shape(B, H, W, C, heads, window, precision);
  if (rc != DD_OK) return rc;
  if (shift < 0 || shift >= window) return g_swin_err.fail(DD_ERR_INVALID_ARG, "shift must be in 0 .. window - 1 (got %d, window %d)", shift, window);
  if ((((uintptr_t)qkv | (uintptr_t)qkv_pad | (uintptr_t)grad_out | (uintptr_t)grad_qkv | (uintptr_t)workspace) & 15) != 0)
    return g_swin_err.fail(DD_ERR_INVALID_ARG, "qkv, qkv_pad, grad_out, grad_qkv and the workspace must be 16-byte aligned");
  DD_STATUS_HIP(g_swin_err, ddswin::launch_window_attention_backward(qkv, qkv_pad, rel_bias, grad_out, grad_qkv, grad_qkv_pad, grad_rel_bias,
                                                                     static_cast<float*>(workspace), scale, B, H, W, heads, shift,
                                                                     mode_of(precision), (hipStream_t)stream));
  return DD_OK;
}

}  // extern "C"
