// dd_api_swin.cpp -- the C ABI of include/ddepth_swin.h: argument checks and the launch; the kernel is in dd_swin.hip.
#include "../../include/ddepth.h"
#include "../../include/ddepth_swin.h"
#include "dd_status.h"
#include "dd_swin.h"

#include <cstdint>

namespace ddswin {
__attribute__((visibility("hidden"))) thread_local ddstatus::LastError g_swin_err;      // shared with dd_api_swin_bwd.cpp: one dd_swin_last_error() for both headers
}

namespace {

using ddswin::g_swin_err;

int mode_of(int precision) { return precision == DD_PREC_FP32 ? 0 : precision == DD_PREC_BF16 ? 1 : precision == DD_PREC_F16 ? 2 : -1; }

}  // namespace

extern "C" {

const char* dd_swin_last_error(void) { return g_swin_err.text.c_str(); }

int dd_window_attention_supported(int C, int heads, int window, int precision) {
  return heads >= 1 && heads <= (1 << 16) && C == ddswin::kHeadDim * heads && window == ddswin::kWindow && mode_of(precision) >= 0;
}

int dd_window_attention_forward(const float* qkv, const float* qkv_pad, const float* rel_bias, float* out, int B, int H, int W, int C,
                                int heads, int window, int shift, int precision, void* stream) {
  if (!qkv || !rel_bias || !out) return g_swin_err.fail(DD_ERR_INVALID_ARG, "null pointer");
  if (out == qkv || out == rel_bias || (qkv_pad && out == qkv_pad)) return g_swin_err.fail(DD_ERR_INVALID_ARG, "out may not alias an input");
  if (B < 1 || H < 1 || W < 1 || C < 1 || heads < 1 || window < 1)
    return g_swin_err.fail(DD_ERR_INVALID_ARG, "B, H, W, C, heads, window must be positive (got %d, %d, %d, %d, %d, %d)", B, H, W, C, heads, window);
  if (shift < 0 || shift >= window) return g_swin_err.fail(DD_ERR_INVALID_ARG, "shift must be in 0 .. window - 1 (got %d, window %d)", shift, window);
  if (mode_of(precision) < 0)
    return g_swin_err.fail(DD_ERR_UNSUPPORTED, "precision %d: DD_PREC_FP32, DD_PREC_BF16 or DD_PREC_F16", precision);
  if (!dd_window_attention_supported(C, heads, window, precision))
    return g_swin_err.fail(DD_ERR_UNSUPPORTED, "C = %d, heads = %d, window = %d: only window 7 and C == 32 * heads", C, heads, window);
  if ((((uintptr_t)qkv | (uintptr_t)qkv_pad) & 15) != 0) return g_swin_err.fail(DD_ERR_INVALID_ARG, "qkv and qkv_pad must be 16-byte aligned");
  // token indices and the task count are 32-bit in the kernel
  const int64_t tokens = (int64_t)B * H * W;
  const int64_t tasks = (int64_t)B * ((H + 6) / 7) * ((W + 6) / 7) * heads;
  if (tokens > (int64_t)1 << 30 || tasks > (int64_t)1 << 30)
    return g_swin_err.fail(DD_ERR_INVALID_ARG, "B * H * W = %lld tokens, %lld tasks: at most 2^30 each per call", (long long)tokens, (long long)tasks);
  DD_STATUS_HIP(g_swin_err, ddswin::launch_window_attention(qkv, qkv_pad, rel_bias, out, B, H, W, heads, shift, mode_of(precision), (hipStream_t)stream));
  return DD_OK;
}

}  // extern "C"
