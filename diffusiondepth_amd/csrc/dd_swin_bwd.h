// dd_swin_bwd.h -- the launcher of dd_swin_bwd.hip, called by dd_api_swin_bwd.cpp (which has checked every argument).
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace ddswin {

// How the windows of one head are cut into slices, each reduced by one wave into one partial of grad_rel_bias and grad_qkv_pad: a function of
// the shape alone, never of the device.  nwin = B * ceil(H / 7) * ceil(W / 7).
inline int backward_windows_per_slice(int64_t nwin) { return nwin >= 1024 ? 16 : nwin >= 64 ? (int)(nwin / 64) : 1; }
inline int64_t backward_slices(int64_t nwin) { const int per = backward_windows_per_slice(nwin); return (nwin + per - 1) / per; }
// floats per (slice, head) in the workspace: the [key][query] partial of the bias gradient, then the q, k, v rows of the pad gradient
constexpr int kBwdBiasPartial = 49 * 49, kBwdPadPartial = 3 * 32;
inline int64_t backward_workspace_bytes(int64_t nwin, int heads) {
  return backward_slices(nwin) * heads * (int64_t)(kBwdBiasPartial + kBwdPadPartial) * (int64_t)sizeof(float);
}

// mode as in dd_swin.h; scale: NULL or the device pair {s, 1 / s} of dd_conv_grad_scale, read in mode 2 only
hipError_t launch_window_attention_backward(const float* qkv, const float* qkv_pad, const float* rel_bias, const float* grad_out, float* grad_qkv,
                                            float* grad_qkv_pad, float* grad_rel_bias, float* workspace, const float* scale, int B, int H, int W,
                                            int heads, int shift, int mode, hipStream_t stream);

}  // namespace ddswin
