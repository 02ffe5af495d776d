// dd_swin.h -- the launcher of dd_swin.hip, called by dd_api_swin.cpp (which has checked every argument).
#pragma once
#include <hip/hip_runtime.h>

namespace ddswin {

constexpr int kWindow = 7;        // the one window size the kernel is written for
constexpr int kHeadDim = 32;      // ... and the one head dimension

// mode: 0 = fp32 operands (v_mfma_f32_32x32x2_f32), 1 = bf16, 2 = f16 (v_mfma_f32_32x32x16_*); accumulation and softmax are fp32 in all three
hipError_t launch_window_attention(const float* qkv, const float* qkv_pad, const float* rel_bias, float* out, int B, int H, int W, int heads,
                                   int shift, int mode, hipStream_t stream);

}  // namespace ddswin
