// dd_bn.h -- launchers of csrc/dd_bn.hip (batch-statistics BatchNorm, forward and backward) for the C ABI unit csrc/dd_api_bn.cpp.
// Everything is enqueued on `stream`; nothing here synchronises, allocates or reads device memory on the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ddbn {

constexpr int kThreads = 256;          // 4 waves of 64
constexpr int kMaxGroups = 128;        // workgroups per plane at most
constexpr int kGroupElems = kThreads * 4 * 4;      // values one workgroup is sized for: four 16-byte loads per thread
constexpr size_t kHeaderBytes = 256;   // reserved at the start of the workspace (zeroed by the caller, never written here)

// workgroups per plane of hw values
int groups_for(int64_t hw);
// bytes of workspace for a (B, C, hw) tensor: header + one fp64 pair per workgroup of a reduction
size_t workspace_bytes(int B, int C, int64_t hw);

hipError_t launch_stats(const float* x, double* sums, void* workspace, int B, int C, int hw, hipStream_t st);
hipError_t launch_finalize(const double* sums, float eps, float momentum, float* mean_invstd, float* running_mean, float* running_var, int C,
                           hipStream_t st);
hipError_t launch_apply(const float* x, const float* mean_invstd, const float* weight, const float* bias, float* y, int act, float slope,
                        int B, int C, int hw, hipStream_t st);
hipError_t launch_backward_reduce(const float* x, const float* grad_y, const float* mean_invstd, const float* weight, const float* bias,
                                  int act, float slope, double* sums2, void* workspace, int B, int C, int hw, hipStream_t st);
hipError_t launch_backward_apply(const float* x, const float* grad_y, const float* mean_invstd, const float* weight, const float* bias,
                                 const double* sums2, const double* sums, float* grad_x, int act, float slope, int B, int C, int hw,
                                 hipStream_t st);
// include/ddepth_bn_add.h: the apply with an addend (post != 0: behind the activation) and the PRE mode's one-pass backward reduction
hipError_t launch_apply_add(const float* x, const float* mean_invstd, const float* weight, const float* bias, const float* addend, float* y,
                            int act, float slope, int post, int B, int C, int hw, hipStream_t st);
hipError_t launch_backward_reduce_add(const float* x, const float* grad_y, const float* y, const float* mean_invstd, int act, float slope,
                                      float* g, double* sums2, void* workspace, int B, int C, int hw, hipStream_t st);

}  // namespace ddbn
