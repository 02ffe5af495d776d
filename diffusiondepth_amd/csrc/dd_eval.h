// dd_eval.h -- launchers of csrc/dd_eval.hip (depth metrics, supervised L1/L2 loss) for the C ABI unit csrc/dd_api_eval.cpp.
// Everything is enqueued on `stream`; nothing here synchronises, allocates or reads device memory on the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ddeval {

constexpr int kThreads = 256;         // 4 waves of 64
constexpr int kMaxGroups = 128;       // workgroups per image at most (the combine step reads one partial per thread: <= kThreads)
constexpr int kMetricSums = 9;        // [n_valid, S|d|, Sd^2, S|dinv|, Sdinv^2, S|d|/(gt+1e-8), #d1, #d2, #d3]
constexpr int kLossSums = 3;          // [S|p-g|m, S(p-g)^2 m, Sm]
constexpr int kMaxTicketImages = 1023; // batches beyond this combine by the second launch whatever was asked
constexpr size_t kTicketBytes = 4096;  // 32-bit arrival counters (one per image + one over the images) in a block of their own at the start of the workspace

// workgroups per image for an image of n pixels
int groups_for(int64_t n);
// bytes of workspace for B images of n pixels (ticket block + the partial slab of the wider of the two families)
size_t workspace_bytes(int B, int64_t n);

// reduce: 1 = partials combined by a second small launch, 2 = by the last workgroup to arrive (integer ticket in the workspace)
hipError_t launch_metric_sums(const float* pred, const float* gt, double* sums, void* workspace, int B, int n, float t_valid, int reduce,
                              hipStream_t st);
hipError_t launch_metric_finalize(const double* sums, float* batch_metrics, float* image_metrics, int B, hipStream_t st);
hipError_t launch_loss_forward(const float* pred, const float* gt, float* loss, double* sums, void* workspace, int B, int n, float max_depth,
                               float t_valid, int reduce, hipStream_t st);
hipError_t launch_loss_backward(const float* pred, const float* gt, const double* sums, const float* grad_l1, const float* grad_l2,
                                float* grad_pred, int B, int n, float max_depth, float t_valid, hipStream_t st);

}  // namespace ddeval
