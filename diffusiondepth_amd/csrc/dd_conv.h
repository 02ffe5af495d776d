// dd_conv.h -- launchers of csrc/dd_conv.hip (the condition FPN's and the HAHI neck's training convolutions, forward and backward) for the C ABI unit
// csrc/dd_api_conv.cpp.  Everything is enqueued on `stream`; nothing here synchronises, allocates or reads device memory on the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ddconv {

enum { kPrecBf16 = 0, kPrecF16 = 1, kPrecF16x3 = 2 };      // operand modes of the kernels (dd_api_conv.cpp maps dd_precision onto them)
enum { kOpConv3 = 0, kOpDeconv2 = 1, kOpConv1 = 2 };

constexpr int kThreads = 256;            // 4 waves of 64
constexpr int kTileH = 4, kTileW = 32;   // output pixels of one workgroup of the implicit GEMM: one 32-pixel row per wave
constexpr int kTileN = 64;               // output channels of one workgroup
constexpr int kPwTile = 128;             // 1x1: consecutive pixels of ONE plane a workgroup owns (32 per wave), forward, data and weight gradient alike
constexpr int kSplitTiles = 8;           // pixel tiles one workgroup of the weight gradient adds up, at least
constexpr int kMaxSplits = 64;           // pixel splits of the weight gradient at most (the tiles per split grow beyond)

// pixel tiles of the weight gradient (32 pixels wide, rows_per_tile high; 1x1: kPwTile consecutive pixels of a plane) and how they are split
// across workgroups
struct WgradSplit {
  int64_t tiles;
  int tiles_per_split, splits;
};
WgradSplit wgrad_split(int op, int B, int H, int W);

// bytes of workspace one shape needs: the packed 16-bit weights of forward / data gradient, or the weight gradient's partials
size_t workspace_bytes(int op, int B, int Cin, int Cout, int H, int W, int prec);

// dir: 0 forward, 1 data gradient.  `in` / `out` are x / y (forward) or grad_y / grad_x (data gradient); H, W = input size of the forward.
hipError_t launch_conv(int op, int dir, const float* in, const float* w, float* out, void* workspace, int B, int Cin, int Cout, int H,
                       int W, int prec, hipStream_t st);
hipError_t launch_wgrad(int op, const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H, int W,
                        int prec, hipStream_t st);

}  // namespace ddconv
