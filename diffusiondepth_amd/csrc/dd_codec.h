// dd_codec.h -- launchers of csrc/dd_codec.hip (the latent depth codec's four training convolutions, forward and backward, and the fused decoder
// tail) for the C ABI unit csrc/dd_api_codec.cpp.  Everything is enqueued on `stream`; nothing here synchronises, allocates or reads device memory
// on the host.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ddcodec {

enum { kOpEnc0 = 0, kOpEnc1 = 1, kOpDec0 = 2, kOpDec1 = 3 };      // dd_codec_op

constexpr int kC = 16;                   // the codec's hidden width: every op is 1 -> 16, 16 -> 16 or 16 -> 1
constexpr int kThreads = 256;            // 4 waves of 64
constexpr int kPackedFloats = 16 * kC * kC;   // forward / data gradient: the packed weights wp[tap][c][16] at the start of the workspace, at most (DEC0)
constexpr int kWgTileW = 64;             // weight gradient: a pixel tile is kWgTileW consecutive pixels of ONE row of the unshifted operand
constexpr int kSplitTiles = 8;           // pixel tiles one workgroup of the weight gradient adds up, at least
constexpr int kMaxSplits = 1024;         // pixel splits of the weight gradient at most (four workgroups per CU hide each other's tile fills; the tiles per split grow beyond)

// pixel tiles of the weight gradient and how they are split across workgroups
struct WgradSplit {
  int64_t tiles;
  int tiles_per_split, splits;
};
WgradSplit wgrad_split(int op, int B, int H, int W);      // H, W = the op's INPUT size

// output size of the forward
inline void out_size(int op, int H, int W, int* Ho, int* Wo) {
  if (op == kOpEnc0) { *Ho = (H - 1) / 2 + 1; *Wo = (W - 1) / 2 + 1; }
  else if (op == kOpDec0) { *Ho = 2 * H; *Wo = 2 * W; }
  else { *Ho = H; *Wo = W; }
}

// bytes of workspace one shape needs: the packed weights of forward / data gradient, or the weight (and bias) gradient's partials
size_t workspace_bytes(int op, int B, int H, int W);

// dir: 0 forward (in = x, out = y, bias may be null), 1 data gradient (in = grad_y, out = grad_x, bias ignored).  H, W = input size of the forward.
hipError_t launch_conv(int op, int dir, const float* in, const float* w, const float* bias, float* out, void* workspace, int B, int H, int W,
                       hipStream_t st);
hipError_t launch_wgrad(int op, const float* x, const float* grad_y, float* grad_w, float* grad_bias, void* workspace, int B, int H, int W,
                        hipStream_t st);
hipError_t launch_tail_forward(const float* z, float* depth, int64_t n, float eps, hipStream_t st);
hipError_t launch_tail_backward(const float* z, const float* grad_depth, float* grad_z, int64_t n, float eps, hipStream_t st);

}  // namespace ddcodec
