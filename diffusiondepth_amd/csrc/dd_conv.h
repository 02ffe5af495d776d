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
constexpr int kPwKStep = 32;             // 1x1: channels per turn of the GEMM kernel's K loop (two MFMA steps), what its weight rows are padded to
constexpr int kSplitTiles = 8;           // pixel tiles one workgroup of the weight gradient adds up, at least
constexpr int kMaxSplits = 64;           // pixel splits of the weight gradient at most (the tiles per split grow beyond)

// pixel tiles of the weight gradient (32 pixels wide, rows_per_tile high; 1x1: kPwTile consecutive pixels of a plane) and how they are split
// across workgroups
struct WgradSplit {
  int64_t tiles;
  int tiles_per_split, splits;
};
WgradSplit wgrad_split(int op, int B, int H, int W);

// Channel counts: the two contracts of include/ddepth_conv.h, said here once for the argument checks of dd_api_conv.cpp and for the launchers.
// A pair inside the block-64 contract runs the unguarded instantiations; every other pair of the extended contract (dd_convx_*) runs the guarded
// ("ragged") ones, which fill channels beyond the count as zeros, store only real rows, and read a weight image padded to whole tiles.
// launch_conv / launch_wgrad choose by the shape alone.
enum ChannelContract { kChannelsBlock64, kChannelsExtended };
constexpr bool channels_block64(int c) { return c >= 64 && c <= 1536 && c % 64 == 0; }
constexpr bool channels_extended(int c) { return c >= 8 && c <= 2048 && c % 8 == 0; }
constexpr bool channels_ok(ChannelContract contract, int c) { return contract == kChannelsBlock64 ? channels_block64(c) : channels_extended(c); }
bool block64(int Cin, int Cout);      // both counts inside the block-64 contract

// halfs of the packed weight image of one direction (dir as in launch_conv): taps * (N rounded up to kTileN) * (K rounded up to the GEMM's K
// step); taps * Cin * Cout for block-64 counts
size_t packed_halfs(int op, int dir, int Cin, int Cout);

// bytes of workspace one shape needs: the larger packed 16-bit weight image of forward / data gradient (padded, see packed_halfs; twice in the
// split mode), or the weight gradient's partials [splits][taps * Cin * Cout] fp32.  The partials grow with the channel range: the 3x3 weight
// gradient of 2048 -> 1536 at the KITTI level-3 geometry (B = 4, 11 x 38) takes 6 splits of 113 MB, about 680 MB.
size_t workspace_bytes(int op, int B, int Cin, int Cout, int H, int W, int prec);

// dir: 0 forward, 1 data gradient.  `in` / `out` are x / y (forward) or grad_y / grad_x (data gradient); H, W = input size of the forward.
// scale (include/ddepth_conv_scaled.h; NULL: none): the device pair {s, 1 / s} of launch_grad_scale.  With it the two gradients of the f16 modes
// run the scaled twins of their kernels -- grad_y times s before it is rounded, the result times 1 / s; kBf16 and the forward ignore it.
hipError_t launch_conv(int op, int dir, const float* in, const float* w, float* out, void* workspace, int B, int Cin, int Cout, int H,
                       int W, int prec, hipStream_t st, const float* scale = nullptr);
hipError_t launch_wgrad(int op, const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H, int W,
                        int prec, hipStream_t st, const float* scale = nullptr);

// scale[0..3] = {s, 1 / s, bits of amax, 0} with amax the largest finite |grad_y[i]| and s = 2^(amax_exp - floor(log2 amax)) (shift within +-126;
// amax == 0: s = 1): a memset, one reduction pass (integer atomicMax: order-independent) and a single-thread kernel.  kPrecBf16: {1, 1}, no pass.
constexpr int kGradAmaxExp = 14;      // s * amax < 2^15 <= 65504, the largest f16: one GEMM accumulates in fp32, nothing behind it can overflow
hipError_t launch_grad_scale(const float* grad_y, int64_t n, int prec, int amax_exp, float* scale, hipStream_t st);

// ---- the 3x3 stride 2 pad 1 operator of include/ddepth_conv_strided.h ----------------------------------------------------------------------------------
// Not a dd_conv_op: the ABI of ddepth_conv.h keeps its three.  Inside this unit it is a fourth row of the one GEMM table.
enum { kOpConv3S2 = 3 };
// its channel contract: Cout extended; Cin extended or 3 (the guarded kernels check every channel, the weight image is padded to the K step)
constexpr bool channels_s2_in(int c) { return c == 3 || channels_extended(c); }
constexpr int strided_out(int n) { return (n - 1) / 2 + 1; }      // Ho of H: k3 s2 p1

// H, W = the INPUT size everywhere.  bias / grad_bias / scale may be NULL; scale as in launch_conv (the two gradients of the f16 modes).
size_t workspace_bytes_s2(int B, int Cin, int Cout, int H, int W, int prec);
hipError_t launch_conv_s2_forward(const float* x, const float* w, const float* bias, float* y, void* workspace, int B, int Cin, int Cout, int H, int W,
                                  int prec, hipStream_t st);
hipError_t launch_conv_s2_dgrad(const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int Cin, int Cout, int H, int W, int prec,
                                hipStream_t st, const float* scale);
hipError_t launch_conv_s2_wgrad(const float* x, const float* grad_y, float* grad_w, float* grad_bias, void* workspace, int B, int Cin, int Cout, int H,
                                int W, int prec, hipStream_t st, const float* scale);

// ---- the folded eval-mode forward of include/ddepth_conv_fused.h: 3x3 pad 1, stride 1 or 2, BatchNorm + residual + ReLU in the epilogue ------------------
// scale_shift [2][Cout] (launch_bn_fold writes it: fp64 per channel, rounded once; mean and var both NULL: no normalisation); addend NULL or y's
// layout; H, W = the INPUT size.  The workspace is the forward's packed weight image alone.  stride 1: the channel range of kChannelsExtended;
// stride 2: channels_s2_in / channels_extended.
size_t workspace_bytes_affine(int stride, int Cin, int Cout, int prec);
hipError_t launch_bn_fold(const float* weight, const float* bias, const float* mean, const float* var, double eps, const float* conv_bias,
                          float* scale_shift, int C, hipStream_t st);
hipError_t launch_conv_affine(int stride, const float* x, const float* w, const float* scale_shift, const float* addend, float* y, void* workspace,
                              int relu, int B, int Cin, int Cout, int H, int W, int prec, hipStream_t st);

// ---- the statistics-emitting forward of include/ddepth_conv_stats.h: 3x3 pad 1, stride 1 or 2, optional bias ---------------------------------------
// y as launch_conv(kOpConv3, 0) / launch_conv_s2_forward store it; sums[2 Cout + 1] = [sum | sum of squares | B Ho Wo] of y per channel in fp64, the
// layout of dd_bn_stats.  The workspace: the forward's packed weight image, then (256-byte aligned) the partials [Cout][B][tiles][2] fp64.
// H, W = the INPUT size.  Channel ranges as workspace_bytes_affine.
size_t workspace_bytes_stats(int stride, int B, int Cin, int Cout, int H, int W, int prec);
hipError_t launch_conv_stats(int stride, const float* x, const float* w, const float* bias, float* y, double* sums, void* workspace, int B, int Cin,
                             int Cout, int H, int W, int prec, hipStream_t st);

}  // namespace ddconv
