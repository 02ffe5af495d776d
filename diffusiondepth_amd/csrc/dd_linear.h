// dd_linear.h -- the launchers of dd_linear.hip, called by dd_api_linear.cpp (which has checked every argument).
#pragma once
#include <hip/hip_runtime.h>

namespace ddlinear {

constexpr int kTileN = 128;           // output columns of a workgroup tile
constexpr int kTileMBig = 128;        // output rows of a workgroup tile where those tiles fill the device ...
constexpr int kTileMSmall = 64;       // ... and where they do not
constexpr int kFillTiles = 256;       // "fill": at least this many big tiles (the MI355X has 256 CUs; a constant, so the choice needs no device)

// mode: 0 = fp32 operands (v_mfma_f32_32x32x2_f32), 1 = bf16, 2 = f16 (v_mfma_f32_32x32x16_*); accumulation and the epilogue are fp32 in all three
inline int operand_bytes(int mode) { return mode == 0 ? 4 : 2; }

// rows of the workgroup tile that launch_linear uses: a function of the shape and the mode alone.  The fp32 mode keeps a second set of
// accumulators (dd_linear.hip) and would run the big tile at one wave per SIMD: it always takes the small one.
inline int tile_rows(long long M, int N, int mode) {
  if (mode == 0) return kTileMSmall;
  const long long big = ((M + kTileMBig - 1) / kTileMBig) * ((N + kTileN - 1) / kTileN);
  return big >= kFillTiles ? kTileMBig : kTileMSmall;
}

hipError_t launch_linear_pack(const float* w, void* wp, int K, int N, int mode, hipStream_t stream);
hipError_t launch_linear(const float* x, const void* wp, const float* bias, const float* addend, float* y, long long M, int K, int N, int act,
                         int mode, hipStream_t stream);

}  // namespace ddlinear
