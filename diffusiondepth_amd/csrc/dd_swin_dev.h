// dd_swin_dev.h -- what the forward (dd_swin.hip) and the backward (dd_swin_bwd.hip) kernels of the shifted-window attention share: the constants,
// the slot -> token map of the rolled padded frame, the live score registers and the 16-bit MFMA operand types.  Device code, internal linkage:
// every unit that includes it gets its own copy, and the kernels' mangled names stay those of a unit-local type.
#pragma once
#include "dd_swin.h"

#include <stdint.h>

#include <cmath>

namespace ddswin {
namespace {

constexpr int kTok = kWindow * kWindow;      // 49
constexpr int kSlots = 64;
constexpr int kVStride = 40;      // floats per key row of the V image: rows 4 apart (the two half-waves) are 32 banks apart
constexpr int kBStride = 52;      // floats per query row of the bias [query][key]: a lane reads 4 keys as 16 bytes, 16 lanes cover the 64 banks once
constexpr float kScale = 0.17677669529663687f;      // 32^-0.5

typedef __attribute__((ext_vector_type(8))) float f32x8_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

struct Frame { int H, W, Hp, Wp, nwx, nwy, shift; };

__device__ __forceinline__ int band(int r, int n, int shift) { return r < n - kWindow ? 0 : (r < n - shift ? 1 : 2); }

// slot s < 49 of window (wy, wx) of image b: its token index in the image or -1, and its mask label
__device__ __forceinline__ int slot_token(const Frame& f, int b, int wy, int wx, int s, int& label) {
  const int r = wy * kWindow + s / kWindow, c = wx * kWindow + s % kWindow;
  int y = r + f.shift, x = c + f.shift;
  if (y >= f.Hp) y -= f.Hp;
  if (x >= f.Wp) x -= f.Wp;
  label = f.shift > 0 ? 3 * band(r, f.Hp, f.shift) + band(c, f.Wp, f.shift) : 0;
  return (y < f.H && x < f.W) ? (b * f.H + y) * f.W + x : -1;
}

// registers of a score block that can hold a key < 49 in at least one half-wave: all of block 0, registers 0..8 of block 1
__device__ __forceinline__ constexpr bool live(int jb, int r) { return jb == 0 || r <= 8; }

// exp(x) as 2^(x log2 e) on the transcendental unit (v_exp_f32, 1 ulp): the rounding of the product costs |x| 2^-24 relative, on a value e^x
__device__ __forceinline__ float exp_fast(float x) {
#ifdef DD_HOST_EMULATION
  return exp2f(x * 1.4426950408889634f);
#else
  return __builtin_amdgcn_exp2f(x * 1.4426950408889634f);
#endif
}

__device__ __forceinline__ float4 load4(const float* p) { return *reinterpret_cast<const float4*>(p); }

template <int MODE> struct Operand;
template <> struct Operand<1> {
  typedef bf16x8_t T;
  static __device__ __forceinline__ T pack(const f32x8_t& x) { return __builtin_convertvector(x, bf16x8_t); }
  static __device__ __forceinline__ f32x16_t mma(T a, T b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};
template <> struct Operand<2> {
  typedef f16x8_t T;
  static __device__ __forceinline__ T pack(const f32x8_t& x) { return __builtin_convertvector(x, f16x8_t); }
  static __device__ __forceinline__ f32x16_t mma(T a, T b, f32x16_t c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};

}  // namespace
}  // namespace ddswin
