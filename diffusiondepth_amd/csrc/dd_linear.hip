// dd_linear.hip -- the token Linears of a Swin block (include/swin/ddepth_linear.h): y = act(x . w^T + bias) + addend, fp32 in and out.
//
// Both operands are contiguous along K, which is the A and B lane map of the 32x32 MFMAs as it stands (lane l: row l % 32, eight k at
// 8 (l / 32)): neither needs a transpose.  A = x (rows = tokens), B = the packed weight (rows = output columns), so D register r of a block is
// token 8 (r / 4) + 4 (l / 32) + r % 4, column l % 32, and a half-wave stores the 128 contiguous bytes of one row.
//
// A workgroup is four waves, 2 (M) x 2 (N), on a BM x 128 tile of y, BM = 128 (a wave owns 64 x 64: 2 x 2 MFMA blocks) or 64 (32 x 64);
// dd_linear.h: tile_rows chooses.
// K advances in stages of 64 operand BYTES per row -- 32 k in the 16-bit modes, 16 k in the fp32 mode -- so the LDS image has one geometry at
// every precision: [BM + 128 rows][64 bytes + 16 of padding].  Rows 80 bytes = 20 banks apart put the sixteen lanes that a ds_read_b128 serves
// together (rows 0-3, 12-15, 20-27 of one k half, ...) on sixteen different 4-bank groups.  A fragment is one 16-byte read: eight 16-bit
// operands for one 32x32x16 MFMA, or four floats for four 32x32x2 MFMAs, where k step e takes k = 4 half + e of the group of eight -- the
// contraction index may be permuted as long as A and B agree.
//   x is staged global fp32 -> registers -> (16-bit modes: rounded once) -> LDS; the packed weight is copied as it is.
//   Two LDS buffers, one barrier per stage: the global loads of stage t + 1 are issued before the MFMAs of stage t and written behind them.
// The sum over k runs stage by stage, k step by k step, in one accumulator per output (fp32 mode: one per 256 k, added to a total in
// order): its order depends on K and the precision alone.
// Rows >= M and columns >= N are staged as zeros (never read from memory) and never stored.
#include "dd_linear.h"

#include <stdint.h>

#include <cmath>

namespace ddlinear {
namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(8))) float f32x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;

constexpr int kThreads = 256;
constexpr int kRowVecs = 5;      // 16-byte pieces per LDS row: 4 of payload, 1 of padding
constexpr int kFlushStages = 16;      // fp32 mode: stages (of 16 k) whose sum is formed before it joins the total

template <int MODE> struct Operand;
template <> struct Operand<1> {
  typedef bf16x8_t T;
  static __device__ __forceinline__ u32x4_t pack(const f32x8_t& v) { return __builtin_bit_cast(u32x4_t, __builtin_convertvector(v, bf16x8_t)); }
  static __device__ __forceinline__ f32x16_t mma(u32x4_t a, u32x4_t b, f32x16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(T, a), __builtin_bit_cast(T, b), c, 0, 0, 0);
  }
};
template <> struct Operand<2> {
  typedef f16x8_t T;
  static __device__ __forceinline__ u32x4_t pack(const f32x8_t& v) { return __builtin_bit_cast(u32x4_t, __builtin_convertvector(v, f16x8_t)); }
  static __device__ __forceinline__ f32x16_t mma(u32x4_t a, u32x4_t b, f32x16_t c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(T, a), __builtin_bit_cast(T, b), c, 0, 0, 0);
  }
};

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

// w fp32 [N][K] -> the operand image [N][K]: thread i converts (fp32 mode: copies) elements 8 i ..+ 8
template <int MODE>
__global__ __launch_bounds__(kThreads) void linear_pack_kernel(const float* __restrict__ w, unsigned char* __restrict__ wp, long long pieces) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= pieces) return;
  const f32x4_t lo = *reinterpret_cast<const f32x4_t*>(w + 8 * i), hi = *reinterpret_cast<const f32x4_t*>(w + 8 * i + 4);
  if constexpr (MODE == 0) {
    *reinterpret_cast<f32x4_t*>(wp + 32 * i) = lo;
    *reinterpret_cast<f32x4_t*>(wp + 32 * i + 16) = hi;
  } else {
    const f32x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    *reinterpret_cast<u32x4_t*>(wp + 16 * i) = Operand<MODE>::pack(v);
  }
}

template <int MODE, int BM>
__global__ __launch_bounds__(kThreads) void linear_kernel(const float* __restrict__ x, const unsigned char* __restrict__ wp,
                                                          const float* __restrict__ bias, const float* __restrict__ addend,
                                                          float* __restrict__ y, long long M, int K, int N, int act, int ntn) {
  constexpr int TI = BM / 64;                        // 32-row MFMA blocks per wave
  constexpr int kEs = MODE == 0 ? 4 : 2;             // operand bytes
  constexpr int kStageK = 64 / kEs;                  // k per stage
  constexpr int kXVecs = MODE == 0 ? 1 : 2;          // 16-byte global loads of x per staged piece
  __shared__ u32x4_t lds[2][(BM + kTileN) * kRowVecs];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l32 = lane & 31, half = lane >> 5;
  const int wm = wave >> 1, wn = wave & 1;
  const long long tile = blockIdx.x;
  const long long m0 = (tile / ntn) * BM;
  const int n0 = (int)(tile % ntn) * kTileN;

  // staging: thread -> (row tid / 4 (+ 64 per item), 16-byte piece tid % 4 of the row's 64 bytes): four lanes cover a row's stage
  const int srow = tid >> 2, sc = tid & 3;
  const float* ap[TI];
  bool av[TI];
#pragma unroll
  for (int i = 0; i < TI; ++i) {
    const long long gm = m0 + srow + 64 * i;
    av[i] = gm < M;
    ap[i] = x + (size_t)(av[i] ? gm : 0) * K + 4 * kXVecs * sc;
  }
  const unsigned char* bp[2];
  bool bv[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int gn = n0 + srow + 64 * j;
    bv[j] = gn < N;
    bp[j] = wp + (size_t)(bv[j] ? gn : 0) * K * kEs + 16 * sc;
  }

  f32x4_t ra[TI][kXVecs];
  u32x4_t rb[2];
  const f32x4_t fzero = {0.f, 0.f, 0.f, 0.f};
  const u32x4_t uzero = {0u, 0u, 0u, 0u};

  auto load_stage = [&](int t) {
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int v = 0; v < kXVecs; ++v) ra[i][v] = av[i] ? *reinterpret_cast<const f32x4_t*>(ap[i] + (size_t)t * kStageK + 4 * v) : fzero;
#pragma unroll
    for (int j = 0; j < 2; ++j) rb[j] = bv[j] ? *reinterpret_cast<const u32x4_t*>(bp[j] + (size_t)t * 64) : uzero;
  };
  auto store_stage = [&](int buf) {
#pragma unroll
    for (int i = 0; i < TI; ++i) {
      u32x4_t piece;
      if constexpr (MODE == 0) {
        piece = __builtin_bit_cast(u32x4_t, ra[i][0]);
      } else {
        const f32x4_t lo = ra[i][0], hi = ra[i][kXVecs - 1];
        const f32x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        piece = Operand<MODE == 0 ? 1 : MODE>::pack(v);
      }
      lds[buf][(srow + 64 * i) * kRowVecs + sc] = piece;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) lds[buf][(BM + srow + 64 * j) * kRowVecs + sc] = rb[j];
  };

  f32x16_t acc[TI][2];
#pragma unroll
  for (int i = 0; i < TI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // fp32 mode: the sum of every 256 k is formed on its own and added to the total, so that a chain of fp32 additions is 128 + K / 256 long and
  // not K / 2: at K = 6144 a single chain's rounding errors would add up to several 1e-6 on outputs of size 1
  [[maybe_unused]] f32x16_t tot[MODE == 0 ? TI : 1][2];
  if constexpr (MODE == 0) {
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) tot[i][j][r] = 0.f;
  }

  const int stages = K / kStageK;
  load_stage(0);
  store_stage(0);
  __syncthreads();
  for (int t = 0; t < stages; ++t) {
    const int buf = t & 1;
    if (t + 1 < stages) load_stage(t + 1);      // in flight behind this stage's MFMAs
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      u32x4_t fa[TI], fb[2];
#pragma unroll
      for (int i = 0; i < TI; ++i) fa[i] = lds[buf][(wm * (BM / 2) + 32 * i + l32) * kRowVecs + 2 * kk + half];
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = lds[buf][(BM + wn * 64 + 32 * j + l32) * kRowVecs + 2 * kk + half];
      if constexpr (MODE == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int i = 0; i < TI; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(__builtin_bit_cast(f32x4_t, fa[i])[e], __builtin_bit_cast(f32x4_t, fb[j])[e],
                                                               acc[i][j], 0, 0, 0);
      } else {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = Operand<MODE == 0 ? 1 : MODE>::mma(fa[i], fb[j], acc[i][j]);
      }
    }
    if constexpr (MODE == 0) {
      if ((t & (kFlushStages - 1)) == kFlushStages - 1 || t + 1 == stages) {
#pragma unroll
        for (int i = 0; i < TI; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            tot[i][j] += acc[i][j];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
          }
      }
    }
    // the other buffer was last read in stage t - 1, which every wave left at the barrier that ended it
    if (t + 1 < stages) store_stage(buf ^ 1);
    __syncthreads();
  }
  if constexpr (MODE == 0) {
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = tot[i][j];
  }

  // ---- epilogue: + bias, GELU, + addend, all fp32; a half-wave writes 128 contiguous bytes of a row ---------------------------------------------
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn * 64 + 32 * j + l32;
    if (n >= N) continue;
    const float b = bias ? bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long long m = m0 + wm * (BM / 2) + 32 * i + 8 * (r / 4) + 4 * half + r % 4;
        if (m >= M) continue;
        const size_t at = (size_t)m * N + n;
        float v = acc[i][j][r] + b;
        if (act == 1) v = gelu_erf(v);
        if (addend) v += addend[at];
        y[at] = v;
      }
  }
}

template <int MODE>
hipError_t launch_mode(const float* x, const void* wp, const float* bias, const float* addend, float* y, long long M, int K, int N, int act,
                       hipStream_t stream) {
  const int ntn = (N + kTileN - 1) / kTileN;
  const int bm = tile_rows(M, N, MODE);
  const long long tiles = ((M + bm - 1) / bm) * ntn;
  const dim3 grid((unsigned)tiles), blk(kThreads);
  const unsigned char* w8 = static_cast<const unsigned char*>(wp);
  if constexpr (MODE != 0) {
    if (bm == kTileMBig) {
      hipLaunchKernelGGL((linear_kernel<MODE, kTileMBig>), grid, blk, 0, stream, x, w8, bias, addend, y, M, K, N, act, ntn);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL((linear_kernel<MODE, kTileMSmall>), grid, blk, 0, stream, x, w8, bias, addend, y, M, K, N, act, ntn);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_linear_pack(const float* w, void* wp, int K, int N, int mode, hipStream_t stream) {
  const long long pieces = (long long)N * K / 8;
  const dim3 grid((unsigned)((pieces + kThreads - 1) / kThreads)), blk(kThreads);
  unsigned char* p8 = static_cast<unsigned char*>(wp);
  if (mode == 0) hipLaunchKernelGGL(linear_pack_kernel<0>, grid, blk, 0, stream, w, p8, pieces);
  else if (mode == 1) hipLaunchKernelGGL(linear_pack_kernel<1>, grid, blk, 0, stream, w, p8, pieces);
  else hipLaunchKernelGGL(linear_pack_kernel<2>, grid, blk, 0, stream, w, p8, pieces);
  return hipGetLastError();
}

hipError_t launch_linear(const float* x, const void* wp, const float* bias, const float* addend, float* y, long long M, int K, int N, int act,
                         int mode, hipStream_t stream) {
  if (mode == 0) return launch_mode<0>(x, wp, bias, addend, y, M, K, N, act, stream);
  if (mode == 1) return launch_mode<1>(x, wp, bias, addend, y, M, K, N, act, stream);
  return launch_mode<2>(x, wp, bias, addend, y, M, K, N, act, stream);
}

}  // namespace ddlinear
