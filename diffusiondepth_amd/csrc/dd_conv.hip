// dd_conv.hip -- the training convolutions of the condition FPN and the HAHI neck as GEMM HIP kernels for gfx950 (include/ddepth_conv.h): Conv3x3 s1 p1,
// ConvTranspose2d k2 s2 and the pointwise Conv1x1, all without bias; forward, data gradient and weight gradient.  Tensors are contiguous fp32 NCHW as torch holds
// them; the operands are rounded to 16 bits on the way into LDS and contracted on v_mfma_f32_32x32x16_{bf16,f16} with fp32 accumulation.
//
// Structure:
//   dd_conv_pack_kernel     the raw fp32 weights -> wp[tap][n][k] in 16 bits (hi, and lo in the split-f16 mode) in the workspace, on EVERY call
//                           (the parameters change every optimiser step).  The data gradients are the same GEMM on the transposed (3x3: and
//                           flipped) weights, so this kernel is all that tells the directions apart.
//   dd_conv_igemm_kernel    D[n][pixel] += wp[tap][n][k] . patch[pixel + tap][k].  A workgroup owns a 4 x 32 pixel tile and 64 output channels,
//                           wave w the tile's row w: the weights are the MFMA's A operand (read from global / L2, 16 bytes per lane), 32
//                           consecutive pixels of a row its B operand, so lane l of the accumulator holds pixel l % 32 and every store
//                           instruction writes 32 consecutive floats of one output plane.  The input patch with its halo is converted into
//                           LDS KC channels at a time, consecutive lanes reading consecutive pixels of one NCHW plane; outside the image it is
//                           zero.  <KS, S, PAD>: 3x3 forward / data gradient <3, 1, 1>; transpose-convolution forward <1, 1, 0> with N = 4 Cout
//                           and an epilogue that writes pixel (2y + dy, 2x + dx); its data gradient <2, 2, 0>, which gathers those four.
//   dd_conv_wgrad_kernel    D[p][q][tap] += P[p][pixel] . Q[q][pixel * S + tap]: a GEMM over the pixel dimension (the MFMA's K = 16 consecutive
//                           pixels of a row).  A workgroup owns 64 x 64 channels and every tap, and a contiguous range of pixel tiles (a SPLIT);
//                           it stores its partial into the workspace, and dd_conv_wgrad_reduce_kernel adds the splits in a fixed order.  No
//                           floating-point atomics: two calls give the same bits.
//   dd_conv1x1_gemm_kernel  the 1x1 forward / data gradient: no halo, so a workgroup owns 128 consecutive pixels of a flat plane and the pixel-side MFMA
//   dd_conv1x1_wgrad_kernel operand comes straight from coalesced dword loads (no LDS); the 1x1 weight gradient contracts over the pixels, contiguous for
//                           both operands, through dword LDS stores and 16-byte reads (comments at the kernels).
//   the five kernels above  live in dd_conv_kernels.h, included twice: as they are, and as the twins *_scaled_kernel that multiply grad_y by the power of two
//                           scale[0] before it is rounded and the result by scale[1] = 1 / scale[0] (include/ddepth_conv_scaled.h; f16 modes, the two
//                           gradients).  dd_conv_grad_amax_kernel / dd_conv_grad_scale_pair_kernel make that pair on the device.
//   3x3 stride 2 pad 1      include/ddepth_conv_strided.h (the openings of a ResNet stage, bias allowed, Cin = 3 allowed): the forward is dd_conv_igemm <3, 2, 1>
//                           from a third inclusion of the header that adds the bias to the epilogue (dd_conv_igemm_bias_kernel), the weight gradient is
//                           dd_conv_wgrad <3, 2, 1>; the data gradient is dd_conv_s2_dgrad_kernel, which sorts the nine taps by the parity of the input pixel
//                           (1 + 2 + 2 + 4 tap GEMMs per 2 x 2 pixels); dd_conv_bias_grad_kernel / _reduce_kernel sum grad_y per channel in fp64 in a fixed order.
//   folded eval forward     include/ddepth_conv_fused.h (a BasicBlock in .eval()): dd_bn_fold_kernel turns a BatchNorm's running statistics and the conv's bias
//                           into scale_shift[2][N]; dd_conv_igemm_affine_kernel, a fourth inclusion of the header, is the implicit GEMM <3, 1, 1> or <3, 2, 1> whose
//                           epilogue stores relu(acc * scale + shift + addend).
//   statistics forward      include/ddepth_conv_stats.h (a training conv in front of a BatchNorm): dd_conv_igemm_stats_kernel, a fifth inclusion of the header, is the
//                           biased implicit GEMM <3, 1, 1> or <3, 2, 1> whose epilogue also sums the stored tile per channel in fp64 through the dead patch LDS;
//                           dd_conv_stats_combine_kernel adds the per-tile pairs in a fixed order into the sums vector of dd_bn_stats.
//   host side               gemm_kind(op, dir) is the one table of <KS, S, PAD, KC, SCATTER> and pack mode, gemm_shape adds N and K; the pack launch,
//                           the GEMM launch, packed_halfs and workspace_bytes read them, so the three that must agree on the padded weight image to
//                           the byte cannot drift apart.  dispatch() turns the runtime operand mode and channel contract into template arguments.
//
// Plain HIP C++ and compiler builtins; every write to memory is a plain C++ store.  Only constructs the host emulation of the tests provides.
#include "dd_conv.h"

#include <type_traits>

namespace ddconv {

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(8))) uint16_t u16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

__host__ __device__ constexpr int padded(int n, int step) { return (n + step - 1) / step * step; }

constexpr int kFillBatch = 8;      // global loads a thread has in flight while it fills LDS (one wave per SIMD cannot hide them otherwise)

__device__ __forceinline__ uint16_t f32_to_bf16(float f) {      // round to nearest even
  uint32_t u = __builtin_bit_cast(uint32_t, f);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// one fp32 value -> its 16-bit operand(s): the rounded value, or the f16 pair hi = f16(v), lo = f16(v - hi) of the split mode
template <int PREC>
__device__ __forceinline__ void to_operand(float v, uint16_t& hi, uint16_t& lo) {
  if constexpr (PREC == kPrecBf16) {
    hi = f32_to_bf16(v);
    lo = 0;
  } else {
    const _Float16 h = (_Float16)v;
    hi = __builtin_bit_cast(uint16_t, h);
    if constexpr (PREC == kPrecF16x3) lo = __builtin_bit_cast(uint16_t, (_Float16)(v - (float)h));
    else lo = 0;
  }
}

template <int PREC>
__device__ __forceinline__ f32x16_t mma(const uint4& a, const uint4& b, f32x16_t acc) {
  if constexpr (PREC == kPrecBf16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
}

// acc += a . b with a = ah + al, b = bh + bl: one MFMA, or hi.hi + hi.lo + lo.hi in the split mode
template <int PREC>
__device__ __forceinline__ f32x16_t mma_pair(const uint4& ah, const uint4& al, const uint4& bh, const uint4& bl, f32x16_t acc) {
  acc = mma<PREC>(ah, bh, acc);
  if constexpr (PREC == kPrecF16x3) {
    acc = mma<PREC>(ah, bl, acc);
    acc = mma<PREC>(al, bh, acc);
  }
  return acc;
}

// ---- weights -> wp[tap][n][k], 16 bits ----------------------------------------------------------------------------------------------------------
enum { kPackConvFwd = 0, kPackConvBwd = 1, kPackDeconvFwd = 2, kPackDeconvBwd = 3, kPackPwFwd = 4, kPackPwBwd = 5, kPackConvS2Bwd = 6 };

// RAGGED: the image is wp[tap][Np][Kp] with Np = N rounded up to kTileN and Kp = K rounded up to the GEMM's K step `kstep`; every element of it is
// written on every call, zero where n >= N or k >= K (the workspace arrives with arbitrary contents), so every 16-byte read of the GEMM kernels
// is aligned, inside the image, and meets zeros in the pad.  `wl` starts taps * Np * Kp halfs behind `wh`.
template <int PREC, bool RAGGED>
__global__ __launch_bounds__(kThreads) void dd_conv_pack_kernel(const float* __restrict__ w, uint16_t* __restrict__ wh, uint16_t* __restrict__ wl,
                                                                int mode, int N, int K, int taps, int kstep) {
  const int Kp = RAGGED ? padded(K, kstep) : K, Np = RAGGED ? padded(N, kTileN) : N;
  const size_t total = (size_t)taps * Np * Kp;
  const size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int k = (int)(idx % Kp), n = (int)((idx / Kp) % Np), t = (int)(idx / ((size_t)Kp * Np));
  if constexpr (RAGGED) {
    if (n >= N || k >= K) {
      wh[idx] = 0;
      if constexpr (PREC == kPrecF16x3) wl[idx] = 0;
      return;
    }
  }
  size_t src;
  if (mode == kPackConvFwd) {             // w[co = n][ci = k][tap]
    src = ((size_t)n * K + k) * 9 + t;
  } else if (mode == kPackConvBwd) {      // w'[ci = n][co = k][ky][kx] = w[co][ci][2 - ky][2 - kx]
    src = ((size_t)k * N + n) * 9 + (8 - t);
  } else if (mode == kPackDeconvFwd) {    // n = (dy * 2 + dx) * Cout + co;  w[ci = k][co][dy][dx]
    const int cout = N / 4, t4 = n / cout, co = n - t4 * cout;
    src = ((size_t)k * cout + co) * 4 + t4;
  } else if (mode == kPackDeconvBwd) {    // w[ci = n][co = k][tap]
    src = ((size_t)n * K + k) * 4 + t;
  } else if (mode == kPackPwFwd) {        // 1x1: w[co = n][ci = k]
    src = (size_t)n * K + k;
  } else if (mode == kPackPwBwd) {        // 1x1 data gradient: w'[ci = n][co = k] = w[co][ci]
    src = (size_t)k * N + n;
  } else {                                // 3x3 stride 2 data gradient: w'[ci = n][co = k][ky][kx] = w[co][ci][ky][kx], the taps by parity class in the kernel
    src = ((size_t)k * N + n) * 9 + t;
  }
  uint16_t hi, lo;
  to_operand<PREC>(w[src], hi, lo);
  wh[idx] = hi;
  if constexpr (PREC == kPrecF16x3) wl[idx] = lo;
}

// ---- the GEMM kernels, and their twins on a rescaled grad_y (dd_conv_kernels.h) ---------------------------------------------------------------------
constexpr int wgrad_channel_stride(int halfs) {      // halfs between two channels of the shifted operand in LDS: an ODD number of dwords
  const int even = (halfs + 1) / 2 * 2;
  return (even / 2) % 2 == 0 ? even + 2 : even;
}

#define DD_CONV_SCALED 0
#define DD_CONV_BIAS 0
#define DD_CONV_AFFINE 0
#define DD_CONV_STATS 0
#include "dd_conv_kernels.h"
#undef DD_CONV_SCALED
#define DD_CONV_SCALED 1
#include "dd_conv_kernels.h"
#undef DD_CONV_SCALED
#undef DD_CONV_BIAS
#define DD_CONV_SCALED 0
#define DD_CONV_BIAS 1      // dd_conv_igemm_bias_kernel: the forward of include/ddepth_conv_strided.h
#include "dd_conv_kernels.h"
#undef DD_CONV_SCALED
#undef DD_CONV_BIAS

// the tail of dd_conv_igemm_affine_kernel's epilogue (include/ddepth_conv_fused.h): the residual, then a ReLU that keeps a NaN
__device__ __forceinline__ float affine_tail(float v, const float* __restrict__ addend, size_t o, int relu) {
  if (addend) v += addend[o];
  if (relu) v = v < 0.0f ? 0.0f : v;      // (NaN < 0 is false)
  return v;
}

#undef DD_CONV_AFFINE
#define DD_CONV_SCALED 0
#define DD_CONV_BIAS 0
#define DD_CONV_AFFINE 1      // dd_conv_igemm_affine_kernel: the folded forward of include/ddepth_conv_fused.h
#include "dd_conv_kernels.h"
#undef DD_CONV_SCALED
#undef DD_CONV_BIAS
#undef DD_CONV_AFFINE
#undef DD_CONV_STATS
#define DD_CONV_SCALED 0
#define DD_CONV_BIAS 0
#define DD_CONV_AFFINE 0
#define DD_CONV_STATS 1      // dd_conv_igemm_stats_kernel: the statistics-emitting forward of include/ddepth_conv_stats.h
#include "dd_conv_kernels.h"
#undef DD_CONV_SCALED
#undef DD_CONV_BIAS
#undef DD_CONV_AFFINE
#undef DD_CONV_STATS

// sums[2 C + 1] = [sum | sum of squares | count] of a BatchNorm (the layout of dd_bn_stats) from the slab part[C][rows][2] that
// dd_conv_igemm_stats_kernel wrote, rows = B * tiles: one workgroup per channel, thread t adds the rows t, t + 256, ... in that order, then a tree
// over the 256 pairs in LDS.  The order depends on the shape alone: no atomics, the same bits on every run.
__global__ __launch_bounds__(kThreads) void dd_conv_stats_combine_kernel(const double* __restrict__ part, double* __restrict__ sums, int rows, int C,
                                                                         double count) {
  __shared__ double lds[2][kThreads];
  const int c = blockIdx.x, tid = threadIdx.x;
  const double* row = part + (size_t)c * rows * 2;
  double sa = 0.0, sb = 0.0;
  for (int r = tid; r < rows; r += kThreads) {
    sa += row[2 * r];
    sb += row[2 * r + 1];
  }
  lds[0][tid] = sa;
  lds[1][tid] = sb;
  __syncthreads();
  for (int d = kThreads / 2; d >= 1; d >>= 1) {
    if (tid < d) {
      lds[0][tid] += lds[0][tid + d];
      lds[1][tid] += lds[1][tid + d];
    }
    __syncthreads();
  }
  if (tid < 2) sums[tid * C + c] = lds[tid][0];
  if (c == 0 && tid == 0) sums[2 * C] = count;
}

// scale_shift[2][C] of an eval-mode BatchNorm behind a convolution with the bias conv_bias: one thread per channel, fp64, each result rounded once.
//   scale = weight / sqrt(var + eps),  shift = bias + (conv_bias - mean) * scale;  weight, bias, conv_bias NULL: 1, 0, 0.
// mean and var both NULL: no normalisation (scale = weight, shift = bias + conv_bias * weight) -- a bare biased convolution.
__global__ __launch_bounds__(kThreads) void dd_bn_fold_kernel(const float* __restrict__ weight, const float* __restrict__ bias,
                                                              const float* __restrict__ mean, const float* __restrict__ var, double eps,
                                                              const float* __restrict__ conv_bias, float* __restrict__ scale_shift, int C) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= C) return;
  double s = weight ? (double)weight[c] : 1.0;
  if (var) s /= sqrt((double)var[c] + eps);
  const double m = mean ? (double)mean[c] : 0.0;
  scale_shift[c] = (float)s;
  scale_shift[C + c] = (float)((bias ? (double)bias[c] : 0.0) + ((conv_bias ? (double)conv_bias[c] : 0.0) - m) * s);
}

// ---- the scale of a gradient (include/ddepth_conv_scaled.h) -------------------------------------------------------------------------------------------
// scale[2] = the bits of the largest FINITE |g[i]|, as an integer maximum of the bits of the non-negative floats (their order is that of the
// values): whatever order the atomics land in, the result is the same.  NaN and Inf (exponent field all ones) take no part.  The buffer arrives
// zeroed.  A thread walks the tensor with the grid's stride, four dword loads in flight; a wave combines its 64 maxima before lane 0 adds the one atomic.
constexpr int kAmaxBlocks = 1024;      // workgroups of the reduction at most (4 per CU; the stride loop takes the rest)

__global__ __launch_bounds__(kThreads) void dd_conv_grad_amax_kernel(const float* __restrict__ g, long long n, unsigned* __restrict__ amax_bits) {
  const long long stride = (long long)gridDim.x * kThreads;
  unsigned m = 0;
  for (long long i0 = (long long)blockIdx.x * kThreads + threadIdx.x; i0 < n; i0 += 4 * stride) {
    unsigned u[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long i = i0 + j * stride;
      u[j] = i < n ? __builtin_bit_cast(unsigned, g[i]) & 0x7FFFFFFFu : 0u;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (u[j] < 0x7F800000u && u[j] > m) m = u[j];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned o = (unsigned)__shfl_xor((int)m, d);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0 && m != 0) atomicMax(amax_bits, m);
}

// one thread: s = 2^(amax_exp - floor(log2 amax)) and 1 / s from amax's exponent field, the shift held to +-126 so that both are normal fp32;
// amax == 0 (an all-zero tensor, or no reduction at all: bf16) gives s = 1.  A subnormal amax has floor(log2) < -126: the shift is at its limit.
__global__ void dd_conv_grad_scale_pair_kernel(float* __restrict__ scale, int amax_exp) {
  const unsigned bits = __builtin_bit_cast(unsigned, scale[2]);
  int shift = 0;
  if (bits != 0) {
    shift = amax_exp - ((int)(bits >> 23) - 127);
    shift = shift > 126 ? 126 : shift < -126 ? -126 : shift;
  }
  scale[0] = __builtin_bit_cast(float, (unsigned)(127 + shift) << 23);
  scale[1] = __builtin_bit_cast(float, (unsigned)(127 - shift) << 23);
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// ---- one description of each GEMM ---------------------------------------------------------------------------------------------------------------------
// The forward (dir 0) / data gradient (dir 1) of an operator as the GEMM D[n][pixel] += wp[tap][n][k] . patch[pixel + tap][k]: the arguments its kernel
// template is instantiated with, the K step its weight image is padded to, and the pack mode.  The ONLY place that says them: gemm_shape adds the
// channel counts, and the pack launch, the GEMM launch, packed_halfs and workspace_bytes read these two.
struct GemmKind {
  int ks, stride, pad, kstep, pack_mode;
  bool scatter;
};
constexpr GemmKind gemm_kind(int op, int dir) {
  if (op == kOpConv3) return {3, 1, 1, 32, dir == 0 ? kPackConvFwd : kPackConvBwd, false};
  if (op == kOpConv1) return {1, 1, 0, kPwKStep, dir == 0 ? kPackPwFwd : kPackPwBwd, false};
  // 3x3 s2 p1.  Forward: the 9 x 65 pixel patch at KC = 16 is 28 KB of LDS (56 KB split-f16), so two workgroups still share a CU in the split mode;
  // KC = 32 (46.8 / 93.6 KB) would leave one.  Data gradient: dd_conv_s2_dgrad_kernel, a 5 x 33 patch, KC = 32 (13.2 / 26.4 KB).
  if (op == kOpConv3S2) return {3, 2, 1, dir == 0 ? 16 : 32, dir == 0 ? kPackConvFwd : kPackConvS2Bwd, false};
  if (dir == 0) return {1, 1, 0, 32, kPackDeconvFwd, true};      // N = 4 Cout: GEMM column (dy * 2 + dx) * Cout + co, scattered by the epilogue
  return {2, 2, 0, 16, kPackDeconvBwd, false};                   // ... and gathered again: four taps of stride 2
}

struct GemmShape {
  int taps, N, K, kstep, pack_mode;
};
GemmShape gemm_shape(int op, int dir, int Cin, int Cout) {
  const GemmKind k = gemm_kind(op, dir);
  const int n = dir == 0 ? Cout : Cin;
  return {k.ks * k.ks, k.scatter ? 4 * n : n, dir == 0 ? Cin : Cout, k.kstep, k.pack_mode};
}

// halfs of the image wp[tap][Np][Kp] the pack kernel writes and the GEMM kernel reads ALL of, 16 bytes at a time: Np = N rounded up to kTileN, Kp = K
// rounded up to the K step.  For block-64 channel counts it is taps * Cin * Cout.
size_t packed_halfs(const GemmShape& g) { return (size_t)g.taps * (size_t)padded(g.N, kTileN) * (size_t)padded(g.K, g.kstep); }

// the weight gradient: taps of the filter itself (those of the data gradient's GEMM; the transpose forward folds its four into N), and the rows RH of
// a pixel tile of its instantiation (LDS: 58.5 KB / 43.5 KB split-f16; the 1x1 has flat tiles)
constexpr int taps_of(int op) { return gemm_kind(op, 1).ks * gemm_kind(op, 1).ks; }
constexpr int wgrad_rows(int op) { return op == kOpConv3 || op == kOpConv3S2 ? 2 : 1; }

// the implicit GEMM of (OP, DIR), instantiated from its gemm_kind.  H, W = the tile grid (the forward's input size); the input is `stride` times that.
// SCALED: the twin that rescales `in` (grad_y) by `scale`; data gradients only.
template <int PREC, bool RAGGED, int OP, int DIR, bool SCALED = false>
void launch_igemm(const GemmShape& g, const float* in, const uint16_t* wh, const uint16_t* wl, float* out, const float* scale, int B, int H, int W,
                  hipStream_t st) {
  constexpr GemmKind k = gemm_kind(OP, DIR);
  const int tiles_x = (W + kTileW - 1) / kTileW, tiles_y = (H + kTileH - 1) / kTileH;
  const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)((g.N + kTileN - 1) / kTileN), (unsigned)B);
  if constexpr (SCALED) {
    static_assert(DIR == 1 && !k.scatter, "only the data gradients have a scaled twin");
    hipLaunchKernelGGL((dd_conv_igemm_scaled_kernel<PREC, k.ks, k.stride, k.pad, k.kstep, k.scatter, RAGGED>), grid, dim3(kThreads), 0, st, in, wh, wl, out,
                       g.K, g.N, k.stride * H, k.stride * W, H, W, tiles_x, scale);
  } else {
    hipLaunchKernelGGL((dd_conv_igemm_kernel<PREC, k.ks, k.stride, k.pad, k.kstep, k.scatter, RAGGED>), grid, dim3(kThreads), 0, st, in, wh, wl, out,
                       g.K, g.N, k.stride * H, k.stride * W, H, W, tiles_x);
  }
}

// the 1x1 forward / data gradient: four 32-channel blocks per wave where the channels allow (half the re-reads of the input), else two
template <int PREC, bool RAGGED, bool SCALED>
void launch_gemm1x1(const GemmShape& g, const float* in, const uint16_t* wh, const uint16_t* wl, float* out, const float* scale, int B, int P,
                    hipStream_t st) {
  const unsigned ptiles = (unsigned)((P + kPwTile - 1) / kPwTile);
  const bool four = g.N % 128 == 0;
  const dim3 grid(ptiles * (unsigned)(four ? g.N / 128 : (g.N + 63) / 64), (unsigned)B);
  if constexpr (SCALED) {
    if (four) hipLaunchKernelGGL((dd_conv1x1_gemm_scaled_kernel<PREC, 4, RAGGED>), grid, dim3(kThreads), 0, st, in, wh, wl, out, g.K, g.N, P, scale);
    else hipLaunchKernelGGL((dd_conv1x1_gemm_scaled_kernel<PREC, 2, RAGGED>), grid, dim3(kThreads), 0, st, in, wh, wl, out, g.K, g.N, P, scale);
  } else {
    if (four) hipLaunchKernelGGL((dd_conv1x1_gemm_kernel<PREC, 4, RAGGED>), grid, dim3(kThreads), 0, st, in, wh, wl, out, g.K, g.N, P);
    else hipLaunchKernelGGL((dd_conv1x1_gemm_kernel<PREC, 2, RAGGED>), grid, dim3(kThreads), 0, st, in, wh, wl, out, g.K, g.N, P);
  }
}

// RAGGED launches the guarded instantiations: grids round the channel blocks up, the packed image is the padded one (!RAGGED: no pad to add).
// SCALED (dir == 1, an f16 mode): the same pack launch, then the GEMM's scaled twin.
template <int PREC, bool RAGGED, bool SCALED>
hipError_t launch_conv_prec(int op, int dir, const float* in, const float* w, float* out, void* workspace, const float* scale, int B, int Cin,
                            int Cout, int H, int W, hipStream_t st) {
  const GemmShape g = gemm_shape(op, dir, Cin, Cout);
  uint16_t* wh = reinterpret_cast<uint16_t*>(workspace);
  uint16_t* wl = wh + packed_halfs(g);      // (only the split mode reads or writes it)
  hipLaunchKernelGGL((dd_conv_pack_kernel<PREC, RAGGED>), dim3(blocks_for(packed_halfs(g))), dim3(kThreads), 0, st, w, wh, wl, g.pack_mode, g.N, g.K,
                     g.taps, g.kstep);
  if constexpr (SCALED) {
    if (op == kOpConv1) launch_gemm1x1<PREC, RAGGED, true>(g, in, wh, wl, out, scale, B, H * W, st);
    else if (op == kOpConv3) launch_igemm<PREC, RAGGED, kOpConv3, 1, true>(g, in, wh, wl, out, scale, B, H, W, st);
    else launch_igemm<PREC, RAGGED, kOpDeconv2, 1, true>(g, in, wh, wl, out, scale, B, H, W, st);
  } else if (op == kOpConv1) {
    launch_gemm1x1<PREC, RAGGED, false>(g, in, wh, wl, out, nullptr, B, H * W, st);
  } else if (op == kOpConv3 && dir == 0) {      // (the 3x3's two directions are one instantiation: the pack mode alone tells them apart)
    launch_igemm<PREC, RAGGED, kOpConv3, 0>(g, in, wh, wl, out, nullptr, B, H, W, st);
  } else if (op == kOpConv3) {
    launch_igemm<PREC, RAGGED, kOpConv3, 1>(g, in, wh, wl, out, nullptr, B, H, W, st);
  } else if (dir == 0) {
    launch_igemm<PREC, RAGGED, kOpDeconv2, 0>(g, in, wh, wl, out, nullptr, B, H, W, st);
  } else {
    launch_igemm<PREC, RAGGED, kOpDeconv2, 1>(g, in, wh, wl, out, nullptr, B, H, W, st);
  }
  return hipGetLastError();
}

template <int PREC, bool RAGGED, bool SCALED>
hipError_t launch_wgrad_prec(int op, const float* x, const float* grad_y, float* grad_w, void* workspace, const float* scale, int B, int Cin, int Cout,
                             int H, int W, hipStream_t st) {
  const WgradSplit sp = wgrad_split(op, B, H, W);
  const int tiles_x = (W + 31) / 32, tiles_y = (H + wgrad_rows(op) - 1) / wgrad_rows(op);      // (the 1x1 has flat tiles: sp.tiles)
  float* part = reinterpret_cast<float*>(workspace);
  const dim3 grid((unsigned)(((Cin + 63) / 64) * ((Cout + 63) / 64)), (unsigned)sp.splits);
  const size_t total = (size_t)Cin * Cout * taps_of(op);
  if constexpr (SCALED) {      // grad_y is P of the 3x3 and the 1x1, Q of the transpose
    if (op == kOpConv1) {
      hipLaunchKernelGGL((dd_conv1x1_wgrad_scaled_kernel<PREC, RAGGED>), grid, dim3(kThreads), 0, st, grad_y, x, part, Cout, Cin, H * W,
                         (H * W + kPwTile - 1) / kPwTile, (long long)sp.tiles, sp.tiles_per_split, scale);
    } else if (op == kOpConv3) {
      hipLaunchKernelGGL((dd_conv_wgrad_scaled_kernel<PREC, 3, 1, 1, wgrad_rows(kOpConv3), RAGGED>), grid, dim3(kThreads), 0, st, grad_y, x, part, Cout,
                         Cin, H, W, H, W, tiles_x, tiles_y, (long long)sp.tiles, sp.tiles_per_split, scale);
    } else {
      hipLaunchKernelGGL((dd_conv_wgrad_scaled_kernel<PREC, 2, 2, 0, wgrad_rows(kOpDeconv2), RAGGED>), grid, dim3(kThreads), 0, st, x, grad_y, part,
                         Cin, Cout, H, W, 2 * H, 2 * W, tiles_x, tiles_y, (long long)sp.tiles, sp.tiles_per_split, scale);
    }
    hipLaunchKernelGGL(dd_conv_wgrad_reduce_scaled_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, st, (const float*)part, grad_w, total, sp.splits,
                       scale);
    return hipGetLastError();
  }
  if (op == kOpConv1) {
    hipLaunchKernelGGL((dd_conv1x1_wgrad_kernel<PREC, RAGGED>), grid, dim3(kThreads), 0, st, grad_y, x, part, Cout, Cin, H * W,
                       (H * W + kPwTile - 1) / kPwTile, (long long)sp.tiles, sp.tiles_per_split);
  } else if (op == kOpConv3) {
    hipLaunchKernelGGL((dd_conv_wgrad_kernel<PREC, 3, 1, 1, wgrad_rows(kOpConv3), RAGGED>), grid, dim3(kThreads), 0, st, grad_y, x, part, Cout, Cin,
                       H, W, H, W, tiles_x, tiles_y, (long long)sp.tiles, sp.tiles_per_split);
  } else {
    hipLaunchKernelGGL((dd_conv_wgrad_kernel<PREC, 2, 2, 0, wgrad_rows(kOpDeconv2), RAGGED>), grid, dim3(kThreads), 0, st, x, grad_y, part, Cin, Cout,
                       H, W, 2 * H, 2 * W, tiles_x, tiles_y, (long long)sp.tiles, sp.tiles_per_split);
  }
  hipLaunchKernelGGL(dd_conv_wgrad_reduce_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, st, (const float*)part, grad_w, total, sp.splits);
  return hipGetLastError();
}

// f(precision, ragged, scaled) with the runtime operand mode, contract and rescale as the compile-time constants the kernels are instantiated with.
// A shape of the block-64 contract runs the block-64 instantiations, whichever entry point it came through; only the others run the guarded ones.
// The scaled twins exist for the f16 modes alone: bf16 has fp32's exponent range and runs the unscaled kernels whatever `scaled` says.
template <class F>
hipError_t dispatch(int prec, int Cin, int Cout, bool scaled, F f) {
  const auto by_channels = [&](auto p, auto sc) { return block64(Cin, Cout) ? f(p, std::false_type{}, sc) : f(p, std::true_type{}, sc); };
  const auto by_scale = [&](auto p) { return scaled ? by_channels(p, std::true_type{}) : by_channels(p, std::false_type{}); };
  if (prec == kPrecBf16) return by_channels(std::integral_constant<int, kPrecBf16>{}, std::false_type{});
  if (prec == kPrecF16) return by_scale(std::integral_constant<int, kPrecF16>{});
  return by_scale(std::integral_constant<int, kPrecF16x3>{});
}

// ---- 3x3 stride 2 (include/ddepth_conv_strided.h) ----------------------------------------------------------------------------------------------------
// dir 0: pack, then the implicit GEMM <3, 2, 1> with the bias in its epilogue; dir 1: pack by tap, then the parity-class kernel (SCALED: its twin)
template <int PREC, bool RAGGED, bool SCALED>
hipError_t launch_s2_prec(int dir, const float* in, const float* w, const float* bias, float* out, void* workspace, const float* scale, int B,
                          int Cin, int Cout, int H, int W, hipStream_t st) {
  const GemmShape g = gemm_shape(kOpConv3S2, dir, Cin, Cout);
  const int Ho = strided_out(H), Wo = strided_out(W);      // also the half-resolution grid of the data gradient: ceil(H / 2) x ceil(W / 2)
  uint16_t* wh = reinterpret_cast<uint16_t*>(workspace);
  uint16_t* wl = wh + packed_halfs(g);
  hipLaunchKernelGGL((dd_conv_pack_kernel<PREC, RAGGED>), dim3(blocks_for(packed_halfs(g))), dim3(kThreads), 0, st, w, wh, wl, g.pack_mode, g.N, g.K,
                     g.taps, g.kstep);
  const int tiles_x = (Wo + kTileW - 1) / kTileW, tiles_y = (Ho + kTileH - 1) / kTileH;
  const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)((g.N + kTileN - 1) / kTileN), (unsigned)B);
  if (dir == 0) {
    constexpr GemmKind k = gemm_kind(kOpConv3S2, 0);
    hipLaunchKernelGGL((dd_conv_igemm_bias_kernel<PREC, k.ks, k.stride, k.pad, k.kstep, k.scatter, RAGGED>), grid, dim3(kThreads), 0, st, in,
                       (const uint16_t*)wh, (const uint16_t*)wl, out, g.K, g.N, H, W, Ho, Wo, tiles_x, bias);
  } else {
    constexpr GemmKind k = gemm_kind(kOpConv3S2, 1);
    if constexpr (SCALED) {
      hipLaunchKernelGGL((dd_conv_s2_dgrad_scaled_kernel<PREC, k.kstep, RAGGED>), grid, dim3(kThreads), 0, st, in, (const uint16_t*)wh,
                         (const uint16_t*)wl, out, g.K, g.N, H, W, Ho, Wo, tiles_x, scale);
    } else {
      hipLaunchKernelGGL((dd_conv_s2_dgrad_kernel<PREC, k.kstep, RAGGED>), grid, dim3(kThreads), 0, st, in, (const uint16_t*)wh, (const uint16_t*)wl,
                         out, g.K, g.N, H, W, Ho, Wo, tiles_x);
    }
  }
  return hipGetLastError();
}

// the bias gradient's chunks per plane: one per kBiasChunkPixels pixels, at most kBiasMaxChunks (Cout * chunks workgroups fill the device from 64
// channels on); the partials are Cout * chunks doubles of the workspace
constexpr int kBiasChunkPixels = 4096, kBiasMaxChunks = 64;
inline int bias_grad_chunks(long long plane) {
  const long long c = (plane + kBiasChunkPixels - 1) / kBiasChunkPixels;
  return (int)(c < 1 ? 1 : c > kBiasMaxChunks ? kBiasMaxChunks : c);
}

// P = grad_y on the Ho x Wo grid, Q = x read at (2y - 1 + ky, 2x - 1 + kx); the split rule and the ordered reduce of every weight gradient here
template <int PREC, bool RAGGED, bool SCALED>
hipError_t launch_s2_wgrad_prec(const float* x, const float* grad_y, float* grad_w, float* grad_bias, void* workspace, const float* scale, int B,
                                int Cin, int Cout, int H, int W, hipStream_t st) {
  constexpr int RH = wgrad_rows(kOpConv3S2);
  const int Ho = strided_out(H), Wo = strided_out(W);
  const WgradSplit sp = wgrad_split(kOpConv3S2, B, Ho, Wo);
  const int tiles_x = (Wo + 31) / 32, tiles_y = (Ho + RH - 1) / RH;
  float* part = reinterpret_cast<float*>(workspace);
  const dim3 grid((unsigned)(((Cin + 63) / 64) * ((Cout + 63) / 64)), (unsigned)sp.splits);
  const size_t total = (size_t)Cin * Cout * 9;
  const long long plane = (long long)Ho * Wo;
  const int chunks = bias_grad_chunks(plane);
  const long long per_chunk = (plane + chunks - 1) / chunks;
  double* bias_part = reinterpret_cast<double*>(workspace);      // [Cout][chunks]
  if constexpr (SCALED) {
    hipLaunchKernelGGL((dd_conv_wgrad_scaled_kernel<PREC, 3, 2, 1, RH, RAGGED>), grid, dim3(kThreads), 0, st, grad_y, x, part, Cout, Cin, Ho, Wo, H, W,
                       tiles_x, tiles_y, (long long)sp.tiles, sp.tiles_per_split, scale);
    hipLaunchKernelGGL(dd_conv_wgrad_reduce_scaled_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, st, (const float*)part, grad_w, total, sp.splits,
                       scale);
    if (grad_bias) {      // (the reduce above has read the partial sums: the workspace is free again)
      hipLaunchKernelGGL((dd_conv_bias_grad_scaled_kernel<PREC>), dim3((unsigned)Cout, (unsigned)chunks), dim3(kThreads), 0, st, grad_y, bias_part, B, Cout,
                         plane, per_chunk, scale);
      hipLaunchKernelGGL(dd_conv_bias_grad_reduce_scaled_kernel, dim3(blocks_for((size_t)Cout)), dim3(kThreads), 0, st, (const double*)bias_part, grad_bias,
                         Cout, chunks, scale);
    }
  } else {
    hipLaunchKernelGGL((dd_conv_wgrad_kernel<PREC, 3, 2, 1, RH, RAGGED>), grid, dim3(kThreads), 0, st, grad_y, x, part, Cout, Cin, Ho, Wo, H, W, tiles_x,
                       tiles_y, (long long)sp.tiles, sp.tiles_per_split);
    hipLaunchKernelGGL(dd_conv_wgrad_reduce_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, st, (const float*)part, grad_w, total, sp.splits);
    if (grad_bias) {
      hipLaunchKernelGGL((dd_conv_bias_grad_kernel<PREC>), dim3((unsigned)Cout, (unsigned)chunks), dim3(kThreads), 0, st, grad_y, bias_part, B, Cout, plane,
                         per_chunk);
      hipLaunchKernelGGL(dd_conv_bias_grad_reduce_kernel, dim3(blocks_for((size_t)Cout)), dim3(kThreads), 0, st, (const double*)bias_part, grad_bias, Cout,
                         chunks);
    }
  }
  return hipGetLastError();
}

// ---- the folded eval-mode forward (include/ddepth_conv_fused.h) ---------------------------------------------------------------------------------------
// pack as the forward of the stride's operator packs, then the implicit GEMM of that row of the table with the affine epilogue
template <int PREC, bool RAGGED>
hipError_t launch_affine_prec(int stride, const float* x, const float* w, const float* scale_shift, const float* addend, float* y, void* workspace,
                              int relu, int B, int Cin, int Cout, int H, int W, hipStream_t st) {
  const GemmShape g = gemm_shape(stride == 2 ? kOpConv3S2 : kOpConv3, 0, Cin, Cout);
  const int Ho = stride == 2 ? strided_out(H) : H, Wo = stride == 2 ? strided_out(W) : W;
  uint16_t* wh = reinterpret_cast<uint16_t*>(workspace);
  uint16_t* wl = wh + packed_halfs(g);
  hipLaunchKernelGGL((dd_conv_pack_kernel<PREC, RAGGED>), dim3(blocks_for(packed_halfs(g))), dim3(kThreads), 0, st, w, wh, wl, g.pack_mode, g.N, g.K,
                     g.taps, g.kstep);
  const int tiles_x = (Wo + kTileW - 1) / kTileW, tiles_y = (Ho + kTileH - 1) / kTileH;
  const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)((g.N + kTileN - 1) / kTileN), (unsigned)B);
  if (stride == 2) {
    constexpr GemmKind k = gemm_kind(kOpConv3S2, 0);
    hipLaunchKernelGGL((dd_conv_igemm_affine_kernel<PREC, k.ks, k.stride, k.pad, k.kstep, k.scatter, RAGGED>), grid, dim3(kThreads), 0, st, x,
                       (const uint16_t*)wh, (const uint16_t*)wl, y, g.K, g.N, H, W, Ho, Wo, tiles_x, scale_shift, addend, relu);
  } else {
    constexpr GemmKind k = gemm_kind(kOpConv3, 0);
    hipLaunchKernelGGL((dd_conv_igemm_affine_kernel<PREC, k.ks, k.stride, k.pad, k.kstep, k.scatter, RAGGED>), grid, dim3(kThreads), 0, st, x,
                       (const uint16_t*)wh, (const uint16_t*)wl, y, g.K, g.N, H, W, Ho, Wo, tiles_x, scale_shift, addend, relu);
  }
  return hipGetLastError();
}

// ---- the statistics-emitting forward (include/ddepth_conv_stats.h) ------------------------------------------------------------------------------------
// the weight image (twice in the split mode), rounded up to 256 bytes: where the partials start
size_t stats_packed_bytes(int stride, int Cin, int Cout, int prec) {
  const size_t packed = packed_halfs(gemm_shape(stride == 2 ? kOpConv3S2 : kOpConv3, 0, Cin, Cout)) * sizeof(uint16_t) * (prec == kPrecF16x3 ? 2 : 1);
  return (packed + 255) / 256 * 256;
}

// pack as the forward of the stride's operator packs, the implicit GEMM of that row of the table with the statistics epilogue, then the combine
template <int PREC, bool RAGGED>
hipError_t launch_stats_prec(int stride, const float* x, const float* w, const float* bias, float* y, double* sums, void* workspace, int B, int Cin,
                             int Cout, int H, int W, hipStream_t st) {
  const GemmShape g = gemm_shape(stride == 2 ? kOpConv3S2 : kOpConv3, 0, Cin, Cout);
  const int Ho = stride == 2 ? strided_out(H) : H, Wo = stride == 2 ? strided_out(W) : W;
  uint16_t* wh = reinterpret_cast<uint16_t*>(workspace);
  uint16_t* wl = wh + packed_halfs(g);
  double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + stats_packed_bytes(stride, Cin, Cout, PREC));
  hipLaunchKernelGGL((dd_conv_pack_kernel<PREC, RAGGED>), dim3(blocks_for(packed_halfs(g))), dim3(kThreads), 0, st, w, wh, wl, g.pack_mode, g.N, g.K,
                     g.taps, g.kstep);
  const int tiles_x = (Wo + kTileW - 1) / kTileW, tiles_y = (Ho + kTileH - 1) / kTileH;
  const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)((g.N + kTileN - 1) / kTileN), (unsigned)B);
  if (stride == 2) {
    constexpr GemmKind k = gemm_kind(kOpConv3S2, 0);
    hipLaunchKernelGGL((dd_conv_igemm_stats_kernel<PREC, k.ks, k.stride, k.pad, k.kstep, k.scatter, RAGGED>), grid, dim3(kThreads), 0, st, x,
                       (const uint16_t*)wh, (const uint16_t*)wl, y, g.K, g.N, H, W, Ho, Wo, tiles_x, bias, part);
  } else {
    constexpr GemmKind k = gemm_kind(kOpConv3, 0);
    hipLaunchKernelGGL((dd_conv_igemm_stats_kernel<PREC, k.ks, k.stride, k.pad, k.kstep, k.scatter, RAGGED>), grid, dim3(kThreads), 0, st, x,
                       (const uint16_t*)wh, (const uint16_t*)wl, y, g.K, g.N, H, W, Ho, Wo, tiles_x, bias, part);
  }
  hipLaunchKernelGGL(dd_conv_stats_combine_kernel, dim3((unsigned)Cout), dim3(kThreads), 0, st, (const double*)part, sums, B * tiles_x * tiles_y, Cout,
                     (double)B * (double)Ho * (double)Wo);
  return hipGetLastError();
}

}  // namespace

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------------
WgradSplit wgrad_split(int op, int B, int H, int W) {
  WgradSplit s;
  if (op == kOpConv1) s.tiles = (int64_t)B * (((int64_t)H * W + kPwTile - 1) / kPwTile);      // flat tiles, none across an image
  else s.tiles = (int64_t)B * ((H + wgrad_rows(op) - 1) / wgrad_rows(op)) * ((W + 31) / 32);
  int64_t per = (s.tiles + kMaxSplits - 1) / kMaxSplits;
  if (per < kSplitTiles) per = kSplitTiles;
  s.tiles_per_split = (int)per;
  s.splits = (int)((s.tiles + per - 1) / per);
  return s;
}

bool block64(int Cin, int Cout) { return channels_block64(Cin) && channels_block64(Cout); }

size_t packed_halfs(int op, int dir, int Cin, int Cout) { return packed_halfs(gemm_shape(op, dir, Cin, Cout)); }

size_t workspace_bytes(int op, int B, int Cin, int Cout, int H, int W, int prec) {
  const size_t fwd = packed_halfs(op, 0, Cin, Cout), bwd = packed_halfs(op, 1, Cin, Cout);
  const size_t packed = (fwd > bwd ? fwd : bwd) * sizeof(uint16_t) * (prec == kPrecF16x3 ? 2 : 1);      // hi, and lo behind it in the split mode
  const size_t partials = (size_t)wgrad_split(op, B, H, W).splits * (size_t)taps_of(op) * (size_t)Cin * (size_t)Cout * sizeof(float);
  const size_t need = packed > partials ? packed : partials;
  return (need + 255) / 256 * 256;
}

hipError_t launch_conv(int op, int dir, const float* in, const float* w, float* out, void* workspace, int B, int Cin, int Cout, int H, int W,
                       int prec, hipStream_t st, const float* scale) {
  return dispatch(prec, Cin, Cout, scale != nullptr && dir == 1, [&](auto p, auto ragged, auto scaled) {
    return launch_conv_prec<decltype(p)::value, decltype(ragged)::value, decltype(scaled)::value>(op, dir, in, w, out, workspace, scale, B, Cin, Cout,
                                                                                                  H, W, st);
  });
}

hipError_t launch_wgrad(int op, const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H, int W,
                        int prec, hipStream_t st, const float* scale) {
  return dispatch(prec, Cin, Cout, scale != nullptr, [&](auto p, auto ragged, auto scaled) {
    return launch_wgrad_prec<decltype(p)::value, decltype(ragged)::value, decltype(scaled)::value>(op, x, grad_y, grad_w, workspace, scale, B, Cin,
                                                                                                   Cout, H, W, st);
  });
}

hipError_t launch_grad_scale(const float* grad_y, int64_t n, int prec, int amax_exp, float* scale, hipStream_t st) {
  if (hipError_t e = hipMemsetAsync(scale, 0, 4 * sizeof(float), st)) return e;
  if (prec != kPrecBf16 && n > 0) {
    const int64_t want = (n + 4 * kThreads - 1) / (4 * kThreads);      // four elements per thread and turn of the loop
    hipLaunchKernelGGL(dd_conv_grad_amax_kernel, dim3((unsigned)(want < kAmaxBlocks ? want : kAmaxBlocks)), dim3(kThreads), 0, st, grad_y, (long long)n,
                       reinterpret_cast<unsigned*>(scale) + 2);
  }
  hipLaunchKernelGGL(dd_conv_grad_scale_pair_kernel, dim3(1), dim3(1), 0, st, scale, amax_exp);
  return hipGetLastError();
}

// ---- 3x3 stride 2 ----------------------------------------------------------------------------------------------------------------------------------
size_t workspace_bytes_s2(int B, int Cin, int Cout, int H, int W, int prec) {
  const size_t fwd = packed_halfs(kOpConv3S2, 0, Cin, Cout), bwd = packed_halfs(kOpConv3S2, 1, Cin, Cout);
  const size_t packed = (fwd > bwd ? fwd : bwd) * sizeof(uint16_t) * (prec == kPrecF16x3 ? 2 : 1);
  const size_t partials = (size_t)wgrad_split(kOpConv3S2, B, strided_out(H), strided_out(W)).splits * 9 * (size_t)Cin * (size_t)Cout * sizeof(float);
  const size_t bias_part = (size_t)Cout * (size_t)bias_grad_chunks((long long)strided_out(H) * strided_out(W)) * sizeof(double);
  size_t need = packed > partials ? packed : partials;
  if (bias_part > need) need = bias_part;      // (the weight gradient's partials, at least 36 Cin bytes per output channel and split, are the larger)
  return (need + 255) / 256 * 256;
}

hipError_t launch_conv_s2_forward(const float* x, const float* w, const float* bias, float* y, void* workspace, int B, int Cin, int Cout, int H, int W,
                                  int prec, hipStream_t st) {
  return dispatch(prec, Cin, Cout, false, [&](auto p, auto ragged, auto scaled) {
    return launch_s2_prec<decltype(p)::value, decltype(ragged)::value, decltype(scaled)::value>(0, x, w, bias, y, workspace, nullptr, B, Cin, Cout, H,
                                                                                                W, st);
  });
}

hipError_t launch_conv_s2_dgrad(const float* grad_y, const float* w, float* grad_x, void* workspace, int B, int Cin, int Cout, int H, int W, int prec,
                                hipStream_t st, const float* scale) {
  return dispatch(prec, Cin, Cout, scale != nullptr, [&](auto p, auto ragged, auto scaled) {
    return launch_s2_prec<decltype(p)::value, decltype(ragged)::value, decltype(scaled)::value>(1, grad_y, w, nullptr, grad_x, workspace, scale, B,
                                                                                                Cin, Cout, H, W, st);
  });
}

hipError_t launch_conv_s2_wgrad(const float* x, const float* grad_y, float* grad_w, float* grad_bias, void* workspace, int B, int Cin, int Cout, int H,
                                int W, int prec, hipStream_t st, const float* scale) {
  return dispatch(prec, Cin, Cout, scale != nullptr, [&](auto p, auto ragged, auto scaled) {
    return launch_s2_wgrad_prec<decltype(p)::value, decltype(ragged)::value, decltype(scaled)::value>(x, grad_y, grad_w, grad_bias, workspace, scale,
                                                                                                      B, Cin, Cout, H, W, st);
  });
}

// ---- the folded eval-mode forward --------------------------------------------------------------------------------------------------------------------
size_t workspace_bytes_affine(int stride, int Cin, int Cout, int prec) {
  const size_t packed = packed_halfs(stride == 2 ? kOpConv3S2 : kOpConv3, 0, Cin, Cout) * sizeof(uint16_t) * (prec == kPrecF16x3 ? 2 : 1);
  return (packed + 255) / 256 * 256;
}

hipError_t launch_bn_fold(const float* weight, const float* bias, const float* mean, const float* var, double eps, const float* conv_bias,
                          float* scale_shift, int C, hipStream_t st) {
  hipLaunchKernelGGL(dd_bn_fold_kernel, dim3(blocks_for((size_t)C)), dim3(kThreads), 0, st, weight, bias, mean, var, eps, conv_bias, scale_shift, C);
  return hipGetLastError();
}

hipError_t launch_conv_affine(int stride, const float* x, const float* w, const float* scale_shift, const float* addend, float* y, void* workspace,
                              int relu, int B, int Cin, int Cout, int H, int W, int prec, hipStream_t st) {
  return dispatch(prec, Cin, Cout, false, [&](auto p, auto ragged, auto) {
    return launch_affine_prec<decltype(p)::value, decltype(ragged)::value>(stride, x, w, scale_shift, addend, y, workspace, relu, B, Cin, Cout, H, W,
                                                                           st);
  });
}

// ---- the statistics-emitting forward ------------------------------------------------------------------------------------------------------------------
size_t workspace_bytes_stats(int stride, int B, int Cin, int Cout, int H, int W, int prec) {
  const int Ho = stride == 2 ? strided_out(H) : H, Wo = stride == 2 ? strided_out(W) : W;
  const size_t tiles = (size_t)((Wo + kTileW - 1) / kTileW) * (size_t)((Ho + kTileH - 1) / kTileH);
  const size_t partials = (size_t)Cout * (size_t)B * tiles * 2 * sizeof(double);
  return stats_packed_bytes(stride, Cin, Cout, prec) + (partials + 255) / 256 * 256;
}

hipError_t launch_conv_stats(int stride, const float* x, const float* w, const float* bias, float* y, double* sums, void* workspace, int B, int Cin,
                             int Cout, int H, int W, int prec, hipStream_t st) {
  return dispatch(prec, Cin, Cout, false, [&](auto p, auto ragged, auto) {
    return launch_stats_prec<decltype(p)::value, decltype(ragged)::value>(stride, x, w, bias, y, sums, workspace, B, Cin, Cout, H, W, st);
  });
}

}  // namespace ddconv
