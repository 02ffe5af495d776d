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
enum { kPackConvFwd = 0, kPackConvBwd = 1, kPackDeconvFwd = 2, kPackDeconvBwd = 3, kPackPwFwd = 4, kPackPwBwd = 5 };

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
  } else {                                // 1x1 data gradient: w'[ci = n][co = k] = w[co][ci]
    src = (size_t)k * N + n;
  }
  uint16_t hi, lo;
  to_operand<PREC>(w[src], hi, lo);
  wh[idx] = hi;
  if constexpr (PREC == kPrecF16x3) wl[idx] = lo;
}

// ---- forward and data gradient --------------------------------------------------------------------------------------------------------------------
// in [B][K][Hin][Win], wp [KS * KS][N][K]; grid (tiles, N / 64, B).  The tile grid is Ht x Wt pixels:
//   !SCATTER: out [B][N][Ht][Wt], pixel (y, x) of the tile grid reads input pixels (y * S - PAD + ky, x * S - PAD + kx)
//   SCATTER:  out [B][N / 4][2 Ht][2 Wt], GEMM column n = (dy * 2 + dx) * (N / 4) + co goes to pixel (2y + dy, 2x + dx) of plane co
// RAGGED (K, N multiples of 8, not of the tiles): the weight image is the padded one of the pack kernel, channels >= K are filled as zeros, rows
// >= N are not stored, and grid y is ceil(N / 64).  The K chunks and their order are those of the block-64 instantiation.
template <int PREC, int KS, int S, int PAD, int KC, bool SCATTER, bool RAGGED>
__global__ __launch_bounds__(kThreads) void dd_conv_igemm_kernel(const float* __restrict__ in, const uint16_t* __restrict__ wh,
                                                                 const uint16_t* __restrict__ wl, float* __restrict__ out, int K, int N,
                                                                 int Hin, int Win, int Ht, int Wt, int tiles_x) {
  constexpr int PH = (kTileH - 1) * S + KS, PW = (kTileW - 1) * S + KS, PP = PH * PW;
  constexpr int PS = KC + 8;      // halfs per patch pixel: a multiple of 8, so every 16-byte read is aligned
  constexpr int NL = PREC == kPrecF16x3 ? 2 : 1;
  __shared__ uint16_t patch[NL][PP * PS] __attribute__((aligned(16)));

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x, n0 = blockIdx.y * kTileN, b = blockIdx.z;
  const int iy0 = ty * kTileH * S - PAD, ix0 = tx * kTileW * S - PAD;
  const size_t plane = (size_t)Hin * Win;
  const float* inb = in + (size_t)b * K * plane;
  const int Kp = RAGGED ? padded(K, KC) : K, Np = RAGGED ? padded(N, kTileN) : N;      // the weight image's row length and rows per tap

  f32x16_t acc[2];
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc[0][i] = 0.0f; acc[1][i] = 0.0f; }

  for (int kc = 0; kc < K; kc += KC) {
    __syncthreads();      // the previous chunk's reads are over
    // consecutive lanes: consecutive pixels of one plane; kFillBatch loads are issued before the first one is converted
    for (int base = tid; base < KC * PP; base += kThreads * kFillBatch) {
      float v[kFillBatch];
#pragma unroll
      for (int j = 0; j < kFillBatch; ++j) {
        const int idx = base + j * kThreads, ch = idx / PP, rem = idx - ch * PP, pr = rem / PW, pc = rem - pr * PW;
        const int iy = iy0 + pr, ix = ix0 + pc;
        v[j] = 0.0f;
        if (idx < KC * PP && (!RAGGED || kc + ch < K) && iy >= 0 && iy < Hin && ix >= 0 && ix < Win)
          v[j] = inb[(size_t)(kc + ch) * plane + (size_t)iy * Win + ix];
      }
#pragma unroll
      for (int j = 0; j < kFillBatch; ++j) {
        const int idx = base + j * kThreads, ch = idx / PP, rem = idx - ch * PP;
        if (idx >= KC * PP) break;
        uint16_t hi, lo;
        to_operand<PREC>(v[j], hi, lo);
        patch[0][rem * PS + ch] = hi;
        if constexpr (PREC == kPrecF16x3) patch[NL - 1][rem * PS + ch] = lo;
      }
    }
    __syncthreads();
#pragma unroll
    for (int ky = 0; ky < KS; ++ky) {
#pragma unroll
      for (int kx = 0; kx < KS; ++kx) {
        const int pp = ((wave * S + ky) * PW + (l32 * S + kx)) * PS + 8 * half;
        const size_t wrow = ((size_t)(ky * KS + kx) * Np + n0 + l32) * Kp + kc + 8 * half;
#pragma unroll
        for (int kk = 0; kk < KC; kk += 16) {
          const uint4 bh = *reinterpret_cast<const uint4*>(&patch[0][pp + kk]);
          uint4 bl = bh;
          if constexpr (PREC == kPrecF16x3) bl = *reinterpret_cast<const uint4*>(&patch[NL - 1][pp + kk]);
#pragma unroll
          for (int nb = 0; nb < 2; ++nb) {
            const size_t wo = wrow + (size_t)nb * 32 * Kp + kk;
            const uint4 ah = *reinterpret_cast<const uint4*>(wh + wo);
            uint4 al = ah;
            if constexpr (PREC == kPrecF16x3) al = *reinterpret_cast<const uint4*>(wl + wo);
            acc[nb] = mma_pair<PREC>(ah, al, bh, bl, acc[nb]);
          }
        }
      }
    }
  }

  // accumulator entry r of lane l: column (pixel) l % 32, row (output channel) 8 * (r / 4) + 4 * (l / 32) + r % 4
  const int y = ty * kTileH + wave, x = tx * kTileW + l32;
  if (y >= Ht || x >= Wt) return;
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + nb * 32 + 8 * (r / 4) + 4 * half + (r % 4);
      if constexpr (RAGGED) {
        if (n >= N) continue;
      }
      if constexpr (SCATTER) {
        const int cout = N / 4, t4 = n / cout, co = n - t4 * cout;
        const size_t oy = 2 * (size_t)y + (t4 >> 1), ox = 2 * (size_t)x + (t4 & 1);
        out[(((size_t)b * cout + co) * (2 * (size_t)Ht) + oy) * (2 * (size_t)Wt) + ox] = acc[nb][r];
      } else {
        out[(((size_t)b * N + n) * Ht + y) * (size_t)Wt + x] = acc[nb][r];
      }
    }
  }
}

// ---- weight gradient --------------------------------------------------------------------------------------------------------------------------------
constexpr int wgrad_channel_stride(int halfs) {      // halfs between two channels of the shifted operand in LDS: an ODD number of dwords
  const int even = (halfs + 1) / 2 * 2;
  return (even / 2) % 2 == 0 ? even + 2 : even;
}

// P [B][Cp][Hp][Wp] is read at the pixel itself, Q [B][Cq][Hq][Wq] at (y * S - PAD + ky, x * S - PAD + kx):
//   3x3:        P = grad_y, Q = x       -> grad_w[co][ci][ky][kx]          transpose convolution:  P = x, Q = grad_y -> grad_w[ci][co][dy][dx]
// part [splits][Cp][Cq][KS * KS]; grid ((Cp / 64) * (Cq / 64), splits).  A pixel tile is RH rows of 32 pixels.
// RAGGED: grid x is ceil(Cp / 64) * ceil(Cq / 64); channel rows >= Cp / Cq are filled as zeros and not stored (part keeps the real counts).
template <int PREC, int KS, int S, int PAD, int RH, bool RAGGED>
__global__ __launch_bounds__(kThreads) void dd_conv_wgrad_kernel(const float* __restrict__ P, const float* __restrict__ Q, float* __restrict__ part,
                                                                 int Cp, int Cq, int Hp, int Wp, int Hq, int Wq, int tiles_x, int tiles_y,
                                                                 long long tiles, int tiles_per_split) {
  constexpr int T = KS * KS;
  constexpr int QH = (RH - 1) * S + KS, QW = 31 * S + KS, QP = QH * QW, QCS = wgrad_channel_stride(QP);
  constexpr int PP = RH * 32, PCS = PP + 8;      // a multiple of 8 halfs: the A operand's 16-byte reads are aligned
  constexpr int NQ = 7 * S + KS;                 // values of one row of Q that the 8 pixels of a lane touch, all kx together
  constexpr int NL = PREC == kPrecF16x3 ? 2 : 1;
  __shared__ uint16_t PL[NL][64 * PCS] __attribute__((aligned(16)));
  __shared__ uint16_t QL[NL][64 * QCS] __attribute__((aligned(16)));

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const int nq = RAGGED ? (Cq + 63) / 64 : Cq / 64, p0 = (blockIdx.x / nq) * 64, q0 = (blockIdx.x % nq) * 64, split = blockIdx.y;
  const int wp = wave & 1, wq = wave >> 1;
  const size_t plane_p = (size_t)Hp * Wp, plane_q = (size_t)Hq * Wq;

  f32x16_t acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;

  const long long t_begin = (long long)split * tiles_per_split;
  const long long t_end = t_begin + tiles_per_split < tiles ? t_begin + tiles_per_split : tiles;
  for (long long t = t_begin; t < t_end; ++t) {
    const int txi = (int)(t % tiles_x), tyi = (int)((t / tiles_x) % tiles_y), b = (int)(t / ((long long)tiles_x * tiles_y));
    const int y0 = tyi * RH, x0 = txi * 32;
    const int qy0 = y0 * S - PAD, qx0 = x0 * S - PAD;
    __syncthreads();      // the previous tile's reads are over
    for (int base = tid; base < 64 * PP; base += kThreads * kFillBatch) {      // (kFillBatch loads in flight, as in the implicit GEMM)
      float v[kFillBatch];
#pragma unroll
      for (int j = 0; j < kFillBatch; ++j) {
        const int idx = base + j * kThreads, ch = idx / PP, rem = idx - ch * PP, y = y0 + rem / 32, x = x0 + rem % 32;
        v[j] = 0.0f;
        if (idx < 64 * PP && (!RAGGED || p0 + ch < Cp) && y < Hp && x < Wp) v[j] = P[((size_t)b * Cp + p0 + ch) * plane_p + (size_t)y * Wp + x];
      }
#pragma unroll
      for (int j = 0; j < kFillBatch; ++j) {
        const int idx = base + j * kThreads, ch = idx / PP, rem = idx - ch * PP;
        if (idx >= 64 * PP) break;
        uint16_t hi, lo;
        to_operand<PREC>(v[j], hi, lo);
        PL[0][ch * PCS + rem] = hi;
        if constexpr (PREC == kPrecF16x3) PL[NL - 1][ch * PCS + rem] = lo;
      }
    }
    for (int base = tid; base < 64 * QP; base += kThreads * kFillBatch) {
      float v[kFillBatch];
#pragma unroll
      for (int j = 0; j < kFillBatch; ++j) {
        const int idx = base + j * kThreads, ch = idx / QP, rem = idx - ch * QP, qr = rem / QW, y = qy0 + qr, x = qx0 + (rem - qr * QW);
        v[j] = 0.0f;
        if (idx < 64 * QP && (!RAGGED || q0 + ch < Cq) && y >= 0 && y < Hq && x >= 0 && x < Wq) v[j] = Q[((size_t)b * Cq + q0 + ch) * plane_q + (size_t)y * Wq + x];
      }
#pragma unroll
      for (int j = 0; j < kFillBatch; ++j) {
        const int idx = base + j * kThreads, ch = idx / QP, rem = idx - ch * QP;
        if (idx >= 64 * QP) break;
        uint16_t hi, lo;
        to_operand<PREC>(v[j], hi, lo);
        QL[0][ch * QCS + rem] = hi;
        if constexpr (PREC == kPrecF16x3) QL[NL - 1][ch * QCS + rem] = lo;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RH; ++r) {
#pragma unroll
      for (int k16 = 0; k16 < 32; k16 += 16) {
        const int po = (wp * 32 + l32) * PCS + r * 32 + k16 + 8 * half;
        const uint4 ah = *reinterpret_cast<const uint4*>(&PL[0][po]);
        uint4 al = ah;
        if constexpr (PREC == kPrecF16x3) al = *reinterpret_cast<const uint4*>(&PL[NL - 1][po]);
#pragma unroll
        for (int ky = 0; ky < KS; ++ky) {
          const int qo = (wq * 32 + l32) * QCS + (r * S + ky) * QW + (k16 + 8 * half) * S;
          uint16_t qh[NQ], ql[NQ];
#pragma unroll
          for (int i = 0; i < NQ; ++i) {
            qh[i] = QL[0][qo + i];
            ql[i] = PREC == kPrecF16x3 ? QL[NL - 1][qo + i] : (uint16_t)0;
          }
#pragma unroll
          for (int kx = 0; kx < KS; ++kx) {
            u16x8_t vh, vl;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              vh[e] = qh[e * S + kx];
              vl[e] = ql[e * S + kx];
            }
            acc[ky * KS + kx] = mma_pair<PREC>(ah, al, __builtin_bit_cast(uint4, vh), __builtin_bit_cast(uint4, vl), acc[ky * KS + kx]);
          }
        }
      }
    }
  }

  // accumulator entry r of lane l: column q = l % 32, row p = 8 * (r / 4) + 4 * (l / 32) + r % 4
  float* dst = part + (size_t)split * Cp * Cq * T;
  const int q = q0 + wq * 32 + l32;
#pragma unroll
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int p = p0 + wp * 32 + 8 * (r / 4) + 4 * half + (r % 4);
      if constexpr (RAGGED) {
        if (p >= Cp || q >= Cq) continue;
      }
      dst[((size_t)p * Cq + q) * T + t] = acc[t][r];
    }
  }
}

// ---- 1x1: forward and data gradient ---------------------------------------------------------------------------------------------------------------
// out[b][n][p] = sum_k wp[n][k] . in[b][k][p] over the FLAT pixels p of a plane (P = H * W): no halo, so a workgroup owns kPwTile consecutive
// pixels of one plane (wave w the 32 from 32 w on) and 32 * NB output channels; a tile never crosses an image, what lies behind the plane's end
// is read as zero and not written.  Lane l of the MFMA's pixel-side operand needs channels k + 8 * (l / 32) .. + 7 of pixel l % 32: eight dword
// loads, each one 32 consecutive floats of one plane (any P, any alignment), converted in registers and already in operand order -- no LDS and no
// barrier in this kernel.  The weights are the A operand, 16 bytes per lane from the packed image (L1 / L2), as in the implicit GEMM.
// grid (pixel tiles * N / (32 NB), B): the workgroups of one pixel tile are neighbours in dispatch order, so its re-reads for the other output
// channels meet the cache.
// RAGGED (K, N multiples of 8): the weight image is the padded one of the pack kernel (rows of K rounded up to kPwKStep, N rounded up to 64 rows); the
// pixel-side loads are guarded per 8-channel lane-half group -- K is a multiple of 8, so a tail is always a whole group -- and rows >= N are not
// stored; N / (32 NB) rounds up.
template <int PREC, int NB, bool RAGGED>
__global__ __launch_bounds__(kThreads) void dd_conv1x1_gemm_kernel(const float* __restrict__ in, const uint16_t* __restrict__ wh,
                                                                   const uint16_t* __restrict__ wl, float* __restrict__ out, int K, int N, int P) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const int Kp = RAGGED ? padded(K, kPwKStep) : K;      // the weight image's row length
  const int nblocks = RAGGED ? (N + 32 * NB - 1) / (32 * NB) : N / (32 * NB);
  const int n0 = (int)(blockIdx.x % (unsigned)nblocks) * (32 * NB), b = blockIdx.y;
  const int pw = (int)(blockIdx.x / (unsigned)nblocks) * kPwTile + wave * 32;      // first pixel of this wave
  if (pw >= P) return;                                                             // (the whole wave: nothing here waits for it)
  const int p = pw + l32;
  const bool live = p < P;
  const float* src = in + ((size_t)b * K + 8 * half) * (size_t)P + (live ? p : 0);
  const uint16_t* wrow = wh + (size_t)(n0 + l32) * Kp + 8 * half;
  const uint16_t* wrow_lo = wl + (size_t)(n0 + l32) * Kp + 8 * half;

  f32x16_t acc[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nb][i] = 0.0f;

  for (int kc = 0; kc < K; kc += kPwKStep) {      // (!RAGGED: K is a multiple of 64) sixteen loads in flight, then two MFMA steps
    float v[2][8];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bool take = live && (!RAGGED || kc + 16 * s + 8 * half < K);      // this lane's eight channels: all below K, or none
#pragma unroll
      for (int e = 0; e < 8; ++e) v[s][e] = take ? src[(size_t)(kc + 16 * s + e) * P] : 0.0f;
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      u16x8_t vh, vl;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        uint16_t hi, lo;
        to_operand<PREC>(v[s][e], hi, lo);
        vh[e] = hi;
        vl[e] = lo;
      }
      const uint4 bh = __builtin_bit_cast(uint4, vh), bl = __builtin_bit_cast(uint4, vl);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        const size_t wo = (size_t)nb * 32 * Kp + kc + 16 * s;
        const uint4 ah = *reinterpret_cast<const uint4*>(wrow + wo);
        uint4 al = ah;
        if constexpr (PREC == kPrecF16x3) al = *reinterpret_cast<const uint4*>(wrow_lo + wo);
        acc[nb] = mma_pair<PREC>(ah, al, bh, bl, acc[nb]);
      }
    }
  }

  // accumulator entry r of lane l: column (pixel) l % 32, row (output channel) 8 * (r / 4) + 4 * (l / 32) + r % 4
  if (!live) return;
  float* dst = out + ((size_t)b * N + n0 + 4 * half) * (size_t)P + p;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = nb * 32 + 8 * (r / 4) + (r % 4);
      if constexpr (RAGGED) {
        if (n0 + 4 * half + row >= N) continue;
      }
      dst[(size_t)row * P] = acc[nb][r];
    }
}

// ---- 1x1: weight gradient -----------------------------------------------------------------------------------------------------------------------------
// part[split][cp][cq] = sum over the split's pixels of Pm[b][cp][p] . Q[b][cq][p]  (Pm = grad_y, Q = x -> grad_w[co][ci]): the contraction runs over
// the pixels, contiguous in memory for BOTH operands and shifted for neither.  A workgroup owns 64 x 64 channels and a contiguous range of pixel
// tiles (a SPLIT, in a fixed order), a tile being kPwTile consecutive pixels of one plane (zero behind its end).  Fill: a wave reads one channel
// row of the tile with two dword loads per lane, pixels l and 64 + l (coalesced, any alignment), and stores them as ONE dword at slots 2 l,
// 2 l + 1 of the channel's LDS row -- the MFMA's K runs over the slots, and both operands use the same pixel -> slot map, so the products pair up
// the same pixels.  Dword stores of consecutive lanes to consecutive addresses, 16-byte operand reads from rows of kPwTile + 8 halfs (the four
// 16-lane groups of a 16-byte read meet every bank once): no 2-byte scatter or gather anywhere.
// RAGGED: as in dd_conv_wgrad_kernel -- the grid rounds the channel blocks up, rows >= Cp / Cq are filled as zeros and not stored.
template <int PREC, bool RAGGED>
__global__ __launch_bounds__(kThreads) void dd_conv1x1_wgrad_kernel(const float* __restrict__ Pm, const float* __restrict__ Q, float* __restrict__ part,
                                                                    int Cp, int Cq, int P, int tiles_per_plane, long long tiles, int tiles_per_split) {
  constexpr int RS = kPwTile + 8;      // halfs per channel row
  constexpr int NL = PREC == kPrecF16x3 ? 2 : 1;
  constexpr int kFillChannels = kFillBatch / 2;      // channel rows a wave has in flight (two loads each)
  __shared__ uint16_t PL[NL][64 * RS] __attribute__((aligned(16)));
  __shared__ uint16_t QL[NL][64 * RS] __attribute__((aligned(16)));

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const int nq = RAGGED ? (Cq + 63) / 64 : Cq / 64, p0 = (blockIdx.x / nq) * 64, q0 = (blockIdx.x % nq) * 64, split = blockIdx.y;
  const int wp = wave & 1, wq = wave >> 1;

  f32x16_t acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0f;

  const long long t_begin = (long long)split * tiles_per_split;
  const long long t_end = t_begin + tiles_per_split < tiles ? t_begin + tiles_per_split : tiles;
  for (long long t = t_begin; t < t_end; ++t) {
    const int b = (int)(t / tiles_per_plane), px = (int)(t % tiles_per_plane) * kPwTile + lane;
    const bool live0 = px < P, live1 = px + 64 < P;
    __syncthreads();      // the previous tile's reads are over
    // rows 0..63 are Pm's channels, 64..127 Q's; wave w fills rows w, w + 4, ...
    for (int r0 = wave; r0 < 128; r0 += 4 * kFillChannels) {
      float v[kFillChannels][2];
#pragma unroll
      for (int j = 0; j < kFillChannels; ++j) {
        const int row = r0 + 4 * j;
        const float* g = row < 64 ? Pm + ((size_t)b * Cp + p0 + row) * (size_t)P : Q + ((size_t)b * Cq + q0 + row - 64) * (size_t)P;
        bool take0 = live0, take1 = live1;
        if constexpr (RAGGED) {
          const bool in_range = row < 64 ? p0 + row < Cp : q0 + row - 64 < Cq;
          take0 = take0 && in_range;
          take1 = take1 && in_range;
        }
        v[j][0] = take0 ? g[px] : 0.0f;
        v[j][1] = take1 ? g[px + 64] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < kFillChannels; ++j) {
        const int row = r0 + 4 * j;
        uint16_t h0, l0, h1, l1;
        to_operand<PREC>(v[j][0], h0, l0);
        to_operand<PREC>(v[j][1], h1, l1);
        uint16_t* dh = row < 64 ? &PL[0][row * RS] : &QL[0][(row - 64) * RS];
        *reinterpret_cast<uint32_t*>(dh + 2 * lane) = (uint32_t)h0 | ((uint32_t)h1 << 16);
        if constexpr (PREC == kPrecF16x3) {
          uint16_t* dl = row < 64 ? &PL[NL - 1][row * RS] : &QL[NL - 1][(row - 64) * RS];
          *reinterpret_cast<uint32_t*>(dl + 2 * lane) = (uint32_t)l0 | ((uint32_t)l1 << 16);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int k16 = 0; k16 < kPwTile; k16 += 16) {
      const int po = (wp * 32 + l32) * RS + k16 + 8 * half, qo = (wq * 32 + l32) * RS + k16 + 8 * half;
      const uint4 ah = *reinterpret_cast<const uint4*>(&PL[0][po]);
      const uint4 bh = *reinterpret_cast<const uint4*>(&QL[0][qo]);
      uint4 al = ah, bl = bh;
      if constexpr (PREC == kPrecF16x3) {
        al = *reinterpret_cast<const uint4*>(&PL[NL - 1][po]);
        bl = *reinterpret_cast<const uint4*>(&QL[NL - 1][qo]);
      }
      acc = mma_pair<PREC>(ah, al, bh, bl, acc);
    }
  }

  // accumulator entry r of lane l: column q = l % 32, row p = 8 * (r / 4) + 4 * (l / 32) + r % 4
  float* dst = part + (size_t)split * Cp * Cq + (size_t)(p0 + wp * 32 + 4 * half) * Cq + q0 + wq * 32 + l32;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    if constexpr (RAGGED) {
      if (p0 + wp * 32 + 4 * half + 8 * (r / 4) + (r % 4) >= Cp || q0 + wq * 32 + l32 >= Cq) continue;
    }
    dst[(size_t)(8 * (r / 4) + (r % 4)) * Cq] = acc[r];
  }
}

// grad_w[i] = part[0][i] + part[1][i] + ... in that order
__global__ __launch_bounds__(kThreads) void dd_conv_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ grad_w, size_t total,
                                                                        int splits) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  float s = part[i];
  for (int k = 1; k < splits; ++k) s += part[(size_t)k * total + i];
  grad_w[i] = s;
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
constexpr int wgrad_rows(int op) { return op == kOpConv3 ? 2 : 1; }

// the implicit GEMM of (OP, DIR), instantiated from its gemm_kind.  H, W = the tile grid (the forward's input size); the input is `stride` times that.
template <int PREC, bool RAGGED, int OP, int DIR>
void launch_igemm(const GemmShape& g, const float* in, const uint16_t* wh, const uint16_t* wl, float* out, int B, int H, int W, hipStream_t st) {
  constexpr GemmKind k = gemm_kind(OP, DIR);
  const int tiles_x = (W + kTileW - 1) / kTileW, tiles_y = (H + kTileH - 1) / kTileH;
  hipLaunchKernelGGL((dd_conv_igemm_kernel<PREC, k.ks, k.stride, k.pad, k.kstep, k.scatter, RAGGED>),
                     dim3((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)((g.N + kTileN - 1) / kTileN), (unsigned)B), dim3(kThreads), 0, st, in, wh,
                     wl, out, g.K, g.N, k.stride * H, k.stride * W, H, W, tiles_x);
}

// RAGGED launches the guarded instantiations: grids round the channel blocks up, the packed image is the padded one (!RAGGED: no pad to add)
template <int PREC, bool RAGGED>
hipError_t launch_conv_prec(int op, int dir, const float* in, const float* w, float* out, void* workspace, int B, int Cin, int Cout, int H, int W,
                            hipStream_t st) {
  const GemmShape g = gemm_shape(op, dir, Cin, Cout);
  uint16_t* wh = reinterpret_cast<uint16_t*>(workspace);
  uint16_t* wl = wh + packed_halfs(g);      // (only the split mode reads or writes it)
  hipLaunchKernelGGL((dd_conv_pack_kernel<PREC, RAGGED>), dim3(blocks_for(packed_halfs(g))), dim3(kThreads), 0, st, w, wh, wl, g.pack_mode, g.N, g.K,
                     g.taps, g.kstep);
  if (op == kOpConv1) {
    const int P = H * W;
    const unsigned ptiles = (unsigned)((P + kPwTile - 1) / kPwTile);
    if (g.N % 128 == 0)      // four 32-channel blocks per wave where the channels allow: half the re-reads of the input
      hipLaunchKernelGGL((dd_conv1x1_gemm_kernel<PREC, 4, RAGGED>), dim3(ptiles * (unsigned)(g.N / 128), (unsigned)B), dim3(kThreads), 0, st, in,
                         (const uint16_t*)wh, (const uint16_t*)wl, out, g.K, g.N, P);
    else
      hipLaunchKernelGGL((dd_conv1x1_gemm_kernel<PREC, 2, RAGGED>), dim3(ptiles * (unsigned)((g.N + 63) / 64), (unsigned)B), dim3(kThreads), 0, st,
                         in, (const uint16_t*)wh, (const uint16_t*)wl, out, g.K, g.N, P);
  } else if (op == kOpConv3 && dir == 0) {      // (the 3x3's two directions are one instantiation: the pack mode alone tells them apart)
    launch_igemm<PREC, RAGGED, kOpConv3, 0>(g, in, wh, wl, out, B, H, W, st);
  } else if (op == kOpConv3) {
    launch_igemm<PREC, RAGGED, kOpConv3, 1>(g, in, wh, wl, out, B, H, W, st);
  } else if (dir == 0) {
    launch_igemm<PREC, RAGGED, kOpDeconv2, 0>(g, in, wh, wl, out, B, H, W, st);
  } else {
    launch_igemm<PREC, RAGGED, kOpDeconv2, 1>(g, in, wh, wl, out, B, H, W, st);
  }
  return hipGetLastError();
}

template <int PREC, bool RAGGED>
hipError_t launch_wgrad_prec(int op, const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H, int W,
                             hipStream_t st) {
  const WgradSplit sp = wgrad_split(op, B, H, W);
  const int tiles_x = (W + 31) / 32, tiles_y = (H + wgrad_rows(op) - 1) / wgrad_rows(op);      // (the 1x1 has flat tiles: sp.tiles)
  float* part = reinterpret_cast<float*>(workspace);
  const dim3 grid((unsigned)(((Cin + 63) / 64) * ((Cout + 63) / 64)), (unsigned)sp.splits);
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
  const size_t total = (size_t)Cin * Cout * taps_of(op);
  hipLaunchKernelGGL(dd_conv_wgrad_reduce_kernel, dim3(blocks_for(total)), dim3(kThreads), 0, st, (const float*)part, grad_w, total, sp.splits);
  return hipGetLastError();
}

// f(precision, ragged) with the runtime operand mode and contract as the compile-time constants the kernels are instantiated with.  A shape of the
// block-64 contract runs the block-64 instantiations, whichever entry point it came through; only the others run the guarded ones.
template <class F>
hipError_t dispatch(int prec, int Cin, int Cout, F f) {
  const auto by_channels = [&](auto p) { return block64(Cin, Cout) ? f(p, std::false_type{}) : f(p, std::true_type{}); };
  if (prec == kPrecBf16) return by_channels(std::integral_constant<int, kPrecBf16>{});
  if (prec == kPrecF16) return by_channels(std::integral_constant<int, kPrecF16>{});
  return by_channels(std::integral_constant<int, kPrecF16x3>{});
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
                       int prec, hipStream_t st) {
  return dispatch(prec, Cin, Cout, [&](auto p, auto ragged) {
    return launch_conv_prec<decltype(p)::value, decltype(ragged)::value>(op, dir, in, w, out, workspace, B, Cin, Cout, H, W, st);
  });
}

hipError_t launch_wgrad(int op, const float* x, const float* grad_y, float* grad_w, void* workspace, int B, int Cin, int Cout, int H, int W,
                        int prec, hipStream_t st) {
  return dispatch(prec, Cin, Cout, [&](auto p, auto ragged) {
    return launch_wgrad_prec<decltype(p)::value, decltype(ragged)::value>(op, x, grad_y, grad_w, workspace, B, Cin, Cout, H, W, st);
  });
}

}  // namespace ddconv
