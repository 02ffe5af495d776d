// dd_conv_kernels.h -- the GEMM kernels of csrc/dd_conv.hip, written ONCE and included there TWICE (and a third time, DD_CONV_BIAS 1, for the biased
// forward of include/ddepth_conv_strided.h alone, a fourth, DD_CONV_AFFINE 1, for the folded eval-mode forward of include/ddepth_conv_fused.h
// alone, and a fifth, DD_CONV_STATS 1, for the statistics-emitting training forward of include/ddepth_conv_stats.h alone: below): with DD_CONV_SCALED 0 it defines the kernels of include/ddepth_conv.h and ddepth_conv_strided.h
// (dd_conv_igemm_kernel, dd_conv_wgrad_kernel, dd_conv1x1_gemm_kernel, dd_conv1x1_wgrad_kernel, dd_conv_wgrad_reduce_kernel, dd_conv_s2_dgrad_kernel,
// dd_conv_bias_grad_kernel, dd_conv_bias_grad_reduce_kernel), with
// DD_CONV_SCALED 1 their twins *_scaled_kernel of include/ddepth_conv_scaled.h, which take the device pair scale = {s, 1 / s} as one more (last)
// argument, multiply every loaded value of grad_y by s before it is rounded to its 16-bit operand, and undo it with 1 / s where the result is stored:
//   dd_conv_igemm / dd_conv1x1_gemm   `in` is grad_y (the twins are launched for the data gradients only); the accumulators times 1 / s in the epilogue
//   dd_conv_wgrad                     grad_y is P for the 3x3 (KS == 3, either stride) and Q for the transpose convolution (KS == 2); the partials stay scaled
//   dd_conv1x1_wgrad                  grad_y is Pm; the partials stay scaled
//   dd_conv_wgrad_reduce              writes sum * 1 / s
//   dd_conv_s2_dgrad                  the 3x3 stride-2 data gradient: `gy` is grad_y; the accumulators times 1 / s in the epilogue
//   dd_conv_bias_grad                 the sum of the rounded grad_y * s, times 1 / s
// Both factors are powers of two, and the order of every accumulation is untouched.  The preprocessor and not a template argument makes the
// twins: a kernel's name and argument list are part of what a change may not touch (tools/code_object_diff.py); a template argument would
// rename every instantiation, and a shared __device__ body inlined into two kernels does not compile to the instruction stream the kernel had.
// In the unscaled pass every macro below expands to its argument or to nothing: that pass is the text the kernels always had.
#if DD_CONV_SCALED
#define DD_CONV_KERNEL(name) name##_scaled_kernel
#define DD_CONV_SCALE_PARAM , const float* __restrict__ scale      /* the address is the same for every lane: scalar loads */
#define DD_CONV_GY(is_grad_y, v) ((is_grad_y) ? (v) * scale[0] : (v))
#define DD_CONV_UNSCALED(v) ((v) * scale[1])
#define DD_CONV_EPILOGUE(v, n, o) (v)
#elif DD_CONV_BIAS
// a third pass (include/ddepth_conv_strided.h): dd_conv_igemm_bias_kernel alone, the implicit GEMM with one more (last) argument bias[N] or NULL,
// added in fp32 where the accumulator is stored.  Its own kernel for the reason the twins are: the argument list of dd_conv_igemm_kernel stays.
#define DD_CONV_KERNEL(name) name##_bias_kernel
#define DD_CONV_SCALE_PARAM , const float* __restrict__ bias
#define DD_CONV_GY(is_grad_y, v) (v)
#define DD_CONV_UNSCALED(v) (v)
#define DD_CONV_EPILOGUE(v, n, o) (bias ? (v) + bias[n] : (v))
#elif DD_CONV_AFFINE
// a fourth pass (include/ddepth_conv_fused.h): dd_conv_igemm_affine_kernel alone, the implicit GEMM with three more (last) arguments -- scale_shift[2][N]
// (an eval-mode BatchNorm folded by dd_bn_fold_kernel: row 0 the scale, row 1 the shift), addend (out's layout, or NULL) and relu.  Where the
// accumulator is stored, in fp32:  v = fmaf(acc, scale[n], shift[n]);  with an addend v += addend[o];  with relu v = v < 0 ? 0 : v -- a NaN is not
// below zero and stays one, as in torch (fmaxf(v, 0) would give 0).  One rounding for the fma, one for the add: two at most.  The expression sits
// behind the guards of the store, so a RAGGED instantiation reads scale_shift for rows n < N only and addend inside the Ht x Wt grid only.
#define DD_CONV_KERNEL(name) name##_affine_kernel
#define DD_CONV_SCALE_PARAM , const float* __restrict__ scale_shift, const float* __restrict__ addend, int relu
#define DD_CONV_GY(is_grad_y, v) (v)
#define DD_CONV_UNSCALED(v) (v)
#define DD_CONV_EPILOGUE(v, n, o) affine_tail(fmaf((v), scale_shift[n], scale_shift[N + (n)]), addend, (o), relu)
#elif DD_CONV_STATS
// a fifth pass (include/ddepth_conv_stats.h): dd_conv_igemm_stats_kernel alone, the implicit GEMM of the bias pass (bias[N] or NULL, the same add where
// the accumulator is stored) with one more argument, part[N][B][tiles][2] in fp64: per workgroup and output channel of its tile the sum of the STORED
// fp32 values of the tile's pixels inside the Ht x Wt grid and the sum of their squares -- what dd_bn_stats would read back from `out`.  The
// epilogue of this pass is its own text below (every lane reaches its barriers); the other passes keep theirs.
#define DD_CONV_KERNEL(name) name##_stats_kernel
#define DD_CONV_SCALE_PARAM , const float* __restrict__ bias, double* __restrict__ part
#define DD_CONV_GY(is_grad_y, v) (v)
#define DD_CONV_UNSCALED(v) (v)
#define DD_CONV_EPILOGUE(v, n, o) (bias ? (v) + bias[n] : (v))
#else
#define DD_CONV_KERNEL(name) name##_kernel
#define DD_CONV_SCALE_PARAM
#define DD_CONV_GY(is_grad_y, v) (v)
#define DD_CONV_UNSCALED(v) (v)
#define DD_CONV_EPILOGUE(v, n, o) (v)
#endif

// ---- forward and data gradient --------------------------------------------------------------------------------------------------------------------
// in [B][K][Hin][Win], wp [KS * KS][N][K]; grid (tiles, N / 64, B).  The tile grid is Ht x Wt pixels:
//   !SCATTER: out [B][N][Ht][Wt], pixel (y, x) of the tile grid reads input pixels (y * S - PAD + ky, x * S - PAD + kx)
//   SCATTER:  out [B][N / 4][2 Ht][2 Wt], GEMM column n = (dy * 2 + dx) * (N / 4) + co goes to pixel (2y + dy, 2x + dx) of plane co
// RAGGED (K, N multiples of 8, not of the tiles): the weight image is the padded one of the pack kernel, channels >= K are filled as zeros, rows
// >= N are not stored, and grid y is ceil(N / 64).  The K chunks and their order are those of the block-64 instantiation.
template <int PREC, int KS, int S, int PAD, int KC, bool SCATTER, bool RAGGED>
__global__ __launch_bounds__(kThreads) void DD_CONV_KERNEL(dd_conv_igemm)(const float* __restrict__ in, const uint16_t* __restrict__ wh,
                                                                 const uint16_t* __restrict__ wl, float* __restrict__ out, int K, int N,
                                                                 int Hin, int Win, int Ht, int Wt, int tiles_x DD_CONV_SCALE_PARAM) {
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
        to_operand<PREC>(DD_CONV_GY(true, v[j]), hi, lo);
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
#if DD_CONV_STATS
  // Store as the bias pass stores, and sum what is stored.  The patch is dead behind the main loop: the tile's fp32 values are staged there, CH
  // output channels at a time (as many of 64 / 32 / 16 as the patch of this instantiation holds), a channel a row of 128 pixels (pixel p at float
  // p + p / 16: the strips below start in different banks); a pixel outside the grid is staged as +0.0 by a SELECT -- its accumulator holds real
  // neighbour sums.  Then 256 / CH threads per channel add one strip of 128 / (256 / CH) consecutive pixels each, in pixel order, in fp64 (the
  // square of a widened fp32 is exact), and an xor tree over those neighbouring lanes adds the strips: one fixed order, no atomics.  Every lane
  // reaches every barrier and shuffle; a row n >= N of a RAGGED instantiation reads no bias and writes no partial.
  static_assert(!SCATTER, "the stats pass is the plain 3x3 forward");
  constexpr int kRow = kTileH * kTileW + kTileH * kTileW / 16;      // floats per staged channel
  constexpr int kPatchBytes = (int)sizeof(uint16_t) * NL * PP * PS;
  constexpr int CH = kPatchBytes >= 64 * kRow * 4 ? 64 : kPatchBytes >= 32 * kRow * 4 ? 32 : 16;
  static_assert(kPatchBytes >= CH * kRow * 4, "the patch holds one staging pass");
  constexpr int TPC = kThreads / CH, SL = kTileH * kTileW / TPC;      // threads per channel, pixels per strip
  float* stage = reinterpret_cast<float*>(&patch[0][0]);
  const bool inside = y < Ht && x < Wt;
  const int pix = wave * kTileW + l32;
#pragma unroll
  for (int p = 0; p < kTileN / CH; ++p) {
    __syncthreads();      // the main loop's reads of the patch (the previous pass's reads of the stage) are over
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if ((nb * 32 + 8 * (r / 4)) / CH != p) continue;      // (known where the loops are unrolled)
        const int cl = nb * 32 + 8 * (r / 4) + 4 * half + (r % 4), n = n0 + cl;
        float v = acc[nb][r];
        if (!RAGGED || n < N) {
          v = DD_CONV_EPILOGUE(DD_CONV_UNSCALED(v), n, 0);
          if (inside) out[(((size_t)b * N + n) * Ht + y) * (size_t)Wt + x] = v;
        }
        stage[(cl - p * CH) * kRow + pix + (pix >> 4)] = inside ? v : 0.0f;
      }
    }
    __syncthreads();
    const int c = tid / TPC, s = tid % TPC;
    const float* strip = stage + c * kRow + s * SL + (s * SL >> 4);
    double sa = 0.0, sb = 0.0;
#pragma unroll
    for (int i = 0; i < SL; ++i) {
      const double d = (double)strip[i + (i >> 4)];
      sa += d;
      sb += d * d;
    }
#pragma unroll
    for (int d = 1; d < TPC; d <<= 1) {
      sa += __shfl_xor(sa, d);
      sb += __shfl_xor(sb, d);
    }
    const int n = n0 + p * CH + c;
    if (s == 0 && (!RAGGED || n < N)) {
      double* dst = part + (((size_t)n * gridDim.z + b) * gridDim.x + blockIdx.x) * 2;
      dst[0] = sa;
      dst[1] = sb;
    }
  }
#else
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
        // (the index is said twice: every pass but the affine one drops the macro's last argument, and is then the text it always was)
        out[(((size_t)b * N + n) * Ht + y) * (size_t)Wt + x] =
            DD_CONV_EPILOGUE(DD_CONV_UNSCALED(acc[nb][r]), n, (((size_t)b * N + n) * Ht + y) * (size_t)Wt + x);
      }
    }
  }
#endif      // DD_CONV_STATS
}

#if !DD_CONV_BIAS && !DD_CONV_AFFINE && !DD_CONV_STATS      // (the bias, the affine and the stats pass: the implicit GEMM alone)
// ---- weight gradient --------------------------------------------------------------------------------------------------------------------------------
// P [B][Cp][Hp][Wp] is read at the pixel itself, Q [B][Cq][Hq][Wq] at (y * S - PAD + ky, x * S - PAD + kx):
//   3x3:        P = grad_y, Q = x       -> grad_w[co][ci][ky][kx]          transpose convolution:  P = x, Q = grad_y -> grad_w[ci][co][dy][dx]
// part [splits][Cp][Cq][KS * KS]; grid ((Cp / 64) * (Cq / 64), splits).  A pixel tile is RH rows of 32 pixels.
// RAGGED: grid x is ceil(Cp / 64) * ceil(Cq / 64); channel rows >= Cp / Cq are filled as zeros and not stored (part keeps the real counts).
template <int PREC, int KS, int S, int PAD, int RH, bool RAGGED>
__global__ __launch_bounds__(kThreads) void DD_CONV_KERNEL(dd_conv_wgrad)(const float* __restrict__ P, const float* __restrict__ Q, float* __restrict__ part,
                                                                 int Cp, int Cq, int Hp, int Wp, int Hq, int Wq, int tiles_x, int tiles_y,
                                                                 long long tiles, int tiles_per_split DD_CONV_SCALE_PARAM) {
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
        to_operand<PREC>(DD_CONV_GY(KS != 2, v[j]), hi, lo);      // (P is grad_y for the 3x3, stride 1 or 2, ...
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
        to_operand<PREC>(DD_CONV_GY(KS == 2, v[j]), hi, lo);      // ... and Q for the transpose convolution)
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
__global__ __launch_bounds__(kThreads) void DD_CONV_KERNEL(dd_conv1x1_gemm)(const float* __restrict__ in, const uint16_t* __restrict__ wh,
                                                                   const uint16_t* __restrict__ wl, float* __restrict__ out, int K, int N, int P DD_CONV_SCALE_PARAM) {
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
        to_operand<PREC>(DD_CONV_GY(true, v[s][e]), hi, lo);
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
      dst[(size_t)row * P] = DD_CONV_UNSCALED(acc[nb][r]);
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
__global__ __launch_bounds__(kThreads) void DD_CONV_KERNEL(dd_conv1x1_wgrad)(const float* __restrict__ Pm, const float* __restrict__ Q, float* __restrict__ part,
                                                                    int Cp, int Cq, int P, int tiles_per_plane, long long tiles, int tiles_per_split DD_CONV_SCALE_PARAM) {
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
        to_operand<PREC>(DD_CONV_GY(row < 64, v[j][0]), h0, l0);      // (rows 0..63 are grad_y's; the same choice for a whole wave)
        to_operand<PREC>(DD_CONV_GY(row < 64, v[j][1]), h1, l1);
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

// grad_w[i] = part[0][i] + part[1][i] + ... in that order (the scaled pass: times 1 / s, the partials being those of the scaled grad_y)
__global__ __launch_bounds__(kThreads) void DD_CONV_KERNEL(dd_conv_wgrad_reduce)(const float* __restrict__ part, float* __restrict__ grad_w, size_t total,
                                                                        int splits DD_CONV_SCALE_PARAM) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  float s = part[i];
  for (int k = 1; k < splits; ++k) s += part[(size_t)k * total + i];
  grad_w[i] = DD_CONV_UNSCALED(s);
}

// ---- 3x3 stride 2 pad 1: data gradient (include/ddepth_conv_strided.h) --------------------------------------------------------------------------------
// grad_x[ci][iy][ix] = sum over co, ky, kx of grad_y[co][(iy + 1 - ky) / 2][(ix + 1 - kx) / 2] . w[co][ci][ky][kx] where both quotients are whole and
// inside the Ho x Wo grid.  Input pixel (2y + dy, 2x + dx) of the half-resolution grid (y, x) takes, per axis, the centre tap from grad_y row y when
// dy = 0, and taps 2 and 0 from rows y and y + 1 when dy = 1: tap (ky, kx) belongs to the parity class dy = (ky != 1), dx = (kx != 1) and reads
// grad_y at (y + (ky == 0), x + (kx == 0)).  One class has 1 tap, two have 2, one has 4 -- nine tap GEMMs per 2 x 2 input pixels, no product with an
// inserted zero.  A workgroup owns a 4 x 32 tile of the half-resolution grid, 64 input channels and all four classes (eight accumulators); the
// patch is (4 + 1) x (32 + 1) pixels of grad_y, KC output channels at a time, zero at row Ho / column Wo (the absent tap of an even H / W) and for
// channels >= K.  gy [B][K][Ho][Wo], wp [9][N][K] with wp[ky * 3 + kx][ci][co] = w[co][ci][ky][kx] (pack mode kPackConvS2Bwd), out [B][N][H][W];
// grid (tiles of the ceil(H / 2) x ceil(W / 2) grid, ceil(N / 64), B).  Pixels 2y + dy >= H or 2x + dx >= W are not stored; every other one is.
template <int PREC, int KC, bool RAGGED>
__global__ __launch_bounds__(kThreads) void DD_CONV_KERNEL(dd_conv_s2_dgrad)(const float* __restrict__ gy, const uint16_t* __restrict__ wh,
                                                                    const uint16_t* __restrict__ wl, float* __restrict__ out, int K, int N,
                                                                    int H, int W, int Ho, int Wo, int tiles_x DD_CONV_SCALE_PARAM) {
  constexpr int PH = kTileH + 1, PW = kTileW + 1, PP = PH * PW;
  constexpr int PS = KC + 8;      // halfs per patch pixel: a multiple of 8, so every 16-byte read is aligned
  constexpr int NL = PREC == kPrecF16x3 ? 2 : 1;
  __shared__ uint16_t patch[NL][PP * PS] __attribute__((aligned(16)));

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l32 = lane & 31;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x, n0 = blockIdx.y * kTileN, b = blockIdx.z;
  const int oy0 = ty * kTileH, ox0 = tx * kTileW;
  const size_t plane = (size_t)Ho * Wo;
  const float* gyb = gy + (size_t)b * K * plane;
  const int Kp = RAGGED ? padded(K, KC) : K, Np = RAGGED ? padded(N, kTileN) : N;      // the weight image's row length and rows per tap

  f32x16_t acc[4][2];      // [dy * 2 + dx][32-channel block]
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc[c][0][i] = 0.0f; acc[c][1][i] = 0.0f; }

  for (int kc = 0; kc < K; kc += KC) {
    __syncthreads();      // the previous chunk's reads are over
    for (int base = tid; base < KC * PP; base += kThreads * kFillBatch) {
      float v[kFillBatch];
#pragma unroll
      for (int j = 0; j < kFillBatch; ++j) {
        const int idx = base + j * kThreads, ch = idx / PP, rem = idx - ch * PP, pr = rem / PW, pc = rem - pr * PW;
        const int oy = oy0 + pr, ox = ox0 + pc;
        v[j] = 0.0f;
        if (idx < KC * PP && (!RAGGED || kc + ch < K) && oy < Ho && ox < Wo) v[j] = gyb[(size_t)(kc + ch) * plane + (size_t)oy * Wo + ox];
      }
#pragma unroll
      for (int j = 0; j < kFillBatch; ++j) {
        const int idx = base + j * kThreads, ch = idx / PP, rem = idx - ch * PP;
        if (idx >= KC * PP) break;
        uint16_t hi, lo;
        to_operand<PREC>(DD_CONV_GY(true, v[j]), hi, lo);
        patch[0][rem * PS + ch] = hi;
        if constexpr (PREC == kPrecF16x3) patch[NL - 1][rem * PS + ch] = lo;
      }
    }
    __syncthreads();
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int cls = (ky != 1 ? 2 : 0) + (kx != 1 ? 1 : 0);
        const int pp = ((wave + (ky == 0 ? 1 : 0)) * PW + (l32 + (kx == 0 ? 1 : 0))) * PS + 8 * half;
        const size_t wrow = ((size_t)(ky * 3 + kx) * Np + n0 + l32) * Kp + kc + 8 * half;
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
            acc[cls][nb] = mma_pair<PREC>(ah, al, bh, bl, acc[cls][nb]);
          }
        }
      }
    }
  }

  // accumulator entry r of lane l: column (half-resolution pixel) l % 32, row (input channel) 8 * (r / 4) + 4 * (l / 32) + r % 4
  const int y = oy0 + wave, x = ox0 + l32;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int iy = 2 * y + (c >> 1), ix = 2 * x + (c & 1);
    if (iy >= H || ix >= W) continue;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = n0 + nb * 32 + 8 * (r / 4) + 4 * half + (r % 4);
        if constexpr (RAGGED) {
          if (n >= N) continue;
        }
        out[(((size_t)b * N + n) * H + iy) * (size_t)W + ix] = DD_CONV_UNSCALED(acc[c][nb][r]);
      }
    }
  }
}

// ---- bias gradient --------------------------------------------------------------------------------------------------------------------------------------
// grad_bias[co] = sum over b, y, x of grad_y as the weight gradient sees it -- every element rounded to the operand (hi, plus lo in the split mode; the
// scaled pass: of grad_y * s, the sum times 1 / s) -- so it is the weight gradient of an all-ones input plane.  Two launches, fp64 throughout: workgroup
// (co, c) adds chunk c of every image's plane -- thread t the elements t, t + 256, ... of the chunk, image after image, then a tree over the 256 sums in
// LDS -- into part[co][c]; one thread per channel then adds its `chunks` partials in order.  The chunking depends on the shape alone
// (bias_grad_chunks): fixed order, no atomics, the same bits on every run.
template <int PREC>
__global__ __launch_bounds__(kThreads) void DD_CONV_KERNEL(dd_conv_bias_grad)(const float* __restrict__ gy, double* __restrict__ part, int B, int C,
                                                                     long long plane, long long per_chunk DD_CONV_SCALE_PARAM) {
  __shared__ double sums[kThreads];
  const int co = blockIdx.x, tid = threadIdx.x;
  const long long begin = (long long)blockIdx.y * per_chunk, end = begin + per_chunk < plane ? begin + per_chunk : plane;
  double s = 0.0;
  for (int b = 0; b < B; ++b) {
    const float* g = gy + ((size_t)b * C + co) * (size_t)plane;
    for (long long i = begin + tid; i < end; i += kThreads) {
      uint16_t hi, lo;
      to_operand<PREC>(DD_CONV_GY(true, g[i]), hi, lo);
      if constexpr (PREC == kPrecBf16) {
        s += (double)__builtin_bit_cast(float, (uint32_t)hi << 16);
      } else {
        s += (double)(float)__builtin_bit_cast(_Float16, hi);
        if constexpr (PREC == kPrecF16x3) s += (double)(float)__builtin_bit_cast(_Float16, lo);
      }
    }
  }
  sums[tid] = s;
  __syncthreads();
  for (int d = kThreads / 2; d >= 1; d >>= 1) {
    if (tid < d) sums[tid] += sums[tid + d];
    __syncthreads();
  }
  if (tid == 0) part[(size_t)co * gridDim.y + blockIdx.y] = sums[0];
}

__global__ __launch_bounds__(kThreads) void DD_CONV_KERNEL(dd_conv_bias_grad_reduce)(const double* __restrict__ part, float* __restrict__ grad_bias, int C,
                                                                            int chunks DD_CONV_SCALE_PARAM) {
  const int co = blockIdx.x * kThreads + threadIdx.x;
  if (co >= C) return;
  double s = part[(size_t)co * chunks];
  for (int k = 1; k < chunks; ++k) s += part[(size_t)co * chunks + k];
  grad_bias[co] = DD_CONV_UNSCALED((float)s);
}
#endif      // !DD_CONV_BIAS && !DD_CONV_AFFINE && !DD_CONV_STATS

#undef DD_CONV_KERNEL
#undef DD_CONV_SCALE_PARAM
#undef DD_CONV_GY
#undef DD_CONV_UNSCALED
#undef DD_CONV_EPILOGUE
