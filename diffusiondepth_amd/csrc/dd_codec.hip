// dd_codec.hip -- the latent depth codec's training convolutions as fp32 HIP kernels for gfx950 (include/ddepth_codec.h): Conv 1 -> 16 k3 s2 p1
// (ENC0), Conv 16 -> 16 k3 s1 p1 (ENC1), ConvTranspose2d 16 -> 16 k4 s2 p1 with bias (DEC0), Conv 16 -> 1 k3 s1 p1 with bias (DEC1); forward, data
// gradient and weight (+ bias) gradient; and the decoder's tail 1 / max(sigmoid(z), eps) - 1 forward and backward.  Tensors are contiguous fp32 NCHW
// as torch holds them, the weights are the raw parameters; fp32 operands, fp32 FMA.
//
// Structure:
//   dd_codec_pack_kernel     the raw weights, as torch lays them out -> wp[tap][cin][16 outputs] in the workspace, on EVERY call (the parameters change
//                            every optimiser step).  The data gradients are the forward kernels on the transposed (3x3: and flipped) weight map.
//   dd_codec_conv16_kernel   the directions with 16 outputs per pixel and wave-uniform taps (ENC0 / ENC1 forward; ENC1 / DEC0 / DEC1 data gradient).
//                            One work-item per output pixel of a FLAT plane, consecutive lanes consecutive pixels, the 16 outputs in registers as
//                            cout pairs on packed fp32 FMA; a (tap, cin) row of wp is wave-uniform: one 64-byte scalar load, as in the inference
//                            kernels enc1_kernel / dec_fused_kernel (dd_misc.hip).  The stride-2 reads of ENC0's forward and DEC0's data gradient
//                            touch every other pixel per instruction; the neighbouring tap takes the other half of the same cache lines.
//   dd_codec_dec0_fwd_kernel ConvTranspose k4 s2 p1 as a GATHER by output parity: a wave owns one output row (its two live kernel rows are
//                            wave-uniform), a lane the output pair (2 qx, 2 qx + 1), which between them use all four kernel columns: scalar weight
//                            rows again, consecutive input columns per load, consecutive 8-byte pairs per store.  No scatter, no atomics.
//   dd_codec_dec1_fwd_kernel 16 -> 1: one accumulator per pixel, 144 FMAs on scalar weight rows.
//   dd_codec_enc0_bwd_kernel 16 -> 1 gather by parity (k3 s2 p1: 1, 2 or 4 live taps per input pixel); the tap loop is wave-uniform, liveness per lane.
//   dd_codec_wgrad_kernel    D[p][q][tap] = sum over pixels of P[p][pixel] . Q[q][pixel * S - 1 + tap].  A workgroup owns every output and a
//                            contiguous range of pixel tiles (a SPLIT; a tile is 64 consecutive pixels of one row); both operands of a tile go
//                            through LDS, a work-item owns one (p, q) pair and its KS x KS taps and adds the tile's pixels in ascending order.  With
//                            fewer than 256 pairs (ENC0, DEC1) the work-items of a pair take the pixels s, s + NS, ... and their sums are added in
//                            ascending s through LDS.  The split's partial goes to the workspace; dd_codec_wgrad_reduce_kernel adds the splits in
//                            ascending order in fp64 and rounds once.  No floating-point atomics: two calls give the same bits.
//   dd_codec_tail_*_kernel   the elementwise tail, the operation sequence of dec1_kernel (dd_misc.hip).
//
// Plain HIP C++ and compiler builtins; every write to memory is a plain C++ store.  Only constructs the host emulation of the tests provides.
#include "dd_codec.h"

namespace ddcodec {

namespace {

typedef float f32x2_t __attribute__((ext_vector_type(2)));

enum { kGeoS1 = 0, kGeoS2 = 1 };      // input pixel of output (y, x) at tap (ky, kx): (y - 1 + ky, x - 1 + kx) or (2 y - 1 + ky, 2 x - 1 + kx)
enum { kMapEnc0F = 0, kMapEnc1F, kMapEnc1B, kMapDec0F, kMapDec0B, kMapDec1B };

// index into the raw torch weight of entry (tap, c = channel of `in`, o = channel of `out`) of the packed image wp[tap][c][o]
template <int WMAP>
__device__ __forceinline__ int weight_src(int tap, int c, int o) {
  if constexpr (WMAP == kMapEnc0F) return o * 9 + tap;                             // w[co = o][0][tap]
  else if constexpr (WMAP == kMapEnc1F) return (o * kC + c) * 9 + tap;             // w[co = o][ci = c][tap]
  else if constexpr (WMAP == kMapEnc1B) return (c * kC + o) * 9 + (8 - tap);       // w[co = c][ci = o][2 - ky][2 - kx]
  else if constexpr (WMAP == kMapDec0F) return (c * kC + o) * 16 + tap;            // w[ci = c][co = o][tap]
  else if constexpr (WMAP == kMapDec0B) return (o * kC + c) * 16 + tap;            // w[ci = o][co = c][tap]
  else return o * 9 + (8 - tap);                                                   // DEC1 data gradient: w[0][ci = o][2 - ky][2 - kx]
}

#ifdef DD_HOST_EMULATION
#define DD_CODEC_SCHED_FENCE() ((void)0)
#else
#define DD_CODEC_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#endif

// acc[0..15] += row[0..15] * v: `row` is wave-uniform, so its 16 floats are ONE 64-byte scalar load and the eight packed FMAs take SGPR pairs
__device__ __forceinline__ void fma_row(f32x2_t (&acc)[kC / 2], const float* __restrict__ row, float v) {
  const f32x2_t* r2 = reinterpret_cast<const f32x2_t*>(row);
  const f32x2_t a = (f32x2_t){v, v};
#pragma unroll
  for (int co = 0; co < kC / 2; ++co) acc[co] = __builtin_elementwise_fma(r2[co], a, acc[co]);
}

// ---- weights -> wp[tap][c][16 outputs] in the workspace, on EVERY call (the parameters change every optimiser step) ------------------------------------
template <int WMAP>
__global__ __launch_bounds__(kThreads) void dd_codec_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int taps, int cin) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= taps * cin * kC) return;
  wp[i] = w[weight_src<WMAP>(i / (kC * cin), (i / kC) % cin, i % kC)];
}

// ---- 16 outputs per pixel, wave-uniform taps --------------------------------------------------------------------------------------------------------
// in [B][CIN][Hin][Win], out [B][16][Hout][Wout], wp [KS * KS][CIN][16]; grid (ceil(Hout Wout / kThreads), B).  One work-item per output pixel of the
// FLAT plane: consecutive lanes, consecutive pixels.  A tap's CIN loads are in flight together; a tap outside the image contributes an exact zero.
template <int CIN, int KS, int GEO>
__global__ __launch_bounds__(kThreads) void dd_codec_conv16_kernel(const float* __restrict__ in, const float* __restrict__ wp,
                                                                   const float* __restrict__ bias, float* __restrict__ out, int Hin, int Win,
                                                                   int Hout, int Wout) {
  constexpr int T = KS * KS;
  const int b = blockIdx.y;
  const size_t plane_in = (size_t)Hin * Win;
  const long long plane_out = (long long)Hout * Wout;
  const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
  const bool live = p < plane_out;
  const long long pc = live ? p : plane_out - 1;      // (a dead lane computes the last pixel again and stores nothing: the weights stay wave-uniform)
  const int oy = (int)(pc / Wout), ox = (int)(pc - (long long)oy * Wout);
  const int y0 = (GEO == kGeoS2 ? 2 * oy : oy) - 1, x0 = (GEO == kGeoS2 ? 2 * ox : ox) - 1;
  const float* inb = in + (size_t)b * CIN * plane_in;
  f32x2_t acc[kC / 2];
#pragma unroll
  for (int c = 0; c < kC / 2; ++c) acc[c] = bias != nullptr ? (f32x2_t){bias[2 * c], bias[2 * c + 1]} : (f32x2_t){0.0f, 0.0f};

  if constexpr (CIN == 1) {      // every tap's load is issued before the first FMA
    float v[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int iy = y0 + t / KS, ix = x0 + t % KS;
      const bool inside = iy >= 0 && iy < Hin && ix >= 0 && ix < Win;
      v[t] = inside ? inb[(size_t)iy * Win + ix] : 0.0f;
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      fma_row(acc, wp + t * kC, v[t]);
      if (t % 3 == 2) DD_CODEC_SCHED_FENCE();      // three scalar rows in flight
    }
  } else {
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
      const int ky = t / KS, iy = y0 + ky, ix = x0 + (t - ky * KS);
      const bool inside = iy >= 0 && iy < Hin && ix >= 0 && ix < Win;
      const size_t off = inside ? (size_t)iy * Win + ix : 0;
      float v[CIN];
#pragma unroll
      for (int c = 0; c < CIN; ++c) v[c] = inside ? inb[(size_t)c * plane_in + off] : 0.0f;
      const float* rows = wp + t * (CIN * kC);      // wave-uniform
      // channel groups of four, every index a compile-time constant; the fence keeps a group's four scalar rows from being hoisted above the
      // previous group's FMAs (16 rows in flight = 256 SGPRs)
#pragma unroll
      for (int q = 0; q < CIN / 4; ++q) {
#pragma unroll
        for (int j = 0; j < 4; ++j) fma_row(acc, rows + (4 * q + j) * kC, v[4 * q + j]);
        DD_CODEC_SCHED_FENCE();
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int c = 0; c < kC; ++c) out[((size_t)b * kC + c) * (size_t)plane_out + (size_t)p] = acc[c >> 1][c & 1];
}

// ---- DEC0 forward: ConvTranspose2d k4 s2 p1 as a gather by output parity ---------------------------------------------------------------------------
// x [B][16][h][w] -> y [B][16][2h][2w], wp [ky * 4 + kx][ci][16 co].  Output row oy has the two live kernel rows ky = (oy + 1) % 2 + {0, 2} at
// input row (oy + 1 - ky) / 2; a wave owns ONE output row, so they are wave-uniform.  A lane owns the output PAIR ox = 2 qx, 2 qx + 1 -- both
// column parities: ox = 2 qx has kx = 1 (input column qx) and kx = 3 (qx - 1), ox = 2 qx + 1 has kx = 0 (qx + 1) and kx = 2 (qx) -- so all four
// kernel columns of a row are used by every lane and every weight row is a scalar operand.  Loads: consecutive lanes, consecutive input columns;
// stores: consecutive lanes, consecutive 8-byte pairs of one output row (two 4-byte stores each where y is not 8-byte aligned).
// grid (ceil(w / 64), ceil(2h / 4), B)
__global__ __launch_bounds__(kThreads) void dd_codec_dec0_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                                     const float* __restrict__ bias, float* __restrict__ y, int h, int w,
                                                                     int aligned8) {
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int b = blockIdx.z, oy = blockIdx.y * 4 + wave, qx = blockIdx.x * 64 + lane;
  if (oy >= 2 * h) return;      // (the whole wave; no barrier in this kernel)
  const size_t plane = (size_t)h * w;
  const float* xb = x + (size_t)b * kC * plane;
  const int pr = (oy + 1) & 1;
  const bool in_0 = qx < w, in_m = in_0 && qx >= 1, in_p = qx + 1 < w;      // (a lane behind the row loads nothing and stores nothing)
  f32x2_t acc0[kC / 2], acc1[kC / 2];
#pragma unroll
  for (int c = 0; c < kC / 2; ++c) acc0[c] = acc1[c] = bias != nullptr ? (f32x2_t){bias[2 * c], bias[2 * c + 1]} : (f32x2_t){0.0f, 0.0f};
#pragma unroll 1
  for (int a = 0; a < 2; ++a) {
    const int ky = pr + 2 * a, iy = (oy + 1 - ky) >> 1;      // oy + 1 - ky is even
    if (iy < 0 || iy >= h) continue;                         // wave-uniform: a kernel row outside the image contributes nothing
    const float* xr = xb + (size_t)iy * w + (in_0 ? qx : 0);
    const float* wk = wp + (size_t)(ky * 4) * (kC * kC);
#pragma unroll 1
    for (int c0 = 0; c0 < kC; c0 += 4) {
      float vm[4], v0[4], vp[4];      // twelve loads in flight
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* s = xr + (size_t)(c0 + j) * plane;
        vm[j] = in_m ? s[-1] : 0.0f;
        v0[j] = in_0 ? s[0] : 0.0f;
        vp[j] = in_p ? s[1] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* r = wk + (c0 + j) * kC;
        fma_row(acc1, r, vp[j]);                        // kx = 0
        fma_row(acc0, r + 1 * kC * kC, v0[j]);          // kx = 1
        fma_row(acc1, r + 2 * kC * kC, v0[j]);          // kx = 2
        fma_row(acc0, r + 3 * kC * kC, vm[j]);          // kx = 3
        DD_CODEC_SCHED_FENCE();
      }
    }
  }
  if (!in_0) return;
  float* yb = y + ((size_t)b * kC * 2 * h + oy) * (size_t)(2 * w) + 2 * (size_t)qx;
  const size_t plane_out = 4 * plane;
#pragma unroll
  for (int c = 0; c < kC; ++c) {
    float* d = yb + (size_t)c * plane_out;
    if (aligned8) {
      *reinterpret_cast<float2*>(d) = make_float2(acc0[c >> 1][c & 1], acc1[c >> 1][c & 1]);
    } else {
      d[0] = acc0[c >> 1][c & 1];
      d[1] = acc1[c >> 1][c & 1];
    }
  }
}

// ---- DEC1 forward: x [B][16][H][W] -> z [B][1][H][W], wp [tap][ci] ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void dd_codec_dec1_fwd_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                                     const float* __restrict__ bias, float* __restrict__ z, int H, int W) {
  const int b = blockIdx.y;
  const long long plane = (long long)H * W;
  const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= plane) return;
  const float* xb = x + (size_t)b * kC * (size_t)plane;
  const int oy = (int)(p / W), ox = (int)(p - (long long)oy * W);
  float acc = bias != nullptr ? bias[0] : 0.0f;
#pragma unroll 1
  for (int t = 0; t < 9; ++t) {
    const int ky = t / 3, kx = t - ky * 3, iy = oy - 1 + ky, ix = ox - 1 + kx;
    const bool inside = iy >= 0 && iy < H && ix >= 0 && ix < W;
    const size_t off = inside ? (size_t)iy * W + ix : 0;
    float v[kC];
#pragma unroll
    for (int c = 0; c < kC; ++c) v[c] = inside ? xb[(size_t)c * (size_t)plane + off] : 0.0f;
    const float* row = wp + t * kC;      // wave-uniform: one 64-byte scalar load
#pragma unroll
    for (int c = 0; c < kC; ++c) acc = fmaf(row[c], v[c], acc);
  }
  z[(size_t)b * (size_t)plane + (size_t)p] = acc;
}

// ---- ENC0 data gradient: grad_y [B][16][h][w] -> grad_x [B][1][H][W], gathered by parity, wp [tap][co] ---------------------------------------------
// grad_x(iy, ix) = sum over the taps with iy + 1 - ky = 2 oy, ix + 1 - kx = 2 ox inside the output (1, 2 or 4 of the 9), over co, of
// grad_y[co](oy, ox) . w[co][ky][kx].  The tap loop is wave-uniform (its weight row a scalar operand); whether a tap is live is the lane's business.
__global__ __launch_bounds__(kThreads) void dd_codec_enc0_bwd_kernel(const float* __restrict__ gy, const float* __restrict__ wp,
                                                                     float* __restrict__ gx, int H, int W, int h, int wl) {
  const int b = blockIdx.y;
  const long long plane = (long long)H * W;
  const long long p = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= plane) return;
  const size_t plane_y = (size_t)h * wl;
  const float* gyb = gy + (size_t)b * kC * plane_y;
  const int iy = (int)(p / W), ix = (int)(p - (long long)iy * W);
  float acc = 0.0f;
#pragma unroll 1
  for (int t = 0; t < 9; ++t) {
    const int ky = t / 3, kx = t - ky * 3, ty = iy + 1 - ky, tx = ix + 1 - kx;
    const bool live = ty >= 0 && tx >= 0 && ((ty | tx) & 1) == 0 && (ty >> 1) < h && (tx >> 1) < wl;
    const size_t off = live ? (size_t)(ty >> 1) * wl + (tx >> 1) : 0;
    float v[kC];
#pragma unroll
    for (int c = 0; c < kC; ++c) v[c] = live ? gyb[(size_t)c * plane_y + off] : 0.0f;
    const float* row = wp + t * kC;      // wave-uniform: one 64-byte scalar load
#pragma unroll
    for (int c = 0; c < kC; ++c) acc = fmaf(row[c], v[c], acc);
  }
  gx[(size_t)b * (size_t)plane + (size_t)p] = acc;
}

// ---- weight (and bias) gradient -------------------------------------------------------------------------------------------------------------------
// P [B][CP][Hp][Wp] is read at the pixel itself, Q [B][CQ][Hq][Wq] at (y * S - 1 + ky, x * S - 1 + kx):
//   ENC0 / ENC1 / DEC1: P = grad_y, Q = x -> grad_w[co][ci][ky][kx]          DEC0: P = x, Q = grad_y -> grad_w[ci][co][ky][kx]
// BIAS: 0 none; 1 sum of P (DEC1: grad_y is P); 2 sum of Q over the 2 x 2 output pixels of every P pixel (DEC0: grad_y is Q, S = 2)
// part [splits][stride]: CP * CQ * KS * KS weight partials, then the bias partials; grid (splits)
template <int CP, int CQ, int KS, int S, int BIAS>
__global__ __launch_bounds__(kThreads) void dd_codec_wgrad_kernel(const float* __restrict__ P, const float* __restrict__ Q, float* __restrict__ part,
                                                                  int Hp, int Wp, int Hq, int Wq, int tiles_x, long long tiles,
                                                                  int tiles_per_split, int stride) {
  constexpr int T = KS * KS, NPQ = CP * CQ, NS = kThreads / NPQ;
  constexpr int QW = (kWgTileW - 1) * S + KS, QWP = QW | 1;      // an odd row pitch
  static_assert(NPQ * NS == kThreads && NS >= 1, "every work-item owns one (p, q) pair");
  __shared__ float PL[CP][kWgTileW + 1];
  __shared__ float QL[CQ][KS][QWP];
  __shared__ float red[NS > 1 ? kThreads * (T + 1) : 1];

  const int tid = threadIdx.x, s = tid / NPQ, pq = tid - s * NPQ, p = pq / CQ, q = pq - p * CQ, split = blockIdx.x;
  const size_t plane_p = (size_t)Hp * Wp, plane_q = (size_t)Hq * Wq;
  float acc[T], bacc = 0.0f;
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = 0.0f;

  const long long t_begin = (long long)split * tiles_per_split;
  const long long t_end = t_begin + tiles_per_split < tiles ? t_begin + tiles_per_split : tiles;
  for (long long t = t_begin; t < t_end; ++t) {
    const int txi = (int)(t % tiles_x);
    const long long rest = t / tiles_x;
    const int y = (int)(rest % Hp), b = (int)(rest / Hp);
    const int x0 = txi * kWgTileW, npx = Wp - x0 < kWgTileW ? Wp - x0 : kWgTileW;
    const int qy0 = y * S - 1, qx0 = x0 * S - 1;
    __syncthreads();      // the previous tile's reads are over
    // consecutive work-items: consecutive pixels of one row of one plane; what lies outside the image is zero
    for (int i = tid; i < CP * kWgTileW; i += kThreads) {
      const int ch = i / kWgTileW, px = i - ch * kWgTileW;
      PL[ch][px] = px < npx ? P[((size_t)b * CP + ch) * plane_p + (size_t)y * Wp + x0 + px] : 0.0f;
    }
    for (int i = tid; i < CQ * KS * QW; i += kThreads) {
      const int ch = i / (KS * QW), rem = i - ch * (KS * QW), r = rem / QW, c = rem - r * QW;
      const int yy = qy0 + r, xx = qx0 + c;
      QL[ch][r][c] = (yy >= 0 && yy < Hq && xx >= 0 && xx < Wq) ? Q[((size_t)b * CQ + ch) * plane_q + (size_t)yy * Wq + xx] : 0.0f;
    }
    __syncthreads();
    for (int px = s; px < npx; px += NS) {      // only the tile's own pixels: a zero of the padding never meets a value
      const float g = PL[p][px];
#pragma unroll
      for (int ky = 0; ky < KS; ++ky)
#pragma unroll
        for (int kx = 0; kx < KS; ++kx) acc[ky * KS + kx] = fmaf(g, QL[q][ky][px * S + kx], acc[ky * KS + kx]);
      if constexpr (BIAS == 1) {
        if (q == 0) bacc += g;
      } else if constexpr (BIAS == 2) {
        if (p == 0) {
          bacc += QL[q][1][2 * px + 1];
          bacc += QL[q][1][2 * px + 2];
          bacc += QL[q][2][2 * px + 1];
          bacc += QL[q][2][2 * px + 2];
        }
      }
    }
  }

  if constexpr (NS > 1) {      // the NS pixel slices of a pair, added in ascending s
    float* mine = red + (size_t)tid * (T + 1);
#pragma unroll
    for (int t = 0; t < T; ++t) mine[t] = acc[t];
    mine[T] = bacc;
    __syncthreads();
    if (s != 0) return;
    for (int k = 1; k < NS; ++k) {
      const float* other = red + (size_t)(k * NPQ + pq) * (T + 1);
#pragma unroll
      for (int t = 0; t < T; ++t) acc[t] += other[t];
      bacc += other[T];
    }
  }
  float* dst = part + (size_t)split * stride;
#pragma unroll
  for (int t = 0; t < T; ++t) dst[pq * T + t] = acc[t];
  if constexpr (BIAS == 1) {
    if (q == 0) dst[NPQ * T + p] = bacc;
  } else if constexpr (BIAS == 2) {
    if (p == 0) dst[NPQ * T + q] = bacc;
  }
}

// grad[i] = fp32(part[0][i] + part[1][i] + ... in that order, in fp64); the first nw entries are grad_w, the rest grad_bias (skipped when null)
__global__ __launch_bounds__(kThreads) void dd_codec_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ grad_w,
                                                                         float* __restrict__ grad_bias, int nw, int stride, int splits) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= stride) return;
  double sum = 0.0;
#pragma unroll 8
  for (int k = 0; k < splits; ++k) sum += (double)part[(size_t)k * stride + i];      // (eight loads in flight; the additions stay in order)
  if (i < nw) grad_w[i] = (float)sum;
  else if (grad_bias != nullptr) grad_bias[i - nw] = (float)sum;
}

// ---- the decoder's tail -----------------------------------------------------------------------------------------------------------------------------
// depth = 1 / max(sigmoid(z), eps) - 1: the fp32 operation sequence of dec1_kernel (dd_misc.hip), so the training and the eval decoder agree.  A NaN
// passes through both comparisons.
__global__ __launch_bounds__(kThreads) void dd_codec_tail_fwd_kernel(const float* __restrict__ z, float* __restrict__ depth, long long n, float eps) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float sg = 1.f / (1.f + expf(-z[i]));
  depth[i] = 1.f / ((sg < eps) ? eps : sg) - 1.f;
}

// grad_z = -grad_depth . (1 - s) / s where s >= eps (torch's clamp(min): the gradient passes at equality), else 0.  With s = 1 / (1 + e), e = exp(-z),
// the factor (1 - s) / s IS e: it is taken from the exponential the gate's s is recomputed from, not from 1 - s (which cancels for z >> 0).
__global__ __launch_bounds__(kThreads) void dd_codec_tail_bwd_kernel(const float* __restrict__ z, const float* __restrict__ gd, float* __restrict__ gz,
                                                                     long long n, float eps) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float e = expf(-z[i]);
  const float sg = 1.f / (1.f + e);
  gz[i] = (sg < eps) ? 0.f : -gd[i] * e;      // (NaN < eps is false: a NaN in z gives NaN)
}

inline dim3 pixel_grid(long long plane, int B) { return dim3((unsigned)((plane + kThreads - 1) / kThreads), (unsigned)B); }

template <int WMAP>
void run_pack(const float* w, float* wp, int taps, int cin, hipStream_t st) {
  hipLaunchKernelGGL((dd_codec_pack_kernel<WMAP>), dim3((unsigned)((taps * cin * kC + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, w, wp, taps, cin);
}

template <int CP, int CQ, int KS, int S, int BIAS>
void run_wgrad(const WgradSplit& sp, const float* P, const float* Q, float* part, int Hp, int Wp, int Hq, int Wq, int stride, hipStream_t st) {
  hipLaunchKernelGGL((dd_codec_wgrad_kernel<CP, CQ, KS, S, BIAS>), dim3((unsigned)sp.splits), dim3(kThreads), 0, st, P, Q, part, Hp, Wp, Hq, Wq,
                     (Wp + kWgTileW - 1) / kWgTileW, (long long)sp.tiles, sp.tiles_per_split, stride);
}

// weight and bias gradient entries of an op
inline void grad_sizes(int op, int* nw, int* nb) {
  *nw = op == kOpEnc0 ? kC * 9 : op == kOpEnc1 ? kC * kC * 9 : op == kOpDec0 ? kC * kC * 16 : kC * 9;
  *nb = op == kOpDec0 ? kC : op == kOpDec1 ? 1 : 0;
}

}  // namespace

// ---- launchers ----------------------------------------------------------------------------------------------------------------------------------
WgradSplit wgrad_split(int op, int B, int H, int W) {
  int Hp = H, Wp = W;      // the unshifted operand: grad_y of ENC0 (the output), x of DEC0 (the input), either of the stride-1 ops
  if (op == kOpEnc0) out_size(op, H, W, &Hp, &Wp);
  WgradSplit s;
  s.tiles = (int64_t)B * Hp * ((Wp + kWgTileW - 1) / kWgTileW);
  int64_t per = (s.tiles + kMaxSplits - 1) / kMaxSplits;
  if (per < kSplitTiles) per = kSplitTiles;
  s.tiles_per_split = (int)per;
  s.splits = (int)((s.tiles + per - 1) / per);
  return s;
}

size_t workspace_bytes(int op, int B, int H, int W) {
  int nw, nb;
  grad_sizes(op, &nw, &nb);
  const size_t packed = (size_t)kPackedFloats * sizeof(float);      // forward / data gradient: the weights as wp[tap][c][16]
  const size_t partials = (size_t)wgrad_split(op, B, H, W).splits * (size_t)(nw + nb) * sizeof(float);
  const size_t need = packed > partials ? packed : partials;
  return (need + 255) / 256 * 256;
}

hipError_t launch_conv(int op, int dir, const float* in, const float* w, const float* bias, float* out, void* workspace, int B, int H, int W,
                       hipStream_t st) {
  int Ho, Wo;
  out_size(op, H, W, &Ho, &Wo);
  const dim3 block(kThreads);
  float* wp = reinterpret_cast<float*>(workspace);
  const float* wpc = wp;
  const float* none = nullptr;
  if (dir == 0) {
    const dim3 grid = pixel_grid((long long)Ho * Wo, B);
    if (op == kOpEnc0) {
      run_pack<kMapEnc0F>(w, wp, 9, 1, st);
      hipLaunchKernelGGL((dd_codec_conv16_kernel<1, 3, kGeoS2>), grid, block, 0, st, in, wpc, bias, out, H, W, Ho, Wo);
    } else if (op == kOpEnc1) {
      run_pack<kMapEnc1F>(w, wp, 9, kC, st);
      hipLaunchKernelGGL((dd_codec_conv16_kernel<kC, 3, kGeoS1>), grid, block, 0, st, in, wpc, bias, out, H, W, Ho, Wo);
    } else if (op == kOpDec0) {
      run_pack<kMapDec0F>(w, wp, 16, kC, st);
      const dim3 g2((unsigned)((W + 63) / 64), (unsigned)((Ho + 3) / 4), (unsigned)B);
      hipLaunchKernelGGL(dd_codec_dec0_fwd_kernel, g2, block, 0, st, in, wpc, bias, out, H, W, (int)(((uintptr_t)out & 7) == 0));
    } else {
      run_pack<kMapEnc0F>(w, wp, 9, 1, st);      // w[0][ci][tap] -> wp[tap][ci]: the index map of ENC0's forward
      hipLaunchKernelGGL(dd_codec_dec1_fwd_kernel, grid, block, 0, st, in, wpc, bias, out, H, W);
    }
  } else {      // in = grad_y (Ho x Wo), out = grad_x (H x W)
    const dim3 grid = pixel_grid((long long)H * W, B);
    if (op == kOpEnc0) {
      run_pack<kMapEnc0F>(w, wp, 9, 1, st);
      hipLaunchKernelGGL(dd_codec_enc0_bwd_kernel, grid, block, 0, st, in, wpc, out, H, W, Ho, Wo);
    } else if (op == kOpEnc1) {
      run_pack<kMapEnc1B>(w, wp, 9, kC, st);
      hipLaunchKernelGGL((dd_codec_conv16_kernel<kC, 3, kGeoS1>), grid, block, 0, st, in, wpc, none, out, Ho, Wo, H, W);
    } else if (op == kOpDec0) {
      run_pack<kMapDec0B>(w, wp, 16, kC, st);
      hipLaunchKernelGGL((dd_codec_conv16_kernel<kC, 4, kGeoS2>), grid, block, 0, st, in, wpc, none, out, Ho, Wo, H, W);
    } else {
      run_pack<kMapDec1B>(w, wp, 9, 1, st);
      hipLaunchKernelGGL((dd_codec_conv16_kernel<1, 3, kGeoS1>), grid, block, 0, st, in, wpc, none, out, Ho, Wo, H, W);
    }
  }
  return hipGetLastError();
}

hipError_t launch_wgrad(int op, const float* x, const float* grad_y, float* grad_w, float* grad_bias, void* workspace, int B, int H, int W,
                        hipStream_t st) {
  int Ho, Wo, nw, nb;
  out_size(op, H, W, &Ho, &Wo);
  grad_sizes(op, &nw, &nb);
  const WgradSplit sp = wgrad_split(op, B, H, W);
  const int stride = nw + nb;
  float* part = reinterpret_cast<float*>(workspace);
  if (op == kOpEnc0) run_wgrad<kC, 1, 3, 2, 0>(sp, grad_y, x, part, Ho, Wo, H, W, stride, st);
  else if (op == kOpEnc1) run_wgrad<kC, kC, 3, 1, 0>(sp, grad_y, x, part, Ho, Wo, H, W, stride, st);
  else if (op == kOpDec0) run_wgrad<kC, kC, 4, 2, 2>(sp, x, grad_y, part, H, W, Ho, Wo, stride, st);
  else run_wgrad<1, kC, 3, 1, 1>(sp, grad_y, x, part, Ho, Wo, H, W, stride, st);
  hipLaunchKernelGGL(dd_codec_wgrad_reduce_kernel, dim3((unsigned)((stride + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const float*)part,
                     grad_w, grad_bias, nw, stride, sp.splits);
  return hipGetLastError();
}

hipError_t launch_tail_forward(const float* z, float* depth, int64_t n, float eps, hipStream_t st) {
  hipLaunchKernelGGL(dd_codec_tail_fwd_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, z, depth, (long long)n, eps);
  return hipGetLastError();
}

hipError_t launch_tail_backward(const float* z, const float* grad_depth, float* grad_z, int64_t n, float eps, hipStream_t st) {
  hipLaunchKernelGGL(dd_codec_tail_bwd_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, z, grad_depth, grad_z,
                     (long long)n, eps);
  return hipGetLastError();
}

}  // namespace ddcodec
