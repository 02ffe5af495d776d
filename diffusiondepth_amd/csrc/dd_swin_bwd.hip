// dd_swin_bwd.hip -- the backward of the shifted-window attention (include/train/ddepth_swin_backward.h), window 7, head dimension 32.
//
// One wave per workgroup; a workgroup owns one (slice of windows, head) and walks its windows one after the other.  Nothing is saved by the
// forward: per task = (image, window, head) the scores, the row maximum and the row sum are computed again, as dd_swin.hip computes them.
//
//   pass A, transposed (the forward's layout: key in the register index, query in lane % 32; per query block ib)
//     S^T  = K . (scale Q)^T        dP^T = V . dO^T            both operands are the straight 32-byte global loads of the rows
//     P    = softmax(S + bias + mask)       D_i = sum_j P_ij dP_ij: in-lane plus one exchange       dS = P (dP - D)
//     dBias += dS in registers (the wave keeps its head over its slice)
//     dQ   = scale (dS . K)         A = dS as the registers are, B = K from a [key][d] fp32 image in the LDS: the forward's P . V
//     the row maximum, 1 / sum and D of every query go to a 64-entry LDS table
//   pass B, un-transposed (query in the register index, key in lane % 32; per key block jb)
//     S = (scale Q) . K^T  and  dP = dO . V^T  again, with the operand registers of pass A swapped (A and B hold the same elements per lane)
//     P and dS from the table's maximum, 1 / sum and D: dK and dV contract over the query, which now sits in the registers
//     dV   = P^T . dO               dK = dS^T . (scale Q)      B = dO / scale Q from [query][d] fp32 images in the LDS
// Every result row is 128 contiguous bytes per half-wave, stored at the token the slot was read from; a padded slot's rows are summed into
// three per-lane accumulators instead.  At the end of its slice the wave writes its partial of dBias ([key][query]: lanes run along the
// query) and of dPad to the workspace; reduce_partials_kernel sums the slices in ascending order.  No atomics.
// The f16 mode multiplies grad_out by s before it is rounded and every result by 1 / s at its store (both powers of two).
// The workgroup barriers order the wave's own LDS writes and reads.
#include "dd_swin_bwd.h"

#include "dd_swin_dev.h"

namespace ddswin {
namespace {

struct alignas(16) BwdLds {
  float x[kSlots * kVStride];      // pass A: the K image [key][d]; pass B: the scale Q image [query][d]
  float g[kSlots * kVStride];      // the dO image [query][d]
  float bias[kTok * kBStride + 8];
  float stat[3][kSlots];           // per query: row maximum, 1 / row sum, D
  int tok[kSlots];                 // token index of the slot, -1: a padded position, -2: a slot >= 49
  int lab[kSlots];
};

// rows[blk][8 kk + e]: d = 16 kk + 8 half + e of slot 32 blk + lane % 32 -- the A (row = slot) and the B (column = slot) operand of an MFMA alike.
// src[blk]: the slot's 32 floats, or nullptr for zeros.
__device__ __forceinline__ void load_rows(float (&rows)[2][16], const float* const (&src)[2], int half, float mul) {
#pragma unroll
  for (int blk = 0; blk < 2; ++blk)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (src[blk]) v = load4(src[blk] + 16 * (c / 2) + 8 * half + 4 * (c % 2));
      rows[blk][4 * c + 0] = v.x * mul;
      rows[blk][4 * c + 1] = v.y * mul;
      rows[blk][4 * c + 2] = v.z * mul;
      rows[blk][4 * c + 3] = v.w * mul;
    }
}

__device__ __forceinline__ void store_image(float* img, const float (&rows)[2][16], int l32, int half) {
#pragma unroll
  for (int blk = 0; blk < 2; ++blk)
#pragma unroll
    for (int c = 0; c < 4; ++c)
      *reinterpret_cast<float4*>(&img[(32 * blk + l32) * kVStride + 16 * (c / 2) + 8 * half + 4 * (c % 2)]) =
          make_float4(rows[blk][4 * c], rows[blk][4 * c + 1], rows[blk][4 * c + 2], rows[blk][4 * c + 3]);
}

// row of a result or score register r of block blk: 32 blk + 8 (r / 4) + 4 half + r % 4
__device__ __forceinline__ constexpr int reg_row(int blk, int r, int half) { return 32 * blk + 8 * (r / 4) + 4 * half + r % 4; }

template <int MODE> struct Packed {      // the four row sets as MFMA operands; fp32 keeps the rows
  typedef typename Operand<MODE>::T T;
  T q[2][2], k[2][2], v[2][2], g[2][2];      // [slot block][kk]
};
template <> struct Packed<0> {};

template <int MODE>
__device__ __forceinline__ void pack_rows(typename Operand<MODE>::T (&dst)[2][2], const float (&rows)[2][16]) {
#pragma unroll
  for (int blk = 0; blk < 2; ++blk)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      f32x8_t x;
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = rows[blk][8 * kk + e];
      dst[blk][kk] = Operand<MODE>::pack(x);
    }
}

// the B operand of k-step ks from a [row][d] image: element e <-> row 32 (ks / 2) + 8 (2 (ks % 2) + e / 4) + 4 half + e % 4, column d = lane % 32
template <int MODE>
__device__ __forceinline__ typename Operand<MODE>::T image_operand(const float* img, int ks, int l32, int half) {
  f32x8_t x;
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = img[(32 * (ks / 2) + 8 * (2 * (ks % 2) + e / 4) + 4 * half + e % 4) * kVStride + l32];
  return Operand<MODE>::pack(x);
}

// acc = A . B over the 64 rows of the image, A = the registers a[blk][r] as they are (zeros where not live)
template <int MODE>
__device__ __forceinline__ f32x16_t contract(const float (&a)[2][16], const float* img, const typename Operand<MODE == 0 ? 1 : MODE>::T (&b)[4],
                                             int l32, int half) {
  f32x16_t o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
  if constexpr (MODE == 0) {
#pragma unroll
    for (int blk = 0; blk < 2; ++blk)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (!live(blk, r)) continue;      // (a is 0 there)
        o = __builtin_amdgcn_mfma_f32_32x32x2f32(a[blk][r], img[reg_row(blk, r, half) * kVStride + l32], o, 0, 0, 0);
      }
  } else {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      f32x8_t ax;
#pragma unroll
      for (int e = 0; e < 8; ++e) ax[e] = a[ks / 2][8 * (ks % 2) + e];
      o = Operand<MODE>::mma(Operand<MODE>::pack(ax), b[ks], o);
    }
  }
  return o;
}

template <int MODE>
__global__ __launch_bounds__(64) void window_attention_backward_kernel(const float* __restrict__ qkv, const float* __restrict__ qkv_pad,
                                                                       const float* __restrict__ rel_bias, const float* __restrict__ grad_out,
                                                                       float* __restrict__ grad_qkv, float* __restrict__ ws_bias,
                                                                       float* __restrict__ ws_pad, const float* __restrict__ scale, Frame f,
                                                                       int heads, int nwin, int per_slice) {
  typedef Operand<MODE == 0 ? 1 : MODE> Op;
  __shared__ BwdLds L;
  const int lane = threadIdx.x & 63, l32 = lane & 31, half = lane >> 5;
  const int head = blockIdx.x % heads, slice = blockIdx.x / heads;
  const int C = heads * kHeadDim;
  const size_t hoff = (size_t)head * kHeadDim;
  float gs = 1.0f, gi = 1.0f;      // grad_out * gs on the way in, every result * gi on the way out
  if constexpr (MODE == 2) {
    if (scale) {
      gs = scale[0];
      gi = scale[1];
    }
  }

  {
    const float* bsrc = rel_bias + (size_t)head * kTok * kTok;
    for (int idx = lane; idx < kTok * kTok; idx += 64) L.bias[(idx / kTok) * kBStride + idx % kTok] = bsrc[idx];
  }
  float accb[2][2][16];      // [ib][jb][r]: dBias of query 32 ib + lane % 32, key reg_row(jb, r, half), over the slice
#pragma unroll
  for (int ib = 0; ib < 2; ++ib)
#pragma unroll
    for (int jb = 0; jb < 2; ++jb)
#pragma unroll
      for (int r = 0; r < 16; ++r) accb[ib][jb][r] = 0.f;
  float accp[3] = {0.f, 0.f, 0.f};      // the q, k, v rows of the padded slots, d = lane % 32, this half-wave's rows

  const int w0 = slice * per_slice, w1 = min(nwin, w0 + per_slice);
  for (int win = w0; win < w1; ++win) {
    const int wx = win % f.nwx, wy = (win / f.nwx) % f.nwy, b = win / (f.nwx * f.nwy);
    // without a shift, and in every window above the last row and left of the last column of windows, all labels are equal: no mask term
    const bool masked = f.shift > 0 && (wy == f.nwy - 1 || wx == f.nwx - 1);
    {
      int label = 0;
      const int t = lane < kTok ? slot_token(f, b, wy, wx, lane, label) : -2;
      L.tok[lane] = t;
      L.lab[lane] = label;
    }
    __syncthreads();

    // ---- the rows of the task, in operand layout ---------------------------------------------------------------------------------------------
    float qf[2][16], kf[2][16], vf[2][16], gf[2][16];
    {
      const float *sq[2], *sk[2], *sv[2], *sg[2];
#pragma unroll
      for (int blk = 0; blk < 2; ++blk) {
        const int t = L.tok[32 * blk + l32];
        const float* row = t >= 0 ? qkv + (size_t)t * 3 * C + hoff : (t == -1 && qkv_pad ? qkv_pad + hoff : nullptr);
        sq[blk] = row;
        sk[blk] = row ? row + C : nullptr;
        sv[blk] = row ? row + 2 * C : nullptr;
        sg[blk] = t >= 0 ? grad_out + (size_t)t * C + hoff : nullptr;
      }
      load_rows(qf, sq, half, kScale);
      load_rows(kf, sk, half, 1.0f);
      load_rows(vf, sv, half, 1.0f);
      load_rows(gf, sg, half, gs);
    }
    store_image(L.x, kf, l32, half);
    store_image(L.g, gf, l32, half);
    [[maybe_unused]] Packed<MODE> pk;
    if constexpr (MODE != 0) {
      pack_rows<MODE>(pk.q, qf);
      pack_rows<MODE>(pk.k, kf);
      pack_rows<MODE>(pk.v, vf);
      pack_rows<MODE>(pk.g, gf);
    }
    __syncthreads();

    [[maybe_unused]] typename Op::T imgx[4], imgg[4];
    if constexpr (MODE != 0) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) imgx[ks] = image_operand<MODE>(L.x, ks, l32, half);
    }

    // ---- pass A --------------------------------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int ib = 0; ib < 2; ++ib) {
      f32x16_t sc[2], dp[2];      // [jb]
#pragma unroll
      for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sc[jb][r] = 0.f;
          dp[jb][r] = 0.f;
        }
      if constexpr (MODE == 0) {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
          for (int jb = 0; jb < 2; ++jb) {
            sc[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[jb][kk], qf[ib][kk], sc[jb], 0, 0, 0);
            dp[jb] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[jb][kk], gf[ib][kk], dp[jb], 0, 0, 0);
          }
      } else {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int jb = 0; jb < 2; ++jb) {
            sc[jb] = Op::mma(pk.k[jb][kk], pk.q[ib][kk], sc[jb]);
            dp[jb] = Op::mma(pk.v[jb][kk], pk.g[ib][kk], dp[jb]);
          }
      }

      // the forward's softmax: + bias, + mask, - max, exp, / sum.  Registers that are not live() hold keys >= 49 only.
      const int i = 32 * ib + l32;
      const bool qi = i < kTok;
      const int li = L.lab[i];
      float p[2][16];
      float m = -__builtin_inff();
#pragma unroll
      for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          if (!live(jb, 4 * g)) continue;
          const int j0 = 32 * jb + 8 * g + 4 * half;
          float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
          if (qi) b4 = *reinterpret_cast<const float4*>(&L.bias[i * kBStride + j0]);      // (the row's keys j0 ..+ 4; beyond key 48: not used)
          const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int r = 4 * g + t;
            if (!live(jb, r)) continue;
            float x = sc[jb][r];
            if (qi) {
              x += bb[t];
              if (masked) x += (L.lab[(j0 + t) & 63] != li) ? -100.0f : 0.0f;
            }
            if (j0 + t >= kTok) x = -__builtin_inff();
            p[jb][r] = x;
            m = fmaxf(m, x);
          }
        }
      m = fmaxf(m, __shfl_xor(m, 32));
      float sum = 0.f;
#pragma unroll
      for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (live(jb, r)) {
            p[jb][r] = exp_fast(p[jb][r] - m);
            sum += p[jb][r];
          } else {
            p[jb][r] = 0.f;
          }
        }
      sum += __shfl_xor(sum, 32);
      const float inv = 1.0f / sum;
      float dsum = 0.f;
#pragma unroll
      for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (live(jb, r)) {
            p[jb][r] *= inv;
            dsum += p[jb][r] * dp[jb][r];
          }
      dsum += __shfl_xor(dsum, 32);
      if (half == 0) {
        L.stat[0][i] = m;
        L.stat[1][i] = inv;
        L.stat[2][i] = dsum;
      }
      // dS in place of P; a query slot >= 49 has none
#pragma unroll
      for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (live(jb, r)) {
            p[jb][r] = qi ? p[jb][r] * (dp[jb][r] - dsum) : 0.f;
            accb[ib][jb][r] += p[jb][r];
          }

      // dQ = scale (dS . K), stored at the token the slot was read from
      const f32x16_t o = contract<MODE>(p, L.x, imgx, l32, half);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = L.tok[reg_row(ib, r, half)];
        const float val = o[r] * kScale * gi;
        if (t >= 0) grad_qkv[(size_t)t * 3 * C + hoff + l32] = val;
        else if (t == -1) accp[0] += val;
      }
    }
    __syncthreads();      // every read of the K image and every write of the table is done
    store_image(L.x, qf, l32, half);
    __syncthreads();

    // ---- pass B --------------------------------------------------------------------------------------------------------------------------------
    if constexpr (MODE != 0) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        imgx[ks] = image_operand<MODE>(L.x, ks, l32, half);
        imgg[ks] = image_operand<MODE>(L.g, ks, l32, half);
      }
    }
#pragma unroll
    for (int jb = 0; jb < 2; ++jb) {
      f32x16_t sc[2], dp[2];      // [ib]
#pragma unroll
      for (int ib = 0; ib < 2; ++ib)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sc[ib][r] = 0.f;
          dp[ib][r] = 0.f;
        }
      if constexpr (MODE == 0) {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
          for (int ib = 0; ib < 2; ++ib) {
            sc[ib] = __builtin_amdgcn_mfma_f32_32x32x2f32(qf[ib][kk], kf[jb][kk], sc[ib], 0, 0, 0);
            dp[ib] = __builtin_amdgcn_mfma_f32_32x32x2f32(gf[ib][kk], vf[jb][kk], dp[ib], 0, 0, 0);
          }
      } else {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int ib = 0; ib < 2; ++ib) {
            sc[ib] = Op::mma(pk.q[ib][kk], pk.k[jb][kk], sc[ib]);
            dp[ib] = Op::mma(pk.g[ib][kk], pk.v[jb][kk], dp[ib]);
          }
      }
      const int j = 32 * jb + l32;
      const bool kj = j < kTok;
      const int lj = L.lab[j];
      float pp[2][16], ds[2][16];      // [ib][r]: query reg_row(ib, r, half), key j
#pragma unroll
      for (int ib = 0; ib < 2; ++ib)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          pp[ib][r] = 0.f;
          ds[ib][r] = 0.f;
          if (!live(ib, r)) continue;
          const int i = reg_row(ib, r, half);
          if (i < kTok && kj) {
            float x = sc[ib][r] + L.bias[i * kBStride + j];
            if (masked) x += (L.lab[i] != lj) ? -100.0f : 0.0f;
            const float pr = exp_fast(x - L.stat[0][i]) * L.stat[1][i];
            pp[ib][r] = pr;
            ds[ib][r] = pr * (dp[ib][r] - L.stat[2][i]);
          }
        }
      const f32x16_t dv = contract<MODE>(pp, L.g, imgg, l32, half);
      const f32x16_t dk = contract<MODE>(ds, L.x, imgx, l32, half);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = L.tok[reg_row(jb, r, half)];
        const float vk = dk[r] * gi, vv = dv[r] * gi;
        if (t >= 0) {
          float* dst = grad_qkv + (size_t)t * 3 * C + hoff + l32;
          dst[C] = vk;
          dst[2 * C] = vv;
        } else if (t == -1) {
          accp[1] += vk;
          accp[2] += vv;
        }
      }
    }
    __syncthreads();      // the next window rewrites the tables and the images
  }

  // ---- this slice's partials ---------------------------------------------------------------------------------------------------------------------
  const size_t part = (size_t)slice * heads + head;
  float* wb = ws_bias + part * kBwdBiasPartial;
#pragma unroll
  for (int ib = 0; ib < 2; ++ib)
#pragma unroll
    for (int jb = 0; jb < 2; ++jb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (!live(jb, r)) continue;
        const int i = 32 * ib + l32, j = reg_row(jb, r, half);
        if (i < kTok && j < kTok) wb[j * kTok + i] = accb[ib][jb][r] * gi;
      }
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    const float s = accp[w] + __shfl_xor(accp[w], 32);
    if (half == 0) ws_pad[(part * 3 + w) * kHeadDim + l32] = s;
  }
}

// grad_rel_bias[h][i][j] and grad_qkv_pad[w C + h 32 + d]: the slices' partials in ascending order
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ ws_bias, const float* __restrict__ ws_pad,
                                                              float* __restrict__ grad_rel_bias, float* __restrict__ grad_qkv_pad, int heads,
                                                              int nslices) {
  const int nb = heads * kBwdBiasPartial, np = heads * kBwdPadPartial;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx < nb) {
    if (!grad_rel_bias) return;
    const int h = idx / kBwdBiasPartial, rem = idx % kBwdBiasPartial;      // rem = key * 49 + query
    float sum = 0.f;
    for (int s = 0; s < nslices; ++s) sum += ws_bias[((size_t)s * heads + h) * kBwdBiasPartial + rem];
    grad_rel_bias[(size_t)h * kBwdBiasPartial + (rem % kTok) * kTok + rem / kTok] = sum;
  } else if (idx - nb < np) {
    if (!grad_qkv_pad) return;
    const int e = idx - nb, C = heads * kHeadDim;
    const int w = e / C, h = (e % C) / kHeadDim, d = e % kHeadDim;
    float sum = 0.f;
    for (int s = 0; s < nslices; ++s) sum += ws_pad[(((size_t)s * heads + h) * 3 + w) * kHeadDim + d];
    grad_qkv_pad[e] = sum;
  }
}

}  // namespace

hipError_t launch_window_attention_backward(const float* qkv, const float* qkv_pad, const float* rel_bias, const float* grad_out, float* grad_qkv,
                                            float* grad_qkv_pad, float* grad_rel_bias, float* workspace, const float* scale, int B, int H, int W,
                                            int heads, int shift, int mode, hipStream_t stream) {
  Frame f;
  f.H = H;
  f.W = W;
  f.nwy = (H + kWindow - 1) / kWindow;
  f.nwx = (W + kWindow - 1) / kWindow;
  f.Hp = f.nwy * kWindow;
  f.Wp = f.nwx * kWindow;
  f.shift = shift;
  const int nwin = B * f.nwy * f.nwx;
  const int per_slice = backward_windows_per_slice(nwin), nslices = (int)backward_slices(nwin);
  float* ws_bias = workspace;
  float* ws_pad = workspace + (size_t)nslices * heads * kBwdBiasPartial;
  const dim3 g(nslices * heads), blk(64);
  if (mode == 0)
    hipLaunchKernelGGL(window_attention_backward_kernel<0>, g, blk, 0, stream, qkv, qkv_pad, rel_bias, grad_out, grad_qkv, ws_bias, ws_pad, scale, f,
                       heads, nwin, per_slice);
  else if (mode == 1)
    hipLaunchKernelGGL(window_attention_backward_kernel<1>, g, blk, 0, stream, qkv, qkv_pad, rel_bias, grad_out, grad_qkv, ws_bias, ws_pad, scale, f,
                       heads, nwin, per_slice);
  else
    hipLaunchKernelGGL(window_attention_backward_kernel<2>, g, blk, 0, stream, qkv, qkv_pad, rel_bias, grad_out, grad_qkv, ws_bias, ws_pad, scale, f,
                       heads, nwin, per_slice);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || (!grad_rel_bias && !grad_qkv_pad)) return e;
  const int n = heads * (kBwdBiasPartial + kBwdPadPartial);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const float*)ws_bias, (const float*)ws_pad, grad_rel_bias,
                     grad_qkv_pad, heads, nslices);
  return hipGetLastError();
}

}  // namespace ddswin
