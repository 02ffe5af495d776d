// dd_swin.hip -- the shifted-window attention of the Swin backbone (include/ddepth_swin.h), forward, window 7, head dimension 32.
//
// One wave per task = (image, window, head); 49 tokens padded to 64 slots.  What the reference does with copies is addressing here: slot s of
// window (wy, wx) sits at (r, c) = (7 wy + s / 7, 7 wx + s % 7) of the ROLLED padded frame, which is token ((r + shift) mod Hp, (c + shift) mod Wp)
// of the padded frame -- read from qkv when it lies inside the image, from qkv_pad otherwise, and stored only when it lies inside.
//
//   scores, transposed   S^T = K . (scale Q)^T    A = K  (row = key   = lane % 32, 8 contiguous d per lane: a straight 32-byte global load)
//                                                 B = Q^T (col = query = lane % 32, same d)
//                        D register r of block (jb, ib): key 32 jb + 8 (r / 4) + 4 (lane / 32) + r % 4, query 32 ib + lane % 32
//                        so a query's column lives in lanes l and l ^ 32: max and sum are in-lane plus one exchange.
//   output               O = P . V                A = P  (row = query = lane % 32): the contraction index may be permuted, as long as A and B
//                                                 agree, so k-step ks takes registers 8 (ks % 2) .. + 8 of block jb = ks / 2 as they are
//                                                 B = V  (col = d = lane % 32, the same keys): the one operand that needs a transpose, read
//                                                 from a [key][d] fp32 image in the LDS
//                        D register r of block ib: query 32 ib + 8 (r / 4) + 4 (lane / 32) + r % 4, d = lane % 32: a half-wave stores the
//                        128 contiguous bytes of one token's head slice
// The fp32 mode runs the same data through v_mfma_f32_32x32x2_f32, one contraction index per half-wave and step.
//
// A workgroup is two waves with an LDS region each (V image, the head's bias in rows of 52, the slots' token and mask-label tables); the grid is
// persistent and strides over the tasks, and its size is chosen so that a wave keeps its head -- the bias is loaded once per wave then.
// A wave issues the global loads of its NEXT task before it computes the current one: with one wave per SIMD the loads' latency hides behind
// the MFMAs and the softmax, not behind other waves.
// The two workgroup barriers per pass only order a wave's own LDS writes and reads; every wave of a workgroup makes the same number of passes.
#include "dd_swin_dev.h"

namespace ddswin {
namespace {

constexpr int kWaves = 2;

struct alignas(16) WaveLds {
  float v[kSlots * kVStride];
  float bias[kTok * kBStride + 8];      // (+ 8: the 16-byte read of keys 52..55 in the last row stays inside)
  int tok[kSlots];      // token index of the slot inside the image, -1: a padded position or a slot >= 49
  int lab[kSlots];      // shift-mask label 3 * row band + column band (0 without a shift)
};

// The rows of one task as the global loads deliver them.  q, k: [slot block][c]: d = 16 (c / 2) + 8 half + 4 (c % 2) ..+ 4 of slot 32 blk + lane % 32;
// v: key 8 it + lane / 8, d = 4 (lane % 8) ..+ 4 (eight lanes read a token's 128 bytes).  Slots >= 49 and a NULL qkv_pad are zeros.
struct Loaded {
  float4 q[2][4], k[2][4], v[8];
};

__device__ __forceinline__ void load_task(Loaded& r, const float* __restrict__ qkv, const float* __restrict__ qkv_pad, const Frame& f, int heads,
                                          int task, int ntasks, int lane) {
  if (task >= ntasks) return;      // (uniform over the wave; the registers are not read then)
  const int C = heads * kHeadDim, l32 = lane & 31, half = lane >> 5;
  const int head = task % heads, win = task / heads;
  const int wx = win % f.nwx, wy = (win / f.nwx) % f.nwy, b = win / (f.nwx * f.nwy);
  const size_t hoff = (size_t)head * kHeadDim;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    const int s = 32 * blk + l32;
    int label;
    const int t = s < kTok ? slot_token(f, b, wy, wx, s, label) : -1;
    const float* src = s >= kTok ? nullptr : (t >= 0 ? qkv + (size_t)t * 3 * C : qkv_pad);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      r.q[blk][c] = zero;
      r.k[blk][c] = zero;
      if (src) {
        const float* p = src + hoff + 16 * (c / 2) + 8 * half + 4 * (c % 2);
        r.q[blk][c] = load4(p);
        r.k[blk][c] = load4(p + C);
      }
    }
  }
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int s = 8 * it + (lane >> 3);
    r.v[it] = zero;
    if (s < kTok) {
      int label;
      const int t = slot_token(f, b, wy, wx, s, label);
      const float* src = t >= 0 ? qkv + (size_t)t * 3 * C : qkv_pad;
      if (src) r.v[it] = load4(src + 2 * C + hoff + 4 * (lane & 7));
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(kWaves * 64) void window_attention_kernel(const float* __restrict__ qkv, const float* __restrict__ qkv_pad,
                                                                       const float* __restrict__ rel_bias, float* __restrict__ out, Frame f,
                                                                       int heads, int ntasks) {
  __shared__ WaveLds lds[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l32 = lane & 31, half = lane >> 5;
  WaveLds& L = lds[wave];
  const int C = heads * kHeadDim;
  int cached_head = -1;

  const int stride = gridDim.x * kWaves;
  Loaded cur;
  load_task(cur, qkv, qkv_pad, f, heads, blockIdx.x * kWaves + wave, ntasks, lane);

  for (int base = blockIdx.x * kWaves; base < ntasks; base += stride) {
    const int task = base + wave;
    const bool valid = task < ntasks;      // uniform over the wave
    const int head = task % heads, win = task / heads;
    const int wx = win % f.nwx, wy = (win / f.nwx) % f.nwy, b = win / (f.nwx * f.nwy);
    // without a shift, and in every window above the last row and left of the last column of windows, all labels are equal: no mask term
    const bool masked = f.shift > 0 && (wy == f.nwy - 1 || wx == f.nwx - 1);
    float qf[2][16], kf[2][16];      // [slot block][8 kk + e]: d = 16 kk + 8 half + e of slot 32 blk + lane % 32

    if (valid) {
      // ---- this task's rows are in registers (loaded one pass ahead): v into the LDS image, the slot tables, the head's bias ------------------------
#pragma unroll
      for (int it = 0; it < 8; ++it)      // rows 49..63 are zeros: their probabilities are zeros too, and 0 * 0 adds nothing
        *reinterpret_cast<float4*>(&L.v[(8 * it + (lane >> 3)) * kVStride + 4 * (lane & 7)]) = cur.v[it];
      {
        int label = 0;
        const int t = lane < kTok ? slot_token(f, b, wy, wx, lane, label) : -1;
        L.tok[lane] = t;
        L.lab[lane] = label;
      }
      if (head != cached_head) {      // rows of 49 -> rows of kBStride; with a grid that keeps a wave's head this runs once per wave
        const float* bsrc = rel_bias + (size_t)head * kTok * kTok;
        for (int idx = lane; idx < kTok * kTok; idx += 64) L.bias[(idx / kTok) * kBStride + idx % kTok] = bsrc[idx];
        cached_head = head;
      }
#pragma unroll
      for (int blk = 0; blk < 2; ++blk)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float4 q = cur.q[blk][c], k = cur.k[blk][c];
          float* qd = &qf[blk][4 * c];
          float* kd = &kf[blk][4 * c];
          qd[0] = q.x * kScale; qd[1] = q.y * kScale; qd[2] = q.z * kScale; qd[3] = q.w * kScale;
          kd[0] = k.x; kd[1] = k.y; kd[2] = k.z; kd[3] = k.w;
        }
    }
    __syncthreads();
    // the next pass's rows: in flight while this pass computes
    load_task(cur, qkv, qkv_pad, f, heads, task + stride, ntasks, lane);

    if (valid) {
      // ---- S^T = K . Q^T ----------------------------------------------------------------------------------------------------------------------
      f32x16_t sc[2][2];      // [jb][ib]
#pragma unroll
      for (int jb = 0; jb < 2; ++jb)
#pragma unroll
        for (int ib = 0; ib < 2; ++ib)
#pragma unroll
          for (int r = 0; r < 16; ++r) sc[jb][ib][r] = 0.f;
      if constexpr (MODE == 0) {
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
          for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int ib = 0; ib < 2; ++ib) sc[jb][ib] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[jb][kk], qf[ib][kk], sc[jb][ib], 0, 0, 0);
      } else {
        typename Operand<MODE>::T ka[2][2], qb[2][2];
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            f32x8_t kx, qx;
#pragma unroll
            for (int e = 0; e < 8; ++e) { kx[e] = kf[blk][8 * kk + e]; qx[e] = qf[blk][8 * kk + e]; }
            ka[blk][kk] = Operand<MODE>::pack(kx);
            qb[blk][kk] = Operand<MODE>::pack(qx);
          }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int ib = 0; ib < 2; ++ib) sc[jb][ib] = Operand<MODE>::mma(ka[jb][kk], qb[ib][kk], sc[jb][ib]);
      }

      // the V operand of the 16-bit modes: k-step ks, element e <-> key 32 (ks / 2) + 8 (2 (ks % 2) + e / 4) + 4 half + e % 4
      [[maybe_unused]] typename Operand<MODE == 0 ? 1 : MODE>::T vb[4];
      if constexpr (MODE != 0) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          f32x8_t vx;
#pragma unroll
          for (int e = 0; e < 8; ++e) vx[e] = L.v[(32 * (ks / 2) + 8 * (2 * (ks % 2) + e / 4) + 4 * half + e % 4) * kVStride + l32];
          vb[ks] = Operand<MODE>::pack(vx);
        }
      }

#pragma unroll
      for (int ib = 0; ib < 2; ++ib) {
        // ---- softmax over the keys of query i: + bias, + mask, - max, exp, / sum, all fp32 -----------------------------------------------------
        // Registers 9..15 of block jb = 1 hold keys >= 49 in both half-waves and register 8 holds key 48 or 52: they take no part (live()).
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
              float x = sc[jb][ib][r];
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
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (live(jb, r)) p[jb][r] *= inv;

        // ---- O = P . V --------------------------------------------------------------------------------------------------------------------
        f32x16_t o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = 0.f;
        if constexpr (MODE == 0) {
#pragma unroll
          for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
              if (!live(jb, r)) continue;      // (p is 0 there)
              const int j = 32 * jb + 8 * (r / 4) + 4 * half + r % 4;
              o = __builtin_amdgcn_mfma_f32_32x32x2f32(p[jb][r], L.v[j * kVStride + l32], o, 0, 0, 0);
            }
        } else {
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            f32x8_t px;
#pragma unroll
            for (int e = 0; e < 8; ++e) px[e] = p[ks / 2][8 * (ks % 2) + e];
            o = Operand<MODE>::mma(Operand<MODE>::pack(px), vb[ks], o);
          }
        }

        // ---- reverse roll and crop: a slot is stored at the token it was read from, padded positions never -------------------------------
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int t = L.tok[32 * ib + 8 * (r / 4) + 4 * half + r % 4];
          if (t >= 0) out[(size_t)t * C + (size_t)head * kHeadDim + l32] = o[r];
        }
      }
    }
    __syncthreads();
  }
}

}  // namespace

hipError_t launch_window_attention(const float* qkv, const float* qkv_pad, const float* rel_bias, float* out, int B, int H, int W, int heads,
                                   int shift, int mode, hipStream_t stream) {
  Frame f;
  f.H = H;
  f.W = W;
  f.nwy = (H + kWindow - 1) / kWindow;
  f.nwx = (W + kWindow - 1) / kWindow;
  f.Hp = f.nwy * kWindow;
  f.Wp = f.nwx * kWindow;
  f.shift = shift;
  const int ntasks = B * f.nwy * f.nwx * heads;
  int dev = 0, cus = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  // two workgroups (four waves) per CU walk the tasks; a workgroup count that is a multiple of heads / gcd(heads, 2) keeps every wave on one head
  int grid = (ntasks + kWaves - 1) / kWaves;
  const int cap = 2 * (cus > 0 ? cus : 1);
  if (grid > cap) {
    const int keep = heads % 2 == 0 ? heads / 2 : heads;
    grid = cap >= keep ? cap / keep * keep : cap;
  }
  const dim3 g(grid), blk(kWaves * 64);
  if (mode == 0) hipLaunchKernelGGL(window_attention_kernel<0>, g, blk, 0, stream, qkv, qkv_pad, rel_bias, out, f, heads, ntasks);
  else if (mode == 1) hipLaunchKernelGGL(window_attention_kernel<1>, g, blk, 0, stream, qkv, qkv_pad, rel_bias, out, f, heads, ntasks);
  else hipLaunchKernelGGL(window_attention_kernel<2>, g, blk, 0, stream, qkv, qkv_pad, rel_bias, out, f, heads, ntasks);
  return hipGetLastError();
}

}  // namespace ddswin
