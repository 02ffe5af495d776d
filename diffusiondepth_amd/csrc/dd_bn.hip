// dd_bn.hip -- batch-statistics BatchNorm2d with a fused activation, forward and backward, as bandwidth-bound HIP kernels for gfx950
// (include/ddepth_bn.h), and the apply with a fused addend and its one-pass backward reduction (include/ddepth_bn_add.h).  Tensors are contiguous fp32 NCHW: channel c of image b is the PLANE (b * C + c) of HW values.
//
// Structure:
//   grid (G, C, B): the G workgroups of a plane (256 threads each) stride over it with 16-byte loads and stores; a scalar head / tail covers
//   planes whose first value is not 16-byte aligned or whose size is not a multiple of 4 (HW is odd at several pyramid levels, and then the
//   alignment changes from plane to plane).  Splitting planes keeps the chip busy where there are few of them (the decoder: 16 channels at
//   full resolution).  The per-plane constants (mean, invstd * weight, bias, the two backward means) are uniform in a workgroup and are
//   formed once, in front of its loop.
//   The two reductions accumulate per thread in fp64, reduce a wave by cross-lane shuffles and the four waves through LDS, and store ONE
//   fp64 pair per workgroup into the workspace; a second launch of one workgroup per channel adds a channel's B * G pairs in a FIXED order
//   (thread t takes pairs t, t + 256, ..., then the same tree).  No floating-point atomics: two calls on the same inputs give the same bits.
//
// The pre-activation z is formed by ONE function (preact) in the forward and in both backward kernels, as an explicit fused multiply-add:
// the backward's activation mask is then the forward's, bit for bit, without a saved mask.
//
// Only constructs the host emulation of the tests provides (shuffles, __syncthreads): this file runs on the CPU unchanged.
#include "dd_bn.h"

#include <cmath>

namespace ddbn {

namespace {

enum { kActNone = 0, kActRelu = 1, kActLeaky = 2 };

// ---- fixed-order workgroup reduction of a pair: shuffles inside a wave, LDS across the four waves; thread k < 2 returns value k ----------
// lds: 8 doubles.  Contains two barriers; every thread of the workgroup must call it.
__device__ __forceinline__ double block_reduce2(double v0, double v1, double* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    v0 += __shfl_down(v0, off, 64);
    v1 += __shfl_down(v1, off, 64);
  }
  __syncthreads();      // the previous use of lds is over
  if (lane == 0) {
    lds[wave * 2 + 0] = v0;
    lds[wave * 2 + 1] = v1;
  }
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x < 2) r = ((lds[threadIdx.x] + lds[2 + threadIdx.x]) + lds[4 + threadIdx.x]) + lds[6 + threadIdx.x];
  return r;
}

// how one plane is cut into a scalar head, 16-byte vectors and a scalar tail.  Every tensor a kernel touches must agree on the alignment
// of the plane's first value, else the whole plane is scalar.
struct Span {
  int head, nvec, nscalar;      // nscalar = head + tail
};

__device__ __forceinline__ Span make_span(const void* a, const void* b, const void* c, int n) {
  const unsigned long long ua = (unsigned long long)a, ub = (unsigned long long)b, uc = (unsigned long long)c;
  Span s;
  if ((ua & 15) == (ub & 15) && (ua & 15) == (uc & 15) && (ua & 3) == 0) {
    const int h = (int)(((16 - (ua & 15)) & 15) >> 2);
    s.head = h < n ? h : n;
  } else {
    s.head = n;
  }
  s.nvec = (n - s.head) >> 2;
  s.nscalar = n - 4 * s.nvec;
  return s;
}

// the same cut for a kernel of four tensors (dd_bn_backward_reduce_add_kernel)
__device__ __forceinline__ Span make_span(const void* a, const void* b, const void* c, const void* d, int n) {
  if ((((unsigned long long)a) & 15) != (((unsigned long long)d) & 15)) {
    Span s;
    s.head = n;
    s.nvec = 0;
    s.nscalar = n;
    return s;
  }
  return make_span(a, b, c, n);
}

// index of the j-th scalar value (j < nscalar): the head first, then the tail behind the vectors.  Always < n.
__device__ __forceinline__ int scalar_index(const Span& s, int j) { return j < s.head ? j : j + 4 * s.nvec; }

// ---- per-value arithmetic ---------------------------------------------------------------------------------------------------------------------
struct PlaneConst {
  float mean, invstd, scale, shift;      // scale = invstd * weight, shift = bias
};

__device__ __forceinline__ PlaneConst plane_const(const float* mean_invstd, const float* weight, const float* bias, int C, int c) {
  PlaneConst k;
  k.mean = mean_invstd[c];
  k.invstd = mean_invstd[C + c];
  k.scale = weight ? k.invstd * weight[c] : k.invstd;
  k.shift = bias ? bias[c] : 0.0f;
  return k;
}

// z of the forward AND of the backward's mask: one rounding of the product-sum, the same bits wherever it is called
__device__ __forceinline__ float preact(float x, const PlaneConst& k) { return fmaf(x - k.mean, k.scale, k.shift); }

// torch.relu / F.leaky_relu: a NaN passes through
__device__ __forceinline__ float act_forward(float z, int act, float slope) {
  if (act == kActRelu) return z < 0.0f ? 0.0f : z;
  if (act == kActLeaky) return z > 0.0f ? z : z * slope;
  return z;
}

// grad_y * act'(z) with torch's edge rules: ReLU passes nothing at z <= 0, LeakyReLU passes slope there; a NaN z passes grad_y (ReLU)
__device__ __forceinline__ float act_backward(float z, float gy, int act, float slope) {
  if (act == kActRelu) return z <= 0.0f ? 0.0f : gy;
  if (act == kActLeaky) return z > 0.0f ? gy : gy * slope;
  return gy;
}

struct Acc2 {
  double a = 0.0, b = 0.0;
};

__device__ __forceinline__ void stats_value(float x, Acc2& s) {
  const double d = (double)x;
  s.a += d;
  s.b += d * d;
}

__device__ __forceinline__ void bwd_value(float x, float gy, const PlaneConst& k, int act, float slope, Acc2& s) {
  const float g = act_backward(preact(x, k), gy, act, slope);
  const float xh = (x - k.mean) * k.invstd;
  s.a += (double)g;
  s.b += (double)g * (double)xh;
}

// one fp64 pair per workgroup: partials[((c * B + b) * G + g) * 2 + k] -- the pairs of a channel are contiguous, images in order
__device__ __forceinline__ void store_partial(double* partials, double r) {
  if (threadIdx.x < 2) {
    const size_t row = ((size_t)blockIdx.y * gridDim.z + blockIdx.z) * gridDim.x + blockIdx.x;
    partials[row * 2 + threadIdx.x] = r;
  }
}

// ---- kernels ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void dd_bn_stats_kernel(const float* __restrict__ x, double* __restrict__ partials, int C, int hw) {
  __shared__ double lds[8];
  const float* p = x + ((size_t)blockIdx.z * C + blockIdx.y) * (size_t)hw;
  const Span s = make_span(p, p, p, hw);
  const int tid = blockIdx.x * kThreads + threadIdx.x, stride = gridDim.x * kThreads;
  const float4* v = reinterpret_cast<const float4*>(p + s.head);
  Acc2 acc;
  int i = tid;
  for (; i + 3 * stride < s.nvec; i += 4 * stride) {      // four independent 16-byte loads in flight per thread
    const float4 q0 = v[i], q1 = v[i + stride], q2 = v[i + 2 * stride], q3 = v[i + 3 * stride];
    stats_value(q0.x, acc); stats_value(q0.y, acc); stats_value(q0.z, acc); stats_value(q0.w, acc);
    stats_value(q1.x, acc); stats_value(q1.y, acc); stats_value(q1.z, acc); stats_value(q1.w, acc);
    stats_value(q2.x, acc); stats_value(q2.y, acc); stats_value(q2.z, acc); stats_value(q2.w, acc);
    stats_value(q3.x, acc); stats_value(q3.y, acc); stats_value(q3.z, acc); stats_value(q3.w, acc);
  }
  for (; i < s.nvec; i += stride) {
    const float4 q = v[i];
    stats_value(q.x, acc); stats_value(q.y, acc); stats_value(q.z, acc); stats_value(q.w, acc);
  }
  for (int j = tid; j < s.nscalar; j += stride) stats_value(p[scalar_index(s, j)], acc);
  store_partial(partials, block_reduce2(acc.a, acc.b, lds));
}

__global__ __launch_bounds__(kThreads) void dd_bn_backward_reduce_kernel(const float* __restrict__ x, const float* __restrict__ grad_y,
                                                                         const float* __restrict__ mean_invstd, const float* __restrict__ weight,
                                                                         const float* __restrict__ bias, double* __restrict__ partials, int act,
                                                                         float slope, int C, int hw) {
  __shared__ double lds[8];
  const int c = blockIdx.y;
  const PlaneConst k = plane_const(mean_invstd, weight, bias, C, c);
  const size_t base = ((size_t)blockIdx.z * C + c) * (size_t)hw;
  const float* p = x + base;
  const float* q = grad_y + base;
  const Span s = make_span(p, q, q, hw);
  const int tid = blockIdx.x * kThreads + threadIdx.x, stride = gridDim.x * kThreads;
  const float4* vp = reinterpret_cast<const float4*>(p + s.head);
  const float4* vq = reinterpret_cast<const float4*>(q + s.head);
  Acc2 acc;
  int i = tid;
  for (; i + stride < s.nvec; i += 2 * stride) {      // two 16-byte loads per tensor in flight per thread
    const float4 a0 = vp[i], a1 = vp[i + stride], g0 = vq[i], g1 = vq[i + stride];
    bwd_value(a0.x, g0.x, k, act, slope, acc); bwd_value(a0.y, g0.y, k, act, slope, acc);
    bwd_value(a0.z, g0.z, k, act, slope, acc); bwd_value(a0.w, g0.w, k, act, slope, acc);
    bwd_value(a1.x, g1.x, k, act, slope, acc); bwd_value(a1.y, g1.y, k, act, slope, acc);
    bwd_value(a1.z, g1.z, k, act, slope, acc); bwd_value(a1.w, g1.w, k, act, slope, acc);
  }
  for (; i < s.nvec; i += stride) {
    const float4 a = vp[i], g = vq[i];
    bwd_value(a.x, g.x, k, act, slope, acc); bwd_value(a.y, g.y, k, act, slope, acc);
    bwd_value(a.z, g.z, k, act, slope, acc); bwd_value(a.w, g.w, k, act, slope, acc);
  }
  for (int j = tid; j < s.nscalar; j += stride) {
    const int e = scalar_index(s, j);
    bwd_value(p[e], q[e], k, act, slope, acc);
  }
  store_partial(partials, block_reduce2(acc.a, acc.b, lds));
}

// one workgroup per channel: out[c] and out[C + c] from the channel's `rows` pairs; count >= 0 also goes to out[2C] (workgroup 0)
__global__ __launch_bounds__(kThreads) void dd_bn_combine_kernel(const double* __restrict__ partials, double* __restrict__ out, int rows, int C,
                                                                 double count) {
  __shared__ double lds[8];
  const int c = blockIdx.x;
  const double* row = partials + (size_t)c * rows * 2;
  double v0 = 0.0, v1 = 0.0;
  for (int r = threadIdx.x; r < rows; r += kThreads) {
    v0 += row[2 * r];
    v1 += row[2 * r + 1];
  }
  const double r = block_reduce2(v0, v1, lds);
  if (threadIdx.x < 2) out[threadIdx.x * C + c] = r;
  if (count >= 0.0 && c == 0 && threadIdx.x == 0) out[2 * C] = count;
}

__global__ __launch_bounds__(kThreads) void dd_bn_finalize_kernel(const double* __restrict__ sums, float eps, float momentum,
                                                                  float* __restrict__ mean_invstd, float* __restrict__ running_mean,
                                                                  float* __restrict__ running_var, int C) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= C) return;
  const double N = sums[2 * C];
  const double mean = sums[c] / N;
  double var = sums[C + c] / N - mean * mean;
  if (var < 0.0) var = 0.0;      // (a NaN stays a NaN)
  mean_invstd[c] = (float)mean;
  mean_invstd[C + c] = (float)(1.0 / sqrt(var + (double)eps));
  if (running_mean) {
    const double m = (double)momentum;
    running_mean[c] = (float)((1.0 - m) * (double)running_mean[c] + m * mean);
    running_var[c] = (float)((1.0 - m) * (double)running_var[c] + m * (var * (N / (N - 1.0))));
  }
}

__global__ __launch_bounds__(kThreads) void dd_bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean_invstd,
                                                               const float* __restrict__ weight, const float* __restrict__ bias,
                                                               float* __restrict__ y, int act, float slope, int C, int hw) {
  const int c = blockIdx.y;
  const PlaneConst k = plane_const(mean_invstd, weight, bias, C, c);
  const size_t base = ((size_t)blockIdx.z * C + c) * (size_t)hw;
  const float* p = x + base;
  float* o = y + base;
  const Span s = make_span(p, o, o, hw);
  const int tid = blockIdx.x * kThreads + threadIdx.x, stride = gridDim.x * kThreads;
  const float4* vp = reinterpret_cast<const float4*>(p + s.head);
  float4* vo = reinterpret_cast<float4*>(o + s.head);
  for (int i = tid; i < s.nvec; i += stride) {
    const float4 a = vp[i];
    float4 r;
    r.x = act_forward(preact(a.x, k), act, slope);
    r.y = act_forward(preact(a.y, k), act, slope);
    r.z = act_forward(preact(a.z, k), act, slope);
    r.w = act_forward(preact(a.w, k), act, slope);
    vo[i] = r;
  }
  for (int j = tid; j < s.nscalar; j += stride) {
    const int e = scalar_index(s, j);
    o[e] = act_forward(preact(p[e], k), act, slope);
  }
}

struct BwdConst {
  float c0, m1, m2;      // weight * invstd, sum g / N, sum(g * xhat) / N
};

__device__ __forceinline__ float grad_value(float x, float gy, const PlaneConst& k, const BwdConst& w, int act, float slope) {
  const float g = act_backward(preact(x, k), gy, act, slope);
  const float xh = (x - k.mean) * k.invstd;
  return w.c0 * ((g - w.m1) - xh * w.m2);
}

__global__ __launch_bounds__(kThreads) void dd_bn_backward_apply_kernel(const float* __restrict__ x, const float* __restrict__ grad_y,
                                                                        const float* __restrict__ mean_invstd, const float* __restrict__ weight,
                                                                        const float* __restrict__ bias, const double* __restrict__ sums2,
                                                                        const double* __restrict__ sums, float* __restrict__ grad_x, int act,
                                                                        float slope, int C, int hw) {
  const int c = blockIdx.y;
  const PlaneConst k = plane_const(mean_invstd, weight, bias, C, c);
  const double N = sums[2 * C];
  BwdConst w;
  w.c0 = k.scale;
  w.m1 = (float)(sums2[c] / N);
  w.m2 = (float)(sums2[C + c] / N);
  const size_t base = ((size_t)blockIdx.z * C + c) * (size_t)hw;
  const float* p = x + base;
  const float* q = grad_y + base;
  float* o = grad_x + base;
  const Span s = make_span(p, q, o, hw);
  const int tid = blockIdx.x * kThreads + threadIdx.x, stride = gridDim.x * kThreads;
  const float4* vp = reinterpret_cast<const float4*>(p + s.head);
  const float4* vq = reinterpret_cast<const float4*>(q + s.head);
  float4* vo = reinterpret_cast<float4*>(o + s.head);
  for (int i = tid; i < s.nvec; i += stride) {
    const float4 a = vp[i], g = vq[i];
    float4 r;
    r.x = grad_value(a.x, g.x, k, w, act, slope);
    r.y = grad_value(a.y, g.y, k, w, act, slope);
    r.z = grad_value(a.z, g.z, k, w, act, slope);
    r.w = grad_value(a.w, g.w, k, w, act, slope);
    vo[i] = r;
  }
  for (int j = tid; j < s.nscalar; j += stride) {
    const int e = scalar_index(s, j);
    o[e] = grad_value(p[e], q[e], k, w, act, slope);
  }
}

// ---- the apply with an addend, and the one-pass backward reduction of its PRE mode (include/ddepth_bn_add.h) -------------------------------------
// one fp32 add, never contracted into the LeakyReLU's multiply: POST-mode y is dd_bn_apply's y plus r, bit for bit
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// post: act(z) + r (the FPN's top-down add), else act(z + r) (a BasicBlock's tail); z is preact(), as everywhere
__device__ __forceinline__ float apply_add_value(float x, float r, const PlaneConst& k, int act, float slope, bool post) {
  const float z = preact(x, k);
  return post ? add_rn(act_forward(z, act, slope), r) : act_forward(add_rn(z, r), act, slope);
}

__global__ __launch_bounds__(kThreads) void dd_bn_apply_add_kernel(const float* __restrict__ x, const float* __restrict__ mean_invstd,
                                                                   const float* __restrict__ weight, const float* __restrict__ bias,
                                                                   const float* __restrict__ addend, float* __restrict__ y, int act,
                                                                   float slope, int post, int C, int hw) {
  const int c = blockIdx.y;
  const PlaneConst k = plane_const(mean_invstd, weight, bias, C, c);
  const bool po = post != 0;
  const size_t base = ((size_t)blockIdx.z * C + c) * (size_t)hw;
  const float* p = x + base;
  const float* q = addend + base;
  float* o = y + base;
  const Span s = make_span(p, q, o, hw);
  const int tid = blockIdx.x * kThreads + threadIdx.x, stride = gridDim.x * kThreads;
  const float4* vp = reinterpret_cast<const float4*>(p + s.head);
  const float4* vq = reinterpret_cast<const float4*>(q + s.head);
  float4* vo = reinterpret_cast<float4*>(o + s.head);
  for (int i = tid; i < s.nvec; i += stride) {
    const float4 a = vp[i], r = vq[i];
    float4 v;
    v.x = apply_add_value(a.x, r.x, k, act, slope, po);
    v.y = apply_add_value(a.y, r.y, k, act, slope, po);
    v.z = apply_add_value(a.z, r.z, k, act, slope, po);
    v.w = apply_add_value(a.w, r.w, k, act, slope, po);
    vo[i] = v;
  }
  for (int j = tid; j < s.nscalar; j += stride) {
    const int e = scalar_index(s, j);
    o[e] = apply_add_value(p[e], q[e], k, act, slope, po);
  }
}

// g = grad_y * act'(y) from the forward's OUTPUT y (act_backward's edge rules hold for y as they do for z: sign(y) = sign(z + r) for
// slope >= 0), written out, and accumulated exactly as bwd_value accumulates a grad_y that needs no mask
__device__ __forceinline__ float bwd_add_value(float x, float gy, float y, float mean, float invstd, int act, float slope, Acc2& s) {
  const float g = act_backward(y, gy, act, slope);
  const float xh = (x - mean) * invstd;
  s.a += (double)g;
  s.b += (double)g * (double)xh;
  return g;
}

// the grid, the loops, the tree and the combine launch of dd_bn_backward_reduce_kernel: on mutually aligned tensors sums2 has the bits
// dd_bn_backward_reduce(x, g, act none) gives
__global__ __launch_bounds__(kThreads) void dd_bn_backward_reduce_add_kernel(const float* __restrict__ x, const float* __restrict__ grad_y,
                                                                             const float* __restrict__ y,
                                                                             const float* __restrict__ mean_invstd, float* __restrict__ g,
                                                                             double* __restrict__ partials, int act, float slope, int C,
                                                                             int hw) {
  __shared__ double lds[8];
  const int c = blockIdx.y;
  const float mean = mean_invstd[c], invstd = mean_invstd[C + c];
  const size_t base = ((size_t)blockIdx.z * C + c) * (size_t)hw;
  const float* p = x + base;
  const float* q = grad_y + base;
  const float* t = y + base;
  float* o = g + base;
  const Span s = make_span(p, q, t, o, hw);
  const int tid = blockIdx.x * kThreads + threadIdx.x, stride = gridDim.x * kThreads;
  const float4* vp = reinterpret_cast<const float4*>(p + s.head);
  const float4* vq = reinterpret_cast<const float4*>(q + s.head);
  const float4* vt = reinterpret_cast<const float4*>(t + s.head);
  float4* vo = reinterpret_cast<float4*>(o + s.head);
  Acc2 acc;
  int i = tid;
  for (; i + stride < s.nvec; i += 2 * stride) {      // two 16-byte loads per tensor in flight per thread
    const float4 a0 = vp[i], a1 = vp[i + stride], g0 = vq[i], g1 = vq[i + stride], y0 = vt[i], y1 = vt[i + stride];
    float4 r0, r1;
    r0.x = bwd_add_value(a0.x, g0.x, y0.x, mean, invstd, act, slope, acc); r0.y = bwd_add_value(a0.y, g0.y, y0.y, mean, invstd, act, slope, acc);
    r0.z = bwd_add_value(a0.z, g0.z, y0.z, mean, invstd, act, slope, acc); r0.w = bwd_add_value(a0.w, g0.w, y0.w, mean, invstd, act, slope, acc);
    r1.x = bwd_add_value(a1.x, g1.x, y1.x, mean, invstd, act, slope, acc); r1.y = bwd_add_value(a1.y, g1.y, y1.y, mean, invstd, act, slope, acc);
    r1.z = bwd_add_value(a1.z, g1.z, y1.z, mean, invstd, act, slope, acc); r1.w = bwd_add_value(a1.w, g1.w, y1.w, mean, invstd, act, slope, acc);
    vo[i] = r0;
    vo[i + stride] = r1;
  }
  for (; i < s.nvec; i += stride) {
    const float4 a = vp[i], gq = vq[i], yy = vt[i];
    float4 r;
    r.x = bwd_add_value(a.x, gq.x, yy.x, mean, invstd, act, slope, acc); r.y = bwd_add_value(a.y, gq.y, yy.y, mean, invstd, act, slope, acc);
    r.z = bwd_add_value(a.z, gq.z, yy.z, mean, invstd, act, slope, acc); r.w = bwd_add_value(a.w, gq.w, yy.w, mean, invstd, act, slope, acc);
    vo[i] = r;
  }
  for (int j = tid; j < s.nscalar; j += stride) {
    const int e = scalar_index(s, j);
    o[e] = bwd_add_value(p[e], q[e], t[e], mean, invstd, act, slope, acc);
  }
  store_partial(partials, block_reduce2(acc.a, acc.b, lds));
}

double* partial_slab(void* workspace) { return reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + kHeaderBytes); }

}  // namespace

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------
int groups_for(int64_t hw) {
  int64_t g = (hw + kGroupElems - 1) / kGroupElems;
  if (g < 1) g = 1;
  if (g > kMaxGroups) g = kMaxGroups;
  return (int)g;
}

size_t workspace_bytes(int B, int C, int64_t hw) {
  return kHeaderBytes + (size_t)B * (size_t)C * (size_t)groups_for(hw) * 2 * sizeof(double);
}

hipError_t launch_stats(const float* x, double* sums, void* workspace, int B, int C, int hw, hipStream_t st) {
  const int G = groups_for(hw);
  double* partials = partial_slab(workspace);
  hipLaunchKernelGGL(dd_bn_stats_kernel, dim3((unsigned)G, (unsigned)C, (unsigned)B), dim3(kThreads), 0, st, x, partials, C, hw);
  hipLaunchKernelGGL(dd_bn_combine_kernel, dim3((unsigned)C), dim3(kThreads), 0, st, (const double*)partials, sums, B * G, C,
                     (double)B * (double)hw);
  return hipGetLastError();
}

hipError_t launch_finalize(const double* sums, float eps, float momentum, float* mean_invstd, float* running_mean, float* running_var, int C,
                           hipStream_t st) {
  hipLaunchKernelGGL(dd_bn_finalize_kernel, dim3((unsigned)((C + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, sums, eps, momentum,
                     mean_invstd, running_mean, running_var, C);
  return hipGetLastError();
}

hipError_t launch_apply(const float* x, const float* mean_invstd, const float* weight, const float* bias, float* y, int act, float slope,
                        int B, int C, int hw, hipStream_t st) {
  hipLaunchKernelGGL(dd_bn_apply_kernel, dim3((unsigned)groups_for(hw), (unsigned)C, (unsigned)B), dim3(kThreads), 0, st, x, mean_invstd,
                     weight, bias, y, act, slope, C, hw);
  return hipGetLastError();
}

hipError_t launch_backward_reduce(const float* x, const float* grad_y, const float* mean_invstd, const float* weight, const float* bias,
                                  int act, float slope, double* sums2, void* workspace, int B, int C, int hw, hipStream_t st) {
  const int G = groups_for(hw);
  double* partials = partial_slab(workspace);
  hipLaunchKernelGGL(dd_bn_backward_reduce_kernel, dim3((unsigned)G, (unsigned)C, (unsigned)B), dim3(kThreads), 0, st, x, grad_y, mean_invstd,
                     weight, bias, partials, act, slope, C, hw);
  hipLaunchKernelGGL(dd_bn_combine_kernel, dim3((unsigned)C), dim3(kThreads), 0, st, (const double*)partials, sums2, B * G, C, -1.0);
  return hipGetLastError();
}

hipError_t launch_backward_apply(const float* x, const float* grad_y, const float* mean_invstd, const float* weight, const float* bias,
                                 const double* sums2, const double* sums, float* grad_x, int act, float slope, int B, int C, int hw,
                                 hipStream_t st) {
  hipLaunchKernelGGL(dd_bn_backward_apply_kernel, dim3((unsigned)groups_for(hw), (unsigned)C, (unsigned)B), dim3(kThreads), 0, st, x, grad_y,
                     mean_invstd, weight, bias, sums2, sums, grad_x, act, slope, C, hw);
  return hipGetLastError();
}

hipError_t launch_apply_add(const float* x, const float* mean_invstd, const float* weight, const float* bias, const float* addend, float* y,
                            int act, float slope, int post, int B, int C, int hw, hipStream_t st) {
  hipLaunchKernelGGL(dd_bn_apply_add_kernel, dim3((unsigned)groups_for(hw), (unsigned)C, (unsigned)B), dim3(kThreads), 0, st, x, mean_invstd,
                     weight, bias, addend, y, act, slope, post, C, hw);
  return hipGetLastError();
}

hipError_t launch_backward_reduce_add(const float* x, const float* grad_y, const float* y, const float* mean_invstd, int act, float slope,
                                      float* g, double* sums2, void* workspace, int B, int C, int hw, hipStream_t st) {
  const int G = groups_for(hw);
  double* partials = partial_slab(workspace);
  hipLaunchKernelGGL(dd_bn_backward_reduce_add_kernel, dim3((unsigned)G, (unsigned)C, (unsigned)B), dim3(kThreads), 0, st, x, grad_y, y,
                     mean_invstd, g, partials, act, slope, C, hw);
  hipLaunchKernelGGL(dd_bn_combine_kernel, dim3((unsigned)C), dim3(kThreads), 0, st, (const double*)partials, sums2, B * G, C, -1.0);
  return hipGetLastError();
}

}  // namespace ddbn
