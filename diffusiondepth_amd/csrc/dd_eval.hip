// dd_eval.hip -- the two consumers of output['pred'] the reference runs after every batch, as bandwidth-bound HIP kernels for gfx950:
//   * the eight KITTI depth metrics (reference src/metric/diffusion_dcbase_metric.py:31-93): one pass over pred and gt -> nine fp64 sums per image
//   * the supervised L1 + L2 loss (src/loss/submodule/l1loss.py, l2loss.py): one fused forward pass, one elementwise backward pass
//
// Structure of both reductions:
//   grid (G, B): G workgroups of 256 threads stride over one image with 16-byte loads (a scalar head / tail covers images whose first pixel is not
//   16-byte aligned or whose size is not a multiple of 4); every thread accumulates in fp64 (counts in uint32); wave reduction by cross-lane shuffles,
//   the four waves through LDS, ONE fp64 partial row per workgroup into the workspace slab.  The slab is combined in a FIXED order -- thread t reads the
//   row of workgroup t, then the same wave / LDS tree -- either by a second one-block-per-image launch (reduce == 1) or by the last workgroup of an image
//   to arrive (reduce == 2: one integer ticket per image, agent-scope release before the add, agent-scope acquire after it; the last arriver puts the
//   ticket back to 0; the loss adds one more ticket over the images for L1 and L2).  Both orders of combination are the same, so are the bits.
//   No floating-point atomics anywhere: two calls on the same inputs give the same bits.
//
// Per-pixel arithmetic is fp32 in exactly the reference's order, and NOTHING may be contracted into an FMA: the reference rounds d*d to fp32 before it
// adds, and the three delta counts are integers that flip on one ulp of a ratio.  Hence the pragma below (hipcc's default is -ffp-contract=fast).
#pragma clang fp contract(off)

#include "dd_eval.h"

#include <cmath>

namespace ddeval {

namespace {

typedef float float4_t __attribute__((ext_vector_type(4)));

// ---- fixed-order workgroup reduction: shuffles inside a wave, LDS across the four waves; thread k < NV returns value k ----
// lds: 4 * NV doubles.  Contains two barriers; every thread of the workgroup must call it.
template <int NV>
__device__ __forceinline__ double block_reduce(double (&v)[NV], double* lds) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
  }
  __syncthreads();      // the previous use of lds is over
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) lds[wave * NV + k] = v[k];
  }
  __syncthreads();
  double r = 0.0;
  if (threadIdx.x < NV) r = ((lds[threadIdx.x] + lds[NV + threadIdx.x]) + lds[2 * NV + threadIdx.x]) + lds[3 * NV + threadIdx.x];
  return r;
}

// how one image is cut into a scalar head, 16-byte vectors and a scalar tail (both tensors must agree on the alignment, else everything is scalar)
struct Span {
  int head, nvec, nscalar;      // nscalar = head + tail
};

__device__ __forceinline__ Span make_span(const float* a, const float* b, int n) {
  const unsigned long long ua = (unsigned long long)a, ub = (unsigned long long)b;
  Span s;
  if ((ua & 15) == (ub & 15) && (ua & 3) == 0) {
    const int h = (int)(((16 - (ua & 15)) & 15) >> 2);
    s.head = h < n ? h : n;
  } else {
    s.head = n;
  }
  s.nvec = (n - s.head) >> 2;
  s.nscalar = n - 4 * s.nvec;
  return s;
}

// index of the j-th scalar element (j < nscalar): the head first, then the tail behind the vectors.  Always < n.
__device__ __forceinline__ int scalar_index(const Span& s, int j) { return j < s.head ? j : j + 4 * s.nvec; }

// ---- metrics ------------------------------------------------------------------------------------------------------------------------------
struct MetricAcc {
  double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};      // S|d|, Sd^2, S|dinv|, Sdinv^2, S|d|/(gt+1e-8)
  unsigned c[4] = {0u, 0u, 0u, 0u};              // n_valid, #(ratio < 1.25), #(ratio < 1.25^2), #(ratio < 1.25^3)
};

// diffusion_dcbase_metric.py:36-85 for one pixel, fp32, operation for operation
__device__ __forceinline__ void metric_pixel(float p, float g, float t, MetricAcc& a) {
  if (!(g > t)) return;                      // mask = gt > t_valid (:40); a NaN gt is not valid
  a.c[0] += 1u;
  const float pe = p + 1e-8f, ge = g + 1e-8f;
  float pinv = 1.0f / pe;                    // :36
  if (p <= t) pinv = 0.0f;                   // :49 (a NaN pred stays NaN)
  const float ginv = 1.0f / ge;              // :37 (:50 cannot fire: g > t here)
  const float d = p - g;                     // :53
  const float ad = fabsf(d);
  const float dd = d * d;                    // rounded to fp32 before it is added (:55)
  const float di = pinv - ginv;              // :63
  const float adi = fabsf(di);
  const float ddi = di * di;
  const float rel = ad / ge;                 // :73
  const float r1 = g / pe, r2 = p / ge;      // :77-78
  const float ratio = r1 > r2 ? r1 : r2;     // torch.max: NaN in either side gives NaN; the compares below are then false for any ordered result ...
  const bool ordered = (r1 == r1) && (r2 == r2);      // ... and this makes them false when only one side is NaN
  a.s[0] += (double)ad;
  a.s[1] += (double)dd;
  a.s[2] += (double)adi;
  a.s[3] += (double)ddi;
  a.s[4] += (double)rel;
  a.c[1] += (ordered && ratio < 1.25f) ? 1u : 0u;
  a.c[2] += (ordered && ratio < 1.5625f) ? 1u : 0u;        // 1.25^2 and 1.25^3 are exact in fp32
  a.c[3] += (ordered && ratio < 1.953125f) ? 1u : 0u;
}

// ---- supervised loss ----------------------------------------------------------------------------------------------------------------------
// torch.clamp(x, 0, max_depth): NaN passes through
__device__ __forceinline__ float clamp_depth(float x, float md) { return x < 0.0f ? 0.0f : (x > md ? md : x); }

struct LossAcc {
  double s[3] = {0.0, 0.0, 0.0};
};

// l1loss.py:26-31 and l2loss.py:26-31 for one pixel: the mask is MULTIPLIED in, as the reference does
__device__ __forceinline__ void loss_pixel(float pr, float gr, float md, float t, LossAcc& a) {
  const float g = clamp_depth(gr, md), p = clamp_depth(pr, md);
  const float m = g > t ? 1.0f : 0.0f;
  const float d = p - g;
  const float l1 = fabsf(d) * m;
  const float sq = d * d;
  const float l2 = sq * m;
  a.s[0] += (double)l1;
  a.s[1] += (double)l2;
  a.s[2] += (double)m;
}

// ---- the streaming pass shared by both families ---------------------------------------------------------------------------------------------
template <class Acc, class Fn>
__device__ __forceinline__ void stream_image(const float* __restrict__ a, const float* __restrict__ b, int n, Acc& acc, Fn fn) {
  const Span s = make_span(a, b, n);
  const int tid = blockIdx.x * kThreads + threadIdx.x, stride = gridDim.x * kThreads;
  const float4_t* va = reinterpret_cast<const float4_t*>(a + s.head);
  const float4_t* vb = reinterpret_cast<const float4_t*>(b + s.head);
  for (int i = tid; i < s.nvec; i += stride) {
    const float4_t x = va[i], y = vb[i];
    fn(x.x, y.x, acc);
    fn(x.y, y.y, acc);
    fn(x.z, y.z, acc);
    fn(x.w, y.w, acc);
  }
  for (int j = tid; j < s.nscalar; j += stride) {
    const int i = scalar_index(s, j);
    fn(a[i], b[i], acc);
  }
}

// rows of NV doubles, one per workgroup: partials[(b * G + g) * NV + k]
template <int NV>
__device__ __forceinline__ void store_partial(double* partials, double r) {
  if (threadIdx.x < NV) partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NV + threadIdx.x] = r;
}

// sums of image b in fixed order: thread t takes the row of workgroup t (G <= kThreads), then the workgroup tree.  Thread k < NV returns sum k.
template <int NV>
__device__ __forceinline__ double combine_image(const double* partials, int G, int b, double* lds) {
  double v[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = 0.0;
  if ((int)threadIdx.x < G) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = partials[((size_t)b * G + threadIdx.x) * NV + k];
  }
  return block_reduce<NV>(v, lds);
}

// The ticket of reduce == 2.  Returns true in EVERY thread of the one workgroup that arrived last, after the others' partial rows have become visible to it.
// lds_flag: one double of the workgroup's single LDS array.
__device__ __forceinline__ bool arrive_last(unsigned* ticket, unsigned total, double* lds_flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's partial stores have left
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned got = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = got == total - 1u;
    if (last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    *lds_flag = last ? 1.0 : 0.0;
  }
  __syncthreads();
  return *lds_flag != 0.0;
}

__device__ __forceinline__ void rearm(unsigned* ticket) {
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- kernels --------------------------------------------------------------------------------------------------------------------------------
template <bool TICKET>
__global__ __launch_bounds__(kThreads) void dd_metric_sums_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                    double* __restrict__ partials, unsigned* ticket, double* __restrict__ sums,
                                                                    int n, float t_valid) {
  __shared__ double lds[4 * kMetricSums + 1];
  const int b = blockIdx.y;
  MetricAcc acc;
  stream_image(pred + (size_t)b * n, gt + (size_t)b * n, n, acc, [t_valid](float p, float g, MetricAcc& a) { metric_pixel(p, g, t_valid, a); });
  double v[kMetricSums] = {(double)acc.c[0], acc.s[0], acc.s[1], acc.s[2], acc.s[3], acc.s[4], (double)acc.c[1], (double)acc.c[2], (double)acc.c[3]};
  const double r = block_reduce<kMetricSums>(v, lds);
  store_partial<kMetricSums>(partials, r);
  if (TICKET) {      // one ticket per image: the B last arrivers combine their images side by side
    if (!arrive_last(ticket + b, gridDim.x, &lds[4 * kMetricSums])) return;
    const double s = combine_image<kMetricSums>(partials, gridDim.x, b, lds);
    if (threadIdx.x < kMetricSums) sums[b * kMetricSums + threadIdx.x] = s;
    rearm(ticket + b);
  }
}

__global__ __launch_bounds__(kThreads) void dd_metric_combine_kernel(const double* __restrict__ partials, double* __restrict__ sums, int G) {
  __shared__ double lds[4 * kMetricSums];
  const double s = combine_image<kMetricSums>(partials, G, blockIdx.x, lds);
  if (threadIdx.x < kMetricSums) sums[blockIdx.x * kMetricSums + threadIdx.x] = s;
}

// sums (B, 9) fp64 -> the eight metrics with the reference's formulas (:57-90): x / (n_valid + 1e-8), sqrt for the two RMSEs; the batch row pools the sums
// of all images first (what the reference's one masked gather over the whole batch does), in image order.
__device__ __forceinline__ void metrics_from_sums(const double* s, float* out) {
  const double den = s[0] + 1e-8;
  out[0] = (float)sqrt(s[2] / den);
  out[1] = (float)(s[1] / den);
  out[2] = (float)sqrt(s[4] / den);
  out[3] = (float)(s[3] / den);
  out[4] = (float)(s[5] / den);
  out[5] = (float)(s[6] / den);
  out[6] = (float)(s[7] / den);
  out[7] = (float)(s[8] / den);
}

__global__ __launch_bounds__(64) void dd_metric_finalize_kernel(const double* __restrict__ sums, float* __restrict__ batch_metrics,
                                                                float* __restrict__ image_metrics, int B) {
  if (image_metrics) {
    for (int b = threadIdx.x; b < B; b += 64) {
      double s[kMetricSums];
      for (int k = 0; k < kMetricSums; ++k) s[k] = sums[b * kMetricSums + k];
      metrics_from_sums(s, image_metrics + b * 8);
    }
  }
  if (batch_metrics && threadIdx.x == 0) {
    double s[kMetricSums];
    for (int k = 0; k < kMetricSums; ++k) s[k] = 0.0;
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < kMetricSums; ++k) s[k] += sums[b * kMetricSums + k];
    metrics_from_sums(s, batch_metrics);
  }
}

// the per-image sums of the loss and, from them, L1 = sum_b s1_b / (n_b + 1e-8), L2 likewise (l1loss.py:33-37), images in order.  One workgroup.
__device__ __forceinline__ void loss_combine(const double* partials, int G, int B, double* __restrict__ sums, float* __restrict__ loss, double* lds) {
  double l1 = 0.0, l2 = 0.0;
  for (int b = 0; b < B; ++b) {
    const double s = combine_image<kLossSums>(partials, G, b, lds);
    if (threadIdx.x < kLossSums) {
      sums[b * kLossSums + threadIdx.x] = s;
      lds[4 * kLossSums + threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const double den = lds[4 * kLossSums + 2] + 1e-8;
      l1 += lds[4 * kLossSums + 0] / den;
      l2 += lds[4 * kLossSums + 1] / den;
    }
  }
  if (threadIdx.x == 0) {
    loss[0] = (float)l1;
    loss[1] = (float)l2;
  }
}

template <bool TICKET>
__global__ __launch_bounds__(kThreads) void dd_sup_loss_sums_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                      double* __restrict__ partials, unsigned* ticket, double* __restrict__ sums,
                                                                      float* __restrict__ loss, int n, float max_depth, float t_valid) {
  __shared__ double lds[4 * kLossSums + kLossSums + 1];
  const int b = blockIdx.y;
  LossAcc acc;
  stream_image(pred + (size_t)b * n, gt + (size_t)b * n, n, acc,
               [max_depth, t_valid](float p, float g, LossAcc& a) { loss_pixel(p, g, max_depth, t_valid, a); });
  double v[kLossSums] = {acc.s[0], acc.s[1], acc.s[2]};
  const double r = block_reduce<kLossSums>(v, lds);
  store_partial<kLossSums>(partials, r);
  if (TICKET) {      // one ticket per image, then one over the images: whoever finishes the last image adds up L1 and L2
    double* flag = &lds[4 * kLossSums + kLossSums];
    if (!arrive_last(ticket + b, gridDim.x, flag)) return;
    const double s = combine_image<kLossSums>(partials, gridDim.x, b, lds);
    if (threadIdx.x < kLossSums) sums[b * kLossSums + threadIdx.x] = s;
    rearm(ticket + b);
    const int B = gridDim.y;
    if (B > 1) {
      if (!arrive_last(ticket + B, (unsigned)B, flag)) return;
    } else {      // one image: this workgroup wrote the row itself; only its own stores have to land
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      double l1 = 0.0, l2 = 0.0;
      for (int i = 0; i < B; ++i) {      // rows other workgroups wrote: agent-scope loads behind the acquire, image order
        const double s1 = __hip_atomic_load(sums + i * kLossSums + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double s2 = __hip_atomic_load(sums + i * kLossSums + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double den = __hip_atomic_load(sums + i * kLossSums + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1e-8;
        l1 += s1 / den;
        l2 += s2 / den;
      }
      loss[0] = (float)l1;
      loss[1] = (float)l2;
    }
    if (B > 1) rearm(ticket + B);
  }
}

__global__ __launch_bounds__(kThreads) void dd_sup_loss_combine_kernel(const double* __restrict__ partials, double* __restrict__ sums,
                                                                       float* __restrict__ loss, int G, int B) {
  __shared__ double lds[4 * kLossSums + kLossSums];
  loss_combine(partials, G, B, sums, loss, lds);
}

// grad_pred of g1 * L1 + g2 * L2, as torch autograd differentiates the reference's code, fp32, no contraction:
//   division by (n_b + 1e-8) -> expand -> * mask -> abs: * sign(p - g) (0 at 0) | pow 2: * 2 (p - g) -> clamp: * (0 <= pred <= max_depth) -> the two added
__device__ __forceinline__ float loss_grad_pixel(float pr, float gr, float md, float t, float c1, float c2) {
  const float g = clamp_depth(gr, md), p = clamp_depth(pr, md);
  const float m = g > t ? 1.0f : 0.0f;
  const float inside = (pr >= 0.0f && pr <= md) ? 1.0f : 0.0f;
  const float d = p - g;
  const float sgn = (float)((0.0f < d) - (d < 0.0f));
  const float g1 = ((c1 * m) * sgn) * inside;
  const float two_d = d * 2.0f;
  const float g2 = ((c2 * m) * two_d) * inside;
  return g1 + g2;
}

__global__ __launch_bounds__(kThreads) void dd_sup_loss_backward_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                        const double* __restrict__ sums, const float* __restrict__ grad_l1,
                                                                        const float* __restrict__ grad_l2, float* __restrict__ grad_pred, int n,
                                                                        float max_depth, float t_valid) {
  const int b = blockIdx.y;
  const float den = (float)sums[b * kLossSums + 2] + 1e-8f;      // num_valid + 1e-8 in fp32 (l1loss.py:33)
  const float c1 = grad_l1 ? grad_l1[0] / den : 0.0f;
  const float c2 = grad_l2 ? grad_l2[0] / den : 0.0f;
  const float* a = pred + (size_t)b * n;
  const float* g = gt + (size_t)b * n;
  float* o = grad_pred + (size_t)b * n;
  Span s = make_span(a, g, n);
  if ((((unsigned long long)a) & 15) != (((unsigned long long)o) & 15)) {      // the output must share the inputs' alignment for 16-byte stores
    s.head = n;
    s.nvec = 0;
    s.nscalar = n;
  }
  const int tid = blockIdx.x * kThreads + threadIdx.x, stride = gridDim.x * kThreads;
  const float4_t* va = reinterpret_cast<const float4_t*>(a + s.head);
  const float4_t* vg = reinterpret_cast<const float4_t*>(g + s.head);
  float4_t* vo = reinterpret_cast<float4_t*>(o + s.head);
  for (int i = tid; i < s.nvec; i += stride) {
    const float4_t x = va[i], y = vg[i];
    float4_t r;
    r.x = loss_grad_pixel(x.x, y.x, max_depth, t_valid, c1, c2);
    r.y = loss_grad_pixel(x.y, y.y, max_depth, t_valid, c1, c2);
    r.z = loss_grad_pixel(x.z, y.z, max_depth, t_valid, c1, c2);
    r.w = loss_grad_pixel(x.w, y.w, max_depth, t_valid, c1, c2);
    vo[i] = r;
  }
  for (int j = tid; j < s.nscalar; j += stride) {
    const int i = scalar_index(s, j);
    o[i] = loss_grad_pixel(a[i], g[i], max_depth, t_valid, c1, c2);
  }
}

}  // namespace

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------
int groups_for(int64_t n) {
  const int64_t per_group = (int64_t)kThreads * 4 * 4;      // four 16-byte loads per thread and tensor
  int64_t g = (n + per_group - 1) / per_group;
  if (g < 1) g = 1;
  if (g > kMaxGroups) g = kMaxGroups;
  return (int)g;
}

size_t workspace_bytes(int B, int64_t n) {
  return kTicketBytes + (size_t)B * (size_t)groups_for(n) * kMetricSums * sizeof(double);
}

hipError_t launch_metric_sums(const float* pred, const float* gt, double* sums, void* workspace, int B, int n, float t_valid, int reduce,
                              hipStream_t st) {
  const int G = groups_for(n);
  unsigned* ticket = reinterpret_cast<unsigned*>(workspace);
  double* partials = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + kTicketBytes);
  const dim3 grid((unsigned)G, (unsigned)B);
  if (reduce == 2 && B <= kMaxTicketImages) {
    hipLaunchKernelGGL((dd_metric_sums_kernel<true>), grid, dim3(kThreads), 0, st, pred, gt, partials, ticket, sums, n, t_valid);
  } else {
    hipLaunchKernelGGL((dd_metric_sums_kernel<false>), grid, dim3(kThreads), 0, st, pred, gt, partials, ticket, sums, n, t_valid);
    hipLaunchKernelGGL(dd_metric_combine_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, (const double*)partials, sums, G);
  }
  return hipGetLastError();
}

hipError_t launch_metric_finalize(const double* sums, float* batch_metrics, float* image_metrics, int B, hipStream_t st) {
  hipLaunchKernelGGL(dd_metric_finalize_kernel, dim3(1), dim3(64), 0, st, sums, batch_metrics, image_metrics, B);
  return hipGetLastError();
}

hipError_t launch_loss_forward(const float* pred, const float* gt, float* loss, double* sums, void* workspace, int B, int n, float max_depth,
                               float t_valid, int reduce, hipStream_t st) {
  const int G = groups_for(n);
  unsigned* ticket = reinterpret_cast<unsigned*>(workspace);
  double* partials = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + kTicketBytes);
  const dim3 grid((unsigned)G, (unsigned)B);
  if (reduce == 2 && B <= kMaxTicketImages) {
    hipLaunchKernelGGL((dd_sup_loss_sums_kernel<true>), grid, dim3(kThreads), 0, st, pred, gt, partials, ticket, sums, loss, n, max_depth, t_valid);
  } else {
    hipLaunchKernelGGL((dd_sup_loss_sums_kernel<false>), grid, dim3(kThreads), 0, st, pred, gt, partials, ticket, sums, loss, n, max_depth, t_valid);
    hipLaunchKernelGGL(dd_sup_loss_combine_kernel, dim3(1), dim3(kThreads), 0, st, (const double*)partials, sums, loss, G, B);
  }
  return hipGetLastError();
}

hipError_t launch_loss_backward(const float* pred, const float* gt, const double* sums, const float* grad_l1, const float* grad_l2,
                                float* grad_pred, int B, int n, float max_depth, float t_valid, hipStream_t st) {
  const int64_t per_group = (int64_t)kThreads * 4 * 4;
  int64_t G = (n + per_group - 1) / per_group;
  if (G < 1) G = 1;
  if (G > 1024) G = 1024;
  hipLaunchKernelGGL(dd_sup_loss_backward_kernel, dim3((unsigned)G, (unsigned)B), dim3(kThreads), 0, st, pred, gt, sums, grad_l1, grad_l2,
                     grad_pred, n, max_depth, t_valid);
  return hipGetLastError();
}

}  // namespace ddeval
