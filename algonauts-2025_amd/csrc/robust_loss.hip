// Element-wise regression losses over two flat f32 streams: nn.MSELoss (the default loss of every training run), nn.L1Loss,
// nn.SmoothL1Loss(beta) and nn.HuberLoss(delta) (run_ensemble.py draws loss.name from MSELoss / PearsonLoss / SmoothL1Loss / HuberLoss).
// `mean` and `sum` over all elements do not depend on the element order, so the "b d t -> (b t) d" flatten of pl_module.py:54-55 is
// never formed: the kernels read the contiguous [B, V, T'] pair in place.
//
// With d = p - t, a = |d|:
//   L1            value a                                    gradient sign(d) (0 at d == 0, torch's convention)
//   Huber(delta)  value m (a - m / 2), m = min(a, delta)     gradient clamp(d, -delta, delta)
//   SmoothL1(b)   Huber(b) / b for b > 0, L1 for b == 0 (torch dispatches to l1_loss there)
//   MSE           value d^2                                  gradient 2 d
// The min / clamp forms equal torch's piecewise definitions, a == delta included.  Every factor that is the same for all elements
// travels as one numerator (1 / beta, the 2 of MSE's gradient) over one denominator (n for 'mean', 1 for 'sum'), so SmoothL1 runs the
// Huber instantiation and three kinds are compiled.  tribe_mse_fwd / tribe_mse_workspace_bytes / tribe_mse_bwd, at the end of this
// file, are the (MSE, mean) instance under the names and argument checks they have always had.
#include <math.h>

#include "common.h"

namespace {

enum { K_L1 = 0, K_HUBER = 1, K_MSE = 2 };

constexpr int FWD_MAX_WG = 2048;   // tribe_elem_loss_workspace_bytes: one f64 partial sum per workgroup
constexpr int FWD_UNROLL = 4;      // float4 pairs requested before the first is consumed
constexpr int BWD_MAX_WG = 4096;

// the comparisons (not fminf / fmaxf) keep a NaN difference a NaN, as torch does
template <int KIND>
__device__ __forceinline__ float loss_value(float p, float t, float c) {
  const float d = p - t;
  if (KIND == K_MSE) return d * d;
  const float a = fabsf(d);
  if (KIND == K_L1) return a;
  const float m = a < c ? a : c;
  return m * (a - 0.5f * m);
}

// d value / d p, before the common factor
template <int KIND>
__device__ __forceinline__ float loss_slope(float p, float t, float c) {
  const float d = p - t;
  if (KIND == K_MSE) return d;                                  // the 2 is in the launcher's numerator
  if (KIND == K_L1) return d > 0.f ? 1.f : (d < 0.f ? -1.f : d);  // d == 0 -> (+-)0, NaN -> NaN
  return d < -c ? -c : (d > c ? c : d);
}

// The four squared differences of one float4 pair, added as ((d0^2 + d1^2) + d2^2) + d3^2.  These are the roundings the default loss
// has had since hipcc first contracted `d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3` for it: three FMAs onto the rounded d1^2 in the unrolled
// loop (fused), four rounded products in the remainder loop.  Spelled out, with contraction off, they no longer depend on what the
// compiler makes of the expression in a given place.
__device__ __forceinline__ float mse_value4(const float4& a, const float4& b, bool fused) {
#pragma clang fp contract(off)
  const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
  const float s1 = d1 * d1;
  if (fused) return fmaf(d3, d3, fmaf(d2, d2, fmaf(d0, d0, s1)));
  return ((d0 * d0 + s1) + d2 * d2) + d3 * d3;
}

template <int KIND>
__device__ __forceinline__ float loss_value4(const float4& a, const float4& b, float c, bool fused) {
  if (KIND == K_MSE) return mse_value4(a, b, fused);
  return (loss_value<KIND>(a.x, b.x, c) + loss_value<KIND>(a.y, b.y, c)) + (loss_value<KIND>(a.z, b.z, c) + loss_value<KIND>(a.w, b.w, c));
}

// HBM-bound: 8 bytes read per element.  Four independent float4 pairs are requested before any is consumed (128 B in flight per lane;
// 2048 workgroups x 256 lanes cover the ~16 MB the chip needs in flight at 8 TB/s), f32 partial sums of at most 16 terms are folded
// into an f64 carry.  vec == 0 (a pointer that is not 16-byte aligned, e.g. the slice x[1:] of an odd-width tensor): every element
// takes the scalar loop.
template <int KIND>
__global__ __launch_bounds__(256) void elem_loss_partial_kernel(const float* __restrict__ p, const float* __restrict__ t, int64_t n, float c,
                                                                int vec, double* __restrict__ partial) {
  __shared__ double sh[4];
  double dacc = 0.0;
  const int64_t n4 = vec ? (n >> 2) : 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float4* p4 = (const float4*)p;
  const float4* t4 = (const float4*)t;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + (FWD_UNROLL - 1) * stride < n4; i += FWD_UNROLL * stride) {
    float4 a[FWD_UNROLL], b[FWD_UNROLL];
#pragma unroll
    for (int u = 0; u < FWD_UNROLL; ++u) { a[u] = load_nt_f4(p4 + i + u * stride); b[u] = load_nt_f4(t4 + i + u * stride); }
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < FWD_UNROLL; ++u) acc += loss_value4<KIND>(a[u], b[u], c, true);
    dacc += (double)acc;
  }
  for (; i < n4; i += stride) dacc += (double)loss_value4<KIND>(p4[i], t4[i], c, false);
  for (int64_t j = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) dacc += (double)loss_value<KIND>(p[j], t[j], c);
  const double tot = block_sum_d(dacc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// one workgroup, a fixed summation order: two calls on the same input return the same bits
__global__ __launch_bounds__(256) void elem_loss_final_kernel(const double* __restrict__ partial, int nparts, double num, double den,
                                                              float* __restrict__ out) {
  __shared__ double sh[4];
  double v = 0.0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) v += partial[i];
  const double tot = block_sum_d(v, sh);
  if (threadIdx.x == 0) out[0] = (float)(tot * num / den);
}

// dpred = gs * num / den * slope(p - t).  HBM-bound: 12 bytes per element; float4 streams, two pairs in flight per lane, a scalar loop
// for the n % 4 tail and for pointers that are not 16-byte aligned.
template <int KIND>
__global__ __launch_bounds__(256) void elem_loss_bwd_kernel(const float* __restrict__ p, const float* __restrict__ t, int64_t n, float c,
                                                            float num, float den, const float* __restrict__ gs, float* __restrict__ dp,
                                                            int vec) {
  const float k = gs[0] * num / den;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n4 = vec ? (n >> 2) : 0;
  const float4* p4 = (const float4*)p;
  const float4* t4 = (const float4*)t;
  float4* d4 = (float4*)dp;
#define TRIBE_SLOPE4(a, b)                                                                                          \
  make_float4(k * loss_slope<KIND>(a.x, b.x, c), k * loss_slope<KIND>(a.y, b.y, c), k * loss_slope<KIND>(a.z, b.z, c), \
              k * loss_slope<KIND>(a.w, b.w, c))
  for (; i + stride < n4; i += 2 * stride) {
    const float4 a0 = load_nt_f4(p4 + i), b0 = load_nt_f4(t4 + i);
    const float4 a1 = load_nt_f4(p4 + i + stride), b1 = load_nt_f4(t4 + i + stride);
    d4[i] = TRIBE_SLOPE4(a0, b0);
    d4[i + stride] = TRIBE_SLOPE4(a1, b1);
  }
  for (; i < n4; i += stride) {
    const float4 a = p4[i], b = t4[i];
    d4[i] = TRIBE_SLOPE4(a, b);
  }
#undef TRIBE_SLOPE4
  for (int64_t j = (n4 << 2) + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) dp[j] = k * loss_slope<KIND>(p[j], t[j], c);
}

// kind / param / reduction -> compiled kind, clamp point and the factor num / den common to all elements (without MSE's gradient 2)
struct Plan {
  int kind;
  float c;
  double num, den;
};

static int make_plan(const char* who, int64_t n, int32_t kind, float param, int32_t reduction, Plan* plan) {
  TRIBE_REQUIRE(n > 0, "%s: empty input", who);
  TRIBE_REQUIRE(kind == TRIBE_LOSS_L1 || kind == TRIBE_LOSS_SMOOTH_L1 || kind == TRIBE_LOSS_HUBER || kind == TRIBE_LOSS_MSE,
                "%s: unknown loss kind %d", who, (int)kind);
  TRIBE_REQUIRE(reduction == TRIBE_REDUCE_MEAN || reduction == TRIBE_REDUCE_SUM, "%s: unknown reduction %d", who, (int)reduction);
  plan->kind = kind == TRIBE_LOSS_MSE ? K_MSE : K_L1;
  plan->c = 0.f;
  plan->num = 1.0;
  plan->den = reduction == TRIBE_REDUCE_MEAN ? (double)n : 1.0;
  if (kind == TRIBE_LOSS_HUBER) {
    TRIBE_REQUIRE(isfinite(param), "%s: huber_loss delta must be finite", who);
    TRIBE_REQUIRE(param > 0.f, "%s: huber_loss does not support non-positive values for delta.", who);
    plan->kind = K_HUBER;
    plan->c = param;
  } else if (kind == TRIBE_LOSS_SMOOTH_L1) {
    TRIBE_REQUIRE(isfinite(param), "%s: smooth_l1_loss beta must be finite", who);
    TRIBE_REQUIRE(param >= 0.f, "%s: smooth_l1_loss does not support negative values for beta.", who);
    if (param > 0.f) {   // beta == 0 is L1
      plan->kind = K_HUBER;
      plan->c = param;
      plan->num = 1.0 / (double)param;
    }
  }
  return 0;
}

// the two launches of a forward; the pointers are checked by the caller.  Pointers that are not 16-byte aligned take the scalar form.
static int launch_fwd(const Plan& plan, const float* pred, const float* truth, int64_t n, float* out, void* workspace, void* stream) {
  const int vec = ((uintptr_t)pred % 16) == 0 && ((uintptr_t)truth % 16) == 0;
  // one trip of the unrolled loop per lane: FWD_UNROLL float4 pairs (vec) / as many lanes as the vector form would use (scalar)
  int64_t nb = (n / 4 + 256 * FWD_UNROLL - 1) / (256 * FWD_UNROLL);
  if (nb > FWD_MAX_WG) nb = FWD_MAX_WG;
  if (nb < 1) nb = 1;
  hipStream_t s = (hipStream_t)stream;
  double* partial = (double*)workspace;
  switch (plan.kind) {
    case K_L1: hipLaunchKernelGGL(elem_loss_partial_kernel<K_L1>, dim3((unsigned)nb), dim3(256), 0, s, pred, truth, n, plan.c, vec, partial); break;
    case K_HUBER: hipLaunchKernelGGL(elem_loss_partial_kernel<K_HUBER>, dim3((unsigned)nb), dim3(256), 0, s, pred, truth, n, plan.c, vec, partial); break;
    default: hipLaunchKernelGGL(elem_loss_partial_kernel<K_MSE>, dim3((unsigned)nb), dim3(256), 0, s, pred, truth, n, plan.c, vec, partial); break;
  }
  hipLaunchKernelGGL(elem_loss_final_kernel, dim3(1), dim3(256), 0, s, (const double*)partial, (int)nb, plan.num, plan.den, out);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

static int launch_bwd(const Plan& plan, const float* pred, const float* truth, int64_t n, const float* gscale, float* dpred, void* stream) {
  const int vec = ((uintptr_t)pred % 16) == 0 && ((uintptr_t)truth % 16) == 0 && ((uintptr_t)dpred % 16) == 0;
  const float num = (float)(plan.kind == K_MSE ? 2.0 * plan.num : plan.num), den = (float)plan.den;
  int64_t nb = (n / 4 + 511) / 512;
  if (nb > BWD_MAX_WG) nb = BWD_MAX_WG;
  if (nb < 1) nb = 1;
  hipStream_t s = (hipStream_t)stream;
  switch (plan.kind) {
    case K_L1: hipLaunchKernelGGL(elem_loss_bwd_kernel<K_L1>, dim3((unsigned)nb), dim3(256), 0, s, pred, truth, n, plan.c, num, den, gscale, dpred, vec); break;
    case K_HUBER: hipLaunchKernelGGL(elem_loss_bwd_kernel<K_HUBER>, dim3((unsigned)nb), dim3(256), 0, s, pred, truth, n, plan.c, num, den, gscale, dpred, vec); break;
    default: hipLaunchKernelGGL(elem_loss_bwd_kernel<K_MSE>, dim3((unsigned)nb), dim3(256), 0, s, pred, truth, n, plan.c, num, den, gscale, dpred, vec); break;
  }
  TRIBE_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" size_t tribe_elem_loss_workspace_bytes(int64_t n) {
  (void)n;
  return FWD_MAX_WG * sizeof(double);
}

extern "C" int tribe_elem_loss_fwd(const float* pred, const float* truth, int64_t n, int32_t kind, float param, int32_t reduction, float* out,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(pred && truth && out && workspace, "tribe_elem_loss_fwd: null pointer");
  Plan plan;
  if (int rc = make_plan("tribe_elem_loss_fwd", n, kind, param, reduction, &plan)) return rc;
  TRIBE_REQUIRE(workspace_bytes >= tribe_elem_loss_workspace_bytes(n), "tribe_elem_loss_fwd: workspace too small");
  TRIBE_REQUIRE(((uintptr_t)pred % 4) == 0 && ((uintptr_t)truth % 4) == 0 && ((uintptr_t)workspace % 8) == 0,
                "tribe_elem_loss_fwd: misaligned pointer");
  return launch_fwd(plan, pred, truth, n, out, workspace, stream);
}

extern "C" int tribe_elem_loss_bwd(const float* pred, const float* truth, int64_t n, int32_t kind, float param, int32_t reduction,
                                   const float* gscale, float* dpred, void* stream) {
  TRIBE_REQUIRE(pred && truth && gscale && dpred, "tribe_elem_loss_bwd: null pointer");
  Plan plan;
  if (int rc = make_plan("tribe_elem_loss_bwd", n, kind, param, reduction, &plan)) return rc;
  TRIBE_REQUIRE(((uintptr_t)pred % 4) == 0 && ((uintptr_t)truth % 4) == 0 && ((uintptr_t)dpred % 4) == 0 && ((uintptr_t)gscale % 4) == 0,
                "tribe_elem_loss_bwd: misaligned pointer");
  return launch_bwd(plan, pred, truth, n, gscale, dpred, stream);
}

// nn.MSELoss() under its own names: the (MSE, mean) plan behind the argument checks these entry points have always made
extern "C" size_t tribe_mse_workspace_bytes(int64_t n) { return tribe_elem_loss_workspace_bytes(n); }

extern "C" int tribe_mse_fwd(const float* pred, const float* truth, int64_t n, float* out, void* workspace, size_t workspace_bytes,
                             void* stream) {
  TRIBE_REQUIRE(pred && truth && out && workspace, "tribe_mse_fwd: null pointer");
  TRIBE_REQUIRE(n > 0, "tribe_mse_fwd: empty input");
  TRIBE_REQUIRE(workspace_bytes >= tribe_mse_workspace_bytes(n), "tribe_mse_fwd: workspace too small");
  TRIBE_REQUIRE(((uintptr_t)pred % 16) == 0 && ((uintptr_t)truth % 16) == 0, "tribe_mse_fwd: inputs must be 16-byte aligned");
  return launch_fwd(Plan{K_MSE, 0.f, 1.0, (double)n}, pred, truth, n, out, workspace, stream);
}

extern "C" int tribe_mse_bwd(const float* pred, const float* truth, int64_t n, const float* gscale, float* dpred, void* stream) {
  TRIBE_REQUIRE(pred && truth && gscale && dpred && n > 0, "tribe_mse_bwd: bad argument");
  return launch_bwd(Plan{K_MSE, 0.f, 1.0, (double)n}, pred, truth, n, gscale, dpred, stream);
}
