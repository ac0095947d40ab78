// Streaming regression metrics (MSE / RMSE / MAE / R2 / explained variance) on [B, V, T'] predictions and targets, per (group, voxel).
// The state is f64 [G, V, 6] = {sum d, sum d^2, sum |d|, sum t, sum t^2, n} with d = t - p formed in f64 from the widened f32 values:
// the residual sums are taken directly.  The Pearson moments {Sx, Sy, Sxx, Syy, Sxy} cannot serve here: sum |d| has no expression in
// moments, and sum d^2 = Sxx - 2 Sxy + Syy cancels when the prediction follows the target on an offset (t = 1e3 + N(0, 1),
// p = t + 1e-3 N(0, 1): the moment form loses 1e-4 .. 1e-2 of the residual sum, the direct sum stays within n ulps).
// Addressing, grouping and launch branches are the shared kernel pair of bvt_stats.h, which the Pearson statistics of loss.hip use too;
// this file supplies the accumulator and the finalisers.  HBM-bound at 8 bytes read per element.
#include "bvt_stats.h"

namespace {

// {sum d, sum d^2, sum |d|, sum t, sum t^2} of bvt_stats.h's [G, V, 6] state (x = prediction, y = target, d = y - x)
struct RegressionAcc {
  static __device__ __forceinline__ void one(double (&s)[5], const float* x, const float* y, int64_t o) {
    const double c = (double)y[o], d = c - (double)x[o];
    s[0] += d; s[1] = fma(d, d, s[1]); s[2] += fabs(d); s[3] += c; s[4] = fma(c, c, s[4]);
  }
  static __device__ __forceinline__ void quad(double (&s)[5], const float4& a, const float4& c) {
    // a = prediction, c = target.  The f32 squares are exact in f64 after widening; d rounds once, d^2 only inside the fma
    const double cx = c.x, cy = c.y, cz = c.z, cw = c.w;
    const double dx = cx - (double)a.x, dy = cy - (double)a.y, dz = cz - (double)a.z, dw = cw - (double)a.w;
    s[0] += (dx + dy) + (dz + dw);
    s[1] = fma(dx, dx, fma(dy, dy, fma(dz, dz, fma(dw, dw, s[1]))));
    s[2] += (fabs(dx) + fabs(dy)) + (fabs(dz) + fabs(dw));
    s[3] += (cx + cy) + (cz + cw);
    s[4] = fma(cx, cx, fma(cy, cy, fma(cz, cz, fma(cw, cw, s[4]))));
  }
};

// One voxel's score in f64 (scikit-learn's force_finite=True conventions).  tss and the residual variance use the Pearson finaliser's
// rule: a centred sum of squares within n ulps of its raw sum of squares counts as 0.
struct regression_terms {
  double n, rss, sad, tss, vres;
};

__device__ __forceinline__ regression_terms regression_load(const double* __restrict__ s) {
  regression_terms q;
  q.n = s[5];
  q.rss = s[1];
  q.sad = s[2];
  q.tss = onepass_centred_ss(s[3], s[4], q.n);
  q.vres = onepass_centred_ss(s[0], s[1], q.n);
  return q;
}

__device__ __forceinline__ double regression_score(const regression_terms& q, int kind) {
  const double nan = __builtin_nan("");
  if (!(q.n > 0.0)) return nan;
  switch (kind) {
    case TRIBE_REGRESSION_MSE: return q.rss / q.n;
    case TRIBE_REGRESSION_RMSE: return sqrt(q.rss / q.n);
    case TRIBE_REGRESSION_MAE: return q.sad / q.n;
    case TRIBE_REGRESSION_R2:
      if (q.n < 2.0) return nan;
      if (q.tss == 0.0) return q.rss == 0.0 ? 1.0 : 0.0;
      return 1.0 - q.rss / q.tss;
    default:  // TRIBE_REGRESSION_EXPLAINED_VARIANCE
      if (q.tss == 0.0) return q.vres == 0.0 ? 1.0 : 0.0;
      return 1.0 - q.vres / q.tss;
  }
}

__global__ void regression_from_stats_kernel(const double* __restrict__ stats, int64_t n, int kind, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = (float)regression_score(regression_load(stats + i * 6), kind);
}

// One workgroup per group; every lane walks its voxels in order and block_sum_d adds the lanes in a fixed order: equal stats give
// equal bits.
__global__ __launch_bounds__(256) void regression_reduce_kernel(const double* __restrict__ stats, int64_t V, int kind, int mode,
                                                                double* __restrict__ out) {
  __shared__ double sh[4];
  const double* gs = stats + (int64_t)blockIdx.x * V * 6;
  double a = 0.0, b = 0.0, c = 0.0;
  for (int64_t v = threadIdx.x; v < V; v += blockDim.x) {
    const regression_terms q = regression_load(gs + v * 6);
    if (mode == TRIBE_REGRESSION_POOLED) {
      a += kind == TRIBE_REGRESSION_MAE ? q.sad : q.rss;
      b += q.n;
    } else {
      const double sc = regression_score(q, kind);
      a += sc;
      b += q.tss;
      c += q.tss * sc;
    }
  }
  a = block_sum_d(a, sh);
  b = block_sum_d(b, sh);
  c = block_sum_d(c, sh);
  if (threadIdx.x != 0) return;
  double r;
  if (mode == TRIBE_REGRESSION_POOLED) {
    r = b > 0.0 ? a / b : __builtin_nan("");
    if (kind == TRIBE_REGRESSION_RMSE) r = sqrt(r);
  } else if (mode == TRIBE_REGRESSION_VARIANCE_WEIGHTED && b != 0.0) {   // every tss 0: the uniform average (as scikit-learn)
    r = c / b;
  } else {
    r = a / (double)V;
  }
  out[blockIdx.x] = r;
}

}  // namespace

extern "C" int tribe_regression_stats_update(const float* pred, const float* truth, int64_t B, int64_t V, int64_t T, int64_t sb,
                                             int64_t sv, int64_t st, const int64_t* group, int64_t n_groups, double* stats,
                                             void* stream) {
  if (check_bvt_stats_args("tribe_regression_stats_update", pred, truth, stats, B, V, T, n_groups)) return -1;
  launch_bvt_stats<RegressionAcc>(pred, truth, B, V, T, sb, sv, st, group, n_groups, stats, (hipStream_t)stream);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_regression_from_stats(const double* stats, int64_t n_groups, int64_t V, int32_t kind, float* out, void* stream) {
  TRIBE_REQUIRE(stats && out, "tribe_regression_from_stats: null pointer");
  TRIBE_REQUIRE(n_groups > 0 && V > 0, "tribe_regression_from_stats: bad shape");
  TRIBE_REQUIRE(kind >= TRIBE_REGRESSION_MSE && kind <= TRIBE_REGRESSION_EXPLAINED_VARIANCE, "tribe_regression_from_stats: unknown kind %d",
                (int)kind);
  const int64_t n = n_groups * V;
  TRIBE_REQUIRE((n + 255) / 256 <= 0x7fffffff, "tribe_regression_from_stats: %lld outputs exceed the grid", (long long)n);
  hipLaunchKernelGGL(regression_from_stats_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, stats, n, (int)kind,
                     out);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_regression_reduce(const double* stats, int64_t n_groups, int64_t V, int32_t kind, int32_t mode, double* out,
                                       void* stream) {
  TRIBE_REQUIRE(stats && out, "tribe_regression_reduce: null pointer");
  TRIBE_REQUIRE(n_groups > 0 && n_groups <= 0x7fffffff && V > 0, "tribe_regression_reduce: bad shape");
  TRIBE_REQUIRE(kind >= TRIBE_REGRESSION_MSE && kind <= TRIBE_REGRESSION_EXPLAINED_VARIANCE, "tribe_regression_reduce: unknown kind %d",
                (int)kind);
  TRIBE_REQUIRE(mode >= TRIBE_REGRESSION_POOLED && mode <= TRIBE_REGRESSION_VARIANCE_WEIGHTED, "tribe_regression_reduce: unknown mode %d",
                (int)mode);
  TRIBE_REQUIRE(mode != TRIBE_REGRESSION_POOLED || kind <= TRIBE_REGRESSION_MAE,
                "tribe_regression_reduce: 'pooled' is defined for mse, rmse and mae only");
  hipLaunchKernelGGL(regression_reduce_kernel, dim3((unsigned)n_groups), dim3(256), 0, (hipStream_t)stream, stats, V, (int)kind, (int)mode,
                     out);
  TRIBE_LAUNCH_CHECK();
  return 0;
}
