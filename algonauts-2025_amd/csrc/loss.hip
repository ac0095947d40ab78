// The Pearson statistics, metric and loss on [B, V, T'] predictions and targets (T' contiguous); the element-wise losses, the
// default MSE among them, are in robust_loss.hip.
// pl_module.py:54-56 flattens to [(B T'), V] before the loss; every reduction here is
// a per-voxel (or global) sum, so the flatten is never materialised: a workgroup owns
// one voxel of a run of sequences and its waves walk whole rows of T' contiguous floats
// (coalesced float4 streams, HBM-bound: 2 * B*V*T' * 4 bytes per call, the roofline
// these kernels are measured against in scripts/loss_bench.py).  Sums are carried in f64
// so that the cov = Sxy - Sx*Sy/n form stays exact to f32 output precision.
#include "bvt_stats.h"

namespace {

// The five Pearson moments {Sx, Sy, Sxx, Syy, Sxy} of bvt_stats.h's [G, V, 6] state (x = prediction, y = target)
struct PearsonAcc {
  static __device__ __forceinline__ void one(double (&s)[5], const float* x, const float* y, int64_t o) {
    const double a = (double)x[o], c = (double)y[o];
    s[0] += a; s[1] += c; s[2] += a * a; s[3] += c * c; s[4] += a * c;
  }
  static __device__ __forceinline__ void quad(double (&s)[5], const float4& a, const float4& c) {
    // f32 products of one float4 pair are exact in f64 after widening; five f64 fma chains per lane
    const double ax = a.x, ay = a.y, az = a.z, aw = a.w, cx = c.x, cy = c.y, cz = c.z, cw = c.w;
    s[0] += (ax + ay) + (az + aw);
    s[1] += (cx + cy) + (cz + cw);
    s[2] = fma(ax, ax, fma(ay, ay, fma(az, az, fma(aw, aw, s[2]))));
    s[3] = fma(cx, cx, fma(cy, cy, fma(cz, cz, fma(cw, cw, s[3]))));
    s[4] = fma(ax, cx, fma(ay, cy, fma(az, cz, fma(aw, cw, s[4]))));
  }
};

__global__ void pearson_from_stats_kernel(const double* __restrict__ stats, int64_t n, float* __restrict__ r) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* s = stats + i * 6;
  const double cnt = s[5];
  const double vx = onepass_centred_ss(s[0], s[2], cnt), vy = onepass_centred_ss(s[1], s[3], cnt);
  // n < 2 or a constant column -> NaN, as scipy / torchmetrics give
  if (cnt < 2.0 || vx == 0.0 || vy == 0.0) { r[i] = __builtin_nanf(""); return; }
  const double cov = s[4] - s[0] * s[1] / cnt;
  double v = cov / sqrt(vx * vy);
  if (v > 1.0) v = 1.0;
  if (v < -1.0) v = -1.0;
  r[i] = (float)v;
}

// PearsonLoss (losses.py:17-42): per voxel 1 - cov / (sqrt(Sxx_c) * sqrt(Syy_c) + 1e-8), then mean | sum over voxels
__global__ __launch_bounds__(256) void pearson_loss_final_kernel(const double* __restrict__ stats, int64_t V, int reduction_sum,
                                                                 float* __restrict__ out) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (int64_t v = threadIdx.x; v < V; v += blockDim.x) {
    const double* s = stats + v * 6;
    const double cnt = s[5];
    const double vx = onepass_centred_ss(s[0], s[2], cnt), vy = onepass_centred_ss(s[1], s[3], cnt);
    // |cov| <= sqrt(vx vy): a column without variance has no covariance either (the reference's centred sums give exactly 0)
    const double cov = (vx > 0.0 && vy > 0.0) ? s[4] - s[0] * s[1] / cnt : 0.0;
    // the reference works in f32: mirror its rounding of the two square roots and of the eps add
    const float xs = sqrtf((float)vx), ys = sqrtf((float)vy);
    const float pcc = (float)cov / (xs * ys + 1e-8f);
    acc += (double)(1.0f - pcc);
  }
  const double tot = block_sum_d(acc, sh);
  if (threadIdx.x == 0) out[0] = (float)(reduction_sum ? tot : tot / (double)V);
}

}  // namespace

extern "C" int tribe_pearson_stats_update(const float* pred, const float* truth, int64_t B, int64_t V, int64_t T, int64_t sb,
                                          int64_t sv, int64_t st, const int64_t* group, int64_t n_groups, double* stats,
                                          void* stream) {
  if (check_bvt_stats_args("tribe_pearson_stats_update", pred, truth, stats, B, V, T, n_groups)) return -1;
  launch_bvt_stats<PearsonAcc>(pred, truth, B, V, T, sb, sv, st, group, n_groups, stats, (hipStream_t)stream);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_pearson_from_stats(const double* stats, int64_t n_groups, int64_t V, float* r, void* stream) {
  TRIBE_REQUIRE(stats && r, "tribe_pearson_from_stats: null pointer");
  TRIBE_REQUIRE(n_groups > 0 && V > 0, "tribe_pearson_from_stats: bad shape");
  const int64_t n = n_groups * V;
  hipLaunchKernelGGL(pearson_from_stats_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, stats, n, r);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t tribe_pearson_loss_workspace_bytes(int64_t V) { return (size_t)V * 6 * sizeof(double); }

extern "C" int tribe_pearson_loss_fwd(const float* pred, const float* truth, int64_t B, int64_t V, int64_t T, int64_t sb,
                                      int64_t sv, int64_t st, int32_t reduction_sum, float* out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(pred && truth && out && workspace, "tribe_pearson_loss_fwd: null pointer");
  TRIBE_REQUIRE(B > 0 && V > 0 && T > 0, "tribe_pearson_loss_fwd: bad shape");
  TRIBE_REQUIRE(V <= 0x7fffffff, "tribe_pearson_loss_fwd: V=%lld exceeds the grid", (long long)V);
  TRIBE_REQUIRE(workspace_bytes >= tribe_pearson_loss_workspace_bytes(V), "tribe_pearson_loss_fwd: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(workspace, 0, tribe_pearson_loss_workspace_bytes(V), s);
  if (e != hipSuccess) { tribe_set_error("tribe_pearson_loss_fwd: memset failed: %s", hipGetErrorString(e)); return (int)e; }
  launch_bvt_stats<PearsonAcc>(pred, truth, B, V, T, sb, sv, st, (const int64_t*)nullptr, (int64_t)1, (double*)workspace, s);
  hipLaunchKernelGGL(pearson_loss_final_kernel, dim3(1), dim3(256), 0, s, (const double*)workspace, V, (int)reduction_sum, out);
  TRIBE_LAUNCH_CHECK();
  return 0;
}
