// Streaming per-(group, voxel) statistics on [B, V, T'] predictions and targets: the one skeleton behind the Pearson moments (loss.hip)
// and the regression residual sums (regression_metrics.hip).  The state is f64 [G, V, 6] = {five sums, n}; what the five sums are is the
// accumulator's business:
//   struct Acc {
//     static __device__ __forceinline__ void one(double (&s)[5], const float* x, const float* y, int64_t o);   // the sample pred x[o], truth y[o]
//     static __device__ __forceinline__ void quad(double (&s)[5], const float4& a, const float4& c);        // one float4 pair
//   };
#pragma once
#include "common.h"

namespace {

// Strided fallback (any st): one workgroup per voxel v; for each row b: 5 sums over t, added into dst[g(b)][v][0..5]
template <class Acc>
__global__ __launch_bounds__(256) void bvt_stats_strided_kernel(const float* __restrict__ pred, const float* __restrict__ truth, int64_t B,
                                                                int64_t V, int64_t T, int64_t sb, int64_t sv, int64_t st,
                                                                const int64_t* __restrict__ group, int64_t n_groups,
                                                                double* __restrict__ stats) {
  __shared__ double sh[4];
  const int64_t v = blockIdx.x;
  for (int64_t b = 0; b < B; ++b) {
    const float* x = pred + b * sb + v * sv;
    const float* y = truth + b * sb + v * sv;
    double s[5] = {0, 0, 0, 0, 0};
    for (int64_t t = threadIdx.x; t < T; t += blockDim.x) Acc::one(s, x, y, t * st);
    double r[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) r[k] = block_sum_d(s[k], sh);
    if (threadIdx.x == 0) {
      int64_t g = group ? group[b] : 0;
      if (g >= 0 && g < n_groups) {
        double* dst = stats + (g * V + v) * 6;
#pragma unroll
        for (int k = 0; k < 5; ++k) dst[k] += r[k];
        dst[5] += (double)T;
      }
    }
  }
}

// Contiguous rows (st == 1, 16-byte aligned, T % 4 == 0) -- the layout the voxel head writes.  HBM-bound: 8 bytes read per
// (row, voxel, t).  Workgroup (v, chunk) owns voxel v of `rows_per_wg` consecutive sequences; each of its four waves walks
// whole rows (T contiguous floats per tensor: float4 per lane, two rows-worth of requests in flight) and keeps the five f64
// sums IN REGISTERS across rows of the same group; only a change of group (grouped metric: one state per subject,
// metrics/base.py) or the end of the chunk costs a wave reduction and six vector f64 atomics.  No LDS, no barrier.
__device__ __forceinline__ void bvt_stats_flush(double (&s)[5], double cnt, double* __restrict__ dst) {
#pragma unroll
  for (int k = 0; k < 5; ++k) s[k] = wave_sum_d(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 5; ++k) unsafeAtomicAdd(dst + k, s[k]);
    unsafeAtomicAdd(dst + 5, cnt);
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) s[k] = 0.0;
}

template <class Acc>
__global__ __launch_bounds__(256) void bvt_stats_rows_kernel(const float* __restrict__ pred, const float* __restrict__ truth, int64_t B,
                                                             int64_t V, int64_t T, int64_t sb, int64_t sv,
                                                             const int64_t* __restrict__ group, int64_t n_groups, int64_t rows_per_wg,
                                                             double* __restrict__ stats) {
  const int64_t v = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b0 = (int64_t)blockIdx.y * rows_per_wg;
  const int64_t b1 = (b0 + rows_per_wg < B) ? b0 + rows_per_wg : B;
  const int64_t T4 = T >> 2;
  double s[5] = {0, 0, 0, 0, 0};
  double cnt = 0.0;
  int64_t g_cur = -1;
  for (int64_t b = b0 + wave; b < b1; b += 4) {
    int64_t g = group ? group[b] : 0;
    if (g < 0 || g >= n_groups) continue;                       // rows of an unknown group are skipped
    if (g != g_cur) {
      if (g_cur >= 0) bvt_stats_flush(s, cnt, stats + (g_cur * V + v) * 6);
      g_cur = g;
      cnt = 0.0;
    }
    const float4* x = (const float4*)(pred + b * sb + v * sv);
    const float4* y = (const float4*)(truth + b * sb + v * sv);
    int64_t i = lane;
    for (; i + 192 < T4; i += 256) {                            // four float4 pairs requested before the first is used
      float4 a[4], c[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { a[u] = load_nt_f4(x + i + 64 * u); c[u] = load_nt_f4(y + i + 64 * u); }
#pragma unroll
      for (int u = 0; u < 4; ++u) Acc::quad(s, a[u], c[u]);
    }
    for (; i < T4; i += 64) {
      const float4 a = load_nt_f4(x + i), c = load_nt_f4(y + i);
      Acc::quad(s, a, c);
    }
    cnt += (double)T;
  }
  if (g_cur >= 0) bvt_stats_flush(s, cnt, stats + (g_cur * V + v) * 6);
}

// Rows branch: st == 1, T % 4 == 0, sb % 4 == 0, sv % 4 == 0, both tensors 16-byte aligned and V <= 0x7fffffff; anything else strided
template <class Acc>
static void launch_bvt_stats(const float* pred, const float* truth, int64_t B, int64_t V, int64_t T, int64_t sb, int64_t sv, int64_t st,
                             const int64_t* group, int64_t n_groups, double* stats, hipStream_t s) {
  const bool rows = st == 1 && T % 4 == 0 && sb % 4 == 0 && sv % 4 == 0 && ((uintptr_t)pred % 16) == 0 && ((uintptr_t)truth % 16) == 0 &&
                    V <= 0x7fffffff;
  if (!rows) {
    hipLaunchKernelGGL(bvt_stats_strided_kernel<Acc>, dim3((unsigned)V), dim3(256), 0, s, pred, truth, B, V, T, sb, sv, st, group, n_groups,
                       stats);
    return;
  }
  // >= ~4096 workgroups when the batch allows it (256 CUs x 8 resident), at least 4 rows (one per wave) per workgroup
  int64_t chunks = (4096 + V - 1) / V;
  const int64_t max_chunks = (B + 3) / 4;
  if (chunks > max_chunks) chunks = max_chunks;
  if (chunks < 1) chunks = 1;
  if (chunks > 65535) chunks = 65535;
  const int64_t rows_per_wg = (B + chunks - 1) / chunks;
  chunks = (B + rows_per_wg - 1) / rows_per_wg;
  hipLaunchKernelGGL(bvt_stats_rows_kernel<Acc>, dim3((unsigned)V, (unsigned)chunks), dim3(256), 0, s, pred, truth, B, V, T, sb, sv, group,
                     n_groups, rows_per_wg, stats);
}

// The argument check of every entry point that launches the pair: 0, or -1 with the error set under the entry point's name
static int check_bvt_stats_args(const char* name, const float* pred, const float* truth, const double* stats, int64_t B, int64_t V,
                                int64_t T, int64_t n_groups) {
  TRIBE_REQUIRE(pred && truth && stats, "%s: null pointer", name);
  TRIBE_REQUIRE(B > 0 && V > 0 && T > 0 && n_groups > 0, "%s: bad shape B=%lld V=%lld T=%lld groups=%lld", name, (long long)B,
                (long long)V, (long long)T, (long long)n_groups);
  TRIBE_REQUIRE(V <= 0x7fffffff, "%s: V=%lld exceeds the grid", name, (long long)V);
  return 0;
}

}  // namespace
