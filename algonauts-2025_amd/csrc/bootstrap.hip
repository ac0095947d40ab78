// Block bootstrap of the per-parcel Pearson r (modeling_utils/metrics/bootstrap.py: BootstrapPearsonCorrCoef): the resampling unit
// is a block (one batch row = one stimulus segment) whose f64 statistics {Sx, Sy, Sxx, Syy, Sxy, n} per parcel are already kept
// (bvt_stats.h), so a replicate is a weighted sum of block statistics followed by the finaliser of pearson_from_stats_kernel.
//
//   counts  : draw k (0 <= k < n_sel) of replicate r is word k & 3 of Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl
//             constants 0x9E3779B9 / 0xBB67AE85) with counter (k >> 2, r, 0, 0) and key (seed & 0xffffffff, seed >> 32); the drawn
//             index is (u * n_sel) >> 32 (64-bit product; not rejection-corrected: an index is over-represented by less than
//             n_sel / 2^32 < 8e-6).  The draw depends on (seed, r, k, n_sel) alone.  One workgroup per replicate histograms its
//             draws in LDS (integer adds: any order gives the same counts) and writes int32 counts[n_boot][n_sel].
//   pearson : S[r][v][0..6) = sum_j counts[r][j] * stats[blocks[j]][v][0..6), one f64 fma chain per sum with j ascending, then
//             the finaliser.  Row n_boot takes every count as 1: the observed r, from the same code.  The [n_boot, V, 6] sums are
//             never written: a workgroup owns 32 replicates x 64 parcels, a lane 4 x 2 of them (48 f64 accumulators in registers),
//             and 8 blocks at a time are staged through LDS (statistics as [block][sum][parcel], so a wave reads consecutive f64;
//             counts as f64 [block][replicate], read as broadcasts); the next stage's global loads are in flight while the current
//             one is consumed.  Vector f64 FMA, no MFMA.  A block with count 0 still enters
//             every chain as fma(0, s, acc): a non-finite statistic makes every replicate of its parcel NaN, drawn or not.
//             A second kernel takes the mean over parcels of every row: the f32 results summed in f64 in a fixed order (lane-
//             strided, shuffle tree, waves in order), rounded once; NaN as soon as one parcel is NaN.
//   summary : one workgroup per column of a replicate table f32 [n][C]: the column's keys (lds_sort.h; NaN -> RC_PAD, so NaNs and
//             the padding land last) are sorted in LDS; m = #non-NaN.  Quantiles by numpy's "linear" rule over the m valid values
//             (h = (m - 1) q, i = floor(h), s[i] + (h - i) (s[min(i + 1, m - 1)] - s[i]) in f64, rounded once), the standard
//             deviation (ddof = 1, two passes in f64 over the sorted values, NaN for m < 2), and the integer counts #{x <= 0},
//             #{x >= 0}, m.  -0.0 sorts and reads back as +0.0.
//
// No floating-point atomics anywhere: equal inputs give equal bits.
#include "common.h"
#include "lds_sort.h"
#include "philox.h"

namespace {

constexpr int BS_MAX_SEL = 32768;     // int32 histogram of one replicate: 128 KiB of the 160 KiB LDS
constexpr int BS_MAX_BOOT = 16384;    // one column of replicates as u32 keys: 64 KiB of LDS
constexpr int BS_MAX_Q = 1024;
constexpr int BP_R = 32;              // replicates per workgroup
constexpr int BP_V = 64;              // parcels per workgroup
constexpr int BP_J = 8;               // blocks per LDS stage
constexpr int BS_LANES = 1024;

// grid n_boot, dynamic LDS: n_sel int32
__global__ __launch_bounds__(256) void bootstrap_counts_kernel(unsigned k0, unsigned k1, int n_sel, int* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) int hist[];
  const int tid = threadIdx.x;
  const unsigned r = blockIdx.x;
  for (int i = tid; i < n_sel; i += 256) hist[i] = 0;
  __syncthreads();
  const int quads = (n_sel + 3) >> 2;
  for (int q = tid; q < quads; q += 256) {
    const uint4 o = philox4x32_10(make_uint4((unsigned)q, r, 0u, 0u), k0, k1);
    const unsigned u[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
    for (int w = 0; w < 4; ++w)
      if (4 * q + w < n_sel) atomicAdd(&hist[(int)(((unsigned long long)u[w] * (unsigned)n_sel) >> 32)], 1);   // index < n_sel: u < 2^32
  }
  __syncthreads();
  int* dst = counts + (int64_t)r * n_sel;
  for (int i = tid; i < n_sel; i += 256) dst[i] = hist[i];
}

// the rule of pearson_from_stats_kernel (loss.hip)
__device__ __forceinline__ float pearson_of(const double (&s)[6]) {
  const double cnt = s[5];
  const double vx = onepass_centred_ss(s[0], s[2], cnt), vy = onepass_centred_ss(s[1], s[3], cnt);
  if (!(cnt >= 2.0) || vx == 0.0 || vy == 0.0) return __builtin_nanf("");   // n < 2, a constant column (or NaN statistics)
  const double cov = s[4] - s[0] * s[1] / cnt;
  double v = cov / sqrt(vx * vy);
  if (v > 1.0) v = 1.0;
  if (v < -1.0) v = -1.0;
  return (float)v;
}

constexpr int BP_LOADS = BP_J * BP_V * 6 / 256;   // statistics a lane stages per LDS stage
constexpr int BP_LD = BP_V + 12;                  // row stride of the staged statistics: spreads the six sums of a parcel over the banks

// The part of stage j0 that lane `tid` stages: BP_LOADS statistics (a block's tile is 384 consecutive f64 of its row) and one count.
__device__ __forceinline__ void bootstrap_stage_load(const double* __restrict__ stats, int64_t n_blocks, int64_t V, const int64_t* __restrict__ blocks,
                                                     int n_sel, const int* __restrict__ counts, int n_boot, int64_t v0, int r0, int j0, int tid,
                                                     double (&xs)[BP_LOADS], double& c) {
#pragma unroll
  for (int i = 0; i < BP_LOADS; ++i) {
    const int e = tid + 256 * i;
    const int jj = e / (BP_V * 6), rem = e % (BP_V * 6);
    const int j = j0 + jj;
    const int64_t v = v0 + rem / 6;
    double x = 0.0;   // beyond the data: adds nothing
    if (j < n_sel && v < V) {
      const int64_t b = blocks[j];
      x = (b >= 0 && b < n_blocks) ? stats[(b * V + v0) * 6 + rem] : __builtin_nan("");   // a block index outside the state shows as NaN
    }
    xs[i] = x;
  }
  const int j = j0 + (tid & (BP_J - 1)), r = r0 + (tid >> 3);   // BP_J * BP_R == 256 lanes
  c = 0.0;
  if (j < n_sel) {
    if (r < n_boot) c = (double)counts[(int64_t)r * n_sel + j];
    else if (r == n_boot) c = 1.0;
  }
}

// grid (ceil(V / BP_V), ceil((n_boot + 1) / BP_R)), 256 lanes.  Lane (tr = tid >> 5, tv = tid & 31) owns the replicates
// r0 + 4 tr + {0..3} and the parcels v0 + tv + {0, 32}.  r_out: f32 [n_boot + 1][ld], row n_boot = the observed r.
// The loads of stage s + 1 are issued into registers before stage s is consumed from LDS, so their latency hides under its FMAs.
__global__ __launch_bounds__(256) void bootstrap_pearson_kernel(const double* __restrict__ stats, int64_t n_blocks, int64_t V,
                                                                const int64_t* __restrict__ blocks, int n_sel, const int* __restrict__ counts,
                                                                int n_boot, float* __restrict__ r_out, int64_t ld) {
  __shared__ double sS[BP_J][6][BP_LD];
  __shared__ __attribute__((aligned(16))) double sC[BP_J][BP_R];
  const int tid = threadIdx.x, tv = tid & 31, tr = tid >> 5;
  const int64_t v0 = (int64_t)blockIdx.x * BP_V;
  const int r0 = (int)blockIdx.y * BP_R;
  double acc[4][2][6];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int q = 0; q < 6; ++q) acc[a][b][q] = 0.0;
  double xs[BP_LOADS], cs;
  bootstrap_stage_load(stats, n_blocks, V, blocks, n_sel, counts, n_boot, v0, r0, 0, tid, xs, cs);
  for (int j0 = 0; j0 < n_sel; j0 += BP_J) {
    __syncthreads();   // the previous stage is consumed
#pragma unroll
    for (int i = 0; i < BP_LOADS; ++i) {
      const int e = tid + 256 * i;
      const int jj = e / (BP_V * 6), rem = e % (BP_V * 6);
      sS[jj][rem % 6][rem / 6] = xs[i];
    }
    sC[tid & (BP_J - 1)][tid >> 3] = cs;
    __syncthreads();
    if (j0 + BP_J < n_sel) bootstrap_stage_load(stats, n_blocks, V, blocks, n_sel, counts, n_boot, v0, r0, j0 + BP_J, tid, xs, cs);
#pragma unroll 4
    for (int jj = 0; jj < BP_J; ++jj) {
      double c[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) c[a] = sC[jj][tr * 4 + a];
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          const double s = sS[jj][q][tv + 32 * b];
#pragma unroll
          for (int a = 0; a < 4; ++a) acc[a][b][q] = fma(c[a], s, acc[a][b][q]);
        }
    }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int r = r0 + tr * 4 + a;
      const int64_t v = v0 + tv + 32 * b;
      if (r <= n_boot && v < V) r_out[(int64_t)r * ld + v] = pearson_of(acc[a][b]);
    }
}

// grid rows, 256 lanes: mean[row * mean_stride] = the mean of r[row][0..V)
__global__ __launch_bounds__(256) void bootstrap_row_mean_kernel(const float* __restrict__ r, int64_t V, int64_t ld, float* __restrict__ mean,
                                                                 int64_t mean_stride) {
  __shared__ double sh[4];
  const int64_t row = blockIdx.x;
  double s = 0.0;
  for (int64_t v = threadIdx.x; v < V; v += 256) s += (double)r[row * ld + v];
  const double tot = block_sum_d(s, sh);
  if (threadIdx.x == 0) mean[row * mean_stride] = (float)(tot / (double)V);
}

// grid C, BS_LANES lanes, dynamic LDS: P u32 (P: a power of two >= max(n, 64))
__global__ __launch_bounds__(BS_LANES) void bootstrap_summary_kernel(const float* __restrict__ x, int n, int64_t ld, int P,
                                                                     const double* __restrict__ quant, int n_q, int64_t C,
                                                                     float* __restrict__ qv, float* __restrict__ sd, int* __restrict__ n_le,
                                                                     int* __restrict__ n_ge, int* __restrict__ n_valid) {
  extern __shared__ __attribute__((aligned(16))) unsigned keys[];
  __shared__ double sh[BS_LANES / 64];
  __shared__ int cnt[3];
  const int tid = threadIdx.x;
  const int64_t col = blockIdx.x;
  if (tid < 3) cnt[tid] = 0;
  __syncthreads();
  int valid = 0, le = 0, ge = 0;
  for (int i = tid; i < P; i += BS_LANES) {
    unsigned k = RC_PAD;
    if (i < n) {
      const float v = x[(int64_t)i * ld + col];
      if (v == v) {
        k = key_of(v);
        valid += 1;
        le += v <= 0.0f ? 1 : 0;
        ge += v >= 0.0f ? 1 : 0;
      }
    }
    keys[i] = k;
  }
  if (valid) {   // integer adds: any order
    atomicAdd(&cnt[0], valid);
    atomicAdd(&cnt[1], le);
    atomicAdd(&cnt[2], ge);
  }
  __syncthreads();
  const int m = cnt[0];
  block_sort(keys, nullptr, P);
  double s = 0.0;
  for (int i = tid; i < m; i += BS_LANES) s += (double)value_of(keys[i]);
  const double mean = block_sum_d(s, sh) / (double)m;
  double ss = 0.0;
  for (int i = tid; i < m; i += BS_LANES) {
    const double d = (double)value_of(keys[i]) - mean;
    ss = fma(d, d, ss);
  }
  const double tot = block_sum_d(ss, sh);
  if (tid == 0) {
    sd[col] = m < 2 ? __builtin_nanf("") : (float)sqrt(tot / (double)(m - 1));
    n_le[col] = cnt[1];
    n_ge[col] = cnt[2];
    n_valid[col] = m;
  }
  for (int k = tid; k < n_q; k += BS_LANES) {
    float out = __builtin_nanf("");
    if (m > 0) {
      const double h = (double)(m - 1) * quant[k];
      int i = (int)floor(h);
      if (i < 0) i = 0;
      if (i > m - 1) i = m - 1;
      const int i1 = i + 1 < m ? i + 1 : m - 1;
      const double lo = (double)value_of(keys[i]), hi = (double)value_of(keys[i1]);
      out = (float)(lo + (h - (double)i) * (hi - lo));
    }
    qv[(int64_t)k * C + col] = out;
  }
}

}  // namespace

extern "C" int tribe_bootstrap_counts(uint64_t seed, int64_t n_boot, int64_t n_sel, int32_t* counts, void* stream) {
  TRIBE_REQUIRE(counts, "tribe_bootstrap_counts: null pointer");
  TRIBE_REQUIRE(n_boot >= 1 && n_boot <= BS_MAX_BOOT, "tribe_bootstrap_counts: n_boot=%lld outside [1, %d]", (long long)n_boot, BS_MAX_BOOT);
  TRIBE_REQUIRE(n_sel >= 1 && n_sel <= BS_MAX_SEL, "tribe_bootstrap_counts: n_sel=%lld outside [1, %d] (one replicate's histogram lives in LDS)",
                (long long)n_sel, BS_MAX_SEL);
  const size_t smem = (size_t)n_sel * sizeof(int);
  if (smem > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)bootstrap_counts_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, BS_MAX_SEL * (int)sizeof(int));
  hipLaunchKernelGGL(bootstrap_counts_kernel, dim3((unsigned)n_boot), dim3(256), smem, (hipStream_t)stream, (unsigned)(seed & 0xffffffffu),
                     (unsigned)(seed >> 32), (int)n_sel, (int*)counts);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_bootstrap_pearson(const double* stats, int64_t n_blocks, int64_t V, const int64_t* blocks, int64_t n_sel,
                                       const int32_t* counts, int64_t n_boot, float* r, int64_t ld, float* mean, int64_t mean_stride,
                                       void* stream) {
  TRIBE_REQUIRE(stats && blocks && r && mean, "tribe_bootstrap_pearson: null pointer");
  TRIBE_REQUIRE(n_boot >= 0 && n_boot <= BS_MAX_BOOT, "tribe_bootstrap_pearson: n_boot=%lld outside [0, %d]", (long long)n_boot, BS_MAX_BOOT);
  TRIBE_REQUIRE(counts || n_boot == 0, "tribe_bootstrap_pearson: null counts with n_boot=%lld", (long long)n_boot);
  TRIBE_REQUIRE(n_blocks >= 1 && V >= 1 && ld >= V && mean_stride >= 1, "tribe_bootstrap_pearson: bad shape n_blocks=%lld V=%lld ld=%lld mean_stride=%lld",
                (long long)n_blocks, (long long)V, (long long)ld, (long long)mean_stride);
  TRIBE_REQUIRE(n_sel >= 1 && n_sel <= BS_MAX_SEL, "tribe_bootstrap_pearson: n_sel=%lld outside [1, %d]", (long long)n_sel, BS_MAX_SEL);
  const int64_t vt = (V + BP_V - 1) / BP_V, rt = (n_boot + 1 + BP_R - 1) / BP_R;
  TRIBE_REQUIRE(vt <= 0x7fffffff, "tribe_bootstrap_pearson: V=%lld exceeds the grid", (long long)V);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(bootstrap_pearson_kernel, dim3((unsigned)vt, (unsigned)rt), dim3(256), 0, s, stats, n_blocks, V, blocks, (int)n_sel,
                     (const int*)counts, (int)n_boot, r, ld);
  TRIBE_LAUNCH_CHECK();
  hipLaunchKernelGGL(bootstrap_row_mean_kernel, dim3((unsigned)(n_boot + 1)), dim3(256), 0, s, (const float*)r, V, ld, mean, mean_stride);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_bootstrap_summary(const float* replicates, int64_t n, int64_t C, int64_t ld, const double* quantiles, int64_t n_q,
                                       float* quantile_values, float* std, int32_t* n_le, int32_t* n_ge, int32_t* n_valid, void* stream) {
  TRIBE_REQUIRE(replicates && quantiles && quantile_values && std && n_le && n_ge && n_valid, "tribe_bootstrap_summary: null pointer");
  TRIBE_REQUIRE(n >= 1 && n <= BS_MAX_BOOT, "tribe_bootstrap_summary: n=%lld replicates outside [1, %d] (a column is sorted in LDS)", (long long)n,
                BS_MAX_BOOT);
  TRIBE_REQUIRE(C >= 1 && C <= 0x7fffffff && ld >= C, "tribe_bootstrap_summary: bad shape C=%lld ld=%lld", (long long)C, (long long)ld);
  TRIBE_REQUIRE(n_q >= 1 && n_q <= BS_MAX_Q, "tribe_bootstrap_summary: n_q=%lld quantiles outside [1, %d]", (long long)n_q, BS_MAX_Q);
  int P = 64;
  while (P < n) P <<= 1;
  if ((size_t)P * sizeof(unsigned) + 1024 > 64 * 1024)   // the keys and the kernel's static LDS together pass the default limit
    (void)hipFuncSetAttribute((const void*)bootstrap_summary_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, BS_MAX_BOOT * (int)sizeof(unsigned));
  hipLaunchKernelGGL(bootstrap_summary_kernel, dim3((unsigned)C), dim3(BS_LANES), (size_t)P * sizeof(unsigned), (hipStream_t)stream, replicates, (int)n,
                     ld, P, quantiles, (int)n_q, C, quantile_values, std, (int*)n_le, (int*)n_ge, (int*)n_valid);
  TRIBE_LAUNCH_CHECK();
  return 0;
}
