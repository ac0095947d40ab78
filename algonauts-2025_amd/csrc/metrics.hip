// Retrieval metrics (metrics.py:66-218 of the reference: Rank / TopkAcc) on the GPU.
//
//   prep   : strided [N, V, T] f32 view -> row means over T ([N, V], contiguous) and / or the L2 norm of every mean row.  The
//            retrieval branch of _run_step (pl_module.py:98-99) time-averages predictions and targets; this reads them in place.
//   ranks  : s[n, m] = dot(x_n, y_m) * inv_y[m] (_compute_sim, norm_kind "y"), then per query the rank of its true gallery row
//            rank = (#{s > s_true} + #{s >= s_true} - 1) / 2, with the reference's NaN and `relative` rules.  The [N, M] score
//            matrix is never written: a workgroup owns 64 queries, walks the gallery in 64-row tiles (operands staged through LDS,
//            4 x 4 f32 FMA register tile per lane) and counts in registers.
//   scores : the materialised [N, M] matrix of _compute_sim for all four norm kinds (diagnostics, not hot).
//   reduce : ranks -> {mean, unbiased std, lower median, fraction < topk} in one workgroup (f64 sums, radix select on the f32
//            bit patterns for the median: ranks are >= 0, so bit order is value order).
//
// Every score is one sequential fmaf chain over v = 0 .. V-1 followed by one multiply with 1 / (1e-15 + ||y_m||).  The true score
// s[n, t(n)] is computed by the very same tile code (a tile whose gallery rows are the true rows t(q0 + j)), so it is bit-identical
// to the entry the gallery walk meets at m = t(n), and a query always counts itself in `ge`; exact ties (duplicated gallery rows)
// give the same half-integer ranks as the reference.  The scores kernel keeps the same chain, so its "y" scores equal the ones
// the ranks kernel compares.
#include "common.h"

namespace {

constexpr int RQ = 64;   // queries per workgroup
constexpr int RG = 64;   // gallery rows per tile
constexpr int RK = 32;   // v per LDS stage
constexpr int RPAD = RQ + 4;

__device__ __forceinline__ float inv_norm(float nrm) { return 1.0f / (1e-15f + nrm); }

// ---- prep ------------------------------------------------------------------------------------------------------------------
// grid (N, n_tensors), 1024 lanes.  Fast path (T' contiguous, 16-byte aligned rows, T % 4 == 0): sixteen lanes own one (n, v) row
// of T floats (float4 per lane) and each group keeps four rows' loads in flight (256 rows per workgroup); strided fallback: one lane
// per v, any strides.  Sums in f64 (the same order for every row), the mean is rounded once to f32, and the norm is taken of the
// rounded means (the values the ranks kernel will read).
constexpr int PREP_LANES = 1024;

__global__ __launch_bounds__(PREP_LANES) void retrieval_prep_kernel(const float* __restrict__ a, const float* __restrict__ b, int64_t V,
                                                                    int64_t T, int64_t sn, int64_t sv, int64_t st, int fast,
                                                                    float* __restrict__ a_mean, float* __restrict__ b_mean,
                                                                    float* __restrict__ a_norm, float* __restrict__ b_norm) {
  __shared__ double sh[PREP_LANES / 64];
  const int64_t n = blockIdx.x;
  const bool second = blockIdx.y == 1;
  const float* src = (second ? b : a) + n * sn;
  float* mean = second ? b_mean : a_mean;
  float* norm = second ? b_norm : a_norm;
  const double inv_t = 1.0 / (double)T;
  double sumsq = 0.0;
  if (fast) {
    constexpr int GROUPS = PREP_LANES / 16;
    const int grp = threadIdx.x >> 4, l16 = threadIdx.x & 15;
    const int64_t T4 = T >> 2;
    for (int64_t v0 = grp; v0 < V; v0 += 4 * GROUPS) {
      double s[4] = {0.0, 0.0, 0.0, 0.0};
      for (int64_t i = l16; i < T4; i += 16) {
        float4 q[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t v = v0 + u * GROUPS;
          q[u] = v < V ? load_nt_f4((const float4*)(src + v * sv) + i) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] += ((double)q[u].x + (double)q[u].y) + ((double)q[u].z + (double)q[u].w);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) s[u] += __shfl_xor(s[u], off, 64);
        const int64_t v = v0 + u * GROUPS;
        const float m = (float)(s[u] * inv_t);
        if (l16 == 0 && v < V) {
          if (mean) mean[n * V + v] = m;
          sumsq += (double)m * (double)m;
        }
      }
    }
  } else {
    for (int64_t v = threadIdx.x; v < V; v += blockDim.x) {
      const float* row = src + v * sv;
      double s = 0.0;
      for (int64_t t = 0; t < T; ++t) s += (double)row[t * st];
      const float m = (float)(s * inv_t);
      if (mean) mean[n * V + v] = m;
      sumsq += (double)m * (double)m;
    }
  }
  if (norm) {
    const double tot = block_sum_d(sumsq, sh);
    if (threadIdx.x == 0) norm[n] = (float)sqrt(tot);
  }
}

// ---- ranks -----------------------------------------------------------------------------------------------------------------
struct RanksSmem {
  float xs[RK][RPAD];   // v-major: xs[k][j] = x[q0 + j][v0 + k]
  float ys[RK][RPAD];
  float ts[RQ];         // true score of every query of the workgroup
  int tvalid[RQ];       // 0: the query's true index lies outside the gallery (rank NaN)
  int64_t grow[RG];     // gallery row of each tile row (-1: none)
};

// acc[i][j] = sum_v x[q0 + 4 tq + i][v] * y[grow[4 tg + j]][v] as ONE fmaf chain per entry in v order; rows outside the data read 0
// (fmaf(0, 0, acc) leaves acc unchanged up to the sign of a zero, so padding never changes a comparison).
__device__ __forceinline__ void tile_dot(const float* __restrict__ x, int64_t ldx, int64_t N, int64_t q0, const float* __restrict__ y,
                                         int64_t ldy, int64_t V, RanksSmem& sm, float (&acc)[4][4]) {
  const int tid = threadIdx.x, tq = tid >> 4, tg = tid & 15;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0f;
  for (int64_t v0 = 0; v0 < V; v0 += RK) {
    __syncthreads();   // previous stage consumed (and grow[] written before the first)
#pragma unroll
    for (int r = 0; r < (RQ * RK) / 256; ++r) {   // 8 elements per lane, runs of RK consecutive v per row (coalesced)
      const int e = tid + 256 * r;
      const int j = e / RK, k = e % RK;
      const int64_t v = v0 + k;
      const int64_t qn = q0 + j;
      const int64_t gm = sm.grow[j];
      sm.xs[k][j] = (qn < N && v < V) ? x[qn * ldx + v] : 0.0f;
      sm.ys[k][j] = (gm >= 0 && v < V) ? y[gm * ldy + v] : 0.0f;
    }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < RK; ++k) {
      const float4 a = *(const float4*)&sm.xs[k][tq * 4];
      const float4 c = *(const float4*)&sm.ys[k][tg * 4];
      const float av[4] = {a.x, a.y, a.z, a.w}, cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_fmaf(av[i], cv[j], acc[i][j]);
    }
  }
}

__global__ __launch_bounds__(256) void retrieval_ranks_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ y,
                                                              int64_t ldy, const float* __restrict__ y_norm, int64_t N, int64_t M,
                                                              int64_t V, const int64_t* __restrict__ true_idx, int relative,
                                                              float* __restrict__ ranks) {
  __shared__ RanksSmem sm;
  const int tid = threadIdx.x, tq = tid >> 4, tg = tid & 15;
  const int64_t q0 = (int64_t)blockIdx.x * RQ;
  float acc[4][4];

  // 1) true scores: a tile whose gallery row j is t(q0 + j); its diagonal is s[n, t(n)]
  if (tid < RG) {
    const int64_t n = q0 + tid;
    int64_t t = -1;
    if (n < N) t = true_idx ? true_idx[n] : n;
    sm.grow[tid] = (t >= 0 && t < M) ? t : -1;
  }
  tile_dot(x, ldx, N, q0, y, ldy, V, sm, acc);
  if (tq == tg) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = tq * 4 + i;
      const int64_t t = sm.grow[j];
      sm.ts[j] = t >= 0 ? acc[i][i] * inv_norm(y_norm[t]) : __builtin_nanf("");
      sm.tvalid[j] = t >= 0;
    }
  }
  __syncthreads();
  float ts[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) ts[i] = sm.ts[tq * 4 + i];

  // 2) walk the gallery: count s > s_true and s >= s_true in registers (comparisons with NaN are false)
  int gt[4] = {0, 0, 0, 0}, ge[4] = {0, 0, 0, 0};
  for (int64_t g0 = 0; g0 < M; g0 += RG) {
    __syncthreads();   // everyone is done reading grow[] of the previous tile
    if (tid < RG) sm.grow[tid] = (g0 + tid < M) ? g0 + tid : -1;
    tile_dot(x, ldx, N, q0, y, ldy, V, sm, acc);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t m = g0 + tg * 4 + j;
      if (m < M) {
        const float iv = inv_norm(y_norm[m]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float s = acc[i][j] * iv;
          gt[i] += s > ts[i] ? 1 : 0;
          ge[i] += s >= ts[i] ? 1 : 0;
        }
      }
    }
  }

  // 3) the 16 lanes of a query group are consecutive lanes of one wave: integer shuffle sums, then one lane writes the ranks
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
      gt[i] += __shfl_xor(gt[i], off, 64);
      ge[i] += __shfl_xor(ge[i], off, 64);
    }
  }
  if (tg == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = tq * 4 + i;
      const int64_t n = q0 + j;
      if (n >= N) continue;
      float r = (float)(gt[i] + ge[i] - 1) * 0.5f;
      if (r < 0.0f) r = (float)(N / 2);           // true score NaN: ge == -1
      if (relative) r = r / (float)M;
      ranks[n] = sm.tvalid[j] ? r : __builtin_nanf("");
    }
  }
}

// ---- scores (diagnostic) ----------------------------------------------------------------------------------------------------
// 16 x 16 lanes, one (n, m) per lane, the same sequential fmaf chain as tile_dot.  norm_kind: 0 none, 1 x, 2 y, 3 xy, with the
// reference's factors 1 / (eps + |x|), 1 / (eps + |y|), 1 / (eps + |x| |y|).
__global__ __launch_bounds__(256) void retrieval_scores_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ y,
                                                               int64_t ldy, int64_t N, int64_t M, int64_t V,
                                                               const float* __restrict__ x_norm, const float* __restrict__ y_norm,
                                                               int norm_kind, float* __restrict__ out) {
  const int64_t m = (int64_t)blockIdx.x * 16 + (threadIdx.x & 15);
  const int64_t n = (int64_t)blockIdx.y * 16 + (threadIdx.x >> 4);
  if (n >= N || m >= M) return;
  const float* xr = x + n * ldx;
  const float* yr = y + m * ldy;
  float acc = 0.0f;
  for (int64_t v = 0; v < V; ++v) acc = __builtin_fmaf(xr[v], yr[v], acc);
  float f = 1.0f;
  if (norm_kind == 1) f = inv_norm(x_norm[n]);
  else if (norm_kind == 2) f = inv_norm(y_norm[m]);
  else if (norm_kind == 3) f = 1.0f / (1e-15f + x_norm[n] * y_norm[m]);
  out[n * M + m] = norm_kind == 0 ? acc : acc * f;
}

// ---- reduce -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void rank_reduce_kernel(const float* __restrict__ r, int64_t n, float topk, float* __restrict__ out) {
  __shared__ double sh[16];
  __shared__ int hist[256];
  __shared__ unsigned int sel[2];   // prefix, remaining k
  const int tid = threadIdx.x;
  double s = 0.0, hit = 0.0;
  for (int64_t i = tid; i < n; i += blockDim.x) {
    const float v = r[i];
    s += (double)v;
    hit += v < topk ? 1.0 : 0.0;
  }
  // block sums (f64, fixed order)
  auto bsum = [&](double v) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((tid & 63) == 0) sh[tid >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
    return t;
  };
  const double mean = bsum(s) / (double)n;
  const double hits = bsum(hit);
  double ss = 0.0;
  for (int64_t i = tid; i < n; i += blockDim.x) {
    const double d = (double)r[i] - mean;
    ss += d * d;
  }
  const double var = bsum(ss) / (double)(n - 1);   // n == 1: 0 / 0 = NaN, as torch.std

  // lower median: the element of rank k = (n - 1) / 2 in sorted order, radix select 8 bits at a time from the top
  unsigned int prefix = 0, mask = 0;
  if (tid == 0) sel[1] = (unsigned int)((n - 1) / 2);
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = tid; i < 256; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    for (int64_t i = tid; i < n; i += blockDim.x) {
      const unsigned int bits = __float_as_uint(r[i]);
      if ((bits & mask) == prefix) atomicAdd(&hist[(bits >> shift) & 255u], 1);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned int k = sel[1], bin = 0;
      for (; bin < 255u; ++bin) {
        const unsigned int c = (unsigned int)hist[bin];
        if (k < c) break;
        k -= c;
      }
      sel[0] = prefix | (bin << shift);
      sel[1] = k;
    }
    __syncthreads();
    prefix = sel[0];
    mask |= 255u << shift;
    __syncthreads();
  }
  if (tid == 0) {
    out[0] = (float)mean;
    out[1] = (float)sqrt(var);
    out[2] = __uint_as_float(prefix);
    out[3] = (float)(hits / (double)n);
  }
}

}  // namespace

extern "C" int tribe_retrieval_prep(const float* x, const float* y, int64_t N, int64_t V, int64_t T, int64_t sn, int64_t sv, int64_t st,
                                    float* x_mean, float* y_mean, float* x_norm, float* y_norm, void* stream) {
  TRIBE_REQUIRE(x, "tribe_retrieval_prep: null input");
  TRIBE_REQUIRE(N > 0 && V > 0 && T > 0 && N <= 0x7fffffff, "tribe_retrieval_prep: bad shape N=%lld V=%lld T=%lld", (long long)N,
                (long long)V, (long long)T);
  TRIBE_REQUIRE(x_mean || x_norm || (y && (y_mean || y_norm)), "tribe_retrieval_prep: no output requested");
  const uintptr_t al = ((uintptr_t)x | (y ? (uintptr_t)y : 0)) % 16;
  const int fast = st == 1 && T % 4 == 0 && sn % 4 == 0 && sv % 4 == 0 && al == 0;
  hipLaunchKernelGGL(retrieval_prep_kernel, dim3((unsigned)N, y ? 2u : 1u), dim3(PREP_LANES), 0, (hipStream_t)stream, x, y ? y : x, V, T, sn, sv,
                     st, fast, x_mean, y ? y_mean : nullptr, x_norm, y ? y_norm : nullptr);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_retrieval_ranks(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* y_norm, int64_t N, int64_t M,
                                     int64_t V, const int64_t* true_idx, int32_t relative, float* ranks, void* stream) {
  TRIBE_REQUIRE(x && y && y_norm && ranks, "tribe_retrieval_ranks: null pointer");
  TRIBE_REQUIRE(N > 0 && M > 0 && V > 0 && ldx >= V && ldy >= V, "tribe_retrieval_ranks: bad shape N=%lld M=%lld V=%lld ldx=%lld ldy=%lld",
                (long long)N, (long long)M, (long long)V, (long long)ldx, (long long)ldy);
  TRIBE_REQUIRE(true_idx || N == M, "tribe_retrieval_ranks: without true indices the gallery must have N rows (N=%lld M=%lld)",
                (long long)N, (long long)M);
  TRIBE_REQUIRE(M < (1LL << 24), "tribe_retrieval_ranks: gallery of %lld rows exceeds the exact f32 rank range", (long long)M);
  const int64_t blocks = (N + RQ - 1) / RQ;
  TRIBE_REQUIRE(blocks <= 0x7fffffff, "tribe_retrieval_ranks: too many queries");
  hipLaunchKernelGGL(retrieval_ranks_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, y_norm, N, M, V,
                     true_idx, (int)relative, ranks);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_retrieval_scores(const float* x, int64_t ldx, const float* y, int64_t ldy, int64_t N, int64_t M, int64_t V,
                                      const float* x_norm, const float* y_norm, int32_t norm_kind, float* scores, void* stream) {
  TRIBE_REQUIRE(x && y && scores, "tribe_retrieval_scores: null pointer");
  TRIBE_REQUIRE(N > 0 && M > 0 && V > 0 && ldx >= V && ldy >= V, "tribe_retrieval_scores: bad shape");
  TRIBE_REQUIRE(norm_kind >= 0 && norm_kind <= 3, "tribe_retrieval_scores: norm_kind must be 0 (none), 1 (x), 2 (y) or 3 (xy)");
  TRIBE_REQUIRE((norm_kind != 1 && norm_kind != 3) || x_norm, "tribe_retrieval_scores: norm_kind needs x_norm");
  TRIBE_REQUIRE((norm_kind != 2 && norm_kind != 3) || y_norm, "tribe_retrieval_scores: norm_kind needs y_norm");
  const int64_t gx = (M + 15) / 16, gy = (N + 15) / 16;
  TRIBE_REQUIRE(gx <= 0x7fffffff && gy <= 65535, "tribe_retrieval_scores: shape too large for the diagnostic launch");
  hipLaunchKernelGGL(retrieval_scores_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, N, M, V,
                     x_norm, y_norm, (int)norm_kind, scores);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_rank_reduce(const float* ranks, int64_t n, float topk, float* out, void* stream) {
  TRIBE_REQUIRE(ranks && out, "tribe_rank_reduce: null pointer");
  TRIBE_REQUIRE(n > 0 && n <= 0x7fffffff, "tribe_rank_reduce: bad count %lld", (long long)n);
  hipLaunchKernelGGL(rank_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, ranks, n, topk, out);
  TRIBE_LAUNCH_CHECK();
  return 0;
}
