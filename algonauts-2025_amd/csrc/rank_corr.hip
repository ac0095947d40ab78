// Spearman rank correlation per output column (modeling_utils/metrics/rank_corr.py: MultidimSpearmanCorrCoef): sample store, sort,
// tie-aware rank transform and the Pearson-of-ranks sums.
//
//   append : strided [B, V, T] f32 views of predictions and targets -> the sample state [G, V, capacity] (one contiguous run of
//            samples per (group, column)).  A one-workgroup kernel turns the group of every batch row and the device-side sample
//            counts [G] into a destination per row and advances the counts; a tiled kernel then moves 64 x 64 (v, t) tiles through
//            LDS, so both the read (along whichever of t / v is the closer-packed) and the write (along t) are coalesced.
//   ranks  : a_i = #{x_j < x_i} + #{x_j <= x_i} - n = 2 * averagerank_i - (n + 1), an integer.  The column's keys are sorted without
//            payload; every element then takes a lower and an upper bound in the sorted keys, so ties need no fix-up pass.
//            Keys: -0.0 -> +0.0, then the usual order-preserving map of f32 bits to u32.  A NaN makes the column NaN (flagged
//            while loading; nothing depends on where its key lands).
//            n <= chunk: one workgroup per column holds both key arrays in LDS, sorts both, ranks and reduces, one launch.
//            n >  chunk: chunks of `chunk` keys are sorted in LDS, sorted runs are merged pairwise through a global workspace (every
//            key finds its place by its index in its own run plus a bound in the partner run), then a ranking pass binary-searches
//            the one sorted column and leaves int64 partial sums per tile, which a last kernel adds in tile order.
//   sums   : Sab = sum a_i b_i, Saa = sum a_i^2, Sbb = sum b_i^2 in int64: |a_i| <= n - 1 and n <= 2^20 keep them below 2^60,
//            exact in any order.  rho = Sab / sqrt((double)Saa (double)Sbb), clamped to [-1, 1], rounded once to f32; NaN for
//            n < 2, a constant column (Saa or Sbb == 0) or a NaN among the samples.
//
// LDS sort: a bitonic network.  Its strides j >= 64 run as LDS passes in which lane l of a wave touches dwords base + l and
// base + j + l (consecutive lanes, consecutive banks: conflict-free for ds_read_b32 / ds_write_b32, which bank per 32-lane half);
// the strides j <= 32, whose LDS form would put two lanes of a half on one bank, never touch LDS: a wave loads 64 consecutive
// keys, one per lane, and exchanges through __shfl_xor.  Only the binary searches of the ranking pass read LDS at data-dependent
// addresses.
#include "common.h"
#include "lds_sort.h"

namespace {

constexpr int RC_LANES = 1024;
constexpr int RC_MAX_CHUNK = 16384;          // two key arrays of 16384 u32 = 128 KiB of the 160 KiB LDS
constexpr int64_t RC_MAX_N = 1 << 20;        // n^3 < 2^60
constexpr int RC_VB = 64;                    // columns per round of the merge route (bounds the workspace)
constexpr int RC_TILE = 4096;                // elements per workgroup of the merge and ranking passes (RC_LANES lanes, 4 each)

__device__ __forceinline__ int lower_bound_u(const unsigned* s, int n, unsigned key) {   // #{s < key}
  int lo = 0, hi = n;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (s[m] < key) lo = m + 1; else hi = m;
  }
  return lo;
}
__device__ __forceinline__ int upper_bound_u(const unsigned* s, int n, unsigned key, int lo = 0) {   // #{s <= key}
  int hi = n;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if (s[m] <= key) lo = m + 1; else hi = m;
  }
  return lo;
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the three sums of a workgroup, waves added in wave order; valid in thread 0.  red: [3][16]
__device__ __forceinline__ void block_sum3(long long (&s)[3], long long* red) {
  const int w = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    s[q] = wave_sum_ll(s[q]);
    if ((threadIdx.x & 63) == 0) red[q * 16 + w] = s[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      long long t = 0;
      for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[q * 16 + i];
      s[q] = t;
    }
  }
}

__device__ __forceinline__ float rho_of(int n, long long sab, long long saa, long long sbb, bool has_nan) {
  if (has_nan || n < 2 || saa == 0 || sbb == 0) return __builtin_nanf("");
  double v = (double)sab / sqrt((double)saa * (double)sbb);
  if (v > 1.0) v = 1.0;
  if (v < -1.0) v = -1.0;
  return (float)v;
}

// doubled centred rank of `key` among sorted s[0..n)
__device__ __forceinline__ int centred_rank(const unsigned* s, int n, unsigned key) {
  const int lb = lower_bound_u(s, n, key);
  return lb + upper_bound_u(s, n, key, lb) - n;
}

__device__ __forceinline__ float average_rank(int a, int n) { return (float)(a + n + 1) * 0.5f; }   // exact: a + n + 1 <= 2^21

// ---- append ----------------------------------------------------------------------------------------------------------------
// One workgroup.  pos[b] = where the T samples of batch row b start in the run of its group (-1: group outside [0, G) or the run
// would pass the capacity: the row is dropped), counts[g] += T per row of group g.  Rows are taken 1024 at a time in batch order.
__global__ __launch_bounds__(RC_LANES) void rank_append_positions_kernel(const int64_t* __restrict__ group, int64_t B, int64_t T, int64_t G,
                                                                         int64_t cap, int64_t* __restrict__ counts, int64_t* __restrict__ pos) {
  __shared__ int64_t slot[RC_LANES];
  const int tid = threadIdx.x;
  for (int64_t b0 = 0; b0 < B; b0 += RC_LANES) {
    const int64_t b = b0 + tid;
    const int m = (int)(B - b0 < RC_LANES ? B - b0 : RC_LANES);
    int64_t g = -1;
    if (b < B) {
      g = group ? group[b] : 0;
      if (g < 0 || g >= G) g = -1;
    }
    __syncthreads();   // the previous tile's counts are written and its slots read
    slot[tid] = g;
    __syncthreads();
    int64_t start = -1;
    bool last = false;
    if (g >= 0) {
      int before = 0;
      last = true;
      for (int i = 0; i < m; ++i) {
        const bool same = slot[i] == g;
        before += (same && i < tid) ? 1 : 0;
        last = last && !(same && i > tid);
      }
      start = counts[g] + (int64_t)before * T;
    }
    __syncthreads();   // every thread has read counts[] before the last row of each group moves it
    const bool fits = start >= 0 && start + T <= cap;
    if (b < B) pos[b] = fits ? start : -1;
    // the group's last row that fits moves the count (rows come in order: once one does not fit, none behind it does)
    if (fits && (last || start + 2 * T > cap)) counts[g] = start + T;
  }
}

// grid (B, ceil(V / 64), 2 * ceil(T / 64)), 256 lanes: tile (v0.., t0..) of row b of predictions (even z) or targets (odd z)
__global__ __launch_bounds__(256) void rank_append_scatter_kernel(const float* __restrict__ pred, const float* __restrict__ truth, int64_t V,
                                                                  int64_t T, int64_t sb, int64_t sv, int64_t st, int t_fast,
                                                                  const int64_t* __restrict__ group, const int64_t* __restrict__ pos,
                                                                  int64_t cap, float* __restrict__ pbuf, float* __restrict__ tbuf) {
  __shared__ float tile[64][65];
  const int64_t b = blockIdx.x;
  const int64_t start = pos[b];
  if (start < 0) return;
  const int64_t g = group ? group[b] : 0;
  const bool second = blockIdx.z & 1;
  const int64_t v0 = (int64_t)blockIdx.y * 64, t0 = (int64_t)(blockIdx.z >> 1) * 64;
  const float* src = (second ? truth : pred) + b * sb;
  float* dst = (second ? tbuf : pbuf) + g * V * cap + start;
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  for (int r = ly; r < 64; r += 4) {
    const int64_t v = v0 + (t_fast ? r : lx), t = t0 + (t_fast ? lx : r);
    if (v < V && t < T) tile[v - v0][t - t0] = src[v * sv + t * st];
  }
  __syncthreads();
  for (int r = ly; r < 64; r += 4) {
    const int64_t v = v0 + r, t = t0 + lx;
    if (v < V && t < T) dst[v * cap + t] = tile[r][lx];
  }
}

// ---- n <= chunk: one workgroup per column ------------------------------------------------------------------------------------
// dynamic LDS: 2 * P u32.  rank_p / rank_t (nullptr: not written): average ranks f32 [V][n]
__global__ __launch_bounds__(RC_LANES) void spearman_one_kernel(const float* __restrict__ p, const float* __restrict__ t, int64_t ld, int n, int P,
                                                                float* __restrict__ rho, int64_t* __restrict__ sums, float* __restrict__ rank_p,
                                                                float* __restrict__ rank_t) {
  extern __shared__ __attribute__((aligned(16))) unsigned keys[];
  __shared__ long long red[3 * 16];
  __shared__ int nan_seen;
  unsigned* kp = keys;
  unsigned* kt = keys + P;
  const int tid = threadIdx.x;
  const int64_t col = blockIdx.x;
  const float* pc = p + col * ld;
  const float* tc = t + col * ld;
  if (tid == 0) nan_seen = 0;
  __syncthreads();
  bool bad = false;
  for (int i = tid; i < P; i += RC_LANES) {
    unsigned a = RC_PAD, b = RC_PAD;
    if (i < n) {
      const float x = pc[i], y = tc[i];
      bad = bad || x != x || y != y;
      a = key_of(x);
      b = key_of(y);
    }
    kp[i] = a;
    kt[i] = b;
  }
  if (bad) nan_seen = 1;
  __syncthreads();
  const bool has_nan = nan_seen != 0;   // the same for every thread
  long long s[3] = {0, 0, 0};
  if (!has_nan) {
    block_sort(kp, kt, P);
    for (int i = tid; i < n; i += RC_LANES) {
      const long long a = centred_rank(kp, n, key_of(pc[i])), b = centred_rank(kt, n, key_of(tc[i]));
      s[0] += a * b;
      s[1] += a * a;
      s[2] += b * b;
      if (rank_p) rank_p[col * n + i] = average_rank((int)a, n);
      if (rank_t) rank_t[col * n + i] = average_rank((int)b, n);
    }
  } else {
    for (int i = tid; i < n; i += RC_LANES) {
      if (rank_p) rank_p[col * n + i] = __builtin_nanf("");
      if (rank_t) rank_t[col * n + i] = __builtin_nanf("");
    }
  }
  block_sum3(s, red);
  if (tid == 0) {
    sums[col * 3 + 0] = s[0];
    sums[col * 3 + 1] = s[1];
    sums[col * 3 + 2] = s[2];
    rho[col] = rho_of(n, s[0], s[1], s[2], has_nan);
  }
}

// ---- n > chunk -----------------------------------------------------------------------------------------------------------------
// grid (chunks, columns, 2), dynamic LDS: chunk u32.  Sorted chunk c of column `col` of predictions (z = 0) / targets (z = 1) ->
// out[z][col][c * chunk ..]; flags[col] = 1 when the column holds a NaN.
__global__ __launch_bounds__(RC_LANES) void chunk_sort_kernel(const float* __restrict__ p, const float* __restrict__ t, int64_t ld, int n, int chunk,
                                                              int64_t cols, unsigned* __restrict__ out, int* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) unsigned keys[];
  const int tid = threadIdx.x;
  const int64_t col = blockIdx.y;
  const int c0 = (int)blockIdx.x * chunk;
  const int len = n - c0 < chunk ? n - c0 : chunk;
  int P = 64;
  while (P < len) P <<= 1;
  const float* src = (blockIdx.z ? t : p) + col * ld + c0;
  bool bad = false;
  for (int i = tid; i < P; i += RC_LANES) {
    unsigned a = RC_PAD;
    if (i < len) {
      const float x = src[i];
      bad = bad || x != x;
      a = key_of(x);
    }
    keys[i] = a;
  }
  if (bad) flags[col] = 1;   // every writer stores the same value
  __syncthreads();
  block_sort(keys, nullptr, P);
  unsigned* dst = out + ((int64_t)blockIdx.z * cols + col) * n + c0;
  for (int i = tid; i < len; i += RC_LANES) dst[i] = keys[i];
}

// E binary searches side by side, for keys that live in global memory: pos[e] = #{ptr[e][0..len[e]) < key[e]} (le[e] false) or
// #{... <= key[e]} (true).  Every search takes the same number of steps (half: a power of two above every len / 2, e.g. the largest
// power of two <= the longest run), and the E loads of a step do not depend on each other, so E probes are in flight per lane where
// one search after the other keeps one.  len[e] == 0 loads nothing.
template <int E>
__device__ __forceinline__ void bounds_many(const unsigned* const (&ptr)[E], const int (&len)[E], const unsigned (&key)[E], const bool (&le)[E],
                                            int half, int (&pos)[E]) {
#pragma unroll
  for (int e = 0; e < E; ++e) pos[e] = 0;
  for (; half > 0; half >>= 1) {
    unsigned v[E];
    bool ok[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int nx = pos[e] + half;
      ok[e] = nx <= len[e];
      v[e] = ok[e] ? ptr[e][nx - 1] : 0u;
    }
#pragma unroll
    for (int e = 0; e < E; ++e)
      if (ok[e] && (le[e] ? v[e] <= key[e] : v[e] < key[e])) pos[e] += half;
  }
}

constexpr int RC_PER_LANE = RC_TILE / RC_LANES;   // keys a lane of the merge and ranking passes searches side by side

// grid (ceil(n / RC_TILE), columns, 2): sorted runs of length L (a power of two), merged pairwise (run 2q with run 2q + 1; a last run
// without a partner is copied).  A key of the left run lands at its index plus #{right < key}, one of the right run at its index
// plus #{left <= key}: together a permutation, and equal keys are interchangeable.
__global__ __launch_bounds__(RC_LANES) void merge_pass_kernel(const unsigned* __restrict__ in, unsigned* __restrict__ out, int n, int L, int64_t cols) {
  const int64_t col = blockIdx.y;
  const unsigned* src = in + ((int64_t)blockIdx.z * cols + col) * n;
  unsigned* dst = out + ((int64_t)blockIdx.z * cols + col) * n;
  const int i0 = (int)blockIdx.x * RC_TILE + (int)threadIdx.x;
  const unsigned* ptr[RC_PER_LANE];
  int len[RC_PER_LANE], own[RC_PER_LANE], pos[RC_PER_LANE];
  unsigned key[RC_PER_LANE];
  bool le[RC_PER_LANE];
#pragma unroll
  for (int e = 0; e < RC_PER_LANE; ++e) {
    const int i = i0 + e * RC_LANES;
    ptr[e] = src;
    len[e] = 0;
    own[e] = -1;
    key[e] = 0u;
    le[e] = false;
    if (i < n) {
      key[e] = src[i];
      const int base = (i / (2 * L)) * (2 * L);
      const int mid = base + L < n ? base + L : n;
      const int end = base + 2 * L < n ? base + 2 * L : n;
      le[e] = i >= mid;
      ptr[e] = src + (le[e] ? base : mid);       // the partner run
      len[e] = le[e] ? mid - base : end - mid;
      own[e] = le[e] ? base + (i - mid) : i;     // the index the key has among its own run's keys, from the pair's start
    }
  }
  bounds_many<RC_PER_LANE>(ptr, len, key, le, L, pos);
#pragma unroll
  for (int e = 0; e < RC_PER_LANE; ++e)
    if (own[e] >= 0) dst[own[e] + pos[e]] = key[e];
}

// grid (ceil(n / RC_TILE), columns): ranks of the tile's elements in the sorted column, partial sums -> partial[col][tile][3].
// half: the largest power of two <= n.  The lower bounds of a lane's predictions and targets are searched side by side; the upper bound
// is one more probe where the key is the only one of its value (the key itself sits at the lower bound), a search of its own in a tie.
__global__ __launch_bounds__(RC_LANES) void rank_partial_kernel(const float* __restrict__ p, const float* __restrict__ t, int64_t ld, int n, int half,
                                                                int64_t cols, const unsigned* __restrict__ sorted, const int* __restrict__ flags,
                                                                long long* __restrict__ partial, float* __restrict__ rank_p,
                                                                float* __restrict__ rank_t) {
  __shared__ long long red[3 * 16];
  constexpr int E = 2 * RC_PER_LANE;
  const int64_t col = blockIdx.y;
  const float* pc = p + col * ld;
  const float* tc = t + col * ld;
  const unsigned* sp = sorted + col * n;
  const unsigned* st = sorted + (cols + col) * n;
  const bool has_nan = flags[col] != 0;
  const int i0 = (int)blockIdx.x * RC_TILE + (int)threadIdx.x;
  long long s[3] = {0, 0, 0};
  if (has_nan) {
    for (int e = 0; e < RC_PER_LANE; ++e) {
      const int i = i0 + e * RC_LANES;
      if (i < n && rank_p) rank_p[col * n + i] = __builtin_nanf("");
      if (i < n && rank_t) rank_t[col * n + i] = __builtin_nanf("");
    }
  } else {
    const unsigned* ptr[E];
    int len[E], pos[E];
    unsigned key[E];
    bool le[E];
#pragma unroll
    for (int e = 0; e < RC_PER_LANE; ++e) {
      const int i = i0 + e * RC_LANES;
      const bool in = i < n;
      ptr[2 * e] = sp;
      ptr[2 * e + 1] = st;
      len[2 * e] = len[2 * e + 1] = in ? n : 0;
      key[2 * e] = in ? key_of(pc[i]) : 0u;
      key[2 * e + 1] = in ? key_of(tc[i]) : 0u;
      le[2 * e] = le[2 * e + 1] = false;
    }
    bounds_many<E>(ptr, len, key, le, half, pos);
    int r[E];
#pragma unroll
    for (int q = 0; q < E; ++q) {
      r[q] = 0;
      if (len[q] > 0) {
        const int lb = pos[q];
        const bool tie = lb + 1 < n && ptr[q][lb + 1] == key[q];
        const int ub = tie ? upper_bound_u(ptr[q], n, key[q], lb + 2) : lb + 1;
        r[q] = lb + ub - n;
      }
    }
#pragma unroll
    for (int e = 0; e < RC_PER_LANE; ++e) {
      const int i = i0 + e * RC_LANES;
      if (i >= n) continue;
      const long long a = r[2 * e], b = r[2 * e + 1];
      s[0] += a * b;
      s[1] += a * a;
      s[2] += b * b;
      if (rank_p) rank_p[col * n + i] = average_rank((int)a, n);
      if (rank_t) rank_t[col * n + i] = average_rank((int)b, n);
    }
  }
  block_sum3(s, red);
  if (threadIdx.x == 0) {
    long long* dst = partial + (col * gridDim.x + blockIdx.x) * 3;
    dst[0] = s[0];
    dst[1] = s[1];
    dst[2] = s[2];
  }
}

__global__ __launch_bounds__(256) void spearman_final_kernel(const long long* __restrict__ partial, const int* __restrict__ flags, int n, int tiles,
                                                             int64_t cols, float* __restrict__ rho, int64_t* __restrict__ sums) {
  const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= cols) return;
  long long s[3] = {0, 0, 0};
  for (int i = 0; i < tiles; ++i)
#pragma unroll
    for (int q = 0; q < 3; ++q) s[q] += partial[(col * tiles + i) * 3 + q];
#pragma unroll
  for (int q = 0; q < 3; ++q) sums[col * 3 + q] = s[q];
  rho[col] = rho_of(n, s[0], s[1], s[2], flags[col] != 0);
}

int effective_chunk(int64_t chunk) { return chunk <= 0 ? RC_MAX_CHUNK : (int)chunk; }

bool chunk_ok(int64_t chunk) { return chunk <= 0 || (chunk >= 64 && chunk <= RC_MAX_CHUNK && (chunk & (chunk - 1)) == 0); }

// merge-route workspace of one round of `cols` columns: keys u32 [2 buffers][2 tensors][cols][n], partial i64 [cols][tiles][3], flags
struct MergeWs {
  size_t keys_bytes, partial_bytes, flags_bytes;
  size_t total() const { return 2 * keys_bytes + partial_bytes + flags_bytes; }
};
MergeWs merge_ws(int64_t n, int64_t cols) {
  const int64_t tiles = (n + RC_TILE - 1) / RC_TILE;
  return {(size_t)(2 * cols * n) * sizeof(unsigned), (size_t)(cols * tiles * 3) * sizeof(long long), (size_t)round_up(cols * 4, 16)};
}

}  // namespace

extern "C" int64_t tribe_spearman_default_chunk(void) { return RC_MAX_CHUNK; }

extern "C" int64_t tribe_spearman_max_samples(void) { return RC_MAX_N; }

extern "C" size_t tribe_spearman_workspace_bytes(int64_t n, int64_t V, int64_t chunk) {
  if (n <= 0 || V <= 0 || !chunk_ok(chunk) || n <= effective_chunk(chunk)) return 0;
  return merge_ws(n, V < RC_VB ? V : RC_VB).total();
}

extern "C" int tribe_rank_append(const float* pred, const float* truth, int64_t B, int64_t V, int64_t T, int64_t sb, int64_t sv, int64_t st,
                                 const int64_t* group, int64_t n_groups, int64_t capacity, int64_t* counts, int64_t* positions,
                                 float* pred_state, float* truth_state, void* stream) {
  TRIBE_REQUIRE(pred && truth && counts && positions && pred_state && truth_state, "tribe_rank_append: null pointer");
  TRIBE_REQUIRE(B > 0 && V > 0 && T > 0 && n_groups > 0, "tribe_rank_append: bad shape B=%lld V=%lld T=%lld G=%lld", (long long)B, (long long)V,
                (long long)T, (long long)n_groups);
  TRIBE_REQUIRE(capacity >= T, "tribe_rank_append: capacity %lld below one row of %lld samples", (long long)capacity, (long long)T);
  const int64_t vt = (V + 63) / 64, tt = (T + 63) / 64;
  TRIBE_REQUIRE(B <= 0x7fffffff && vt <= 65535 && 2 * tt <= 65535, "tribe_rank_append: shape too large B=%lld V=%lld T=%lld", (long long)B,
                (long long)V, (long long)T);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rank_append_positions_kernel, dim3(1), dim3(RC_LANES), 0, s, group, B, T, n_groups, capacity, counts, positions);
  TRIBE_LAUNCH_CHECK();
  const int64_t ast = st < 0 ? -st : st, asv = sv < 0 ? -sv : sv;
  const int t_fast = (T > 1 && ast <= asv) || V == 1;
  hipLaunchKernelGGL(rank_append_scatter_kernel, dim3((unsigned)B, (unsigned)vt, (unsigned)(2 * tt)), dim3(256), 0, s, pred, truth, V, T, sb, sv, st,
                     t_fast, group, (const int64_t*)positions, capacity, pred_state, truth_state);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_spearman_columns(const float* pred, const float* truth, int64_t ld, int64_t n, int64_t V, int64_t chunk, float* rho,
                                      int64_t* sums, float* rank_pred, float* rank_truth, void* workspace, size_t workspace_bytes,
                                      void* stream) {
  TRIBE_REQUIRE(pred && truth && rho && sums, "tribe_spearman_columns: null pointer");
  TRIBE_REQUIRE(n >= 1 && V >= 1 && ld >= n, "tribe_spearman_columns: bad shape n=%lld V=%lld ld=%lld", (long long)n, (long long)V, (long long)ld);
  TRIBE_REQUIRE(n <= RC_MAX_N, "tribe_spearman_columns: %lld samples exceed 2^20 (the int64 rank sums are exact up to there)", (long long)n);
  TRIBE_REQUIRE(chunk_ok(chunk), "tribe_spearman_columns: chunk must be <= 0 (default) or a power of two in [64, %d], got %lld", RC_MAX_CHUNK,
                (long long)chunk);
  TRIBE_REQUIRE(V <= 0x7fffffff, "tribe_spearman_columns: too many columns");
  hipStream_t s = (hipStream_t)stream;
  const int ch = effective_chunk(chunk);
  if (n <= ch) {
    int P = 64;
    while (P < n) P <<= 1;
    const size_t smem = (size_t)2 * P * sizeof(unsigned);
    if (smem > 64 * 1024)   // per device, and only compute() comes here: not worth a cache
      (void)hipFuncSetAttribute((const void*)spearman_one_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * RC_MAX_CHUNK * (int)sizeof(unsigned));
    hipLaunchKernelGGL(spearman_one_kernel, dim3((unsigned)V), dim3(RC_LANES), smem, s, pred, truth, ld, (int)n, P, rho, sums, rank_pred, rank_truth);
    TRIBE_LAUNCH_CHECK();
    return 0;
  }
  const size_t need = tribe_spearman_workspace_bytes(n, V, chunk);
  TRIBE_REQUIRE(workspace && workspace_bytes >= need, "tribe_spearman_columns: workspace too small (%zu bytes, need %zu)", workspace_bytes, need);
  const int64_t vb = V < RC_VB ? V : RC_VB;
  const MergeWs w = merge_ws(n, vb);
  unsigned* buf[2] = {(unsigned*)workspace, (unsigned*)((char*)workspace + w.keys_bytes)};
  long long* partial = (long long*)((char*)workspace + 2 * w.keys_bytes);
  int* flags = (int*)((char*)workspace + 2 * w.keys_bytes + w.partial_bytes);
  const int chunks = (int)((n + ch - 1) / ch), tiles = (int)((n + RC_TILE - 1) / RC_TILE);
  int half = 1;
  while (2 * (int64_t)half <= n) half *= 2;
  for (int64_t c0 = 0; c0 < V; c0 += vb) {
    const int64_t cols = V - c0 < vb ? V - c0 : vb;
    const float* pc = pred + c0 * ld;
    const float* tc = truth + c0 * ld;
    hipError_t e = hipMemsetAsync(flags, 0, w.flags_bytes, s);
    if (e != hipSuccess) { tribe_set_error("tribe_spearman_columns: memset failed: %s", hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(chunk_sort_kernel, dim3((unsigned)chunks, (unsigned)cols, 2), dim3(RC_LANES), (size_t)ch * sizeof(unsigned), s, pc, tc, ld, (int)n,
                       ch, cols, buf[0], flags);
    TRIBE_LAUNCH_CHECK();
    int cur = 0;
    for (int64_t L = ch; L < n; L *= 2) {
      hipLaunchKernelGGL(merge_pass_kernel, dim3((unsigned)tiles, (unsigned)cols, 2), dim3(RC_LANES), 0, s, (const unsigned*)buf[cur], buf[cur ^ 1], (int)n,
                         (int)L, cols);
      TRIBE_LAUNCH_CHECK();
      cur ^= 1;
    }
    hipLaunchKernelGGL(rank_partial_kernel, dim3((unsigned)tiles, (unsigned)cols), dim3(RC_LANES), 0, s, pc, tc, ld, (int)n, half, cols, (const unsigned*)buf[cur],
                       (const int*)flags, partial, rank_pred ? rank_pred + c0 * n : nullptr, rank_truth ? rank_truth + c0 * n : nullptr);
    TRIBE_LAUNCH_CHECK();
    hipLaunchKernelGGL(spearman_final_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, s, (const long long*)partial, (const int*)flags, (int)n,
                       tiles, cols, rho + c0, sums + c0 * 3);
    TRIBE_LAUNCH_CHECK();
  }
  return 0;
}
