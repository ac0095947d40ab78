// Causal attention of the training path (modeling_utils.autograd.Attention with causal=True): the two row kernels around the materialised
// scores, the causal counterparts of tribe_softmax_dropout_fwd / _bwd (attn_dropout.hip).  Their contract plus one rule: row r of a slab
// is query i = (row0 + r) % T of the logical tensor [B heads T, T], and columns j > i are masked.
//   tribe_softmax_causal_fwd   S f32 [rows, T] -> Pd[r, j <= i] = bf16(softmax(S[r, 0..i])[j] * m), +0.0 bits for i < j < T_pad; lse2 f32 [rows]
//                              of the visible scores
//   tribe_softmax_causal_bwd   P bf16, dPd f32, negD f32 [rows] -> for j <= i: dS = bf16(P * (scale * (m * dPd) + negD)), Pd = bf16(P * m);
//                              +0.0 bits elsewhere in both (Pd == P allowed)
// m is attn_dropout.hip's mask unchanged -- idx = (row0 + r) * T + j, the same Philox counter, key and word -- so the causal mask is that one
// restricted to the lower triangle.
//
// Skip, don't select: a row loads, draws and computes its visible quads 0 .. i / 4 only; every other quad of the row (pad columns
// included) is zero-filled with 8-byte stores and its Philox call is not made.  What lies above the diagonal in S, P and dPd is not read
// outside the quad that holds the diagonal, and there it is dropped by a select: P comes from the ACT_EXP2 epilogue, which knows no mask,
// and holds exp2(s - lse2) against a log-sum-exp without those keys -- possibly inf.
//
// Kernel selection (reg for T in {256, 512, 1024, 2048}, vec walk, elem walk), the elements a lane owns and the order of every sum are
// those of attn_dropout.hip; a skipped element adds an exact zero there (exp(-inf - max) = +0.0), so on columns <= i the results -- lse
// included -- have the bits of tribe_softmax_dropout_fwd / _bwd run on the same scores with -inf written above the diagonal.
// One wave per row, four rows per 256-thread workgroup.  No atomics; bit-reproducible.
#include <float.h>

#include "common.h"
#include "philox.h"

namespace {

// the arithmetic of attn_dropout.hip, restated (that file keeps its helpers to itself): any change there is one here
constexpr float SC_LOG2E = 1.4426950408889634f;

struct sc_key {
  unsigned thr, k0, k1, s0, s1;
  float keep;
};

__device__ __forceinline__ uint4 sc_words(const sc_key& k, int64_t quad) {
  return philox4x32_10(make_uint4((unsigned)((uint64_t)quad & 0xffffffffu), (unsigned)((uint64_t)quad >> 32), k.s0, k.s1), k.k0, k.k1);
}
__device__ __forceinline__ unsigned short sc_fwd(float p, unsigned word, const sc_key& k) {
  return word >= k.thr ? f32_to_bf16(__fmul_rn(p, k.keep)) : (unsigned short)0;
}
__device__ __forceinline__ float sc_lse2(float m, float sum) { return fmaf(m, SC_LOG2E, __log2f(sum)); }

// columns [from, to) of a row <- +0.0: 8-byte stores over the whole quads when the row start is 8-byte aligned, elements at the ragged ends
__device__ __forceinline__ void sc_zero(unsigned short* p, int64_t from, int64_t to, int lane) {
  if (from >= to) return;
  if (((uintptr_t)p & 7) != 0) {
    for (int64_t c = from + lane; c < to; c += 64) p[c] = (unsigned short)0;
    return;
  }
  const int64_t q0 = (from + 3) >> 2, q1 = to >> 2;   // whole quads [q0, q1)
  if (q0 >= q1) {
    for (int64_t c = from + lane; c < to; c += 64) p[c] = (unsigned short)0;
    return;
  }
  if (from + lane < q0 * 4) p[from + lane] = (unsigned short)0;
  const u16x4_t z = {0, 0, 0, 0};
  for (int64_t q = q0 + lane; q < q1; q += 64) *(u16x4_t*)(p + q * 4) = z;
  if (q1 * 4 + lane < to) p[q1 * 4 + lane] = (unsigned short)0;
}

template <int NV>
__global__ __launch_bounds__(256) void softmax_causal_reg_kernel(const float* __restrict__ S, int64_t R, int64_t ld_s,
                                                                 unsigned short* __restrict__ P, int64_t ld_p, float* __restrict__ lse,
                                                                 int64_t row0, sc_key k) {
  constexpr int T = 256 * NV;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int qi = (int)((row0 + row) % T);   // the query: columns 0 .. qi are visible, quads 0 .. qi / 4
  const int last = qi >> 2;
  const float* s = S + row * ld_s;
  float4 v[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int q = lane + 64 * j;
    v[j] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    if (q <= last) {
      v[j] = load_nt_f4(s + q * 4);
      if (q == last) {   // the quad that holds the diagonal
        const int c = q * 4;
        if (c + 1 > qi) v[j].y = -INFINITY;
        if (c + 2 > qi) v[j].z = -INFINITY;
        if (c + 3 > qi) v[j].w = -INFINITY;
      }
    }
  }
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < NV; ++j) m = fmaxf(m, fmaxf(fmaxf(v[j].x, v[j].y), fmaxf(v[j].z, v[j].w)));
  m = wave_max(m);
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    if (lane + 64 * j <= last) {   // (a masked element of the diagonal's quad: exp(-inf - m) = +0.0)
      v[j].x = __expf(v[j].x - m); v[j].y = __expf(v[j].y - m); v[j].z = __expf(v[j].z - m); v[j].w = __expf(v[j].w - m);
      sum += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    }
  }
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  if (lane == 0) lse[row] = sc_lse2(m, sum);
  const int64_t quad0 = (row0 + row) * (64 * NV);   // T / 4 counters per row
  unsigned short* p = P + row * ld_p;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int q = lane + 64 * j;
    u16x4_t o = {0, 0, 0, 0};
    if (q <= last) {
      const uint4 w = sc_words(k, quad0 + q);
      const int c = q * 4;
      o[0] = sc_fwd(__fmul_rn(v[j].x, inv), w.x, k);
      o[1] = c + 1 <= qi ? sc_fwd(__fmul_rn(v[j].y, inv), w.y, k) : (unsigned short)0;
      o[2] = c + 2 <= qi ? sc_fwd(__fmul_rn(v[j].z, inv), w.z, k) : (unsigned short)0;
      o[3] = c + 3 <= qi ? sc_fwd(__fmul_rn(v[j].w, inv), w.w, k) : (unsigned short)0;
    }
    *(u16x4_t*)(p + q * 4) = o;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void softmax_causal_walk_kernel(const float* __restrict__ S, int64_t R, int64_t T, int64_t ld_s,
                                                                  unsigned short* __restrict__ P, int64_t T_pad, int64_t ld_p,
                                                                  float* __restrict__ lse, int64_t row0, sc_key k) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t qi = (row0 + row) % T, n = qi + 1;   // n visible columns
  const float* s = S + row * ld_s;
  float m = -INFINITY;
  for (int64_t i = lane; i < n; i += 64) m = fmaxf(m, s[i]);
  m = wave_max(m);
  float sum = 0.f;
  for (int64_t i = lane; i < n; i += 64) sum += __expf(s[i] - m);
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  if (lane == 0) lse[row] = sc_lse2(m, sum);
  unsigned short* p = P + row * ld_p;
  const int64_t base = (row0 + row) * T;   // idx of the row's column 0
  if constexpr (VEC) {
    const int64_t quad0 = base >> 2, nq = (qi >> 2) + 1;   // T % 4 == 0: column 4 c4 starts counter quad0 + c4
    for (int64_t c4 = lane; c4 < nq; c4 += 64) {
      const float4 x = *(const float4*)(s + c4 * 4);
      const uint4 w = sc_words(k, quad0 + c4);
      const int64_t c = c4 * 4;
      u16x4_t o;
      o[0] = sc_fwd(__fmul_rn(__expf(x.x - m), inv), w.x, k);
      o[1] = c + 1 <= qi ? sc_fwd(__fmul_rn(__expf(x.y - m), inv), w.y, k) : (unsigned short)0;
      o[2] = c + 2 <= qi ? sc_fwd(__fmul_rn(__expf(x.z - m), inv), w.z, k) : (unsigned short)0;
      o[3] = c + 3 <= qi ? sc_fwd(__fmul_rn(__expf(x.w - m), inv), w.w, k) : (unsigned short)0;
      *(u16x4_t*)(p + c4 * 4) = o;
    }
    sc_zero(p, nq * 4, T_pad, lane);
  } else {
    const int64_t q_last = (base + qi) >> 2;
    for (int64_t q = (base >> 2) + lane; q <= q_last; q += 64) {
      const uint4 o = sc_words(k, q);
      const unsigned w[4] = {o.x, o.y, o.z, o.w};
      const int64_t c0 = q * 4 - base;   // -3 .. qi: column of the counter's first element
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t c = c0 + e;
        if (c >= 0 && c < n) p[c] = sc_fwd(__fmul_rn(__expf(s[c] - m), inv), w[e], k);
      }
    }
    sc_zero(p, n, T_pad, lane);
  }
}

struct sc_pair {
  unsigned short ds, pd;
};
__device__ __forceinline__ sc_pair sc_bwd(unsigned short pb, float dp, unsigned word, float nd, float scale, const sc_key& k) {
  const bool keep = word >= k.thr;
  const float pf = bf16_to_f32(pb);
  const float g = keep ? __fmul_rn(dp, k.keep) : 0.f;   // m * dPd
  return {f32_to_bf16(pf * fmaf(scale, g, nd)), keep ? f32_to_bf16(__fmul_rn(pf, k.keep)) : (unsigned short)0};
}
// the same where the column is visible, +0.0 bits where it is not: whatever P and dPd hold there (inf, NaN) goes no further than the select
__device__ __forceinline__ sc_pair sc_bwd_if(bool visible, unsigned short pb, float dp, unsigned word, float nd, float scale, const sc_key& k) {
  const sc_pair r = sc_bwd(pb, dp, word, nd, scale, k);
  return {visible ? r.ds : (unsigned short)0, visible ? r.pd : (unsigned short)0};
}

// P and Pd may be the same buffer (no __restrict__ on either): a lane reads its elements of P before it writes them, no other lane touches
// them, and the zero fill covers columns nobody reads
template <bool VEC>
__global__ __launch_bounds__(256) void softmax_causal_bwd_kernel(const unsigned short* P, const float* __restrict__ dPd,
                                                                 const float* __restrict__ negD, int64_t R, int64_t T, int64_t T_pad, int64_t ld_p,
                                                                 int64_t ld_dp, float scale, unsigned short* __restrict__ dS, int64_t ld_ds,
                                                                 unsigned short* Pd, int64_t ld_pd, int64_t row0, sc_key k) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t qi = (row0 + row) % T, n = qi + 1;
  const unsigned short* p = P + row * ld_p;
  const float* dp = dPd + row * ld_dp;
  unsigned short* ds = dS + row * ld_ds;
  unsigned short* pd = Pd + row * ld_pd;
  const float nd = negD[row];
  const int64_t base = (row0 + row) * T;
  int64_t filled;   // first column of the zero fill
  if constexpr (VEC) {
    const int64_t quad0 = base >> 2, nq = (qi >> 2) + 1;
    for (int64_t c4 = lane; c4 < nq; c4 += 64) {
      const u16x4_t pv = *(const u16x4_t*)(p + c4 * 4);
      const float4 dv = load_nt_f4(dp + c4 * 4);
      const uint4 w = sc_words(k, quad0 + c4);
      const int64_t c = c4 * 4;
      const sc_pair r0 = sc_bwd(pv[0], dv.x, w.x, nd, scale, k), r1 = sc_bwd_if(c + 1 <= qi, pv[1], dv.y, w.y, nd, scale, k);
      const sc_pair r2 = sc_bwd_if(c + 2 <= qi, pv[2], dv.z, w.z, nd, scale, k), r3 = sc_bwd_if(c + 3 <= qi, pv[3], dv.w, w.w, nd, scale, k);
      u16x4_t o, q;
      o[0] = r0.ds; o[1] = r1.ds; o[2] = r2.ds; o[3] = r3.ds;
      q[0] = r0.pd; q[1] = r1.pd; q[2] = r2.pd; q[3] = r3.pd;
      *(u16x4_t*)(ds + c4 * 4) = o;
      *(u16x4_t*)(pd + c4 * 4) = q;
    }
    filled = nq * 4;
  } else {
    const int64_t q_last = (base + qi) >> 2;
    for (int64_t q = (base >> 2) + lane; q <= q_last; q += 64) {
      const uint4 o = sc_words(k, q);
      const unsigned w[4] = {o.x, o.y, o.z, o.w};
      const int64_t c0 = q * 4 - base;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t c = c0 + e;
        if (c >= 0 && c < n) {
          const sc_pair r = sc_bwd(p[c], dp[c], w[e], nd, scale, k);
          ds[c] = r.ds;
          pd[c] = r.pd;
        }
      }
    }
    filled = n;
  }
  sc_zero(ds, filled, T_pad, lane);
  sc_zero(pd, filled, T_pad, lane);
}

bool sc_aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p % bytes) == 0; }

sc_key make_key(uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site) {
  return {threshold, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)(site & 0xffffffffu), (unsigned)(site >> 32), scale_keep};
}

}  // namespace

#define TRIBE_SC_SHAPE(name)                                                                                                              \
  TRIBE_REQUIRE(rows > 0 && T > 0 && rows < (1ll << 31) && T < (1ll << 31) && T_pad >= T && T_pad < (1ll << 31), name ": rows=%lld T=%lld " \
                "T_pad=%lld (need 0 < rows < 2^31, 0 < T <= T_pad < 2^31)", (long long)rows, (long long)T, (long long)T_pad);              \
  TRIBE_REQUIRE(row0 >= 0 && row0 < (1ll << 31), name ": row0=%lld (need 0 <= row0 < 2^31)", (long long)row0);                             \
  TRIBE_REQUIRE(scale_keep >= 1.f && scale_keep <= FLT_MAX, name ": scale_keep = 1 / (1 - p) must be finite and >= 1, got %g", (double)scale_keep)

extern "C" int tribe_softmax_causal_fwd(const float* S, uint16_t* Pd, float* lse, int64_t rows, int64_t T, int64_t T_pad, int64_t ld_s,
                                        int64_t ld_p, int64_t row0, uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site,
                                        void* stream) {
  TRIBE_REQUIRE(S && Pd && lse, "tribe_softmax_causal_fwd: null pointer");
  TRIBE_SC_SHAPE("tribe_softmax_causal_fwd");
  TRIBE_REQUIRE(ld_s >= T && ld_p >= T_pad && ld_s < (1ll << 40) && ld_p < (1ll << 40),
                "tribe_softmax_causal_fwd: ld_s=%lld ld_p=%lld (need ld_s >= T = %lld, ld_p >= T_pad = %lld)", (long long)ld_s, (long long)ld_p,
                (long long)T, (long long)T_pad);
  const sc_key k = make_key(threshold, scale_keep, seed, site);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((rows + 3) / 4));
  const bool vec = T % 4 == 0 && ld_s % 4 == 0 && ld_p % 4 == 0 && sc_aligned(S, 16) && sc_aligned(Pd, 8);
  const bool reg = vec && T_pad == T && T % 256 == 0 && T <= 2048;   // tribe_softmax_dropout_fwd's conditions: the same summation order
  if (reg && T == 256) hipLaunchKernelGGL(softmax_causal_reg_kernel<1>, grid, dim3(256), 0, st, S, rows, ld_s, Pd, ld_p, lse, row0, k);
  else if (reg && T == 512) hipLaunchKernelGGL(softmax_causal_reg_kernel<2>, grid, dim3(256), 0, st, S, rows, ld_s, Pd, ld_p, lse, row0, k);
  else if (reg && T == 1024) hipLaunchKernelGGL(softmax_causal_reg_kernel<4>, grid, dim3(256), 0, st, S, rows, ld_s, Pd, ld_p, lse, row0, k);
  else if (reg && T == 2048) hipLaunchKernelGGL(softmax_causal_reg_kernel<8>, grid, dim3(256), 0, st, S, rows, ld_s, Pd, ld_p, lse, row0, k);
  else if (vec) hipLaunchKernelGGL(softmax_causal_walk_kernel<true>, grid, dim3(256), 0, st, S, rows, T, ld_s, Pd, T_pad, ld_p, lse, row0, k);
  else hipLaunchKernelGGL(softmax_causal_walk_kernel<false>, grid, dim3(256), 0, st, S, rows, T, ld_s, Pd, T_pad, ld_p, lse, row0, k);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_softmax_causal_bwd(const uint16_t* P, const float* dPd, const float* negD, uint16_t* dS, uint16_t* Pd, int64_t rows,
                                        int64_t T, int64_t T_pad, int64_t ld_p, int64_t ld_dp, int64_t ld_ds, int64_t ld_pd, float scale,
                                        int64_t row0, uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site, void* stream) {
  TRIBE_REQUIRE(P && dPd && negD && dS && Pd, "tribe_softmax_causal_bwd: null pointer");
  TRIBE_SC_SHAPE("tribe_softmax_causal_bwd");
  TRIBE_REQUIRE(ld_p >= T_pad && ld_dp >= T && ld_ds >= T_pad && ld_pd >= T_pad && ld_p < (1ll << 40) && ld_dp < (1ll << 40) &&
                    ld_ds < (1ll << 40) && ld_pd < (1ll << 40),
                "tribe_softmax_causal_bwd: ld_p=%lld ld_dp=%lld ld_ds=%lld ld_pd=%lld (need ld_dp >= T = %lld, the others >= T_pad = %lld)",
                (long long)ld_p, (long long)ld_dp, (long long)ld_ds, (long long)ld_pd, (long long)T, (long long)T_pad);
  TRIBE_REQUIRE((const void*)dS != (const void*)P && dS != Pd, "tribe_softmax_causal_bwd: dS must not be P or Pd");
  TRIBE_REQUIRE((const void*)Pd != (const void*)P || ld_pd == ld_p, "tribe_softmax_causal_bwd: in place (Pd == P) needs ld_pd == ld_p");
  const sc_key k = make_key(threshold, scale_keep, seed, site);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((rows + 3) / 4));
  const bool vec = T % 4 == 0 && ld_p % 4 == 0 && ld_dp % 4 == 0 && ld_ds % 4 == 0 && ld_pd % 4 == 0 && sc_aligned(P, 8) && sc_aligned(dPd, 16) &&
                   sc_aligned(dS, 8) && sc_aligned(Pd, 8);
  if (vec)
    hipLaunchKernelGGL(softmax_causal_bwd_kernel<true>, grid, dim3(256), 0, st, P, dPd, negD, rows, T, T_pad, ld_p, ld_dp, scale, dS, ld_ds, Pd,
                       ld_pd, row0, k);
  else
    hipLaunchKernelGGL(softmax_causal_bwd_kernel<false>, grid, dim3(256), 0, st, P, dPd, negD, rows, T, T_pad, ld_p, ld_dp, scale, dS, ld_ds, Pd,
                       ld_pd, row0, k);
  TRIBE_LAUNCH_CHECK();
  return 0;
}
