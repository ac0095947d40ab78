// The row kernels around the materialised scores of the training path (modeling_utils.autograd.Attention with attn_dropout > 0 or
// causal=True): one family, compiled with and without the causal rule.
//   tribe_softmax_dropout_fwd   S f32 [rows, T] -> Pd = bf16(softmax(S) * m) [rows, T_pad] (pad columns zero) and lse2 f32 [rows]
//   tribe_softmax_dropout_bwd   P bf16, dPd f32, negD f32 [rows] -> dS = bf16(P * (scale * (m * dPd) + negD)), and Pd = bf16(P * m) over P
//   tribe_softmax_causal_fwd / _bwd   the same with CAUSAL: row r of a slab is query i = (row0 + r) % T of the logical tensor
//                               [B heads T, T] and sees its n = i + 1 first columns (non-causal: n = T).  The softmax and lse2 are those of
//                               S[r, 0..i]; every column n <= j < T_pad of Pd and dS holds +0.0 bits (Pd == P allowed in both settings)
// m is the mask factor of tribe_dropout_apply (dropout.hip) on the LOGICAL tensor [row0 + rows, T]: element (r, j) of the slab has
// idx = (row0 + r) * T + j (64-bit; from T, never from a pitch or T_pad), its word is word idx & 3 of Philox4x32-10 (philox.h) with counter
// (lo32(idx >> 2), hi32(idx >> 2), lo32(site), hi32(site)) and key (lo32(seed), hi32(seed)); kept iff word >= threshold; kept values are
// multiplied by scale_keep in f32 with one rounding (__fmul_rn), dropped ones are +0.0 by a select.  No mask tensor exists: both kernels
// draw it in registers, one Philox call per four consecutive idx.  row0 makes the mask independent of how the caller chunks the batch.
//
// One wave per row, four rows per 256-thread workgroup (as softmax_kernel / softmax_bwd_kernel).  The row statistics are softmax_row.h's,
// which are tribe_softmax_fwd's too, so threshold = 0, scale_keep = 1 reproduces its bits:
//   reg   T = 256 NV (NV = 1, 2, 4, 8), T_pad == T, pitches % 4 == 0, S 16-byte / P 8-byte aligned: the row in registers, 16-byte loads,
//         8-byte stores, lane l holds quads l + 64 j of the row (row starts are quad-aligned: T % 4 == 0)
//   walk  every other shape: maximum and sum by lanes striding over elements (softmax_kernel's order); the store pass goes by quads:
//         vec (T % 4 == 0 and the alignments above): the row's quads start at its column 0, 16-byte loads / 8-byte stores;
//         elem: lane l takes the counters (first idx of the row >> 2) + l + 64 k and writes whichever of their four elements lie in the
//         row -- a quad that straddles a row end is drawn by both rows (at most two extra calls per row).
// The backward has no row reduction (D comes in from tribe_rowdot_heads_bf16): vec / elem as above.  No atomics; bit-reproducible.
//
// CAUSAL is a template parameter and n its only consequence.  Skip, don't select: a causal row loads, draws and computes its visible quads
// 0 .. i / 4 only; every other quad of the row (pad columns included) is zero-filled with 8-byte stores and its Philox call is not made.
// What lies above the diagonal in S, P and dPd is not read outside the quad that holds the diagonal, and there it is dropped by a select: P
// comes from the ACT_EXP2 epilogue, which knows no mask, and holds exp2(s - lse2) against a log-sum-exp without those keys -- possibly inf.
// The elements a lane owns and the order of every sum do not depend on CAUSAL, and a skipped element adds an exact zero
// (exp(-inf - max) = +0.0), so on columns <= i the causal results -- lse included -- have the bits of the non-causal kernels run on the
// same scores with -inf written above the diagonal.
#include <float.h>

#include "common.h"
#include "philox.h"
#include "row_wave.h"
#include "softmax_row.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

struct mask_key {
  unsigned thr, k0, k1, s0, s1;
  float keep;
};

__device__ __forceinline__ uint4 words(const mask_key& k, int64_t quad) {
  return philox4x32_10(make_uint4((unsigned)((uint64_t)quad & 0xffffffffu), (unsigned)((uint64_t)quad >> 32), k.s0, k.s1), k.k0, k.k1);
}
// p = softmax value (f32) -> the bf16 of Pd
__device__ __forceinline__ unsigned short fwd(float p, unsigned word, const mask_key& k) {
  return word >= k.thr ? f32_to_bf16(__fmul_rn(p, k.keep)) : (unsigned short)0;
}
// base-2 log-sum-exp of a row with maximum m and sum = sum exp(s - m): what ACT_EXP2 subtracts from scale log2e q.k
__device__ __forceinline__ float lse2(float m, float sum) { return fmaf(m, LOG2E, __log2f(sum)); }

// columns [from, to) of a row <- +0.0: 8-byte stores over the whole quads when the row start is 8-byte aligned, elements at the ragged ends
__device__ __forceinline__ void zero_fill(unsigned short* p, int64_t from, int64_t to, int lane) {
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

template <int NV, bool CAUSAL>
__global__ __launch_bounds__(256) void softmax_rows_reg_kernel(const float* __restrict__ S, int64_t R, int64_t ld_s,
                                                               unsigned short* __restrict__ P, int64_t ld_p, float* __restrict__ lse,
                                                               int64_t row0, mask_key k) {
  constexpr int T = 256 * NV;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int n = CAUSAL ? (int)((row0 + row) % T) + 1 : T;   // visible columns 0 .. qi, quads 0 .. last
  const int qi = n - 1, last = qi >> 2;
  const float* s = S + row * ld_s;
  float4 v[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int q = lane + 64 * j;
    if constexpr (CAUSAL) {
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
    } else {
      v[j] = load_nt_f4(s + q * 4);
    }
  }
  const auto [m, sum] = softmax_row_reg<CAUSAL>(v, lane, last);
  const float inv = 1.0f / sum;
  if (lane == 0) lse[row] = lse2(m, sum);
  const int64_t quad0 = (row0 + row) * (64 * NV);   // T / 4 counters per row
  unsigned short* p = P + row * ld_p;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int q = lane + 64 * j;
    u16x4_t o = {0, 0, 0, 0};
    if (!CAUSAL || q <= last) {
      const uint4 w = words(k, quad0 + q);
      const int c = q * 4;
      o[0] = fwd(__fmul_rn(v[j].x, inv), w.x, k);
      o[1] = !CAUSAL || c + 1 <= qi ? fwd(__fmul_rn(v[j].y, inv), w.y, k) : (unsigned short)0;
      o[2] = !CAUSAL || c + 2 <= qi ? fwd(__fmul_rn(v[j].z, inv), w.z, k) : (unsigned short)0;
      o[3] = !CAUSAL || c + 3 <= qi ? fwd(__fmul_rn(v[j].w, inv), w.w, k) : (unsigned short)0;
    }
    *(u16x4_t*)(p + q * 4) = o;
  }
}

template <bool VEC, bool CAUSAL>
__global__ __launch_bounds__(256) void softmax_rows_walk_kernel(const float* __restrict__ S, int64_t R, int64_t T, int64_t ld_s,
                                                                unsigned short* __restrict__ P, int64_t T_pad, int64_t ld_p,
                                                                float* __restrict__ lse, int64_t row0, mask_key k) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t n = CAUSAL ? (row0 + row) % T + 1 : T, qi = n - 1;   // n visible columns
  const float* s = S + row * ld_s;
  const auto [m, sum] = softmax_row_walk(s, n, lane);
  const float inv = 1.0f / sum;
  if (lane == 0) lse[row] = lse2(m, sum);
  unsigned short* p = P + row * ld_p;
  const int64_t base = (row0 + row) * T;                // idx of the row's column 0
  const int64_t nq = CAUSAL ? (qi >> 2) + 1 : T >> 2;   // vec: the visible quads
  if constexpr (VEC) {
    const int64_t quad0 = base >> 2;   // T % 4 == 0: column 4 c4 starts counter quad0 + c4
    for (int64_t c4 = lane; c4 < nq; c4 += 64) {
      const float4 x = *(const float4*)(s + c4 * 4);
      const uint4 w = words(k, quad0 + c4);
      const int64_t c = c4 * 4;
      u16x4_t o;
      o[0] = fwd(__fmul_rn(__expf(x.x - m), inv), w.x, k);
      o[1] = !CAUSAL || c + 1 <= qi ? fwd(__fmul_rn(__expf(x.y - m), inv), w.y, k) : (unsigned short)0;
      o[2] = !CAUSAL || c + 2 <= qi ? fwd(__fmul_rn(__expf(x.z - m), inv), w.z, k) : (unsigned short)0;
      o[3] = !CAUSAL || c + 3 <= qi ? fwd(__fmul_rn(__expf(x.w - m), inv), w.w, k) : (unsigned short)0;
      *(u16x4_t*)(p + c4 * 4) = o;
    }
  } else {
    const int64_t q_last = (base + n - 1) >> 2;
    for (int64_t q = (base >> 2) + lane; q <= q_last; q += 64) {
      const uint4 o = words(k, q);
      const unsigned w[4] = {o.x, o.y, o.z, o.w};
      const int64_t c0 = q * 4 - base;   // -3 .. qi: column of the counter's first element
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t c = c0 + e;
        if (c >= 0 && c < n) p[c] = fwd(__fmul_rn(__expf(s[c] - m), inv), w[e], k);
      }
    }
  }
  if constexpr (CAUSAL) zero_fill(p, VEC ? nq * 4 : n, T_pad, lane);
  else for (int64_t i = T + lane; i < T_pad; i += 64) p[i] = (unsigned short)0;
}

// one element of the backward: P's bits, dPd, the element's word, negD of the row -> the bits of dS and Pd
struct bwd_pair {
  unsigned short ds, pd;
};
__device__ __forceinline__ bwd_pair bwd(unsigned short pb, float dp, unsigned word, float nd, float scale, const mask_key& k) {
  const bool keep = word >= k.thr;
  const float pf = bf16_to_f32(pb);
  const float g = keep ? __fmul_rn(dp, k.keep) : 0.f;   // m * dPd
  return {f32_to_bf16(pf * fmaf(scale, g, nd)), keep ? f32_to_bf16(__fmul_rn(pf, k.keep)) : (unsigned short)0};
}
// the same where the column is visible, +0.0 bits where it is not: whatever P and dPd hold there (inf, NaN) goes no further than the select
__device__ __forceinline__ bwd_pair bwd_if(bool visible, unsigned short pb, float dp, unsigned word, float nd, float scale, const mask_key& k) {
  const bwd_pair r = bwd(pb, dp, word, nd, scale, k);
  return {visible ? r.ds : (unsigned short)0, visible ? r.pd : (unsigned short)0};
}

// P and Pd may be the same buffer (no __restrict__ on either): a lane reads its elements of P before it writes them, no other lane touches
// them, and the zero fill covers columns nobody reads
template <bool VEC, bool CAUSAL>
__global__ __launch_bounds__(256) void softmax_rows_bwd_kernel(const unsigned short* P, const float* __restrict__ dPd,
                                                               const float* __restrict__ negD, int64_t R, int64_t T, int64_t T_pad, int64_t ld_p,
                                                               int64_t ld_dp, float scale, unsigned short* __restrict__ dS, int64_t ld_ds,
                                                               unsigned short* Pd, int64_t ld_pd, int64_t row0, mask_key k) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int64_t n = CAUSAL ? (row0 + row) % T + 1 : T, qi = n - 1;
  const unsigned short* p = P + row * ld_p;
  const float* dp = dPd + row * ld_dp;
  unsigned short* ds = dS + row * ld_ds;
  unsigned short* pd = Pd + row * ld_pd;
  const float nd = negD[row];
  const int64_t base = (row0 + row) * T;
  const int64_t nq = CAUSAL ? (qi >> 2) + 1 : T >> 2;
  if constexpr (VEC) {
    const int64_t quad0 = base >> 2;
    for (int64_t c4 = lane; c4 < nq; c4 += 64) {
      const u16x4_t pv = *(const u16x4_t*)(p + c4 * 4);
      const float4 dv = load_nt_f4(dp + c4 * 4);
      const uint4 w = words(k, quad0 + c4);
      const int64_t c = c4 * 4;
      const bwd_pair r0 = bwd(pv[0], dv.x, w.x, nd, scale, k), r1 = bwd_if(!CAUSAL || c + 1 <= qi, pv[1], dv.y, w.y, nd, scale, k);
      const bwd_pair r2 = bwd_if(!CAUSAL || c + 2 <= qi, pv[2], dv.z, w.z, nd, scale, k);
      const bwd_pair r3 = bwd_if(!CAUSAL || c + 3 <= qi, pv[3], dv.w, w.w, nd, scale, k);
      u16x4_t o, q;
      o[0] = r0.ds; o[1] = r1.ds; o[2] = r2.ds; o[3] = r3.ds;
      q[0] = r0.pd; q[1] = r1.pd; q[2] = r2.pd; q[3] = r3.pd;
      *(u16x4_t*)(ds + c4 * 4) = o;
      *(u16x4_t*)(pd + c4 * 4) = q;
    }
  } else {
    const int64_t q_last = (base + n - 1) >> 2;
    for (int64_t q = (base >> 2) + lane; q <= q_last; q += 64) {
      const uint4 o = words(k, q);
      const unsigned w[4] = {o.x, o.y, o.z, o.w};
      const int64_t c0 = q * 4 - base;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t c = c0 + e;
        if (c >= 0 && c < n) {
          const bwd_pair r = bwd(p[c], dp[c], w[e], nd, scale, k);
          ds[c] = r.ds;
          pd[c] = r.pd;
        }
      }
    }
  }
  if constexpr (CAUSAL) {
    zero_fill(ds, VEC ? nq * 4 : n, T_pad, lane);
    zero_fill(pd, VEC ? nq * 4 : n, T_pad, lane);
  } else {
    for (int64_t i = T + lane; i < T_pad; i += 64) {
      ds[i] = (unsigned short)0;
      pd[i] = (unsigned short)0;
    }
  }
}

bool aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p % bytes) == 0; }

mask_key make_key(uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site) {
  return {threshold, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)(site & 0xffffffffu), (unsigned)(site >> 32), scale_keep};
}

// the checks both directions share; name = the C entry point, which every error text begins with
int check_slab(const char* name, int64_t rows, int64_t T, int64_t T_pad, int64_t row0, float scale_keep) {
  TRIBE_REQUIRE(rows > 0 && T > 0 && rows < (1ll << 31) && T < (1ll << 31) && T_pad >= T && T_pad < (1ll << 31), "%s: rows=%lld T=%lld "
                "T_pad=%lld (need 0 < rows < 2^31, 0 < T <= T_pad < 2^31)", name, (long long)rows, (long long)T, (long long)T_pad);
  TRIBE_REQUIRE(row0 >= 0 && row0 < (1ll << 31), "%s: row0=%lld (need 0 <= row0 < 2^31)", name, (long long)row0);
  TRIBE_REQUIRE(scale_keep >= 1.f && scale_keep <= FLT_MAX, "%s: scale_keep = 1 / (1 - p) must be finite and >= 1, got %g", name, (double)scale_keep);
  return 0;
}

template <bool CAUSAL>
void launch_fwd(bool vec, bool reg, hipStream_t st, const float* S, uint16_t* Pd, float* lse, int64_t rows, int64_t T, int64_t T_pad, int64_t ld_s,
                int64_t ld_p, int64_t row0, mask_key k) {
  const dim3 grid((unsigned)((rows + 3) / 4));
  // NV: vec, T_pad == T and T = 256 / 512 / 1024 / 2048 -> the row in 1 / 2 / 4 / 8 float4 per lane; else a walk, 16 bytes at a time if vec
  if (reg && first_nv<1, 2, 4, 8>([&](int nv) { return T == 256 * nv; }, [&](auto nv) {
        hipLaunchKernelGGL((softmax_rows_reg_kernel<decltype(nv)::value, CAUSAL>), grid, dim3(256), 0, st, S, rows, ld_s, Pd, ld_p, lse, row0, k);
      }))
    return;
  if (vec) hipLaunchKernelGGL((softmax_rows_walk_kernel<true, CAUSAL>), grid, dim3(256), 0, st, S, rows, T, ld_s, Pd, T_pad, ld_p, lse, row0, k);
  else hipLaunchKernelGGL((softmax_rows_walk_kernel<false, CAUSAL>), grid, dim3(256), 0, st, S, rows, T, ld_s, Pd, T_pad, ld_p, lse, row0, k);
}

int softmax_rows_fwd(bool causal, const char* name, const float* S, uint16_t* Pd, float* lse, int64_t rows, int64_t T, int64_t T_pad, int64_t ld_s,
                     int64_t ld_p, int64_t row0, uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site, void* stream) {
  TRIBE_REQUIRE(S && Pd && lse, "%s: null pointer", name);
  if (check_slab(name, rows, T, T_pad, row0, scale_keep)) return -1;
  TRIBE_REQUIRE(ld_s >= T && ld_p >= T_pad && ld_s < (1ll << 40) && ld_p < (1ll << 40),
                "%s: ld_s=%lld ld_p=%lld (need ld_s >= T = %lld, ld_p >= T_pad = %lld)", name, (long long)ld_s, (long long)ld_p, (long long)T,
                (long long)T_pad);
  const mask_key k = make_key(threshold, scale_keep, seed, site);
  const bool vec = T % 4 == 0 && ld_s % 4 == 0 && ld_p % 4 == 0 && aligned(S, 16) && aligned(Pd, 8);
  const bool reg = vec && T_pad == T && T % 256 == 0 && T <= 2048;   // tribe_softmax_fwd's condition: the same summation order
  if (causal) launch_fwd<true>(vec, reg, (hipStream_t)stream, S, Pd, lse, rows, T, T_pad, ld_s, ld_p, row0, k);
  else launch_fwd<false>(vec, reg, (hipStream_t)stream, S, Pd, lse, rows, T, T_pad, ld_s, ld_p, row0, k);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

int softmax_rows_bwd(bool causal, const char* name, const uint16_t* P, const float* dPd, const float* negD, uint16_t* dS, uint16_t* Pd,
                     int64_t rows, int64_t T, int64_t T_pad, int64_t ld_p, int64_t ld_dp, int64_t ld_ds, int64_t ld_pd, float scale, int64_t row0,
                     uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site, void* stream) {
  TRIBE_REQUIRE(P && dPd && negD && dS && Pd, "%s: null pointer", name);
  if (check_slab(name, rows, T, T_pad, row0, scale_keep)) return -1;
  TRIBE_REQUIRE(ld_p >= T_pad && ld_dp >= T && ld_ds >= T_pad && ld_pd >= T_pad && ld_p < (1ll << 40) && ld_dp < (1ll << 40) &&
                    ld_ds < (1ll << 40) && ld_pd < (1ll << 40),
                "%s: ld_p=%lld ld_dp=%lld ld_ds=%lld ld_pd=%lld (need ld_dp >= T = %lld, the others >= T_pad = %lld)", name, (long long)ld_p,
                (long long)ld_dp, (long long)ld_ds, (long long)ld_pd, (long long)T, (long long)T_pad);
  TRIBE_REQUIRE((const void*)dS != (const void*)P && dS != Pd, "%s: dS must not be P or Pd", name);
  TRIBE_REQUIRE((const void*)Pd != (const void*)P || ld_pd == ld_p, "%s: in place (Pd == P) needs ld_pd == ld_p", name);
  const mask_key k = make_key(threshold, scale_keep, seed, site);
  const bool vec = T % 4 == 0 && ld_p % 4 == 0 && ld_dp % 4 == 0 && ld_ds % 4 == 0 && ld_pd % 4 == 0 && aligned(P, 8) && aligned(dPd, 16) &&
                   aligned(dS, 8) && aligned(Pd, 8);
  static constexpr decltype(&softmax_rows_bwd_kernel<false, false>) kernels[2][2] = {   // [causal][vec]: one signature
      {softmax_rows_bwd_kernel<false, false>, softmax_rows_bwd_kernel<true, false>},
      {softmax_rows_bwd_kernel<false, true>, softmax_rows_bwd_kernel<true, true>}};
  hipLaunchKernelGGL(kernels[causal][vec], dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, P, dPd, negD, rows, T, T_pad, ld_p,
                     ld_dp, scale, dS, ld_ds, Pd, ld_pd, row0, k);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int tribe_softmax_dropout_fwd(const float* S, uint16_t* Pd, float* lse, int64_t rows, int64_t T, int64_t T_pad, int64_t ld_s,
                                         int64_t ld_p, int64_t row0, uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site,
                                         void* stream) {
  return softmax_rows_fwd(false, "tribe_softmax_dropout_fwd", S, Pd, lse, rows, T, T_pad, ld_s, ld_p, row0, threshold, scale_keep, seed, site, stream);
}
extern "C" int tribe_softmax_dropout_bwd(const uint16_t* P, const float* dPd, const float* negD, uint16_t* dS, uint16_t* Pd, int64_t rows,
                                         int64_t T, int64_t T_pad, int64_t ld_p, int64_t ld_dp, int64_t ld_ds, int64_t ld_pd, float scale,
                                         int64_t row0, uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site, void* stream) {
  return softmax_rows_bwd(false, "tribe_softmax_dropout_bwd", P, dPd, negD, dS, Pd, rows, T, T_pad, ld_p, ld_dp, ld_ds, ld_pd, scale, row0,
                          threshold, scale_keep, seed, site, stream);
}
extern "C" int tribe_softmax_causal_fwd(const float* S, uint16_t* Pd, float* lse, int64_t rows, int64_t T, int64_t T_pad, int64_t ld_s,
                                        int64_t ld_p, int64_t row0, uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site,
                                        void* stream) {
  return softmax_rows_fwd(true, "tribe_softmax_causal_fwd", S, Pd, lse, rows, T, T_pad, ld_s, ld_p, row0, threshold, scale_keep, seed, site, stream);
}
extern "C" int tribe_softmax_causal_bwd(const uint16_t* P, const float* dPd, const float* negD, uint16_t* dS, uint16_t* Pd, int64_t rows,
                                        int64_t T, int64_t T_pad, int64_t ld_p, int64_t ld_dp, int64_t ld_ds, int64_t ld_pd, float scale,
                                        int64_t row0, uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site, void* stream) {
  return softmax_rows_bwd(true, "tribe_softmax_causal_bwd", P, dPd, negD, dS, Pd, rows, T, T_pad, ld_p, ld_dp, ld_ds, ld_pd, scale, row0,
                          threshold, scale_keep, seed, site, stream);
}
