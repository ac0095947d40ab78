// Attention dropout of the training path (modeling_utils.autograd.Attention with p > 0): the two row kernels around the materialised scores.
//   tribe_softmax_dropout_fwd   S f32 [rows, T] -> Pd = bf16(softmax(S) * m) [rows, T_pad] (pad columns zero) and lse2 f32 [rows]
//   tribe_softmax_dropout_bwd   P bf16, dPd f32, negD f32 [rows] -> dS = bf16(P * (scale * (m * dPd) + negD)), and Pd = bf16(P * m) over P
// m is the mask factor of tribe_dropout_apply (dropout.hip) on the LOGICAL tensor [row0 + rows, T]: element (r, j) of the slab has
// idx = (row0 + r) * T + j (64-bit; from T, never from a pitch or T_pad), its word is word idx & 3 of Philox4x32-10 (philox.h) with counter
// (lo32(idx >> 2), hi32(idx >> 2), lo32(site), hi32(site)) and key (lo32(seed), hi32(seed)); kept iff word >= threshold; kept values are
// multiplied by scale_keep in f32 with one rounding (__fmul_rn), dropped ones are +0.0 by a select.  No mask tensor exists: both kernels
// draw it in registers, one Philox call per four consecutive idx.  row0 makes the mask independent of how the caller chunks the batch.
//
// One wave per row, four rows per 256-thread workgroup (as softmax_kernel / softmax_bwd_kernel).  The softmax arithmetic -- and the order of
// its row sum -- is that of tribe_softmax_fwd on the same arguments, so threshold = 0, scale_keep = 1 reproduces its bits:
//   reg   T = 256 NV (NV = 1, 2, 4, 8), T_pad == T, pitches % 4 == 0, S 16-byte / P 8-byte aligned: the row in registers, 16-byte loads,
//         8-byte stores, lane l holds quads l + 64 j of the row (row starts are quad-aligned: T % 4 == 0)
//   walk  every other shape: maximum and sum by lanes striding over elements (softmax_kernel's order); the store pass goes by quads:
//         vec (T % 4 == 0 and the alignments above): the row's quads start at its column 0, 16-byte loads / 8-byte stores;
//         elem: lane l takes the counters (first idx of the row >> 2) + l + 64 k and writes whichever of their four elements lie in the
//         row -- a quad that straddles a row end is drawn by both rows (at most two extra calls per row).
// The backward has no row reduction (D comes in from tribe_rowdot_heads_bf16): vec / elem as above.  No atomics; bit-reproducible.
#include <float.h>

#include "common.h"
#include "philox.h"

namespace {

constexpr float SD_LOG2E = 1.4426950408889634f;

struct sd_key {
  unsigned thr, k0, k1, s0, s1;
  float keep;
};

__device__ __forceinline__ uint4 sd_words(const sd_key& k, int64_t quad) {
  return philox4x32_10(make_uint4((unsigned)((uint64_t)quad & 0xffffffffu), (unsigned)((uint64_t)quad >> 32), k.s0, k.s1), k.k0, k.k1);
}
// p = softmax value (f32) -> the bf16 of Pd
__device__ __forceinline__ unsigned short sd_fwd(float p, unsigned word, const sd_key& k) {
  return word >= k.thr ? f32_to_bf16(__fmul_rn(p, k.keep)) : (unsigned short)0;
}
// base-2 log-sum-exp of a row with maximum m and sum = sum exp(s - m): what ACT_EXP2 subtracts from scale log2e q.k
__device__ __forceinline__ float sd_lse2(float m, float sum) { return fmaf(m, SD_LOG2E, __log2f(sum)); }

template <int NV>
__global__ __launch_bounds__(256) void softmax_dropout_reg_kernel(const float* __restrict__ S, int64_t R, int64_t ld_s,
                                                                  unsigned short* __restrict__ P, int64_t ld_p, float* __restrict__ lse,
                                                                  int64_t row0, sd_key k) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* s = S + row * ld_s;
  float4 v[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) v[j] = load_nt_f4(s + (lane + 64 * j) * 4);
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < NV; ++j) m = fmaxf(m, fmaxf(fmaxf(v[j].x, v[j].y), fmaxf(v[j].z, v[j].w)));
  m = wave_max(m);
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    v[j].x = __expf(v[j].x - m); v[j].y = __expf(v[j].y - m); v[j].z = __expf(v[j].z - m); v[j].w = __expf(v[j].w - m);
    sum += (v[j].x + v[j].y) + (v[j].z + v[j].w);
  }
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  if (lane == 0) lse[row] = sd_lse2(m, sum);
  const int64_t quad0 = (row0 + row) * (64 * NV);   // T / 4 counters per row
  unsigned short* p = P + row * ld_p;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const uint4 w = sd_words(k, quad0 + lane + 64 * j);
    u16x4_t o;
    o[0] = sd_fwd(__fmul_rn(v[j].x, inv), w.x, k); o[1] = sd_fwd(__fmul_rn(v[j].y, inv), w.y, k);
    o[2] = sd_fwd(__fmul_rn(v[j].z, inv), w.z, k); o[3] = sd_fwd(__fmul_rn(v[j].w, inv), w.w, k);
    *(u16x4_t*)(p + (lane + 64 * j) * 4) = o;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void softmax_dropout_walk_kernel(const float* __restrict__ S, int64_t R, int64_t T, int64_t ld_s,
                                                                   unsigned short* __restrict__ P, int64_t T_pad, int64_t ld_p,
                                                                   float* __restrict__ lse, int64_t row0, sd_key k) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* s = S + row * ld_s;
  float m = -INFINITY;
  for (int64_t i = lane; i < T; i += 64) m = fmaxf(m, s[i]);
  m = wave_max(m);
  float sum = 0.f;
  for (int64_t i = lane; i < T; i += 64) sum += __expf(s[i] - m);
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  if (lane == 0) lse[row] = sd_lse2(m, sum);
  unsigned short* p = P + row * ld_p;
  const int64_t base = (row0 + row) * T;   // idx of the row's column 0
  if constexpr (VEC) {
    const int64_t quad0 = base >> 2, nq = T >> 2;   // T % 4 == 0: column 4 c4 starts counter quad0 + c4
    for (int64_t c4 = lane; c4 < nq; c4 += 64) {
      const float4 x = *(const float4*)(s + c4 * 4);
      const uint4 w = sd_words(k, quad0 + c4);
      u16x4_t o;
      o[0] = sd_fwd(__fmul_rn(__expf(x.x - m), inv), w.x, k); o[1] = sd_fwd(__fmul_rn(__expf(x.y - m), inv), w.y, k);
      o[2] = sd_fwd(__fmul_rn(__expf(x.z - m), inv), w.z, k); o[3] = sd_fwd(__fmul_rn(__expf(x.w - m), inv), w.w, k);
      *(u16x4_t*)(p + c4 * 4) = o;
    }
  } else {
    const int64_t q_last = (base + T - 1) >> 2;
    for (int64_t q = (base >> 2) + lane; q <= q_last; q += 64) {
      const uint4 o = sd_words(k, q);
      const unsigned w[4] = {o.x, o.y, o.z, o.w};
      const int64_t c0 = q * 4 - base;   // -3 .. T - 1: column of the counter's first element
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t c = c0 + e;
        if (c >= 0 && c < T) p[c] = sd_fwd(__fmul_rn(__expf(s[c] - m), inv), w[e], k);
      }
    }
  }
  for (int64_t i = T + lane; i < T_pad; i += 64) p[i] = (unsigned short)0;
}

// one element of the backward: P's bits, dPd, the element's word, negD of the row -> the bits of dS and Pd
struct sd_pair {
  unsigned short ds, pd;
};
__device__ __forceinline__ sd_pair sd_bwd(unsigned short pb, float dp, unsigned word, float nd, float scale, const sd_key& k) {
  const bool keep = word >= k.thr;
  const float pf = bf16_to_f32(pb);
  const float g = keep ? __fmul_rn(dp, k.keep) : 0.f;   // m * dPd
  return {f32_to_bf16(pf * fmaf(scale, g, nd)), keep ? f32_to_bf16(__fmul_rn(pf, k.keep)) : (unsigned short)0};
}

// P and Pd may be the same buffer (no __restrict__ on either): a lane reads its elements of P before it writes them and no other lane
// touches them
template <bool VEC>
__global__ __launch_bounds__(256) void softmax_dropout_bwd_kernel(const unsigned short* P, const float* __restrict__ dPd,
                                                                  const float* __restrict__ negD, int64_t R, int64_t T, int64_t T_pad, int64_t ld_p,
                                                                  int64_t ld_dp, float scale, unsigned short* __restrict__ dS, int64_t ld_ds,
                                                                  unsigned short* Pd, int64_t ld_pd, int64_t row0, sd_key k) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const unsigned short* p = P + row * ld_p;
  const float* dp = dPd + row * ld_dp;
  unsigned short* ds = dS + row * ld_ds;
  unsigned short* pd = Pd + row * ld_pd;
  const float nd = negD[row];
  const int64_t base = (row0 + row) * T;
  if constexpr (VEC) {
    const int64_t quad0 = base >> 2, nq = T >> 2;
    for (int64_t c4 = lane; c4 < nq; c4 += 64) {
      const u16x4_t pv = *(const u16x4_t*)(p + c4 * 4);
      const float4 dv = load_nt_f4(dp + c4 * 4);
      const uint4 w = sd_words(k, quad0 + c4);
      const sd_pair r0 = sd_bwd(pv[0], dv.x, w.x, nd, scale, k), r1 = sd_bwd(pv[1], dv.y, w.y, nd, scale, k);
      const sd_pair r2 = sd_bwd(pv[2], dv.z, w.z, nd, scale, k), r3 = sd_bwd(pv[3], dv.w, w.w, nd, scale, k);
      u16x4_t o, q;
      o[0] = r0.ds; o[1] = r1.ds; o[2] = r2.ds; o[3] = r3.ds;
      q[0] = r0.pd; q[1] = r1.pd; q[2] = r2.pd; q[3] = r3.pd;
      *(u16x4_t*)(ds + c4 * 4) = o;
      *(u16x4_t*)(pd + c4 * 4) = q;
    }
  } else {
    const int64_t q_last = (base + T - 1) >> 2;
    for (int64_t q = (base >> 2) + lane; q <= q_last; q += 64) {
      const uint4 o = sd_words(k, q);
      const unsigned w[4] = {o.x, o.y, o.z, o.w};
      const int64_t c0 = q * 4 - base;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t c = c0 + e;
        if (c >= 0 && c < T) {
          const sd_pair r = sd_bwd(p[c], dp[c], w[e], nd, scale, k);
          ds[c] = r.ds;
          pd[c] = r.pd;
        }
      }
    }
  }
  for (int64_t i = T + lane; i < T_pad; i += 64) {
    ds[i] = (unsigned short)0;
    pd[i] = (unsigned short)0;
  }
}

bool sd_aligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p % bytes) == 0; }

sd_key make_key(uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site) {
  return {threshold, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)(site & 0xffffffffu), (unsigned)(site >> 32), scale_keep};
}

}  // namespace

#define TRIBE_SD_SHAPE(name)                                                                                                              \
  TRIBE_REQUIRE(rows > 0 && T > 0 && rows < (1ll << 31) && T < (1ll << 31) && T_pad >= T && T_pad < (1ll << 31), name ": rows=%lld T=%lld " \
                "T_pad=%lld (need 0 < rows < 2^31, 0 < T <= T_pad < 2^31)", (long long)rows, (long long)T, (long long)T_pad);              \
  TRIBE_REQUIRE(row0 >= 0 && row0 < (1ll << 31), name ": row0=%lld (need 0 <= row0 < 2^31)", (long long)row0);                             \
  TRIBE_REQUIRE(scale_keep >= 1.f && scale_keep <= FLT_MAX, name ": scale_keep = 1 / (1 - p) must be finite and >= 1, got %g", (double)scale_keep)

extern "C" int tribe_softmax_dropout_fwd(const float* S, uint16_t* Pd, float* lse, int64_t rows, int64_t T, int64_t T_pad, int64_t ld_s,
                                         int64_t ld_p, int64_t row0, uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site,
                                         void* stream) {
  TRIBE_REQUIRE(S && Pd && lse, "tribe_softmax_dropout_fwd: null pointer");
  TRIBE_SD_SHAPE("tribe_softmax_dropout_fwd");
  TRIBE_REQUIRE(ld_s >= T && ld_p >= T_pad && ld_s < (1ll << 40) && ld_p < (1ll << 40),
                "tribe_softmax_dropout_fwd: ld_s=%lld ld_p=%lld (need ld_s >= T = %lld, ld_p >= T_pad = %lld)", (long long)ld_s, (long long)ld_p,
                (long long)T, (long long)T_pad);
  const sd_key k = make_key(threshold, scale_keep, seed, site);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((rows + 3) / 4));
  const bool vec = T % 4 == 0 && ld_s % 4 == 0 && ld_p % 4 == 0 && sd_aligned(S, 16) && sd_aligned(Pd, 8);
  const bool reg = vec && T_pad == T && T % 256 == 0 && T <= 2048;   // tribe_softmax_fwd's condition: the same summation order
  if (reg && T == 256) hipLaunchKernelGGL(softmax_dropout_reg_kernel<1>, grid, dim3(256), 0, st, S, rows, ld_s, Pd, ld_p, lse, row0, k);
  else if (reg && T == 512) hipLaunchKernelGGL(softmax_dropout_reg_kernel<2>, grid, dim3(256), 0, st, S, rows, ld_s, Pd, ld_p, lse, row0, k);
  else if (reg && T == 1024) hipLaunchKernelGGL(softmax_dropout_reg_kernel<4>, grid, dim3(256), 0, st, S, rows, ld_s, Pd, ld_p, lse, row0, k);
  else if (reg && T == 2048) hipLaunchKernelGGL(softmax_dropout_reg_kernel<8>, grid, dim3(256), 0, st, S, rows, ld_s, Pd, ld_p, lse, row0, k);
  else if (vec) hipLaunchKernelGGL(softmax_dropout_walk_kernel<true>, grid, dim3(256), 0, st, S, rows, T, ld_s, Pd, T_pad, ld_p, lse, row0, k);
  else hipLaunchKernelGGL(softmax_dropout_walk_kernel<false>, grid, dim3(256), 0, st, S, rows, T, ld_s, Pd, T_pad, ld_p, lse, row0, k);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_softmax_dropout_bwd(const uint16_t* P, const float* dPd, const float* negD, uint16_t* dS, uint16_t* Pd, int64_t rows,
                                         int64_t T, int64_t T_pad, int64_t ld_p, int64_t ld_dp, int64_t ld_ds, int64_t ld_pd, float scale,
                                         int64_t row0, uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site, void* stream) {
  TRIBE_REQUIRE(P && dPd && negD && dS && Pd, "tribe_softmax_dropout_bwd: null pointer");
  TRIBE_SD_SHAPE("tribe_softmax_dropout_bwd");
  TRIBE_REQUIRE(ld_p >= T_pad && ld_dp >= T && ld_ds >= T_pad && ld_pd >= T_pad && ld_p < (1ll << 40) && ld_dp < (1ll << 40) &&
                    ld_ds < (1ll << 40) && ld_pd < (1ll << 40),
                "tribe_softmax_dropout_bwd: ld_p=%lld ld_dp=%lld ld_ds=%lld ld_pd=%lld (need ld_dp >= T = %lld, the others >= T_pad = %lld)",
                (long long)ld_p, (long long)ld_dp, (long long)ld_ds, (long long)ld_pd, (long long)T, (long long)T_pad);
  TRIBE_REQUIRE((const void*)dS != (const void*)P && dS != Pd, "tribe_softmax_dropout_bwd: dS must not be P or Pd");
  TRIBE_REQUIRE((const void*)Pd != (const void*)P || ld_pd == ld_p, "tribe_softmax_dropout_bwd: in place (Pd == P) needs ld_pd == ld_p");
  const sd_key k = make_key(threshold, scale_keep, seed, site);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((rows + 3) / 4));
  const bool vec = T % 4 == 0 && ld_p % 4 == 0 && ld_dp % 4 == 0 && ld_ds % 4 == 0 && ld_pd % 4 == 0 && sd_aligned(P, 8) && sd_aligned(dPd, 16) &&
                   sd_aligned(dS, 8) && sd_aligned(Pd, 8);
  if (vec)
    hipLaunchKernelGGL(softmax_dropout_bwd_kernel<true>, grid, dim3(256), 0, st, P, dPd, negD, rows, T, T_pad, ld_p, ld_dp, scale, dS, ld_ds, Pd,
                       ld_pd, row0, k);
  else
    hipLaunchKernelGGL(softmax_dropout_bwd_kernel<false>, grid, dim3(256), 0, st, P, dPd, negD, rows, T, T_pad, ld_p, ld_dp, scale, dS, ld_ds, Pd,
                       ld_pd, row0, k);
  TRIBE_LAUNCH_CHECK();
  return 0;
}
