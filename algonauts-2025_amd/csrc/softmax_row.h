// The row statistics of the softmax kernels that give one wave a row: maximum -> exp -> sum, stated once so that tribe_softmax_fwd
// (elementwise.hip) and the softmax-dropout / causal row kernels of the training path (attn_softmax.hip) share their bits.  The order in
// which a lane and then the wave add is part of the contract.  All 64 lanes of the wave call; the result is wave-uniform.
#pragma once
#include "common.h"

struct softmax_row_stat {
  float m, sum;   // the row maximum and sum exp(s - m)
};

// Registers form: lane l holds quads l + 64 j of a row of 256 NV columns in v[j].  On return v holds exp(v - m); a lane adds
// (x + y) + (z + w) per quad in the order of j, then wave_sum.  LIMIT (a causal row): `last` is the last visible quad; the quads beyond it
// hold -inf, stay as they are and are left out of the sum, where they would add exact zeros.
// (softmax_reg_kernel in elementwise.hip states the LIMIT = false form itself, to keep its machine code.)
template <bool LIMIT = false, int NV>
__device__ __forceinline__ softmax_row_stat softmax_row_reg(float4 (&v)[NV], int lane, int last = 0) {
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < NV; ++j) m = fmaxf(m, fmaxf(fmaxf(v[j].x, v[j].y), fmaxf(v[j].z, v[j].w)));
  m = wave_max(m);
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    if (!LIMIT || lane + 64 * j <= last) {   // (a masked element of the diagonal's quad: exp(-inf - m) = +0.0)
      v[j].x = __expf(v[j].x - m); v[j].y = __expf(v[j].y - m); v[j].z = __expf(v[j].z - m); v[j].w = __expf(v[j].w - m);
      sum += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    }
  }
  return {m, wave_sum(sum)};
}

// Walk form: lane l takes columns l + 64 k of the first n columns of s, once for the maximum and once for sum exp(s - m).
__device__ __forceinline__ softmax_row_stat softmax_row_walk(const float* s, int64_t n, int lane) {
  float m = -INFINITY;
  for (int64_t i = lane; i < n; i += 64) m = fmaxf(m, s[i]);
  m = wave_max(m);
  float sum = 0.f;
  for (int64_t i = lane; i < n; i += 64) sum += __expf(s[i] - m);
  return {m, wave_sum(sum)};
}
