// The LDS sort shared by the rank-correlation kernels (rank_corr.hip) and the bootstrap summary (bootstrap.hip): the
// order-preserving map of f32 bits to u32 keys, its inverse, and an ascending bitonic sort of one or two key arrays held in LDS.
//
// The network's strides j >= 64 run as LDS passes in which lane l of a wave touches dwords base + l and base + j + l (consecutive
// lanes, consecutive banks: conflict-free for ds_read_b32 / ds_write_b32, which bank per 32-lane half); the strides j <= 32, whose
// LDS form would put two lanes of a half on one bank, never touch LDS: a wave loads 64 consecutive keys, one per lane, and exchanges
// through __shfl_xor.
#pragma once
#include "common.h"

namespace {

constexpr unsigned RC_PAD = 0xffffffffu;     // above every key of a non-NaN value (+inf -> 0xff800000)

__device__ __forceinline__ unsigned key_of(float x) {
  unsigned b = __float_as_uint(x);
  if (b == 0x80000000u) b = 0u;   // -0.0 ties with +0.0
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

// the value of a key (the inverse of key_of, except that -0.0 comes back as +0.0)
__device__ __forceinline__ float value_of(unsigned k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

// the strides jmax .. 1 (jmax <= 32) of phase k for the key at index i, one key per lane of a wave
__device__ __forceinline__ unsigned wave_exchange(unsigned v, int i, int k, int jmax) {
  const bool up = (i & k) == 0;
  for (int j = jmax; j > 0; j >>= 1) {
    const unsigned o = __shfl_xor(v, j, 64);
    const bool low = (i & j) == 0;
    v = (low == up) ? min(v, o) : max(v, o);
  }
  return v;
}

// Ascending bitonic sort of s0[0..P) and, when s1 != nullptr, s1[0..P): P a power of two >= 64, blockDim.x a multiple of 64, every
// thread of the workgroup calls it after a barrier that made the keys visible.  Ends with a barrier.
__device__ __forceinline__ void block_sort(unsigned* s0, unsigned* s1, int P) {
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int i = tid; i < P; i += nt) {   // phases k = 2 .. 64: whole waves, each on its own 64 keys
    unsigned a = s0[i], b = s1 ? s1[i] : 0u;
    for (int k = 2; k <= 64; k <<= 1) {
      a = wave_exchange(a, i, k, k >> 1);
      if (s1) b = wave_exchange(b, i, k, k >> 1);
    }
    s0[i] = a;
    if (s1) s1[i] = b;
  }
  __syncthreads();
  for (int k = 128; k <= P; k <<= 1) {
    for (int j = k >> 1; j >= 64; j >>= 1) {
      for (int t = tid; t < (P >> 1); t += nt) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const bool up = (lo & k) == 0;
        const unsigned a = s0[lo], b = s0[hi];
        if ((a > b) == up) { s0[lo] = b; s0[hi] = a; }
        if (s1) {
          const unsigned c = s1[lo], d = s1[hi];
          if ((c > d) == up) { s1[lo] = d; s1[hi] = c; }
        }
      }
      __syncthreads();
    }
    for (int i = tid; i < P; i += nt) {
      s0[i] = wave_exchange(s0[i], i, k, 32);
      if (s1) s1[i] = wave_exchange(s1[i], i, k, 32);
    }
    __syncthreads();
  }
}

}  // namespace
