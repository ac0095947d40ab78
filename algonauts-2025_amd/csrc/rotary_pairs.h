// The pair rotation of the partial rotary embedding, stated once: rotary_kernel (elementwise.hip, whole buffers) and kv_append_kernel
// (attn_decode.hip, one position of a streamed encoder) call the same two functions, so a position gets the same bits from either.
#pragma once
#include "common.h"

// four interleaved pairs (2p, 2p + 1) of one 16-byte piece; cs / sn: the four angles' cosines and sines
__device__ __forceinline__ void rotate_interleaved8(u16x8_t& v, const float cs[4], const float sn[4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float a = bf16_to_f32(v[2 * p]), b = bf16_to_f32(v[2 * p + 1]);
    v[2 * p] = f32_to_bf16(a * cs[p] - b * sn[p]);
    v[2 * p + 1] = f32_to_bf16(b * cs[p] + a * sn[p]);
  }
}

// four half-split pairs (i, i + rot_dim / 2): lo holds elements i .. i + 3, hi their partners
__device__ __forceinline__ void rotate_split4(u16x4_t& lo, u16x4_t& hi, const float cs[4], const float sn[4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float a = bf16_to_f32(lo[p]), b = bf16_to_f32(hi[p]);
    lo[p] = f32_to_bf16(a * cs[p] - b * sn[p]);
    hi[p] = f32_to_bf16(b * cs[p] + a * sn[p]);
  }
}
