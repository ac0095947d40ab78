// One wave per row: the vocabulary of the row kernels (ScaleNorm and RMSNorm / LayerNorm in elementwise.hip, LayerNorm + activation in
// mlp.hip).  A workgroup is four waves, row = blockIdx.x * 4 + wave, and lane l owns the quads (four neighbouring columns) l + 64 j of
// its row.  A kernel is written once over quads_each / row_each and compiled per form:
//   NV > 0    the row sits in NV float4 per lane (row_load): memory is read once, every load of the row is in flight at once
//   NV == 0   a walk over memory per pass, 16 bytes or (row_each without VEC) one element at a time
// Per lane the passes visit the quads in the order of j either way, so one body gives each form the additions of its own order.
#pragma once
#include <type_traits>

#include "common.h"

// f(first column, values, register slot) over this lane's share of a row: NV > 0 -- the row as NV float4 per lane in `v` (columns
// 4 * (lane + 64 j)); NV == 0 -- a walk over memory, 16 bytes (VEC) or one element at a time.  Without VEC only .x of the values counts.
template <int NV, bool VEC, class F>
__device__ __forceinline__ void row_each(const float* zr, const float4* v, int64_t dim, int lane, F f) {
  if constexpr (NV > 0) {
    const int n4 = (int)(dim >> 2);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = lane + 64 * j;
      if (i < n4) f((int64_t)i * 4, v[j], j);
    }
  } else if constexpr (VEC) {
    const int64_t n4 = dim >> 2;
    for (int64_t i = lane; i < n4; i += 64) f(i * 4, *(const float4*)(zr + i * 4), 0);
  } else {
    for (int64_t c = lane; c < dim; c += 64) f(c, make_float4(zr[c], 0.f, 0.f, 0.f), 0);
  }
}
template <int NV>
__device__ __forceinline__ void row_load(const float* zr, float4* v, int64_t dim, int lane) {
  const int n4 = (int)(dim >> 2);
#pragma unroll
  for (int j = 0; j < (NV > 0 ? NV : 1); ++j) {
    const int i = lane + 64 * j;
    v[j] = (NV > 0 && i < n4) ? *(const float4*)(zr + (int64_t)i * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// row_load and row_each for rows that are whole quads: f(index of the quad in its row, quad, register slot).  The index is an int where
// the row sits in registers and an int64_t in a walk, and memory is indexed with it as it comes (quads_load, load4, store4), so that
// every access folds its own constant part into the instruction.  f takes the quad by reference, and the register row is filled by
// plain copies of memory: hipcc decides from the way a quad reaches a reduction which of its products it contracts into FMAs, and so
// what bits the sum has.  FULL: the kernel knows dim == 256 * NV -- every slot of every lane is a quad of the row, and none is guarded.
// (Not row_load / row_each with a FULL switch: whatever changes the index row_each hands out or the way row_load addresses the row --
// tried: the quad index, an int column, float4 indexing -- changes the machine code of mlp.hip's kernels, which take the first column.)
template <int NV, bool FULL = false>
__device__ __forceinline__ void quads_load(const float* zr, float4* v, int64_t dim, int lane) {
  const int n4 = (int)(dim >> 2);
#pragma unroll
  for (int j = 0; j < (NV > 0 ? NV : 1); ++j) {
    const int i = lane + 64 * j;
    if constexpr (NV > 0 && FULL) v[j] = ((const float4*)zr)[i];
    else v[j] = (NV > 0 && i < n4) ? ((const float4*)zr)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
template <int NV, bool FULL = false, class F>
__device__ __forceinline__ void quads_each(const float* zr, const float4* v, int64_t dim, int lane, F f) {
  if constexpr (NV > 0) {
    const int n4 = (int)(dim >> 2);
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const int i = lane + 64 * j;
      if (FULL || i < n4) f(i, v[j], j);
    }
  } else {
    const int64_t n4 = dim >> 2;
    for (int64_t i = lane; i < n4; i += 64) f(i, ((const float4*)zr)[i], 0);
  }
}
// quad q of the f32 row at p
template <class Q>
__device__ __forceinline__ const float4& load4(const float* p, Q q) { return ((const float4*)p)[q]; }
// o as quad q of the row at y, in the format OUT = 0: f32, 1: bf16, 2: e4m3 bytes of the bf16-rounded values times q_inv_scale
// (saturating, NaN passed through: pack_e4m3x4)
template <int OUT, class Q>
__device__ __forceinline__ void store4(void* y, Q q, const float4& o, float q_inv_scale = 0.f) {
  if constexpr (OUT == 2) {
    float r[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = bf16_to_f32(f32_to_bf16(r[k])) * q_inv_scale;
    ((int*)y)[q] = pack_e4m3x4(r[0], r[1], r[2], r[3]);
  } else if constexpr (OUT == 1) {
    u16x4_t h;
    h[0] = f32_to_bf16(o.x); h[1] = f32_to_bf16(o.y); h[2] = f32_to_bf16(o.z); h[3] = f32_to_bf16(o.w);
    ((u16x4_t*)y)[q] = h;
  } else {
    ((f32x4_t*)y)[q] = f32x4_t{o.x, o.y, o.z, o.w};   // one 16-byte store wherever this is inlined
  }
}
// row `row` of y [rows, dim] in the format OUT
template <int OUT>
__device__ __forceinline__ void* out_row(void* y, int64_t row, int64_t dim) {
  return (char*)y + row * dim * (OUT == 0 ? 4 : (OUT == 1 ? 2 : 1));
}
// what a quad adds to a lane's running sum of products: its four in element order, ((ax bx + ay by) + az bz) + aw bw
__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// Host side, which form to launch: f(std::integral_constant<int, NV>) for the first NV of the list that fits(NV); false if none does.
template <int... NVS, class P, class F>
inline bool first_nv(P fits, F f) {
  return ((fits(NVS) && (f(std::integral_constant<int, NVS>{}), true)) || ...);
}
