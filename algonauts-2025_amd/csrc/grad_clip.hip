// Gradient clipping in front of the optimiser step (torch.nn.utils.clip_grad_norm_ / clip_grad_value_; Lightning's gradient_clip_val).
// Same table / work list as Adam (backward.hip): only table[i].g and table[i].n are read.
//   tribe_grad_norm   one streaming read (4 B per parameter) -> {total norm, clip coefficient} in device memory, f64 accumulation in a
//                     fixed order (no atomics: equal inputs give equal bits), two launches
//   tribe_grad_scale  g = clamp(g * coef, +-clip_value) in place (8 B per parameter)
// The fused form, tribe_adam_step_clipped, applies the same arithmetic (clip_grad, common.h) as the Adam kernel loads each gradient.
#include "common.h"

namespace {

enum { NORM_L2 = 0, NORM_MAX = 1 };

// L2: running sum of squares.  Max-abs: running maximum that KEEPS a NaN (fmax would drop it): once either side is NaN the result is.
template <int KIND>
__device__ __forceinline__ double norm_combine(double a, double b) {
  if (KIND == NORM_L2) return a + b;
  return (b > a || b != b) ? b : a;
}
template <int KIND>
__device__ __forceinline__ double norm_take(double acc, float g) {
  const double d = (double)g;                        // an f32 square is exact in f64 (48 significant bits)
  if (KIND == NORM_L2) return fma(d, d, acc);
  return norm_combine<NORM_MAX>(acc, fabs(d));
}
// butterfly over the wave, then the waves' values in index order: a fixed tree; every thread returns the total
template <int KIND>
__device__ __forceinline__ double norm_block_reduce(double v, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = norm_combine<KIND>(v, __shfl_xor(v, off, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = sh[0];
  for (int i = 1; i < (int)(blockDim.x >> 6); ++i) t = norm_combine<KIND>(t, sh[i]);
  return t;
}

// launch 1: workgroup c reduces chunk c to partials[c]
template <int KIND>
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const tribe_adam_tensor* __restrict__ table, const int32_t* __restrict__ chunk_tensor,
                                                                const int64_t* __restrict__ chunk_start, double* __restrict__ partials) {
  __shared__ double sh[4];
  const tribe_adam_tensor t = table[chunk_tensor[blockIdx.x]];
  const int64_t i0 = chunk_start[blockIdx.x];
  const int64_t i1 = (i0 + ADAM_CHUNK < t.n) ? i0 + ADAM_CHUNK : t.n;
  const bool vec = (((uintptr_t)t.g) & 15) == 0 && (i0 & 3) == 0;
  double acc = 0.0;
  int64_t done = i0;
  if (vec) {
    const float4* g4 = (const float4*)(t.g + i0);
    const int64_t n4 = (i1 - i0) / 4;
    int64_t q = threadIdx.x;
    for (; q + 768 < n4; q += 1024) {                // four 16-byte loads requested before the first is used
      float4 g[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) g[u] = g4[q + 256 * u];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc = norm_take<KIND>(acc, g[u].x); acc = norm_take<KIND>(acc, g[u].y);
        acc = norm_take<KIND>(acc, g[u].z); acc = norm_take<KIND>(acc, g[u].w);
      }
    }
    for (; q < n4; q += 256) {
      const float4 g = g4[q];
      acc = norm_take<KIND>(acc, g.x); acc = norm_take<KIND>(acc, g.y); acc = norm_take<KIND>(acc, g.z); acc = norm_take<KIND>(acc, g.w);
    }
    done = i0 + 4 * n4;
  }
  for (int64_t i = done + threadIdx.x; i < i1; i += 256) acc = norm_take<KIND>(acc, t.g[i]);
  acc = norm_block_reduce<KIND>(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// launch 2 (one workgroup): thread t takes partials[t], partials[t + 256], ... in index order, then the fixed tree;
// out = {norm, min(1, max_norm / (norm + 1e-6))}, both formed in f64 and rounded once
template <int KIND>
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const double* __restrict__ partials, int64_t n_chunks, double max_norm,
                                                              float* __restrict__ out) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n_chunks; i += 256) acc = norm_combine<KIND>(acc, partials[i]);
  acc = norm_block_reduce<KIND>(acc, sh);
  if (threadIdx.x != 0) return;
  const double norm = KIND == NORM_L2 ? sqrt(acc) : acc;
  const double coef = max_norm / (norm + 1e-6);
  out[0] = (float)norm;
  out[1] = (float)(coef > 1.0 ? 1.0 : coef);         // a NaN coefficient fails the comparison and stays NaN (torch.clamp(max=1) keeps it too)
}

__global__ __launch_bounds__(256) void grad_scale_kernel(const tribe_adam_tensor* __restrict__ table, const int32_t* __restrict__ chunk_tensor,
                                                         const int64_t* __restrict__ chunk_start, const float* __restrict__ coef_ptr,
                                                         float clip_value) {
  const float coef = coef_ptr ? coef_ptr[0] : 1.f;
  if (coef == 1.f && !(clip_value > 0.f)) return;    // x * 1.0f is x: nothing to read or write
  const tribe_adam_tensor t = table[chunk_tensor[blockIdx.x]];
  float* g = const_cast<float*>(t.g);
  const int64_t i0 = chunk_start[blockIdx.x];
  const int64_t i1 = (i0 + ADAM_CHUNK < t.n) ? i0 + ADAM_CHUNK : t.n;
  const bool vec = (((uintptr_t)g) & 15) == 0 && (i0 & 3) == 0;
  int64_t done = i0;
  if (vec) {
    const int64_t n4 = (i1 - i0) / 4;
    for (int64_t q = threadIdx.x; q < n4; q += 256) {
      f32x4_t x = *(const f32x4_t*)(g + i0 + 4 * q);   // one vector value end to end: the store stays 16 bytes wide
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = clip_grad(x[k], coef, clip_value);
      *(f32x4_t*)(g + i0 + 4 * q) = x;
    }
    done = i0 + 4 * n4;
  }
  for (int64_t i = done + threadIdx.x; i < i1; i += 256) g[i] = clip_grad(g[i], coef, clip_value);
}

}  // namespace

extern "C" int tribe_grad_norm(const tribe_adam_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_start, int64_t n_chunks,
                               int32_t norm_kind, double max_norm, double* partials, float* out, void* stream) {
  TRIBE_REQUIRE(table && chunk_tensor && chunk_start && partials && out, "tribe_grad_norm: null pointer");
  TRIBE_REQUIRE(n_chunks > 0 && n_chunks < (1ll << 31), "tribe_grad_norm: need 1 .. 2^31 chunks");
  TRIBE_REQUIRE(norm_kind == NORM_L2 || norm_kind == NORM_MAX, "tribe_grad_norm: norm_kind must be 0 (L2) or 1 (max-abs), got %d", (int)norm_kind);
  TRIBE_REQUIRE(max_norm == max_norm, "tribe_grad_norm: max_norm is NaN");
  hipStream_t s = (hipStream_t)stream;
  if (norm_kind == NORM_L2) {
    hipLaunchKernelGGL(grad_norm_partial_kernel<NORM_L2>, dim3((unsigned)n_chunks), dim3(256), 0, s, table, chunk_tensor, chunk_start, partials);
    hipLaunchKernelGGL(grad_norm_final_kernel<NORM_L2>, dim3(1), dim3(256), 0, s, partials, n_chunks, max_norm, out);
  } else {
    hipLaunchKernelGGL(grad_norm_partial_kernel<NORM_MAX>, dim3((unsigned)n_chunks), dim3(256), 0, s, table, chunk_tensor, chunk_start, partials);
    hipLaunchKernelGGL(grad_norm_final_kernel<NORM_MAX>, dim3(1), dim3(256), 0, s, partials, n_chunks, max_norm, out);
  }
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_grad_scale(const tribe_adam_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_start, int64_t n_chunks,
                                const float* coef, float clip_value, void* stream) {
  TRIBE_REQUIRE(table && chunk_tensor && chunk_start, "tribe_grad_scale: null pointer");
  TRIBE_REQUIRE(n_chunks > 0 && n_chunks < (1ll << 31), "tribe_grad_scale: need 1 .. 2^31 chunks");
  TRIBE_REQUIRE(clip_value == clip_value, "tribe_grad_scale: clip_value is NaN");
  hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)n_chunks), dim3(256), 0, (hipStream_t)stream, table, chunk_tensor, chunk_start, coef,
                     clip_value);
  TRIBE_LAUNCH_CHECK();
  return 0;
}
