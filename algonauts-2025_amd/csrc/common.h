// Shared helpers for the TRIBE gfx950 kernels (device + host side of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/tribe_hip.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;   // one MFMA A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) float f32x4_t;    // 16x16 accumulator fragment
typedef __attribute__((ext_vector_type(16))) float f32x16_t;  // 32x32 accumulator fragment
typedef __attribute__((ext_vector_type(4))) unsigned short u16x4_t;
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8_t;

#define TRIBE_WAVE 64

// ---- bf16 <-> f32 ------------------------------------------------------------
__device__ __forceinline__ float bf16_to_f32(unsigned short h) {
  return __uint_as_float(((unsigned int)h) << 16);
}
// round-to-nearest-even; a plain cast lowers to v_cvt_pk_bf16_f32 on gfx950 and keeps NaN a NaN
__device__ __forceinline__ unsigned short f32_to_bf16(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(unsigned short, b);
}

// ---- wave / block reductions ---------------------------------------------------
// streaming (read-once) 16-byte load: keeps a one-pass reduction from evicting what L2 / MALL hold for the GEMMs
typedef float tribe_f32x4_nt __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 load_nt_f4(const void* p) {
  const tribe_f32x4_nt v = __builtin_nontemporal_load((const tribe_f32x4_nt*)p);
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ double block_sum_d(double v, double* sh) {   // sh: one slot per wave
  v = wave_sum_d(v);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[w] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sh[i];
  return t;
}
// Centred sum of squares S2 - S1^2 / n of n samples from one-pass f64 sums (Pearson statistics).  Each of the up to n adds behind
// S1 and S2 may be off by an ulp of its running sum, so a result at or below n * DBL_EPSILON * S2 cannot be told from 0 and is 0:
// a constant column of ~1e5 samples otherwise leaves rounding noise of either sign here, and r = noise / noise.
__device__ __forceinline__ double onepass_centred_ss(double s1, double s2, double n) {
  const double v = s2 - s1 * s1 / n;
  return v > n * __DBL_EPSILON__ * s2 ? v : 0.0;
}
// ---- f32 -> e4m3 (OCP e4m3fn), four values to four bytes: saturating, round to nearest even, NaN passed through ----------------
// The clamp keeps v_cvt_pk_fp8_f32 (which turns whatever rounds past 448 into NaN) saturating.  It is ONE ordered compare per value,
// which a NaN fails: a NaN reaches the conversion and leaves as the NaN code, never as a finite +-448.  The clamp gives the MAGNITUDE
// 448 only; the sign of every code comes from pack_e4m3x4 below.
__device__ __forceinline__ float clamp_e4m3_magnitude(float f) {
  return fabsf(f) > 448.f ? 448.f : f;
}
// The conversion gives every NaN the code 0xFF whatever its sign (measured: tests/test_gpu_fp8_bounds.py), while every other code
// carries the sign of its input, zeros included.  So the four sign bits are taken from the inputs -- two byte gathers (v_perm_b32: the
// top byte of each float into its code's place) and one bit select, no compare -- and only the NaN bytes (and the clamped ones, whose
// sign the clamp dropped) change: +NaN -> 0x7F, -NaN -> 0xFF, the codes of torch's float8_e4m3fn cast.
__device__ __forceinline__ int pack_e4m3x4(float a, float b, float c, float d) {
  int pk = __builtin_amdgcn_cvt_pk_fp8_f32(clamp_e4m3_magnitude(a), clamp_e4m3_magnitude(b), 0, false);
  pk = __builtin_amdgcn_cvt_pk_fp8_f32(clamp_e4m3_magnitude(c), clamp_e4m3_magnitude(d), pk, true);
  // v_perm_b32 selects from {src0, src1}: 0..3 = bytes of src1, 4..7 = bytes of src0, 0x0c = zero
  const unsigned int top = __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x0c0c0703u) |
                           __builtin_amdgcn_perm(__float_as_uint(d), __float_as_uint(c), 0x07030c0cu);
  return (int)((top & 0x80808080u) | ((unsigned int)pk & 0x7F7F7F7Fu));
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// ---- optimiser work list (tribe_adam_step, tribe_swa_update, tribe_grad_*) --------------------------
// elements per chunk = per workgroup; the value tribe_adam_chunk_elems() reports
constexpr int ADAM_CHUNK = 16384;
// One gradient under clipping: clamp(g * coef, -clip_value, clip_value), clip_value <= 0 = no clamp.  __fmul_rn keeps the product a
// rounded f32 of its own wherever it is inlined (hipcc contracts a * b + c into an FMA by default), so the in-place pass and the fused
// optimiser step see the same bits.  The comparisons are false for NaN: NaN stays NaN, as under torch.clamp.
__device__ __forceinline__ float clip_grad(float g, float coef, float clip_value) {
  g = __fmul_rn(g, coef);
  const float lim = clip_value > 0.f ? clip_value : INFINITY;   // no clamp = a limit nothing exceeds: two selects, no branch
  return g < -lim ? -lim : (g > lim ? lim : g);
}

// ---- host-side error plumbing ----------------------------------------------------
void tribe_set_error(const char* fmt, ...);

#define TRIBE_REQUIRE(cond, ...)      \
  do {                                \
    if (!(cond)) {                    \
      tribe_set_error(__VA_ARGS__);   \
      return -1;                      \
    }                                 \
  } while (0)

#define TRIBE_LAUNCH_CHECK()                                           \
  do {                                                                 \
    hipError_t e__ = hipGetLastError();                                \
    if (e__ != hipSuccess) {                                           \
      tribe_set_error("HIP launch failed: %s", hipGetErrorString(e__)); \
      return (int)e__;                                                 \
    }                                                                  \
  } while (0)

// in-library HIP-event profile (gemm.hip; bench.py brackets its timed region with tribe_prof_begin / tribe_prof_end): other launchers
// of the path (fused attention) take a slot for their role the same way the GEMM launcher does
int tribe_internal_prof_before(int role, double flops, hipStream_t s);
void tribe_internal_prof_after(int slot, hipStream_t s);

// Raises KERNEL's dynamic-LDS limit to `bytes` before a launch that needs more than the default 64 KiB: once per kernel AND device (one
// process may drive several GPUs, and the attribute is per device); with a device index outside the table the call is made every time.
template <auto KERNEL>
static inline void raise_dynamic_lds_once(int bytes) {
  static bool done[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64 || !done[dev]) {
    (void)hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (dev >= 0 && dev < 64) done[dev] = true;
  }
}

static inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// grid of a 1-D launch of `total` work items: ceil(total / block), at least 1, capped at max_blocks (the default for the
// memory-bound kernels that stride over the rest)
static inline unsigned grid_for(int64_t total, int block, int64_t max_blocks = 256 * 8) {
  int64_t b = (total + block - 1) / block;
  if (b > max_blocks) b = max_blocks;
  if (b < 1) b = 1;
  return (unsigned)b;
}
