// Inverted dropout with a counter-based mask (modeling_utils.autograd.Dropout, FeedForward's ff_dropout, Mlp's HIP dropout):
//   tribe_dropout_apply   y = keep(r, c) ? x * scale : +0.0   over the logical [rows, dim] tensor, f32 or bf16, in place or not.
// The backward of dropout is the same map applied to the gradient, so there is one entry point.
//
//   mask  : element (r, c) has idx = r * dim + c (64-bit; built from dim, never from a pitch: padding does not move the mask).  Its
//           random word is word idx & 3 of Philox4x32-10 (philox.h) with counter (lo32(idx >> 2), hi32(idx >> 2), lo32(site),
//           hi32(site)) and key (lo32(seed), hi32(seed)); the element is kept iff word >= threshold (threshold = trunc(p * 2^32)).
//   kept  : x * scale, one rounding for f32 (__fmul_rn); bf16 is widened, multiplied in f32 and rounded to nearest even.
//   dropped: +0.0 by a select, not a multiply: a dropped NaN, infinity or negative value is +0.0 (torch.dropout multiplies by 0 and
//           hands back NaN / -0.0 there).
// Columns >= dim of a row are neither read nor written.  One Philox call serves the four neighbouring elements that share a counter
// on every branch.  The result depends on (seed, site, r, c, dim, threshold, scale) alone, not on the grid; no atomics.
//
// Branches (tribe_dropout_path): 0 = 16 bytes per access (four f32 / eight bf16: dim and both pitches multiples of that, both pointers
// 16-byte aligned), 1 = 8 bytes per access (four bf16, where 0 does not fit), 2 = element accesses, one lane per counter -- its four
// elements may straddle a row end.  A tensor without padding (both pitches == dim) runs as ONE row of rows * dim elements: same idx.
#include "common.h"
#include "philox.h"

namespace {

enum { DROP_VEC16 = 0, DROP_VEC8 = 1, DROP_ELEM = 2 };

struct drop_key {
  unsigned thr, k0, k1, s0, s1;
  float scale;
};

__device__ __forceinline__ uint4 drop_words(const drop_key& k, int64_t quad) {
  return philox4x32_10(make_uint4((unsigned)((uint64_t)quad & 0xffffffffu), (unsigned)((uint64_t)quad >> 32), k.s0, k.s1), k.k0, k.k1);
}
__device__ __forceinline__ float drop_f32(float v, unsigned word, const drop_key& k) { return word >= k.thr ? __fmul_rn(v, k.scale) : 0.f; }
__device__ __forceinline__ unsigned short drop_bf16(unsigned short h, unsigned word, const drop_key& k) {
  return word >= k.thr ? f32_to_bf16(__fmul_rn(bf16_to_f32(h), k.scale)) : (unsigned short)0;
}

// EPV elements per access: f32 4 (16 B), bf16 8 (16 B) or 4 (8 B).  grid (column blocks, row groups); both stride.
// x and y may be the same buffer: a lane reads its elements before it writes them and no other lane touches them.
template <int EPV, bool BF>
__global__ __launch_bounds__(256) void dropout_vec_kernel(const void* x, void* y, int64_t rows, int64_t dim, int64_t ld_x, int64_t ld_y,
                                                          drop_key k) {
  const int64_t nv = dim / EPV;
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    for (int64_t cv = (int64_t)blockIdx.x * 256 + threadIdx.x; cv < nv; cv += (int64_t)gridDim.x * 256) {
      const int64_t c = cv * EPV;
      const int64_t quad = (row * dim + c) >> 2;   // dim % 4 == 0 and c % 4 == 0: the access starts a counter
      if constexpr (!BF) {
        const float4 v = *(const float4*)((const float*)x + row * ld_x + c);
        const uint4 w = drop_words(k, quad);
        *(float4*)((float*)y + row * ld_y + c) = make_float4(drop_f32(v.x, w.x, k), drop_f32(v.y, w.y, k), drop_f32(v.z, w.z, k), drop_f32(v.w, w.w, k));
      } else if constexpr (EPV == 8) {
        const u16x8_t v = *(const u16x8_t*)((const unsigned short*)x + row * ld_x + c);
        const uint4 w0 = drop_words(k, quad), w1 = drop_words(k, quad + 1);
        u16x8_t o;
        o[0] = drop_bf16(v[0], w0.x, k);
        o[1] = drop_bf16(v[1], w0.y, k);
        o[2] = drop_bf16(v[2], w0.z, k);
        o[3] = drop_bf16(v[3], w0.w, k);
        o[4] = drop_bf16(v[4], w1.x, k);
        o[5] = drop_bf16(v[5], w1.y, k);
        o[6] = drop_bf16(v[6], w1.z, k);
        o[7] = drop_bf16(v[7], w1.w, k);
        *(u16x8_t*)((unsigned short*)y + row * ld_y + c) = o;
      } else {
        const u16x4_t v = *(const u16x4_t*)((const unsigned short*)x + row * ld_x + c);
        const uint4 w = drop_words(k, quad);
        u16x4_t o;
        o[0] = drop_bf16(v[0], w.x, k);
        o[1] = drop_bf16(v[1], w.y, k);
        o[2] = drop_bf16(v[2], w.z, k);
        o[3] = drop_bf16(v[3], w.w, k);
        *(u16x4_t*)((unsigned short*)y + row * ld_y + c) = o;
      }
    }
  }
}

// one lane per counter: elements idx = 4 * quad .. 4 * quad + 3 of the flattened [rows, dim] tensor, wherever their rows end
template <bool BF>
__global__ __launch_bounds__(256) void dropout_elem_kernel(const void* x, void* y, int64_t total, int64_t dim, int64_t ld_x, int64_t ld_y, drop_key k) {
  const int64_t nq = (total + 3) >> 2;
  const bool small = total <= 0xffffffffll;   // a 32-bit division where it is enough (uniform over the grid)
  for (int64_t quad = (int64_t)blockIdx.x * 256 + threadIdx.x; quad < nq; quad += (int64_t)gridDim.x * 256) {
    const int64_t idx0 = quad * 4;
    int64_t r = small ? (int64_t)((unsigned)idx0 / (unsigned)dim) : idx0 / dim;
    int64_t c = idx0 - r * dim;
    const uint4 o = drop_words(k, quad);
    const unsigned w[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (idx0 + e < total) {
        if (BF) ((unsigned short*)y)[r * ld_y + c] = drop_bf16(((const unsigned short*)x)[r * ld_x + c], w[e], k);
        else ((float*)y)[r * ld_y + c] = drop_f32(((const float*)x)[r * ld_x + c], w[e], k);
        if (++c == dim) {
          c = 0;
          ++r;
        }
      }
    }
  }
}

bool aligned_to(const void* p, uintptr_t bytes) { return ((uintptr_t)p % bytes) == 0; }

int pick_path(const void* x, const void* y, int32_t dtype, int64_t dim, int64_t ld_x, int64_t ld_y) {
  const int64_t q = dtype == TRIBE_BF16 ? 8 : 4;   // elements per 16 bytes
  if (dim % q == 0 && ld_x % q == 0 && ld_y % q == 0 && aligned_to(x, 16) && aligned_to(y, 16)) return DROP_VEC16;
  if (dtype == TRIBE_BF16 && dim % 4 == 0 && ld_x % 4 == 0 && ld_y % 4 == 0 && aligned_to(x, 8) && aligned_to(y, 8)) return DROP_VEC8;
  return DROP_ELEM;
}

}  // namespace

extern "C" int tribe_dropout_path(const void* x, const void* y, int32_t dtype, int64_t dim, int64_t ld_x, int64_t ld_y) {
  return pick_path(x, y, dtype, dim, ld_x, ld_y);
}

extern "C" int tribe_dropout_apply(const void* x, void* y, int32_t dtype, int64_t rows, int64_t dim, int64_t ld_x, int64_t ld_y,
                                   uint32_t threshold, float scale, uint64_t seed, uint64_t site, void* stream) {
  TRIBE_REQUIRE(x && y, "tribe_dropout_apply: null pointer");
  TRIBE_REQUIRE(dtype == TRIBE_F32 || dtype == TRIBE_BF16, "tribe_dropout_apply: dtype must be f32 or bf16, got %d", (int)dtype);
  TRIBE_REQUIRE(rows > 0 && dim > 0 && rows < (1ll << 31) && dim < (1ll << 40) && ld_x >= dim && ld_y >= dim && ld_x < (1ll << 40) && ld_y < (1ll << 40),
                "tribe_dropout_apply: rows=%lld dim=%lld ld_x=%lld ld_y=%lld (need 0 < rows < 2^31, 0 < dim <= ld < 2^40)", (long long)rows,
                (long long)dim, (long long)ld_x, (long long)ld_y);
  TRIBE_REQUIRE(rows <= (1ll << 62) / dim, "tribe_dropout_apply: rows * dim = %lld * %lld exceeds 2^62", (long long)rows, (long long)dim);
  TRIBE_REQUIRE(scale >= 1.f && scale <= 3.4028234663852886e38f, "tribe_dropout_apply: scale = 1 / (1 - p) must be finite and >= 1, got %g",
                (double)scale);   // (a NaN fails both comparisons)
  const int path = pick_path(x, y, dtype, dim, ld_x, ld_y);
  if (ld_x == dim && ld_y == dim) {   // no padding: one row of rows * dim elements has the same idx per element
    dim *= rows;
    ld_x = ld_y = dim;
    rows = 1;
  }
  const drop_key k = {threshold, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), (unsigned)(site & 0xffffffffu), (unsigned)(site >> 32), scale};
  hipStream_t s = (hipStream_t)stream;
  const bool bf = dtype == TRIBE_BF16;
  if (path == DROP_ELEM) {
    const int64_t total = rows * dim;
    const dim3 grid(grid_for((total + 3) >> 2, 256));
    if (bf) hipLaunchKernelGGL(dropout_elem_kernel<true>, grid, dim3(256), 0, s, x, y, total, dim, ld_x, ld_y, k);
    else hipLaunchKernelGGL(dropout_elem_kernel<false>, grid, dim3(256), 0, s, x, y, total, dim, ld_x, ld_y, k);
  } else {
    const int epv = (bf && path == DROP_VEC16) ? 8 : 4;
    const unsigned gx = grid_for(dim / epv, 256);
    const int64_t room = 2048 / gx;
    const dim3 grid(gx, (unsigned)(rows < room ? rows : (room < 1 ? 1 : room)));
    if (!bf) hipLaunchKernelGGL((dropout_vec_kernel<4, false>), grid, dim3(256), 0, s, x, y, rows, dim, ld_x, ld_y, k);
    else if (epv == 8) hipLaunchKernelGGL((dropout_vec_kernel<8, true>), grid, dim3(256), 0, s, x, y, rows, dim, ld_x, ld_y, k);
    else hipLaunchKernelGGL((dropout_vec_kernel<4, true>), grid, dim3(256), 0, s, x, y, rows, dim, ld_x, ld_y, k);
  }
  TRIBE_LAUNCH_CHECK();
  return 0;
}
