// Hidden block of an MLP in torchvision.ops.MLP's layout: what stands between two Linear layers, nn.LayerNorm (optional) and the
// activation, as ONE row kernel each way.
//   tribe_norm_act_fwd   y = act(gamma * (z - mean) * rstd + beta)     f32 [rows, dim] -> f32 or bf16 (K-padded GEMM operand) [+ mean, rstd]
//   tribe_norm_act_bwd   dz from dy and the saved z / mean / rstd; dgamma, dbeta as fixed-order column sums (no atomics)
// One wave per row.  Row statistics and the two row means of the backward are f64 sums of the widened f32 values, rounded once; every
// f32 step of the element arithmetic is an explicitly rounded operation (__fsub_rn / __fmul_rn / fmaf), so the register-resident, the
// 16-byte-walk and the element kernels -- and the column-sum kernel that recomputes du and zh -- all form the same bits per element.
// row_load / row_each, which give one kernel body its three forms, are in row_wave.h.
#include <math.h>

#include "common.h"
#include "row_wave.h"

namespace {

enum { PATH_REG4 = 0, PATH_REG16 = 1, PATH_WALK4 = 2, PATH_ELEM = 3 };
constexpr int COL_ROWS = 64;   // rows per partial of the column sums

__device__ __forceinline__ float act_fwd(int act, float u) {
  switch (act) {
    case TRIBE_ACT_GELU: return 0.5f * u * (1.f + erff(u * 0.70710678118654752f));
    case TRIBE_ACT_RELU: return u <= 0.f ? 0.f : u;          // NaN stays NaN, as under torch
    case TRIBE_ACT_ELU: return u <= 0.f ? expm1f(u) : u;
    default: return u;
  }
}
// d act / du as torch's backward formulas take it: ReLU 0 at u <= 0, ELU exp(u) at u <= 0, GELU Phi(u) + u phi(u)
__device__ __forceinline__ float act_bwd(int act, float u) {
  switch (act) {
    case TRIBE_ACT_GELU: return 0.5f * (1.f + erff(u * 0.70710678118654752f)) + u * (0.39894228040143268f * expf(-0.5f * u * u));
    case TRIBE_ACT_RELU: return u <= 0.f ? 0.f : 1.f;
    case TRIBE_ACT_ELU: return u <= 0.f ? expf(u) : 1.f;
    default: return 1.f;
  }
}
// u (and zh) of one element: three roundings -- the difference, the product with rstd, the fma with gamma / beta
__device__ __forceinline__ float norm_u(float z, float mean, float rstd, float g, float b, int norm, float& zh) {
  if (!norm) {
    zh = 0.f;
    return z;
  }
  zh = __fmul_rn(__fsub_rn(z, mean), rstd);
  return fmaf(zh, g, b);
}

template <bool VEC>
__device__ __forceinline__ float4 load_cols(const float* p, int64_t c) {   // p may be NULL only where the caller does not ask
  if (VEC) return *(const float4*)(p + c);
  return make_float4(p[c], 0.f, 0.f, 0.f);
}
template <bool VEC>
__device__ __forceinline__ float4 load_cols_any(const void* p, int bf16, int64_t c) {
  if (!bf16) return load_cols<VEC>((const float*)p, c);
  const unsigned short* h = (const unsigned short*)p + c;
  if (VEC) {
    const u16x4_t v = *(const u16x4_t*)h;
    return make_float4(bf16_to_f32(v[0]), bf16_to_f32(v[1]), bf16_to_f32(v[2]), bf16_to_f32(v[3]));
  }
  return make_float4(bf16_to_f32(h[0]), 0.f, 0.f, 0.f);
}
template <bool VEC>
__device__ __forceinline__ void store_cols_any(void* p, int bf16, int64_t c, const float (&o)[4]) {
  if (bf16) {
    unsigned short* h = (unsigned short*)p + c;
    if (VEC) {
      u16x4_t v;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = f32_to_bf16(o[k]);
      *(u16x4_t*)h = v;
    } else {
      h[0] = f32_to_bf16(o[0]);
    }
  } else {
    if (VEC) *(float4*)((float*)p + c) = make_float4(o[0], o[1], o[2], o[3]);
    else ((float*)p)[c] = o[0];
  }
}
// columns dim .. ld - 1 of one output row
__device__ __forceinline__ void zero_pad(void* p, int bf16, int64_t dim, int64_t ld, int lane) {
  for (int64_t c = dim + lane; c < ld; c += 64) {
    if (bf16) ((unsigned short*)p)[c] = 0;
    else ((float*)p)[c] = 0.f;
  }
}

template <int NV, bool VEC>
__global__ __launch_bounds__(256) void norm_act_fwd_kernel(const float* __restrict__ z, int64_t rows, int64_t dim, int64_t ld_z,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int norm,
                                                           int act, void* __restrict__ y, int y_bf16, int64_t ld_y, float* __restrict__ mean_out,
                                                           float* __restrict__ rstd_out) {
  constexpr int W = VEC ? 4 : 1;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                               // (no block-wide barrier below)
  const float* zr = z + row * ld_z;
  float4 v[NV > 0 ? NV : 1];
  row_load<NV>(zr, v, dim, lane);
  float mean = 0.f, rstd = 1.f;
  if (norm) {
    double s = 0.0;
    row_each<NV, VEC>(zr, v, dim, lane, [&](int64_t, float4 x, int) {
      const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int k = 0; k < W; ++k) s += (double)xs[k];
    });
    const double mu = wave_sum_d(s) / (double)dim;
    double q = 0.0;
    row_each<NV, VEC>(zr, v, dim, lane, [&](int64_t, float4 x, int) {
      const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const double d = (double)xs[k] - mu;
        q = fma(d, d, q);
      }
    });
    const double var = wave_sum_d(q) / (double)dim;
    mean = (float)mu;
    rstd = (float)(1.0 / sqrt(var + (double)eps));
    if (lane == 0) {
      if (mean_out) mean_out[row] = mean;
      if (rstd_out) rstd_out[row] = rstd;
    }
  }
  const bool has_g = norm && gamma, has_b = norm && beta;
  void* yr = y_bf16 ? (void*)((unsigned short*)y + row * ld_y) : (void*)((float*)y + row * ld_y);
  row_each<NV, VEC>(zr, v, dim, lane, [&](int64_t c, float4 x, int) {
    const float4 g4 = has_g ? load_cols<VEC>(gamma, c) : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 b4 = has_b ? load_cols<VEC>(beta, c) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float xs[4] = {x.x, x.y, x.z, x.w}, gs[4] = {g4.x, g4.y, g4.z, g4.w}, bs[4] = {b4.x, b4.y, b4.z, b4.w};
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < W; ++k) {
      float zh;
      o[k] = act_fwd(act, norm_u(xs[k], mean, rstd, gs[k], bs[k], norm, zh));
    }
    store_cols_any<VEC>(yr, y_bf16, c, o);
  });
  zero_pad(yr, y_bf16, dim, ld_y, lane);
}

// du and zh of up to four neighbouring columns of one row; dzh = du * gamma
template <bool VEC>
__device__ __forceinline__ void bwd_cols(float4 x, float4 dy4, float4 g4, float4 b4, float mean, float rstd, int norm, int act, float (&zh)[4],
                                         float (&du)[4], float (&dzh)[4]) {
  constexpr int W = VEC ? 4 : 1;
  const float xs[4] = {x.x, x.y, x.z, x.w}, ds[4] = {dy4.x, dy4.y, dy4.z, dy4.w}, gs[4] = {g4.x, g4.y, g4.z, g4.w},
              bs[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) zh[k] = du[k] = dzh[k] = 0.f;
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const float u = norm_u(xs[k], mean, rstd, gs[k], bs[k], norm, zh[k]);
    du[k] = __fmul_rn(ds[k], act_bwd(act, u));
    dzh[k] = __fmul_rn(du[k], gs[k]);
  }
}

template <int NV, bool VEC>
__global__ __launch_bounds__(256) void norm_act_bwd_kernel(const void* __restrict__ dy, int dy_bf16, int64_t ld_dy, const float* __restrict__ z,
                                                           int64_t rows, int64_t dim, int64_t ld_z, const float* __restrict__ mean_in,
                                                           const float* __restrict__ rstd_in, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int norm, int act, void* __restrict__ dz, int dz_bf16,
                                                           int64_t ld_dz) {
  constexpr int W = VEC ? 4 : 1;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* zr = z + row * ld_z;
  const void* dyr = dy_bf16 ? (const void*)((const unsigned short*)dy + row * ld_dy) : (const void*)((const float*)dy + row * ld_dy);
  void* dzr = dz_bf16 ? (void*)((unsigned short*)dz + row * ld_dz) : (void*)((float*)dz + row * ld_dz);
  const float mean = norm ? mean_in[row] : 0.f, rstd = norm ? rstd_in[row] : 1.f;
  const bool has_g = norm && gamma, has_b = norm && beta;
  float4 v[NV > 0 ? NV : 1], w[NV > 0 ? NV : 1];        // z and dzh of the register-resident row
  row_load<NV>(zr, v, dim, lane);
  auto cols = [&](int64_t c, float4 x, float (&zh)[4], float (&du)[4], float (&dzh)[4]) {
    const float4 g4 = has_g ? load_cols<VEC>(gamma, c) : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 b4 = has_b ? load_cols<VEC>(beta, c) : make_float4(0.f, 0.f, 0.f, 0.f);
    bwd_cols<VEC>(x, load_cols_any<VEC>(dyr, dy_bf16, c), g4, b4, mean, rstd, norm, act, zh, du, dzh);
  };
  if (!norm) {                                           // dz = du: one pass
    row_each<NV, VEC>(zr, v, dim, lane, [&](int64_t c, float4 x, int) {
      float zh[4], du[4], dzh[4];
      cols(c, x, zh, du, dzh);
      store_cols_any<VEC>(dzr, dz_bf16, c, du);
    });
    zero_pad(dzr, dz_bf16, dim, ld_dz, lane);
    return;
  }
  double s1 = 0.0, s2 = 0.0;
  row_each<NV, VEC>(zr, v, dim, lane, [&](int64_t c, float4 x, int j) {
    float zh[4], du[4], dzh[4];
    cols(c, x, zh, du, dzh);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      s1 += (double)dzh[k];
      s2 = fma((double)dzh[k], (double)zh[k], s2);
    }
    if (NV > 0) w[j] = make_float4(dzh[0], dzh[1], dzh[2], dzh[3]);
  });
  const float m1 = (float)(wave_sum_d(s1) / (double)dim), m2 = (float)(wave_sum_d(s2) / (double)dim);
  row_each<NV, VEC>(zr, v, dim, lane, [&](int64_t c, float4 x, int j) {
    float zh[4], du[4], dzh[4];
    if (NV > 0) {                                        // dzh was kept; zh is two operations away
      const float xs[4] = {x.x, x.y, x.z, x.w}, ks[4] = {w[j].x, w[j].y, w[j].z, w[j].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        zh[k] = __fmul_rn(__fsub_rn(xs[k], mean), rstd);
        dzh[k] = ks[k];
      }
    } else {
      cols(c, x, zh, du, dzh);
    }
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < W; ++k) o[k] = __fmul_rn(fmaf(-zh[k], m2, __fsub_rn(dzh[k], m1)), rstd);
    store_cols_any<VEC>(dzr, dz_bf16, c, o);
  });
  zero_pad(dzr, dz_bf16, dim, ld_dz, lane);
}

// partial column sums of du * zh and du over rows [COL_ROWS * blockIdx.y, ...).  A workgroup is 64 columns x 4 groups of COL_ROWS / 4 rows:
// a wave reads 256 contiguous bytes of a row, a thread adds its rows in order, the four groups are added in group order -- a fixed tree.
__global__ __launch_bounds__(256) void norm_act_colsum_kernel(const void* __restrict__ dy, int dy_bf16, int64_t ld_dy, const float* __restrict__ z,
                                                              int64_t rows, int64_t dim, int64_t ld_z, const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, int act, double* __restrict__ part) {
  __shared__ double sh[2][4][64];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  const int64_t r0 = (int64_t)blockIdx.y * COL_ROWS + grp * (COL_ROWS / 4);
  const int64_t r1 = r0 + COL_ROWS / 4 < rows ? r0 + COL_ROWS / 4 : rows;
  double sg = 0.0, sb = 0.0;
  if (c < dim) {
    const float g = gamma ? gamma[c] : 1.f, b = beta ? beta[c] : 0.f;
#pragma unroll 4
    for (int64_t r = r0; r < r1; ++r) {
      const float d = dy_bf16 ? bf16_to_f32(((const unsigned short*)dy)[r * ld_dy + c]) : ((const float*)dy)[r * ld_dy + c];
      float zh;
      const float u = norm_u(z[r * ld_z + c], mean[r], rstd[r], g, b, 1, zh);
      const float du = __fmul_rn(d, act_bwd(act, u));
      sg = fma((double)du, (double)zh, sg);
      sb += (double)du;
    }
  }
  sh[0][grp][lane] = sg;
  sh[1][grp][lane] = sb;
  __syncthreads();
  if (grp == 0 && c < dim) {
    part[((int64_t)blockIdx.y * 2 + 0) * dim + c] = ((sh[0][0][lane] + sh[0][1][lane]) + sh[0][2][lane]) + sh[0][3][lane];
    part[((int64_t)blockIdx.y * 2 + 1) * dim + c] = ((sh[1][0][lane] + sh[1][1][lane]) + sh[1][2][lane]) + sh[1][3][lane];
  }
}
// the partials of one column, rounded once: four groups of consecutive partials, each in order, then the groups in order
__global__ __launch_bounds__(256) void norm_act_colsum_final_kernel(const double* __restrict__ part, int64_t nparts, int64_t dim,
                                                                    float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ double sh[2][4][64];
  const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int64_t c = (int64_t)blockIdx.x * 64 + lane;
  const int64_t per = (nparts + 3) / 4, p0 = grp * per, p1 = p0 + per < nparts ? p0 + per : nparts;
  double sg = 0.0, sb = 0.0;
  if (c < dim) {
#pragma unroll 4
    for (int64_t p = p0; p < p1; ++p) {
      sg += part[(p * 2 + 0) * dim + c];
      sb += part[(p * 2 + 1) * dim + c];
    }
  }
  sh[0][grp][lane] = sg;
  sh[1][grp][lane] = sb;
  __syncthreads();
  if (grp == 0 && c < dim) {
    if (dgamma) dgamma[c] = (float)(((sh[0][0][lane] + sh[0][1][lane]) + sh[0][2][lane]) + sh[0][3][lane]);
    if (dbeta) dbeta[c] = (float)(((sh[1][0][lane] + sh[1][1][lane]) + sh[1][2][lane]) + sh[1][3][lane]);
  }
}

bool aligned_to(const void* p, uintptr_t bytes) { return ((uintptr_t)p % bytes) == 0; }   // NULL counts as aligned
uintptr_t quad_bytes(int32_t dtype) { return dtype == TRIBE_BF16 ? 8 : 16; }              // four elements

int pick_path(const float* z, int64_t dim, int64_t ld_z, const float* gamma, const float* beta, const void* y, int32_t y_dtype, int64_t ld_y,
              const void* dy, int32_t dy_dtype, int64_t ld_dy) {
  const bool vec = dim % 4 == 0 && ld_z % 4 == 0 && ld_y % 4 == 0 && aligned_to(z, 16) && aligned_to(gamma, 16) && aligned_to(beta, 16) &&
                   aligned_to(y, quad_bytes(y_dtype)) && (!dy || (ld_dy % 4 == 0 && aligned_to(dy, quad_bytes(dy_dtype))));
  if (!vec) return PATH_ELEM;
  return dim <= 1024 ? PATH_REG4 : (dim <= 4096 ? PATH_REG16 : PATH_WALK4);
}

bool act_ok(int32_t act) { return act == TRIBE_ACT_NONE || act == TRIBE_ACT_GELU || act == TRIBE_ACT_RELU || act == TRIBE_ACT_ELU; }
bool dtype_ok(int32_t d) { return d == TRIBE_F32 || d == TRIBE_BF16; }

}  // namespace

extern "C" int tribe_norm_act_path(const float* z, int64_t dim, int64_t ld_z, const float* gamma, const float* beta, const void* y,
                                   int32_t y_dtype, int64_t ld_y, const void* dy, int32_t dy_dtype, int64_t ld_dy) {
  return pick_path(z, dim, ld_z, gamma, beta, y, y_dtype, ld_y, dy, dy_dtype, ld_dy);
}

extern "C" int tribe_norm_act_fwd(const float* z, int64_t rows, int64_t dim, int64_t ld_z, const float* gamma, const float* beta, float eps,
                                  int32_t norm, int32_t act, void* y, int32_t y_dtype, int64_t ld_y, float* mean, float* rstd, void* stream) {
  TRIBE_REQUIRE(z && y, "tribe_norm_act_fwd: null pointer");
  TRIBE_REQUIRE(rows > 0 && rows < (1ll << 31) && dim > 0 && ld_z >= dim && ld_y >= dim,
                "tribe_norm_act_fwd: rows=%lld dim=%lld ld_z=%lld ld_y=%lld (need 0 < rows < 2^31, 0 < dim <= ld)", (long long)rows, (long long)dim,
                (long long)ld_z, (long long)ld_y);
  TRIBE_REQUIRE(norm == 0 || norm == 1, "tribe_norm_act_fwd: norm must be 0 (none) or 1 (LayerNorm), got %d", (int)norm);
  TRIBE_REQUIRE(act_ok(act), "tribe_norm_act_fwd: act must be NONE, GELU, RELU or ELU, got %d", (int)act);
  TRIBE_REQUIRE(dtype_ok(y_dtype), "tribe_norm_act_fwd: y_dtype must be f32 or bf16");
  TRIBE_REQUIRE(!norm || (eps == eps && eps >= 0.f), "tribe_norm_act_fwd: eps must be >= 0");
  const dim3 grid((unsigned)((rows + 3) / 4));
  const int bf = y_dtype == TRIBE_BF16;
#define TRIBE_NA_FWD(NV, VEC)                                                                                                              \
  hipLaunchKernelGGL((norm_act_fwd_kernel<NV, VEC>), grid, dim3(256), 0, (hipStream_t)stream, z, rows, dim, ld_z, gamma, beta, eps, (int)norm, \
                     (int)act, y, bf, ld_y, mean, rstd)
  switch (pick_path(z, dim, ld_z, norm ? gamma : nullptr, norm ? beta : nullptr, y, y_dtype, ld_y, nullptr, 0, 0)) {
    case PATH_REG4: TRIBE_NA_FWD(4, true); break;
    case PATH_REG16: TRIBE_NA_FWD(16, true); break;
    case PATH_WALK4: TRIBE_NA_FWD(0, true); break;
    default: TRIBE_NA_FWD(0, false); break;
  }
#undef TRIBE_NA_FWD
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t tribe_norm_act_bwd_workspace_bytes(int64_t rows, int64_t dim) {
  if (rows <= 0 || dim <= 0) return 0;
  return (size_t)((rows + COL_ROWS - 1) / COL_ROWS) * 2 * (size_t)dim * sizeof(double);
}

extern "C" int tribe_norm_act_bwd(const void* dy, int32_t dy_dtype, int64_t ld_dy, const float* z, int64_t rows, int64_t dim, int64_t ld_z,
                                  const float* mean, const float* rstd, const float* gamma, const float* beta, int32_t norm, int32_t act,
                                  void* dz, int32_t dz_dtype, int64_t ld_dz, float* dgamma, float* dbeta, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(dy && z && dz, "tribe_norm_act_bwd: null pointer");
  TRIBE_REQUIRE(rows > 0 && rows < (1ll << 31) && dim > 0 && ld_z >= dim && ld_dy >= dim && ld_dz >= dim,
                "tribe_norm_act_bwd: rows=%lld dim=%lld ld_dy=%lld ld_z=%lld ld_dz=%lld (need 0 < rows < 2^31, 0 < dim <= ld)", (long long)rows,
                (long long)dim, (long long)ld_dy, (long long)ld_z, (long long)ld_dz);
  TRIBE_REQUIRE(norm == 0 || norm == 1, "tribe_norm_act_bwd: norm must be 0 (none) or 1 (LayerNorm), got %d", (int)norm);
  TRIBE_REQUIRE(act_ok(act), "tribe_norm_act_bwd: act must be NONE, GELU, RELU or ELU, got %d", (int)act);
  TRIBE_REQUIRE(dtype_ok(dy_dtype) && dtype_ok(dz_dtype), "tribe_norm_act_bwd: dy_dtype and dz_dtype must be f32 or bf16");
  TRIBE_REQUIRE(!norm || (mean && rstd), "tribe_norm_act_bwd: the LayerNorm backward needs the saved mean and rstd");
  TRIBE_REQUIRE(norm || (!dgamma && !dbeta), "tribe_norm_act_bwd: dgamma / dbeta exist only with norm = 1");
  const bool colsums = dgamma || dbeta;
  const int64_t nparts = (rows + COL_ROWS - 1) / COL_ROWS;
  TRIBE_REQUIRE(!colsums || (workspace && workspace_bytes >= tribe_norm_act_bwd_workspace_bytes(rows, dim) && aligned_to(workspace, 8)),
                "tribe_norm_act_bwd: workspace of %zu bytes (8-byte aligned) needed, got %zu", tribe_norm_act_bwd_workspace_bytes(rows, dim),
                workspace_bytes);
  TRIBE_REQUIRE(!colsums || nparts <= 65535, "tribe_norm_act_bwd: at most %d rows with dgamma / dbeta", 65535 * COL_ROWS);
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((rows + 3) / 4));
  const int dyb = dy_dtype == TRIBE_BF16, dzb = dz_dtype == TRIBE_BF16;
  if (!norm) gamma = beta = nullptr;
#define TRIBE_NA_BWD(NV, VEC)                                                                                                               \
  hipLaunchKernelGGL((norm_act_bwd_kernel<NV, VEC>), grid, dim3(256), 0, s, dy, dyb, ld_dy, z, rows, dim, ld_z, mean, rstd, gamma, beta, (int)norm, \
                     (int)act, dz, dzb, ld_dz)
  switch (pick_path(z, dim, ld_z, gamma, beta, dz, dz_dtype, ld_dz, dy, dy_dtype, ld_dy)) {
    case PATH_REG4: TRIBE_NA_BWD(4, true); break;
    case PATH_REG16: TRIBE_NA_BWD(16, true); break;
    case PATH_WALK4: TRIBE_NA_BWD(0, true); break;
    default: TRIBE_NA_BWD(0, false); break;
  }
#undef TRIBE_NA_BWD
  TRIBE_LAUNCH_CHECK();
  if (colsums) {
    const unsigned col_blocks = (unsigned)((dim + 63) / 64);
    hipLaunchKernelGGL(norm_act_colsum_kernel, dim3(col_blocks, (unsigned)nparts), dim3(256), 0, s, dy, dyb, ld_dy, z, rows, dim, ld_z, mean, rstd,
                       gamma, beta, (int)act, (double*)workspace);
    hipLaunchKernelGGL(norm_act_colsum_final_kernel, dim3(col_blocks), dim3(256), 0, s, (const double*)workspace, nparts, dim, dgamma, dbeta);
    TRIBE_LAUNCH_CHECK();
  }
  return 0;
}
