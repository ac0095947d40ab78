// The 8-wave GEMM kernel (gemm_8wave.h) at NB = 4, 256 x 256 tiles: the NT table over every (dtype, role) pair, the plane forms of the
// two residual roles, the transposed-operand (weight-gradient) form and the reduce kernel behind its stream-K launches.
#include "gemm_8wave.h"

namespace {
// Second launch of a stream-K GEMM: workgroup t sums the parts of tile tiles_dp + t in worker order (first parts and second parts of the runs
// that touch it) and writes alpha * sum.  Thread tid holds the same 128 values the GEMM kernel's thread tid held: accumulator register r of
// sub-tile (i, j) of lane l is D[4 (l >> 4) + r][l & 15] of the 16 x 16 sub-tile at rows wr 128 + 16 i, columns wc 64 + 16 j.
__global__ __launch_bounds__(512) void streamk_reduce_kernel(const tribe_gemm_desc g, int tiles_m, int tiles_n, const SkSched sk) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 2, wc = wave & 3;
  const int nk = (int)(g.K / BK);
  const int t_loc = (int)blockIdx.x;
  const int u_lo = t_loc * nk, u_hi = u_lo + nk - 1;
  const int w_lo = u_lo / sk.q, w_hi = u_hi / sk.q;
  if (w_lo == w_hi) return;   // one run holds the whole tile: stored by the GEMM kernel itself
  int tm, tn;
  tile_coords(sk.tiles_dp + t_loc, tiles_m, tiles_n, tm, tn);
  const int64_t m0 = (int64_t)tm * 256, n0 = (int64_t)tn * 256;
  float* C = (float*)g.C;
  for (int sub = 0; sub < 32; ++sub) {
    f32x4_t sum = {0.f, 0.f, 0.f, 0.f};
    for (int w = w_lo; w <= w_hi; ++w) {
      const int part = w * sk.q < u_lo ? 1 : 0;   // the run began in the previous tile: this tile holds its second part
      sum += *(const f32x4_t*)(sk.ws + (int64_t)(2 * w + part) * SK_SLOT_FLOATS + sub * 2048 + tid * 4);
    }
    const int i = sub >> 2, j = sub & 3;
    const int64_t col = n0 + wc * 64 + j * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = m0 + wr * 128 + i * 16 + 4 * (lane >> 4) + r;
      if (row < g.M && col < g.N) C[row * g.ldc + col] = sum[r] * g.alpha;
    }
  }
}
}  // namespace

namespace tribe_gemm_detail {
#define TRIBE_GEMM_CASE_launch_big4(idx, bf, role) \
  case idx: launch_k<gemm_nt_256x256x64<bf, role, 0, 4>, 512, big::SMEM_BYTES>(grid, s, d, tiles_m, tiles_n, kernel_arg(no_stream_k())); break;
TRIBE_GEMM_TABLE(launch_big4)
// the plane forms of the two residual roles (desc.c_dtype = an enum tribe_c_planes value; gemm_resolve lets nothing else through)
template <int ROLE>
static void launch_planes_of(dim3 grid, hipStream_t s, const tribe_gemm_desc* d, int tiles_m, int tiles_n) {
  const SkSched sk = kernel_arg(no_stream_k());
  switch (d->c_dtype) {
    case TRIBE_F32_PLANES_OUT: launch_k<gemm_nt_256x256x64<0, ROLE, 0, 4, 1>, 512, big::SMEM_BYTES>(grid, s, d, tiles_m, tiles_n, sk); break;
    case TRIBE_F32_PLANES_INOUT: launch_k<gemm_nt_256x256x64<0, ROLE, 0, 4, 2>, 512, big::SMEM_BYTES>(grid, s, d, tiles_m, tiles_n, sk); break;
    default: launch_k<gemm_nt_256x256x64<0, ROLE, 0, 4, 3>, 512, big::SMEM_BYTES>(grid, s, d, tiles_m, tiles_n, sk); break;
  }
}
void launch_big4_planes(dim3 grid, hipStream_t s, const tribe_gemm_desc* d, int tiles_m, int tiles_n) {
  if (d->role == TRIBE_ROLE_OUT_PROJ) launch_planes_of<TRIBE_ROLE_OUT_PROJ>(grid, s, d, tiles_m, tiles_n);
  else launch_planes_of<TRIBE_ROLE_FF2>(grid, s, d, tiles_m, tiles_n);
}
// transposed operands: a stream-K launch leaves the split tiles to the reduce kernel
void launch_big4_tn(int bf, dim3 grid, hipStream_t s, const tribe_gemm_desc* d, int tiles_m, int tiles_n, const SkSchedule& plan, unsigned reduce_grid_x) {
  const SkSched sk = kernel_arg(plan, d->stream_k_ws);
  if (bf) launch_k<gemm_nt_256x256x64<1, TRIBE_ROLE_GENERIC, 1, 4>, 512, big::SMEM_BYTES>(grid, s, d, tiles_m, tiles_n, sk);
  else launch_k<gemm_nt_256x256x64<0, TRIBE_ROLE_GENERIC, 1, 4>, 512, big::SMEM_BYTES>(grid, s, d, tiles_m, tiles_n, sk);
  if (reduce_grid_x) hipLaunchKernelGGL(streamk_reduce_kernel, dim3(reduce_grid_x), dim3(512), 0, s, *d, tiles_m, tiles_n, sk);
}
}  // namespace tribe_gemm_detail
