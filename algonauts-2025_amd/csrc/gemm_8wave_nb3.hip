// The 8-wave GEMM kernel (gemm_8wave.h) at NB = 3, 256 x 192 tiles: the NT table over every (dtype, role) pair, for grids whose 256-wide
// tiles quantise badly on the chip's compute units (the planner picks it: gemm_plan.cpp).
#include "gemm_8wave.h"

namespace tribe_gemm_detail {
#define TRIBE_GEMM_CASE_launch_big3(idx, bf, role) \
  case idx: launch_k<gemm_nt_256x256x64<bf, role, 0, 3>, 512, 2 * (big::A_BYTES + 192 * BK * 2)>(grid, s, d, tiles_m, tiles_n, kernel_arg(no_stream_k())); break;
TRIBE_GEMM_TABLE(launch_big3)
}  // namespace tribe_gemm_detail
