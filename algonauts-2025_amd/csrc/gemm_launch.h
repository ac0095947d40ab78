// What the bf16 GEMM's translation units share: the K step, two device helpers, and the launch tables' interface.
//
// Launch tables.  Each kernel family is one unit, compiled once: gemm_8wave_nb4.hip (the 8-wave 256 x 256 kernel with its plane and
// transposed-operand forms, and the stream-K reduce), gemm_8wave_nb3.hip (the same template at 256 x 192), gemm_128.hip (the two
// 128 x 128 kernels and the split-K epilogue) and gemm_4wave.hip (the one-wave-per-SIMD 256 x 256 kernel).  A unit instantiates its
// kernels through the launch_* tables it DEFINES; gemm.hip, which holds the C entry points and no GEMM kernel, calls them through the
// declarations below.  Which table a launch goes through, and with which pair, grid and schedule, is decided in gemm_plan.cpp (host code
// only, no kernel: gemm_resolve); the list of pairs, TRIBE_GEMM_PAIRS, lives in gemm_plan.h.
// ROLE gives each call site of the path its own kernel symbol, so that rocprofv3 --stats reports per-operator rows; in the 8-wave NT kernel the
// four encoder roles (QKV, FF1, OUT_PROJ, FF2) also compile the epilogue of exactly their operator set (epilogue_role, planner: role8_ok).
#pragma once
#include "gemm_common.h"
#include "gemm_plan.h"

namespace {
constexpr int BK = tribe_gemm_detail::K_STEP;
typedef __attribute__((ext_vector_type(4))) short s16x4_tn;   // operand of ds_read_b64_tr_b16
template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
}  // namespace

namespace tribe_gemm_detail {
// gemm_8wave_nb4.hip.  The transposed-operand launch takes the planned schedule `sk` (its parts travel through desc.stream_k_ws) and, for
// a stream-K launch (reduce_grid_x != 0), puts the reduce kernel behind the GEMM.
void launch_big4(int pair, dim3 grid, hipStream_t s, const tribe_gemm_desc* d, int tiles_m, int tiles_n);
void launch_big4_tn(int bf, dim3 grid, hipStream_t s, const tribe_gemm_desc* d, int tiles_m, int tiles_n, const SkSchedule& sk, unsigned reduce_grid_x);
void launch_big4_planes(dim3 grid, hipStream_t s, const tribe_gemm_desc* d, int tiles_m, int tiles_n);
// gemm_8wave_nb3.hip
void launch_big3(int pair, dim3 grid, hipStream_t s, const tribe_gemm_desc* d, int tiles_m, int tiles_n);
// gemm_128.hip
void launch_ring(int pair, dim3 grid, hipStream_t s, const tribe_gemm_desc* d, int tiles_m, int tiles_n, int splits, float* ws);
void launch_splitk_epilogue(int bf, hipStream_t s, const tribe_gemm_desc* d, int splits, const float* ws);
void launch_small(int pair, dim3 grid, hipStream_t s, const tribe_gemm_desc* d, int tiles_m, int tiles_n);
// gemm_4wave.hip
void launch_4w(int pair, dim3 grid, hipStream_t s, const tribe_gemm_desc* d, int tiles_m, int tiles_n);

// a table over every pair: the unit defines TRIBE_GEMM_CASE_<NAME>(idx, bf, role), one `case idx: launch_k<...>(...); break;`
#define TRIBE_GEMM_TABLE(NAME)                                                                                         \
  void NAME(int pair, dim3 grid, hipStream_t s, const tribe_gemm_desc* d, int tiles_m, int tiles_n) {                  \
    switch (pair) {                                                                                                    \
      TRIBE_GEMM_PAIRS(TRIBE_GEMM_CASE_##NAME)                                                                         \
      default: break;                                                                                                  \
    }                                                                                                                  \
  }
}  // namespace tribe_gemm_detail
