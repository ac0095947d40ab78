// What a GEMM launch will be, decided once on the host (gemm_plan.cpp): every check of the descriptor, the kernel and its tiles, the kernel
// symbol, the grid, the split-K / stream-K schedule and the workspace it needs.  tribe_gemm_bf16 / tribe_gemm_fp8 launch from this struct and
// the three queries (tribe_gemm_stream_k_workspace_bytes, tribe_gemm_sumsq_slots, tribe_gemm_epilogue_path) read it.  Host code only: no
// HIP header, so that the planner builds in seconds and apart from the kernel instantiations.
#pragma once
#include <stdint.h>

#include "../../include/tribe_hip.h"

void tribe_set_error(const char* fmt, ...);

// The stream-K schedule the transposed-operand kernel takes by value (gemm_8wave.h wraps it as its kernel-parameter type SkSched; the
// schedule itself is described there).
struct SkSchedule {
  int tiles_dp;   // tiles (linear index < tiles_dp) computed whole; >= tiles_m * tiles_n: no stream-K
  int rem_units;  // K-steps of the stream-K region: (tiles - tiles_dp) * nk
  int q;          // K-steps per worker
  int workers;
  float* ws;      // 2 * workers slots of 256 x 256 f32
  unsigned short second_worker[256];
};
constexpr int SK_SLOT_FLOATS = 256 * 256;
constexpr int TRIBE_ROLE_EXT = 100;  // kernel instantiation carrying the extended epilogue (see gemm_common.h)

namespace tribe_gemm_detail {
constexpr int K_STEP = 64;        // BK of every bf16 kernel
constexpr int K_STEP_FP8 = 128;
enum { KIND_SMALL = 0, KIND_BIG = 1, KIND_RING = 2, KIND_BIG4W = 3 };
// (kernel symbol, output is bf16, role template argument) of every pair that exists as a kernel; every other (dtype, role) combination
// runs under the GENERIC symbol of its dtype.  The launch tables (gemm_launch.h) and the enum below are generated from this list.
#define TRIBE_GEMM_PAIRS(X)                                                                                            \
  X(PAIR_GENERIC_BF16, 1, TRIBE_ROLE_GENERIC) X(PAIR_GENERIC_F32, 0, TRIBE_ROLE_GENERIC)                               \
  X(PAIR_EXT_BF16, 1, TRIBE_ROLE_EXT) X(PAIR_EXT_F32, 0, TRIBE_ROLE_EXT)                                               \
  X(PAIR_PROJECTOR, 0, TRIBE_ROLE_PROJECTOR) X(PAIR_QKV, 1, TRIBE_ROLE_QKV) X(PAIR_ATTN_SCORES, 0, TRIBE_ROLE_ATTN_SCORES) \
  X(PAIR_ATTN_PV, 1, TRIBE_ROLE_ATTN_PV) X(PAIR_OUT_PROJ, 0, TRIBE_ROLE_OUT_PROJ) X(PAIR_FF1, 1, TRIBE_ROLE_FF1)       \
  X(PAIR_FF2, 0, TRIBE_ROLE_FF2) X(PAIR_VOXEL_HEAD, 0, TRIBE_ROLE_VOXEL_HEAD)
// the four of them whose 8-wave kernel holds ONLY the epilogue compiled for the role's operator set (epilogue_role), and the only
// ones the one-wave-per-SIMD kernel exists for (epilogue_w4)
#define TRIBE_GEMM_ROLE_PAIRS(X) \
  X(PAIR_QKV, 1, TRIBE_ROLE_QKV) X(PAIR_OUT_PROJ, 0, TRIBE_ROLE_OUT_PROJ) X(PAIR_FF1, 1, TRIBE_ROLE_FF1) X(PAIR_FF2, 0, TRIBE_ROLE_FF2)
#define TRIBE_GEMM_PAIR_ENUM(pair, bf, role) pair,
enum GemmPair { TRIBE_GEMM_PAIRS(TRIBE_GEMM_PAIR_ENUM) PAIR_COUNT };
#undef TRIBE_GEMM_PAIR_ENUM

struct GemmLaunch {
  int kind, bm, bn, sumsq_cols, splits;   // kernel, tile, columns per row_sumsq slot (one slot per wave column group), split-K shares (1 = none)
  int pair;                               // GemmPair: the kernel symbol
  int epilogue_path;                      // 0 generic, 1 role (8-wave), 2 one-wave-per-SIMD
  int64_t tiles_m, tiles_n, nz;
  unsigned grid_x, reduce_grid_x;         // reduce_grid_x: the second launch of stream-K (0 = none)
  SkSchedule sk;                          // no_stream_k() when not split; sk.ws stays null (the launcher points it at desc.stream_k_ws)
  int64_t ws_need;                        // bytes of stream_k_ws this launch needs, 0 = not split
};

inline SkSchedule no_stream_k() { return SkSchedule{0x7fffffff}; }   // every tile whole
// Stream-K plan of a launch with `tiles` output tiles of nk K-steps each on cu_count compute units: fills *sk and returns the grid size.
unsigned plan_stream_k(int tiles, int nk, int cu_count, SkSchedule* sk);
// The plan alone, without a check (the queries take half-filled descriptors).
GemmLaunch gemm_plan(const tribe_gemm_desc* d, int cu_count);
// Every check of tribe_gemm_bf16 (`who` = the message prefix) but the workspace's, and the plan.  0, or -1 with tribe_last_error set.
int gemm_resolve(const tribe_gemm_desc* d, const char* who, int cu_count, GemmLaunch* out);
// desc.stream_k_ws against out->ws_need
int gemm_check_workspace(const tribe_gemm_desc* d, const char* who, const GemmLaunch& launch);
// tribe_gemm_fp8: the shared descriptor checks, its own, and the one kernel's grid (pair = GENERIC or EXT of the dtype)
int gemm_fp8_resolve(const tribe_gemm_desc* d, const char* who, GemmLaunch* out);
}  // namespace tribe_gemm_detail
