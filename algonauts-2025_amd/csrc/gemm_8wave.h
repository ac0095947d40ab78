// bf16 MFMA GEMM for gfx950:  C = epi(alpha * A . B^T),  A [M,K], B [N,K], K contiguous -- the 8-wave kernel template.
// A header because two units instantiate it: gemm_8wave_nb4.hip (256 x 256, with the plane and transposed-operand forms) and
// gemm_8wave_nb3.hip (256 x 192).  They are the two slowest compilations of the library and build side by side.
//
//    256 x (64 NB) x 64, 512 threads (8 waves as 2x4, 128 x (16 NB) per wave, 8 x NB v_mfma_f32_16x16x32_bf16
//    accumulators), 128 KiB LDS = 2 K-tile buffers.  Operands go HBM/L2 -> LDS with
//    global_load_lds_dwordx4 (no VGPR round trip) in "half-tiles" of 128 rows.  A half-tile is the set
//    of tile rows whose fragments are read in ONE phase, so it can be restaged right after that phase:
//    per K-tile there are two phases (two C quadrants = 32 MFMAs per wave each); phase B restages three
//    half-tiles of K-tile t+2, phase A the fourth, and every phase ends its read slot with a COUNTED
//    s_waitcnt vmcnt(8) -- four half-tiles (80 KiB per CU) stay in flight across the raw s_barriers,
//    each with two full phases of slack (the counted-vmcnt schedule of cdna_hip_programming.md
//    section 5, re-derived for 2 LDS buffers).  The two wave groups wr = 0 / 1 (= the two waves of each
//    SIMD) run one barrier apart, so one group's LDS-read slot overlaps the other group's MFMA slot.
//    In-kernel stamps (scripts/gemm_stamps.py): MFMA cluster 42 %, LDS reads 18 %, stage + vmcnt 21 %,
//    barriers 18 % of a wave's K-loop time; matrix pipe ~78 % busy inside the loop.
// The 128 x 128 kernels (gemm_128.hip) take over when M or N is too small to fill 256-wide tiles; all share one operator
// epilogue (gemm_common.h).
// The LDS image is lane-linear (a glds requirement), so the bank-conflict swizzle
// chunk ^= (row & 7) is applied to the per-lane SOURCE address and undone on the ds_read_b128
// fragment read (guide rule 21 / T2).  Roofline: MFMA (dense bf16) -- see DESIGN.md "Kernels".
#pragma once
#include "gemm_launch.h"

namespace {

// =============================================================================================
// 256 x 256 x 64, counted-vmcnt pipeline
// =============================================================================================
namespace big {
constexpr int BM = 256, BN = 256;
constexpr int A_BYTES = BM * BK * 2;          // 32 KiB
constexpr int BUF_BYTES = 2 * A_BYTES;        // A + B of one K-tile: 64 KiB
constexpr int SMEM_BYTES = 2 * BUF_BYTES;     // 128 KiB
}  // namespace big

// Loads a wave leaves in flight at the two steady-state waits.  Experiment (profiles/r02_h_gemm_inflight_experiment.txt): 4 / 2
// instead of 8 cost FF1 +13 % / +28 % and FF2 +30 % / +34 % -- the loop needs its full K-tile of lead; a THIRD A slot (160 KiB
// LDS, A half-tiles issued two K-tiles ahead) bought nothing (3.88 vs 3.89 ms), so the two-buffer ring stays.
#ifndef TRIBE_GEMM_VM_STEADY
#define TRIBE_GEMM_VM_STEADY 8
#endif

// Diagnostic build only (-DTRIBE_GEMM_STAMPS): s_memtime stamps around the slots of the K loop, summed per wave and
// written to a side buffer that no other code reads (its pointer rides in desc.gadd_index while desc.gadd == NULL).
// Never quote the run time of this build; read the SHARES.
#ifdef TRIBE_GEMM_STAMPS
#define TRIBE_STAMP(var)                                                                  \
  do {                                                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                    \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(var)::"memory");           \
    __builtin_amdgcn_sched_barrier(0);                                                    \
  } while (0)
#define TRIBE_STAMP_ACC(slot, t_from, t_to) stamp_acc[slot] += (t_to) - (t_from)
#else
#define TRIBE_STAMP(var) do { } while (0)
#define TRIBE_STAMP_ACC(slot, t_from, t_to) do { } while (0)
#endif

// TN = 1 (desc.trans_ab): the operands arrive TRANSPOSED -- At [K, M] and Bt [K, N] row-major, the layout of the two factors of a
// weight gradient dW = dY^T X as the forward left them -- and C[m][n] = sum_k At[k][m] Bt[k][n].  Same schedule, same LDS bytes; what
// changes is the LDS image (per half-tile [64 k][128 out] rows of 256 bytes, 16-byte chunks XOR-swizzled by (k & 7) << 1 on the source
// side) and the fragment reads (two ds_read_b64_tr_b16 per fragment instead of one ds_read_b128: the hardware transposes; A and B use
// the same k order inside an MFMA, so the sum is unchanged).  Replaces the explicit bf16 transposes of the wgrad operands.
//
// NB = tile columns / 64 (round 3): the tile is 256 x (64 NB), a wave owns 128 x (16 NB), NB accumulator columns of 16.  NB = 4 is
// the 256 x 256 kernel; NB = 3 (256 x 192) exists for grids whose 256-wide tiles quantise badly on 256 CUs -- the BASELINE config at
// B = 4 has M = 4096: QKV 576 tiles (2.25 rounds), out-proj / FF2 192 tiles (0.75 of the chip) become 768 / 256 / 256.  The B tile is
// staged as NB LDS-DMA loads per wave (rows in tile order), all read in phase A and restaged in phase B, so the counted waits leave
// 4 + NB loads in flight.

// Stream-K schedule of the transposed-operand (weight-gradient) form, desc.stream_k: the tiles of the last, PARTIAL round -- rem = tiles % W
// on W CUs -- are cut into W equal runs of q = ceil(rem nk / W) K-steps, one per CU; a run that crosses a tile boundary is two workgroups (its
// part of the first tile, its part of the next), so no workgroup loops.  blockIdx.x: [0, tiles_dp) whole tiles as ever; then W "first parts"
// (worker w = index); then the "second parts" in DESCENDING length (second_worker[]), so that the dispatcher hands the CU whose first part
// was shortest the longest second part -- every CU ends up with ~q K-steps.  A workgroup that holds a whole tile stores it; a partial one
// leaves its accumulators in the workspace (slot 2 w + part, 256 KiB, in register order: 1 KiB per store instruction) and
// streamk_reduce_kernel, launched behind it, sums the parts of every split tile IN ORDER (deterministic) and writes alpha * sum to C.
// (First version: f32 atomics into a zeroed C -- the chip sustains only ~0.65 TB/s of them, ~100 us per 256-KiB part when every CU adds at
// once; profiles/r03_z11_gemm_streamk.txt.)  Only remainders of up to half a round are cut (plan_stream_k, gemm_plan.cpp): dW of FF1 / FF2 at
// B = 16 (576 tiles, remainder 64) and of the projectors (64 tiles); dW of out-proj (144 tiles) and of QKV (remainder 176) measured slower split.
// The fields live in SkSchedule (gemm_plan.h), which the host planner fills; this is the kernels' parameter type.
struct SkSched : SkSchedule {};

// PL (out-proj / FF2 at NB = 4 only): the residual stream as two 16-bit planes, see epilogue_role.
template <int OUT_BF16, int ROLE, int TN = 0, int NB = 4, int PL = 0>
__global__ __launch_bounds__(512, 2) void gemm_nt_256x256x64(const tribe_gemm_desc g, int tiles_m, int tiles_n, const SkSched sk) {
  static_assert(NB >= 2 && NB <= 4 && (!TN || NB == 4), "tile columns: 128, 192 or 256; transposed operands: 256 only");
  static_assert(PL == 0 || (!TN && NB == 4 && !OUT_BF16 && (ROLE == TRIBE_ROLE_OUT_PROJ || ROLE == TRIBE_ROLE_FF2)), "planes: out-proj / FF2, 256 x 256");
  constexpr int BM = big::BM, BN = 64 * NB, A_BYTES = big::A_BYTES, BUF_BYTES = A_BYTES + BN * BK * 2;
  constexpr int WN = 16 * NB;                      // columns per wave
  constexpr int VM_STEADY = NB == 4 ? TRIBE_GEMM_VM_STEADY : 4 + NB;
  extern __shared__ __attribute__((aligned(16))) char smem[];
#ifdef TRIBE_GEMM_STAMPS
  unsigned long long ts_entry = 0, ts_loop = 0, ts_end = 0;
  TRIBE_STAMP(ts_entry);
#endif
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..7
  const int wr = wave >> 2, wc = wave & 3;

  // which tile, which K-steps of it [k_first, k_first + nk), and whether that is the whole tile
  int tile_lin = (int)blockIdx.x, k_first = 0, nk = (int)(g.K / BK);
  bool partial = false;
  int sk_slot = 0;
  if constexpr (TN) {
    if ((int)blockIdx.x >= sk.tiles_dp) {
      const int sidx = (int)blockIdx.x - sk.tiles_dp;
      const bool second = sidx >= sk.workers;
      const int w = second ? (int)sk.second_worker[sidx - sk.workers] : sidx;
      const int u0 = w * sk.q;
      if (u0 >= sk.rem_units) return;                                    // (ceil: the last workers may have nothing)
      const int run = min(sk.q, sk.rem_units - u0);
      const int t_loc = u0 / nk, x = u0 - t_loc * nk, first_len = min(run, nk - x);
      if (second && first_len >= run) return;                            // this worker's run stays inside one tile
      tile_lin = sk.tiles_dp + t_loc + (second ? 1 : 0);
      k_first = second ? 0 : x;
      const int len = second ? run - first_len : first_len;
      partial = len != nk;
      nk = len;
      sk_slot = 2 * w + (second ? 1 : 0);
    }
  }
  int tm, tn;
  tile_coords(tile_lin, tiles_m, tiles_n, tm, tn);
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;

  const int64_t z = blockIdx.y;
  const int64_t b1 = z / g.batch0, b0 = z - b1 * g.batch0;
  const int64_t b1g = g.gather1 ? g.gather1[b1] : b1;
  const unsigned short* A = (const unsigned short*)g.A + (g.gather_a ? b1g : b1) * g.sA1 + b0 * g.sA0;
  const unsigned short* B = (const unsigned short*)g.B + (g.gather_b ? b1g : b1) * g.sB1 + b0 * g.sB0;

  // ---- staging: each LDS-DMA instruction of a wave moves a slab of 8 tile rows x 128 bytes (row r of an operand tile at r * 128) ----
  //   A half h = the 128 tile rows phase h reads: {wr' * 128 + h * 64 + 0..63, wr' = 0, 1}; slab j of this wave: row0 = j * 128 + h * 64 + wave * 8
  //   B: slab q (0 .. NB-1) of this wave: row0 = q * 64 + wave * 8 (TN: the two half images of the round-2 layout, see below)
  const int srow = lane >> 3;
  const int schunk = (lane & 7) ^ srow;  // swizzle on the SOURCE chunk (row & 7 == srow for every slab)
#ifdef TRIBE_ABL_SAME_TILE   // ablation build: every workgroup streams the operand panels of tile (0, 0) -> all L2 hits (results are wrong)
#define m0 ((int64_t)0)
#define n0 ((int64_t)0)
#endif
  const unsigned short* a_src[2][2];
  const unsigned short* b_src[NB];
  int a_lds[2][2], b_lds[NB];  // wave-uniform LDS byte offsets of the slabs inside a K-tile buffer
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (TN) {
        // half-image h of an operand: [64 k][128 out] = 16 pieces of 4 k-rows; piece p = 8 j + wave; lane l fills physical chunk l & 15
        // of k-row 4 p + (l >> 4) from the logical chunk the swizzle maps there.  Logical chunk c of A's half h holds tile rows
        // (c >> 3) * 128 + h * 64 + (c & 7) * 8 .. + 7 (the two wave groups wr), of B's half h tile columns (c >> 2) * 64 + h * 32 +
        // (c & 3) * 8 .. + 7 (the four wc): exactly the rows / columns phase h reads.
        const int piece = 8 * j + wave, krow = 4 * piece + (lane >> 4);
        const int lc = (lane & 15) ^ ((krow & 7) << 1);
        int64_t gm = m0 + (lc >> 3) * 128 + h * 64 + (lc & 7) * 8; gm = gm + 8 <= g.M ? gm : g.M - 8;   // clamp to the last whole chunk
        int64_t gn = n0 + (lc >> 2) * 64 + h * 32 + (lc & 3) * 8; gn = gn + 8 <= g.N ? gn : g.N - 8;
        a_src[h][j] = A + (int64_t)krow * g.lda + gm;
        b_src[(2 * h + j) % NB] = B + (int64_t)krow * g.ldb + gn;
        a_lds[h][j] = h * 16384 + piece * 1024;
        b_lds[(2 * h + j) % NB] = A_BYTES + h * 16384 + piece * 1024;
      } else {
        const int ra = j * 128 + h * 64 + wave * 8;
        int64_t gr = m0 + ra + srow; gr = gr < g.M ? gr : g.M - 1;  // clamp: edge rows re-read a valid row, stores are masked
        a_src[h][j] = A + gr * g.lda + schunk * 8;
        a_lds[h][j] = ra * 128;
      }
    }
  if (!TN) {
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const int rb = q * 64 + wave * 8;
      int64_t gc = n0 + rb + srow; gc = gc < g.N ? gc : g.N - 1;
      b_src[q] = B + gc * g.ldb + schunk * 8;
      b_lds[q] = A_BYTES + rb * 128;
    }
  }

#ifdef TRIBE_ABL_SAME_TILE
#undef m0
#undef n0
#endif
  // which: 0 = A half 0, 1 = the B tile (NB loads), 3 = A half 1
  auto stage = [&](int which, int buf, int kt) {
#ifdef TRIBE_ABL_NO_STAGE   // ablation build (scripts/gemm_ablation.py): no LDS-DMA, the K loop computes on whatever LDS holds
    return;
#endif
    char* base = smem + buf * BUF_BYTES;
    const int64_t koff_a = TN ? (int64_t)kt * BK * g.lda : (int64_t)kt * BK;   // K runs along the rows of a transposed operand
    const int64_t koff_b = TN ? (int64_t)kt * BK * g.ldb : (int64_t)kt * BK;
    if (which == 0 || which == 3) {
      const int h = which == 3;
      __builtin_amdgcn_global_load_lds((gptr_t)(a_src[h][0] + koff_a), (lptr_t)(base + a_lds[h][0]), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(a_src[h][1] + koff_a), (lptr_t)(base + a_lds[h][1]), 16, 0, 0);
    } else {
#pragma unroll
      for (int q = 0; q < NB; ++q)
        __builtin_amdgcn_global_load_lds((gptr_t)(b_src[q] + koff_b), (lptr_t)(base + b_lds[q]), 16, 0, 0);
    }
  };

  f32x4_t acc[8][NB];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < NB; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fq = lane >> 4;
  const int coff0 = ((fq ^ (frow & 7)) << 4), coff1 = (((4 + fq) ^ (frow & 7)) << 4);
  const int a_rd = (wr * 128 + frow) * 128;            // + mh*8192 + i*2048 + coff
  // NT form (TACC): the MFMAs run with their operands SWAPPED and the B fragments are read with their row quads permuted (0, 2, 1, 3), so that
  // every 16 x 16 accumulator holds its sub-tile transposed with lanes l / l + 32 on adjacent column quads -- what epilogue_fast<.., TACC = 1>
  // stores without a quad transpose and, for bf16 outputs, 16 bytes per lane.  The transposed-operand (TN) form keeps the
  // round-2 orientation.
#ifdef TRIBE_GEMM_NO_TACC
  constexpr int TACC = 0;
#else
  constexpr int TACC = TN ? 0 : 1;
#endif
  const int prow = TACC ? ((frow & 3) | ((frow & 4) << 1) | ((frow & 8) >> 1)) : frow;
  const int bcoff0 = ((fq ^ (prow & 7)) << 4), bcoff1 = (((4 + fq) ^ (prow & 7)) << 4);
  const int b_rd = A_BYTES + (wc * WN + prow) * 128;   // + j*2048 + bcoff

  bf16x8_t fa[4][2], fb[NB][2];
#ifdef TRIBE_ABL_NO_LDSREAD
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      fa[i][k] = bf16x8_t{(short)(0x3c00 + lane), (short)0x3f80, (short)(0xbf00 + i), (short)0x3e00, (short)0xbe80, (short)0x3f00, (short)(0x3d00 + k), (short)0xbd00};
      if (i < NB) fb[i][k] = fa[i][k];
    }
#endif

  // TN fragment reads: lane i of a 16-lane group supplies k-row 4 fq + (i >> 2) (and + 16) of the k-step and 4 of the fragment's 16
  // tile rows; after the hardware transpose lane (frow, fq) holds k = {4 fq .. + 3, 16 + 4 fq .. + 3} of tile row frow, for A and B alike.
  // Fragment i of A's half image sits at logical chunks wr * 8 + 2 i (+ 1), fragment j of B's half image nh at wc * 4 + 2 j (+ 1).
  const int tq = frow >> 2, tp = frow & 3;
  const int t_row = 4 * fq + tq, t_sw = (t_row & 7) << 1;
  int ta_off[4], tb_off[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) ta_off[i] = t_row * 256 + (((wr * 8 + 2 * i + (tp >> 1)) ^ t_sw) << 4) + (tp & 1) * 8;
#pragma unroll
  for (int j = 0; j < 2; ++j) tb_off[j] = A_BYTES + t_row * 256 + (((wc * 4 + 2 * j + (tp >> 1)) ^ t_sw) << 4) + (tp & 1) * 8;
  auto tr_frag = [&](const char* p) -> bf16x8_t {   // k-rows r and r + 16 of one k-step
    const s16x4_tn lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_tn*)(p));
    const s16x4_tn hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_tn*)(p + 16 * 256));
    bf16x8_t f;
#pragma unroll
    for (int e = 0; e < 4; ++e) { f[e] = lo[e]; f[4 + e] = hi[e]; }
    return f;
  };

#ifdef TRIBE_ABL_NO_LDSREAD   // ablation build: fragments stay what the prologue put in the registers (opaque to the optimiser)
#define TRIBE_LDS_A(base, MH) _Pragma("unroll") for (int i = 0; i < 4; ++i) { asm volatile("" : "+v"(fa[i][0]), "+v"(fa[i][1])); }
#define TRIBE_LDS_B(base) _Pragma("unroll") for (int j = 0; j < NB; ++j) { asm volatile("" : "+v"(fb[j][0]), "+v"(fb[j][1])); }
#else
#define TRIBE_LDS_A(base, MH)                                                                  \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                              \
    if (TN) {                                                                                  \
      fa[i][0] = tr_frag((base) + (MH) * 16384 + ta_off[i]);                                   \
      fa[i][1] = tr_frag((base) + (MH) * 16384 + ta_off[i] + 32 * 256);                        \
    } else {                                                                                   \
      fa[i][0] = *(const bf16x8_t*)((base) + a_rd + (MH) * 8192 + i * 2048 + coff0);           \
      fa[i][1] = *(const bf16x8_t*)((base) + a_rd + (MH) * 8192 + i * 2048 + coff1);           \
    }                                                                                          \
  }
#define TRIBE_LDS_B(base)                                                                      \
  _Pragma("unroll") for (int j = 0; j < NB; ++j) {                                             \
    if (TN) {                                                                                  \
      fb[j][0] = tr_frag((base) + (j >> 1) * 16384 + tb_off[j & 1]);                           \
      fb[j][1] = tr_frag((base) + (j >> 1) * 16384 + tb_off[j & 1] + 32 * 256);                \
    } else {                                                                                   \
      fb[j][0] = *(const bf16x8_t*)((base) + b_rd + j * 2048 + bcoff0);                        \
      fb[j][1] = *(const bf16x8_t*)((base) + b_rd + j * 2048 + bcoff1);                        \
    }                                                                                          \
  }
#endif
#ifdef TRIBE_ABL_NO_MFMA   // ablation build: the fragments are consumed by an empty asm instead of the matrix pipe
#define TRIBE_MMA(MH)                                                                          \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) { asm volatile("" :: "v"(fa[i][0]), "v"(fa[i][1])); } \
  _Pragma("unroll") for (int j = 0; j < NB; ++j) { asm volatile("" :: "v"(fb[j][0]), "v"(fb[j][1])); }
#else
#define TRIBE_MMA(MH)                                                                          \
  _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                \
  _Pragma("unroll") for (int j = 0; j < NB; ++j) {                                             \
    acc[(MH) * 4 + i][j] = TACC ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j][0], fa[i][0], acc[(MH) * 4 + i][j], 0, 0, 0)   \
                                : __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], fb[j][0], acc[(MH) * 4 + i][j], 0, 0, 0);  \
    acc[(MH) * 4 + i][j] = TACC ? __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j][1], fa[i][1], acc[(MH) * 4 + i][j], 0, 0, 0)   \
                                : __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], fb[j][1], acc[(MH) * 4 + i][j], 0, 0, 0);  \
  }
#endif
// Priority: ONE s_setprio 1 for the younger wave group (wr = 1, the arbitration loser on every slot) before the K loop instead of
// flips around every MFMA cluster (guide T5, static form); the clusters are pinned between their barriers by sched_barrier.  Same-box
// A/B (profiles/r03_b / r03_c_gemm_ablation.txt): FF1 +0.7 ... +5 %, FF2 +0.9 ... +3.6 % across two boxes, 8192^3 +-0.3 %.
#ifdef TRIBE_GEMM_PRIO_FLIPS
#define TRIBE_PRIO_UP() __builtin_amdgcn_s_setprio(1)
#define TRIBE_PRIO_DOWN() __builtin_amdgcn_s_setprio(0)
#else
#define TRIBE_PRIO_UP() __builtin_amdgcn_sched_barrier(0)
#define TRIBE_PRIO_DOWN() __builtin_amdgcn_sched_barrier(0)
#endif
// The fragment reads are retired BEFORE the barrier: the two wave groups (wr = 0 / 1 = the two waves of every
// SIMD) run one barrier apart, so while one group sits in this wait the other group's MFMA cluster owns the
// matrix pipe, and at every barrier all LDS reads issued so far are complete (restaging is then hazard-free).
#define TRIBE_PHASE_SYNC_MMA(MH)                           \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       \
  __builtin_amdgcn_sched_barrier(0);                       \
  TRIBE_STAMP(ts2);                                        \
  __builtin_amdgcn_s_barrier();                            \
  TRIBE_STAMP(ts3);                                        \
  TRIBE_PRIO_UP();                                         \
  TRIBE_MMA(MH)                                            \
  TRIBE_PRIO_DOWN();                                       \
  TRIBE_STAMP(ts4);                                        \
  __builtin_amdgcn_s_barrier();                            \
  TRIBE_STAMP(ts5);                                        \
  TRIBE_STAMP_ACC(1, ts1, ts2); TRIBE_STAMP_ACC(2, ts2, ts3); TRIBE_STAMP_ACC(3, ts3, ts4); TRIBE_STAMP_ACC(4, ts4, ts5);

  // K rotation: the workgroups that share an operand panel in an XCD's L2 (the 4 x 8 patch of tile_coords) walk K from different
  // starting K-tiles, one apart, and wrap around.  Walking in lockstep, all sharers of a line wait on the SAME fill from beyond L2;
  // one K-tile apart, the first brings the line in and the others hit (profiles/r03_b_gemm_ablation.txt: with every load an L2 hit
  // FF1 / FF2 run 5 - 12 / 9 - 17 % faster).  Changes only the order of the f32 accumulation.
  // Measured (profiles/r03_c_gemm_ablation.txt, same box, interleaved): FF1 +2.0 %, FF2 +1.3 %, 8192^3 +0.1 %.
#ifdef TRIBE_GEMM_NO_KROT
  const int krot = 0;
#else
  const int krot = ((tn & 7) + (tm & 3)) % nk;
#endif
  // (Also tried, profiles/r03_h_gemm_kperm.txt: a cyclic shift inside every window of 8 K-tiles, which spreads the first touches evenly
  // over the sharers instead of leaving them to the one that walks ahead -- FF1 / FF2 / QKV within +-0.7 % of the plain rotation.)
  auto ktile = [&](int t) { const int k = t + krot; return k_first + (k >= nk ? k - nk : k); };
#ifdef TRIBE_GEMM_STAMPS
  unsigned long long ts0 = 0, ts1 = 0, ts2 = 0, ts3 = 0, ts4 = 0, ts5 = 0;
  unsigned long long stamp_acc[5] = {0, 0, 0, 0, 0};  // 0 LDS reads, 1 stage + vmcnt wait, 2 barrier 1, 3 MFMA cluster, 4 barrier 2
#endif

  // ---- prologue: K-tile 0 completely, K-tile 1 minus its last half-tile ----
  stage(0, 0, ktile(0)); stage(1, 0, ktile(0)); stage(3, 0, ktile(0));
  if (nk > 1) {
    stage(0, 1, ktile(1)); stage(1, 1, ktile(1));
    wait_vmcnt<2 + NB>();
  } else {
    wait_vmcnt<0>();
  }
  __builtin_amdgcn_s_barrier();
  // stagger: group wr = 1 runs one barrier behind group wr = 0 for the whole K loop (LDS-read slots of one
  // group overlap MFMA slots of the other); group 0 pays the matching barrier after the loop.
  if (wr == 1) __builtin_amdgcn_s_barrier();
#if !defined(TRIBE_GEMM_PRIO_FLIPS) && !defined(TRIBE_ABL_NO_PRIO)
  if (wr == 1) __builtin_amdgcn_s_setprio(1);
#endif

  TRIBE_STAMP(ts_loop);
  for (int t = 0; t < nk; ++t) {
    const int cur = t & 1;
    const char* base = smem + cur * BUF_BYTES;
    // ---- phase A: accumulator rows 0..3 x all NB columns: 2 NB + 8 fragment reads, 8 NB MFMAs.  Restage: the last half-tile
    // (A half 1) of K-tile t+1 into the other buffer (its previous content was last read in phase B of K-tile t-1).
    TRIBE_STAMP(ts0);
    TRIBE_LDS_B(base)
    TRIBE_LDS_A(base, 0)
    TRIBE_STAMP(ts1);
    TRIBE_STAMP_ACC(0, ts0, ts1);
    // retire A half 1 of THIS K-tile (read in phase B): behind it in the queue are A half 0 + B of K-tile t+1 issued in the
    // previous phase B (2 + NB loads) and the half-tile issued just now (2)
    if (t + 1 < nk) { stage(3, cur ^ 1, ktile(t + 1)); wait_vmcnt<VM_STEADY>(); } else { wait_vmcnt<0>(); }
    TRIBE_PHASE_SYNC_MMA(0)
    // ---- phase B: accumulator rows 4..7: 8 fragment reads (the B fragments stay in registers), 8 NB MFMAs.  A half 0 and the
    // B tile of THIS buffer were last read in phase A -> restage them for K-tile t+2.
    TRIBE_STAMP(ts0);
    TRIBE_LDS_A(base, 1)
    TRIBE_STAMP(ts1);
    TRIBE_STAMP_ACC(0, ts0, ts1);
    if (t + 2 < nk) {
      const int k2 = ktile(t + 2);
      stage(0, cur, k2); stage(1, cur, k2);
      wait_vmcnt<VM_STEADY>();  // retire A0 / B of K-tile t+1; behind them: A1(t+1) (2) and the 2 + NB just issued
    } else if (t + 1 < nk) {
      wait_vmcnt<2>();  // behind them: only A1(t+1)
    }
    TRIBE_PHASE_SYNC_MMA(1)
  }
  if (wr == 0) __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_s_setprio(0);
  TRIBE_STAMP(ts_end);
#ifdef TRIBE_GEMM_STAMPS
  if (g.gadd == nullptr && g.gadd_index != nullptr && lane == 0 && blockIdx.y == 0) {
    unsigned long long* dbg = (unsigned long long*)g.gadd_index + ((size_t)blockIdx.x * 8 + wave) * 8;
    for (int i = 0; i < 5; ++i) dbg[i] = stamp_acc[i];
  }
#endif
#undef TRIBE_LDS_A
#undef TRIBE_LDS_B
#undef TRIBE_MMA
#undef TRIBE_PHASE_SYNC_MMA

  // ---- epilogue straight from registers (quad transpose -> one 16-/8-byte store per lane).  Staging the sub-tile
  // through LDS to get whole-row 256-byte stores was measured 2x SLOWER (K = 64 probe: 158 vs 75 us f32, 138 vs 43 us
  // bf16 per 16384 x 3072 output): the extra LDS round trip costs more than the wider store segments save.
  const EpiCtx ctx = make_epi_ctx(g, b1, b0, b1g);
  if constexpr (TN && !OUT_BF16) {
    if (partial) {
      // part of a tile's reduction (stream-K): the raw accumulators go to this part's workspace slot in register order
      float* slot = sk.ws + (int64_t)sk_slot * SK_SLOT_FLOATS + tid * 4;
      static_for<8 * NB>([&](auto t) {
        constexpr int i = decltype(t)::value / NB, j = decltype(t)::value % NB;
        *(f32x4_t*)(slot + (i * NB + j) * 2048) = acc[i][j];
      });
      return;
    }
  }
  // The four encoder roles: the epilogue compiled for exactly their operator set, and nothing else -- the launcher (role8_ok) sends these
  // instantiations only descriptors that carry it (un-batched, alpha == 1, N a multiple of the tile width, 16-byte operands); every other
  // launch of such a role runs under the GENERIC symbol.
  constexpr bool ROLE_EPI = TACC && (ROLE == TRIBE_ROLE_QKV || ROLE == TRIBE_ROLE_FF1 || ROLE == TRIBE_ROLE_OUT_PROJ || ROLE == TRIBE_ROLE_FF2);
  if constexpr (ROLE_EPI) {
    epilogue_role<OUT_BF16, ROLE, 8, NB, TACC, PL>(g, acc, m0 + wr * 128, n0 + wc * WN, lane, smem + wave * (4 * NB * 1024));
  } else if (epilogue_fast_ok<(ROLE == TRIBE_ROLE_EXT)>(g, ctx) && n0 + BN <= g.N) {
    // nothing inside the sub-tile loop waits on memory (gemm_common.h); the staging buffers are idle by now
    epilogue_fast<OUT_BF16, 8, NB, (ROLE == TRIBE_ROLE_EXT), TACC>(g, ctx, acc, m0 + wr * 128, n0 + wc * WN, lane, smem + wave * (4 * NB * 1024));
  } else {
    static_for<8 * NB>([&](auto t) {
      constexpr int i = decltype(t)::value / NB, j = decltype(t)::value % NB;
      epilogue_tile16<OUT_BF16, (ROLE == TRIBE_ROLE_EXT), TACC>(g, ctx, acc[i][j], m0 + wr * 128 + i * 16, n0 + wc * WN + j * 16, lane);
    });
  }
#ifdef TRIBE_GEMM_STAMPS
  // slots 5 .. 7: kernel entry -> first K-loop iteration; end of the K loop -> last store issued; -> every store retired (wave end)
  TRIBE_STAMP(ts1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  TRIBE_STAMP(ts2);
  if (g.gadd == nullptr && g.gadd_index != nullptr && lane == 0 && blockIdx.y == 0) {
    unsigned long long* dbg = (unsigned long long*)g.gadd_index + ((size_t)blockIdx.x * 8 + wave) * 8;
    dbg[5] = ts_loop - ts_entry; dbg[6] = ts1 - ts_end; dbg[7] = ts2 - ts_end;
  }
#endif
}

}  // namespace

namespace tribe_gemm_detail {
// a planned schedule as the kernels' parameter, its parts travelling through the workspace `ws`
inline SkSched kernel_arg(const SkSchedule& plan, void* ws = nullptr) {
  SkSched k{};
  static_cast<SkSchedule&>(k) = plan;
  k.ws = (float*)ws;
  return k;
}
}  // namespace tribe_gemm_detail
