// The bf16 GEMM's 128 x 128 tile kernels, for launches whose M or N is too small to fill the 256-wide tiles of the 8-wave kernel
// (gemm_8wave.h; same operands, same operator epilogue, same swizzled lane-linear LDS image):
//  * gemm_nt_128x128x64: 256 threads (4 waves, 64x64 per wave), double buffered, one vmcnt(0)+barrier per K-tile;
//  * gemm_nt_ring128: 8 waves over a ring of four stages, for grids of about one workgroup per CU, with a split-K form whose shares
//    splitk_epilogue_kernel sums.
#include "gemm_launch.h"

namespace {

// =============================================================================================
// 128 x 128 x 64, double buffered
// =============================================================================================
namespace small {
constexpr int BM = 128, BN = 128;
constexpr int TILE_BYTES = BM * BK * 2;       // 16 KiB per operand tile
constexpr int BUF_BYTES = 2 * TILE_BYTES;     // A + B
constexpr int SMEM_BYTES = 2 * BUF_BYTES;     // double buffered: 64 KiB
}  // namespace small

// ROLE only gives each call site of the path its own kernel symbol, so that rocprofv3 --stats and the
// in-library HIP-event profile (tribe_prof_*) report per-operator durations; the code is identical.
template <int OUT_BF16, int ROLE>
__global__ __launch_bounds__(256, 2) void gemm_nt_128x128x64(const tribe_gemm_desc g, int tiles_m, int tiles_n) {
  using namespace small;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;

  int tm, tn;
  tile_coords(blockIdx.x, tiles_m, tiles_n, tm, tn);
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;

  const int64_t z = blockIdx.y;
  const int64_t b1 = z / g.batch0, b0 = z - b1 * g.batch0;
  const int64_t b1g = g.gather1 ? g.gather1[b1] : b1;
  const unsigned short* A = (const unsigned short*)g.A + (g.gather_a ? b1g : b1) * g.sA1 + b0 * g.sA0;
  const unsigned short* B = (const unsigned short*)g.B + (g.gather_b ? b1g : b1) * g.sB1 + b0 * g.sB0;

  // ---- staging addresses: pass p covers tile rows [32p, 32p+32), wave w rows 8w.. of those ----
  const int srow = lane >> 3;
  const int schunk = (lane & 7) ^ srow;  // swizzle on the source chunk
  const unsigned short* a_src[4];
  const unsigned short* b_src[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r = p * 32 + wave * 8 + srow;
    int64_t gr = m0 + r; gr = gr < g.M ? gr : g.M - 1;   // clamp: edge rows re-read a valid row, stores are masked
    int64_t gc = n0 + r; gc = gc < g.N ? gc : g.N - 1;
    a_src[p] = A + gr * g.lda + schunk * 8;
    b_src[p] = B + gc * g.ldb + schunk * 8;
  }

  auto stage = [&](int buf, int kt) {
    char* base = smem + buf * BUF_BYTES + wave * 1024;
    const int koff = kt * BK;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      __builtin_amdgcn_global_load_lds((gptr_t)(a_src[p] + koff), (lptr_t)(base + p * 4096), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(b_src[p] + koff), (lptr_t)(base + TILE_BYTES + p * 4096), 16, 0, 0);
    }
  };

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fq = lane >> 4;
  const int a_base = (wr * 64 + frow) * 128;
  const int b_base = TILE_BYTES + (wc * 64 + frow) * 128;

  auto compute = [&](int buf) {
    const char* base = smem + buf * BUF_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int coff = (((ks * 4 + fq) ^ (frow & 7)) << 4);
      bf16x8_t a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = *(const bf16x8_t*)(base + a_base + i * 2048 + coff);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = *(const bf16x8_t*)(base + b_base + j * 2048 + coff);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  };

  const int nk = (int)(g.K / BK);
  stage(0, 0);
  __syncthreads();  // hipcc emits vmcnt(0) before the barrier while a glds is in flight
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
    compute(cur);
    __syncthreads();
  }

  const EpiCtx ctx = make_epi_ctx(g, b1, b0, b1g);
  if (epilogue_fast_ok<(ROLE == TRIBE_ROLE_EXT)>(g, ctx) && n0 + BN <= g.N) {
    // (the K loop ends with a barrier: every wave's fragment reads are done, the buffers can stage the residual)
    epilogue_fast<OUT_BF16, 4, 4, (ROLE == TRIBE_ROLE_EXT)>(g, ctx, acc, m0 + wr * 64, n0 + wc * 64, lane, smem + wave * 16384);
    return;
  }
  static_for<16>([&](auto t) {
    constexpr int i = decltype(t)::value / 4, j = decltype(t)::value % 4;
    epilogue_tile16<OUT_BF16, (ROLE == TRIBE_ROLE_EXT)>(g, ctx, acc[i][j], m0 + wr * 64 + i * 16, n0 + wc * 64 + j * 16, lane);
  });
}


// =============================================================================================
// 128 x 128 x 64 ring (round 3): small grids -- at most ~one workgroup per CU
// =============================================================================================
// The double-buffered 128^2 kernel above waits vmcnt(0) + barrier once per K-tile with one K-tile in flight.  That is fine with two
// or three workgroups per CU covering for each other, and slow when the grid gives a CU ONE workgroup (BASELINE config at B = 4:
// projector and voxel head are 256 tiles of 128^2 -- 0.18 / 0.16 of the MFMA peak in BENCH_r02): every K-step then pays a whole
// L2 -> LDS round trip.  Here: 8 waves (two per SIMD; a wave owns 32 x 64), four 32-KiB stages = 128 KiB of LDS, THREE K-tiles in
// flight by LDS-DMA across ONE raw barrier per K-tile with counted waits:
//   iteration t:  s_waitcnt vmcnt(8)  (own loads of K-tile t landed; t+1, t+2 stay in flight)
//                 s_barrier           (everybody's have; and everybody finished reading K-tile t-1: its reads were retired before
//                                      the MFMAs of iteration t-1)
//                 issue K-tile t+3 into the stage K-tile t-1 occupied
//                 12 ds_read_b128, 16 MFMAs
// Per K-step a CU moves 32 KiB from L2 for 512 MFMA cycles, so the stream (~0.5-0.6 us per 32 KiB per CU) bounds it, not the
// matrix pipe; 96 KiB in flight keep that stream busy.
namespace ring {
constexpr int BM = 128, BN = 128, STAGES = 4;
constexpr int TILE_BYTES = BM * BK * 2;           // 16 KiB per operand tile
constexpr int STAGE_BYTES = 2 * TILE_BYTES;       // A + B
constexpr int SMEM_BYTES = STAGES * STAGE_BYTES;  // 128 KiB
}  // namespace ring

// Split-K (round 3, desc.stream_k on an NT launch): grids far below one round of tiles -- M = 128 rows, BASELINE config 1: FF2 is 24 tiles of
// 192 K-steps -- run `splits` workgroups per tile, each over a contiguous share of the K-steps; they store their raw accumulators to
// ws[split][M][N] (f32) and splitk_epilogue_kernel, launched behind, sums the shares in order and applies the launch's epilogue operators.
template <int OUT_BF16, int ROLE>
__global__ __launch_bounds__(512, 2) void gemm_nt_ring128(const tribe_gemm_desc g, int tiles_m, int tiles_n, int splits, float* ws) {
  using namespace ring;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0..7
  const int wr = wave >> 1, wc = wave & 1;                    // 4 x 2 waves of 32 x 64

  const int ntile = tiles_m * tiles_n;
  const int split = splits > 1 ? (int)blockIdx.x / ntile : 0;
  int tm, tn;
  tile_coords((int)blockIdx.x - split * ntile, tiles_m, tiles_n, tm, tn);
  const int64_t m0 = (int64_t)tm * BM, n0 = (int64_t)tn * BN;

  const int64_t z = blockIdx.y;
  const int64_t b1 = z / g.batch0, b0 = z - b1 * g.batch0;
  const int64_t b1g = g.gather1 ? g.gather1[b1] : b1;
  const unsigned short* A = (const unsigned short*)g.A + (g.gather_a ? b1g : b1) * g.sA1 + b0 * g.sA0;
  const unsigned short* B = (const unsigned short*)g.B + (g.gather_b ? b1g : b1) * g.sB1 + b0 * g.sB0;

  // staging: a tile is 16 slabs of 8 rows x 128 bytes (row r at r * 128, 16-byte chunks XOR-swizzled by r & 7 on the SOURCE side);
  // this wave moves slabs `wave` and `wave + 8` of both operands: 4 LDS-DMA loads per K-tile
  const int srow = lane >> 3;
  const int schunk = (lane & 7) ^ srow;
  const unsigned short* a_src[2];
  const unsigned short* b_src[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int r = (wave + 8 * p) * 8 + srow;
    int64_t gr = m0 + r; gr = gr < g.M ? gr : g.M - 1;   // clamp: edge rows re-read a valid row, stores are masked
    int64_t gc = n0 + r; gc = gc < g.N ? gc : g.N - 1;
    a_src[p] = A + gr * g.lda + schunk * 8;
    b_src[p] = B + gc * g.ldb + schunk * 8;
  }
  const int nk_all = (int)(g.K / BK);
  const int k_first = splits > 1 ? (int)((int64_t)split * nk_all / splits) : 0;
  const int nk = splits > 1 ? (int)((int64_t)(split + 1) * nk_all / splits) - k_first : nk_all;
  auto stage = [&](int buf, int kt) {
    char* base = smem + buf * STAGE_BYTES + wave * 1024;
    const int koff = (k_first + kt) * BK;
    __builtin_amdgcn_global_load_lds((gptr_t)(a_src[0] + koff), (lptr_t)(base), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gptr_t)(b_src[0] + koff), (lptr_t)(base + TILE_BYTES), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gptr_t)(a_src[1] + koff), (lptr_t)(base + 8192), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((gptr_t)(b_src[1] + koff), (lptr_t)(base + TILE_BYTES + 8192), 16, 0, 0);
  };

  f32x4_t acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  const int frow = lane & 15, fq = lane >> 4;
  const int coff0 = ((fq ^ (frow & 7)) << 4), coff1 = (((4 + fq) ^ (frow & 7)) << 4);
  const int a_rd = (wr * 32 + frow) * 128;                 // + i * 2048 + coff
  const int b_rd = TILE_BYTES + (wc * 64 + frow) * 128;    // + j * 2048 + coff

  if (0 < nk) stage(0, 0);
  if (1 < nk) stage(1, 1);
  if (2 < nk) stage(2, 2);
  bf16x8_t fa[2][2], fb[4][2];
  auto sync_and_restage = [&](int t) {
    const int ahead = nk - 1 - t;   // K-tiles issued behind K-tile t (capped at 2 by the ring)
    if (ahead >= 2) wait_vmcnt<8>(); else if (ahead == 1) wait_vmcnt<4>(); else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    if (t + 3 < nk) stage((t + 3) & 3, t + 3);
  };
  auto read_frags = [&](int t) {
    const char* base = smem + (t & 3) * STAGE_BYTES;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      fb[j][0] = *(const bf16x8_t*)(base + b_rd + j * 2048 + coff0);
      fb[j][1] = *(const bf16x8_t*)(base + b_rd + j * 2048 + coff1);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      fa[i][0] = *(const bf16x8_t*)(base + a_rd + i * 2048 + coff0);
      fa[i][1] = *(const bf16x8_t*)(base + a_rd + i * 2048 + coff1);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every read retired before the next barrier can be reached (restaging is then safe)
    __builtin_amdgcn_sched_barrier(0);
  };
  auto mma = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], fb[j][0], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], fb[j][1], acc[i][j], 0, 0, 0);
      }
    __builtin_amdgcn_sched_barrier(0);
  };
  // Tried and left off (-DTRIBE_RING_STAGGER): the two waves of a SIMD (w and w + 4) run the same program, so waves 4..7 were made to
  // run their MFMAs half an iteration late (multiply K-tile t-1 while waves 0..3 read K-tile t; guide: "two waves per SIMD that run the
  // same program with one barrier per block: try a stagger").  Same-box A/B (profiles/r03_f_gemm_tiles*.txt): projector 46.2 vs 44.1 us
  // without, voxel head 36.7 vs 36.2 -- this loop waits on the L2 -> LDS stream, not on the matrix pipe, so there is nothing to overlap.
#ifdef TRIBE_RING_STAGGER
  if (wave >= 4) {
    for (int t = 0; t < nk; ++t) {
      sync_and_restage(t);
      if (t > 0) mma();
      read_frags(t);
    }
    mma();
  } else
#endif
  {
    for (int t = 0; t < nk; ++t) {
      sync_and_restage(t);
      read_frags(t);
      mma();
    }
  }
  __builtin_amdgcn_s_barrier();   // the staging buffers become the epilogue's scratch: every wave is past its last fragment read

  if (splits > 1) {   // this workgroup's share of the reduction, raw: [split][M][N] f32, four consecutive columns of a row per lane
    float* wsp = ws + (int64_t)split * g.M * g.N;
    static_for<8>([&](auto t) {
      constexpr int i = decltype(t)::value / 4, j = decltype(t)::value % 4;
      float v[4];
      quad_transpose(acc[i][j], 1.0f, lane, v);
      const int64_t m = m0 + wr * 32 + i * 16 + ((lane >> 4) << 2) + (lane & 3), n = n0 + wc * 64 + j * 16 + (((lane & 15) >> 2) << 2);
      if (m < g.M && n < g.N) *(float4*)(wsp + m * g.N + n) = make_float4(v[0], v[1], v[2], v[3]);
    });
    return;
  }
  const EpiCtx ctx = make_epi_ctx(g, b1, b0, b1g);
  if (epilogue_fast_ok<(ROLE == TRIBE_ROLE_EXT)>(g, ctx) && n0 + BN <= g.N) {
    epilogue_fast<OUT_BF16, 2, 4, (ROLE == TRIBE_ROLE_EXT)>(g, ctx, acc, m0 + wr * 32, n0 + wc * 64, lane, smem + wave * 8192);
    return;
  }
  static_for<8>([&](auto t) {
    constexpr int i = decltype(t)::value / 4, j = decltype(t)::value % 4;
    epilogue_tile16<OUT_BF16, (ROLE == TRIBE_ROLE_EXT)>(g, ctx, acc[i][j], m0 + wr * 32 + i * 16, n0 + wc * 64 + j * 16, lane);
  });
}


// Second launch of a split-K GEMM: thread = four consecutive columns of one row; sums the shares in split order (deterministic) and applies
// the operators of the wait-free epilogue in its order: alpha, row_scale, row / column bias, GELU (the bf16 / f32 forms of the GEMM epilogues),
// scaled residual or periodic row add, store, bf16 copy, row sums of squares (slot n / 64: 16 consecutive lanes hold 64 columns of a row).
template <int OUT_BF16>
__global__ __launch_bounds__(256) void splitk_epilogue_kernel(const tribe_gemm_desc g, int splits, const float* __restrict__ ws) {
  const int64_t n4 = g.N >> 2, total = g.M * n4;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = idx < total;
  const int64_t id = live ? idx : total - 1;
  const int64_t m = id / n4, n = (id - m * n4) << 2;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int sp = 0; sp < splits; ++sp) {
    const float4 p = *(const float4*)(ws + ((int64_t)sp * g.M + m) * g.N + n);
    acc.x += p.x; acc.y += p.y; acc.z += p.z; acc.w += p.w;
  }
  float v[4] = {acc.x * g.alpha, acc.y * g.alpha, acc.z * g.alpha, acc.w * g.alpha};
  if (g.row_scale) {
    const float sc = g.row_scale[m];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] *= sc;
  }
  if (g.bias_mode == TRIBE_BIAS_ROW) {
    const float b = g.bias[m];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += b;
  } else if (g.bias_mode == TRIBE_BIAS_COL) {
    const float4 b = *(const float4*)(g.bias + n);
    v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
  }
  if (g.act == TRIBE_ACT_GELU) {
    if (OUT_BF16) {
      const f32x2_t lo = gelu_poly2(f32x2_t{v[0], v[1]}), hi = gelu_poly2(f32x2_t{v[2], v[3]});
      v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = gelu_erf(v[k]);
    }
  }
  if (g.res) {
    const float4 r = *(const float4*)(g.res + m * g.ldres + n);
    if (g.res_scale) {
      const float4 sc = *(const float4*)(g.res_scale + n);
      v[0] += r.x * sc.x; v[1] += r.y * sc.y; v[2] += r.z * sc.z; v[3] += r.w * sc.w;
    } else {
      v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
    }
  } else if (g.rowadd) {
    const float4 r = *(const float4*)(g.rowadd + (m % g.rowadd_period) * g.ld_rowadd + n);
    v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
  }
  u16x4_t o;
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = f32_to_bf16(v[k]);
  if (OUT_BF16) {
    if (live) *(u16x4_t*)((unsigned short*)g.C + m * g.ldc + n) = o;
  } else {
    if (live) *(float4*)((float*)g.C + m * g.ldc + n) = make_float4(v[0], v[1], v[2], v[3]);
    if (g.c_bf16 && live) *(u16x4_t*)(g.c_bf16 + m * g.ld_c_bf16 + n) = o;
    if (g.row_sumsq) {   // (the planner guarantees N % 64 == 0: a 16-lane group never straddles two rows)
      float t = live ? v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3] : 0.f;
      t += __shfl_xor(t, 1, 64); t += __shfl_xor(t, 2, 64); t += __shfl_xor(t, 4, 64); t += __shfl_xor(t, 8, 64);
      if (live && (threadIdx.x & 15) == 0) g.row_sumsq[m * g.ld_row_sumsq + (n >> 6)] = t;
    }
  }
}

}  // namespace

namespace tribe_gemm_detail {
#define TRIBE_GEMM_CASE_launch_ring(idx, bf, role) \
  case idx: launch_k<gemm_nt_ring128<bf, role>, 512, ring::SMEM_BYTES>(grid, s, d, tiles_m, tiles_n, splits, ws); break;
void launch_ring(int pair, dim3 grid, hipStream_t s, const tribe_gemm_desc* d, int tiles_m, int tiles_n, int splits, float* ws) {
  switch (pair) {
    TRIBE_GEMM_PAIRS(TRIBE_GEMM_CASE_launch_ring)
    default: break;
  }
}
void launch_splitk_epilogue(int bf, hipStream_t s, const tribe_gemm_desc* d, int splits, const float* ws) {
  const int64_t threads = d->M * (d->N / 4);
  const dim3 grid((unsigned)((threads + 255) / 256));
  if (bf) hipLaunchKernelGGL(splitk_epilogue_kernel<1>, grid, dim3(256), 0, s, *d, splits, ws);
  else hipLaunchKernelGGL(splitk_epilogue_kernel<0>, grid, dim3(256), 0, s, *d, splits, ws);
}
#define TRIBE_GEMM_CASE_launch_small(idx, bf, role) \
  case idx: launch_k<gemm_nt_128x128x64<bf, role>, 256, small::SMEM_BYTES>(grid, s, d, tiles_m, tiles_n); break;
TRIBE_GEMM_TABLE(launch_small)
}  // namespace tribe_gemm_detail
