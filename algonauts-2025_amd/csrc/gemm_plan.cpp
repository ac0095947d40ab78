// Host-side resolve step of the GEMM launchers (gemm_plan.h): descriptor checks and the measured rules that pick kernel, tile, symbol, grid
// and split.  No device code and no HIP call; the compute-unit count comes in as an argument.
#include "gemm_plan.h"

#ifndef TRIBE_GEMM_4W_DEFAULT
#define TRIBE_GEMM_4W_DEFAULT 0   // see plan_tiles: after the 8-wave kernel took over its epilogue techniques the two tie; tile_hint 5 selects it
#endif

#define REQUIRE(cond, fmt, ...)                        \
  do {                                                 \
    if (!(cond)) {                                     \
      tribe_set_error("%s: " fmt, who, ##__VA_ARGS__); \
      return -1;                                       \
    }                                                  \
  } while (0)

namespace tribe_gemm_detail {
namespace {
bool aligned(const void* p, unsigned bytes) { return ((uintptr_t)p % bytes) == 0; }
bool is_fused_norm(const tribe_gemm_desc* d) { return d->c_bf16 || d->row_sumsq || d->row_scale; }
bool is_gated(const tribe_gemm_desc* d) { return d->act == TRIBE_ACT_SWIGLU || d->act == TRIBE_ACT_GLU; }
// the residual stream as two 16-bit planes (enum tribe_c_planes): hi in c_bf16, lo in res (in) / C (out)
bool is_planes(const tribe_gemm_desc* d) { return d->c_dtype >= TRIBE_F32_PLANES_OUT && d->c_dtype <= TRIBE_F32_PLANES_IN; }

// true when the descriptor carries exactly the operator set a role-compiled epilogue holds, un-batched, no tile of width `bn` crossing N,
// and every operand as aligned as its vector accesses need.  [row_scale] of QKV / FF1 and [res_scale], [c_bf16], [row_sumsq] of
// out-proj / FF2 may be absent (first layer, last layer, unfused norm).  The two such epilogues differ in four requirements:
//   epilogue_role (8-wave NT kernel, make_epi_ctx's alignments): alpha == 1, a bf16 C 8-byte aligned, tiles `bn` wide
//   epilogue_w4 (one-wave-per-SIMD kernel): any alpha, C 16-byte aligned, 256-wide tiles, 32-bit per-lane offsets of the LDS-DMA pieces
bool role_operators_ok(const tribe_gemm_desc* d, int bn, bool alpha_must_be_1, unsigned bf16_c_align, bool lds_dma_offsets_32bit) {
  const bool res_role = d->role == TRIBE_ROLE_OUT_PROJ || d->role == TRIBE_ROLE_FF2;
  const bool bf_role = d->role == TRIBE_ROLE_QKV || d->role == TRIBE_ROLE_FF1;
  if (!res_role && !bf_role) return false;
  if (d->batch1 * d->batch0 != 1 || d->trans_ab || d->gather1 || d->N % bn != 0 || (alpha_must_be_1 && d->alpha != 1.0f) || d->rowadd || d->gadd || d->aux)
    return false;
  const bool planes = res_role && is_planes(d);
  if (!planes && d->c_dtype != (bf_role ? TRIBE_BF16 : TRIBE_F32)) return false;
  if (d->ldc % 4 != 0 || !aligned(d->C, bf_role ? bf16_c_align : 16)) return false;
  // planes: 8 columns per 16-byte request / paired store in each plane, and a hi plane to read or write
  if (planes && (d->ldc % 8 != 0 || d->ldres % 8 != 0 || !d->c_bf16 || d->ld_c_bf16 % 8 != 0 || !aligned(d->c_bf16, 16))) return false;
  // a lo row is 2 N 16-bit slots wide (the first half of every 64-column strip's f32 bytes: it can live in the f32 buffer itself)
  if (planes && ((d->c_dtype != TRIBE_F32_PLANES_IN && d->ldc < 2 * d->N) || (d->c_dtype != TRIBE_F32_PLANES_OUT && d->ldres < 2 * d->N))) return false;
  const bool wants_bias = d->role == TRIBE_ROLE_FF1 || d->role == TRIBE_ROLE_FF2;
  if (wants_bias ? (d->bias_mode != TRIBE_BIAS_COL || !d->bias || !aligned(d->bias, 16)) : d->bias_mode != TRIBE_BIAS_NONE) return false;
  if (d->act != (d->role == TRIBE_ROLE_FF1 ? TRIBE_ACT_GELU : TRIBE_ACT_NONE)) return false;
  if (res_role) {
    if (!d->res || d->ldres % 4 != 0 || !aligned(d->res, 16) || d->row_scale) return false;
    if (d->res_scale && !aligned(d->res_scale, 16)) return false;
    if (d->c_bf16 && (d->ld_c_bf16 % 4 != 0 || !aligned(d->c_bf16, 8))) return false;
  } else {
    if (d->res || d->res_scale || d->c_bf16 || d->row_sumsq) return false;
  }
  return !lds_dma_offsets_32bit || (int64_t)255 * (d->lda > d->ldb ? d->lda : d->ldb) * 2 + 8192 < (1ll << 32);
}
bool w4_role_ok(const tribe_gemm_desc* d) { return role_operators_ok(d, 256, false, 16, true); }
bool role8_ok(const tribe_gemm_desc* d, int bn) { return role_operators_ok(d, bn, true, 8, false); }

// split-K (desc.stream_k on an NT launch): operators the second launch knows, 16-byte accessible operands
bool split_k_operators_ok(const tribe_gemm_desc* d, int64_t nz) {
  return nz == 1 && !d->gather1 && !d->gadd && !d->aux && (d->act == TRIBE_ACT_NONE || d->act == TRIBE_ACT_GELU) && !(d->res && d->rowadd) &&
         d->N % 4 == 0 && (!d->row_sumsq || d->N % 64 == 0) && d->ldc % 4 == 0 && aligned(d->C, 16) &&
         (d->bias_mode != TRIBE_BIAS_COL || aligned(d->bias, 16)) && (!d->res || (d->ldres % 4 == 0 && aligned(d->res, 16))) &&
         (!d->res_scale || aligned(d->res_scale, 16)) && (!d->rowadd || (d->ld_rowadd % 4 == 0 && aligned(d->rowadd, 16))) &&
         (!d->c_bf16 || (d->ld_c_bf16 % 4 == 0 && aligned(d->c_bf16, 8)));
}
// stream-K (desc.stream_k on a trans_ab launch): the reduce kernel writes alpha * sum and nothing else
bool stream_k_operators_ok(const tribe_gemm_desc* d, int64_t nz) {
  return d->c_dtype != TRIBE_BF16 && nz == 1 && d->bias_mode == TRIBE_BIAS_NONE && d->act == TRIBE_ACT_NONE && !d->res && !d->rowadd && !d->gadd;
}

// Which kernel and tile a launch gets: kind, bm, bn, sumsq_cols, splits of *p.
void plan_tiles(const tribe_gemm_desc* d, int cu_count, GemmLaunch* p) {
  auto set = [&](int kind, int bm, int bn, int sumsq_cols) { p->kind = kind; p->bm = bm; p->bn = bn; p->sumsq_cols = sumsq_cols; p->splits = 1; };
  const int64_t nz = d->batch1 * d->batch0;
  auto tiles = [&](int64_t bm, int64_t bn) { return ((d->M + bm - 1) / bm) * ((d->N + bn - 1) / bn) * nz; };
  const int64_t t256 = tiles(256, 256), t128 = tiles(128, 128);
  const bool fused_norm = is_fused_norm(d);
  // 256^2 tiles when both extents fill them and the grid still covers the chip, else 128^2
  int use_big = (d->M >= 256 && d->N >= 256 && t256 >= 96);
  // Narrow, short-K products whose 256^2 grid is under two rounds of the 256 CUs (ViT-g attention projection: 8192 x 1408 x 1408 =
  // 192 tiles) run faster on 128^2 tiles (60 -> 47 us; profiles/r02_o_gemm_shapes.txt); with K > 2048 or N > 2048 the 256^2 tiles'
  // higher operand reuse wins back more than the idle CUs cost.
  if (use_big && t256 < 512 && t128 >= 512 && d->K <= 2048 && d->N <= 2048) use_big = 0;
  // 256-wide tiles that hang a quarter or more over the edge of a narrow C (dQ = dS K per head: N = 384 fills 1.5 of them) lose more MFMA
  // work than 128^2 tiles cost: batched 1024 x 384 x 1024, 128 batches: 246 -> 204 us
  if (use_big && t128 >= 512 && (double)t128 * 128 * 128 * 1.25 <= (double)t256 * 256 * 256) use_big = 0;
  if (fused_norm && d->N % 128 != 0) use_big = 1;   // (the launcher then reports the N it needs)
  if (d->tile_hint == 1 || d->tile_hint == 3) use_big = 0;
  if (d->tile_hint == 2 || d->tile_hint == 4 || d->tile_hint == 5 || d->tile_hint == 6) use_big = 1;
  if (d->trans_ab) return set(KIND_BIG, 256, 256, 64);
  if (!use_big) {
    // one workgroup per CU or fewer: the ring kernel (three K-tiles in flight); more: the double-buffered kernel, whose two or three
    // co-resident workgroups per CU cover for each other
    const bool ring = d->tile_hint == 3 || (d->tile_hint != 1 && t128 <= 256 && d->K >= 256);
    set(ring ? KIND_RING : KIND_SMALL, 128, 128, 64);
    // split-K (desc.stream_k): a grid of at most half a round whose tiles have K-steps to share out -- as many workgroups per tile as fit one
    // round, at least 8 K-steps each, at most 8 shares (so at most 128 tiles x 8: the grid and the second launch stay far inside 32 bits).
    // A round is counted on at most 256 CUs, as the stream-K planner counts it: the same plan as ever on the 256-CU target.
    if (ring && d->stream_k && split_k_operators_ok(d, nz)) {
      const int64_t nk = d->K / K_STEP;
      int64_t sp = (cu_count < 256 ? cu_count : 256) / t128;
      if (sp > nk / 8) sp = nk / 8;
      if (sp > 8) sp = 8;
      if (sp >= 2) p->splits = (int)sp;
    }
    return;
  }
  // Tile quantisation on 256 CUs: a grid of 256 x 192 tiles when that cuts the rounds' worth of work (BASELINE config at B = 4, M = 4096:
  // QKV 576 -> 768 tiles = 3 rounds of 3/4-size tiles instead of 3 of full size; out-proj / FF2 192 -> 256 tiles: the whole chip
  // instead of 3/4 of it).  A 192-wide tile costs ~0.78 of a 256-wide one; large grids keep 256^2 (higher operand reuse).
  int bn = 256;
  if (d->tile_hint == 4) bn = 192;
  else if (d->tile_hint == 6) bn = (d->N % 256 != 0 && d->N % 192 == 0) ? 192 : 256;   // the width whose tiles stay inside N (A/B against the role kernels)
  else if (d->tile_hint == 0 && d->N % 192 == 0 && t256 <= 2048) {
    const int64_t t192 = tiles(256, 192);
    const double cost4 = (double)((t256 + 255) / 256), cost3 = (double)((t192 + 255) / 256) * 0.78;
    if (cost3 < 0.95 * cost4) bn = 192;
  }
  if (fused_norm && d->N % bn != 0) bn = (d->N % 256 == 0) ? 256 : 192;
  // 256 x 256 tiles of the four encoder GEMMs: the one-wave-per-SIMD kernel, whose epilogue is compiled for exactly their operator sets
  // (tile_hint 2 keeps the 8-wave form for A/B runs; everything else -- other roles, batched, transposed operands -- stays 8-wave)
  // The one-wave-per-SIMD kernel (tile_hint 5; QKV / FF1 / out-proj / FF2 with their model epilogues).  History of the default: with the round-2
  // epilogue in the 8-wave kernel it won QKV / FF1 by 4.4 / 4.5 % (profiles/r03_z1_4w_lab.txt); its epilogue techniques (transposed accumulation,
  // paired 16-byte bf16 stores) then went into the 8-wave kernel (TACC), after which the two tie in isolation (profiles/r03_z2_4w_lab.txt) and in the
  // whole step (same box, bench.py: 8-wave only 639.7 - 640.4 k TRs/s, 4-wave for QKV / FF1 637.2 - 638.2 k: the step runs at the chip's power
  // limit, a kernel that draws less lets its neighbours clock higher and vice versa).  Default: 8-wave everywhere.
  const bool w4_default = TRIBE_GEMM_4W_DEFAULT && d->tile_hint == 0 && (d->role == TRIBE_ROLE_QKV || d->role == TRIBE_ROLE_FF1);
  if (bn == 256 && (d->tile_hint == 5 || w4_default) && w4_role_ok(d)) return set(KIND_BIG4W, 256, 256, 64);
  set(KIND_BIG, 256, bn, bn / 4);
}
// the 8-wave NT kernel with the role-compiled epilogue (tile_hint 6 = the same tiles with the generic epilogue, for A/B runs and tests).
// Default per role by the same-box measurements of DESIGN 4.1b (B = 64, parent -> role kernel): QKV 2.774 -> 2.737 ms, FF1 3.881 -> 3.704 ms,
// out-proj 1.212 -> 1.182 ms take it; FF2 (3.795 -> 3.782 ms, 3813 -> 3811 us in the kernel trace: inside the run-to-run spread -- its K = 12288
// loop is 4x as long and its epilogue waits on the residual, not on instructions) keeps the generic epilogue unless tile_hint 2 / 4 asks.
bool takes_role_epilogue(const tribe_gemm_desc* d, const GemmLaunch& p) {
  if (p.kind != KIND_BIG || d->trans_ab || d->tile_hint == 6 || !role8_ok(d, p.bn)) return false;
  if (is_planes(d)) return p.bn == 256;   // the plane epilogues exist in the 256 x 256 role kernels only, FF2's included
  return d->role != TRIBE_ROLE_FF2 || d->tile_hint == 2 || d->tile_hint == 4;
}
// The kernel symbol: the (dtype, role) combinations the encode path launches have kernels of their own.
int plan_pair(const tribe_gemm_desc* d, const GemmLaunch& p) {
  const int bf = d->c_dtype == TRIBE_BF16 ? 1 : 0;
  const int generic = bf ? PAIR_GENERIC_BF16 : PAIR_GENERIC_F32;
  if (d->trans_ab) return generic;   // transposed operands: the 256^2 kernel only, under the GENERIC symbol
  const bool ext = d->aux != nullptr || is_gated(d) || d->act == TRIBE_ACT_SILU || d->act == TRIBE_ACT_GELU_BWD || d->act == TRIBE_ACT_EXP2 ||
                   d->act == TRIBE_ACT_MUL_AUX;
  const int symbol_role = ext ? TRIBE_ROLE_EXT : ((d->role >= 0 && d->role < TRIBE_ROLE_COUNT) ? d->role : TRIBE_ROLE_GENERIC);
  int pair = generic, role_only = 0;
#define TRIBE_GEMM_MATCH(idx, is_bf, role) if (symbol_role == (role) && bf == (is_bf)) pair = idx;
#define TRIBE_GEMM_MATCH_ROLE(idx, is_bf, role) role_only |= symbol_role == (role) && bf == (is_bf);
  TRIBE_GEMM_PAIRS(TRIBE_GEMM_MATCH)
  TRIBE_GEMM_ROLE_PAIRS(TRIBE_GEMM_MATCH_ROLE)
#undef TRIBE_GEMM_MATCH
#undef TRIBE_GEMM_MATCH_ROLE
  // The 8-wave kernels of QKV / FF1 / out-proj / FF2 carry ONLY the epilogue of their role's operator set (epilogue_role): a launch of such a
  // role with any other descriptor -- or with tile_hint 6, the A/B switch -- runs the generic epilogue under the GENERIC symbol.
  return (p.kind == KIND_BIG && role_only && p.epilogue_path != 1) ? generic : pair;
}
}  // namespace

// Whole rounds of W tiles stay whole; the remainder is cut into W runs.  Not worth it (or not possible) -> the plain grid.
unsigned plan_stream_k(int tiles, int nk, int cu_count, SkSchedule* sk) {
  const int W = cu_count < 256 ? cu_count : 256;
  const int rem = tiles % W;
  *sk = no_stream_k();
  // Worth it only for remainders up to half a round.  Measured at B = 16 (profiles/r03_z12_gemm_streamk.txt, same numbers with atomics and
  // with the workspace): remainder 64 of 256 (dW of FF1 / FF2: 576 tiles; the projectors: 64 tiles) 1284 -> 1076 us / 1294 -> 1086 us /
  // 328 -> 161 us -- there a run is a clean quarter of a tile; remainder 176 (QKV) 848 -> 1007 us and 144 (out-proj) 334 -> 439 us: SLOWER --
  // every run straddles two tiles at its own K offset, so the 32 workgroups of an XCD stop sharing operand panels in its L2 (the 4 x 8 patch
  // of tile_coords) and the region turns memory-bound; and every part pays a prologue + epilogue (~45 us) for at most 1/2 tile of work.
  // Also: runs of at least 8 K-steps.
  if (rem == 0 || rem * 2 > W || (int64_t)rem * nk < (int64_t)W * 8) return (unsigned)tiles;
  sk->tiles_dp = tiles - rem;
  sk->rem_units = rem * nk;
  sk->q = (sk->rem_units + W - 1) / W;
  sk->workers = W;
  // second parts, longest first
  int len2[256], n2 = 0;
  unsigned short who[256];
  for (int w = 0; w < W; ++w) {
    const int u0 = w * sk->q;
    if (u0 >= sk->rem_units) break;
    const int run = sk->q < sk->rem_units - u0 ? sk->q : sk->rem_units - u0;
    const int x = u0 % nk, first = run < nk - x ? run : nk - x;
    if (first < run) { len2[n2] = run - first; who[n2] = (unsigned short)w; ++n2; }
  }
  for (int i = 1; i < n2; ++i) {   // insertion sort, descending, stable
    const int l = len2[i]; const unsigned short v = who[i];
    int j = i - 1;
    for (; j >= 0 && len2[j] < l; --j) { len2[j + 1] = len2[j]; who[j + 1] = who[j]; }
    len2[j + 1] = l; who[j + 1] = v;
  }
  for (int i = 0; i < n2; ++i) sk->second_worker[i] = who[i];
  return (unsigned)(sk->tiles_dp + W + n2);
}

GemmLaunch gemm_plan(const tribe_gemm_desc* d, int cu_count) {
  GemmLaunch launch{}, *p = &launch;
  plan_tiles(d, cu_count, p);
  p->epilogue_path = p->kind == KIND_BIG4W ? 2 : (takes_role_epilogue(d, *p) ? 1 : 0);
  p->pair = plan_pair(d, *p);
  p->tiles_m = (d->M + p->bm - 1) / p->bm;
  p->tiles_n = (d->N + p->bn - 1) / p->bn;
  p->nz = d->batch1 * d->batch0;
  const int64_t tiles = p->tiles_m * p->tiles_n;
  p->grid_x = (unsigned)(tiles * p->splits);
  p->sk = no_stream_k();
  p->ws_need = p->splits > 1 ? (int64_t)p->splits * d->M * d->N * 4 : 0;
  // a stream_k request the launch refuses for its operators (gemm_resolve) is not split: it needs no workspace
  if (d->trans_ab && d->stream_k && stream_k_operators_ok(d, p->nz) && tiles < (1ll << 31)) {
    p->grid_x = plan_stream_k((int)tiles, (int)(d->K / K_STEP), cu_count, &p->sk);
    if (p->sk.tiles_dp < tiles) {
      p->reduce_grid_x = (unsigned)(tiles - p->sk.tiles_dp);
      p->ws_need = (int64_t)2 * p->sk.workers * SK_SLOT_FLOATS * 4;
    }
  }
  return launch;
}

// The descriptor checks tribe_gemm_bf16 and tribe_gemm_fp8 share; they differ in the K-step and in the elements of a 16-byte row.
static int check_operands(const tribe_gemm_desc* d, const char* who, bool fp8) {
  const int k_step = fp8 ? K_STEP_FP8 : K_STEP, row16 = fp8 ? 16 : 8;
  REQUIRE(d != nullptr, "null descriptor");
  REQUIRE(d->M > 0 && d->N > 0 && d->K > 0, "M, N, K must be positive (got %lld %lld %lld)", (long long)d->M, (long long)d->N, (long long)d->K);
  REQUIRE(d->K % k_step == 0, "K=%lld must be a multiple of %d (zero-pad K)", (long long)d->K, k_step);
  REQUIRE(d->batch1 > 0 && d->batch0 > 0, "batch counts must be positive");
  REQUIRE(d->A && d->B && d->C, "null operand");
  REQUIRE(d->lda % row16 == 0 && d->ldb % row16 == 0 && d->sA1 % row16 == 0 && d->sA0 % row16 == 0 && d->sB1 % row16 == 0 && d->sB0 % row16 == 0,
          "lda/ldb/batch strides must be multiples of %d elements (16-byte rows)", row16);
  REQUIRE(aligned(d->A, 16) && aligned(d->B, 16), "A/B must be 16-byte aligned");
  REQUIRE(((!fp8 && d->trans_ab) || (d->lda >= d->K && d->ldb >= d->K)) && d->ldc >= (is_gated(d) ? d->N / 2 : d->N), "leading dimension too small");
  REQUIRE(!is_gated(d) || (d->N % 2 == 0 && !d->res && !d->rowadd && !d->gadd && d->bias_mode != TRIBE_BIAS_ROW),
          "%s an even N and no residual / row adds", fp8 ? "SWIGLU / GLU need" : "SWIGLU needs");
  REQUIRE(d->c_dtype == TRIBE_F32 || d->c_dtype == TRIBE_BF16 || (!fp8 && is_planes(d)), "c_dtype must be f32 or bf16");
  REQUIRE(d->bias_mode == TRIBE_BIAS_NONE || d->bias != nullptr, "bias_mode set without bias");
  REQUIRE(!d->rowadd || d->rowadd_period > 0, "rowadd needs a positive period");
  REQUIRE(!d->gadd || (d->gadd_index && d->gadd_div > 0), "gadd needs index and divisor");
  REQUIRE(!(d->gather_a || d->gather_bias || d->gather_b) || d->gather1, "gather flags set without gather1");
  return 0;
}

int gemm_resolve(const tribe_gemm_desc* d, const char* who, int cu_count, GemmLaunch* p) {
  if (check_operands(d, who, false) != 0) return -1;
  REQUIRE(d->act != TRIBE_ACT_GELU_BWD || d->aux, "GELU_BWD needs the saved pre-activation in aux");
  REQUIRE(d->act != TRIBE_ACT_MUL_AUX || (d->aux && d->ld_aux == d->ldc), "MUL_AUX needs aux laid out like C (ld_aux == ldc)");
  REQUIRE((d->act != TRIBE_ACT_EXP2 && d->act != TRIBE_ACT_MUL_AUX) || (!d->res && !d->rowadd && !d->gadd && d->bias_mode != TRIBE_BIAS_COL),
          "EXP2 / MUL_AUX take a row bias only");
  // (aux is addressed with C's batch offsets: the GELU pre-activation is un-batched, MUL_AUX's factor shares C's layout)
  REQUIRE(!d->aux || (d->ld_aux >= d->N && (d->batch1 * d->batch0 == 1 || d->act == TRIBE_ACT_MUL_AUX)),
          "aux is supported for un-batched GEMMs (and for MUL_AUX)");
  REQUIRE(d->sBias0 == 0 || d->bias_mode == TRIBE_BIAS_ROW, "sBias0 belongs to a row bias");
  const int64_t nz = d->batch1 * d->batch0;
  if (is_fused_norm(d)) {
    // fused ScaleNorm operands exist only in the wait-free epilogue: insist on everything that path needs
    REQUIRE(nz == 1 && !d->rowadd && !d->gadd && !d->aux && (d->act == TRIBE_ACT_NONE || d->act == TRIBE_ACT_GELU),
            "c_bf16 / row_sumsq / row_scale need an un-batched launch with plain operators");
    REQUIRE(d->ldc % 4 == 0 && aligned(d->C, 16) && (!d->bias || aligned(d->bias, 16)) && (!d->res || (d->ldres % 4 == 0 && aligned(d->res, 16))) &&
                (!d->res_scale || aligned(d->res_scale, 16)),
            "c_bf16 / row_sumsq / row_scale need 16-byte aligned operands");
    REQUIRE((!d->c_bf16 && !d->row_sumsq) || d->c_dtype == TRIBE_F32 || is_planes(d), "c_bf16 / row_sumsq accompany an f32 C");
    REQUIRE(!d->c_bf16 || (d->ld_c_bf16 >= d->N && d->ld_c_bf16 % 4 == 0 && aligned(d->c_bf16, 8)), "bad c_bf16");
  }
  *p = gemm_plan(d, cu_count);
  // (split-K plans are KIND_RING, transposed operands never take the role epilogue)
  REQUIRE(!is_planes(d) || (p->kind == KIND_BIG && p->bn == 256 && p->epilogue_path == 1),
          "the plane c_dtype values (16-bit hi / lo residual stream) run on the out-proj / FF2 role kernels at 256 x 256 tiles only");
  if (is_fused_norm(d)) {
    REQUIRE(d->N % p->bn == 0, "c_bf16 / row_sumsq / row_scale need N (%lld) to be a multiple of the tile width %d", (long long)d->N, p->bn);
    REQUIRE(!d->row_sumsq || d->ld_row_sumsq >= d->N / p->sumsq_cols, "ld_row_sumsq must cover N / %d slots (tribe_gemm_sumsq_slots)", p->sumsq_cols);
  }
  if (d->trans_ab) {
    REQUIRE(d->M >= 8 && d->N >= 8 && d->M % 8 == 0 && d->N % 8 == 0 && d->lda >= d->M && d->ldb >= d->N,
            "trans_ab takes At [K, M] and Bt [K, N] with M and N multiples of 8 and lda >= M, ldb >= N");
    REQUIRE(!d->aux && !is_gated(d) && d->act != TRIBE_ACT_SILU && d->act != TRIBE_ACT_GELU_BWD && d->act != TRIBE_ACT_EXP2 &&
                d->act != TRIBE_ACT_MUL_AUX && !d->gather_a && !d->gather_b,
            "trans_ab supports the plain epilogue operators and no operand gather");
  }
  REQUIRE(p->tiles_m * p->tiles_n < (1ll << 31) && nz < 65536, "grid too large");
  REQUIRE(!d->trans_ab || !d->stream_k || stream_k_operators_ok(d, nz), "stream_k takes a plain un-batched f32 product");
  return 0;
}

int gemm_check_workspace(const tribe_gemm_desc* d, const char* who, const GemmLaunch& p) {
  if (p.ws_need == 0) return 0;
  const bool ok = d->stream_k_ws && d->stream_k_ws_bytes >= p.ws_need && aligned(d->stream_k_ws, 16);
  if (d->trans_ab) REQUIRE(ok, "stream_k needs a 16-byte aligned workspace of %lld bytes (tribe_gemm_stream_k_workspace_bytes)", (long long)p.ws_need);
  REQUIRE(ok, "this launch is split over K: stream_k_ws must hold %lld bytes (tribe_gemm_stream_k_workspace_bytes)", (long long)p.ws_need);
  return 0;
}

int gemm_fp8_resolve(const tribe_gemm_desc* d, const char* who, GemmLaunch* p) {
  if (check_operands(d, who, true) != 0) return -1;
  REQUIRE(d->act != TRIBE_ACT_GELU_BWD && !d->aux, "the training-only epilogues (aux, GELU_BWD) are bf16-only");
  *p = GemmLaunch{};
  p->kind = KIND_BIG; p->bm = 256; p->bn = 256; p->sumsq_cols = 64; p->splits = 1;   // one kernel: 256 x 256 x 128
  const bool bf = d->c_dtype == TRIBE_BF16, ext = is_gated(d) || d->act == TRIBE_ACT_SILU;
  p->pair = ext ? (bf ? PAIR_EXT_BF16 : PAIR_EXT_F32) : (bf ? PAIR_GENERIC_BF16 : PAIR_GENERIC_F32);
  p->tiles_m = (d->M + 255) / 256; p->tiles_n = (d->N + 255) / 256; p->nz = d->batch1 * d->batch0;
  REQUIRE(p->tiles_m * p->tiles_n < (1ll << 31) && p->nz < 65536, "grid too large");
  p->grid_x = (unsigned)(p->tiles_m * p->tiles_n);
  p->sk = no_stream_k();
  return 0;
}
}  // namespace tribe_gemm_detail
