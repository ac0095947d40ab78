r"""Records tests/golden/gemm_plan.npz: what tribe_gemm_bf16 / tribe_gemm_fp8 decide for a few thousand descriptors -- return code, error
text, kernel kind, tile, kernel symbol, epilogue path, grid, split-K / stream-K schedule and workspace need -- read through the debug
export tribe_debug_gemm_plan (host only, made-up addresses, nothing is launched).

DO NOT REGENERATE FROM THE CODE UNDER TEST.  The fixture was recorded from the commit BEFORE the launchers were rebuilt around one resolve
step (csrc/gemm_plan.cpp), so that tests/test_gemm_plan_golden.py proves the rebuilt dispatch decides what the old one decided.  That
commit had no such export; it was recorded from a scratch copy with the patch below applied to csrc/gemm.hip (the body of the two entry
points duplicated, every launch replaced by writes to `out`), built with the Makefile, and selected with TRIBE_HIP_LIB:

    TRIBE_HIP_LIB=/path/to/patched/libtribe_hip.so python tests/golden/make_golden_gemm_plan.py

The one answer that changed on purpose is not in the table: tribe_gemm_stream_k_workspace_bytes (a query, not the launch) now says 0
for a stream_k request whose operators the launch refuses.  Recorded without a GPU: both planners then count 256 compute units, the
MI355X's number.

--- a/algonauts-2025_amd/csrc/gemm.hip
+++ b/algonauts-2025_amd/csrc/gemm.hip
@@ -1696,4 +1696,164 @@
   if (plan.kind == tribe_gemm_detail::KIND_BIG4W) return 2;
   return tribe_gemm_detail::takes_role_epilogue(d, plan) ? 1 : 0;
 }
+// ---- recording only: the body of tribe_gemm_bf16 / tribe_gemm_fp8 with every launch replaced by writes to out ----
+namespace {
+enum { DP_RC, DP_KIND, DP_BM, DP_BN, DP_SUMSQ_COLS, DP_SPLITS, DP_PAIR, DP_PATH, DP_TILES_M, DP_TILES_N, DP_NZ, DP_GRID_X, DP_REDUCE_GRID_X,
+       DP_SK_TILES_DP, DP_SK_REM_UNITS, DP_SK_Q, DP_SK_WORKERS, DP_SK_SECOND, DP_WS_NEED, DP_COUNT };
+int debug_plan_fp8(const tribe_gemm_desc* d, int64_t* out) {
+  TRIBE_REQUIRE(d != nullptr, "tribe_gemm_fp8: null descriptor");
+  TRIBE_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0, "tribe_gemm_fp8: M, N, K must be positive (got %lld %lld %lld)", (long long)d->M,
+                (long long)d->N, (long long)d->K);
+  TRIBE_REQUIRE(d->K % 128 == 0, "tribe_gemm_fp8: K=%lld must be a multiple of 128 (zero-pad K)", (long long)d->K);
+  TRIBE_REQUIRE(d->batch1 > 0 && d->batch0 > 0, "tribe_gemm_fp8: batch counts must be positive");
+  TRIBE_REQUIRE(d->A && d->B && d->C, "tribe_gemm_fp8: null operand");
+  TRIBE_REQUIRE(d->lda % 16 == 0 && d->ldb % 16 == 0 && d->sA1 % 16 == 0 && d->sA0 % 16 == 0 && d->sB1 % 16 == 0 && d->sB0 % 16 == 0,
+                "tribe_gemm_fp8: lda/ldb/batch strides must be multiples of 16 elements (16-byte rows)");
+  TRIBE_REQUIRE(((uintptr_t)d->A % 16) == 0 && ((uintptr_t)d->B % 16) == 0, "tribe_gemm_fp8: A/B must be 16-byte aligned");
+  TRIBE_REQUIRE(d->lda >= d->K && d->ldb >= d->K && d->ldc >= ((d->act == TRIBE_ACT_SWIGLU || d->act == TRIBE_ACT_GLU) ? d->N / 2 : d->N),
+                "tribe_gemm_fp8: leading dimension too small");
+  TRIBE_REQUIRE((d->act != TRIBE_ACT_SWIGLU && d->act != TRIBE_ACT_GLU) || (d->N % 2 == 0 && !d->res && !d->rowadd && !d->gadd && d->bias_mode != TRIBE_BIAS_ROW),
+                "tribe_gemm_fp8: SWIGLU / GLU need an even N and no residual / row adds");
+  TRIBE_REQUIRE(d->c_dtype == TRIBE_F32 || d->c_dtype == TRIBE_BF16, "tribe_gemm_fp8: c_dtype must be f32 or bf16");
+  TRIBE_REQUIRE(d->bias_mode == TRIBE_BIAS_NONE || d->bias != nullptr, "tribe_gemm_fp8: bias_mode set without bias");
+  TRIBE_REQUIRE(!d->rowadd || d->rowadd_period > 0, "tribe_gemm_fp8: rowadd needs a positive period");
+  TRIBE_REQUIRE(!d->gadd || (d->gadd_index && d->gadd_div > 0), "tribe_gemm_fp8: gadd needs index and divisor");
+  TRIBE_REQUIRE(!(d->gather_a || d->gather_bias || d->gather_b) || d->gather1, "tribe_gemm_fp8: gather flags set without gather1");
+  TRIBE_REQUIRE(d->act != TRIBE_ACT_GELU_BWD && !d->aux, "tribe_gemm_fp8: the training-only epilogues (aux, GELU_BWD) are bf16-only");
+  const int64_t nz = d->batch1 * d->batch0;
+  const int64_t tiles_m = (d->M + big::BM - 1) / big::BM, tiles_n = (d->N + big::BN - 1) / big::BN;
+  TRIBE_REQUIRE(tiles_m * tiles_n < (1ll << 31) && nz < 65536, "tribe_gemm_fp8: grid too large");
+  const bool bf = d->c_dtype == TRIBE_BF16;
+  const bool ext = d->act == TRIBE_ACT_SWIGLU || d->act == TRIBE_ACT_GLU || d->act == TRIBE_ACT_SILU;
+  out[DP_KIND] = tribe_gemm_detail::KIND_BIG; out[DP_BM] = 256; out[DP_BN] = 256; out[DP_SUMSQ_COLS] = 64; out[DP_SPLITS] = 1;
+  out[DP_PAIR] = ext ? (bf ? 2 : 3) : (bf ? 0 : 1);   // TRIBE_FP8_LAUNCH(bf, ext)
+  out[DP_TILES_M] = tiles_m; out[DP_TILES_N] = tiles_n; out[DP_NZ] = nz; out[DP_GRID_X] = (unsigned)(tiles_m * tiles_n);
+  out[DP_SK_TILES_DP] = tribe_gemm_detail::no_stream_k().tiles_dp;
+  return 0;
+}
+int debug_plan_bf16(const tribe_gemm_desc* d, int64_t* out) {
+  TRIBE_REQUIRE(d != nullptr, "tribe_gemm_bf16: null descriptor");
+  TRIBE_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0, "tribe_gemm_bf16: M, N, K must be positive (got %lld %lld %lld)",
+                (long long)d->M, (long long)d->N, (long long)d->K);
+  TRIBE_REQUIRE(d->K % BK == 0, "tribe_gemm_bf16: K=%lld must be a multiple of %d (zero-pad K)", (long long)d->K, BK);
+  TRIBE_REQUIRE(d->batch1 > 0 && d->batch0 > 0, "tribe_gemm_bf16: batch counts must be positive");
+  TRIBE_REQUIRE(d->A && d->B && d->C, "tribe_gemm_bf16: null operand");
+  TRIBE_REQUIRE(d->lda % 8 == 0 && d->ldb % 8 == 0 && d->sA1 % 8 == 0 && d->sA0 % 8 == 0 && d->sB1 % 8 == 0 &&
+                    d->sB0 % 8 == 0,
+                "tribe_gemm_bf16: lda/ldb/batch strides must be multiples of 8 elements (16-byte rows)");
+  TRIBE_REQUIRE(((uintptr_t)d->A % 16) == 0 && ((uintptr_t)d->B % 16) == 0, "tribe_gemm_bf16: A/B must be 16-byte aligned");
+  TRIBE_REQUIRE((d->trans_ab || (d->lda >= d->K && d->ldb >= d->K)) && d->ldc >= ((d->act == TRIBE_ACT_SWIGLU || d->act == TRIBE_ACT_GLU) ? d->N / 2 : d->N),
+                "tribe_gemm_bf16: leading dimension too small");
+  TRIBE_REQUIRE((d->act != TRIBE_ACT_SWIGLU && d->act != TRIBE_ACT_GLU) || (d->N % 2 == 0 && !d->res && !d->rowadd && !d->gadd && d->bias_mode != TRIBE_BIAS_ROW),
+                "tribe_gemm_bf16: SWIGLU needs an even N and no residual / row adds");
+  TRIBE_REQUIRE(d->c_dtype == TRIBE_F32 || d->c_dtype == TRIBE_BF16, "tribe_gemm_bf16: c_dtype must be f32 or bf16");
+  TRIBE_REQUIRE(d->bias_mode == TRIBE_BIAS_NONE || d->bias != nullptr, "tribe_gemm_bf16: bias_mode set without bias");
+  TRIBE_REQUIRE(!d->rowadd || d->rowadd_period > 0, "tribe_gemm_bf16: rowadd needs a positive period");
+  TRIBE_REQUIRE(!d->gadd || (d->gadd_index && d->gadd_div > 0), "tribe_gemm_bf16: gadd needs index and divisor");
+  TRIBE_REQUIRE(!(d->gather_a || d->gather_bias || d->gather_b) || d->gather1, "tribe_gemm_bf16: gather flags set without gather1");
+  TRIBE_REQUIRE(d->act != TRIBE_ACT_GELU_BWD || d->aux, "tribe_gemm_bf16: GELU_BWD needs the saved pre-activation in aux");
+  TRIBE_REQUIRE(d->act != TRIBE_ACT_MUL_AUX || (d->aux && d->ld_aux == d->ldc), "tribe_gemm_bf16: MUL_AUX needs aux laid out like C (ld_aux == ldc)");
+  TRIBE_REQUIRE((d->act != TRIBE_ACT_EXP2 && d->act != TRIBE_ACT_MUL_AUX) || (!d->res && !d->rowadd && !d->gadd && d->bias_mode != TRIBE_BIAS_COL),
+                "tribe_gemm_bf16: EXP2 / MUL_AUX take a row bias only");
+  TRIBE_REQUIRE(!d->aux || (d->ld_aux >= d->N && (d->batch1 * d->batch0 == 1 || d->act == TRIBE_ACT_MUL_AUX)),
+                "tribe_gemm_bf16: aux is supported for un-batched GEMMs (and for MUL_AUX)");
+  TRIBE_REQUIRE(d->sBias0 == 0 || d->bias_mode == TRIBE_BIAS_ROW, "tribe_gemm_bf16: sBias0 belongs to a row bias");
+  const int64_t nz = d->batch1 * d->batch0;
+  if (d->c_bf16 || d->row_sumsq || d->row_scale) {
+    TRIBE_REQUIRE(nz == 1 && !d->rowadd && !d->gadd && !d->aux && (d->act == TRIBE_ACT_NONE || d->act == TRIBE_ACT_GELU),
+                  "tribe_gemm_bf16: c_bf16 / row_sumsq / row_scale need an un-batched launch with plain operators");
+    TRIBE_REQUIRE(d->ldc % 4 == 0 && ((uintptr_t)d->C % 16) == 0 && (!d->bias || ((uintptr_t)d->bias % 16) == 0) &&
+                      (!d->res || (d->ldres % 4 == 0 && ((uintptr_t)d->res % 16) == 0)) && (!d->res_scale || ((uintptr_t)d->res_scale % 16) == 0),
+                  "tribe_gemm_bf16: c_bf16 / row_sumsq / row_scale need 16-byte aligned operands");
+    TRIBE_REQUIRE((!d->c_bf16 && !d->row_sumsq) || d->c_dtype == TRIBE_F32, "tribe_gemm_bf16: c_bf16 / row_sumsq accompany an f32 C");
+    TRIBE_REQUIRE(!d->c_bf16 || (d->ld_c_bf16 >= d->N && d->ld_c_bf16 % 4 == 0 && ((uintptr_t)d->c_bf16 % 8) == 0), "tribe_gemm_bf16: bad c_bf16");
+  }
+  const tribe_gemm_detail::GemmPlan plan = tribe_gemm_detail::gemm_plan(d);
+  if (d->c_bf16 || d->row_sumsq || d->row_scale) {
+    TRIBE_REQUIRE(d->N % plan.bn == 0, "tribe_gemm_bf16: c_bf16 / row_sumsq / row_scale need N (%lld) to be a multiple of the tile width %d",
+                  (long long)d->N, plan.bn);
+    TRIBE_REQUIRE(!d->row_sumsq || d->ld_row_sumsq >= d->N / plan.sumsq_cols, "tribe_gemm_bf16: ld_row_sumsq must cover N / %d slots (tribe_gemm_sumsq_slots)",
+                  plan.sumsq_cols);
+  }
+  if (d->trans_ab) {
+    TRIBE_REQUIRE(d->M >= 8 && d->N >= 8 && d->M % 8 == 0 && d->N % 8 == 0 && d->lda >= d->M && d->ldb >= d->N,
+                  "tribe_gemm_bf16: trans_ab takes At [K, M] and Bt [K, N] with M and N multiples of 8 and lda >= M, ldb >= N");
+    TRIBE_REQUIRE(!d->aux && d->act != TRIBE_ACT_SWIGLU && d->act != TRIBE_ACT_GLU && d->act != TRIBE_ACT_SILU && d->act != TRIBE_ACT_GELU_BWD &&
+                      d->act != TRIBE_ACT_EXP2 && d->act != TRIBE_ACT_MUL_AUX && !d->gather_a && !d->gather_b,
+                  "tribe_gemm_bf16: trans_ab supports the plain epilogue operators and no operand gather");
+  }
+  const int64_t tiles_m = (d->M + plan.bm - 1) / plan.bm, tiles_n = (d->N + plan.bn - 1) / plan.bn;
+  TRIBE_REQUIRE(tiles_m * tiles_n < (1ll << 31) && nz < 65536, "tribe_gemm_bf16: grid too large");
+
+  dim3 grid((unsigned)(tiles_m * tiles_n), (unsigned)nz, 1);
+  const int role = (d->role >= 0 && d->role < TRIBE_ROLE_COUNT) ? d->role : TRIBE_ROLE_GENERIC;
+  const bool bf = d->c_dtype == TRIBE_BF16;
+  out[DP_KIND] = plan.kind; out[DP_BM] = plan.bm; out[DP_BN] = plan.bn; out[DP_SUMSQ_COLS] = plan.sumsq_cols; out[DP_SPLITS] = plan.splits;
+  out[DP_TILES_M] = tiles_m; out[DP_TILES_N] = tiles_n; out[DP_NZ] = nz;
+  out[DP_PATH] = plan.kind == tribe_gemm_detail::KIND_BIG4W ? 2 : (tribe_gemm_detail::takes_role_epilogue(d, plan) ? 1 : 0);   // tribe_gemm_epilogue_path
+  if (d->trans_ab) {   // transposed operands: the 256^2 kernel only, plain epilogue operators
+    SkSched sk = tribe_gemm_detail::no_stream_k();
+    int64_t need = 0;
+    if (d->stream_k) {
+      TRIBE_REQUIRE(!bf && nz == 1 && d->bias_mode == TRIBE_BIAS_NONE && d->act == TRIBE_ACT_NONE && !d->res && !d->rowadd && !d->gadd,
+                    "tribe_gemm_bf16: stream_k takes a plain un-batched f32 product");
+      grid.x = tribe_gemm_detail::plan_stream_k((int)(tiles_m * tiles_n), (int)(d->K / BK), &sk);
+      if (sk.tiles_dp < tiles_m * tiles_n) {
+        need = (int64_t)2 * sk.workers * SK_SLOT_FLOATS * 4;
+        TRIBE_REQUIRE(d->stream_k_ws && d->stream_k_ws_bytes >= need && ((uintptr_t)d->stream_k_ws % 16) == 0,
+                      "tribe_gemm_bf16: stream_k needs a 16-byte aligned workspace of %lld bytes (tribe_gemm_stream_k_workspace_bytes)", (long long)need);
+        sk.ws = (float*)d->stream_k_ws;
+      }
+    }
+    const bool split = sk.tiles_dp < tiles_m * tiles_n;
+    out[DP_PAIR] = bf ? 0 : 1;   // launch_big4_tn: the GENERIC symbol of the dtype
+    out[DP_GRID_X] = grid.x;
+    out[DP_REDUCE_GRID_X] = split ? (unsigned)(tiles_m * tiles_n - sk.tiles_dp) : 0;   // streamk_reduce_kernel
+    out[DP_SK_TILES_DP] = sk.tiles_dp; out[DP_SK_REM_UNITS] = sk.rem_units; out[DP_SK_Q] = sk.q; out[DP_SK_WORKERS] = sk.workers;
+    out[DP_SK_SECOND] = split ? (int64_t)grid.x - sk.tiles_dp - sk.workers : 0;
+    out[DP_WS_NEED] = need;
+    return 0;
+  }
+  const bool ext = d->aux != nullptr || d->act == TRIBE_ACT_SWIGLU || d->act == TRIBE_ACT_GLU || d->act == TRIBE_ACT_SILU ||
+                   d->act == TRIBE_ACT_GELU_BWD || d->act == TRIBE_ACT_EXP2 || d->act == TRIBE_ACT_MUL_AUX;
+  int pair = bf ? 0 : 1;   // GENERIC
+  if (ext) {
+    pair = bf ? 2 : 3;
+  } else {
+    switch (role) {     // the (dtype, role) combinations the encode path launches have kernels of their own
+    case TRIBE_ROLE_PROJECTOR: if (!bf) pair = 4; break;
+    case TRIBE_ROLE_QKV: if (bf) pair = 5; break;
+    case TRIBE_ROLE_ATTN_SCORES: if (!bf) pair = 6; break;
+    case TRIBE_ROLE_ATTN_PV: if (bf) pair = 7; break;
+    case TRIBE_ROLE_OUT_PROJ: if (!bf) pair = 8; break;
+    case TRIBE_ROLE_FF1: if (bf) pair = 9; break;
+    case TRIBE_ROLE_FF2: if (!bf) pair = 10; break;
+    case TRIBE_ROLE_VOXEL_HEAD: if (!bf) pair = 11; break;
+    default: break;
+    }
+  }
+  using namespace tribe_gemm_detail;
+  if (plan.kind == KIND_BIG && (pair == 5 || pair == 8 || pair == 9 || pair == 10) && !takes_role_epilogue(d, plan)) pair = bf ? 0 : 1;
+  out[DP_PAIR] = pair;
+  out[DP_SK_TILES_DP] = no_stream_k().tiles_dp;
+  if (plan.kind == KIND_RING && plan.splits > 1) {
+    const int64_t need = (int64_t)plan.splits * d->M * d->N * 4;
+    TRIBE_REQUIRE(d->stream_k_ws && d->stream_k_ws_bytes >= need && ((uintptr_t)d->stream_k_ws % 16) == 0,
+                  "tribe_gemm_bf16: this launch is split over K: stream_k_ws must hold %lld bytes (tribe_gemm_stream_k_workspace_bytes)", (long long)need);
+    TRIBE_REQUIRE(tiles_m * tiles_n * plan.splits < (1ll << 31) && d->M * (d->N / 4) < (1ll << 39), "tribe_gemm_bf16: grid too large");
+    grid.x = (unsigned)(tiles_m * tiles_n * plan.splits);
+    out[DP_WS_NEED] = need;
+  }
+  out[DP_GRID_X] = grid.x;
+  return 0;
+}
+}  // namespace
+extern "C" int tribe_debug_gemm_plan(const tribe_gemm_desc* d, int32_t fp8, int64_t* out, int32_t n) {
+  TRIBE_REQUIRE(out != nullptr && n >= DP_COUNT, "tribe_debug_gemm_plan: out must hold %d entries", (int)DP_COUNT);
+  for (int i = 0; i < DP_COUNT; ++i) out[i] = 0;
+  const int rc = fp8 ? debug_plan_fp8(d, out) : debug_plan_bf16(d, out);
+  if (rc != 0) for (int i = 0; i < DP_COUNT; ++i) out[i] = 0;
+  out[DP_RC] = rc;
+  return rc;
+}
 #endif  // part 0
"""

import ctypes as C
import random
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "algonauts-2025_amd"))
OUT = Path(__file__).resolve().parent / "gemm_plan.npz"

OUT_FIELDS = ["rc", "kind", "bm", "bn", "sumsq_cols", "splits", "pair", "epilogue_path", "tiles_m", "tiles_n", "nz", "grid_x", "reduce_grid_x",
              "sk_tiles_dp", "sk_rem_units", "sk_q", "sk_workers", "sk_second_parts", "ws_need"]
P = 0x7F0000000000   # a 16-byte aligned "device address"; operand i lives at P + (i << 32)
F32, BF16 = 0, 1
NONE, GELU, SWIGLU, SILU, GLU, GELU_BWD, EXP2, MUL_AUX = range(8)
BIAS_NONE, BIAS_COL, BIAS_ROW = 0, 1, 2
ROLE = {n: i for i, n in enumerate(["generic", "projector", "qkv", "attn_scores", "attn_pv", "out_proj", "ff1", "ff2", "voxel_head", "attention"])}
KIND_SMALL, KIND_BIG, KIND_RING, KIND_BIG4W = range(4)


def addr(i, off=0):
    return P + (i << 32) + off


def nt(M, N, K, c_dtype=F32, **kw):
    """A valid plain NT descriptor; keywords override or add fields."""
    d = dict(M=M, N=N, K=K, batch1=1, batch0=1, A=addr(1), lda=K, B=addr(2), ldb=K, C=addr(3), ldc=N, c_dtype=c_dtype, alpha=1.0)
    d.update(kw)
    return d


def tn(M, N, K, **kw):
    """The weight-gradient form: At [K, M], Bt [K, N]."""
    return nt(M, N, K, **dict(dict(lda=M, ldb=N, trans_ab=1), **kw))


def workspace(kind):
    return {"none": {}, "ok": dict(stream_k_ws=addr(12), stream_k_ws_bytes=1 << 40), "small": dict(stream_k_ws=addr(12), stream_k_ws_bytes=4096),
            "odd": dict(stream_k_ws=addr(12, 8), stream_k_ws_bytes=1 << 40)}[kind]


def model_ops(role, M, N, K, **kw):
    """The operator set the encoder gives each of its four GEMMs."""
    if role in ("qkv", "ff1"):
        d = nt(M, N, K, BF16, role=ROLE[role], row_scale=addr(4))
    else:
        d = nt(M, N, K, F32, role=ROLE[role], res=addr(3), ldres=N, res_scale=addr(5), c_bf16=addr(6), ld_c_bf16=N, row_sumsq=addr(7),
               ld_row_sumsq=N // 48)
    if role in ("ff1", "ff2"):
        d.update(bias=addr(8), bias_mode=BIAS_COL)
    if role == "ff1":
        d["act"] = GELU
    d.update(kw)
    return d


def model_cases():
    cases = []
    D, FF, H3 = 3072, 12288, 9216
    for M in (128, 4096, 16384):
        for hint in range(7):
            for sk in (0, 1):
                ws = workspace("ok") if sk else {}
                cases += [model_ops("qkv", M, H3, D, tile_hint=hint, stream_k=sk, **ws), model_ops("out_proj", M, D, D, tile_hint=hint, stream_k=sk, **ws),
                          model_ops("ff1", M, FF, D, tile_hint=hint, stream_k=sk, **ws), model_ops("ff2", M, D, FF, tile_hint=hint, stream_k=sk, **ws)]
        # first-layer QKV (no row_scale), last-layer FF2 (no fused norm), projectors with pos_embed, the batched voxel head with its subject gather
        cases += [model_ops("qkv", M, H3, D, row_scale=0), model_ops("ff2", M, D, FF, c_bf16=0, row_sumsq=0, res_scale=0)]
        for Kp in (2048, 1024, 1408):
            cases.append(nt(M, 1024, Kp, F32, role=ROLE["projector"], bias=addr(8), bias_mode=BIAS_COL, rowadd=addr(9), ld_rowadd=1024, rowadd_period=128, stream_k=1,
                            **workspace("ok")))
        cases.append(nt(1024, 100, 2048, F32, role=ROLE["voxel_head"], batch1=M // 128, sA1=100 * 2048, sB1=1024 * 2048, sC1=1024 * 100, gather1=addr(10),
                        gather_a=1, bias=addr(8), bias_mode=BIAS_COL, sBias1=1024, gather_bias=1, ldc=100))
    # the training backward (modeling_utils/autograd.py)
    for tokens in (4096, 16384):
        for n_out, k_in in ((D, D), (H3, D), (FF, D), (D, FF), (1024, 2048), (1024, 1408)):
            for sk, ws in ((0, "none"), (1, "ok"), (1, "none"), (1, "small"), (1, "odd")):
                cases.append(tn(n_out, k_in, tokens, ldc=k_in, stream_k=sk, **workspace(ws)))             # wgrad
            cases.append(nt(tokens, k_in, n_out, F32))                                                  # dgrad
            cases.append(nt(tokens, k_in, n_out, BF16))
        cases.append(nt(tokens, FF, D, BF16, role=ROLE["ff1"], bias=addr(8), bias_mode=BIAS_COL, act=GELU, aux=addr(11), ld_aux=FF))   # training forward
        cases.append(nt(tokens, FF, D, BF16, act=GELU_BWD, aux=addr(11), ld_aux=FF))                      # dh * gelu'(pre)
    T, d, h, nb, ld, inner = 1024, 384, 8, 4, 3 * 3072, 3072
    batch = dict(batch1=nb, batch0=h, sA1=T * ld, sA0=d, sB1=T * ld, sB0=d, sC1=h * T * T, sC0=T * T)
    cases.append(nt(T, T, d, BF16, lda=ld, ldb=ld, ldc=T, alpha=0.0736, act=EXP2, bias=addr(8), bias_mode=BIAS_ROW, sBias1=h * T, sBias0=T, **batch))
    cases.append(nt(T, T, d, BF16, lda=inner, ldb=ld, ldc=T, alpha=0.051, act=MUL_AUX, aux=addr(11), ld_aux=T, bias=addr(8), bias_mode=BIAS_ROW,
                    sBias1=h * T, sBias0=T, **dict(batch, sA1=T * inner)))
    cases.append(nt(T, T, d, F32, lda=ld, ldb=ld, ldc=T, alpha=0.051, role=ROLE["attn_scores"], **batch))
    cases.append(nt(T, d, T, BF16, lda=T, ldb=T, ldc=ld, role=ROLE["attn_pv"], batch1=nb, batch0=h, sA1=h * T * T, sA0=T * T, sB1=h * d * T, sB0=d * T,
                    sC1=T * ld, sC0=d))                                                                  # dQ = dS K
    cases.append(tn(T, d, T, c_dtype=BF16, lda=T, ldb=inner, ldc=ld, batch1=nb, batch0=h, sA1=h * T * T, sA0=T * T, sB1=T * inner, sB0=d, sC1=T * ld, sC0=d))   # dV = P^T dO
    cases.append(nt(100, 2048, 1024, F32, batch1=8, sA1=100 * 1024, sB1=2048 * 1024, sC1=100 * 2048, gather1=addr(10), gather_b=1))   # voxel head dgrad
    cases.append(nt(2048, 1000, 128, F32, batch1=8, sA1=2048 * 128, sB1=1000 * 128, sC1=2048 * 1000))     # voxel head wgrad slabs
    # the stream-K schedules of tests/test_abi_and_host.py as launches: 576 and 64 tiles split, 144 and 432 (remainder above half a round) declined
    for M, N in ((12288, 3072), (2048, 2048), (3072, 3072), (9216, 3072), (512, 512), (4352, 4096)):
        for K in (16384, 128, 4096):
            cases.append(tn(M, N, K, stream_k=1, **workspace("ok")))
    return cases


OPERATORS = {
    "none": lambda N: {},
    "bias_col": lambda N: dict(bias=addr(8), bias_mode=BIAS_COL),
    "bias_row": lambda N: dict(bias=addr(8), bias_mode=BIAS_ROW),
    "gelu": lambda N: dict(bias=addr(8), bias_mode=BIAS_COL, act=GELU),
    "swiglu": lambda N: dict(act=SWIGLU, ldc=N // 2),
    "glu": lambda N: dict(act=GLU, ldc=N // 2, bias=addr(8), bias_mode=BIAS_COL),
    "silu": lambda N: dict(act=SILU),
    "res": lambda N: dict(res=addr(3), ldres=N),
    "res_scale": lambda N: dict(res=addr(3), ldres=N, res_scale=addr(5)),
    "fused_norm": lambda N: dict(res=addr(3), ldres=N, c_bf16=addr(6), ld_c_bf16=N, row_sumsq=addr(7), ld_row_sumsq=N // 48),
    "sumsq_short": lambda N: dict(row_sumsq=addr(7), ld_row_sumsq=N // 64),
    "row_scale": lambda N: dict(row_scale=addr(4)),
    "gelu_aux": lambda N: dict(act=GELU, aux=addr(11), ld_aux=N),
    "gelu_bwd": lambda N: dict(act=GELU_BWD, aux=addr(11), ld_aux=N),
    "exp2": lambda N: dict(act=EXP2, bias=addr(8), bias_mode=BIAS_ROW),
    "mul_aux": lambda N: dict(act=MUL_AUX, aux=addr(11), ld_aux=N, bias=addr(8), bias_mode=BIAS_ROW),
    "gather": lambda N: dict(gather1=addr(10), gather_a=1, gather_b=1),
    "rowadd": lambda N: dict(rowadd=addr(9), ld_rowadd=N, rowadd_period=8),
    "rowadd_res": lambda N: dict(rowadd=addr(9), ld_rowadd=N, rowadd_period=8, res=addr(3), ldres=N),
    "gadd": lambda N: dict(gadd=addr(9), gadd_index=addr(10), gadd_div=4, ld_gadd=N),
}
MISALIGN = [dict(C=addr(3, 4)), dict(C=addr(3, 8)), dict(bias=addr(8, 4)), dict(res=addr(3, 4)), dict(res_scale=addr(5, 8)), dict(c_bf16=addr(6, 2)),
            dict(rowadd=addr(9, 4)), dict(A=addr(1, 8))]


def sampled_cases(n, seed=20251020):
    rng = random.Random(seed)
    cases = []
    for _ in range(n):
        M = rng.choice([64, 128, 256, 512, 4096, 16384])
        N = rng.choice([128, 192, 384, 1408, 3072, 9216, 12288])
        K = rng.choice([64, 256, 3072, 12288])
        role = rng.choice(list(ROLE))
        trans = rng.random() < 0.2
        d = (tn if trans else nt)(M, N, K, c_dtype=rng.choice([F32, BF16]), role=ROLE[role], tile_hint=rng.randrange(7))
        if role in ("qkv", "ff1", "out_proj", "ff2") and rng.random() < 0.5:
            d = model_ops(role, M, N, K, tile_hint=d["tile_hint"])   # the role's own operator set, so that the role kernels are reached
            if trans:
                d.update(lda=M, ldb=N, trans_ab=1)
            if rng.random() < 0.3:
                d["alpha"] = 0.5
        else:
            d.update(OPERATORS[rng.choice(list(OPERATORS))](N))
        if rng.random() < 0.2:
            d.update(batch1=rng.choice([2, 4]), batch0=rng.choice([1, 3]), sA1=M * K * 3, sA0=M * K, sB1=N * K * 3, sB0=N * K, sC1=M * N * 3, sC0=M * N)
        if rng.random() < 0.4:
            d["stream_k"] = 1
            d.update(workspace(rng.choice(["ok", "ok", "ok", "none", "small", "odd"])))
        if rng.random() < 0.15:
            d.update({k: v for k, v in rng.choice(MISALIGN).items() if d.get(k) or k in ("A", "C")})
        if rng.random() < 0.1:
            d["ldc"] = d["ldc"] + rng.choice([1, 2, 6])
        cases.append(d)
    return cases


def invalid_cases():
    """One deliberately invalid descriptor per check of tribe_gemm_bf16, in the order of the checks."""
    big = 256 * 46341   # 46341^2 tiles of 256^2 > 2^31
    fused = OPERATORS["fused_norm"]
    return [
        None,
        nt(0, 128, 64), nt(128, 128, 96), nt(128, 128, 64, batch0=0), nt(128, 128, 64, B=0), nt(128, 128, 64, lda=68), nt(128, 128, 64, sB0=4),
        nt(128, 128, 64, A=addr(1, 8)), nt(128, 128, 128, ldb=64), nt(128, 128, 64, ldc=64), nt(128, 129, 64, act=SWIGLU, ldc=129),
        nt(128, 128, 64, act=SWIGLU, res=addr(3), ldres=128), nt(128, 128, 64, c_dtype=2), nt(128, 128, 64, bias_mode=BIAS_COL),
        nt(128, 128, 64, rowadd=addr(9), ld_rowadd=128), nt(128, 128, 64, gadd=addr(9), ld_gadd=128, gadd_div=4), nt(128, 128, 64, gather_b=1),
        nt(128, 128, 64, act=GELU_BWD), nt(128, 128, 64, act=MUL_AUX, aux=addr(11), ld_aux=256), nt(128, 128, 64, act=EXP2, res=addr(3), ldres=128),
        nt(128, 128, 64, act=GELU, aux=addr(11), ld_aux=64), nt(128, 128, 64, act=GELU, aux=addr(11), ld_aux=128, batch1=2), nt(128, 128, 64, sBias0=8),
        nt(256, 256, 64, batch1=2, **fused(256)), nt(256, 256, 64, act=SILU, row_scale=addr(4)), nt(256, 256, 64, **dict(fused(256), ldres=258)),
        nt(256, 256, 64, **dict(fused(256), C=addr(3, 8))), nt(256, 256, 64, BF16, **fused(256)), nt(256, 256, 64, **dict(fused(256), ld_c_bf16=128)),
        nt(256, 320, 64, **fused(320)), nt(512, 3072, 64, tile_hint=4, **dict(fused(3072), ld_row_sumsq=48)), nt(256, 256, 64, **dict(fused(256), ld_row_sumsq=3)),
        tn(260, 256, 64), tn(256, 256, 64, lda=128), tn(256, 256, 64, act=SILU), tn(256, 256, 64, gather1=addr(10), gather_a=1),
        nt(big, big, 64), nt(128, 128, 64, batch1=65536),
        tn(256, 256, 512, stream_k=1, bias=addr(8), bias_mode=BIAS_COL, **workspace("ok")), tn(256, 256, 512, c_dtype=BF16, stream_k=1, **workspace("ok")),
        tn(2048, 2048, 16384, stream_k=1), tn(2048, 2048, 16384, stream_k=1, **workspace("small")), tn(2048, 2048, 16384, stream_k=1, **workspace("odd")),
        nt(128, 3072, 12288, stream_k=1), nt(128, 3072, 12288, stream_k=1, **workspace("small")), nt(128, 3072, 12288, stream_k=1, **workspace("odd")),
    ]


def fp8_cases():
    good = [nt(M, N, K, dt, **dict(ops(N), **extra)) for M in (128, 4096) for N in (1408, 3072) for K in (128, 3072) for dt in (F32, BF16)
            for ops in (OPERATORS["none"], OPERATORS["gelu"], OPERATORS["swiglu"], OPERATORS["glu"], OPERATORS["silu"], OPERATORS["res_scale"])
            for extra in ({}, dict(batch1=3, sA1=M * K, sB1=N * K, sC1=M * N))]
    big = 256 * 46341
    bad = [None, nt(128, 128, 0), nt(128, 128, 64), nt(128, 128, 128, batch1=0), nt(128, 128, 128, C=0), nt(128, 128, 128, lda=136), nt(128, 128, 128, B=addr(2, 4)),
           nt(128, 128, 256, lda=128), tn(128, 256, 256), nt(128, 130, 128, act=GLU, ldc=64), nt(128, 128, 128, act=SWIGLU, bias=addr(8), bias_mode=BIAS_ROW),
           nt(128, 128, 128, c_dtype=7), nt(128, 128, 128, bias_mode=BIAS_ROW), nt(128, 128, 128, rowadd=addr(9), rowadd_period=-1),
           nt(128, 128, 128, gadd=addr(9), gadd_index=addr(10)), nt(128, 128, 128, gather_a=1), nt(128, 128, 128, act=GELU_BWD, aux=addr(11), ld_aux=128),
           nt(128, 128, 128, act=GELU, aux=addr(11), ld_aux=128), nt(big, big, 128), nt(128, 128, 128, batch0=70000)]
    return good + bad


def record():
    from tribe_hip import _lib

    fields = [name for name, _ in _lib.GemmDesc._fields_ if name != "alpha"]
    cases = [(0, d) for d in model_cases() + sampled_cases(2600) + invalid_cases()] + [(1, d) for d in fp8_cases()]
    desc = np.zeros((len(cases), len(fields)), dtype=np.int64)
    alpha = np.zeros(len(cases), dtype=np.float32)
    null = np.zeros(len(cases), dtype=np.int8)
    fp8 = np.array([f for f, _ in cases], dtype=np.int8)
    out = np.zeros((len(cases), len(OUT_FIELDS)), dtype=np.int64)
    messages, message_of = [""], np.zeros(len(cases), dtype=np.int32)
    handle = _lib.lib()
    for i, (is_fp8, spec) in enumerate(cases):
        got = (C.c_int64 * len(OUT_FIELDS))()
        if spec is None:
            null[i] = 1
            rc = handle.tribe_debug_gemm_plan(None, is_fp8, got, len(OUT_FIELDS))
        else:
            d = _lib.GemmDesc()
            for k, v in spec.items():
                setattr(d, k, v)
            desc[i] = [getattr(d, name) or 0 for name in fields]
            alpha[i] = d.alpha
            rc = handle.tribe_debug_gemm_plan(C.byref(d), is_fp8, got, len(OUT_FIELDS))
        out[i] = list(got)
        assert rc == out[i][0]
        text = handle.tribe_last_error().decode() if rc != 0 else ""
        if text not in messages:
            messages.append(text)
        message_of[i] = messages.index(text)
    np.savez_compressed(OUT, note=np.array("recorded from the commit before csrc/gemm_plan.cpp; do not regenerate (see make_golden_gemm_plan.py)"),
                        fields=np.array(fields), out_fields=np.array(OUT_FIELDS), desc=desc, alpha=alpha, null=null, fp8=fp8, out=out,
                        messages=np.array(messages), message_of=message_of)
    print(f"{len(cases)} cases, {len(messages) - 1} distinct error texts, {int((out[:, 0] == 0).sum())} accepted -> {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    record()
    sys.path.insert(0, str(ROOT / "tests"))
    import test_gemm_plan_golden as t   # the coverage conditions are conditions on the fixture: check them when recording

    t.test_fixture_covers_the_dispatch()
    print("coverage conditions hold")
