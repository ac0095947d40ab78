/*
 * tribe_hip.h -- C ABI of libtribe_hip.so: the MI355X (gfx950) native trimodal
 * fMRI-encode hot path of TRIBE (vovw/algonauts-2025).
 *
 * This is the drop-in boundary: plain pointers and sizes only, no torch types.
 * Every entry point below replaces one piece of the reference's Python/PyTorch
 * hot path; the reference line range it replaces is cited (paths relative to
 * the reference checkout).  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *  - All pointers are DEVICE pointers unless a name ends in _host.
 *  - The caller owns every buffer including the workspace; the library never
 *    allocates or frees device memory and keeps no pointer past return.
 *  - Every call is asynchronous on the `hipStream_t` passed as `void* stream`
 *    (torch: torch.cuda.current_stream().cuda_stream).
 *  - Return value: 0 = OK; < 0 = argument / shape / alignment error (message
 *    via tribe_last_error()); > 0 = hipError_t from the launch.  No exception
 *    crosses the ABI.
 *  - "bf16" buffers are uint16_t bit patterns (round-to-nearest-even from f32).
 *  - Row-major everywhere; "ld*" are leading dimensions in ELEMENTS.
 */
#ifndef TRIBE_HIP_H
#define TRIBE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRIBE_ABI_VERSION 5   /* bumped whenever a descriptor struct changes layout (round 2 changed three without a bump) */

enum tribe_dtype { TRIBE_F32 = 0, TRIBE_BF16 = 1, TRIBE_F64 = 2 };
/* tribe_gemm_desc.c_dtype only: the f32 residual stream kept as TWO 16-bit planes, hi = bf16(x) rounded to nearest even (what c_bf16
 * holds anyway: the next GEMM's A operand) and lo = the low 16 bits of the f32 word, so that the stream is written once instead of as
 * f32 + bf16 copy.  Decode: word = ((hi - (lo > 0x8000)) << 16) | lo.  Lossless except for the exact tie that rounded UP (lo == 0x8000
 * under an odd top half), which is stored as lo = 0x8001: that element carries x + 1 ulp.  hi is never altered.
 * A lo row is 2 N 16-bit slots wide: column c sits at slot 2 (c & ~63) + (c & 63), i.e. in the first 128 bytes of the 256 that the f32 words
 * of its 64-column strip take.  The plane can therefore live INSIDE the f32 buffer it stands for (lo pointer = the f32 pointer, pitch 2 * ld):
 * every launch below then runs in place on that buffer, as the f32 epilogue does, and the stream needs no memory of its own.
 * Out-proj / FF2 role kernels at 256 x 256 tiles only (tribe_gemm_epilogue_path == 1); every other launch refuses these values.
 *   PLANES_OUT    res = f32 [M, ldres];                c_bf16 = hi out, C = lo out (ldc >= 2 N 16-bit slots; may be res itself)
 *   PLANES_INOUT  hi in = c_bf16, lo in = res (ldres >= 2 N slots, may alias C);   c_bf16 = hi out (in place), C = lo out
 *   PLANES_IN     hi in = c_bf16 (read only), lo in = res (ldres >= 2 N slots);    C = f32 out (may be res itself), no bf16 copy */
enum tribe_c_planes { TRIBE_F32_PLANES_OUT = 16, TRIBE_F32_PLANES_INOUT = 17, TRIBE_F32_PLANES_IN = 18 };
enum tribe_act {
  TRIBE_ACT_NONE = 0,
  TRIBE_ACT_GELU = 1,   /* exact (erf) GELU */
  TRIBE_ACT_SWIGLU = 2, /* columns come in (gate, up) pairs: out[:, j] = silu(v[:, 2j]) * v[:, 2j+1]; C has N/2 columns */
  TRIBE_ACT_SILU = 3,
  TRIBE_ACT_GLU = 4,    /* (a, b) column pairs: out[:, j] = v[:, 2j] * sigmoid(v[:, 2j+1]); C has N/2 columns (nn.GLU) */
  TRIBE_ACT_GELU_BWD = 5, /* backward of GELU: out = v * gelu'(aux[m][n]), aux = saved pre-activation (bf16) */
  /* attention backward without [B, h, T, T] f32 tensors (round 3): with alpha = scale * log2(e) and a ROW bias of -lse2 (the forward kernel's
   * base-2 log-sum-exp) the score GEMM writes P = exp2(alpha * q.k - lse2[row]) directly ... */
  TRIBE_ACT_EXP2 = 6,
  /* ... and with alpha = scale and a row bias of -scale * D[row] (D = rowsum(dO * O)) the dP GEMM writes dS = (alpha * dO.v + bias[row]) * aux[m][n],
   * aux = P (bf16, same layout AND batch strides as C) */
  TRIBE_ACT_MUL_AUX = 7,
  /* codes of tribe_norm_act_fwd / tribe_norm_act_bwd (which also take NONE and GELU); no GEMM epilogue implements them */
  TRIBE_ACT_RELU = 8,
  TRIBE_ACT_ELU = 9     /* alpha = 1 */
};
enum tribe_bias_mode { TRIBE_BIAS_NONE = 0, TRIBE_BIAS_COL = 1, TRIBE_BIAS_ROW = 2 };
/* which operator of the path a GEMM launch serves: selects the kernel SYMBOL (per-operator rows in
 * rocprofv3 --stats and in the tribe_prof_* event profile); arithmetic is identical for all roles */
enum tribe_gemm_role {
  TRIBE_ROLE_GENERIC = 0, TRIBE_ROLE_PROJECTOR = 1, TRIBE_ROLE_QKV = 2, TRIBE_ROLE_ATTN_SCORES = 3, TRIBE_ROLE_ATTN_PV = 4,
  TRIBE_ROLE_OUT_PROJ = 5, TRIBE_ROLE_FF1 = 6, TRIBE_ROLE_FF2 = 7, TRIBE_ROLE_VOXEL_HEAD = 8,
  TRIBE_ROLE_ATTENTION = 9, /* the fused attention launches (not a GEMM role: profile slot only; flops = 4 * T * dim_head per query row and head) */
  TRIBE_ROLE_COUNT = 10
};

int tribe_version(void);
/* sizeof() of every descriptor struct of this header, in declaration order (gemm_desc, attention_desc, encoder_layer, encoder_desc,
 * vit_layer, vit_fp8_layer, vjepa2_desc, conformer_layer, conformer_fp8_layer, w2vbert_desc, llama_layer, llama_fp8_layer, llama_desc,
 * feature_piece, adam_tensor): a binding compares them with its own mirrors at load time, so that a stale library or a stale mirror
 * fails loudly instead of mis-striding a table.  Writes min(n, 15) entries, returns 15. */
int tribe_abi_struct_sizes(int64_t* sizes, int32_t n);
/* thread-local, valid until the next failing call on this thread */
const char* tribe_last_error(void);

/* ------------------------------------------------------------------------- *
 * Generic MFMA GEMM (the workhorse every dense contraction below lowers to)
 *   C[b1][b0][m][n] = epi( alpha * sum_k A[b1][b0][m][k] * B[b1][b0][n][k] )
 * A, B bf16 with K contiguous ("NT" form == nn.Linear's [out,in] weights).
 * K must be a multiple of 64 (callers zero-pad K); M, N arbitrary.
 * epi(v) = act(v + bias) + res * res_scale + rowadd[m % period] + gadd[gidx[m / div]]
 * Replaces torch.nn.functional.linear / torch.einsum / torch.bmm call sites of
 * model.py:157, common.py:64 and the x_transformers Attention / FeedForward.
 * ------------------------------------------------------------------------- */
typedef struct tribe_gemm_desc {
  int64_t M, N, K;
  int64_t batch1, batch0; /* grid z = batch1 * batch0; b1 = z / batch0, b0 = z % batch0 */
  const void* A; int64_t lda, sA1, sA0;
  const void* B; int64_t ldb, sB1, sB0;
  void* C; int64_t ldc, sC1, sC0;
  int32_t c_dtype;         /* TRIBE_F32 or TRIBE_BF16 (or an enum tribe_c_planes value: the residual stream as two 16-bit planes) */
  float alpha;
  const int64_t* gather1;  /* optional [batch1]: index replacing b1 for A (gather_a) and bias (gather_bias) */
  int32_t gather_a, gather_bias;
  const float* bias; int32_t bias_mode; int64_t sBias1; /* f32; per-col [N] or per-row [M]; + b1' * sBias1 */
  int32_t act;
  const float* res; int64_t ldres, sRes1, sRes0; /* f32 residual, may alias C when c_dtype == F32 */
  const float* res_scale;  /* f32 [N] or NULL (= 1) */
  const float* rowadd; int64_t ld_rowadd, rowadd_period; /* + rowadd[(m % period)][n] */
  const float* gadd; const int64_t* gadd_index; int64_t gadd_div, ld_gadd; /* + gadd[gadd_index[m / div]][n] */
  /* aux bf16 [M, N] (ld_aux): with act == GELU the PRE-activation is also stored there (training forward);
   * with act == GELU_BWD it is read.  NULL = unused. */
  void* aux; int64_t ld_aux;
  int32_t gather_b;        /* gather1 also replaces b1 for the B operand */
  int32_t role;            /* enum tribe_gemm_role */
  int32_t tile_hint;       /* 0 = automatic; tests / tuning: 1 = 128x128 double-buffered, 2 = 256x256, 3 = 128x128 ring, 4 = 256x192, 5 = 256x256 one-wave-per-SIMD,
                            * 6 = 8-wave 256-row tiles (256x192 when only that width divides N) with the GENERIC epilogue even where the role-compiled one applies (A/B runs, tests) */
  /* 1 = the operands are given TRANSPOSED: A is At [K, M] (lda >= M), B is Bt [K, N] (ldb >= N), C[m][n] = sum_k At[k][m] Bt[k][n] --
   * the weight gradient dW = dY^T X straight from the row-major dY [tokens, N_out] and X [tokens, K_in] the forward produced, without
   * the explicit transposes (torch.nn.functional.linear's backward in the reference).  M, N multiples of 8; plain epilogue only. */
  int32_t trans_ab;
  /* ScaleNorm folded into the GEMMs either side of it (x_transformers pre-norm: y = W . (x * s_m), s_m = g sqrt(d) / |x_m|):
   * the PRODUCER of x (f32 C) also emits a bf16 copy and per-row partial sums of squares, one slot per wave column group
   * (row_sumsq[m * ld_row_sumsq + n / w], w = 64 or 48 columns by the tile the launch gets: tribe_gemm_sumsq_slots() says how
   * many slots per row THIS descriptor will write -- pass it on as n_partial); tribe_rownorm_scale_fwd turns them into s_m; the CONSUMER multiplies its
   * accumulator rows by row_scale[m] before bias / activation (the scaling commutes with the product).  Un-batched
   * launches whose N is a multiple of the tile and whose operands are 16-byte aligned only; NULL = unused. */
  uint16_t* c_bf16; int64_t ld_c_bf16;
  float* row_sumsq; int64_t ld_row_sumsq;
  const float* row_scale;
  int64_t sBias0;          /* + b0 * sBias0 on the bias pointer (a ROW bias per (b1, b0) batch: the attention backward's -lse2 / -scale * D); 0 = none */
  /* 1 = the launcher may share out the REDUCTION of a launch whose output tiles do not fill the chip over more workgroups; the parts travel
   * through stream_k_ws and a second launch on the same stream sums them in a fixed order (bit-reproducible) and writes C.
   *   trans_ab (the weight-gradient form): stream-K -- the tiles of the last, partial round are cut into equal runs of K-steps over all CUs,
   *     when that round is at most HALF full and a run gets at least 8 K-steps: dW of a 12288 x 3072 layer (576 tiles = 2 rounds + 64 on 256 CUs)
   *     and of the 64-tile projectors are split; dW of a 3072 x 3072 layer (144 tiles) is not -- fuller remainders measured slower split.
   *     Plain f32 product only (no bias / activation / residual / batch): the launch refuses anything else.
   *   otherwise (NT form): split-K of grids of at most half a round of 128 x 128 tiles (M = 128 rows: BASELINE config 1) -- 2..8 workgroups
   *     per tile; the second launch applies alpha, row_scale, bias, GELU, the scaled residual or periodic row add, c_bf16 and row_sumsq.
   * The workspace must hold tribe_gemm_stream_k_workspace_bytes(desc) bytes (0 = this launch is not split), 16-byte aligned, and is free
   * again when the launch is done. */
  int32_t stream_k; int32_t reserved0;
  void* stream_k_ws; int64_t stream_k_ws_bytes;
} tribe_gemm_desc;

int tribe_gemm_bf16(const tribe_gemm_desc* desc, void* stream);
/* number of row_sumsq slots per row the launch of `desc` writes (N / 64, or N / 48 when the launch gets 256 x 192 tiles); < 0 on a bad
 * descriptor.  Depends on M, N, K, the batch counts, tile_hint and the fused-norm operands only. */
int tribe_gemm_sumsq_slots(const tribe_gemm_desc* desc);
/* which epilogue the launch of `desc` runs (host-side, no GPU call): 0 = generic (operators decided at run time), 1 = the 8-wave 256-row
 * kernel's epilogue compiled for the operator set of desc->role (QKV / FF1 / OUT_PROJ / FF2 with exactly their model operators, un-batched,
 * alpha == 1, N a multiple of the tile width, 16-byte operands; FF2 only under tile_hint 2 / 4 or with a tribe_c_planes c_dtype, which reports 1
 * at 256 x 256 tiles only), 2 = the one-wave-per-SIMD kernel's (tile_hint 5); < 0 on a bad descriptor */
int tribe_gemm_epilogue_path(const tribe_gemm_desc* desc);
/* The plane format of enum tribe_c_planes as stand-alone kernels (tests, debugging; not on the hot path): n f32 words -> hi, lo and back. */
int tribe_f32_to_planes(const float* x, int64_t n, uint16_t* hi, uint16_t* lo, void* stream);
int tribe_planes_to_f32(const uint16_t* hi, const uint16_t* lo, int64_t n, float* x, void* stream);
/* bytes of desc->stream_k_ws this launch needs, read from the plan the launch itself reads: 0 when it would not be split (stream_k clear, no
 * partial round or small grid worth cutting, or a trans_ab request with operators the launch refuses) */
int64_t tribe_gemm_stream_k_workspace_bytes(const tribe_gemm_desc* desc);
/* The stream-K schedule of a launch with `tiles` output tiles of `nk` K-steps on this device (host-only, for inspection and tests):
 * out[0..3] = {tiles computed whole, K-steps in the split region, K-steps per run, runs}, out[4 .. 259] = the order in which the runs' second
 * parts are queued.  Returns the grid size (== tiles when nothing is split, and then out[0] >= tiles). */
int tribe_gemm_stream_k_plan(int32_t tiles, int32_t nk, int32_t* out);
/* scale[m] = g[0] * gain_scale / max(sqrt(sum_p partial[m, p]), eps): the ScaleNorm factor from the partial sums of squares a
 * GEMM epilogue left in row_sumsq (partial f32 [rows, n_partial], row-major). */
int tribe_rownorm_scale_fwd(const float* partial, int64_t rows, int64_t n_partial, const float* g, float gain_scale, float eps,
                            float* scale, void* stream);

/* D[row][h] = sum_d a[row][h * dim_head + d] * b[row][h * dim_head + d] * scale (bf16 inputs [rows, heads * dim_head], row strides in elements,
 * f32 output [B, heads, T] with row = b * T + t): the rowsum(dO * O) term of the attention backward, written negated and pre-scaled as the row bias
 * of the dS GEMM wants it when scale < 0. */
int tribe_rowdot_heads_bf16(const uint16_t* a, int64_t ld_a, const uint16_t* b, int64_t ld_b, int64_t B, int64_t T, int32_t heads, int32_t dim_head,
                            float scale, float* out, void* stream);

/* Measurement hook (bench.py): while enabled, every GEMM launch is bracketed by HIP events on ITS
 * stream.  tribe_prof_end synchronises them and returns, per role, the summed kernel time (ms), the
 * launch count and the summed algorithmic FLOPs (2*M*N*K*batches).  Host arrays of >= TRIBE_ROLE_COUNT.
 * PROCESS-WIDE state (one mutex-guarded record list): the compute entry points are re-entrant and keep no state, but this
 * diagnostic pair, tribe_attention_set_mode and the one-time hipFuncSetAttribute flags of the kernels are per process, not
 * per device or per thread -- in line with the deployment model (one process per GPU, main.py:388-395).  Call begin / end
 * from the thread that launches. */
int tribe_prof_begin(int32_t max_records);
int tribe_prof_end(int32_t n_roles, double* total_ms_host, int64_t* count_host, double* flops_host);

/* ------------------------------------------------------------------------- *
 * Packing (one-time per parameter version; fp32 master weights stay in torch)
 * ------------------------------------------------------------------------- */
/* f32 [rows, cols] (ld = ld_src) -> bf16 [rows_pad, cols_pad], zero padded */
int tribe_pack_weight_bf16(const float* src, int64_t rows, int64_t cols, int64_t ld_src,
                           uint16_t* dst, int64_t rows_pad, int64_t cols_pad, void* stream);
/* SubjectLayers weights (common.py:26) f32 [S, C, V] -> bf16 [S, V_pad, C_pad] (transposed, zero padded) */
int tribe_pack_subject_weights(const float* w, int64_t S, int64_t C, int64_t V,
                               uint16_t* dst, int64_t V_pad, int64_t C_pad, void* stream);

/* ------------------------------------------------------------------------- *
 * a3: FmriEncoder.aggregate_features prologue (model.py:146-155)
 *   feat [B, L, D, T] (f32 / bf16 / f64) -> bf16 [B*T, K_pad]
 *   layer_mean == 0: "b l d t -> b t (l d)"; == 1: mean over l then "b d t -> b t d"
 * ------------------------------------------------------------------------- */
int tribe_pack_features(const void* feat, int32_t dtype, int64_t B, int64_t L, int64_t D, int64_t T,
                        int32_t layer_mean, uint16_t* dst, int64_t K_pad, void* stream);

/* a3/a4: one modality's projector nn.Linear (model.py:157) writing its column
 * slice of the fused [B*T, hidden] f32 stream (torch.cat, model.py:161-162) and
 * adding time_pos_embed[:, :T] (+ subject_embed[subject_id]) (model.py:169-172).
 * accumulate != 0 adds into x (feature_aggregation == "sum", model.py:163-164). */
int tribe_projector_fwd(const uint16_t* feat_packed, int64_t BT, int64_t T, int64_t K_pad,
                        const uint16_t* w_packed /*[N_out, K_pad]*/, const float* bias /*[N_out]*/, int64_t N_out,
                        float* x, int64_t hidden, int64_t col0, int32_t accumulate,
                        const float* pos_embed /*[>=T, hidden] or NULL*/,
                        const float* subj_embed /*[S, hidden] or NULL*/, const int64_t* subject_id /*[B]*/,
                        void* stream);
/* zero-filled block for a modality without projector (model.py:143-144) incl. the pos/subject adds */
int tribe_projector_zero_fwd(int64_t BT, int64_t T, int64_t N_out, float* x, int64_t hidden, int64_t col0,
                             const float* pos_embed, const float* subj_embed, const int64_t* subject_id,
                             void* stream);

/* ------------------------------------------------------------------------- *
 * a6: x_transformers.Encoder (called at model.py:173)
 * ------------------------------------------------------------------------- */
/* ScaleNorm: y = x / max(||x||_2, eps) * gain_scale * g[0]  (g read on device) */
int tribe_scalenorm_fwd(const float* x, int64_t rows, int64_t dim, const float* g, float gain_scale, float eps,
                        void* y, int32_t y_dtype, void* stream);
/* (partial) rotary embedding, in place, on the first n_heads heads of every row of a bf16 buffer with row stride
 * row_stride elements (a fused qkv buffer: q heads followed by k heads).  Position of row r is r % T.
 * cos/sin: f32 [T, rot_dim/2]; interleaved != 0 pairs (2i,2i+1) (x_transformers 2.x), else (i, i+rot_dim/2)
 * (x_transformers 1.27 and HF rotate_half, modeling_llama.py). */
/* interleaved == 2: per-ELEMENT tables f32 [T, rot_dim] with (2i, 2i+1) pairs -- out[2i] = x[2i] C[2i] - x[2i+1] S[2i],
 * out[2i+1] = x[2i+1] C[2i+1] + x[2i] S[2i+1] (VJEPA2RopeAttention.apply_rotary_embeddings, modeling_vjepa2.py:180-294) */
int tribe_rotary_fwd(uint16_t* x, int64_t rows, int64_t T, int64_t row_stride, int32_t n_heads, int32_t dim_head,
                     int32_t rot_dim, const float* cos_tab, const float* sin_tab, int32_t interleaved, void* stream);
/* softmax(q k^T * scale) v for all (batch, head); qkv as above; out bf16 [rows, heads*dim_head] */
size_t tribe_attention_workspace_bytes(int64_t B, int64_t T, int32_t heads, int32_t dim_head);
/* 0 (default): fused flash-style kernel for dim_head in {64,128,192,384}, else the materialised path;
 * 1: always materialise scores (QK^T GEMM -> f32 softmax -> PV GEMM), kept as a cross-check;
 * 2: fused, but dim_head 384 and 64 on the 16-query-row kernel of the other head sizes instead of their own kernels
 *    (A/B measurements);
 * 3: fused, dim_head 384 on the key-split kernel (two waves per SIMD, each owning half of the head dimension);
 * 4: fused, dim_head 64 (bidirectional) on the 64-rows-per-wave kernel in phase-separated order (the default interleaves the two row
 *    tiles of a wave); 5: dim_head 64 on the anti-phase 8-wave kernel.  Modes 2-5 exist for A/B measurements (csrc/attention_d64.hip).
 * Process-wide switch: set it from one thread, between launches. */
int tribe_attention_set_mode(int32_t mode);
int tribe_attention_fwd(const uint16_t* qkv, int64_t B, int64_t T, int32_t heads, int32_t dim_head, float scale,
                        uint16_t* out, void* workspace, size_t workspace_bytes, void* stream);
/* general form of the fused kernel: separate q / k / v views (row = b*T + t, row strides in elements, ld_k == ld_v),
 * grouped-query attention (heads_q % heads_kv == 0; query head h reads kv head h / (heads_q/heads_kv)) and an
 * optional causal mask (key <= query).  dim_head in {64, 128, 192, 384}.  out[row][h*dim_head + d]. */
typedef struct tribe_attention_desc {
  const uint16_t* q; const uint16_t* k; const uint16_t* v;
  int64_t ld_q, ld_k, ld_v;
  uint16_t* out; int64_t ld_out;
  int64_t B, T;
  int32_t heads_q, heads_kv, dim_head, causal;
  float scale;
  /* optional "relative_key" position bias (Wav2Vec2BertSelfAttention, modeling_wav2vec2_bert.py:308-320):
   * score[i][j] += rel_qe[b*T + i][h * rel_stride_h + clamp(j - i, -rel_left, rel_right) + rel_left], where
   * rel_qe = q . distance_embedding^T (f32, computed by a GEMM beforehand).  NULL = none.  dim_head 64 only. */
  const float* rel_qe; int64_t ld_rel_qe; int32_t rel_stride_h, rel_left, rel_right;
  /* optional: base-2 log-sum-exp of every query's scaled scores, f32 [B, heads_q, T]: lse2 = max + log2(sum 2^(s * scale * log2 e - max)), so
   * that P = exp2(s * scale * log2 e - lse2) -- what a backward pass needs to recompute P without a softmax.  dim_head 384, bidirectional,
   * default mode only (the one-wave-per-SIMD kernel): tribe_attention_fwd_ex fails otherwise.  NULL = not wanted. */
  float* lse;
} tribe_attention_desc;
int tribe_attention_fwd_ex(const tribe_attention_desc* desc, void* stream);
/* 1 when tribe_attention_fwd_ex can write desc->lse for this head size under the current tribe_attention_set_mode */
int tribe_attention_lse_supported(int32_t dim_head, int32_t causal);

typedef struct tribe_encoder_layer {
  /* attention block */
  const float* attn_norm_g;       /* [1] */
  const uint16_t* w_qkv;          /* bf16 [3*inner, dim]  rows: q | k | v */
  const uint16_t* w_out;          /* bf16 [dim, inner] */
  const float* attn_res_scale;    /* [dim] or NULL */
  /* feed-forward block */
  const float* ff_norm_g;         /* [1] */
  const uint16_t* w_ff1;          /* bf16 [ff_inner, dim] */
  const float* b_ff1;             /* [ff_inner] */
  const uint16_t* w_ff2;          /* bf16 [dim, ff_inner] */
  const float* b_ff2;             /* [dim] */
  const float* ff_res_scale;      /* [dim] or NULL */
} tribe_encoder_layer;

typedef struct tribe_encoder_desc {
  int64_t B, T;
  int32_t dim, depth, heads, dim_head, ff_inner, rot_dim, rotary_interleaved;
  float norm_gain_scale, norm_eps;   /* ScaleNorm flavour */
  const tribe_encoder_layer* layers_host; /* HOST array [depth] of device pointers */
  const float* final_norm_g;         /* [1] */
  const float* cos_tab; const float* sin_tab; /* f32 [T, rot_dim/2] or NULL when rot_dim == 0 */
} tribe_encoder_desc;

/* Process-wide switches beside tribe_attention_set_mode (set them from one thread, between launches):
 * residual planes, 1 (default) = between the first out-proj and the last FF2 the residual stream lives as two 16-bit planes (enum
 *   tribe_c_planes: hi in the workspace's bf16 buffer, lo inside x itself) wherever the fused norms hold, M > 512 and every residual GEMM
 *   runs the 256 x 256 role kernel; 0 = the f32 stream + bf16 copy.  x is f32 on entry and on return either way; the workspace is the same.
 * residual tile hint: the tribe_gemm_desc.tile_hint of the out-proj / FF2 launches, 0 (default) or 2 (256 x 256 role kernel whatever
 *   the shape: tests and A/B runs of small shapes). */
int tribe_encoder_set_residual_planes(int32_t on);
int tribe_encoder_set_residual_tile_hint(int32_t hint);
size_t tribe_encoder_workspace_bytes(const tribe_encoder_desc* d);
/* x: f32 [B*T, dim] residual stream, updated in place; y: final-normed output (bf16 or f32) [B*T, dim] */
int tribe_encoder_fwd(const tribe_encoder_desc* d, float* x, void* y, int32_t y_dtype,
                      void* workspace, size_t workspace_bytes, void* stream);
/* tribe_encoder_fwd with option bits; flags = 0 is tribe_encoder_fwd itself, an unknown bit is an error.  The workspace is the same.
 * TRIBE_ENCODER_CAUSAL: every layer attends under a causal mask (key <= query; x_transformers' Decoder).  q and k heads are rotated by
 *   tribe_rotary_fwd and the attention is tribe_attention_fwd_ex with causal = 1: dim_head in {64, 128, 192, 384}. */
#define TRIBE_ENCODER_CAUSAL 1u
int tribe_encoder_fwd_ex(const tribe_encoder_desc* d, uint32_t flags, float* x, void* y, int32_t y_dtype,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ---- streaming a causal encoder one position at a time: KV cache and single-query attention (csrc/attn_decode.hip) ----
 * A cache is two bf16 tensors K, V [B, heads, cap, dim_head] per layer (cap = capacity in positions): each (sequence, head) owns one
 * contiguous run of keys.  The encoder entry points take all layers at once: [depth, B, heads, cap, dim_head].
 *
 * tribe_kv_append: one position of every sequence.  qkv: the step's fused bf16 [B, 3 * heads * dim_head] rows (q heads | k heads | v heads).
 *   Rotates the q heads and the k heads in place at position `pos` -- tribe_rotary_fwd's arithmetic, bit for bit; interleaved 0 or 1;
 *   cos / sin f32 [> pos, rot_dim / 2]; rot_dim == 0: no rotation, tables unused -- and stores the rotated k heads and the v heads into slot
 *   `pos` of the two caches.  One launch; no other slot is touched.  Buffers 16-byte aligned. */
int tribe_kv_append(uint16_t* qkv, int64_t B, int32_t heads, int32_t dim_head, int32_t rot_dim, int32_t interleaved,
                    const float* cos_tab, const float* sin_tab, int64_t pos, uint16_t* k_cache, uint16_t* v_cache, int64_t cap,
                    void* stream);
/* tribe_attention_decode_fwd: out[b, h] = softmax(scale * q[b, h] . K[b, h, 0:n]^T) V[b, h, 0:n] for one query row per (b, h), n = pos + 1
 *   keys, 1 <= n <= cap; dim_head in {64, 128, 192, 384}.  q: bf16, head h of sequence b at q + b * ld_q + h * dim_head (ld_q = 3 * inner
 *   reads the q heads of a fused row); out: bf16 [B, heads * dim_head].  Softmax in f32, p rounded to bf16 before it multiplies V.  The keys
 *   of one (b, h) are split over tribe_attention_decode_splits(B, heads, n) workgroups -- a function of these three alone -- whose f32
 *   (m, l, o) parts travel through the workspace (tribe_attention_decode_workspace_bytes, 256-byte aligned; unused at one split) and are
 *   summed in split order by a second launch: no atomics, the same call gives the same bits.  Nothing at or beyond slot n is read. */
int32_t tribe_attention_decode_splits(int64_t B, int32_t heads, int64_t n);
size_t tribe_attention_decode_workspace_bytes(int64_t B, int32_t heads, int32_t dim_head, int64_t n);
int tribe_attention_decode_fwd(const uint16_t* q, int64_t ld_q, const uint16_t* k_cache, const uint16_t* v_cache, int64_t B,
                               int32_t heads, int32_t dim_head, int64_t cap, int64_t n, float scale, uint16_t* out,
                               void* workspace, size_t workspace_bytes, void* stream);
/* tribe_encoder_step_fwd: the causal encoder at position `pos` (0 <= pos < cap) given the caches of positions 0 .. pos-1; d->T must be 1,
 *   x f32 [B, dim] (updated in place), y [B, dim]; d->cos_tab / sin_tab hold at least pos + 1 rows.  Per layer: ScaleNorm, QKV GEMM,
 *   tribe_kv_append (slot pos), tribe_attention_decode_fwd (n = pos + 1), out-proj + residual, ScaleNorm, FF1 + GELU, FF2 + residual;
 *   then the final ScaleNorm.  The workspace size depends on the capacity, not on pos. */
size_t tribe_encoder_step_workspace_bytes(const tribe_encoder_desc* d, int64_t cap);
int tribe_encoder_step_fwd(const tribe_encoder_desc* d, float* x, void* y, int32_t y_dtype, uint16_t* k_cache, uint16_t* v_cache,
                           int64_t cap, int64_t pos, void* workspace, size_t workspace_bytes, void* stream);
/* tribe_encoder_prefill_fwd: tribe_encoder_fwd_ex with TRIBE_ENCODER_CAUSAL over d->T <= cap positions from an empty cache (same
 *   workspace: tribe_encoder_workspace_bytes), which also copies every layer's rotated k heads and v heads into slots 0 .. T-1: one more
 *   launch per layer. */
int tribe_encoder_prefill_fwd(const tribe_encoder_desc* d, float* x, void* y, int32_t y_dtype, uint16_t* k_cache, uint16_t* v_cache,
                              int64_t cap, void* workspace, size_t workspace_bytes, void* stream);

/* ---- block append: k positions at once onto a cache that holds `pos` of them (k >= 1, pos >= 0, pos + k <= cap; pos = 0 is a prefill) ----
 * Rows of a block are ordered [B, k]: row b * k + t is step t of sequence b, at position pos + t.
 *
 * tribe_kv_append_block: tribe_kv_append for k rows per sequence.  qkv: fused bf16 [B * k, 3 * heads * dim_head].  Rotates the q heads and
 *   the k heads of row b * k + t in place at position pos + t (cos / sin f32 [>= pos + k, rot_dim / 2]; tribe_rotary_fwd's arithmetic, bit
 *   for bit) and stores the rotated k heads and the v heads into slot pos + t.  One launch; no other slot is touched.
 * tribe_attention_extend_fwd: rectangular causal attention against the cache (the 16-query-rows-per-wave flash kernel of
 *   csrc/attention.hip in its block-append form).  Query row b * k + t (head h at q + row * ld_q + h * dim_head; ld_q = 3 * inner reads the
 *   q heads of the block's fused rows, already rotated) sees keys j <= pos + t of K, V [B, heads, cap, dim_head], which must already hold
 *   slots 0 .. pos + k - 1 (tribe_kv_append_block first).  out: bf16 [B * k, heads * dim_head].  dim_head in {64, 128, 192, 384}.  Nothing
 *   at or beyond slot pos + k is read.  B * heads * ceil(k / 128) workgroups, each walking its keys serially: no workspace, the same call
 *   gives the same bits.
 * tribe_encoder_extend_fwd: the causal encoder at positions pos .. pos + k - 1 given the caches of positions 0 .. pos - 1; d->T = k,
 *   x f32 [B * k, dim] (updated in place), y [B * k, dim]; d->cos_tab / sin_tab hold at least pos + k rows.  Per layer what
 *   tribe_encoder_step_fwd does, for k rows per sequence: ScaleNorm, QKV GEMM, tribe_kv_append_block, tribe_attention_extend_fwd,
 *   out-proj + residual, ScaleNorm, FF1 + GELU, FF2 + residual; then the final ScaleNorm. */
int tribe_kv_append_block(uint16_t* qkv, int64_t B, int64_t k, int32_t heads, int32_t dim_head, int32_t rot_dim, int32_t interleaved,
                          const float* cos_tab, const float* sin_tab, int64_t pos, uint16_t* k_cache, uint16_t* v_cache, int64_t cap,
                          void* stream);
int tribe_attention_extend_fwd(const uint16_t* q, int64_t ld_q, const uint16_t* k_cache, const uint16_t* v_cache, int64_t B,
                               int32_t heads, int32_t dim_head, int64_t cap, int64_t pos, int64_t k, float scale, uint16_t* out,
                               void* stream);
size_t tribe_encoder_extend_workspace_bytes(const tribe_encoder_desc* d, int64_t cap);
int tribe_encoder_extend_fwd(const tribe_encoder_desc* d, float* x, void* y, int32_t y_dtype, uint16_t* k_cache, uint16_t* v_cache,
                             int64_t cap, int64_t pos, void* workspace, size_t workspace_bytes, void* stream);

/* ---- slots: every sequence of a cache at a position of its own (independent timelines in one cache) ----
 * pos: a device array int32 [B], 4-byte aligned.  pos[b] is the number of positions sequence ("slot") b already holds; -1 marks a slot that
 * takes no part in the call.  A kernel cannot report a bad value without a synchronisation, so none ever dereferences a position outside
 * [0, cap - k]: a sequence with such a value is treated exactly as one that takes no part.  Callers validate their host copy.
 *
 * tribe_kv_append_slots: tribe_kv_append_block with a position per sequence.  Row b * k + t of the fused bf16 qkv [B * k, 3 * heads *
 *   dim_head] is rotated in place at position pos[b] + t and its k and v heads are stored into slot pos[b] + t of sequence b -- the block
 *   append's arithmetic, bit for bit; k = 1 is the step.  Neither the cache run nor the qkv rows of a sequence that takes no part are
 *   touched.  cos / sin f32 [>= cap, rot_dim / 2].  1 <= k <= cap.  One launch.
 * tribe_attention_decode_slots_fwd: tribe_attention_decode_fwd with n_b = pos[b] + 1 keys for sequence b.  n_max (host, 1 <= n_max <= cap)
 *   is an upper bound of every n_b; the kernel clamps n_b to it.  tribe_attention_decode_splits(B, heads, n_max) workgroups per (b, h), the
 *   chunk tribe_attention_decode_fwd takes at n = n_max: split s of sequence b owns keys [s * chunk, min(n_b, (s + 1) * chunk)), which may
 *   be empty, and the parts are merged in split order by the same rule -- no atomics, the same call gives the same bits, and with every
 *   pos[b] + 1 == n_max the bits are those of tribe_attention_decode_fwd(..., n = n_max).  The out row of a sequence that takes no part is
 *   written as zeros (bf16 +0).  Nothing at or beyond slot n_b of sequence b is read.  Workspace:
 *   tribe_attention_decode_workspace_bytes(B, heads, dim_head, n_max).
 * tribe_attention_extend_slots_fwd: tribe_attention_extend_fwd with the k query rows of sequence b at positions pos[b] .. pos[b] + k - 1
 *   against its slots 0 .. pos[b] + k - 1 (tribe_kv_append_slots first).  Every workgroup reads the position of its own sequence: the
 *   bits of sequence b are those of tribe_attention_extend_fwd run on that sequence alone at pos = pos[b].  The rows of a sequence that
 *   takes no part are written as zeros; nothing at or beyond slot pos[b] + k is read.
 * tribe_encoder_step_slots_fwd / tribe_encoder_extend_slots_fwd: tribe_encoder_step_fwd / tribe_encoder_extend_fwd with the two
 *   cache-aware launches of every layer in their slot forms and the same workspace (tribe_encoder_step_workspace_bytes /
 *   tribe_encoder_extend_workspace_bytes, which size by cap).  The step takes n_max as above.  Rows of sequences that take no part run
 *   through the norms and GEMMs like any other row and their outputs are to be discarded (their attention rows are zeros): pass finite
 *   values, zeros for example; rows are not compacted.  d->cos_tab / sin_tab hold at least cap rows. */
int tribe_kv_append_slots(uint16_t* qkv, int64_t B, int64_t k, int32_t heads, int32_t dim_head, int32_t rot_dim, int32_t interleaved,
                          const float* cos_tab, const float* sin_tab, const int32_t* pos, uint16_t* k_cache, uint16_t* v_cache, int64_t cap,
                          void* stream);
int tribe_attention_decode_slots_fwd(const uint16_t* q, int64_t ld_q, const uint16_t* k_cache, const uint16_t* v_cache, int64_t B,
                                     int32_t heads, int32_t dim_head, int64_t cap, const int32_t* pos, int64_t n_max, float scale,
                                     uint16_t* out, void* workspace, size_t workspace_bytes, void* stream);
int tribe_attention_extend_slots_fwd(const uint16_t* q, int64_t ld_q, const uint16_t* k_cache, const uint16_t* v_cache, int64_t B,
                                     int32_t heads, int32_t dim_head, int64_t cap, const int32_t* pos, int64_t k, float scale, uint16_t* out,
                                     void* stream);
int tribe_encoder_step_slots_fwd(const tribe_encoder_desc* d, float* x, void* y, int32_t y_dtype, uint16_t* k_cache, uint16_t* v_cache,
                                 int64_t cap, const int32_t* pos, int64_t n_max, void* workspace, size_t workspace_bytes, void* stream);
int tribe_encoder_extend_slots_fwd(const tribe_encoder_desc* d, float* x, void* y, int32_t y_dtype, uint16_t* k_cache, uint16_t* v_cache,
                                   int64_t cap, const int32_t* pos, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * a16-a18: building blocks of the frozen extractors (HF transformers architectures)
 * ------------------------------------------------------------------------- */
/* x[i, :] = table[ids[i], :]  (nn.Embedding; table f32 or bf16 -> x f32) */
int tribe_embedding_fwd(const void* table, int32_t table_dtype, const int64_t* ids, int64_t n, int64_t dim, int64_t vocab,
                        float* x, void* stream);
/* LlamaRMSNorm (modeling_llama.py:51-66): y = x * rsqrt(mean(x^2) + eps) * w */
int tribe_rmsnorm_fwd(const float* x, int64_t rows, int64_t dim, const float* w, float eps, void* y, int32_t y_dtype,
                      void* stream);
/* nn.LayerNorm over the last axis: y = (x - mean) * rsqrt(var + eps) * w + b */
int tribe_layernorm_fwd(const float* x, int64_t rows, int64_t dim, const float* w, const float* b, float eps, void* y,
                        int32_t y_dtype, void* stream);
/* out[b, :] = mean_{t in [start[b], start[b]+len[b])} x[b*T + t, :]   (text.py:245-254: mean of the last len(word)
 * non-pad positions; video.py:228: mean over all tokens).  x f32 [B*T, dim] -> out f32, row stride ld_out. */
int tribe_segment_mean_fwd(const float* x, int64_t B, int64_t T, int64_t dim, const int64_t* start, const int64_t* len,
                           float* out, int64_t ld_out, void* stream);
/* out[w, :] = mean_{t in [win_start[w], win_start[w]+win_len[w])} x[win_row[w]*T + t, :] for a LIST of W windows: several may name
 * the same sequence, overlap or be equal (the words of nested contexts pooled from one forward).  x f32 [B*T, dim] -> out f32
 * [W, dim], row stride ld_out; win_* are device int64 [W].  A window is clamped into [0, T] (start < 0 -> 0, the end cut to T); one
 * that is empty after clamping, or whose win_row is outside [0, B), gives zeros and reads nothing.  Rows are summed first to last by
 * one lane, divided once and stored once: no atomics and no memset, so two launches on the same input give the same bits. */
int tribe_window_mean_fwd(const float* x, int64_t B, int64_t T, int64_t dim, const int64_t* win_row, const int64_t* win_start,
                          const int64_t* win_len, int64_t W, float* out, int64_t ld_out, void* stream);

/* Conv3d patch embedding with stride == kernel (VJEPA2PatchEmbeddings3D, modeling_vjepa2.py:84-117) as im2col:
 * pixels f32 [B, frames, chans, H, W] -> bf16 [B * tokens, K_pad], K = chans*tubelet*patch*patch in Conv3d weight order */
int tribe_im2col3d_fwd(const float* pixels, int64_t B, int32_t frames, int32_t chans, int32_t height, int32_t width,
                       int32_t tubelet, int32_t patch, uint16_t* out, int64_t K_pad, void* stream);

typedef struct tribe_vit_layer {
  const float* norm1_w; const float* norm1_b;
  const uint16_t* w_qkv; const float* b_qkv;   /* bf16 [3*dim, dim] rows q | k | v, f32 [3*dim] */
  const uint16_t* w_proj; const float* b_proj; /* bf16 [dim, dim] */
  const float* norm2_w; const float* norm2_b;
  const uint16_t* w_fc1; const float* b_fc1;   /* bf16 [mlp, dim] */
  const uint16_t* w_fc2; const float* b_fc2;   /* bf16 [dim, mlp] */
} tribe_vit_layer;

/* fp8 variant of a ViT layer's four Linear weights (see tribe_llama_fp8_layer): i = 0 qkv, 1 proj, 2 fc1, 3 fc2 */
typedef struct tribe_vit_fp8_layer {
  const uint8_t* w_qkv; const uint8_t* w_proj; const uint8_t* w_fc1; const uint8_t* w_fc2;
  float w_scale[4];
  float in_scale[4];
} tribe_vit_fp8_layer;

typedef struct tribe_vjepa2_desc {
  int64_t B;                                   /* clips */
  int32_t frames, chans, height, width, tubelet, patch;
  int32_t dim, depth, heads, dim_head, mlp;
  float ln_eps;
  const uint16_t* w_patch; const float* b_patch; int64_t K_pad;  /* bf16 [dim, K_pad] */
  const tribe_vit_layer* layers_host;          /* HOST array [depth] */
  const float* cos_tab; const float* sin_tab;  /* f32 [tokens, dim_head] per-element 3-D rope tables */
  const float* pixels;                         /* f32 [B, frames, chans, H, W] (output of the HF video processor) */
  const tribe_vit_fp8_layer* fp8_host;         /* HOST array [depth] or NULL: e4m3 GEMMs (dim and mlp multiples of 128) */
  float* amax_out;                             /* device f32 [depth, 4] or NULL: calibration of the bf16 path (max-accumulated) */
} tribe_vjepa2_desc;

size_t tribe_vjepa2_workspace_bytes(const tribe_vjepa2_desc* d);
/* VJEPA2Model encoder forward with output_hidden_states (video.py:247-274), fused with the token mean of
 * video.py:228: states f32 [depth + 1, B, dim] (state 0 = patch embeddings, state l = output of layer l). */
int tribe_vjepa2_fwd(const tribe_vjepa2_desc* d, float* states, void* workspace, size_t workspace_bytes, void* stream);

/* causal depthwise Conv1d over time (left pad K-1, no bias) + LayerNorm over channels + swish
 * (Wav2Vec2BertConvolutionModule, modeling_wav2vec2_bert.py:214-222).  x, y bf16 [B*T, C]; w_kc f32 [K, C] (tap-major). */
int tribe_dwconv_ln_swish_fwd(const uint16_t* x, int64_t B, int64_t T, int32_t C, int32_t K, const float* w_kc,
                              const float* ln_w, const float* ln_b, float eps, uint16_t* y, void* stream);
/* out[b, i, :] = x[b*T + idx[i], :]  (nearest-neighbour F.interpolate along time, audio.py:163-171) */
int tribe_gather_rows_fwd(const float* x, int64_t B, int64_t T, int64_t dim, const int64_t* idx, int64_t n, float* out,
                          void* stream);

typedef struct tribe_conformer_layer {
  const float* ffn1_ln_w; const float* ffn1_ln_b;
  const uint16_t* w_ffn1_in; const float* b_ffn1_in;     /* bf16 [inter, dim] */
  const uint16_t* w_ffn1_out; const float* b_ffn1_out_half; /* bf16 [dim, inter]; bias pre-multiplied by 0.5 */
  const float* attn_ln_w; const float* attn_ln_b;
  const uint16_t* w_qkv; const float* b_qkv;             /* bf16 [3*dim, dim] */
  const uint16_t* dist_emb;                              /* bf16 [left + right + 1, dim_head] */
  const uint16_t* w_attn_out; const float* b_attn_out;   /* bf16 [dim, dim] */
  const float* conv_ln_w; const float* conv_ln_b;
  const uint16_t* w_pw1;                                 /* bf16 [2*dim, dim], rows interleaved (a_0, b_0, a_1, b_1, ...) for the GLU epilogue */
  const float* w_dw_kc;                                  /* f32 [K, dim] depthwise taps, tap-major */
  const float* dw_ln_w; const float* dw_ln_b;
  const uint16_t* w_pw2;                                 /* bf16 [dim, dim] */
  const float* ffn2_ln_w; const float* ffn2_ln_b;
  const uint16_t* w_ffn2_in; const float* b_ffn2_in;
  const uint16_t* w_ffn2_out; const float* b_ffn2_out_half;
  const float* final_ln_w; const float* final_ln_b;
} tribe_conformer_layer;

/* fp8 variant of a Conformer layer's four feed-forward weights (see tribe_llama_fp8_layer): i = 0 ffn1.intermediate_dense, 1 ffn1.output_dense,
 * 2 ffn2.intermediate_dense, 3 ffn2.output_dense -- 70 % of the layer's GEMM flops; the attention and convolution-module projections stay bf16 */
typedef struct tribe_conformer_fp8_layer {
  const uint8_t* w_ffn1_in; const uint8_t* w_ffn1_out; const uint8_t* w_ffn2_in; const uint8_t* w_ffn2_out;
  float w_scale[4];
  float in_scale[4];
} tribe_conformer_fp8_layer;

typedef struct tribe_w2vbert_desc {
  int64_t B, T;                       /* chunks x frames (no padding mask: the reference passes single unpadded chunks) */
  int32_t feat_dim, feat_pad;         /* 160, padded to a multiple of 64 */
  int32_t dim, depth, heads, dim_head, inter, conv_kernel, rel_left, rel_right;
  float ln_eps;
  const float* fp_ln_w; const float* fp_ln_b;            /* feature_projection.layer_norm */
  const uint16_t* w_fp; const float* b_fp;               /* bf16 [dim, feat_pad] */
  const tribe_conformer_layer* layers_host;              /* HOST array [depth] */
  const float* features;              /* f32 [B*T, feat_dim] (output of the HF SeamlessM4T feature extractor) */
  const int64_t* out_index; int64_t n_out;               /* frame index of every output time point (nearest interpolation) */
  const tribe_conformer_fp8_layer* fp8_host;             /* HOST array [depth] or NULL: e4m3 feed-forward GEMMs (BASELINE config 5) */
  float* amax_out;                                       /* device f32 [depth, 4] or NULL: calibration of the bf16 path (max-accumulated) */
} tribe_w2vbert_desc;

size_t tribe_w2vbert_workspace_bytes(const tribe_w2vbert_desc* d);
/* Wav2Vec2BertModel forward with output_hidden_states (audio.py:253-263) fused with the nearest-neighbour resampling
 * to 2 Hz (audio.py:163-171): states f32 [depth + 1, B, n_out, dim]. */
int tribe_w2vbert_fwd(const tribe_w2vbert_desc* d, float* states, void* workspace, size_t workspace_bytes, void* stream);

typedef struct tribe_llama_layer {
  const float* input_norm_w;     /* [dim] */
  const uint16_t* w_qkv;         /* bf16 [(hq + 2 hkv) * dh, dim]: q | k | v rows */
  const uint16_t* w_o;           /* bf16 [dim, hq * dh] */
  const float* post_norm_w;      /* [dim] */
  const uint16_t* w_gate_up;     /* bf16 [2 * inter, dim], rows interleaved: gate_0, up_0, gate_1, up_1, ... */
  const uint16_t* w_down;        /* bf16 [dim, inter] */
} tribe_llama_layer;

/* fp8 variant of a layer's four Linear weights (BASELINE config 5): e4m3 bytes in the same row order as the bf16 packs,
 * per-tensor scales w_scale[i] (weight = byte value * scale) and static per-tensor input scales in_scale[i] for the
 * four GEMM inputs, i = 0 qkv (normed x), 1 o_proj (attention output), 2 gate_up (normed x), 3 down (SwiGLU output). */
typedef struct tribe_llama_fp8_layer {
  const uint8_t* w_qkv; const uint8_t* w_o; const uint8_t* w_gate_up; const uint8_t* w_down;
  float w_scale[4];
  float in_scale[4];
} tribe_llama_fp8_layer;

typedef struct tribe_llama_desc {
  int64_t B, T;                  /* right-padded batch of token ids */
  int32_t dim, depth, heads_q, heads_kv, dim_head, inter;
  float rms_eps;
  const void* embed; int32_t embed_dtype; int64_t vocab;
  const tribe_llama_layer* layers_host;   /* HOST array [depth] */
  const float* final_norm_w;
  const float* cos_tab; const float* sin_tab;   /* f32 [T, dim_head/2] (rope scaling already applied) */
  const int64_t* ids;            /* [B*T] */
  const int64_t* pool_start; const int64_t* pool_len;  /* [B] token window averaged per hidden state */
  const tribe_llama_fp8_layer* fp8_host;  /* HOST array [depth] or NULL: run the four Linear GEMMs of every layer in fp8
                                             (needs dim, heads_q * dim_head and inter to be multiples of 128) */
  float* amax_out;               /* device f32 [depth, 4] or NULL: max |input| of the four GEMMs per layer (calibration run
                                    of the bf16 path; accumulated with max, zero it first) */
} tribe_llama_desc;

size_t tribe_llama_workspace_bytes(const tribe_llama_desc* d);
/* LlamaModel forward with output_hidden_states (text.py:236-240) fused with the per-word pooling of
 * text.py:245-254: states f32 [depth + 1, B, dim] (state 0 = embeddings, last = after the final RMSNorm). */
int tribe_llama_fwd(const tribe_llama_desc* d, float* states, void* workspace, size_t workspace_bytes, void* stream);

size_t tribe_llama_windows_workspace_bytes(const tribe_llama_desc* d);
/* The same forward (embedding, layers, final RMSNorm, bf16 or fp8 route, amax_out calibration) pooled over a LIST of W windows
 * instead of one window per row: window w is positions [win_start[w], win_start[w] + win_len[w]) of row win_row[w] (device int64
 * [W], semantics of tribe_window_mean_fwd); states f32 [depth + 1, W, dim].  d->pool_start and d->pool_len are ignored and may be
 * NULL.  With a causal mask and right padding the state at position t depends on tokens 0..t only, so ONE row holding the longest
 * of a run of nested contexts (each a prefix of the next) serves every word of the run -- as long as the contexts nest. */
int tribe_llama_windows_fwd(const tribe_llama_desc* d, const int64_t* win_row, const int64_t* win_start, const int64_t* win_len,
                            int64_t W, float* states, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------- *
 * a7 + a8: SubjectLayers.forward (common.py:45-67) and AdaptiveAvgPool1d (model.py:119-120)
 *   y[b, v, t] = sum_c x[b, t, c] * w[subj[b], c, v] + bias[subj[b], v]
 * x bf16 [B, T, C_pad]; w_packed from tribe_pack_subject_weights; y f32 [B, V, T].
 * subjects: int64 [B] device; every entry must be < S (checked by the host wrapper,
 * mirroring the assert at common.py:53-55).
 * ------------------------------------------------------------------------- */
int tribe_voxel_head_fwd(const uint16_t* x, int64_t B, int64_t T, int64_t C_pad,
                         const uint16_t* w_packed, int64_t S, int64_t V, int64_t V_pad,
                         const float* bias /*[S, V] or NULL*/, const int64_t* subjects,
                         float* y, void* stream);
int tribe_adaptive_avg_pool_fwd(const float* x, int64_t rows, int64_t T_in, float* y, int64_t T_out, void* stream);

/* ------------------------------------------------------------------------- *
 * a10-a14: loss and per-voxel Pearson on [B, V, T'] predictions / targets
 * (pl_module.py:54-56 flattens "b d t -> (b t) d"; the reductions below are
 * order-independent so the flatten is never materialised).
 * ------------------------------------------------------------------------- */
/* nn.MSELoss(): out[0] = mean((pred-true)^2) over all elements (f32 scalar).  The (TRIBE_LOSS_MSE, TRIBE_REDUCE_MEAN) instance of
 * tribe_elem_loss_fwd below (the same kernels, the same bits, the same workspace size) behind this entry point's own contract: pred and
 * truth 16-byte aligned. */
int tribe_mse_fwd(const float* pred, const float* truth, int64_t n, float* out,
                  void* workspace, size_t workspace_bytes, void* stream);
size_t tribe_mse_workspace_bytes(int64_t n);
/* nn.L1Loss / nn.SmoothL1Loss(beta) / nn.HuberLoss(delta) / nn.MSELoss over all n elements of two flat f32 streams (the default
 * loss and those of the run_ensemble.py grid).  With d = pred - true:
 *   L1: |d|;  Huber: m (|d| - m / 2), m = min(|d|, delta);  SmoothL1: Huber(beta) / beta, and L1 for beta == 0;  MSE: d^2.
 * param = beta (SmoothL1, >= 0) or delta (Huber, > 0), ignored otherwise.  out[0] = (float)(sum * num / den) in f64, num = 1 / beta
 * (SmoothL1) | 1, den = n (mean) | 1 (sum); the partial sums are
 * added in a fixed order, so equal inputs give equal bits.  Pointers need 4-byte alignment only (16-byte aligned ones stream float4). */
enum tribe_loss_kind { TRIBE_LOSS_L1 = 0, TRIBE_LOSS_SMOOTH_L1 = 1, TRIBE_LOSS_HUBER = 2, TRIBE_LOSS_MSE = 3 };
enum tribe_loss_reduction { TRIBE_REDUCE_MEAN = 0, TRIBE_REDUCE_SUM = 1 };
int tribe_elem_loss_fwd(const float* pred, const float* truth, int64_t n, int32_t kind, float param, int32_t reduction, float* out,
                        void* workspace, size_t workspace_bytes, void* stream);
size_t tribe_elem_loss_workspace_bytes(int64_t n);
/* accumulate f64 sufficient statistics per (group, voxel):
 *   stats[g][v][0..5] += {sum x, sum y, sum x^2, sum y^2, sum xy, count}
 * x = pred, y = true, over rows b with group[b] == g (group == NULL: all rows -> g = 0) and all t.
 * metrics/base.py:26-29,52-78 (MultidimPearsonCorrCoef / GroupedMetric) and main.py:459-477. */
int tribe_pearson_stats_update(const float* pred, const float* truth, int64_t B, int64_t V, int64_t T,
                               int64_t sb, int64_t sv, int64_t st, /* element strides of b, v, t ([B,V,T] contiguous: V*T, T, 1) */
                               const int64_t* group, int64_t n_groups, double* stats, void* stream);
/* r[g][v] from stats (f32 out); count < 2 or zero variance -> NaN (scipy/torchmetrics behaviour) */
int tribe_pearson_from_stats(const double* stats, int64_t n_groups, int64_t V, float* r, void* stream);
/* PearsonLoss (losses.py:17-42) over the flattened [(B T'), V] view: out[0] = mean|sum_v (1 - r_v), eps 1e-8 */
int tribe_pearson_loss_fwd(const float* pred, const float* truth, int64_t B, int64_t V, int64_t T,
                           int64_t sb, int64_t sv, int64_t st,
                           int32_t reduction_sum, float* out, void* workspace, size_t workspace_bytes, void* stream);
size_t tribe_pearson_loss_workspace_bytes(int64_t V);
/* Retrieval metrics Rank / TopkAcc (modeling_utils/metrics/metrics.py:66-218, fed by pl_module.py:98-99).  No workspace.
 * prep: x (and y, same shape and strides, or NULL) are strided [N, V, T] f32 views; per row n and tensor:
 *   *_mean[n][v] = mean_t in[n][v][t] ([N, V] contiguous; NULL: not written),
 *   *_norm[n]    = || mean row n ||_2 (NULL: not computed).  T = 1 with (sn, sv) = (ld, 1) reads a plain [N, V] matrix. */
int tribe_retrieval_prep(const float* x, const float* y, int64_t N, int64_t V, int64_t T, int64_t sn, int64_t sv, int64_t st,
                         float* x_mean, float* y_mean, float* x_norm, float* y_norm, void* stream);
/* ranks[n] of query x[n] among gallery rows y[0..M) (rows ld elements apart), s[n][m] = dot(x_n, y_m) / (1e-15 + y_norm[m]):
 * rank = (#{m: s > s[n][t(n)]} + #{m: s >= s[n][t(n)]} - 1) / 2, t(n) = true_idx[n] (NULL: t(n) = n, needs N == M);
 * rank < 0 (NaN true score) -> N / 2; relative != 0 -> rank / M; t(n) outside [0, M) -> NaN.  No [N, M] buffer is formed. */
int tribe_retrieval_ranks(const float* x, int64_t ldx, const float* y, int64_t ldy, const float* y_norm, int64_t N, int64_t M,
                          int64_t V, const int64_t* true_idx, int32_t relative, float* ranks, void* stream);
/* scores[N][M] = dot(x_n, y_m) * f (Rank._compute_sim): norm_kind 0 none (f = 1), 1 "x" 1/(1e-15 + x_norm[n]),
 * 2 "y" 1/(1e-15 + y_norm[m]), 3 "xy" 1/(1e-15 + x_norm[n] y_norm[m]).  Diagnostic; "y" scores equal the ones ranks compares. */
int tribe_retrieval_scores(const float* x, int64_t ldx, const float* y, int64_t ldy, int64_t N, int64_t M, int64_t V,
                           const float* x_norm, const float* y_norm, int32_t norm_kind, float* scores, void* stream);
/* out[0..4) = {mean, unbiased std, lower median, mean(ranks < topk)} of ranks[0..n) (ranks >= 0), one launch */
int tribe_rank_reduce(const float* ranks, int64_t n, float topk, float* out, void* stream);
/* Regression metrics MeanSquaredError / MeanAbsoluteError / R2Score / ExplainedVariance (modeling_utils/metrics/regression.py), plain
 * and per group.  No workspace.  stats_update takes the arguments of tribe_pearson_stats_update and accumulates, with d = true - pred
 * formed in f64:   stats[g][v][0..5] += {sum d, sum d^2, sum |d|, sum t, sum t^2, count}
 * (direct residual sums: the Pearson moments cancel for a prediction that follows its target on an offset, and hold no sum |d|). */
int tribe_regression_stats_update(const float* pred, const float* truth, int64_t B, int64_t V, int64_t T,
                                  int64_t sb, int64_t sv, int64_t st, const int64_t* group, int64_t n_groups, double* stats,
                                  void* stream);
enum tribe_regression_kind {
  TRIBE_REGRESSION_MSE = 0, TRIBE_REGRESSION_RMSE = 1, TRIBE_REGRESSION_MAE = 2, TRIBE_REGRESSION_R2 = 3,
  TRIBE_REGRESSION_EXPLAINED_VARIANCE = 4
};
enum tribe_regression_mode { TRIBE_REGRESSION_POOLED = 0, TRIBE_REGRESSION_UNIFORM_AVERAGE = 1, TRIBE_REGRESSION_VARIANCE_WEIGHTED = 2 };
/* out[g][v] (f32, computed in f64 and rounded once) with n = count, rss = sum d^2, tss = sum t^2 - (sum t)^2 / n and
 * vres = sum d^2 - (sum d)^2 / n, each centred sum 0 when within n ulps of its raw sum of squares (as the Pearson finaliser):
 *   mse rss / n;  rmse sqrt(mse);  mae sum |d| / n;  r2 1 - rss / tss;  explained_variance 1 - vres / tss.
 * tss == 0: 1 when the numerator is 0, else 0 (scikit-learn's force_finite).  n == 0: NaN; r2 with n < 2: NaN. */
int tribe_regression_from_stats(const double* stats, int64_t n_groups, int64_t V, int32_t kind, float* out, void* stream);
/* out[g] (f64), one workgroup per group, sums added in a fixed order (equal stats give equal bits):
 *   pooled (mse, rmse, mae only): sum_v rss / sum_v n (then sqrt), sum_v sum |d| / sum_v n;
 *   uniform_average: mean_v score_v;  variance_weighted: sum_v tss_v score_v / sum_v tss_v, the uniform average when every tss_v is 0. */
int tribe_regression_reduce(const double* stats, int64_t n_groups, int64_t V, int32_t kind, int32_t mode, double* out, void* stream);
/* Spearman rank correlation per output column (modeling_utils/metrics/rank_corr.py: MultidimSpearmanCorrCoef), csrc/rank_corr.hip.
 * The sample state is pred_state / truth_state f32 [n_groups][V][capacity]: one contiguous run of samples per (group, column), of
 * which counts[g] (int64, on the device) are filled.
 * append: pred / truth are strided [B, V, T] views (the arguments of tribe_pearson_stats_update); the T samples of batch row b go
 *   behind the samples of group[b] (NULL: group 0) in batch order, and counts[group[b]] += T.  positions: int64 [B] scratch.  A row
 *   whose group lies outside [0, n_groups) or whose run would pass `capacity` is dropped: the caller, who knows how many rows it
 *   has appended, keeps capacity at or above that.  No host synchronisation. */
int tribe_rank_append(const float* pred, const float* truth, int64_t B, int64_t V, int64_t T, int64_t sb, int64_t sv, int64_t st,
                      const int64_t* group, int64_t n_groups, int64_t capacity, int64_t* counts, int64_t* positions,
                      float* pred_state, float* truth_state, void* stream);
/* Column v holds the n samples pred[v * ld .. + n) / truth[v * ld .. + n), 1 <= n <= tribe_spearman_max_samples() = 2^20.  With
 * a_i = #{x_j < x_i} + #{x_j <= x_i} - n (= 2 * average rank - (n + 1); -0.0 ties with +0.0, the infinities are ordinary values)
 * of the predictions and b_i of the targets:
 *   sums[v][0..3) = {sum a_i b_i, sum a_i^2, sum b_i^2}   (int64: exact, bit-reproducible)
 *   rho[v] = sums[0] / sqrt((double)sums[1] * (double)sums[2]) clamped to [-1, 1], rounded once to f32; NaN for n < 2, a constant
 *            column or a NaN among the column's samples (its sums are then 0)
 *   rank_pred / rank_truth (NULL: not written): the average ranks (1-based) f32 [V][n]; NaN in a column with a NaN.
 * chunk <= 0: tribe_spearman_default_chunk(); else a power of two in [64, default].  n <= chunk: one workgroup sorts and ranks a column
 * in LDS (no workspace).  n > chunk: chunks sorted in LDS, merged pairwise through `workspace`
 * (tribe_spearman_workspace_bytes(n, V, chunk); columns are taken in rounds, so it does not grow with V), ranked by binary search. */
int tribe_spearman_columns(const float* pred, const float* truth, int64_t ld, int64_t n, int64_t V, int64_t chunk, float* rho,
                           int64_t* sums, float* rank_pred, float* rank_truth, void* workspace, size_t workspace_bytes, void* stream);
size_t tribe_spearman_workspace_bytes(int64_t n, int64_t V, int64_t chunk);
int64_t tribe_spearman_default_chunk(void);
int64_t tribe_spearman_max_samples(void);
/* Block bootstrap of the per-parcel Pearson r (modeling_utils/metrics/bootstrap.py: BootstrapPearsonCorrCoef), csrc/bootstrap.hip.
 * counts: int32 [n_boot][n_sel], how often replicate r draws each of n_sel blocks.  Draw k of replicate r is word k & 3 of
 *   Philox4x32-10 with counter (k >> 2, r, 0, 0) and key (seed & 0xffffffff, seed >> 32), mapped to (u * n_sel) >> 32 (64-bit
 *   product, no rejection step: the bias is below n_sel / 2^32).  1 <= n_boot <= 16384, 1 <= n_sel <= 32768. */
int tribe_bootstrap_counts(uint64_t seed, int64_t n_boot, int64_t n_sel, int32_t* counts, void* stream);
/* stats: f64 [n_blocks][V][6] block statistics (the state of tribe_pearson_stats_update, one group per block); blocks: int64 [n_sel]
 * (device), the blocks that are resampled, each in [0, n_blocks) (one outside makes every result NaN).  For r < n_boot and parcel v:
 *   S = sum_j counts[r][j] * stats[blocks[j]][v][0..6), f64, j ascending;  r[r * ld + v] = tribe_pearson_from_stats' rule on S
 * and row n_boot takes every count as 1 (the observed r): r is f32 [n_boot + 1][ld], ld >= V.  n_boot == 0 (counts may be NULL)
 * gives the observed row alone.  mean[row * mean_stride] = the mean over v of the row's f32 results, summed in f64 in a fixed order
 * and rounded once (NaN when a parcel is NaN).  No floating-point atomics: equal inputs give equal bits. */
int tribe_bootstrap_pearson(const double* stats, int64_t n_blocks, int64_t V, const int64_t* blocks, int64_t n_sel,
                            const int32_t* counts, int64_t n_boot, float* r, int64_t ld, float* mean, int64_t mean_stride, void* stream);
/* Per column c of replicates f32 [n][ld] (c < C <= ld, 1 <= n <= 16384), over its m non-NaN values sorted ascending (s):
 *   quantile_values[k * C + c] = s[i] + (h - i) (s[min(i + 1, m - 1)] - s[i]), h = (m - 1) quantiles[k], i = floor(h)  (numpy's "linear";
 *     f64, rounded once; quantiles: f64 [n_q] on the device, each in [0, 1]; NaN for m = 0)
 *   std[c] = sqrt(sum (s - mean)^2 / (m - 1)) (two passes, f64; NaN for m < 2);  n_le[c] = #{s <= 0}, n_ge[c] = #{s >= 0}, n_valid[c] = m. */
int tribe_bootstrap_summary(const float* replicates, int64_t n, int64_t C, int64_t ld, const double* quantiles, int64_t n_q,
                            float* quantile_values, float* std, int32_t* n_le, int32_t* n_ge, int32_t* n_valid, void* stream);

/* ------------------------------------------------------------------------- *
 * Backward building blocks (pl_module.training_step: loss.backward() of the path).
 * Composition lives in the host-side autograd functions (modeling_utils/autograd.py).
 * ------------------------------------------------------------------------- */
/* out[z, c, r] = in[z, r, c] as bf16, rows of `out` zero-padded to R_pad; `in` is f32 or bf16 with element strides
 * (s_z, s_r, 1).  Used for the transposed operands of the weight-gradient GEMMs and of attention backward. */
int tribe_transpose_bf16(const void* in, int32_t in_dtype, int64_t Z, int64_t R, int64_t C, int64_t s_z, int64_t s_r,
                         uint16_t* out, int64_t so_z, int64_t R_pad, void* stream);
/* the same with two batch levels (z = z1 * Z0 + z0 reads in + z1 * s_z1 + z0 * s_z0; out batch z contiguous at so_z):
 * all (batch, head) slices of a fused [B*T, heads*dim] activation in one launch */
int tribe_transpose_bf16_b2(const void* in, int32_t in_dtype, int64_t Z1, int64_t Z0, int64_t R, int64_t C, int64_t s_z1, int64_t s_z0,
                            int64_t s_r, uint16_t* out, int64_t so_z, int64_t R_pad, void* stream);
/* out[n] (+)= sum_m a[m, n] * (b ? b[m, n] : 1)   (bias, residual_scale and positional-embedding gradients) */
int tribe_colsum_fwd(const void* a, int32_t a_dtype, const float* b, int64_t M, int64_t N, int64_t ld, float* out,
                     int32_t accumulate, void* stream);
/* ScaleNorm backward: y = x * s / max(||x||, eps), s = gain_scale * g.
 *   dx[m, :] = (dres ? dres[m, :] * (rs ? rs : 1) : 0) + s / ||x|| * (dy - xhat * <xhat, dy>);   dg += gain_scale * sum_m <xhat, dy>
 * dy bf16 or f32 [M, dim]; dres / dx f32 (may alias). */
int tribe_scalenorm_bwd(const float* x, const void* dy, int32_t dy_dtype, const float* g, float gain_scale, float eps,
                        int64_t rows, int64_t dim, const float* dres, const float* rs, float* dx, float* dg, void* stream);
/* The same with a reproducible gain gradient: every row's term gain_scale * <xhat, dy> is staged in dg_rows (f32 [rows]) and a second launch
 * WRITES dg[0] = their sum in a fixed order (f64, rounded once) -- no atomics, equal inputs give equal bits.  dg and dg_rows are required. */
int tribe_scalenorm_bwd_ordered(const float* x, const void* dy, int32_t dy_dtype, const float* g, float gain_scale, float eps, int64_t rows,
                                int64_t dim, const float* dres, const float* rs, float* dx, float* dg, float* dg_rows, void* stream);
/* dS = P * (dP - rowsum(P * dP)) * scale   (softmax backward; P bf16, dP f32, dS bf16; row strides ld_p, ld_dp, ld_ds;
 * columns >= T of dS are zero-filled up to T_pad) */
int tribe_softmax_bwd(const uint16_t* P, const float* dP, int64_t rows, int64_t T, int64_t T_pad, int64_t ld_p, int64_t ld_dp,
                      float scale, uint16_t* dS, int64_t ld_ds, void* stream);
/* row softmax used by the materialised attention of the training path: S f32 [rows, T] -> P bf16 [rows, T_pad] */
int tribe_softmax_fwd(const float* S, int64_t rows, int64_t T, int64_t ld_s, uint16_t* P, int64_t T_pad, int64_t ld_p, void* stream);
/* d pred = gscale[0] * 2 / n * (pred - true)   (nn.MSELoss backward): tribe_elem_loss_bwd's (TRIBE_LOSS_MSE, TRIBE_REDUCE_MEAN) instance; any
 * pointer that is not 16-byte aligned selects the scalar form */
int tribe_mse_bwd(const float* pred, const float* truth, int64_t n, const float* gscale, float* dpred, void* stream);
/* d pred = gscale[0] * num / den * slope(d), the gradient of tribe_elem_loss_fwd: the factor is formed in f32 from left to right, den = n
 * (mean) | 1 (sum), num = 1 / beta (SmoothL1) | 2 (MSE) | 1;  slope: L1 sign(d) (0 at d == 0), Huber clamp(d, -delta, delta), SmoothL1
 * clamp(d, -beta, beta), MSE d.  gscale is a device scalar. */
int tribe_elem_loss_bwd(const float* pred, const float* truth, int64_t n, int32_t kind, float param, int32_t reduction,
                        const float* gscale, float* dpred, void* stream);
/* adaptive average pool backward: dx[r, t] = sum_{i: t in window i} dy[r, i] / |window i| */
int tribe_adaptive_avg_pool_bwd(const float* dy, int64_t rows, int64_t T_in, int64_t T_out, float* dx, void* stream);
/* out[idx[b], v] += sum_t x[b, v, t]   (SubjectLayers bias gradient) */
int tribe_rowsum_scatter(const float* x, int64_t B, int64_t V, int64_t T, const int64_t* idx, float* out, void* stream);
/* One pass over a gradient dy = a f32 [M, N] (row stride ld): sum_a[n] = sum_m a[m, n] (bias gradient), sum_ab[n] = sum_m a[m, n] b[m, n]
 * (res_scale gradient: b = the residual input), a_bf16 = bf16(a) with row stride ld_bf16 (the GEMM operand of dgrad / wgrad).  Any of the
 * three outputs may be NULL; N % 4 == 0.  Replaces `grad.sum(0)`, `(grad * res).sum(0)` and the cast of autograd's Linear backward. */
int tribe_colsum_cast_fwd(const float* a, const float* b, int64_t M, int64_t N, int64_t ld, float* sum_a, float* sum_ab, uint16_t* a_bf16,
                          int64_t ld_bf16, void* stream);
/* dst[idx[b], :] += src[b, :] for b = 0 .. B-1 in that order (deterministic; no atomics): src f32 [B, n], dst f32 [S, n], n % 4 == 0.
 * SubjectLayers weight gradient: the per-sample products x_b^T dy_b of one batched GEMM summed into their subject's slab
 * (modeling_utils/models/common.py:60-76 is the forward it differentiates). */
int tribe_slab_scatter_sum(const float* src, int64_t B, int64_t n, const int64_t* idx, float* dst, void* stream);
/* y = x * rs (columns), f32 [M, N]; rs NULL = copy */
int tribe_scale_cols_fwd(const float* x, const float* rs, int64_t M, int64_t N, float* y, void* stream);
/* PearsonLoss backward (losses.py:17-42) on [B, V, T] views (element strides sb, sv, st shared by pred / true / dpred
 * which is contiguous [B, V, T]): stats f64 [V, 6] as produced by tribe_pearson_stats_update (one group);
 * dpred = gscale[0] * w * d(1 - r_v)/d pred,  w = 1/V (mean) or 1 (sum). */
int tribe_pearson_loss_bwd(const float* pred, const float* truth, int64_t B, int64_t V, int64_t T, int64_t sb, int64_t sv,
                           int64_t st, const double* stats, int32_t reduction_sum, const float* gscale, float* dpred, void* stream);
/* InfoNCE pieces (model.py:208-221): lse[r] = log sum_j exp(S[r, j]) and diag[r] = S[r, r] of a square f32 matrix;
 * dL[i, j] = gscale[0] * 0.5 / N * (exp(S[i,j] - lse_r[i]) + exp(S[i,j] - lse_c[j]) - 2 [i == j])  as bf16 [N, N_pad] */
int tribe_lse_rows_fwd(const float* S, int64_t N, int64_t ld, float* lse, float* diag, void* stream);
int tribe_infonce_dlogits(const float* S, int64_t N, int64_t ld, const float* lse_r, const float* lse_c, const float* gscale,
                          uint16_t* dL, int64_t N_pad, void* stream);
/* f32 -> bf16 elementwise (gradient casts) */
int tribe_cast_bf16_fwd(const float* x, int64_t n, uint16_t* y, void* stream);

/* ---- segment assembly from HBM-resident extractor outputs --------------------------------
 * Replaces the host-side numpy assembly of a segment's feature tensor: `_aggregate_layers`
 * (data_utils/features/text.py:129-149, audio.py:174-194, video.py:147-167), `TimedArray.overlap` / `__iadd__`
 * (data_utils/base.py:130-211) driven by the feature `__call__`s (text.py:85-124, audio.py:78-120, neuro.py:60-106),
 * plus the fp32 H2D copy and the "b (l d) t -> b t (l d)" transpose of model.py:146-155.  The index decisions
 * (rounding, clamping) stay on the host (data_utils/base.py of this build); these kernels move the bytes. */

/* one time slice of a cached, layer-aggregated array that lands in a segment's output (32 bytes, device memory) */
typedef struct tribe_feature_piece {
  const float* src;   /* device pointer to an f32 [C, ld] array: channel c starts at src + c * ld              */
  int64_t ld;         /* samples per channel row                                                               */
  int32_t src_first;  /* first source sample                                                                   */
  int32_t src_count;  /* == dst_count, or 1 = that one sample is broadcast over the destination run            */
  int32_t dst_first;  /* first destination step (0 <= dst_first, dst_first + dst_count <= T)                   */
  int32_t dst_count;  /* destination run length                                                                */
} tribe_feature_piece;

/* out[b, g, i] = mean over s in [lo[g], hi[g]) of states[b, s, i]  (f32; sequential adds in layer order, one divide:
 * bit-identical to numpy's latents[l1:l2].mean(0)); groups of one select single layers (layer_aggregation = None).
 * states [batch, n_states, plane], out [batch, n_groups, plane]; lo / hi int32 device arrays of n_groups entries. */
int tribe_group_mean_fwd(const float* states, int64_t batch, int64_t n_states, int64_t plane, const int32_t* lo,
                         const int32_t* hi, int32_t n_groups, float* out, void* stream);
/* Sum the pieces of each segment (seg_ptr: int32 [B + 1] CSR offsets into pieces, in the order the reference adds
 * them) into a zero-initialised output:
 *   out_dtype = TRIBE_BF16: packed projector operand, bf16 [B * T, C_pad] rows (time-major, channels contiguous,
 *                           columns >= C zero) -- what tribe_pack_features would have produced from [B, C, T];
 *   out_dtype = TRIBE_F32 : reference layout f32 [B, C, T] (targets such as the fMRI array; C_pad ignored).
 * The caller guarantees src_first + src_count <= ld and the dst bounds above (checked on the host by the binding). */
int tribe_segment_gather_fwd(const tribe_feature_piece* pieces, const int32_t* seg_ptr, int64_t B, int64_t C, int64_t T,
                             void* out, int32_t out_dtype, int64_t C_pad, void* stream);
/* Word features (frequency-0 arrays held for a word's duration, text.py:190-202): out[row] = bf16(sum of
 * table[word_idx[k]] for k in [row_ptr[row], row_ptr[row + 1])), rows = B * T, table f32 [n_words, C],
 * out bf16 [rows, C_pad]; lists keep the segment's event order, so the f32 sum is the reference's sum. */
int tribe_word_bag_fwd(const float* table, int64_t n_words, int64_t C, const int32_t* row_ptr, const int32_t* word_idx,
                       int64_t rows, uint16_t* out, int64_t C_pad, void* stream);
/* Same sums kept in f32, out f32 [rows, C]: the exact tensor a feature plugin's __call__ returns (text.py:85-124,
 * `out += ta` over the segment's words) before any rounding; the plugin transposes it to [C, T] with
 * tribe_transpose_f32_fwd. */
int tribe_word_bag_f32_fwd(const float* table, int64_t n_words, int64_t C, const int32_t* row_ptr, const int32_t* word_idx,
                           int64_t rows, float* out, void* stream);

/* ---- audio front end: 16 kHz waveform -> Wav2Vec-BERT input_features (data_utils/features/audio.py:123-127, 224-234) ----
 * Replaces `_preprocess_wav` (mean over channels, z-score over the chunk with torch's std; only when zscore != 0) and
 * transformers' SeamlessM4TFeatureExtractor at its defaults: * 2^15; frames of 400 samples every 160, F = 1 + (n - 400) / 160;
 * per frame DC removal, pre-emphasis 0.97, `window` f32 [400] (Povey), 512-point one-sided DFT, power; `mel` f32 [257, 80];
 * max(., FLT_EPSILON); log; per mel bin over the chunk's F frames (x - mean) / sqrt(var(ddof = 1) + 1e-7); one zero frame
 * appended when F is odd; pairs of frames stacked: T = ceil(F / 2) rows of 160.
 * wavs_host: B device pointers in a HOST array, chunk b f32 [n_host[b], channels] sample-major; n_host[b] >= 400 (else < 0).
 * out f32 [B, T_max, 160], T_max >= every chunk's T, rows past a chunk's own T zero; lengths_host (optional) int32 [B]
 * receives every T.  At most TRIBE_FBANK_MAX_CHUNKS chunks per call, all in one launch sequence; a chunk's rows do not
 * depend on the rest of the batch, bit for bit.  tribe_fbank_workspace_bytes returns 0 for arguments the forward refuses. */
#define TRIBE_FBANK_MAX_CHUNKS 32
size_t tribe_fbank_workspace_bytes(const int64_t* n_host, int32_t B);
int tribe_fbank_fwd(const float* const* wavs_host, const int64_t* n_host, int32_t B, int32_t channels, int32_t zscore,
                    const float* window, const float* mel, float* out, int64_t T_max, int32_t* lengths_host, void* workspace,
                    size_t workspace_bytes, void* stream);

/* ---- audio front end: native-rate waveform -> 16 kHz (data_utils/features/audio.py:129-138 `julius.resample.ResampleFrac`) ----
 * Replaces the resampler in front of the filterbank with julius' windowed-sinc polyphase filter.  old_sr / new_sr are the REDUCED
 * rates (divided by their gcd; 44100 -> 16000 is 441 / 160), width = W of the filter, K = 2 * width + old_sr taps per phase;
 * `table`: DEVICE f32 [new_sr, K], built on the host in float32 by `data_utils.features.audio.julius_resample_kernels`
 * (zeros = 24, rolloff = 0.945).  For chunk b, channel c, frame f and phase i < new_sr, with j = f * new_sr + i < n_out_host[b]:
 *   out[j, c] = sum_{k < K} table[i, k] * wav[clamp(f * old_sr + k - width, 0, n - 1), c]
 * (julius' replicate padding), one f32 fma chain in k order.  wavs_host / out_host: B device pointers each in HOST arrays, chunk b
 * f32 [n_host[b], channels] -> f32 [n_out_host[b], channels], both sample-major, so out_host can be tribe_fbank_fwd's wavs_host.
 * n_out_host[b] is julius' output length (`resample_output_length`: floor of new_sr * n / old_sr rounded to float32, NOT the
 * integer floor); nothing is written at or past it.  Checked before anything is launched (a violation returns < 0): B in 1 ..
 * TRIBE_RESAMPLE_MAX_CHUNKS; channels >= 1; both rates >= 1, different and coprime; width >= 1; the table at most 64 MiB (44100 ->
 * 16001 would ask for gigabytes); n >= 1; 1 <= n_out <= (n / old_sr + 1) * new_sr, the samples the strided convolution has; no
 * null or misaligned pointer.  Asynchronous, one launch, no workspace, no allocation; a chunk's samples do not depend on the rest
 * of the batch or on the channel count, bit for bit. */
#define TRIBE_RESAMPLE_MAX_CHUNKS 32
int tribe_resample_frac_fwd(const float* const* wavs_host, const int64_t* n_host, int32_t B, int32_t channels, int32_t old_sr,
                            int32_t new_sr, int32_t width, const float* table, float* const* out_host, const int64_t* n_out_host,
                            void* stream);

/* ---- video front end: decoded uint8 frames -> V-JEPA2 pixel_values_videos (data_utils/features/video.py `default_video_processor`) ----
 * Replaces the host processor in front of the ViT: antialiased bilinear resize (torch's `interpolate(mode="bilinear",
 * antialias=True)`: a separable triangle filter) of frames to resized_h x resized_w, a crop window of crop x crop, / 255,
 * (v - mean[c]) / std[c].  Only the crop window is computed.  Along an axis, output position i of the window is
 * sum_k w[i][k] * in[first[i] + k], an f32 fma chain in tap order, W pass first; `data_utils.features.video.aa_resize_taps`
 * builds the tables.  frames: DEVICE uint8 [n_src, H, W, 3], contiguous (no row alignment is assumed).  Everything else
 * that is indexed arrives in HOST arrays and is checked before anything is launched: src_host int32 [n_out], the source frame
 * of every output slot, each in [0, n_src); first_h_host int32 [crop] / w_h_host f32 [crop, taps_h] with 0 <= first and
 * first + taps_h <= H, non-decreasing; first_w_host / w_w_host / taps_w likewise against W; crop <= resized_h, resized_w;
 * mean_host, std_host f32 [3], std > 0; taps_h <= 64 (a tile's input rows are staged through LDS).  A violation returns < 0.
 * The tables are copied into the workspace in-stream; the host arrays may be reused when the call returns.
 * out: DEVICE f32 [n_out, 3, crop, crop] (= [clips, frames, 3, crop, crop] of tribe_vjepa2_fwd's `pixels`).  One launch; a
 * slot's values depend on its source frame only and are the same bits on every call and in every batch.
 * tribe_video_preprocess_workspace_bytes returns 0 for arguments the forward refuses. */
size_t tribe_video_preprocess_workspace_bytes(int64_t n_out, int32_t crop, int32_t taps_h, int32_t taps_w);
int tribe_video_preprocess_fwd(const uint8_t* frames, int64_t n_src, int32_t H, int32_t W, const int32_t* src_host, int64_t n_out,
                               int32_t resized_h, int32_t resized_w, int32_t crop, const int32_t* first_h_host, const float* w_h_host,
                               int32_t taps_h, const int32_t* first_w_host, const float* w_w_host, int32_t taps_w,
                               const float* mean_host, const float* std_host, float* out, void* workspace, size_t workspace_bytes,
                               void* stream);

/* ---- steps after the model ------------------------------------------------------------ */
/* out[z, c, r] = in[z, r, c], f32: predictions [B, V, T'] -> [B, T', V] rows for the submission writer
 * (`pred = y_pred[i].cpu().numpy().T`, algonauts2025/callbacks.py:63-64), one launch + one D2H copy per batch. */
int tribe_transpose_f32_fwd(const float* in, int64_t Z, int64_t R, int64_t C, float* out, void* stream);
/* Ensemble averaging (algonauts2025/grids/average_submissions.py:107-125): out[i] = sum_n preds[n, i] * w, i < M,
 * sequential in n, product and sum rounded separately (numpy's `np.sum(preds * weights, axis=0)`):
 *   w_column f32 [N, V] (per-voxel weights, :96-99): w = w_column[n, i % V], f32 arithmetic, out f32 [M];
 *   w_set    f64 [N]    (score weights,    :100-103): w = w_set[n], f64 arithmetic, out f64 [M].
 * Exactly one of the two is non-NULL.  The unweighted mean (:121) is tribe_group_mean_fwd with one group [0, N). */
int tribe_weighted_sum_fwd(const float* preds, int64_t N, int64_t M, int64_t V, const float* w_column, const double* w_set,
                           void* out, void* stream);
/* corr f64 [N, N] = np.corrcoef of the N rows of x f32 [N, K] (average_submissions.py:38-53; N <= 64): f64 row means,
 * f64 products of the centred rows accumulated per K slice and merged with f64 atomics (order not fixed: agreement
 * with numpy to ~1e-12, not bit-exact). */
size_t tribe_corr_matrix_workspace_bytes(int64_t N);
int tribe_corr_matrix_fwd(const float* x, int64_t N, int64_t K, double* corr, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fp8 (OCP e4m3) GEMM for the frozen extractors (BASELINE config 5: "fp8 MFMA extractor GEMMs") ----------------
 * Same descriptor and epilogue as tribe_gemm_bf16 (the nn.Linear calls of transformers' modeling_llama.py /
 * modeling_vjepa2.py / modeling_wav2vec2_bert.py), but A [M, K] and B [N, K] hold e4m3 bytes (K contiguous; lda / ldb /
 * batch strides in elements = bytes, multiples of 16; K a multiple of 128) and `alpha` carries scale_A * scale_B of the
 * per-tensor quantisation.  v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales, f32 accumulation. */
int tribe_gemm_fp8(const tribe_gemm_desc* d, void* stream);
/* out[m, k] = e4m3(clamp(x[m, k] * inv_scale, -448, 448)) (round to nearest even), x f32 | bf16 [M, K] with row stride ld,
 * out [M, K_pad] bytes, columns K..K_pad zero; K_pad a multiple of 16.  Saturating: +-inf and everything past 448 give +-448.
 * Zeros keep their sign.  A NaN is passed through as the NaN code with its sign (+NaN 0x7F, -NaN 0xFF), never as a finite value. */
int tribe_quantize_fp8_fwd(const void* x, int32_t x_dtype, int64_t M, int64_t K, int64_t ld, float inv_scale, uint8_t* out,
                           int64_t K_pad, void* stream);
/* The pre-norm of an extractor layer fused with the quantisation of the Linear input that follows it (transformers' LlamaRMSNorm /
 * nn.LayerNorm inside modeling_llama.py / modeling_vjepa2.py, then the e4m3 operand): y8 = tribe_quantize_fp8_fwd(bf16 output of
 * tribe_rmsnorm_fwd (layernorm = 0, b NULL) or tribe_layernorm_fwd (layernorm = 1, b may be NULL)), bit for bit, in ONE pass over x
 * (f32 [rows, dim], dim % 16 == 0; y8 [rows, dim] bytes). */
int tribe_norm_quantize_fp8_fwd(const float* x, int64_t rows, int64_t dim, const float* w, const float* b, int32_t layernorm, float eps,
                                float inv_scale, uint8_t* y8, void* stream);
/* out[0] = max(out[0] if accumulate else 0, max |x|)  (device float; calibration of the per-tensor scales).  A NaN anywhere in x, or
 * already in out[0] when accumulating, gives NaN (it orders above inf), so that poisoned activations cannot yield a usable scale. */
int tribe_absmax_fwd(const void* x, int32_t x_dtype, int64_t M, int64_t K, int64_t ld, float* out, int32_t accumulate, void* stream);

/* ---- optimiser step of pl_module.training_step's loop (grids/defaults.py:126-133: torch.optim.Adam, lr 1e-4, wd 0) ----
 * One launch per parameter group: p, m (exp_avg), v (exp_avg_sq) updated in place from g with torch.optim.Adam's
 * arithmetic (decoupled = 1: AdamW).  `step` is the 1-based count used for the bias corrections.  The work list cuts
 * every tensor into chunks of tribe_adam_chunk_elems() elements: chunk c = elements [chunk_start[c], +chunk) of
 * table[chunk_tensor[c]].  All three arrays live in device memory. */
typedef struct tribe_adam_tensor {
  float* p; const float* g; float* m; float* v; int64_t n;
  uint16_t* p_bf16;   /* optional (NULL = none): bf16 copy of the updated parameter, same element order -- the packed GEMM operand of the next
                       * forward, written by the optimiser step instead of a separate cast pass (tribe_adam_step only) */
} tribe_adam_tensor;
int64_t tribe_adam_chunk_elems(void);
int tribe_adam_step(const tribe_adam_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_start, int64_t n_chunks, float lr,
                    float beta1, float beta2, float eps, float weight_decay, int64_t step, int32_t decoupled, void* stream);
/* Running weight average of the reference's StochasticWeightAveraging callback (algonauts2025/main.py:365-373; the averaging rule is
 * torch.optim.swa_utils.AveragedModel's default: avg += (p - avg) * weight with weight = 1 / (n_averaged + 1), weight 1 = copy).
 * Same table and work list as tribe_adam_step: table[i].p = the average (updated in place), table[i].g = the live parameter;
 * m and v are not touched and may be NULL. */
int tribe_swa_update(const tribe_adam_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_start, int64_t n_chunks, float weight,
                     void* stream);
/* ---- gradient clipping in front of the optimiser step (torch.nn.utils.clip_grad_norm_ / clip_grad_value_; Lightning's
 * Trainer(gradient_clip_val, gradient_clip_algorithm)).  Same table and work list as tribe_adam_step.
 *
 * tribe_grad_norm reads table[i].g and table[i].n only (p, m, v, p_bf16 may be NULL).  norm_kind 0: the L2 norm of all gradients taken
 * as one vector; 1: max |g|.  Every element is widened to f64 (its square is then exact), chunk c is reduced to partials[c] (workspace:
 * n_chunks doubles, device memory) and one workgroup reduces those, all in a fixed order without atomics: equal inputs give equal bits.
 * out (two floats, device memory) receives
 *   out[0] = (float)norm                                   the total norm
 *   out[1] = (float)min(1, max_norm / (norm + 1e-6))       torch's clip coefficient, formed in f64 and rounded once
 * A NaN element gives out = {NaN, NaN} for both kinds; an infinite element (and no NaN) gives {inf, 0}; all zeros give {0, 1}.
 * Nothing is copied to the host. */
int tribe_grad_norm(const tribe_adam_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_start, int64_t n_chunks, int32_t norm_kind,
                    double max_norm, double* partials, float* out, void* stream);
/* In place on the gradients: g = clamp(g * coef[0], -clip_value, clip_value).  Reads table[i].g and table[i].n and WRITES through
 * table[i].g.  coef: device pointer (tribe_grad_norm's out + 1) or NULL = 1; clip_value <= 0 = no clamp.  The product is rounded to f32
 * before the clamp; NaN stays NaN (torch.clamp's rule), +-inf clamps to +-clip_value.  With a coefficient of exactly 1 and no clamp
 * nothing is read or written. */
int tribe_grad_scale(const tribe_adam_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_start, int64_t n_chunks, const float* coef,
                     float clip_value, void* stream);
/* tribe_adam_step (all table fields, p_bf16 included) with every gradient replaced, as it is loaded, by tribe_grad_scale's value of it:
 * bit for bit the result of tribe_grad_scale followed by tribe_adam_step, without the 8 B per parameter of the in-place pass and with
 * table[i].g left as it was.  grad_coef: device pointer or NULL = 1; clip_value <= 0 = no clamp.  A NaN coefficient (NaN norm) makes
 * every updated value NaN, as stepping on NaN gradients does. */
int tribe_adam_step_clipped(const tribe_adam_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_start, int64_t n_chunks, float lr,
                            float beta1, float beta2, float eps, float weight_decay, int64_t step, int32_t decoupled, const float* grad_coef,
                            float clip_value, void* stream);

/* ---- hidden block of an MLP (torchvision.ops.MLP layout: Linear -> LayerNorm -> activation), csrc/mlp.hip ----
 * y = act(u),  u = gamma * (z - mean) * rstd + beta  (norm = 1: nn.LayerNorm over the last axis, biased variance, rstd = 1 / sqrt(var + eps))
 *              u = z                                  (norm = 0; gamma, beta, eps ignored)
 * z f32 [rows, dim] with row pitch ld_z; gamma / beta f32 [dim] or NULL (= 1 / 0); act: TRIBE_ACT_NONE, _GELU (erf), _RELU, _ELU.
 * y f32 or bf16 with row pitch ld_y >= dim; columns dim .. ld_y - 1 are written as zeros (the bf16 form is the K-padded operand of the
 * next GEMM).  mean / rstd: optional f32 [rows] outputs (norm = 1), the values the arithmetic above used.  The row statistics are f64
 * sums of the widened inputs, rounded once; the bf16 result is the round-to-nearest-even of the f32 one. */
int tribe_norm_act_fwd(const float* z, int64_t rows, int64_t dim, int64_t ld_z, const float* gamma, const float* beta, float eps,
                       int32_t norm, int32_t act, void* y, int32_t y_dtype, int64_t ld_y, float* mean, float* rstd, void* stream);
/* Backward of the above from dy (f32 or bf16, pitch ld_dy) and the saved z, mean, rstd (norm = 1):
 *   zh = (z - mean) * rstd, du = dy * act'(u), dzh = du * gamma,
 *   dz = rstd * (dzh - mean_H(dzh) - zh * mean_H(dzh * zh))   (norm = 0: dz = du), f32 or bf16, pitch ld_dz, pad columns zero;
 *   dgamma = sum_rows du * zh, dbeta = sum_rows du (f32 [dim], each optional, norm = 1 only).
 * act': ReLU 0 at u <= 0, ELU exp(u) at u <= 0, GELU Phi(u) + u phi(u).  Row means are f64; the column sums are f64 partials per block
 * of rows in the workspace (tribe_norm_act_bwd_workspace_bytes), summed in block order by a second launch: no atomics, equal inputs
 * give equal bits. */
size_t tribe_norm_act_bwd_workspace_bytes(int64_t rows, int64_t dim);
int tribe_norm_act_bwd(const void* dy, int32_t dy_dtype, int64_t ld_dy, const float* z, int64_t rows, int64_t dim, int64_t ld_z,
                       const float* mean, const float* rstd, const float* gamma, const float* beta, int32_t norm, int32_t act, void* dz,
                       int32_t dz_dtype, int64_t ld_dz, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
/* Which row kernel the two launchers above pick for these arguments: 0 = row in registers, 4 x 16 bytes per lane (dim <= 1024),
 * 1 = the same with 16 (dim <= 4096), 2 = 16-byte walk over the row in memory, 3 = element walk (a dim, pitch or pointer that is not
 * a multiple of four elements).  dy / dz NULL: the forward's choice for (z, y); else the backward's for (dy, z, dz). */
int tribe_norm_act_path(const float* z, int64_t dim, int64_t ld_z, const float* gamma, const float* beta, const void* y, int32_t y_dtype,
                        int64_t ld_y, const void* dy, int32_t dy_dtype, int64_t ld_dy);

/* ---- dropout with a counter-based mask (ff_dropout, Mlp dropout; csrc/dropout.hip) ----
 * y = keep(r, c) ? x * scale : +0.0 over the logical [rows, dim] tensor (f32 or bf16, row pitches ld_x / ld_y >= dim, x == y allowed;
 * any other overlap is undefined).  Element (r, c) has idx = r * dim + c (64-bit, from dim and never from a pitch); its random word is
 * word idx & 3 of Philox4x32-10 with counter (lo32(idx >> 2), hi32(idx >> 2), lo32(site), hi32(site)) and key (lo32(seed),
 * hi32(seed)); it is kept iff word >= threshold.  The host passes threshold = trunc(p * 2^32) and scale = (float)(1 / (1 - p)).
 * Kept: one f32 multiply, rounded to nearest (bf16: widened, multiplied in f32, rounded to nearest even).  Dropped: +0.0 by a select --
 * a dropped NaN, infinity or negative value is +0.0, where torch.dropout's multiply by zero gives NaN or -0.0.  Columns >= dim are
 * neither read nor written.  The backward of dropout is this call on the gradient with the same (threshold, scale, seed, site).
 * Integer-exact mask, no atomics: the result depends on (seed, site, r, c, dim, threshold, scale) alone.
 * Errors (< 0, nothing launched): null pointer, dtype, rows / dim <= 0, ld < dim, scale not in [1, FLT_MAX]. */
int tribe_dropout_apply(const void* x, void* y, int32_t dtype /* TRIBE_F32 | TRIBE_BF16 */, int64_t rows, int64_t dim, int64_t ld_x,
                        int64_t ld_y, uint32_t threshold, float scale, uint64_t seed, uint64_t site, void* stream);
/* Which kernel the launcher picks: 0 = 16-byte accesses (four f32 / eight bf16: dim and both pitches multiples of that, both pointers
 * 16-byte aligned), 1 = 8-byte accesses (four bf16 where 0 does not fit: multiples of four, 8-byte aligned), 2 = element accesses. */
int tribe_dropout_path(const void* x, const void* y, int32_t dtype, int64_t dim, int64_t ld_x, int64_t ld_y);

/* ---- the softmax row kernels of the training path (non-causal and causal), dropout mask drawn in registers (csrc/attn_softmax.hip) ----
 * One contract for the four entry points; the causal pair adds the one rule stated after it.
 * All work on a slab of `rows` rows of the logical tensor [B * heads * T, T] that starts at its row `row0`.  Element (r, j) of the slab
 * has idx = (row0 + r) * T + j (64-bit; from T, never from T_pad or a pitch) and is kept iff its word -- tribe_dropout_apply's: word
 * idx & 3 of Philox4x32-10 with counter (lo32(idx >> 2), hi32(idx >> 2), lo32(site), hi32(site)), key (lo32(seed), hi32(seed)) -- is
 * >= threshold.  m = scale_keep where kept, 0 where dropped; the host passes threshold = trunc(p * 2^32), scale_keep = (float)(1 / (1 - p)).
 * The mask depends on (seed, site, row0 + r, j, T, threshold) alone -- not on how a caller cuts the rows into slabs -- and is never
 * stored: the backward draws it again.  One Philox call serves four consecutive idx; a counter that straddles a row end (T % 4 != 0)
 * is drawn by both rows.  One wave per row, no atomics: bit-reproducible.  Any T >= 1.
 *
 * tribe_softmax_dropout_fwd: S f32 [rows, T] (pitch ld_s), the scaled scores scale * q.k ->
 *   Pd  bf16 [rows, T_pad] (pitch ld_p): kept: bf16(softmax(S) * scale_keep) -- the f32 softmax of tribe_softmax_fwd (row maximum
 *       subtracted, same summation order: threshold = 0, scale_keep = 1 gives its bits), one f32 multiply, one rounding to bf16;
 *       dropped: +0.0 by a select; columns T .. T_pad - 1: zero.
 *   lse f32 [rows]: the base-2 log-sum-exp log2 sum_j 2^(S[r, j] * log2 e) of the UNDROPPED row, the convention of the fused attention
 *       kernel's lse output: the ACT_EXP2 GEMM epilogue rebuilds P = exp2(scale * log2 e * q.k - lse) from it.
 * tribe_softmax_dropout_bwd: P bf16 [rows, T_pad] (ld_p; the undropped softmax), dPd f32 [rows, T] (ld_dp; dO V^T, unscaled) and
 *   negD f32 [rows] = -scale * D, D[r] = sum_j Pd[r, j] dPd[r, j] = sum_d dO[r, d] O[r, d] (what tribe_rowdot_heads_bf16 writes with
 *   its scale argument set to -scale) ->
 *   dS  bf16 [rows, T_pad] (ld_ds) = bf16(P * (scale * (m * dPd) + negD)) = scale * P * (m * dPd - D); columns >= T zero.  A dropped
 *       score keeps the gradient -scale * P * D.
 *   Pd  bf16 [rows, T_pad] (ld_pd) = bf16(P * m) (one f32 multiply), columns >= T zero.  Pd == P (with ld_pd == ld_p) overwrites P in
 *       place; dS must be a buffer of its own.
 * Errors (< 0, nothing launched): null pointer, rows / T <= 0, T_pad < T, row0 < 0, a pitch below its width (ld_s, ld_dp >= T; ld_p,
 * ld_ds, ld_pd >= T_pad), dS aliasing P or Pd, Pd == P with another pitch, scale_keep not in [1, FLT_MAX]. */
int tribe_softmax_dropout_fwd(const float* S, uint16_t* Pd, float* lse, int64_t rows, int64_t T, int64_t T_pad, int64_t ld_s, int64_t ld_p,
                              int64_t row0, uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site, void* stream);
int tribe_softmax_dropout_bwd(const uint16_t* P, const float* dPd, const float* negD, uint16_t* dS, uint16_t* Pd, int64_t rows, int64_t T,
                              int64_t T_pad, int64_t ld_p, int64_t ld_dp, int64_t ld_ds, int64_t ld_pd, float scale, int64_t row0,
                              uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site, void* stream);

/* The causal rule (the same kernel templates, compiled with CAUSAL): arguments, mask, errors and kernel selection are those of
 * tribe_softmax_dropout_fwd / _bwd, and row r of the slab is query
 * i = (row0 + r) % T of the logical tensor [B * heads * T, T], and columns j > i are masked (x_transformers' Decoder: scores with key >
 * query filled with -finfo.max before the softmax).  threshold = 0, scale_keep = 1 is causal attention without dropout.
 *   fwd: for j <= i Pd[r, j] = bf16(softmax(S[r, 0..i])[j] * m); +0.0 bits for every other column below T_pad; lse[r] = the base-2
 *        log-sum-exp of the visible scores.
 *   bwd: for j <= i dS = bf16(P * (scale * (m * dPd) + negD)) and Pd = bf16(P * m); +0.0 bits for every other column below T_pad of both.
 *        Pd == P (with ld_pd == ld_p) is allowed.
 * A row loads, draws and computes its quads 0 .. i / 4 only and zero-fills the rest; S, P and dPd above the diagonal are never used, so P
 * may come straight from a TRIBE_ACT_EXP2 epilogue that knows no mask (there it may hold inf).  On the columns <= i the results, lse
 * included, have the bits of the non-causal kernels run on the same scores with -inf written above the diagonal. */
int tribe_softmax_causal_fwd(const float* S, uint16_t* Pd, float* lse, int64_t rows, int64_t T, int64_t T_pad, int64_t ld_s, int64_t ld_p,
                             int64_t row0, uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site, void* stream);
int tribe_softmax_causal_bwd(const uint16_t* P, const float* dPd, const float* negD, uint16_t* dS, uint16_t* Pd, int64_t rows, int64_t T,
                             int64_t T_pad, int64_t ld_p, int64_t ld_dp, int64_t ld_ds, int64_t ld_pd, float scale, int64_t row0,
                             uint32_t threshold, float scale_keep, uint64_t seed, uint64_t site, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TRIBE_HIP_H */
