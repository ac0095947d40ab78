// Op-level entry points of the TRIBE encode path: each lowers one reference
// function to launches of the MFMA GEMM (gemm.hip) and the streaming kernels
// (elementwise.hip) on the caller's stream.  Host code only; no allocation, no sync.
#include "host_plan.h"

int tribe_internal_softmax(const float* S, int64_t R, int64_t T, int64_t ld_s, uint16_t* P, int64_t T_pad, int64_t ld_p,
                           hipStream_t stream);
int tribe_internal_transpose_v(const uint16_t* qkv, int64_t B, int64_t T, int heads, int dim_head, uint16_t* vt, int64_t T_pad,
                               hipStream_t stream);
int tribe_internal_attention_fused_supported(int dim_head);
int tribe_internal_attention_fused(const uint16_t* qkv, int64_t B, int64_t T, int heads, int dim_head, float scale, uint16_t* out,
                                   hipStream_t s);

int tribe_internal_kv_fill(const uint16_t* qkv, int64_t B, int64_t T, int heads, int dim_head, uint16_t* k_cache, uint16_t* v_cache,
                           int64_t cap, hipStream_t stream);

void tribe_internal_attention_set_wide384(int on);
void tribe_internal_attention_set_d64_variant(int v);
int tribe_internal_attention_rotates_q(int dim_head);
int tribe_internal_attention_fused_qrot(const uint16_t* qkv, int64_t B, int64_t T, int heads, int dim_head, float scale, uint16_t* out,
                                        const float* cos_tab, const float* sin_tab, int rot_dim, hipStream_t s);
static int g_attn_mode = 0;  // 0 = fused kernel when the head size has one, 1 = always the 3-kernel (materialised) path
extern "C" int tribe_attention_set_mode(int32_t mode) {
  TRIBE_REQUIRE(mode >= 0 && mode <= 5, "tribe_attention_set_mode: mode must be 0 (auto), 1 (materialised scores), 2 (fused, 16-row waves at every head size), 3 (dim_head 384 on the key-split kernel), 4 / 5 (dim_head 64 on the 4-wave / the anti-phase 8-wave kernel)");
  tribe_internal_attention_set_wide384(mode == 2 ? 0 : (mode == 3 ? 2 : 1));
  tribe_internal_attention_set_d64_variant(mode == 4 ? 1 : (mode == 5 ? 2 : 0));
  g_attn_mode = mode == 1 ? 1 : 0;
  return 0;
}

// The residual stream between the first out-proj and the last FF2 as two 16-bit planes (enum tribe_c_planes) instead of f32 + bf16 copy:
// one third fewer bytes written by the 2 * depth - 2 middle residual epilogues.  Process-wide, like g_attn_mode.
static int g_res_planes = 1;
static int g_res_tile_hint = 0;   // tile_hint of the out-proj / FF2 launches (2: the 256 x 256 role kernel at any shape, for tests and A/B runs)
extern "C" int tribe_encoder_set_residual_planes(int32_t on) {
  TRIBE_REQUIRE(on == 0 || on == 1, "tribe_encoder_set_residual_planes: 0 (f32 stream + bf16 copy) or 1 (16-bit hi / lo planes where the kernels allow)");
  g_res_planes = on;
  return 0;
}
extern "C" int tribe_encoder_set_residual_tile_hint(int32_t hint) {
  TRIBE_REQUIRE(hint == 0 || hint == 2, "tribe_encoder_set_residual_tile_hint: 0 (automatic) or 2 (256 x 256 role kernel)");
  g_res_tile_hint = hint;
  return 0;
}

namespace {

// attention is processed in batch chunks so that the f32 score block stays near the Infinity Cache size
constexpr size_t ATTN_SCORE_BUDGET = 192ull << 20;

struct AttnLayout {
  int64_t T_pad, chunk;
  float* S;       // [chunk, heads, T, T_pad] scores
  uint16_t* P;    // the same shape, softmax rounded to bf16
  uint16_t* Vt;   // [chunk, heads, dim_head, T_pad]
};

inline AttnLayout layout(int64_t B, int64_t T, int heads, int dim_head, Arena& ws) {
  AttnLayout p;
  p.T_pad = round_up(T, 64);
  const size_t per_b = (size_t)heads * T * p.T_pad * sizeof(float);
  int64_t chunk = (int64_t)(ATTN_SCORE_BUDGET / per_b);
  if (chunk < 1) chunk = 1;
  if (chunk > B) chunk = B;
  p.chunk = chunk;
  p.S = ws.take<float>((size_t)chunk * per_b);
  p.P = ws.take<uint16_t>((size_t)chunk * heads * T * p.T_pad * 2);
  p.Vt = ws.take<uint16_t>((size_t)chunk * heads * dim_head * p.T_pad * 2);
  return p;
}

}  // namespace

extern "C" int tribe_projector_fwd(const uint16_t* feat_packed, int64_t BT, int64_t T, int64_t K_pad, const uint16_t* w_packed,
                                   const float* bias, int64_t N_out, float* x, int64_t hidden, int64_t col0, int32_t accumulate,
                                   const float* pos_embed, const float* subj_embed, const int64_t* subject_id, void* stream) {
  TRIBE_REQUIRE(feat_packed && w_packed && x, "tribe_projector_fwd: null pointer");
  TRIBE_REQUIRE(BT > 0 && T > 0 && BT % T == 0, "tribe_projector_fwd: BT=%lld must be a positive multiple of T=%lld",
                (long long)BT, (long long)T);
  TRIBE_REQUIRE(N_out > 0 && col0 >= 0 && col0 + N_out <= hidden, "tribe_projector_fwd: column slice [%lld, %lld) outside hidden=%lld",
                (long long)col0, (long long)(col0 + N_out), (long long)hidden);
  TRIBE_REQUIRE(!subj_embed || subject_id, "tribe_projector_fwd: subject_embed without subject_id");
  Linear d(TRIBE_ROLE_PROJECTOR, BT, feat_packed, K_pad, w_packed, bias, x + col0, N_out, TRIBE_F32);
  d.ldc = hidden;   // a column slice of the fused stream
  if (accumulate) d.residual(x + col0);
  if (pos_embed) { d.rowadd = pos_embed + col0; d.ld_rowadd = hidden; d.rowadd_period = T; }
  if (subj_embed) { d.gadd = subj_embed + col0; d.gadd_index = subject_id; d.gadd_div = T; d.ld_gadd = hidden; }
  return tribe_gemm_bf16(&d, stream);
}

extern "C" size_t tribe_attention_workspace_bytes(int64_t B, int64_t T, int32_t heads, int32_t dim_head) {
  if (B <= 0 || T <= 0 || heads <= 0 || dim_head <= 0) return 0;
  Arena ws;
  layout(B, T, heads, dim_head, ws);
  return ws.off;
}

extern "C" int tribe_attention_fwd(const uint16_t* qkv, int64_t B, int64_t T, int32_t heads, int32_t dim_head, float scale,
                                   uint16_t* out, void* workspace, size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(qkv && out && workspace, "tribe_attention_fwd: null pointer");
  TRIBE_REQUIRE(B > 0 && T > 0 && heads > 0 && dim_head > 0, "tribe_attention_fwd: bad shape");
  TRIBE_REQUIRE(dim_head % 64 == 0, "tribe_attention_fwd: dim_head=%d must be a multiple of 64", dim_head);
  Arena ws(workspace);
  const AttnLayout p = layout(B, T, heads, dim_head, ws);
  TRIBE_REQUIRE(workspace_bytes >= ws.off, "tribe_attention_fwd: workspace too small");
  TRIBE_REQUIRE(((uintptr_t)workspace % 256) == 0, "tribe_attention_fwd: workspace must be 256-byte aligned");
  if (g_attn_mode == 0 && tribe_internal_attention_fused_supported(dim_head))
    return tribe_internal_attention_fused(qkv, B, T, heads, dim_head, scale, out, (hipStream_t)stream);
  const int64_t inner = (int64_t)heads * dim_head, Tp = p.T_pad;
  hipStream_t s = (hipStream_t)stream;
  for (int64_t b0 = 0; b0 < B; b0 += p.chunk) {
    const int64_t nb = (B - b0 < p.chunk) ? B - b0 : p.chunk;
    const uint16_t* q = qkv + b0 * T * 3 * inner;
    int rc = tribe_internal_transpose_v(q, nb, T, heads, dim_head, p.Vt, Tp, s);
    if (rc) return rc;
    // S[b,h] = scale * Q K^T  (strided views of the fused rows, batched over (b, h): not a Linear)
    tribe_gemm_desc d = gemm_zero();
    d.M = T; d.N = T; d.K = dim_head; d.batch1 = nb; d.batch0 = heads;
    d.A = q; d.lda = 3 * inner; d.sA1 = T * 3 * inner; d.sA0 = dim_head;
    d.B = q + inner; d.ldb = 3 * inner; d.sB1 = T * 3 * inner; d.sB0 = dim_head;
    d.C = p.S; d.ldc = Tp; d.sC1 = (int64_t)heads * T * Tp; d.sC0 = T * Tp; d.c_dtype = TRIBE_F32;
    d.alpha = scale;
    d.role = TRIBE_ROLE_ATTN_SCORES;
    rc = tribe_gemm_bf16(&d, stream);
    if (rc) return rc;
    // softmax in f32 (x_transformers Attend: softmax(dtype=float32)), P rounded to bf16 for the second MFMA product
    rc = tribe_internal_softmax(p.S, nb * heads * T, T, Tp, p.P, Tp, Tp, s);
    if (rc) return rc;
    // O[b,h] = P V   (B operand = V^T, K = T_pad zero padded on both sides)
    d = gemm_zero();
    d.M = T; d.N = dim_head; d.K = Tp; d.batch1 = nb; d.batch0 = heads;
    d.A = p.P; d.lda = Tp; d.sA1 = (int64_t)heads * T * Tp; d.sA0 = T * Tp;
    d.B = p.Vt; d.ldb = Tp; d.sB1 = (int64_t)heads * dim_head * Tp; d.sB0 = (int64_t)dim_head * Tp;
    d.C = out + b0 * T * inner; d.ldc = inner; d.sC1 = T * inner; d.sC0 = dim_head; d.c_dtype = TRIBE_BF16;
    d.role = TRIBE_ROLE_ATTN_PV;
    rc = tribe_gemm_bf16(&d, stream);
    if (rc) return rc;
  }
  return 0;
}

namespace {
struct EncLayout {
  int64_t M, inner;
  bool fuse_norm;      // ScaleNorm folded into the GEMMs either side of it (needs whole 256-column tiles)
  uint16_t* xn;        // [M, dim] bf16 input of QKV / FF1
  uint16_t* qkv;       // [M, 3*inner]
  uint16_t* ao;        // [M, inner], behind qkv
  uint16_t* hbuf;      // [M, ff_inner], over qkv | ao (dead by then)
  void* attn_ws; size_t attn_bytes;
  float* ssq;          // [M, n_part] partial sums of squares (<= dim / 32 slots per row, by the producer's tile)
  float* rowf;         // [M] ScaleNorm factors, behind ssq
  void* split_ws; size_t split_bytes;
};
inline EncLayout layout(const tribe_encoder_desc* d, Arena& ws) {
  EncLayout p;
  const int64_t M = p.M = d->B * d->T;
  const int64_t inner = p.inner = (int64_t)d->heads * d->dim_head;
  p.xn = ws.take<uint16_t>((size_t)M * d->dim * 2);
  const int64_t wide = (4 * inner > d->ff_inner) ? 4 * inner : d->ff_inner;
  p.qkv = p.hbuf = ws.take<uint16_t>((size_t)M * wide * 2);
  p.ao = p.qkv + (size_t)M * 3 * inner;
  p.attn_bytes = tribe_attention_workspace_bytes(d->B, d->T, d->heads, d->dim_head);
  p.attn_ws = ws.take<void>(p.attn_bytes);
  p.fuse_norm = d->dim % 256 == 0 && inner % 256 == 0 && d->ff_inner % 256 == 0;
  p.ssq = p.fuse_norm ? ws.take<float>((size_t)M * (d->dim / 32 + 1) * 4) : nullptr;
  p.rowf = p.fuse_norm ? p.ssq + (size_t)M * (d->dim / 32) : nullptr;
  // few rows (BASELINE config 1: M = 128): the four GEMMs of a layer are well under one round of tiles and run split over K
  // (tribe_gemm_desc.stream_k) -- up to 8 f32 shares of the widest output
  const int64_t widest = 3 * inner > d->ff_inner ? (3 * inner > d->dim ? 3 * inner : d->dim) : (d->ff_inner > d->dim ? d->ff_inner : d->dim);
  p.split_bytes = M <= 512 ? align256((size_t)8 * M * widest * 4) : 0;
  p.split_ws = p.split_bytes ? ws.take<void>(p.split_bytes) : nullptr;
  return p;
}
// where a prefill leaves every layer's rotated k heads and v heads: caches [depth, B, heads, cap, dim_head]
struct KvSink {
  uint16_t *k, *v;
  int64_t cap;
};
// A GEMM of a small batch may run split over K: hand it the workspace when the launcher says it would use one
inline void allow_split_k(tribe_gemm_desc& g, void* split_ws, size_t split_bytes) {
  if (split_bytes == 0) return;
  g.stream_k = 1;
  const int64_t need = tribe_gemm_stream_k_workspace_bytes(&g);
  if (need > 0 && (size_t)need <= split_bytes) { g.stream_k_ws = split_ws; g.stream_k_ws_bytes = (int64_t)split_bytes; }
  else g.stream_k = 0;
}
inline int enc_validate(const tribe_encoder_desc* d) {
  TRIBE_REQUIRE(d != nullptr, "tribe_encoder: null descriptor");
  TRIBE_REQUIRE(d->B > 0 && d->T > 0 && d->dim > 0 && d->depth >= 0 && d->heads > 0 && d->dim_head > 0 && d->ff_inner > 0,
                "tribe_encoder: bad shape");
  TRIBE_REQUIRE(d->dim % 64 == 0 && d->dim_head % 64 == 0 && d->ff_inner % 64 == 0,
                "tribe_encoder: dim=%d, dim_head=%d, ff_inner=%d must be multiples of 64", d->dim, d->dim_head, d->ff_inner);
  TRIBE_REQUIRE(d->rot_dim == 0 || (d->cos_tab && d->sin_tab), "tribe_encoder: rotary tables missing");
  TRIBE_REQUIRE(d->depth == 0 || d->layers_host, "tribe_encoder: layers_host missing");
  TRIBE_REQUIRE(d->final_norm_g, "tribe_encoder: final_norm_g missing");
  return 0;
}
}  // namespace

extern "C" size_t tribe_encoder_workspace_bytes(const tribe_encoder_desc* d) {
  if (!d || d->B <= 0 || d->T <= 0) return 0;
  Arena ws;
  layout(d, ws);
  return ws.off;
}

// the body of tribe_encoder_fwd (flags = 0), tribe_encoder_fwd_ex and tribe_encoder_prefill_fwd (causal, with a sink: one more launch
// per layer, after the rotary pass; without a sink the launches are what they were)
static int encoder_fwd_body(const tribe_encoder_desc* d, uint32_t flags, float* x, void* y, int32_t y_dtype, void* workspace,
                            size_t workspace_bytes, void* stream, const KvSink* sink = nullptr) {
  int rc = enc_validate(d);
  if (rc) return rc;
  const bool causal = (flags & TRIBE_ENCODER_CAUSAL) != 0;
  TRIBE_REQUIRE(x && y && workspace, "tribe_encoder_fwd: null pointer");
  TRIBE_REQUIRE(((uintptr_t)workspace % 256) == 0, "tribe_encoder_fwd: workspace must be 256-byte aligned");
  Arena ws(workspace);
  const EncLayout p = layout(d, ws);
  TRIBE_REQUIRE(workspace_bytes >= ws.off, "tribe_encoder_fwd: workspace too small (%zu < %zu)", workspace_bytes, ws.off);
  const int64_t M = p.M, inner = p.inner, dim = d->dim;
  uint16_t *xn = p.xn, *qkv = p.qkv, *ao = p.ao, *hbuf = p.hbuf;
  float *ssq = p.ssq, *rowf = p.rowf;
  auto allow_split = [&](tribe_gemm_desc& g) { allow_split_k(g, p.split_ws, p.split_bytes); };
  int64_t n_part = dim / 64;   // slots per row the LAST producer wrote (one per wave column group of its tile: tribe_gemm_sumsq_slots)
  const float scale = 1.0f / sqrtf((float)d->dim_head);
  // With whole 256-column tiles the pre-norms are folded into the GEMMs: the GEMM that writes x also leaves bf16(x) in `xn` and
  // the per-row partial sums of squares; a [M]-sized kernel turns them into the ScaleNorm factors; the next GEMM reads the raw
  // bf16(x) and scales its accumulator rows (W . (x s) = s (W . x)).  Only the first norm (x comes from the projector) and the
  // final one (its consumer, the voxel head, has x on the column side) stay stand-alone launches: 2 instead of 2 * depth + 1.
  const bool fuse = p.fuse_norm;
  bool have_factors = false;   // rowf / xn describe the current x
  // The two GEMMs of layer l that write the residual stream (ff2 = false: out-proj), ld_row_sumsq left to the caller.  as_planes: between the
  // first out-proj (f32 x in) and the last FF2 (f32 x out) the stream is the pair (hi = xn, lo = half the bytes of x), read and written in place.
  auto residual_gemm = [&](int l, bool ff2, bool as_planes) {
    const tribe_encoder_layer& L = d->layers_host[l];
    const bool first = l == 0 && !ff2, last = l + 1 == d->depth && ff2;
    tribe_gemm_desc g = ff2 ? Linear(TRIBE_ROLE_FF2, M, hbuf, d->ff_inner, L.w_ff2, L.b_ff2, x, dim, TRIBE_F32).residual(x)
                            : Linear(TRIBE_ROLE_OUT_PROJ, M, ao, inner, L.w_out, nullptr, x, dim, TRIBE_F32).residual(x);
    g.res_scale = ff2 ? L.ff_res_scale : L.attn_res_scale;
    g.tile_hint = g_res_tile_hint;
    if (fuse && !last) { g.c_bf16 = xn; g.ld_c_bf16 = dim; g.row_sumsq = ssq; }
    if (as_planes) {   // lo lives in x itself: the first 128 bytes of every 64-column strip's 256 (rows 2 dim 16-bit slots apart), in place
      g.c_dtype = first ? TRIBE_F32_PLANES_OUT : (last ? TRIBE_F32_PLANES_IN : TRIBE_F32_PLANES_INOUT);
      g.c_bf16 = xn; g.ld_c_bf16 = dim;
      if (!first) g.ldres = 2 * dim;
      if (!last) g.ldc = 2 * dim;
    }
    return g;
  };
  // planes: only where every residual launch of the forward runs the 256 x 256 role kernel (else the path is the f32 one throughout)
  bool planes = g_res_planes && fuse && p.split_bytes == 0 && d->depth > 0;
  for (int l = 0; planes && l < d->depth; ++l) {
    for (int ff2 = 0; planes && ff2 < 2; ++ff2) {
      const tribe_gemm_desc g = residual_gemm(l, ff2 != 0, true);
      planes = tribe_gemm_epilogue_path(&g) == 1;
    }
  }

  for (int l = 0; l < d->depth; ++l) {
    const tribe_encoder_layer& L = d->layers_host[l];
    TRIBE_REQUIRE(L.attn_norm_g && L.w_qkv && L.w_out && L.ff_norm_g && L.w_ff1 && L.b_ff1 && L.w_ff2 && L.b_ff2,
                  "tribe_encoder_fwd: layer %d has a null parameter", l);
    // ---- attention block: x = to_out(attn(rotary(qkv(norm(x))))) + x * residual_scale ----
    rc = have_factors ? tribe_rownorm_scale_fwd(ssq, M, n_part, L.attn_norm_g, d->norm_gain_scale, d->norm_eps, rowf, stream)
                      : tribe_scalenorm_fwd(x, M, dim, L.attn_norm_g, d->norm_gain_scale, d->norm_eps, xn, TRIBE_BF16, stream);
    if (rc) return rc;
    tribe_gemm_desc g = Linear(TRIBE_ROLE_QKV, M, xn, dim, L.w_qkv, nullptr, qkv, 3 * inner, TRIBE_BF16);
    if (have_factors) g.row_scale = rowf;
    allow_split(g);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
    // q heads and k heads are adjacent in the fused row.  The DH = 384 attention kernel rotates Q while it loads its Q fragments
    // (interleaved pairs; bit-identical arithmetic), so only the k heads go through the stand-alone pass: half its 805 MB.
    const bool q_in_attn = !causal && g_attn_mode == 0 && d->rot_dim > 0 && d->rotary_interleaved == 1 && d->rot_dim % 16 == 0 &&
                           tribe_internal_attention_rotates_q(d->dim_head);
    if (d->rot_dim > 0) {
      rc = q_in_attn ? tribe_rotary_fwd(qkv + inner, M, d->T, 3 * inner, d->heads, d->dim_head, d->rot_dim, d->cos_tab, d->sin_tab,
                                        d->rotary_interleaved, stream)
                     : tribe_rotary_fwd(qkv, M, d->T, 3 * inner, 2 * d->heads, d->dim_head, d->rot_dim, d->cos_tab, d->sin_tab,
                                        d->rotary_interleaved, stream);
      if (rc) return rc;
    }
    if (sink) {   // the rotated k heads and the v heads of all T positions into slots 0 .. T-1 of this layer's caches
      const int64_t per_layer = d->B * inner * sink->cap;
      rc = tribe_internal_kv_fill(qkv, d->B, d->T, d->heads, d->dim_head, sink->k + l * per_layer, sink->v + l * per_layer, sink->cap,
                                  (hipStream_t)stream);
      if (rc) return rc;
    }
    if (causal) {   // the fused kernel under the mask (the 16-row kernel at every head size): q and k arrive rotated
      tribe_attention_desc a{};
      a.q = qkv; a.k = qkv + inner; a.v = qkv + 2 * inner;
      a.ld_q = a.ld_k = a.ld_v = 3 * inner;
      a.out = ao; a.ld_out = inner;
      a.B = d->B; a.T = d->T;
      a.heads_q = a.heads_kv = d->heads; a.dim_head = d->dim_head; a.causal = 1;
      a.scale = scale;
      rc = tribe_attention_fwd_ex(&a, stream);
    } else {
      rc = q_in_attn ? tribe_internal_attention_fused_qrot(qkv, d->B, d->T, d->heads, d->dim_head, scale, ao, d->cos_tab, d->sin_tab,
                                                           d->rot_dim, (hipStream_t)stream)
                     : tribe_attention_fwd(qkv, d->B, d->T, d->heads, d->dim_head, scale, ao, p.attn_ws, p.attn_bytes, stream);
    }
    if (rc) return rc;
    g = residual_gemm(l, false, planes);
    if (fuse) {
      n_part = tribe_gemm_sumsq_slots(&g);
      TRIBE_REQUIRE(n_part > 0 && n_part <= dim / 32, "tribe_encoder_fwd: unexpected row_sumsq slot count %lld", (long long)n_part);
      g.ld_row_sumsq = n_part;
    }
    allow_split(g);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
    // ---- feed-forward block: x = W2 gelu(W1 norm(x) + b1) + b2 + x * residual_scale ----
    rc = fuse ? tribe_rownorm_scale_fwd(ssq, M, n_part, L.ff_norm_g, d->norm_gain_scale, d->norm_eps, rowf, stream)
              : tribe_scalenorm_fwd(x, M, dim, L.ff_norm_g, d->norm_gain_scale, d->norm_eps, xn, TRIBE_BF16, stream);
    if (rc) return rc;
    g = Linear(TRIBE_ROLE_FF1, M, xn, dim, L.w_ff1, L.b_ff1, hbuf, d->ff_inner, TRIBE_BF16).activation(TRIBE_ACT_GELU);
    if (fuse) g.row_scale = rowf;
    allow_split(g);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
    g = residual_gemm(l, true, planes);
    have_factors = fuse && l + 1 < d->depth;   // the next layer's QKV takes the raw bf16(x) + factors
    if (have_factors) {
      n_part = tribe_gemm_sumsq_slots(&g);
      TRIBE_REQUIRE(n_part > 0 && n_part <= dim / 32, "tribe_encoder_fwd: unexpected row_sumsq slot count %lld", (long long)n_part);
      g.ld_row_sumsq = n_part;
    }
    allow_split(g);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
  }
  return tribe_scalenorm_fwd(x, M, dim, d->final_norm_g, d->norm_gain_scale, d->norm_eps, y, y_dtype, stream);
}

extern "C" int tribe_encoder_fwd(const tribe_encoder_desc* d, float* x, void* y, int32_t y_dtype, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return encoder_fwd_body(d, 0u, x, y, y_dtype, workspace, workspace_bytes, stream);
}

extern "C" int tribe_encoder_fwd_ex(const tribe_encoder_desc* d, uint32_t flags, float* x, void* y, int32_t y_dtype, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE((flags & ~TRIBE_ENCODER_CAUSAL) == 0, "tribe_encoder_fwd_ex: unknown flag bits 0x%x (known: TRIBE_ENCODER_CAUSAL = 1)",
                (unsigned)(flags & ~TRIBE_ENCODER_CAUSAL));
  return encoder_fwd_body(d, flags, x, y, y_dtype, workspace, workspace_bytes, stream);
}

// ---- streaming: a causal encoder one position at a time (attn_decode.hip) ----
extern "C" int tribe_encoder_prefill_fwd(const tribe_encoder_desc* d, float* x, void* y, int32_t y_dtype, uint16_t* k_cache,
                                         uint16_t* v_cache, int64_t cap, void* workspace, size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(d != nullptr, "tribe_encoder_prefill_fwd: null descriptor");
  TRIBE_REQUIRE(x && y && workspace && k_cache && v_cache, "tribe_encoder_prefill_fwd: null pointer");
  TRIBE_REQUIRE(d->T > 0 && d->T <= cap, "tribe_encoder_prefill_fwd: T=%lld positions do not fit the cache capacity %lld", (long long)d->T,
                (long long)cap);
  TRIBE_REQUIRE(((uintptr_t)k_cache % 16) == 0 && ((uintptr_t)v_cache % 16) == 0, "tribe_encoder_prefill_fwd: caches must be 16-byte aligned");
  const KvSink sink{k_cache, v_cache, cap};
  return encoder_fwd_body(d, TRIBE_ENCODER_CAUSAL, x, y, y_dtype, workspace, workspace_bytes, stream, &sink);
}

namespace {
struct StepLayout {
  int64_t inner;
  uint16_t* xn;     // [B, dim] bf16 input of QKV / FF1
  uint16_t* qkv;    // [B, 3*inner]
  uint16_t* ao;     // [B, inner], behind qkv
  uint16_t* hbuf;   // [B, ff_inner], over qkv | ao (dead by then)
  void* attn_ws; size_t attn_bytes;
  void* split_ws; size_t split_bytes;
};
inline StepLayout step_layout(const tribe_encoder_desc* d, int64_t cap, Arena& ws) {
  StepLayout p;
  const int64_t M = d->B, inner = p.inner = (int64_t)d->heads * d->dim_head;
  p.xn = ws.take<uint16_t>((size_t)M * d->dim * 2);
  const int64_t wide = (4 * inner > d->ff_inner) ? 4 * inner : d->ff_inner;
  p.qkv = p.hbuf = ws.take<uint16_t>((size_t)M * wide * 2);
  p.ao = p.qkv + (size_t)M * 3 * inner;
  p.attn_bytes = tribe_attention_decode_workspace_bytes(d->B, d->heads, d->dim_head, cap);   // the most parts any n <= cap has
  p.attn_ws = ws.take<void>(p.attn_bytes);
  const int64_t widest = 3 * inner > d->ff_inner ? (3 * inner > d->dim ? 3 * inner : d->dim) : (d->ff_inner > d->dim ? d->ff_inner : d->dim);
  p.split_bytes = align256((size_t)8 * M * widest * 4);   // every GEMM of a step is far under one round of tiles (encoder_fwd_body's allowance)
  p.split_ws = ws.take<void>(p.split_bytes);
  return p;
}
}  // namespace

extern "C" size_t tribe_encoder_step_workspace_bytes(const tribe_encoder_desc* d, int64_t cap) {
  if (!d || d->B <= 0 || cap <= 0) return 0;
  Arena ws;
  step_layout(d, cap, ws);
  return ws.off;
}

namespace {
// The launches of a step, after the entry point's own argument checks (`name`, for the messages).  pos_slots == nullptr: every sequence at
// `pos` (tribe_encoder_step_fwd); else sequence b at pos_slots[b], n_max an upper bound of every pos_slots[b] + 1
// (tribe_encoder_step_slots_fwd): the same launches, the two cache-aware ones in their slot forms.
int step_body(const char* name, const tribe_encoder_desc* d, float* x, void* y, int32_t y_dtype, uint16_t* k_cache, uint16_t* v_cache,
              int64_t cap, int64_t pos, const int32_t* pos_slots, int64_t n_max, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = 0;
  TRIBE_REQUIRE(((uintptr_t)workspace % 256) == 0, "%s: workspace must be 256-byte aligned", name);
  Arena ws(workspace);
  const StepLayout p = step_layout(d, cap, ws);
  TRIBE_REQUIRE(workspace_bytes >= ws.off, "%s: workspace too small (%zu < %zu)", name, workspace_bytes, ws.off);
  const int64_t M = d->B, inner = p.inner, dim = d->dim;
  const int64_t per_layer = d->B * inner * cap;
  const float scale = 1.0f / sqrtf((float)d->dim_head);
  // M = B rows never fill the 256-column tiles of rows the fused-norm GEMM path needs: every ScaleNorm is its own launch
  for (int l = 0; l < d->depth; ++l) {
    const tribe_encoder_layer& L = d->layers_host[l];
    TRIBE_REQUIRE(L.attn_norm_g && L.w_qkv && L.w_out && L.ff_norm_g && L.w_ff1 && L.b_ff1 && L.w_ff2 && L.b_ff2,
                  "%s: layer %d has a null parameter", name, l);
    rc = tribe_scalenorm_fwd(x, M, dim, L.attn_norm_g, d->norm_gain_scale, d->norm_eps, p.xn, TRIBE_BF16, stream);
    if (rc) return rc;
    tribe_gemm_desc g = Linear(TRIBE_ROLE_QKV, M, p.xn, dim, L.w_qkv, nullptr, p.qkv, 3 * inner, TRIBE_BF16);
    allow_split_k(g, p.split_ws, p.split_bytes);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
    uint16_t *kc = k_cache + l * per_layer, *vc = v_cache + l * per_layer;
    if (pos_slots) {
      rc = tribe_kv_append_slots(p.qkv, d->B, 1, d->heads, d->dim_head, d->rot_dim, d->rotary_interleaved, d->cos_tab, d->sin_tab, pos_slots, kc,
                                 vc, cap, stream);
      if (rc) return rc;
      rc = tribe_attention_decode_slots_fwd(p.qkv, 3 * inner, kc, vc, d->B, d->heads, d->dim_head, cap, pos_slots, n_max, scale, p.ao, p.attn_ws,
                                            p.attn_bytes, stream);
    } else {
      rc = tribe_kv_append(p.qkv, d->B, d->heads, d->dim_head, d->rot_dim, d->rotary_interleaved, d->cos_tab, d->sin_tab, pos, kc, vc, cap, stream);
      if (rc) return rc;
      rc = tribe_attention_decode_fwd(p.qkv, 3 * inner, kc, vc, d->B, d->heads, d->dim_head, cap, pos + 1, scale, p.ao, p.attn_ws, p.attn_bytes,
                                      stream);
    }
    if (rc) return rc;
    g = Linear(TRIBE_ROLE_OUT_PROJ, M, p.ao, inner, L.w_out, nullptr, x, dim, TRIBE_F32).residual(x);
    g.res_scale = L.attn_res_scale;
    allow_split_k(g, p.split_ws, p.split_bytes);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
    rc = tribe_scalenorm_fwd(x, M, dim, L.ff_norm_g, d->norm_gain_scale, d->norm_eps, p.xn, TRIBE_BF16, stream);
    if (rc) return rc;
    g = Linear(TRIBE_ROLE_FF1, M, p.xn, dim, L.w_ff1, L.b_ff1, p.hbuf, d->ff_inner, TRIBE_BF16).activation(TRIBE_ACT_GELU);
    allow_split_k(g, p.split_ws, p.split_bytes);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
    g = Linear(TRIBE_ROLE_FF2, M, p.hbuf, d->ff_inner, L.w_ff2, L.b_ff2, x, dim, TRIBE_F32).residual(x);
    g.res_scale = L.ff_res_scale;
    allow_split_k(g, p.split_ws, p.split_bytes);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
  }
  return tribe_scalenorm_fwd(x, M, dim, d->final_norm_g, d->norm_gain_scale, d->norm_eps, y, y_dtype, stream);
}
}  // namespace

extern "C" int tribe_encoder_step_fwd(const tribe_encoder_desc* d, float* x, void* y, int32_t y_dtype, uint16_t* k_cache, uint16_t* v_cache,
                                      int64_t cap, int64_t pos, void* workspace, size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(d != nullptr, "tribe_encoder_step_fwd: null descriptor");
  int rc = enc_validate(d);
  if (rc) return rc;
  TRIBE_REQUIRE(x && y && workspace && k_cache && v_cache, "tribe_encoder_step_fwd: null pointer");
  TRIBE_REQUIRE(d->T == 1, "tribe_encoder_step_fwd: a step is one position per sequence (T=%lld)", (long long)d->T);
  TRIBE_REQUIRE(cap > 0 && pos >= 0 && pos < cap, "tribe_encoder_step_fwd: pos=%lld outside the cache capacity %lld", (long long)pos, (long long)cap);
  return step_body("tribe_encoder_step_fwd", d, x, y, y_dtype, k_cache, v_cache, cap, pos, nullptr, 0, workspace, workspace_bytes, stream);
}

// every sequence at a position of its own: pos int32 [B] on the device (-1 = takes no part), n_max >= every pos[b] + 1
extern "C" int tribe_encoder_step_slots_fwd(const tribe_encoder_desc* d, float* x, void* y, int32_t y_dtype, uint16_t* k_cache,
                                            uint16_t* v_cache, int64_t cap, const int32_t* pos, int64_t n_max, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(d != nullptr, "tribe_encoder_step_slots_fwd: null descriptor");
  int rc = enc_validate(d);
  if (rc) return rc;
  TRIBE_REQUIRE(x && y && workspace && k_cache && v_cache && pos, "tribe_encoder_step_slots_fwd: null pointer");
  TRIBE_REQUIRE(d->T == 1, "tribe_encoder_step_slots_fwd: a step is one position per sequence (T=%lld)", (long long)d->T);
  TRIBE_REQUIRE(cap > 0 && n_max >= 1 && n_max <= cap, "tribe_encoder_step_slots_fwd: n_max=%lld keys outside 1 .. capacity %lld",
                (long long)n_max, (long long)cap);
  return step_body("tribe_encoder_step_slots_fwd", d, x, y, y_dtype, k_cache, v_cache, cap, 0, pos, n_max, workspace, workspace_bytes, stream);
}

// ---- block append: d->T = k positions per sequence onto caches that hold `pos` (attention.hip: tribe_attention_extend_fwd) ----
namespace {
struct ExtendLayout {
  int64_t M, inner;
  uint16_t* xn;     // [B*k, dim] bf16 input of QKV / FF1
  uint16_t* qkv;    // [B*k, 3*inner]
  uint16_t* ao;     // [B*k, inner], behind qkv
  uint16_t* hbuf;   // [B*k, ff_inner], over qkv | ao (dead by then)
  void* split_ws; size_t split_bytes;
};
inline ExtendLayout extend_layout(const tribe_encoder_desc* d, Arena& ws) {
  ExtendLayout p;
  const int64_t M = p.M = d->B * d->T, inner = p.inner = (int64_t)d->heads * d->dim_head;
  p.xn = ws.take<uint16_t>((size_t)M * d->dim * 2);
  const int64_t wide = (4 * inner > d->ff_inner) ? 4 * inner : d->ff_inner;
  p.qkv = p.hbuf = ws.take<uint16_t>((size_t)M * wide * 2);
  p.ao = p.qkv + (size_t)M * 3 * inner;
  // few rows: the GEMMs may run split over K, as in encoder_fwd_body
  const int64_t widest = 3 * inner > d->ff_inner ? (3 * inner > d->dim ? 3 * inner : d->dim) : (d->ff_inner > d->dim ? d->ff_inner : d->dim);
  p.split_bytes = M <= 512 ? align256((size_t)8 * M * widest * 4) : 0;
  p.split_ws = p.split_bytes ? ws.take<void>(p.split_bytes) : nullptr;
  return p;
}
}  // namespace

extern "C" size_t tribe_encoder_extend_workspace_bytes(const tribe_encoder_desc* d, int64_t cap) {
  if (!d || d->B <= 0 || d->T <= 0 || cap <= 0) return 0;
  Arena ws;
  extend_layout(d, ws);
  return ws.off;
}

namespace {
// The launches of a block append, after the entry point's own range check (`name`, for the messages).  pos_slots == nullptr: every
// sequence at `pos` (tribe_encoder_extend_fwd); else sequence b at pos_slots[b] (tribe_encoder_extend_slots_fwd): the same launches, the
// two cache-aware ones in their slot forms.
int extend_body(const char* name, const tribe_encoder_desc* d, float* x, void* y, int32_t y_dtype, uint16_t* k_cache, uint16_t* v_cache,
                int64_t cap, int64_t pos, const int32_t* pos_slots, void* workspace, size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(tribe_internal_attention_fused_supported(d->dim_head), "%s: dim_head=%d not in {64,128,192,384}", name, d->dim_head);
  int rc = enc_validate(d);
  if (rc) return rc;
  TRIBE_REQUIRE(x && y && workspace && k_cache && v_cache, "%s: null pointer", name);
  TRIBE_REQUIRE(((uintptr_t)k_cache % 16) == 0 && ((uintptr_t)v_cache % 16) == 0, "%s: caches must be 16-byte aligned", name);
  TRIBE_REQUIRE(((uintptr_t)workspace % 256) == 0, "%s: workspace must be 256-byte aligned", name);
  Arena ws(workspace);
  const ExtendLayout p = extend_layout(d, ws);
  TRIBE_REQUIRE(workspace_bytes >= ws.off, "%s: workspace too small (%zu < %zu)", name, workspace_bytes, ws.off);
  const int64_t M = p.M, inner = p.inner, dim = d->dim;
  const int64_t per_layer = d->B * inner * cap;
  const float scale = 1.0f / sqrtf((float)d->dim_head);
  // tribe_encoder_step_fwd's launches with k rows per sequence: every ScaleNorm its own launch, one GEMM each, and between QKV and
  // out-proj the block's rotary + cache write (one launch) and the rectangular causal attention against the cache plus the block
  for (int l = 0; l < d->depth; ++l) {
    const tribe_encoder_layer& L = d->layers_host[l];
    TRIBE_REQUIRE(L.attn_norm_g && L.w_qkv && L.w_out && L.ff_norm_g && L.w_ff1 && L.b_ff1 && L.w_ff2 && L.b_ff2,
                  "%s: layer %d has a null parameter", name, l);
    rc = tribe_scalenorm_fwd(x, M, dim, L.attn_norm_g, d->norm_gain_scale, d->norm_eps, p.xn, TRIBE_BF16, stream);
    if (rc) return rc;
    tribe_gemm_desc g = Linear(TRIBE_ROLE_QKV, M, p.xn, dim, L.w_qkv, nullptr, p.qkv, 3 * inner, TRIBE_BF16);
    allow_split_k(g, p.split_ws, p.split_bytes);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
    uint16_t *kc = k_cache + l * per_layer, *vc = v_cache + l * per_layer;
    if (pos_slots) {
      rc = tribe_kv_append_slots(p.qkv, d->B, d->T, d->heads, d->dim_head, d->rot_dim, d->rotary_interleaved, d->cos_tab, d->sin_tab, pos_slots,
                                 kc, vc, cap, stream);
      if (rc) return rc;
      rc = tribe_attention_extend_slots_fwd(p.qkv, 3 * inner, kc, vc, d->B, d->heads, d->dim_head, cap, pos_slots, d->T, scale, p.ao, stream);
    } else {
      rc = tribe_kv_append_block(p.qkv, d->B, d->T, d->heads, d->dim_head, d->rot_dim, d->rotary_interleaved, d->cos_tab, d->sin_tab, pos, kc,
                                 vc, cap, stream);
      if (rc) return rc;
      rc = tribe_attention_extend_fwd(p.qkv, 3 * inner, kc, vc, d->B, d->heads, d->dim_head, cap, pos, d->T, scale, p.ao, stream);
    }
    if (rc) return rc;
    g = Linear(TRIBE_ROLE_OUT_PROJ, M, p.ao, inner, L.w_out, nullptr, x, dim, TRIBE_F32).residual(x);
    g.res_scale = L.attn_res_scale;
    allow_split_k(g, p.split_ws, p.split_bytes);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
    rc = tribe_scalenorm_fwd(x, M, dim, L.ff_norm_g, d->norm_gain_scale, d->norm_eps, p.xn, TRIBE_BF16, stream);
    if (rc) return rc;
    g = Linear(TRIBE_ROLE_FF1, M, p.xn, dim, L.w_ff1, L.b_ff1, p.hbuf, d->ff_inner, TRIBE_BF16).activation(TRIBE_ACT_GELU);
    allow_split_k(g, p.split_ws, p.split_bytes);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
    g = Linear(TRIBE_ROLE_FF2, M, p.hbuf, d->ff_inner, L.w_ff2, L.b_ff2, x, dim, TRIBE_F32).residual(x);
    g.res_scale = L.ff_res_scale;
    allow_split_k(g, p.split_ws, p.split_bytes);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
  }
  return tribe_scalenorm_fwd(x, M, dim, d->final_norm_g, d->norm_gain_scale, d->norm_eps, y, y_dtype, stream);
}
}  // namespace

extern "C" int tribe_encoder_extend_fwd(const tribe_encoder_desc* d, float* x, void* y, int32_t y_dtype, uint16_t* k_cache,
                                        uint16_t* v_cache, int64_t cap, int64_t pos, void* workspace, size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(d != nullptr, "tribe_encoder_extend_fwd: null descriptor");
  TRIBE_REQUIRE(d->T >= 1 && cap > 0 && pos >= 0 && pos + d->T <= cap,
                "tribe_encoder_extend_fwd: k=%lld positions from pos=%lld outside the cache capacity %lld (k >= 1, pos >= 0, pos + k <= cap)",
                (long long)d->T, (long long)pos, (long long)cap);
  return extend_body("tribe_encoder_extend_fwd", d, x, y, y_dtype, k_cache, v_cache, cap, pos, nullptr, workspace, workspace_bytes, stream);
}

// every sequence at a position of its own: pos int32 [B] on the device (-1 = takes no part)
extern "C" int tribe_encoder_extend_slots_fwd(const tribe_encoder_desc* d, float* x, void* y, int32_t y_dtype, uint16_t* k_cache,
                                              uint16_t* v_cache, int64_t cap, const int32_t* pos, void* workspace, size_t workspace_bytes,
                                              void* stream) {
  TRIBE_REQUIRE(d != nullptr, "tribe_encoder_extend_slots_fwd: null descriptor");
  TRIBE_REQUIRE(d->T >= 1 && cap > 0 && d->T <= cap,
                "tribe_encoder_extend_slots_fwd: k=%lld positions per sequence do not fit the cache capacity %lld (1 <= k <= cap)",
                (long long)d->T, (long long)cap);
  TRIBE_REQUIRE(pos != nullptr, "tribe_encoder_extend_slots_fwd: null pointer");
  return extend_body("tribe_encoder_extend_slots_fwd", d, x, y, y_dtype, k_cache, v_cache, cap, 0, pos, workspace, workspace_bytes, stream);
}

extern "C" int tribe_voxel_head_fwd(const uint16_t* x, int64_t B, int64_t T, int64_t C_pad, const uint16_t* w_packed, int64_t S,
                                    int64_t V, int64_t V_pad, const float* bias, const int64_t* subjects, float* y, void* stream) {
  TRIBE_REQUIRE(x && w_packed && subjects && y, "tribe_voxel_head_fwd: null pointer");
  TRIBE_REQUIRE(B > 0 && T > 0 && S > 0 && V > 0 && V_pad >= V && C_pad > 0, "tribe_voxel_head_fwd: bad shape");
  // y[b] (V x T) = W_s^T (V x C) . x_b^T (C x T): the T-contiguous output needs no transposed store,
  // and the per-subject weight is selected by the gather index instead of being materialised per sample
  // (the reference's index_select copies B x 12.3 MB, common.py:61).
  // the "input" of this Linear is the weight (rows = voxels, one bias per row) and its "weight" is x_b
  Linear d(TRIBE_ROLE_VOXEL_HEAD, V, w_packed, C_pad, x, nullptr, y, T, TRIBE_F32);
  d.batch1 = B; d.sA1 = V_pad * C_pad; d.gather1 = subjects; d.gather_a = 1;
  d.sB1 = T * C_pad; d.sC1 = V * T;
  if (bias) { d.bias = bias; d.bias_mode = TRIBE_BIAS_ROW; d.gather_bias = 1; d.sBias1 = V; }
  return tribe_gemm_bf16(&d, stream);
}
