// Frozen feature extractors as sequences of the path's own kernels:
// host-side orchestration only (no allocation, no sync), one C entry point per architecture.
//
// tribe_llama_fwd: transformers LlamaModel forward with output_hidden_states=True
// (data_utils/features/text.py:236-240 -> modeling_llama.py LlamaDecoderLayer: RMSNorm -> GQA attention with
// rotary (rotate_half) and a causal mask -> residual -> RMSNorm -> SwiGLU MLP -> residual), fused with the
// reference's per-word pooling of every hidden state (text.py:245-254: strip right padding, mean of the last
// len(word) positions) so that only [n_states, B, dim] floats leave the GPU instead of every hidden state.
#include "host_plan.h"

namespace {
struct LlamaLayout {
  int64_t M, qkv_w, q_w;
  float* x;        // [M, dim] residual stream
  uint16_t* xn;    // [M, dim] normed input of QKV / gate_up
  uint16_t* qkv;   // [M, qkv_w]
  uint16_t* ao;    // [M, q_w]
  uint16_t* act;   // [M, inter]
  float* fin;      // [M, dim] output of the final norm
  uint8_t* q8;     // fp8 only: one e4m3 staging buffer (every quantised input is consumed at once)
};
inline LlamaLayout layout(const tribe_llama_desc* d, Arena& ws) {
  LlamaLayout p;
  const int64_t M = p.M = d->B * d->T;
  p.q_w = (int64_t)d->heads_q * d->dim_head;
  p.qkv_w = (int64_t)(d->heads_q + 2 * d->heads_kv) * d->dim_head;
  p.x = ws.take<float>((size_t)M * d->dim * 4);
  p.xn = ws.take<uint16_t>((size_t)M * d->dim * 2);
  p.qkv = ws.take<uint16_t>((size_t)M * p.qkv_w * 2);
  p.ao = ws.take<uint16_t>((size_t)M * p.q_w * 2);
  p.act = ws.take<uint16_t>((size_t)M * d->inter * 2);
  p.fin = ws.take<float>((size_t)M * d->dim * 4);
  const int64_t widest = d->inter > p.q_w ? (d->inter > d->dim ? d->inter : d->dim) : (p.q_w > d->dim ? p.q_w : d->dim);
  p.q8 = d->fp8_host ? ws.take<uint8_t>((size_t)M * widest) : nullptr;
  return p;
}

// one Linear of an extractor layer: bf16 GEMM, or quantise the bf16 input with its static scale and run the e4m3 GEMM.
// `amax` (calibration, bf16 path only) and the fp8 fields come from the layer's descriptor; tribe_llama_fp8_layer and
// tribe_vit_fp8_layer share this layout: four weight pointers, four weight scales, four input scales.
struct Fp8Linear4 {
  const uint8_t* w[4];
  float w_scale[4];
  float in_scale[4];
};
static_assert(sizeof(Fp8Linear4) == sizeof(tribe_llama_fp8_layer) && sizeof(Fp8Linear4) == sizeof(tribe_vit_fp8_layer) &&
                  sizeof(Fp8Linear4) == sizeof(tribe_conformer_fp8_layer),
              "fp8 layer layouts");

// The pre-norm of a Linear (`b` and `layernorm`: LayerNorm, else RMSNorm): bf16 into `xn`, or, on the fp8 route, the e4m3 operand
// of that Linear straight into the staging buffer (one pass over x instead of norm -> bf16 -> quantise).  *q_in tells which.
inline int extractor_norm(const void* fp8_layers, int layer, int which, const float* x, int64_t rows, int64_t dim, const float* w,
                          const float* b, int layernorm, float eps, uint16_t* xn, uint8_t* q8, void* stream, bool* q_in) {
  const float in_scale = fp8_layers ? ((const Fp8Linear4*)fp8_layers)[layer].in_scale[which] : 0.f;
  *q_in = in_scale > 0.f;   // extractor_linear reports a missing scale
  if (*q_in) return tribe_norm_quantize_fp8_fwd(x, rows, dim, w, b, layernorm, eps, 1.0f / in_scale, q8, stream);
  return layernorm ? tribe_layernorm_fwd(x, rows, dim, w, b, eps, xn, TRIBE_BF16, stream)
                   : tribe_rmsnorm_fwd(x, rows, dim, w, eps, xn, TRIBE_BF16, stream);
}

// `g` is the bf16 Linear; the fp8 route swaps in the layer's e4m3 weight `which` and the staged input
inline int extractor_linear(const char* who, const void* fp8_layers, float* amax_out, int layer, int which, tribe_gemm_desc& g,
                            uint8_t* q8, void* stream, bool a_is_q8 = false) {
  if (amax_out) {
    int rc = tribe_absmax_fwd(g.A, TRIBE_BF16, g.M, g.K, g.lda, amax_out + (int64_t)layer * 4 + which, 1, stream);
    if (rc) return rc;
  }
  if (!fp8_layers) return tribe_gemm_bf16(&g, stream);
  const Fp8Linear4& F = ((const Fp8Linear4*)fp8_layers)[layer];
  TRIBE_REQUIRE(F.w[which] && F.in_scale[which] > 0.f && F.w_scale[which] > 0.f, "%s: layer %d fp8 weight %d or its scales missing", who, layer,
                which);
  if (!a_is_q8) {
    int rc = tribe_quantize_fp8_fwd(g.A, TRIBE_BF16, g.M, g.K, g.lda, 1.0f / F.in_scale[which], q8, g.K, stream);
    if (rc) return rc;
  }
  g.A = q8;
  g.B = F.w[which];
  g.alpha *= F.in_scale[which] * F.w_scale[which];   // on top of the caller's alpha (Conformer half-step FFN: 0.5)
  return tribe_gemm_fp8(&g, stream);
}
}  // namespace

extern "C" size_t tribe_llama_workspace_bytes(const tribe_llama_desc* d) {
  if (!d || d->B <= 0 || d->T <= 0) return 0;
  Arena ws;
  layout(d, ws);
  return ws.off;
}

namespace {
// The forward both Llama entry points run; they differ in `pool(src, state)` alone, which averages the f32 [B*T, dim] hidden state `src`
// into slot `state` (0 = embeddings ... depth = after the final RMSNorm) of the caller's output.
template <typename Pool>
int llama_forward(const char* who, const tribe_llama_desc* d, void* workspace, size_t workspace_bytes, void* stream, Pool pool) {
  TRIBE_REQUIRE(d->B > 0 && d->T > 0 && d->dim > 0 && d->depth >= 0 && d->heads_q > 0 && d->heads_kv > 0 && d->inter > 0,
                "%s: bad shape", who);
  TRIBE_REQUIRE(d->heads_q % d->heads_kv == 0, "%s: heads_q=%d not a multiple of heads_kv=%d", who, d->heads_q, d->heads_kv);
  TRIBE_REQUIRE(d->dim % 64 == 0 && d->inter % 64 == 0 && (d->heads_q * d->dim_head) % 64 == 0,
                "%s: dim, inter and heads_q*dim_head must be multiples of 64", who);
  TRIBE_REQUIRE(d->embed && d->ids && d->final_norm_w && d->cos_tab && d->sin_tab && (d->depth == 0 || d->layers_host),
                "%s: missing parameter pointer", who);
  TRIBE_REQUIRE(((uintptr_t)workspace % 256) == 0, "%s: workspace must be 256-byte aligned", who);
  Arena ws(workspace);
  const LlamaLayout p = layout(d, ws);
  TRIBE_REQUIRE(workspace_bytes >= ws.off, "%s: workspace too small", who);
  float *x = p.x, *fin = p.fin;
  uint16_t *xn = p.xn, *qkv = p.qkv, *ao = p.ao, *act = p.act;
  uint8_t* q8 = p.q8;
  const int64_t M = p.M, dim = d->dim;
  TRIBE_REQUIRE(!d->fp8_host || (d->dim % 128 == 0 && p.q_w % 128 == 0 && d->inter % 128 == 0),
                "%s: the fp8 path needs dim, heads_q * dim_head and inter to be multiples of 128", who);
  TRIBE_REQUIRE(!(d->fp8_host && d->amax_out), "%s: calibrate (amax_out) on the bf16 path, not together with fp8_host", who);
  // Linear `which` (0 qkv, 1 o, 2 gate_up, 3 down) of layer l on the bf16 or the fp8 route
  auto linear = [&](int l, int which, tribe_gemm_desc g, bool a_is_q8 = false) {
    return extractor_linear(who, d->fp8_host, d->amax_out, l, which, g, q8, stream, a_is_q8);
  };

  int rc = tribe_embedding_fwd(d->embed, d->embed_dtype, d->ids, M, dim, d->vocab, x, stream);
  if (rc) return rc;
  rc = pool(x, 0);
  if (rc) return rc;

  for (int l = 0; l < d->depth; ++l) {
    const tribe_llama_layer& L = d->layers_host[l];
    TRIBE_REQUIRE(L.input_norm_w && L.w_qkv && L.w_o && L.post_norm_w && L.w_gate_up && L.w_down,
                  "%s: layer %d has a null parameter", who, l);
    bool q_in = false;
    rc = extractor_norm(d->fp8_host, l, 0, x, M, dim, L.input_norm_w, nullptr, 0, d->rms_eps, xn, q8, stream, &q_in);
    if (rc) return rc;
    rc = linear(l, 0, Linear(TRIBE_ROLE_QKV, M, xn, dim, L.w_qkv, nullptr, qkv, p.qkv_w, TRIBE_BF16), q_in);
    if (rc) return rc;
    // rotate_half rotary over the full head dim on the q heads and the k heads (adjacent in the fused row)
    rc = tribe_rotary_fwd(qkv, M, d->T, p.qkv_w, d->heads_q + d->heads_kv, d->dim_head, d->dim_head, d->cos_tab, d->sin_tab, 0, stream);
    if (rc) return rc;
    tribe_attention_desc a = attn_zero();
    a.q = qkv; a.k = qkv + p.q_w; a.v = qkv + p.q_w + (int64_t)d->heads_kv * d->dim_head;
    a.ld_q = a.ld_k = a.ld_v = p.qkv_w;
    a.out = ao; a.ld_out = p.q_w;
    a.B = d->B; a.T = d->T; a.heads_q = d->heads_q; a.heads_kv = d->heads_kv; a.dim_head = d->dim_head;
    a.causal = 1;  // right padding + causal mask: real tokens never see pad keys, pad rows are never pooled
    a.scale = 1.0f / sqrtf((float)d->dim_head);
    rc = tribe_attention_fwd_ex(&a, stream);
    if (rc) return rc;
    rc = linear(l, 1, Linear(TRIBE_ROLE_OUT_PROJ, M, ao, p.q_w, L.w_o, nullptr, x, dim, TRIBE_F32).residual(x));
    if (rc) return rc;
    rc = extractor_norm(d->fp8_host, l, 2, x, M, dim, L.post_norm_w, nullptr, 0, d->rms_eps, xn, q8, stream, &q_in);
    if (rc) return rc;
    rc = linear(l, 2, Linear(TRIBE_ROLE_FF1, M, xn, dim, L.w_gate_up, nullptr, act, 2 * (int64_t)d->inter, TRIBE_BF16)
                          .activation(TRIBE_ACT_SWIGLU, d->inter), q_in);
    if (rc) return rc;
    rc = linear(l, 3, Linear(TRIBE_ROLE_FF2, M, act, d->inter, L.w_down, nullptr, x, dim, TRIBE_F32).residual(x));
    if (rc) return rc;
    if (l + 1 < d->depth) {
      rc = pool(x, l + 1);
      if (rc) return rc;
    }
  }
  // the last hidden state is the output of the final RMSNorm (LlamaModel.norm)
  if (d->depth > 0) {
    rc = tribe_rmsnorm_fwd(x, M, dim, d->final_norm_w, d->rms_eps, fin, TRIBE_F32, stream);
    if (rc) return rc;
    rc = pool(fin, d->depth);
  }
  return rc;
}
}  // namespace

extern "C" int tribe_llama_fwd(const tribe_llama_desc* d, float* states, void* workspace, size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(d && states && workspace, "tribe_llama_fwd: null pointer");
  return llama_forward("tribe_llama_fwd", d, workspace, workspace_bytes, stream, [&](const float* src, int state) {
    return tribe_segment_mean_fwd(src, d->B, d->T, d->dim, d->pool_start, d->pool_len, states + (int64_t)state * d->B * d->dim, d->dim, stream);
  });
}

// the same workspace: the window list changes what is pooled, not what is computed
extern "C" size_t tribe_llama_windows_workspace_bytes(const tribe_llama_desc* d) { return tribe_llama_workspace_bytes(d); }

extern "C" int tribe_llama_windows_fwd(const tribe_llama_desc* d, const int64_t* win_row, const int64_t* win_start, const int64_t* win_len,
                                       int64_t W, float* states, void* workspace, size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(d && win_row && win_start && win_len && states && workspace, "tribe_llama_windows_fwd: null pointer");
  TRIBE_REQUIRE(W > 0, "tribe_llama_windows_fwd: W=%lld windows", (long long)W);
  return llama_forward("tribe_llama_windows_fwd", d, workspace, workspace_bytes, stream, [&](const float* src, int state) {
    return tribe_window_mean_fwd(src, d->B, d->T, d->dim, win_row, win_start, win_len, W, states + (int64_t)state * W * d->dim, d->dim, stream);
  });
}

// ---------------------------------------------------------------------------------------------------------------
// tribe_vjepa2_fwd: transformers VJEPA2Model encoder (data_utils/features/video.py:239-274 -> modeling_vjepa2.py
// VJEPA2Encoder: Conv3d tubelet patch embedding -> depth x [LayerNorm -> q/k/v Linear(+bias) -> 3-D rotary ->
// bidirectional attention -> proj + residual -> LayerNorm -> fc1 + GELU -> fc2 + residual]); every hidden state
// (embeddings + each layer output, NOT the final LayerNorm) is averaged over tokens (video.py:228).
// ---------------------------------------------------------------------------------------------------------------
namespace {
struct VitLayout {
  int64_t tokens, M;
  float* x;        // [M, dim] residual stream
  uint16_t* xn;    // [M, dim]
  uint16_t* qkv;   // [M, 3*dim]
  uint16_t* ao;    // [M, dim]
  uint16_t* act;   // [M, mlp]
  uint16_t* col;   // [M, K_pad] im2col rows, over act: dead once the embedding GEMM ran
  uint8_t* q8;     // fp8 only: e4m3 staging of one GEMM input
};
inline VitLayout layout(const tribe_vjepa2_desc* d, Arena& ws) {
  VitLayout p;
  p.tokens = (int64_t)(d->frames / d->tubelet) * (d->height / d->patch) * (d->width / d->patch);
  const int64_t M = p.M = d->B * p.tokens;
  p.x = ws.take<float>((size_t)M * d->dim * 4);
  p.xn = ws.take<uint16_t>((size_t)M * d->dim * 2);
  p.qkv = ws.take<uint16_t>((size_t)M * 3 * d->dim * 2);
  p.ao = ws.take<uint16_t>((size_t)M * d->dim * 2);
  p.act = p.col = ws.take<uint16_t>((size_t)M * (d->mlp > d->K_pad ? d->mlp : d->K_pad) * 2);
  p.q8 = d->fp8_host ? ws.take<uint8_t>((size_t)M * (d->mlp > d->dim ? d->mlp : d->dim)) : nullptr;
  return p;
}
}  // namespace

extern "C" size_t tribe_vjepa2_workspace_bytes(const tribe_vjepa2_desc* d) {
  if (!d || d->B <= 0 || d->tubelet <= 0 || d->patch <= 0) return 0;
  Arena ws;
  layout(d, ws);
  return ws.off;
}

extern "C" int tribe_vjepa2_fwd(const tribe_vjepa2_desc* d, float* states, void* workspace, size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(d && states && workspace, "tribe_vjepa2_fwd: null pointer");
  TRIBE_REQUIRE(d->B > 0 && d->dim > 0 && d->depth >= 0 && d->heads > 0 && d->mlp > 0, "tribe_vjepa2_fwd: bad shape");
  TRIBE_REQUIRE(d->heads * d->dim_head == d->dim && d->dim % 64 == 0 && d->mlp % 64 == 0 && d->K_pad % 64 == 0,
                "tribe_vjepa2_fwd: dim = heads * dim_head, and dim / mlp / K_pad must be multiples of 64");
  TRIBE_REQUIRE(d->pixels && d->w_patch && d->cos_tab && d->sin_tab && (d->depth == 0 || d->layers_host),
                "tribe_vjepa2_fwd: missing parameter pointer");
  Arena ws(workspace);
  const VitLayout p = layout(d, ws);
  TRIBE_REQUIRE(((uintptr_t)workspace % 256) == 0 && workspace_bytes >= ws.off, "tribe_vjepa2_fwd: workspace too small or misaligned");
  float* x = p.x;
  uint16_t *xn = p.xn, *qkv = p.qkv, *ao = p.ao, *act = p.act;
  uint8_t* q8 = p.q8;
  const int64_t M = p.M, dim = d->dim, BD = d->B * dim;
  TRIBE_REQUIRE(!d->fp8_host || (d->dim % 128 == 0 && d->mlp % 128 == 0), "tribe_vjepa2_fwd: the fp8 path needs dim and mlp to be multiples of 128");
  TRIBE_REQUIRE(!(d->fp8_host && d->amax_out), "tribe_vjepa2_fwd: calibrate (amax_out) on the bf16 path, not together with fp8_host");
  // Linear `which` (0 qkv, 1 proj, 2 fc1, 3 fc2) of layer l on the bf16 or the fp8 route
  auto linear = [&](int l, int which, tribe_gemm_desc g, bool a_is_q8 = false) {
    return extractor_linear("tribe_vjepa2_fwd", d->fp8_host, d->amax_out, l, which, g, q8, stream, a_is_q8);
  };

  int rc = tribe_im2col3d_fwd(d->pixels, d->B, d->frames, d->chans, d->height, d->width, d->tubelet, d->patch, p.col, d->K_pad, stream);
  if (rc) return rc;
  const Linear embed(TRIBE_ROLE_PROJECTOR, M, p.col, d->K_pad, d->w_patch, d->b_patch, x, dim, TRIBE_F32);
  rc = tribe_gemm_bf16(&embed, stream);
  if (rc) return rc;
  rc = tribe_segment_mean_fwd(x, d->B, p.tokens, dim, nullptr, nullptr, states, dim, stream);
  if (rc) return rc;

  for (int l = 0; l < d->depth; ++l) {
    const tribe_vit_layer& L = d->layers_host[l];
    TRIBE_REQUIRE(L.norm1_w && L.w_qkv && L.w_proj && L.norm2_w && L.w_fc1 && L.w_fc2, "tribe_vjepa2_fwd: layer %d has a null parameter", l);
    bool q_in = false;
    rc = extractor_norm(d->fp8_host, l, 0, x, M, dim, L.norm1_w, L.norm1_b, 1, d->ln_eps, xn, q8, stream, &q_in);
    if (rc) return rc;
    rc = linear(l, 0, Linear(TRIBE_ROLE_QKV, M, xn, dim, L.w_qkv, L.b_qkv, qkv, 3 * dim, TRIBE_BF16), q_in);
    if (rc) return rc;
    rc = tribe_rotary_fwd(qkv, M, p.tokens, 3 * dim, 2 * d->heads, d->dim_head, d->dim_head, d->cos_tab, d->sin_tab, 2, stream);
    if (rc) return rc;
    tribe_attention_desc a = attn_zero();
    a.q = qkv; a.k = qkv + dim; a.v = qkv + 2 * dim;
    a.ld_q = a.ld_k = a.ld_v = 3 * dim;
    a.out = ao; a.ld_out = dim;
    a.B = d->B; a.T = p.tokens; a.heads_q = d->heads; a.heads_kv = d->heads; a.dim_head = d->dim_head;
    a.scale = 1.0f / sqrtf((float)d->dim_head);
    rc = tribe_attention_fwd_ex(&a, stream);
    if (rc) return rc;
    rc = linear(l, 1, Linear(TRIBE_ROLE_OUT_PROJ, M, ao, dim, L.w_proj, L.b_proj, x, dim, TRIBE_F32).residual(x));
    if (rc) return rc;
    rc = extractor_norm(d->fp8_host, l, 2, x, M, dim, L.norm2_w, L.norm2_b, 1, d->ln_eps, xn, q8, stream, &q_in);
    if (rc) return rc;
    rc = linear(l, 2, Linear(TRIBE_ROLE_FF1, M, xn, dim, L.w_fc1, L.b_fc1, act, d->mlp, TRIBE_BF16).activation(TRIBE_ACT_GELU), q_in);
    if (rc) return rc;
    rc = linear(l, 3, Linear(TRIBE_ROLE_FF2, M, act, d->mlp, L.w_fc2, L.b_fc2, x, dim, TRIBE_F32).residual(x));
    if (rc) return rc;
    rc = tribe_segment_mean_fwd(x, d->B, p.tokens, dim, nullptr, nullptr, states + (int64_t)(l + 1) * BD, dim, stream);
    if (rc) return rc;
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// tribe_w2vbert_fwd: transformers Wav2Vec2BertModel (data_utils/features/audio.py:253-263 -> modeling_wav2vec2_bert.py):
// feature projection (LayerNorm + Linear), then depth x conformer block [half-step FFN (swish) -> self-attention with
// "relative_key" position bias -> convolution module (pointwise + GLU, causal depthwise k=31, LayerNorm, swish,
// pointwise) -> half-step FFN -> LayerNorm]; every hidden state is resampled along time by row gather
// (F.interpolate nearest, audio.py:163-171).
// ---------------------------------------------------------------------------------------------------------------
namespace {
struct W2vLayout {
  int64_t M, qe_ld;
  int qe_stride_h;   // columns of `qe` per head: the rel_left + rel_right + 1 distances, padded to a multiple of 8
  float* x;          // [M, dim] residual stream
  uint16_t* xn;      // [M, dim]
  uint16_t* wide;    // [M, max(inter, 3*dim)]: FFN hidden  |  qkv
  float* qe;         // [M, qe_ld] q . distance_embedding^T
  uint16_t* ao;      // [M, dim]
  uint16_t* glu;     // [M, dim]
  float* feat;       // [M, feat_dim] normed input features
  uint16_t* featp;   // [M, feat_pad] the same, bf16, K zero padded
  uint8_t* q8;       // fp8 only: e4m3 staging of one GEMM input
};
inline W2vLayout layout(const tribe_w2vbert_desc* d, Arena& ws) {
  W2vLayout p;
  const int64_t M = p.M = d->B * d->T;
  p.qe_stride_h = (d->rel_left + d->rel_right + 1 + 7) / 8 * 8;
  p.qe_ld = (int64_t)d->heads * p.qe_stride_h;
  p.x = ws.take<float>((size_t)M * d->dim * 4);
  p.xn = ws.take<uint16_t>((size_t)M * d->dim * 2);
  p.wide = ws.take<uint16_t>((size_t)M * (d->inter > 3 * d->dim ? d->inter : 3 * d->dim) * 2);
  p.qe = ws.take<float>((size_t)M * p.qe_ld * 4);
  p.ao = ws.take<uint16_t>((size_t)M * d->dim * 2);
  p.glu = ws.take<uint16_t>((size_t)M * d->dim * 2);
  p.feat = ws.take<float>((size_t)M * d->feat_dim * 4);
  p.featp = ws.take<uint16_t>((size_t)M * d->feat_pad * 2);
  p.q8 = d->fp8_host ? ws.take<uint8_t>((size_t)M * (d->inter > d->dim ? d->inter : d->dim)) : nullptr;
  return p;
}
}  // namespace

extern "C" size_t tribe_w2vbert_workspace_bytes(const tribe_w2vbert_desc* d) {
  if (!d || d->B <= 0 || d->T <= 0) return 0;
  Arena ws;
  layout(d, ws);
  return ws.off;
}

extern "C" int tribe_w2vbert_fwd(const tribe_w2vbert_desc* d, float* states, void* workspace, size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(d && states && workspace, "tribe_w2vbert_fwd: null pointer");
  TRIBE_REQUIRE(d->B > 0 && d->T > 0 && d->dim > 0 && d->depth >= 0 && d->heads > 0 && d->inter > 0 && d->n_out > 0, "tribe_w2vbert_fwd: bad shape");
  TRIBE_REQUIRE(d->heads * d->dim_head == d->dim && d->dim_head == 64, "tribe_w2vbert_fwd: head size must be 64 (relative_key attention kernel)");
  TRIBE_REQUIRE(d->dim % 64 == 0 && d->inter % 64 == 0 && d->feat_pad % 64 == 0 && d->feat_pad >= d->feat_dim && d->feat_dim % 4 == 0,
                "tribe_w2vbert_fwd: dim / inter / feat_pad must be multiples of 64");
  TRIBE_REQUIRE(d->features && d->fp_ln_w && d->fp_ln_b && d->w_fp && d->out_index && (d->depth == 0 || d->layers_host),
                "tribe_w2vbert_fwd: missing parameter pointer");
  Arena ws(workspace);
  const W2vLayout p = layout(d, ws);
  TRIBE_REQUIRE(((uintptr_t)workspace % 256) == 0 && workspace_bytes >= ws.off, "tribe_w2vbert_fwd: workspace too small or misaligned");
  float *x = p.x, *qe = p.qe;
  uint16_t *xn = p.xn, *wide = p.wide, *ao = p.ao, *glu = p.glu;
  uint8_t* q8 = p.q8;
  TRIBE_REQUIRE(!d->fp8_host || (d->dim % 128 == 0 && d->inter % 128 == 0), "tribe_w2vbert_fwd: the fp8 path needs dim and inter to be multiples of 128");
  TRIBE_REQUIRE(!(d->fp8_host && d->amax_out), "tribe_w2vbert_fwd: calibrate (amax_out) on the bf16 path, not together with fp8_host");
  const int64_t M = p.M, dim = d->dim;
  const int64_t state_sz = d->B * d->n_out * dim;

  // feature projection: LayerNorm(feat_dim) -> Linear
  int rc = tribe_layernorm_fwd(d->features, M, d->feat_dim, d->fp_ln_w, d->fp_ln_b, d->ln_eps, p.feat, TRIBE_F32, stream);
  if (rc) return rc;
  rc = tribe_pack_weight_bf16(p.feat, M, d->feat_dim, d->feat_dim, p.featp, M, d->feat_pad, stream);  // cast + zero-pad K
  if (rc) return rc;
  tribe_gemm_desc g = Linear(TRIBE_ROLE_PROJECTOR, M, p.featp, d->feat_pad, d->w_fp, d->b_fp, x, dim, TRIBE_F32);
  rc = tribe_gemm_bf16(&g, stream);
  if (rc) return rc;
  rc = tribe_gather_rows_fwd(x, d->B, d->T, dim, d->out_index, d->n_out, states, stream);
  if (rc) return rc;

  // half-step feed-forward x += 0.5 * (swish(LN(x) W_in^T + b_in) W_out^T + b_out); `which` = 0 (ffn1) or 2 (ffn2) selects the pair of e4m3
  // weights / scales of the layer when fp8_host is set (the LayerNorm then writes the e4m3 operand directly)
  auto ffn = [&](int l, int which, const float* ln_w, const float* ln_b, const uint16_t* w_in, const float* b_in, const uint16_t* w_out,
                 const float* b_out_half) -> int {
    bool q_in = false;
    int r = extractor_norm(d->fp8_host, l, which, x, M, dim, ln_w, ln_b, 1, d->ln_eps, xn, q8, stream, &q_in);
    if (r) return r;
    tribe_gemm_desc q = Linear(TRIBE_ROLE_FF1, M, xn, dim, w_in, b_in, wide, d->inter, TRIBE_BF16).activation(TRIBE_ACT_SILU);
    r = extractor_linear("tribe_w2vbert_fwd", d->fp8_host, d->amax_out, l, which, q, q8, stream, q_in);
    if (r) return r;
    q = Linear(TRIBE_ROLE_FF2, M, wide, d->inter, w_out, b_out_half, x, dim, TRIBE_F32).residual(x).scaled(0.5f);  // x = 0.5 * (h W^T + b) + x
    return extractor_linear("tribe_w2vbert_fwd", d->fp8_host, d->amax_out, l, which + 1, q, q8, stream);
  };

  for (int l = 0; l < d->depth; ++l) {
    const tribe_conformer_layer& L = d->layers_host[l];
    TRIBE_REQUIRE(L.ffn1_ln_w && L.w_ffn1_in && L.w_ffn1_out && L.attn_ln_w && L.w_qkv && L.dist_emb && L.w_attn_out && L.conv_ln_w &&
                      L.w_pw1 && L.w_dw_kc && L.dw_ln_w && L.w_pw2 && L.ffn2_ln_w && L.w_ffn2_in && L.w_ffn2_out && L.final_ln_w,
                  "tribe_w2vbert_fwd: layer %d has a null parameter", l);
    // 1. half-step feed-forward
    rc = ffn(l, 0, L.ffn1_ln_w, L.ffn1_ln_b, L.w_ffn1_in, L.b_ffn1_in, L.w_ffn1_out, L.b_ffn1_out_half);
    if (rc) return rc;
    // 2. self-attention with relative_key bias
    rc = tribe_layernorm_fwd(x, M, dim, L.attn_ln_w, L.attn_ln_b, d->ln_eps, xn, TRIBE_BF16, stream);
    if (rc) return rc;
    uint16_t* qkv = wide;
    g = Linear(TRIBE_ROLE_QKV, M, xn, dim, L.w_qkv, L.b_qkv, qkv, 3 * dim, TRIBE_BF16);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
    // qe[row][h][p] = q[row][h][:] . dist_emb[p][:]: one Linear per head (batch0) on the head's slice of the fused row
    g = Linear(TRIBE_ROLE_ATTN_SCORES, M, qkv, d->dim_head, L.dist_emb, nullptr, qe, d->rel_left + d->rel_right + 1, TRIBE_F32);
    g.batch0 = d->heads;
    g.lda = 3 * dim; g.sA0 = d->dim_head;
    g.ldc = p.qe_ld; g.sC0 = p.qe_stride_h;
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
    tribe_attention_desc a = attn_zero();
    a.q = qkv; a.k = qkv + dim; a.v = qkv + 2 * dim;
    a.ld_q = a.ld_k = a.ld_v = 3 * dim;
    a.out = ao; a.ld_out = dim;
    a.B = d->B; a.T = d->T; a.heads_q = d->heads; a.heads_kv = d->heads; a.dim_head = d->dim_head;
    a.scale = 1.0f / sqrtf((float)d->dim_head);
    a.rel_qe = qe; a.ld_rel_qe = p.qe_ld; a.rel_stride_h = p.qe_stride_h; a.rel_left = d->rel_left; a.rel_right = d->rel_right;
    rc = tribe_attention_fwd_ex(&a, stream);
    if (rc) return rc;
    g = Linear(TRIBE_ROLE_OUT_PROJ, M, ao, dim, L.w_attn_out, L.b_attn_out, x, dim, TRIBE_F32).residual(x);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
    // 3. convolution module
    rc = tribe_layernorm_fwd(x, M, dim, L.conv_ln_w, L.conv_ln_b, d->ln_eps, xn, TRIBE_BF16, stream);
    if (rc) return rc;
    g = Linear(TRIBE_ROLE_GENERIC, M, xn, dim, L.w_pw1, nullptr, glu, 2 * dim, TRIBE_BF16).activation(TRIBE_ACT_GLU, dim);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
    rc = tribe_dwconv_ln_swish_fwd(glu, d->B, d->T, (int32_t)dim, d->conv_kernel, L.w_dw_kc, L.dw_ln_w, L.dw_ln_b, d->ln_eps, xn, stream);
    if (rc) return rc;
    g = Linear(TRIBE_ROLE_GENERIC, M, xn, dim, L.w_pw2, nullptr, x, dim, TRIBE_F32).residual(x);
    rc = tribe_gemm_bf16(&g, stream);
    if (rc) return rc;
    // 4. half-step feed-forward, then the block's final LayerNorm (in place on the residual stream)
    rc = ffn(l, 2, L.ffn2_ln_w, L.ffn2_ln_b, L.w_ffn2_in, L.b_ffn2_in, L.w_ffn2_out, L.b_ffn2_out_half);
    if (rc) return rc;
    rc = tribe_layernorm_fwd(x, M, dim, L.final_ln_w, L.final_ln_b, d->ln_eps, x, TRIBE_F32, stream);
    if (rc) return rc;
    rc = tribe_gather_rows_fwd(x, d->B, d->T, dim, d->out_index, d->n_out, states + (int64_t)(l + 1) * state_sz, stream);
    if (rc) return rc;
  }
  return 0;
}
