// Streaming a causal encoder one position at a time: the KV cache and single-query ("decode") attention.
//
// Cache: per layer two bf16 tensors K, V [B, heads, cap, dim_head] -- every (sequence, head) owns one contiguous run of keys, so a step's
// attention streams 2 * n * dim_head * 2 bytes per head front to back.
//   kv_append_kernel  T positions per sequence (a step: T = 1; a block append: T = k): rotates the q heads (in place) and the k heads of
//                     the fused qkv row b * T + t at position pos + t with rotary_kernel's arithmetic (rotary_pairs.h) and stores k and v
//                     into slot pos + t.
//   kv_fill_kernel    a prefill's T positions: copies the already rotated k heads and the v heads of a fused [B*T, 3*inner] buffer into
//                     slots 0 .. T-1.
//   attn_decode_split_kernel<DH> / attn_decode_combine_kernel   out = softmax(scale q K[0:n]^T) V[0:n] per (b, h).
//
// The attention is VALU, not MFMA: with one query row an MFMA tile would be 1/16 used, and the kernel is bound by the cache bytes either
// way -- per key and lane 2 * DH / 8 multiply-adds and as many bf16 -> f32 shifts against 2 * DH * 2 bytes, an order of magnitude under
// the vector rate that would make it compute-bound.  K and V go straight from global memory to registers (every byte is used once; LDS
// would only add a trip).  Eight lanes share a key: lane j of the group owns the 16-byte pieces j, j + 8, ... of the row, so one load
// instruction of a wave covers eight consecutive keys in 128-byte segments, and a dot product closes with three cross-lane adds.  Each
// group runs an online softmax (f32, base 2) over U keys at a time -- K and V of all U are requested before the first score is needed --
// with p rounded to bf16 before it multiplies V, as in the flash kernels.
// The keys of one (b, h) are split over `splits` workgroups (tribe_attention_decode_splits: a function of B, heads and n alone) so that a
// single sequence still fills the chip.  Groups, waves and splits are merged in a fixed order -- cross-lane butterflies, then LDS, then
// f32 (m, l, o) parts in the workspace summed by a second launch -- no atomics: the same call gives the same bits.  A key at or beyond n is
// never loaded.
#include "host_plan.h"
#include "rotary_pairs.h"
#include <type_traits>

namespace {

constexpr float DECODE_M_EMPTY = -1.0e30f;   // running maximum of a part that has seen no key: finite, so exp2(m - M) is 0, never NaN
constexpr int DECODE_MAX_SPLITS = 32;
constexpr int DECODE_MIN_KEYS = 64;          // keys per split at least: one pass of the four waves at U = 2

// Pos = int64_t: every sequence starts at position pos0 (tribe_kv_append, tribe_kv_append_block).  Pos = const int32_t*: the slot form
// (tribe_kv_append_slots) -- sequence b starts at pos0[b], and one whose value lies outside [0, cap - T] takes no part: neither its cache
// run nor its qkv rows are touched.  The argument has the same size either way, so the int64_t form is the kernel it was.
template <class Pos>
__global__ __launch_bounds__(256) void kv_append_kernel(unsigned short* __restrict__ qkv, int64_t B, int64_t T, int heads, int dim_head,
                                                        int rot_dim, int interleaved, const float* __restrict__ cos_tab,
                                                        const float* __restrict__ sin_tab, Pos pos0, unsigned short* __restrict__ kc,
                                                        unsigned short* __restrict__ vc, int64_t cap) {
  constexpr bool SLOTS = std::is_pointer<Pos>::value;
  const int half = rot_dim >> 1;
  const int items_per_head = dim_head >> 3;   // 8 elements each
  const int rot_items = rot_dim >> 3;
  const int64_t inner = (int64_t)heads * dim_head;
  const int64_t total = B * T * 3 * heads * items_per_head;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = idx;
    const int it = (int)(t % items_per_head); t /= items_per_head;
    const int hh = (int)(t % (3 * heads));
    const int64_t row = t / (3 * heads);                // b * T + step
    const int64_t b = row / T;
    int64_t first;
    if constexpr (SLOTS) {
      first = pos0[b];
      if (first < 0 || first > cap - T) continue;   // takes no part, or out of range: treated the same
    } else {
      first = pos0;
    }
    const int64_t pos = first + (row - b * T);
    const int sec = hh / heads, h = hh - sec * heads;   // 0 q, 1 k, 2 v
    unsigned short* base = qkv + row * 3 * inner + (int64_t)hh * dim_head;
    unsigned short* slot = (sec == 1 ? kc : vc) + ((b * heads + h) * cap + pos) * dim_head;
    if (sec == 2 || it >= rot_items) {   // not rotated: v, and the tail of q / k
      if (sec != 0) *(u16x8_t*)(slot + it * 8) = *(const u16x8_t*)(base + it * 8);
      continue;
    }
    const float4 c = *(const float4*)(cos_tab + pos * half + it * 4);
    const float4 s = *(const float4*)(sin_tab + pos * half + it * 4);
    const float cs[4] = {c.x, c.y, c.z, c.w}, sn[4] = {s.x, s.y, s.z, s.w};
    if (interleaved) {
      u16x8_t v = *(u16x8_t*)(base + it * 8);
      rotate_interleaved8(v, cs, sn);
      *(u16x8_t*)(base + it * 8) = v;
      if (sec == 1) *(u16x8_t*)(slot + it * 8) = v;
    } else {   // half-split pairs sit rot_dim / 2 apart: two 8-byte pieces, as in rotary_kernel
      u16x4_t lo = *(u16x4_t*)(base + it * 4), hi = *(u16x4_t*)(base + half + it * 4);
      rotate_split4(lo, hi, cs, sn);
      *(u16x4_t*)(base + it * 4) = lo;
      *(u16x4_t*)(base + half + it * 4) = hi;
      if (sec == 1) {
        *(u16x4_t*)(slot + it * 4) = lo;
        *(u16x4_t*)(slot + half + it * 4) = hi;
      }
    }
  }
}

__global__ __launch_bounds__(256) void kv_fill_kernel(const unsigned short* __restrict__ qkv, int64_t B, int64_t T, int heads, int dim_head,
                                                      unsigned short* __restrict__ kc, unsigned short* __restrict__ vc, int64_t cap) {
  const int items_per_head = dim_head >> 3;
  const int64_t inner = (int64_t)heads * dim_head;
  const int64_t total = B * T * 2 * heads * items_per_head;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = idx;
    const int it = (int)(t % items_per_head); t /= items_per_head;
    const int hh = (int)(t % (2 * heads)); t /= 2 * heads;
    const int64_t pos = t % T, b = t / T;
    const int sec = hh / heads, h = hh - sec * heads;   // 0 k, 1 v
    const unsigned short* src = qkv + (b * T + pos) * 3 * inner + inner + (int64_t)hh * dim_head + it * 8;
    unsigned short* dst = (sec ? vc : kc) + ((b * heads + h) * cap + pos) * dim_head + it * 8;
    *(u16x8_t*)dst = *(const u16x8_t*)src;
  }
}

// merge of (m, l, o) parts in index order; `get(i, &m, &l, &o)` reads part i.  The compiler contracts `L += l * w` into a fused
// multiply-add in the uniform kernels; FUSED states that arithmetic outright for the slot forms, where it would otherwise leave some of
// the products unfused (seen at dim_head 384) and the two forms would round differently.
template <bool FUSED = false, class Get>
__device__ __forceinline__ void merge_parts(int n_parts, Get get, float* M_out, float* L_out, float* O_out) {
  float M = DECODE_M_EMPTY;
  for (int i = 0; i < n_parts; ++i) { float m, l, o; get(i, &m, &l, &o); M = fmaxf(M, m); }
  float L = 0.f, O = 0.f;
  for (int i = 0; i < n_parts; ++i) {
    float m, l, o;
    get(i, &m, &l, &o);
    const float w = exp2f(m - M);
    if (FUSED) {
      L = fmaf(l, w, L);
      O = fmaf(o, w, O);
    } else {
      L += l * w;
      O += o * w;
    }
  }
  *M_out = M; *L_out = L; *O_out = O;
}

// grid (splits, heads, B); split s owns keys [s * chunk, min(n, (s + 1) * chunk)).  splits == 1: writes `out`; else part (m, l) to ws_ml
// and o to ws_o, part index (b * heads + h) * splits + s.
// SLOTS: a key count per sequence (tribe_attention_decode_slots_fwd).  n is the host's upper bound n_max; sequence b holds
// n_b = min(pos_slots[b] + 1, n) keys, or none when pos_slots[b] lies outside [0, cap - 1] (inactive).  A split whose range starts at or
// beyond n_b loads nothing and hands on the empty part (DECODE_M_EMPTY, 0, 0); a row whose parts are all empty is written as +0.
template <int DH, int SLOTS>
__global__ __launch_bounds__(256) void attn_decode_split_kernel(const unsigned short* __restrict__ q, int64_t ld_q,
                                                                const unsigned short* __restrict__ kc,
                                                                const unsigned short* __restrict__ vc, int heads, int64_t cap, int64_t n,
                                                                int64_t chunk, int splits, float scale_log2e, float* __restrict__ ws_ml,
                                                                float* __restrict__ ws_o, unsigned short* __restrict__ out,
                                                                const int32_t* __restrict__ pos_slots) {
  constexpr int CH = DH / 64;            // 16-byte pieces per lane and key
  constexpr int U = CH <= 2 ? 4 : 2;     // keys per group in flight
  __shared__ float sh_ml[4][2];
  __shared__ float sh_o[4][DH];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 3, j = lane & 7;
  const int s = blockIdx.x, h = blockIdx.y;
  const int64_t b = blockIdx.z;
  int64_t nb = n;
  if (SLOTS) {
    const int64_t p = pos_slots[b];
    nb = (p < 0 || p >= cap) ? 0 : (p + 1 < n ? p + 1 : n);
  }
  const int64_t k0 = (int64_t)s * chunk, k1 = (k0 + chunk < nb) ? k0 + chunk : nb;
  const unsigned short* qrow = q + b * ld_q + (int64_t)h * DH;
  const unsigned short* krun = kc + (b * heads + h) * cap * DH;
  const unsigned short* vrun = vc + (b * heads + h) * cap * DH;

  float qf[CH][8];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const u16x8_t v = *(const u16x8_t*)(qrow + (c * 8 + j) * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) qf[c][e] = bf16_to_f32(v[e]);
  }
  float acc[CH][8];
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[c][e] = 0.f;
  float m = DECODE_M_EMPTY, l = 0.f;

  for (int64_t base = k0 + (int64_t)w * 8 * U; base < k1; base += 4 * 8 * U) {   // wave-uniform bounds
    u16x8_t kk[U][CH], vv[U][CH];
    bool valid[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t key = base + u * 8 + g;
      valid[u] = key < k1;
#pragma unroll
      for (int c = 0; c < CH; ++c) { kk[u][c] = (u16x8_t)0; vv[u][c] = (u16x8_t)0; }
      if (valid[u]) {   // a key at or beyond n is not read
#pragma unroll
        for (int c = 0; c < CH; ++c) kk[u][c] = *(const u16x8_t*)(krun + key * DH + (c * 8 + j) * 8);
#pragma unroll
        for (int c = 0; c < CH; ++c) vv[u][c] = *(const u16x8_t*)(vrun + key * DH + (c * 8 + j) * 8);
      }
    }
    float sc[U];
    float m_new = m;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float d = 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) d += qf[c][e] * bf16_to_f32(kk[u][c][e]);
      d += __shfl_xor(d, 1, 64);
      d += __shfl_xor(d, 2, 64);
      d += __shfl_xor(d, 4, 64);
      sc[u] = d * scale_log2e;
      if (valid[u]) m_new = fmaxf(m_new, sc[u]);
    }
    const float alpha = exp2f(m - m_new);
    m = m_new;
    l *= alpha;
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[c][e] *= alpha;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float p = valid[u] ? exp2f(sc[u] - m) : 0.f;
      l += p;
      const float pb = bf16_to_f32(f32_to_bf16(p));   // P enters the PV product as bf16
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[c][e] += pb * bf16_to_f32(vv[u][c][e]);
    }
  }

  // the eight groups of a wave (lanes j, j + 8, ...): butterflies over lane bits 3..5
  float M = m;
  M = fmaxf(M, __shfl_xor(M, 8, 64));
  M = fmaxf(M, __shfl_xor(M, 16, 64));
  M = fmaxf(M, __shfl_xor(M, 32, 64));
  const float wg = exp2f(m - M);
  l *= wg;
#pragma unroll
  for (int off = 8; off < 64; off <<= 1) l += __shfl_xor(l, off, 64);
#pragma unroll
  for (int c = 0; c < CH; ++c)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float a = acc[c][e] * wg;
#pragma unroll
      for (int off = 8; off < 64; off <<= 1) a += __shfl_xor(a, off, 64);
      acc[c][e] = a;
    }
  if (g == 0) {
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int e = 0; e < 8; ++e) sh_o[w][(c * 8 + j) * 8 + e] = acc[c][e];
    if (j == 0) { sh_ml[w][0] = M; sh_ml[w][1] = l; }
  }
  __syncthreads();
  // the four waves, in order
  const int64_t part = (b * heads + h) * splits + s;
  for (int t = tid; t < DH; t += 256) {
    float Mw, Lw, Ow;
    merge_parts<SLOTS != 0>(4, [&](int i, float* pm, float* pl, float* po) { *pm = sh_ml[i][0]; *pl = sh_ml[i][1]; *po = sh_o[i][t]; }, &Mw, &Lw,
                            &Ow);
    if (splits == 1) {
      if (SLOTS && !(Lw > 0.f)) Lw = 1.f;   // no key (Ow is 0): +0, not 0 / 0
      out[(b * heads + h) * DH + t] = f32_to_bf16(Ow / Lw);
    } else {
      ws_o[part * DH + t] = Ow;
      if (t == 0) { ws_ml[part * 2] = Mw; ws_ml[part * 2 + 1] = Lw; }
    }
  }
}

// grid (heads, B): the parts of one (b, h), in split order.  SLOTS: a row without a key (every part empty, L = 0) is written as +0.
template <int SLOTS>
__global__ __launch_bounds__(256) void attn_decode_combine_kernel(const float* __restrict__ ws_ml, const float* __restrict__ ws_o, int heads,
                                                                  int dim_head, int splits, unsigned short* __restrict__ out) {
  const int64_t bh = (int64_t)blockIdx.y * heads + blockIdx.x;
  const float* ml = ws_ml + bh * splits * 2;
  const float* o = ws_o + bh * splits * dim_head;
  for (int t = threadIdx.x; t < dim_head; t += 256) {
    float M, L, O;
    merge_parts<SLOTS != 0>(splits, [&](int i, float* pm, float* pl, float* po) { *pm = ml[i * 2]; *pl = ml[i * 2 + 1]; *po = o[(int64_t)i * dim_head + t]; },
                &M, &L, &O);
    if (SLOTS && !(L > 0.f)) L = 1.f;   // no key in any part (O is 0): +0, not 0 / 0
    out[bh * dim_head + t] = f32_to_bf16(O / L);
  }
}

inline bool decode_dim_head_ok(int dim_head) { return dim_head == 64 || dim_head == 128 || dim_head == 192 || dim_head == 384; }

// Workgroups per (b, h): a power of two, enough for one workgroup per compute unit at this B * heads, each split at least DECODE_MIN_KEYS keys
inline int decode_splits(int64_t B, int heads, int64_t n) {
  const int64_t bh = B * heads;
  int want = 1;
  while (want < DECODE_MAX_SPLITS && bh * want < 256) want *= 2;
  int sp = 1;
  while (sp * 2 <= want && (int64_t)sp * 2 * DECODE_MIN_KEYS <= n) sp *= 2;
  return sp;
}

}  // namespace

extern "C" int32_t tribe_attention_decode_splits(int64_t B, int32_t heads, int64_t n) {
  if (B <= 0 || heads <= 0 || n <= 0) return 0;
  return decode_splits(B, heads, n);
}

extern "C" size_t tribe_attention_decode_workspace_bytes(int64_t B, int32_t heads, int32_t dim_head, int64_t n) {
  if (B <= 0 || heads <= 0 || dim_head <= 0 || n <= 0) return 0;
  const int sp = decode_splits(B, heads, n);
  if (sp == 1) return 256;   // (one split writes the output itself; a caller may still pass a non-null pointer)
  return align256((size_t)B * heads * sp * 2 * sizeof(float)) + align256((size_t)B * heads * sp * dim_head * sizeof(float));
}

extern "C" int tribe_kv_append(uint16_t* qkv, int64_t B, int32_t heads, int32_t dim_head, int32_t rot_dim, int32_t interleaved,
                               const float* cos_tab, const float* sin_tab, int64_t pos, uint16_t* k_cache, uint16_t* v_cache, int64_t cap,
                               void* stream) {
  TRIBE_REQUIRE(qkv && k_cache && v_cache, "tribe_kv_append: null pointer");
  TRIBE_REQUIRE(B > 0 && heads > 0 && dim_head > 0 && dim_head % 8 == 0, "tribe_kv_append: bad shape (B=%lld, heads=%d, dim_head=%d; dim_head %% 8 == 0)",
                (long long)B, heads, dim_head);
  TRIBE_REQUIRE(cap > 0 && pos >= 0 && pos < cap, "tribe_kv_append: pos=%lld outside the cache capacity %lld", (long long)pos, (long long)cap);
  TRIBE_REQUIRE(rot_dim >= 0 && rot_dim <= dim_head && rot_dim % 8 == 0, "tribe_kv_append: rot_dim=%d must be a multiple of 8 and <= dim_head=%d",
                rot_dim, dim_head);
  TRIBE_REQUIRE(rot_dim == 0 || (cos_tab && sin_tab), "tribe_kv_append: rotary tables missing");
  TRIBE_REQUIRE(interleaved == 0 || interleaved == 1, "tribe_kv_append: interleaved must be 0 or 1");
  TRIBE_REQUIRE(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)k_cache % 16) == 0 && ((uintptr_t)v_cache % 16) == 0 &&
                    ((uintptr_t)cos_tab % 16) == 0 && ((uintptr_t)sin_tab % 16) == 0,
                "tribe_kv_append: buffers must be 16-byte aligned");
  const int64_t total = B * 3 * heads * (dim_head / 8);
  hipLaunchKernelGGL(kv_append_kernel<int64_t>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, qkv, B, (int64_t)1, heads, dim_head,
                     rot_dim, interleaved, cos_tab, sin_tab, pos, k_cache, v_cache, cap);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_kv_append_block(uint16_t* qkv, int64_t B, int64_t k, int32_t heads, int32_t dim_head, int32_t rot_dim,
                                     int32_t interleaved, const float* cos_tab, const float* sin_tab, int64_t pos, uint16_t* k_cache,
                                     uint16_t* v_cache, int64_t cap, void* stream) {
  TRIBE_REQUIRE(qkv && k_cache && v_cache, "tribe_kv_append_block: null pointer");
  TRIBE_REQUIRE(B > 0 && heads > 0 && dim_head > 0 && dim_head % 8 == 0,
                "tribe_kv_append_block: bad shape (B=%lld, heads=%d, dim_head=%d; dim_head %% 8 == 0)", (long long)B, heads, dim_head);
  TRIBE_REQUIRE(k >= 1 && pos >= 0 && pos + k <= cap,
                "tribe_kv_append_block: k=%lld positions from pos=%lld outside the cache capacity %lld (k >= 1, pos >= 0, pos + k <= cap)",
                (long long)k, (long long)pos, (long long)cap);
  TRIBE_REQUIRE(rot_dim >= 0 && rot_dim <= dim_head && rot_dim % 8 == 0,
                "tribe_kv_append_block: rot_dim=%d must be a multiple of 8 and <= dim_head=%d", rot_dim, dim_head);
  TRIBE_REQUIRE(rot_dim == 0 || (cos_tab && sin_tab), "tribe_kv_append_block: rotary tables missing");
  TRIBE_REQUIRE(interleaved == 0 || interleaved == 1, "tribe_kv_append_block: interleaved must be 0 or 1");
  TRIBE_REQUIRE(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)k_cache % 16) == 0 && ((uintptr_t)v_cache % 16) == 0 &&
                    ((uintptr_t)cos_tab % 16) == 0 && ((uintptr_t)sin_tab % 16) == 0,
                "tribe_kv_append_block: buffers must be 16-byte aligned");
  const int64_t total = B * k * 3 * heads * (dim_head / 8);
  hipLaunchKernelGGL(kv_append_kernel<int64_t>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, qkv, B, k, heads, dim_head, rot_dim,
                     interleaved, cos_tab, sin_tab, pos, k_cache, v_cache, cap);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

// the k and v heads of a fused, already rotated [B*T, 3*inner] buffer into slots 0 .. T-1 (tribe_encoder_prefill_fwd)
int tribe_internal_kv_fill(const uint16_t* qkv, int64_t B, int64_t T, int heads, int dim_head, uint16_t* k_cache, uint16_t* v_cache,
                           int64_t cap, hipStream_t stream) {
  TRIBE_REQUIRE(qkv && k_cache && v_cache && B > 0 && T > 0 && T <= cap && heads > 0 && dim_head > 0 && dim_head % 8 == 0,
                "tribe_encoder_prefill_fwd: bad cache fill (T=%lld, capacity %lld)", (long long)T, (long long)cap);
  const int64_t total = B * T * 2 * heads * (dim_head / 8);
  hipLaunchKernelGGL(kv_fill_kernel, dim3(grid_for(total, 256)), dim3(256), 0, stream, qkv, B, T, heads, dim_head, k_cache, v_cache, cap);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_attention_decode_fwd(const uint16_t* q, int64_t ld_q, const uint16_t* k_cache, const uint16_t* v_cache, int64_t B,
                                          int32_t heads, int32_t dim_head, int64_t cap, int64_t n, float scale, uint16_t* out,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(q && k_cache && v_cache && out, "tribe_attention_decode_fwd: null pointer");
  TRIBE_REQUIRE(B > 0 && B < 65536 && heads > 0 && heads < 65536, "tribe_attention_decode_fwd: bad shape (B=%lld, heads=%d)", (long long)B, heads);
  TRIBE_REQUIRE(decode_dim_head_ok(dim_head), "tribe_attention_decode_fwd: dim_head=%d must be 64, 128, 192 or 384", dim_head);
  TRIBE_REQUIRE(n >= 1 && n <= cap, "tribe_attention_decode_fwd: n=%lld keys outside 1 .. capacity %lld", (long long)n, (long long)cap);
  TRIBE_REQUIRE(ld_q >= (int64_t)heads * dim_head && ld_q % 8 == 0, "tribe_attention_decode_fwd: ld_q=%lld must cover heads * dim_head and be a multiple of 8",
                (long long)ld_q);
  TRIBE_REQUIRE(((uintptr_t)q % 16) == 0 && ((uintptr_t)k_cache % 16) == 0 && ((uintptr_t)v_cache % 16) == 0,
                "tribe_attention_decode_fwd: q and the caches must be 16-byte aligned");
  const int sp = decode_splits(B, heads, n);
  float *ws_ml = nullptr, *ws_o = nullptr;
  if (sp > 1) {
    TRIBE_REQUIRE(workspace && ((uintptr_t)workspace % 256) == 0, "tribe_attention_decode_fwd: workspace must be non-null and 256-byte aligned");
    Arena ws(workspace);
    ws_ml = ws.take<float>((size_t)B * heads * sp * 2 * sizeof(float));
    ws_o = ws.take<float>((size_t)B * heads * sp * dim_head * sizeof(float));
    TRIBE_REQUIRE(workspace_bytes >= ws.off, "tribe_attention_decode_fwd: workspace too small (%zu < %zu)", workspace_bytes, ws.off);
  }
  const int64_t chunk = round_up((n + sp - 1) / sp, 8);
  const float scale_log2e = scale * 1.4426950408889634f;
  const dim3 grid((unsigned)sp, (unsigned)heads, (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
#define TRIBE_DECODE_LAUNCH(DH)                                                                                                        \
  hipLaunchKernelGGL((attn_decode_split_kernel<DH, 0>), grid, dim3(256), 0, s, q, ld_q, k_cache, v_cache, heads, cap, n, chunk, sp, \
                     scale_log2e, ws_ml, ws_o, out, (const int32_t*)nullptr)
  switch (dim_head) {
    case 64: TRIBE_DECODE_LAUNCH(64); break;
    case 128: TRIBE_DECODE_LAUNCH(128); break;
    case 192: TRIBE_DECODE_LAUNCH(192); break;
    default: TRIBE_DECODE_LAUNCH(384); break;
  }
#undef TRIBE_DECODE_LAUNCH
  TRIBE_LAUNCH_CHECK();
  if (sp > 1) {
    hipLaunchKernelGGL(attn_decode_combine_kernel<0>, dim3((unsigned)heads, (unsigned)B), dim3(256), 0, s, ws_ml, ws_o, heads, dim_head, sp, out);
    TRIBE_LAUNCH_CHECK();
  }
  return 0;
}

// ---- slots: every sequence of the cache at a position of its own (pos: device int32 [B]; -1, or any value out of range, = takes no part) ----
extern "C" int tribe_kv_append_slots(uint16_t* qkv, int64_t B, int64_t k, int32_t heads, int32_t dim_head, int32_t rot_dim,
                                     int32_t interleaved, const float* cos_tab, const float* sin_tab, const int32_t* pos, uint16_t* k_cache,
                                     uint16_t* v_cache, int64_t cap, void* stream) {
  TRIBE_REQUIRE(qkv && k_cache && v_cache && pos, "tribe_kv_append_slots: null pointer");
  TRIBE_REQUIRE(B > 0 && heads > 0 && dim_head > 0 && dim_head % 8 == 0,
                "tribe_kv_append_slots: bad shape (B=%lld, heads=%d, dim_head=%d; dim_head %% 8 == 0)", (long long)B, heads, dim_head);
  TRIBE_REQUIRE(k >= 1 && k <= cap && cap < (1ll << 31),
                "tribe_kv_append_slots: k=%lld positions per sequence do not fit the cache capacity %lld (1 <= k <= cap < 2^31)", (long long)k,
                (long long)cap);
  TRIBE_REQUIRE(rot_dim >= 0 && rot_dim <= dim_head && rot_dim % 8 == 0,
                "tribe_kv_append_slots: rot_dim=%d must be a multiple of 8 and <= dim_head=%d", rot_dim, dim_head);
  TRIBE_REQUIRE(rot_dim == 0 || (cos_tab && sin_tab), "tribe_kv_append_slots: rotary tables missing");
  TRIBE_REQUIRE(interleaved == 0 || interleaved == 1, "tribe_kv_append_slots: interleaved must be 0 or 1");
  TRIBE_REQUIRE(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)k_cache % 16) == 0 && ((uintptr_t)v_cache % 16) == 0 &&
                    ((uintptr_t)cos_tab % 16) == 0 && ((uintptr_t)sin_tab % 16) == 0 && ((uintptr_t)pos % 4) == 0,
                "tribe_kv_append_slots: buffers must be 16-byte aligned, pos 4-byte aligned");
  const int64_t total = B * k * 3 * heads * (dim_head / 8);
  hipLaunchKernelGGL(kv_append_kernel<const int32_t*>, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, qkv, B, k, heads, dim_head,
                     rot_dim, interleaved, cos_tab, sin_tab, pos, k_cache, v_cache, cap);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

extern "C" int tribe_attention_decode_slots_fwd(const uint16_t* q, int64_t ld_q, const uint16_t* k_cache, const uint16_t* v_cache, int64_t B,
                                                int32_t heads, int32_t dim_head, int64_t cap, const int32_t* pos, int64_t n_max, float scale,
                                                uint16_t* out, void* workspace, size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(q && k_cache && v_cache && out && pos, "tribe_attention_decode_slots_fwd: null pointer");
  TRIBE_REQUIRE(B > 0 && B < 65536 && heads > 0 && heads < 65536, "tribe_attention_decode_slots_fwd: bad shape (B=%lld, heads=%d)", (long long)B,
                heads);
  TRIBE_REQUIRE(decode_dim_head_ok(dim_head), "tribe_attention_decode_slots_fwd: dim_head=%d must be 64, 128, 192 or 384", dim_head);
  TRIBE_REQUIRE(n_max >= 1 && n_max <= cap && cap < (1ll << 31), "tribe_attention_decode_slots_fwd: n_max=%lld keys outside 1 .. capacity %lld",
                (long long)n_max, (long long)cap);
  TRIBE_REQUIRE(ld_q >= (int64_t)heads * dim_head && ld_q % 8 == 0,
                "tribe_attention_decode_slots_fwd: ld_q=%lld must cover heads * dim_head and be a multiple of 8", (long long)ld_q);
  TRIBE_REQUIRE(((uintptr_t)q % 16) == 0 && ((uintptr_t)k_cache % 16) == 0 && ((uintptr_t)v_cache % 16) == 0 && ((uintptr_t)pos % 4) == 0,
                "tribe_attention_decode_slots_fwd: q and the caches must be 16-byte aligned, pos 4-byte aligned");
  // the split count and the chunk of tribe_attention_decode_fwd at n = n_max: with every pos[b] + 1 == n_max the two calls give the same bits
  const int sp = decode_splits(B, heads, n_max);
  float *ws_ml = nullptr, *ws_o = nullptr;
  if (sp > 1) {
    TRIBE_REQUIRE(workspace && ((uintptr_t)workspace % 256) == 0,
                  "tribe_attention_decode_slots_fwd: workspace must be non-null and 256-byte aligned");
    Arena ws(workspace);
    ws_ml = ws.take<float>((size_t)B * heads * sp * 2 * sizeof(float));
    ws_o = ws.take<float>((size_t)B * heads * sp * dim_head * sizeof(float));
    TRIBE_REQUIRE(workspace_bytes >= ws.off, "tribe_attention_decode_slots_fwd: workspace too small (%zu < %zu)", workspace_bytes, ws.off);
  }
  const int64_t chunk = round_up((n_max + sp - 1) / sp, 8);
  const float scale_log2e = scale * 1.4426950408889634f;
  const dim3 grid((unsigned)sp, (unsigned)heads, (unsigned)B);
  hipStream_t s = (hipStream_t)stream;
#define TRIBE_DECODE_LAUNCH(DH)                                                                                                           \
  hipLaunchKernelGGL((attn_decode_split_kernel<DH, 1>), grid, dim3(256), 0, s, q, ld_q, k_cache, v_cache, heads, cap, n_max, chunk, sp, \
                     scale_log2e, ws_ml, ws_o, out, pos)
  switch (dim_head) {
    case 64: TRIBE_DECODE_LAUNCH(64); break;
    case 128: TRIBE_DECODE_LAUNCH(128); break;
    case 192: TRIBE_DECODE_LAUNCH(192); break;
    default: TRIBE_DECODE_LAUNCH(384); break;
  }
#undef TRIBE_DECODE_LAUNCH
  TRIBE_LAUNCH_CHECK();
  if (sp > 1) {
    hipLaunchKernelGGL(attn_decode_combine_kernel<1>, dim3((unsigned)heads, (unsigned)B), dim3(256), 0, s, ws_ml, ws_o, heads, dim_head, sp, out);
    TRIBE_LAUNCH_CHECK();
  }
  return 0;
}
