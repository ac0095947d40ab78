// The V-JEPA2 frame pre-processing (what `default_video_processor` of data_utils/features/video.py does on the host: antialiased
// bilinear resize of the shortest edge, centre crop, / 255, ImageNet normalisation): uint8 frames [n_src, H, W, 3] ->
// pixel_values_videos f32 [n_out, 3, crop, crop], without the host.
//
// The resize is separable.  Along one axis output position i is sum_k weight[i][k] * in[first[i] + k] over `taps` taps; the two
// tables (rows of the crop window only) are built on the host in float64 (`aa_resize_taps`), validated there against H and W, and
// copied into the workspace in-stream.  Output slot s shows source frame src[s], so a frame that several clips share is uploaded
// once and processed once per slot that shows it -- from the same bytes by the same instructions, hence to the same bits.
//
// One workgroup of 192 threads owns a tile of `tile_h` output rows x 64 output columns of one slot, all three channels: wave c is
// channel c, lane x is a column, so a wave's stores are 256 contiguous bytes of one output row.
//   pass 1 (W): for every input row the tile's output rows reach (first_h[y0] .. first_h[y1] + taps_h), four rows at a time, one
//               f32 fma chain over the taps_w taps, in tap order, from single-byte loads (rows are 3 * W bytes: no alignment is
//               assumed anywhere); the filtered rows go to LDS, [row][channel][column].
//   pass 2 (H): per output row one fma chain over taps_h LDS rows, in tap order, then (v / 255 - mean) / std and the store.
// A thread reads back only the LDS column it wrote, so the passes need no barrier between them.  The tap counts are run-time
// values (1 at identity, 2 upscaling, 5 at 720p, 17 for 400 x 300 -> 32): both chains are loops, the four accumulators of pass 1
// have compile-time indices, and the variable-length data lives in LDS, never in a per-lane array.  No atomics, no reduction
// across threads: a slot's values do not depend on the rest of the batch.
#include "common.h"

namespace {

constexpr int VP_TILE_W = 64;                      // output columns per workgroup = lanes of a wave
constexpr int VP_THREADS = 3 * VP_TILE_W;          // wave c = channel c
constexpr int VP_ROWS = 4;                         // input rows per step of pass 1
constexpr int VP_MAX_SPAN = 64;                    // input rows a tile may reach: 64 * 192 * 4 B = 48 KiB of LDS
constexpr int VP_MAX_TILE_H = 16;

struct VpNorm {
  float mean[3], std[3];
};

struct VpLayout {   // the workspace: i32 first_h [crop] | i32 first_w [crop] | i32 src [n_out] | f32 w_h [crop, taps_h] | f32 w_w [crop, taps_w]
  size_t first_h, first_w, src, w_h, w_w, total;
};

static VpLayout vp_layout(int64_t n_out, int64_t crop, int64_t taps_h, int64_t taps_w) {
  VpLayout l;
  l.first_h = 0;
  l.first_w = l.first_h + (size_t)round_up(crop * 4, 16);
  l.src = l.first_w + (size_t)round_up(crop * 4, 16);
  l.w_h = l.src + (size_t)round_up(n_out * 4, 16);
  l.w_w = l.w_h + (size_t)round_up(crop * taps_h * 4, 16);
  l.total = l.w_w + (size_t)round_up(crop * taps_w * 4, 16);
  return l;
}

__global__ __launch_bounds__(VP_THREADS) void video_preprocess_kernel(
    const uint8_t* __restrict__ frames, const int32_t* __restrict__ src, const int32_t* __restrict__ first_h,
    const float* __restrict__ w_h, const int32_t* __restrict__ first_w, const float* __restrict__ w_w, int H, int W, int crop,
    int taps_h, int taps_w, int tile_h, int tiles_y, int tiles_x, VpNorm norm, float* __restrict__ out) {
  extern __shared__ float rows[];                  // [span rounded up to VP_ROWS][3][VP_TILE_W]
  const int tiles = tiles_y * tiles_x;
  const int slot = blockIdx.x / tiles;
  const int tile = blockIdx.x - slot * tiles;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int c = threadIdx.x / VP_TILE_W;           // wave-uniform
  const int x = tx * VP_TILE_W + (threadIdx.x % VP_TILE_W);
  if (x >= crop) return;                           // no barrier below: a thread only reads the LDS column it wrote

  const int y0 = ty * tile_h;
  const int y1 = min(y0 + tile_h, crop);           // exclusive
  const int row0 = first_h[y0];
  const int span = first_h[y1 - 1] + taps_h - row0;   // <= VP_MAX_SPAN and row0 + span <= H: checked on the host
  const int64_t row_bytes = (int64_t)W * 3;
  const uint8_t* __restrict__ frame = frames + (int64_t)src[slot] * H * row_bytes;
  const uint8_t* __restrict__ col = frame + (int64_t)first_w[x] * 3 + c;
  const float* __restrict__ wx = w_w + (int64_t)x * taps_w;
  float* __restrict__ mine = rows + threadIdx.x;

  for (int r = 0; r < span; r += VP_ROWS) {
    // the last step may pass the span: those rows are clamped into the frame, filtered and never read
    const uint8_t* __restrict__ p0 = col + (int64_t)min(row0 + r + 0, H - 1) * row_bytes;
    const uint8_t* __restrict__ p1 = col + (int64_t)min(row0 + r + 1, H - 1) * row_bytes;
    const uint8_t* __restrict__ p2 = col + (int64_t)min(row0 + r + 2, H - 1) * row_bytes;
    const uint8_t* __restrict__ p3 = col + (int64_t)min(row0 + r + 3, H - 1) * row_bytes;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int k = 0; k < taps_w; ++k) {
      const float w = wx[k];
      a0 = fmaf(w, (float)p0[3 * k], a0);
      a1 = fmaf(w, (float)p1[3 * k], a1);
      a2 = fmaf(w, (float)p2[3 * k], a2);
      a3 = fmaf(w, (float)p3[3 * k], a3);
    }
    mine[(r + 0) * VP_THREADS] = a0;
    mine[(r + 1) * VP_THREADS] = a1;
    mine[(r + 2) * VP_THREADS] = a2;
    mine[(r + 3) * VP_THREADS] = a3;
  }

  const float mean = norm.mean[c], std = norm.std[c];
  float* __restrict__ o = out + (((int64_t)slot * 3 + c) * crop + y0) * crop + x;
  for (int y = y0; y < y1; ++y, o += crop) {
    const float* __restrict__ wy = w_h + (int64_t)y * taps_h;
    const float* __restrict__ v = mine + (first_h[y] - row0) * VP_THREADS;
    float a = 0.f;
    for (int k = 0; k < taps_h; ++k) a = fmaf(wy[k], v[k * VP_THREADS], a);
    *o = (a / 255.0f - mean) / std;
  }
}

// input rows the widest tile of `tile_h` output rows reaches; the table is non-decreasing (checked before)
static int vp_span(const int32_t* first_h, int crop, int taps_h, int tile_h) {
  int widest = 0;
  for (int y0 = 0; y0 < crop; y0 += tile_h) {
    const int y1 = y0 + tile_h < crop ? y0 + tile_h : crop;
    const int s = first_h[y1 - 1] + taps_h - first_h[y0];
    if (s > widest) widest = s;
  }
  return widest;
}

static int vp_check_sizes(const char* who, int64_t n_out, int32_t crop, int32_t taps_h, int32_t taps_w) {
  TRIBE_REQUIRE(n_out >= 1 && n_out < (int64_t)1 << 24, "%s: %lld output frames (1 to 2^24 - 1 per call)", who, (long long)n_out);
  TRIBE_REQUIRE(crop >= 1 && crop <= 4096, "%s: crop %d (1 to 4096)", who, (int)crop);
  TRIBE_REQUIRE(taps_h >= 1 && taps_h <= VP_MAX_SPAN && taps_w >= 1 && taps_w <= 4096,
                "%s: %d x %d taps (1 to %d along H, 1 to 4096 along W)", who, (int)taps_h, (int)taps_w, VP_MAX_SPAN);
  return 0;
}

static int vp_check_table(const char* who, const char* axis, const int32_t* first, int32_t taps, int32_t crop, int64_t n_in) {
  for (int i = 0; i < crop; ++i) {
    TRIBE_REQUIRE(first[i] >= 0 && (int64_t)first[i] + taps <= n_in, "%s: %s tap window %d is [%d, %d + %d) of %lld", who, axis, i,
                  (int)first[i], (int)first[i], (int)taps, (long long)n_in);
    TRIBE_REQUIRE(i == 0 || first[i] >= first[i - 1], "%s: %s tap windows must not move backwards (position %d)", who, axis, i);
  }
  return 0;
}

}  // namespace

extern "C" size_t tribe_video_preprocess_workspace_bytes(int64_t n_out, int32_t crop, int32_t taps_h, int32_t taps_w) {
  if (vp_check_sizes("tribe_video_preprocess_workspace_bytes", n_out, crop, taps_h, taps_w)) return 0;
  return vp_layout(n_out, crop, taps_h, taps_w).total;
}

extern "C" int tribe_video_preprocess_fwd(const uint8_t* frames, int64_t n_src, int32_t H, int32_t W, const int32_t* src_host,
                                          int64_t n_out, int32_t resized_h, int32_t resized_w, int32_t crop,
                                          const int32_t* first_h_host, const float* w_h_host, int32_t taps_h,
                                          const int32_t* first_w_host, const float* w_w_host, int32_t taps_w, const float* mean_host,
                                          const float* std_host, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "tribe_video_preprocess_fwd";
  TRIBE_REQUIRE(frames && src_host && first_h_host && w_h_host && first_w_host && w_w_host && mean_host && std_host && out && workspace,
                "%s: null pointer", who);
  TRIBE_REQUIRE(n_src >= 1 && H >= 1 && W >= 1 && W <= (1 << 24), "%s: %lld frames of %d x %d", who, (long long)n_src, (int)H, (int)W);
  if (int rc = vp_check_sizes(who, n_out, crop, taps_h, taps_w)) return rc;
  TRIBE_REQUIRE(resized_h >= 1 && resized_w >= 1 && crop <= resized_h && crop <= resized_w, "%s: crop %d does not fit the resized frame %d x %d",
                who, (int)crop, (int)resized_h, (int)resized_w);
  if (int rc = vp_check_table(who, "H", first_h_host, taps_h, crop, H)) return rc;
  if (int rc = vp_check_table(who, "W", first_w_host, taps_w, crop, W)) return rc;
  for (int64_t i = 0; i < n_out; ++i)
    TRIBE_REQUIRE(src_host[i] >= 0 && src_host[i] < n_src, "%s: src[%lld] = %d names none of the %lld frames", who, (long long)i,
                  (int)src_host[i], (long long)n_src);
  for (int c = 0; c < 3; ++c) TRIBE_REQUIRE(std_host[c] > 0.f, "%s: std[%d] must be positive", who, c);
  const VpLayout l = vp_layout(n_out, crop, taps_h, taps_w);
  TRIBE_REQUIRE(workspace_bytes >= l.total, "%s: workspace too small", who);
  TRIBE_REQUIRE(((uintptr_t)workspace % 16) == 0 && ((uintptr_t)out % 4) == 0, "%s: misaligned pointer", who);

  int tile_h = VP_MAX_TILE_H;                       // the tallest tile whose input rows fit the LDS budget; taps_h <= VP_MAX_SPAN: 1 always fits
  while (tile_h > 1 && vp_span(first_h_host, crop, taps_h, tile_h) > VP_MAX_SPAN) tile_h /= 2;
  const int span = vp_span(first_h_host, crop, taps_h, tile_h);
  TRIBE_REQUIRE(span >= 1 && span <= VP_MAX_SPAN, "%s: a tile reaches %d input rows (at most %d)", who, span, VP_MAX_SPAN);
  const int tiles_y = (crop + tile_h - 1) / tile_h, tiles_x = (crop + VP_TILE_W - 1) / VP_TILE_W;
  const int64_t blocks = n_out * tiles_y * tiles_x;
  TRIBE_REQUIRE(blocks < (int64_t)1 << 31, "%s: output too large", who);
  const size_t lds = (size_t)round_up(span, VP_ROWS) * VP_THREADS * sizeof(float);

  char* ws = (char*)workspace;
  hipStream_t s = (hipStream_t)stream;
  struct { size_t off; const void* from; size_t bytes; } copies[5] = {
      {l.first_h, first_h_host, (size_t)crop * 4}, {l.first_w, first_w_host, (size_t)crop * 4}, {l.src, src_host, (size_t)n_out * 4},
      {l.w_h, w_h_host, (size_t)crop * taps_h * 4}, {l.w_w, w_w_host, (size_t)crop * taps_w * 4}};
  for (const auto& cp : copies) {
    const hipError_t e = hipMemcpyAsync(ws + cp.off, cp.from, cp.bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
      tribe_set_error("%s: table upload failed: %s", who, hipGetErrorString(e));
      return (int)e;
    }
  }
  VpNorm norm;
  for (int c = 0; c < 3; ++c) norm.mean[c] = mean_host[c], norm.std[c] = std_host[c];
  hipLaunchKernelGGL(video_preprocess_kernel, dim3((unsigned)blocks), dim3(VP_THREADS), lds, s, frames, (const int32_t*)(ws + l.src),
                     (const int32_t*)(ws + l.first_h), (const float*)(ws + l.w_h), (const int32_t*)(ws + l.first_w),
                     (const float*)(ws + l.w_w), (int)H, (int)W, (int)crop, (int)taps_h, (int)taps_w, tile_h, tiles_y, tiles_x, norm, out);
  TRIBE_LAUNCH_CHECK();
  return 0;
}
