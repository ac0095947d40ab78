// Fractional resampling with julius' windowed-sinc polyphase filter (reference data_utils/features/audio.py:129-138,
// `julius.resample.ResampleFrac(old_sr, new_sr)` at zeros = 24, rolloff = 0.945): a waveform at its native rate -> 16 kHz,
// without the host.  With the reduced rates old / new, W = `width` and K = 2 W + old, output j = f * new + i (frame f, phase i) is
//   y[j, c] = sum_{k < K} table[i, k] * x[clamp(f * old + k - W, 0, n - 1), c]
// -- julius' replicate padding (W, W + old) followed by a stride-`old` convolution with `new` filters -- as one f32 fma chain in k
// order.  The table (f32 [new, K]) is built on the host in float32 by julius' own torch recipe
// (`data_utils.features.audio.julius_resample_kernels`) and only read here.
//
// A batch of chunks with different lengths is ONE launch: the per-chunk pointers and lengths travel as a kernel argument
// (RsTable, at most TRIBE_RESAMPLE_MAX_CHUNKS chunks).  No float atomics, no reduction across threads, and no thread looks at
// another chunk or channel: an output sample is the same bits alone, in any batch, in any channel count and on every call.
//
// A workgroup owns `ft` consecutive frames of one channel of one chunk.  Their (ft - 1) old + K input samples go through LDS once,
// clamped while they are staged.  A thread owns one phase i and RS_R frames g, g + G, g + 2 G, ... of the tile: a table value read
// once (through L2; the 372 KB table of 441 / 160 is shared by every workgroup) serves RS_R accumulators, and lanes that differ in g
// read LDS `old` words apart (conflict-free for odd `old`), lanes that differ in i the same word (a broadcast).  G is chosen on
// the host so that G * new fills the 256 threads: 256 frame groups at new = 1 (48 kHz), 3 at new = 160 (44.1 kHz).  The plan
// depends on (old, new, K) alone.  Filters longer than the LDS window (old in the thousands) take the same code with the taps cut
// into blocks of `kb`, the window restaged per block and the accumulators kept: the chain stays in k order.
#include "common.h"

namespace {

constexpr int RS_MAX = TRIBE_RESAMPLE_MAX_CHUNKS;
constexpr int RS_THREADS = 256;
constexpr int RS_R = 4;            // frames per thread (accumulators in registers)
constexpr int RS_CAP = 12288;      // f32 words of LDS per workgroup (48 KiB: three workgroups per CU)
constexpr int64_t RS_TABLE_MAX_BYTES = (int64_t)64 << 20;
constexpr int64_t RS_MAX_SAMPLES = (int64_t)1 << 40;

struct RsTable {
  const float* x[RS_MAX];
  float* y[RS_MAX];
  int64_t n[RS_MAX];
  int64_t n_out[RS_MAX];
  int32_t tile_off[RS_MAX + 1];   // first workgroup (grid x) of the chunk
  int32_t B;
};

struct RsPlan {
  int G;    // frame groups across threads: a pass of the workgroup covers G * new (phase, group) items
  int ft;   // frames per workgroup, <= RS_R * G
  int kb;   // taps per staged block; (ft - 1) * old + kb <= RS_CAP
};

// a function of the ratio alone, so a chunk is tiled the same way in every batch
static RsPlan rs_plan(int64_t old, int64_t nw, int64_t K) {
  const int64_t kb_min = K < RS_CAP / 2 ? K : RS_CAP / 2;
  const int64_t ft_max = (RS_CAP - kb_min) / old + 1;           // >= 1
  int64_t g_max = ft_max / RS_R;
  if (g_max > RS_THREADS) g_max = RS_THREADS;
  if (g_max > 8 * RS_THREADS / nw) g_max = 8 * RS_THREADS / nw;   // at most 8 passes' worth of groups: G * new stays far inside int32
  if (g_max < 1) g_max = 1;
  RsPlan p;
  p.G = 1;
  double best = 0.0;
  for (int64_t g = 1; g <= g_max; ++g) {                        // the smallest G with the fullest passes
    const int64_t items = g * nw, passes = (items + RS_THREADS - 1) / RS_THREADS;
    const double eff = (double)items / (double)(passes * RS_THREADS);
    if (eff > best + 1e-9) {
      best = eff;
      p.G = (int)g;
    }
  }
  const int64_t ft = (int64_t)RS_R * p.G < ft_max ? (int64_t)RS_R * p.G : ft_max;
  const int64_t kb = RS_CAP - (ft - 1) * old;
  p.ft = (int)ft;
  p.kb = (int)(K < kb ? K : kb);
  return p;
}

__global__ __launch_bounds__(RS_THREADS) void resample_frac_kernel(RsTable tab, int channels, int old, int nw, int W, int K, RsPlan plan,
                                                                   const float* __restrict__ table) {
  __shared__ float xs[RS_CAP];
  const int tid = threadIdx.x;
  int b = 0;
  while (b + 1 < tab.B && (int)blockIdx.x >= tab.tile_off[b + 1]) ++b;
  const int c = blockIdx.y;
  const int64_t n = tab.n[b], n_out = tab.n_out[b];
  const float* __restrict__ x = tab.x[b] + c;
  float* __restrict__ y = tab.y[b] + c;
  const int64_t frames = (n_out + nw - 1) / nw;                 // <= n / old + 1 (checked on the host)
  const int64_t f0 = (int64_t)((int)blockIdx.x - tab.tile_off[b]) * plan.ft;
  const int nf = (int)(frames - f0 < plan.ft ? frames - f0 : plan.ft);   // >= 1 by the grid
  const int64_t first = f0 * old - W;                           // input sample under tap 0 of frame f0
  const bool one_block = K <= plan.kb;

  // xs[s] = x[clamp(first + k0 + s)], s < (nf - 1) old + taps: every read is inside [0, n)
  auto stage = [&](int k0, int taps) {
    const int span = (nf - 1) * old + taps;                     // <= RS_CAP by the plan
    for (int s = tid; s < span; s += RS_THREADS) {
      int64_t p = first + k0 + s;
      p = p < 0 ? 0 : (p > n - 1 ? n - 1 : p);
      xs[s] = x[p * channels];
    }
  };
  if (one_block) {
    stage(0, K);
    __syncthreads();
  }

  const int items = plan.G * nw;
  for (int base = 0; base < items; base += RS_THREADS) {        // uniform trip count: the barriers below are met by every thread
    const int item = base + tid;
    const bool active = item < items;
    const int g = active ? item / nw : 0;
    const int i = active ? item - g * nw : 0;
    int off[RS_R];
#pragma unroll
    for (int r = 0; r < RS_R; ++r) {
      const int fr = r * plan.G + g;
      off[r] = (fr < nf ? fr : 0) * old;                        // a frame past the tile reads frame 0's window and is not stored
    }
    float acc[RS_R];
#pragma unroll
    for (int r = 0; r < RS_R; ++r) acc[r] = 0.f;
    const float* __restrict__ row = table + (size_t)i * K;
    for (int k0 = 0; k0 < K; k0 += plan.kb) {
      const int taps = K - k0 < plan.kb ? K - k0 : plan.kb;
      if (!one_block) {
        __syncthreads();                                        // the previous block's window is no longer read
        stage(k0, taps);
        __syncthreads();
      }
#pragma unroll 4
      for (int k = 0; k < taps; ++k) {
        const float t = row[k0 + k];
#pragma unroll
        for (int r = 0; r < RS_R; ++r) acc[r] = fmaf(t, xs[off[r] + k], acc[r]);
      }
    }
    if (active) {
#pragma unroll
      for (int r = 0; r < RS_R; ++r) {
        const int fr = r * plan.G + g;
        const int64_t j = (f0 + fr) * nw + i;
        if (fr < nf && j < n_out) y[j * channels] = acc[r];
      }
    }
  }
}

static int64_t rs_gcd(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

}  // namespace

extern "C" int tribe_resample_frac_fwd(const float* const* wavs_host, const int64_t* n_host, int32_t B, int32_t channels, int32_t old_sr,
                                       int32_t new_sr, int32_t width, const float* table, float* const* out_host, const int64_t* n_out_host,
                                       void* stream) {
  const char* who = "tribe_resample_frac_fwd";
  TRIBE_REQUIRE(wavs_host && n_host && table && out_host && n_out_host, "%s: null pointer", who);
  TRIBE_REQUIRE(B >= 1 && B <= RS_MAX, "%s: %d chunks (1 to %d per call)", who, (int)B, RS_MAX);
  TRIBE_REQUIRE(channels >= 1 && channels <= 65535, "%s: %d channels (1 to 65535)", who, (int)channels);
  TRIBE_REQUIRE(old_sr >= 1 && new_sr >= 1, "%s: rates %d -> %d must be >= 1", who, (int)old_sr, (int)new_sr);
  TRIBE_REQUIRE(old_sr != new_sr, "%s: equal rates %d -> %d need no resampling", who, (int)old_sr, (int)new_sr);
  TRIBE_REQUIRE(rs_gcd(old_sr, new_sr) == 1, "%s: rates %d -> %d are not reduced (coprime)", who, (int)old_sr, (int)new_sr);
  TRIBE_REQUIRE(width >= 1, "%s: width %d", who, (int)width);
  const int64_t old = old_sr, nw = new_sr, K = 2 * (int64_t)width + old;
  TRIBE_REQUIRE(nw * K * (int64_t)sizeof(float) <= RS_TABLE_MAX_BYTES, "%s: the table of %d -> %d (%lld x %lld f32) is above 64 MiB", who,
                (int)old_sr, (int)new_sr, (long long)nw, (long long)K);
  TRIBE_REQUIRE(((uintptr_t)table % 4) == 0, "%s: misaligned table", who);
  const RsPlan plan = rs_plan(old, nw, K);
  RsTable tab;
  tab.B = B;
  tab.tile_off[0] = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = n_host[b], n_out = n_out_host[b];
    TRIBE_REQUIRE(n >= 1 && n <= RS_MAX_SAMPLES, "%s: chunk %d has %lld samples (1 to 2^40)", who, b, (long long)n);
    TRIBE_REQUIRE(n_out >= 1 && n_out <= (n / old + 1) * nw, "%s: chunk %d: n_out %lld outside 1 .. (n / old + 1) * new = %lld", who, b,
                  (long long)n_out, (long long)((n / old + 1) * nw));
    TRIBE_REQUIRE(wavs_host[b] && out_host[b] && ((uintptr_t)wavs_host[b] % 4) == 0 && ((uintptr_t)out_host[b] % 4) == 0,
                  "%s: waveform or output %d is null or misaligned", who, b);
    const int64_t frames = (n_out + nw - 1) / nw;
    const int64_t tiles = (frames + plan.ft - 1) / plan.ft;
    TRIBE_REQUIRE((int64_t)tab.tile_off[b] + tiles < (int64_t)1 << 31, "%s: more than 2^31 workgroups in one call", who);
    tab.x[b] = wavs_host[b];
    tab.y[b] = out_host[b];
    tab.n[b] = n;
    tab.n_out[b] = n_out;
    tab.tile_off[b + 1] = tab.tile_off[b] + (int32_t)tiles;
  }
  hipLaunchKernelGGL(resample_frac_kernel, dim3((unsigned)tab.tile_off[B], (unsigned)channels), dim3(RS_THREADS), 0, (hipStream_t)stream, tab,
                     (int)channels, (int)old_sr, (int)new_sr, (int)width, (int)K, plan, table);
  TRIBE_LAUNCH_CHECK();
  return 0;
}
