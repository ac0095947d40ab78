// The Wav2Vec-BERT audio front end (reference data_utils/features/audio.py:123-127 `_preprocess_wav`, then transformers'
// SeamlessM4TFeatureExtractor at its defaults): 16 kHz waveform -> input_features f32 [B, T, 160], without the host.
//
// Per chunk of n samples (F = 1 + (n - 400) / 160 frames, T = ceil(F / 2) rows):
//   1. optional: mean over channels, z-score over the chunk (torch.std, ddof = 1)          fbank_wave_stats_*_kernel
//   2. * 2^15; frames of 400 samples every 160                                             fbank_frame_kernel
//   3. per frame: - mean, pre-emphasis 0.97, Povey window, 512-point one-sided DFT, |X|^2        "
//   4. [257, 80] mel matrix, max(., FLT_EPSILON), log                                            "
//   5. per mel bin over the chunk's frames: - mean, / sqrt(var(ddof = 1) + 1e-7)            fbank_bin_stats_kernel
//   6. zero frame appended when F is odd, pairs of frames stacked to rows of 160           fbank_normalize_kernel
// A batch of chunks with different lengths is ONE launch sequence: the per-chunk pointers, lengths and offsets travel as a
// kernel argument (FbTable, at most TRIBE_FBANK_MAX_CHUNKS chunks).  Every reduction has a fixed order and no float atomics,
// and no kernel looks at another chunk's data: a chunk's rows are the same bits whatever else is in the batch.
//
// The DFT is a matrix product on the f32 matrix pipe (v_mfma_f32_32x32x2_f32: a k-ordered f32 fma chain, bit for bit).  A
// workgroup owns 32 consecutive frames: their 5360 samples go through LDS once, the 32 x 400 windowed frames are the A
// operand, and B[k][j] = cos / -sin(2 pi k j / 512) is looked up in a 512-entry cosine table in LDS by (k j) mod 512 --
// -sin(t) = cos(t + pi / 2) is the same table 128 entries on -- so the 400 x 514 DFT matrix is never read from memory.  Each
// of the 4 waves owns bins [32 w, 32 w + 32) and [32 (w + 4), ...) with the real and the imaginary accumulator of a bin on
// the same lane and register, so the power is lane-local; the Nyquist bin (k j mod 512 alternates 0 / 256: signs +-1) is an
// alternating sum on the vector ALU.  Measured against the extractor, one 400-term f32 chain per bin is closer than numpy's
// all-float32 restatement of the same arithmetic (tests/test_gpu_fbank.py), so the sum is not split or widened.
// The [32, 257] power tile replaces the frames in LDS and is the A operand of the mel product (3 waves x one 32 x 32 tile of
// the 80 filters); the spectrum never goes to HBM.
#include <math.h>

#include "common.h"

namespace {

constexpr int FB_WIN = 400, FB_HOP = 160, FB_NFFT = 512, FB_BINS = 257, FB_MEL = 80;
constexpr int FB_TILE = 32;                                   // frames per workgroup = M of the MFMA
constexpr int FB_RAW = (FB_TILE - 1) * FB_HOP + FB_WIN;       // 5360 samples behind 32 frames
constexpr int FB_XLD = FB_WIN + 1;                            // odd row strides: a column of 32 rows covers 32 banks
constexpr int FB_PLD = FB_BINS + 2;                           // K of the mel product padded to 258 (column 257 is zero)
constexpr int FB_WAVE_PARTS = 64;                             // workgroups per chunk of the stage-1 reduction
constexpr float FB_MEL_FLOOR = 1.192092955078125e-07f;
constexpr int FB_MAX = TRIBE_FBANK_MAX_CHUNKS;

struct FbTable {
  const float* wav[FB_MAX];
  int64_t n[FB_MAX];
  int32_t frames[FB_MAX];
  int32_t frame_off[FB_MAX + 1];   // first row of the chunk in the [sum F, 80] log-mel buffer
  int32_t tile_off[FB_MAX + 1];    // first workgroup of the chunk in fbank_frame_kernel's grid
  int32_t B;
};

struct FbLayout {   // the workspace: f64 [B, 64, 2] | f32 [B, 2] | f32 [B, 80, 2] | f32 [sum F, 80]
  size_t partial, wave_stats, bin_stats, logmel, total;
};

static FbLayout fb_layout(int64_t B, int64_t frames_total) {
  FbLayout l;
  l.partial = 0;
  l.wave_stats = l.partial + (size_t)B * FB_WAVE_PARTS * 2 * sizeof(double);
  l.bin_stats = l.wave_stats + (size_t)round_up(B * 2 * (int64_t)sizeof(float), 16);
  l.logmel = l.bin_stats + (size_t)round_up(B * FB_MEL * 2 * (int64_t)sizeof(float), 16);
  l.total = l.logmel + (size_t)frames_total * FB_MEL * sizeof(float);
  return l;
}

__device__ __forceinline__ float channel_mean(const float* __restrict__ w, int64_t i, int channels) {
  if (channels == 1) return w[i];
  float s = w[i * channels];
  for (int c = 1; c < channels; ++c) s += w[i * channels + c];
  return s / (float)channels;
}

// ---- stage 1: sum and sum of squares of the channel mean, one-pass in f64 (|x| <~ 1, n ~ 1e6: 1e-10 relative) ----
__global__ __launch_bounds__(256) void fbank_wave_stats_partial_kernel(FbTable tab, int channels, double* __restrict__ partial) {
  __shared__ double sh[8];
  const int b = blockIdx.y;
  const float* __restrict__ w = tab.wav[b];
  const int64_t n = tab.n[b];
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)FB_WAVE_PARTS * 256) {
    const double v = (double)channel_mean(w, i, channels);
    s1 += v;
    s2 += v * v;
  }
  s1 = wave_sum_d(s1);
  s2 = wave_sum_d(s2);
  if ((threadIdx.x & 63) == 0) {
    sh[(threadIdx.x >> 6) * 2] = s1;
    sh[(threadIdx.x >> 6) * 2 + 1] = s2;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int t = threadIdx.x;
    partial[((int64_t)b * FB_WAVE_PARTS + blockIdx.x) * 2 + t] = ((sh[t] + sh[2 + t]) + (sh[4 + t] + sh[6 + t]));
  }
}

// stats[b] = (mean, 1e-8 + std) as torch's f32 expression `(wav - wav.mean()) / (1e-8 + wav.std())` uses them
__global__ __launch_bounds__(64) void fbank_wave_stats_final_kernel(FbTable tab, const double* __restrict__ partial, float* __restrict__ stats) {
  const int b = blockIdx.x;
  const double s1 = wave_sum_d(partial[((int64_t)b * FB_WAVE_PARTS + threadIdx.x) * 2]);
  const double s2 = wave_sum_d(partial[((int64_t)b * FB_WAVE_PARTS + threadIdx.x) * 2 + 1]);
  if (threadIdx.x == 0) {
    const double n = (double)tab.n[b];
    const double var = onepass_centred_ss(s1, s2, n) / (n - 1.0);
    stats[b * 2] = (float)(s1 / n);
    stats[b * 2 + 1] = 1e-8f + (float)sqrt(var);
  }
}

// ---- stages 2-4 ----
__global__ __launch_bounds__(256) void fbank_frame_kernel(FbTable tab, int channels, const float* __restrict__ wave_stats,
                                                          const float* __restrict__ window, const float* __restrict__ mel,
                                                          float* __restrict__ logmel) {
  __shared__ float sx[FB_TILE * FB_XLD];   // the windowed frames [32][401]; later the power tile [32][259]
  __shared__ float sraw[FB_RAW];
  __shared__ float tw[FB_NFFT];            // cos(2 pi m / 512)
  __shared__ float nyq[FB_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int b = 0;
  while (b + 1 < tab.B && (int)blockIdx.x >= tab.tile_off[b + 1]) ++b;
  const int f0 = ((int)blockIdx.x - tab.tile_off[b]) * FB_TILE;
  const int nf = min(FB_TILE, tab.frames[b] - f0);
  const int count = (nf - 1) * FB_HOP + FB_WIN;   // f0 * 160 + count <= n by the definition of F
  const float* __restrict__ w = tab.wav[b];
  const int64_t s0 = (int64_t)f0 * FB_HOP;
  float mean = 0.f, den = 1.f;
  if (wave_stats) {
    mean = wave_stats[b * 2];
    den = wave_stats[b * 2 + 1];
  }
  for (int i = tid; i < FB_RAW; i += 256) {
    float v = 0.f;
    if (i < count) {
      v = channel_mean(w, s0 + i, channels);
      if (wave_stats) v = (v - mean) / den;
      v *= 32768.f;
    }
    sraw[i] = v;
  }
  for (int m = tid; m < FB_NFFT; m += 256) tw[m] = (float)cospi((double)m * (1.0 / 256.0));
  __syncthreads();

  // 8 lanes per frame, 50 consecutive samples each; frames past the chunk's end are all zero
  {
    const int fr = tid >> 3, p = tid & 7;
    const float* __restrict__ x = sraw + fr * FB_HOP;
    const int i0 = p * (FB_WIN / 8);
    double s = 0.0;
    for (int q = 0; q < FB_WIN / 8; ++q) s += (double)x[i0 + q];
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    const float dc = (float)(s * (1.0 / FB_WIN));
    float prev = p ? x[i0 - 1] - dc : 0.f;
    float alt = 0.f;
    for (int q = 0; q < FB_WIN / 8; ++q) {
      const int i = i0 + q;
      const float y = x[i] - dc;
      const float z = i ? y - 0.97f * prev : y * 0.03f;
      prev = y;
      const float zw = z * window[i];
      sx[fr * FB_XLD + i] = zw;
      alt += (q & 1) ? -zw : zw;   // i0 is even: the sign of sample i is that of q
    }
    alt += __shfl_xor(alt, 1, 64);
    alt += __shfl_xor(alt, 2, 64);
    alt += __shfl_xor(alt, 4, 64);
    if (p == 0) nyq[fr] = alt;
  }
  __syncthreads();

  const int row = lane & 31, kh = lane >> 5;
  f32x16_t pw[2];
  {
    const int j[2] = {FB_TILE * wave + row, FB_TILE * (wave + 4) + row};
    f32x16_t c[4];   // [2 t] real, [2 t + 1] imaginary part of bin tile t
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) c[u][r] = 0.f;
#pragma unroll 2
    for (int k0 = 0; k0 < FB_WIN; k0 += 2) {
      const int k = k0 + kh;
      const float a = sx[row * FB_XLD + k];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int m = (k * j[t]) & (FB_NFFT - 1);
        c[2 * t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, tw[m], c[2 * t], 0, 0, 0);
        c[2 * t + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, tw[(m + FB_NFFT / 4) & (FB_NFFT - 1)], c[2 * t + 1], 0, 0, 0);
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) pw[t] = c[2 * t] * c[2 * t] + c[2 * t + 1] * c[2 * t + 1];
  }
  __syncthreads();   // every wave is done with the frames: the power tile takes their place

  // C layout of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) sx[((r & 3) + 8 * (r >> 2) + 4 * kh) * FB_PLD + FB_TILE * (wave + 4 * t) + row] = pw[t][r];
  if (tid < FB_TILE) {
    sx[tid * FB_PLD + 256] = nyq[tid] * nyq[tid];
    sx[tid * FB_PLD + 257] = 0.f;
  }
  __syncthreads();

  if (wave < 3) {
    const int j = FB_TILE * wave + row;
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 2
    for (int k0 = 0; k0 < FB_BINS + 1; k0 += 2) {
      const int k = k0 + kh;
      const float a = sx[row * FB_PLD + k];
      const float bv = (j < FB_MEL && k < FB_BINS) ? mel[k * FB_MEL + j] : 0.f;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc, 0, 0, 0);
    }
    float* __restrict__ out = logmel + ((int64_t)tab.frame_off[b] + f0) * FB_MEL;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int fr = (r & 3) + 8 * (r >> 2) + 4 * kh;
      const float v = acc[r] < FB_MEL_FLOOR ? FB_MEL_FLOOR : acc[r];   // a NaN stays a NaN (np.maximum)
      if (fr < nf && j < FB_MEL) out[fr * FB_MEL + j] = logf(v);
    }
  }
}

// ---- stage 5: per chunk and mel bin, two passes in f64 over the chunk's frames; bin_stats[b][bin] = (mean, sqrt(var + 1e-7)) ----
// 16 bins x 16 row lanes per workgroup; the 16 partial sums of a bin are added in lane order.
__global__ __launch_bounds__(256) void fbank_bin_stats_kernel(FbTable tab, const float* __restrict__ logmel, float* __restrict__ bin_stats) {
  __shared__ double sh[16][17];
  const int b = blockIdx.y, bl = threadIdx.x & 15, r = threadIdx.x >> 4;
  const int bin = blockIdx.x * 16 + bl;
  const int F = tab.frames[b];
  const float* __restrict__ x = logmel + (int64_t)tab.frame_off[b] * FB_MEL + bin;
  double s = 0.0;
  for (int f = r; f < F; f += 16) s += (double)x[(int64_t)f * FB_MEL];
  sh[r][bl] = s;
  __syncthreads();
  double tot = 0.0;
  for (int i = 0; i < 16; ++i) tot += sh[i][bl];
  const double mean = tot / (double)F;
  __syncthreads();
  s = 0.0;
  for (int f = r; f < F; f += 16) {
    const double d = (double)x[(int64_t)f * FB_MEL] - mean;
    s += d * d;
  }
  sh[r][bl] = s;
  __syncthreads();
  if (r == 0) {
    tot = 0.0;
    for (int i = 0; i < 16; ++i) tot += sh[i][bl];
    bin_stats[((int64_t)b * FB_MEL + bin) * 2] = (float)mean;
    bin_stats[((int64_t)b * FB_MEL + bin) * 2 + 1] = (float)sqrt(tot / (double)(F - 1) + 1e-7);   // F == 1: NaN, as numpy's ddof = 1
  }
}

// ---- stages 5-6: out[b][t][c] = normalised frame 2 t + (c >= 80), bin c % 80; the frame past an odd F and the rows past the
// chunk's own T are zero (the extractor's padding_value) ----
__global__ __launch_bounds__(256) void fbank_normalize_kernel(FbTable tab, const float* __restrict__ logmel, const float* __restrict__ bin_stats,
                                                              int64_t T_max, float* __restrict__ out) {
  const int64_t per_chunk = T_max * 2 * FB_MEL;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per_chunk * tab.B) return;
  const int b = (int)(i / per_chunk);
  const int64_t rem = i - (int64_t)b * per_chunk;   // = frame * 80 + bin
  const int64_t f = rem / FB_MEL;
  const int bin = (int)(rem - f * FB_MEL);
  float v = 0.f;
  if (f < tab.frames[b]) {
    const float* st = bin_stats + ((int64_t)b * FB_MEL + bin) * 2;
    v = (logmel[((int64_t)tab.frame_off[b] + f) * FB_MEL + bin] - st[0]) / st[1];
  }
  out[i] = v;
}

static int fb_make_table(const char* who, const float* const* wavs_host, const int64_t* n_host, int32_t B, FbTable* tab, int64_t* T_longest) {
  TRIBE_REQUIRE(n_host, "%s: null pointer", who);
  TRIBE_REQUIRE(B >= 1 && B <= FB_MAX, "%s: %d chunks (1 to %d per call)", who, (int)B, FB_MAX);
  tab->B = B;
  tab->frame_off[0] = tab->tile_off[0] = 0;
  *T_longest = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = n_host[b];
    TRIBE_REQUIRE(n >= FB_WIN, "%s: chunk %d has %lld samples, a frame needs %d", who, b, (long long)n, FB_WIN);
    const int64_t F = 1 + (n - FB_WIN) / FB_HOP;
    TRIBE_REQUIRE((int64_t)tab->frame_off[b] + F < (int64_t)1 << 24, "%s: more than 2^24 frames in one call", who);
    tab->wav[b] = wavs_host ? wavs_host[b] : nullptr;
    tab->n[b] = n;
    tab->frames[b] = (int32_t)F;
    tab->frame_off[b + 1] = tab->frame_off[b] + (int32_t)F;
    tab->tile_off[b + 1] = tab->tile_off[b] + (int32_t)((F + FB_TILE - 1) / FB_TILE);
    if ((F + 1) / 2 > *T_longest) *T_longest = (F + 1) / 2;
  }
  return 0;
}

}  // namespace

extern "C" size_t tribe_fbank_workspace_bytes(const int64_t* n_host, int32_t B) {
  FbTable tab;
  int64_t T_longest;
  if (fb_make_table("tribe_fbank_workspace_bytes", nullptr, n_host, B, &tab, &T_longest)) return 0;
  return fb_layout(B, tab.frame_off[B]).total;
}

extern "C" int tribe_fbank_fwd(const float* const* wavs_host, const int64_t* n_host, int32_t B, int32_t channels, int32_t zscore,
                               const float* window, const float* mel, float* out, int64_t T_max, int32_t* lengths_host, void* workspace,
                               size_t workspace_bytes, void* stream) {
  TRIBE_REQUIRE(wavs_host && n_host && window && mel && out && workspace, "tribe_fbank_fwd: null pointer");
  TRIBE_REQUIRE(channels >= 1, "tribe_fbank_fwd: %d channels", (int)channels);
  FbTable tab;
  int64_t T_longest;
  if (int rc = fb_make_table("tribe_fbank_fwd", wavs_host, n_host, B, &tab, &T_longest)) return rc;
  for (int b = 0; b < B; ++b) TRIBE_REQUIRE(tab.wav[b] && ((uintptr_t)tab.wav[b] % 4) == 0, "tribe_fbank_fwd: waveform %d is null or misaligned", b);
  TRIBE_REQUIRE(T_max >= T_longest, "tribe_fbank_fwd: T_max %lld is below the longest chunk's %lld rows", (long long)T_max, (long long)T_longest);
  const FbLayout l = fb_layout(B, tab.frame_off[B]);
  TRIBE_REQUIRE(workspace_bytes >= l.total, "tribe_fbank_fwd: workspace too small");
  TRIBE_REQUIRE(((uintptr_t)workspace % 16) == 0 && ((uintptr_t)out % 4) == 0 && ((uintptr_t)window % 4) == 0 && ((uintptr_t)mel % 4) == 0,
                "tribe_fbank_fwd: misaligned pointer");
  const int64_t out_elems = (int64_t)B * T_max * 2 * FB_MEL;
  TRIBE_REQUIRE((out_elems + 255) / 256 < (int64_t)1 << 31, "tribe_fbank_fwd: output too large");
  if (lengths_host)
    for (int b = 0; b < B; ++b) lengths_host[b] = (tab.frames[b] + 1) / 2;
  char* ws = (char*)workspace;
  double* partial = (double*)(ws + l.partial);
  float* wave_stats = (float*)(ws + l.wave_stats);
  float* bin_stats = (float*)(ws + l.bin_stats);
  float* logmel = (float*)(ws + l.logmel);
  hipStream_t s = (hipStream_t)stream;
  if (zscore) {
    hipLaunchKernelGGL(fbank_wave_stats_partial_kernel, dim3(FB_WAVE_PARTS, B), dim3(256), 0, s, tab, (int)channels, partial);
    hipLaunchKernelGGL(fbank_wave_stats_final_kernel, dim3(B), dim3(64), 0, s, tab, (const double*)partial, wave_stats);
  }
  hipLaunchKernelGGL(fbank_frame_kernel, dim3(tab.tile_off[B]), dim3(256), 0, s, tab, (int)channels, zscore ? (const float*)wave_stats : nullptr,
                     window, mel, logmel);
  hipLaunchKernelGGL(fbank_bin_stats_kernel, dim3(FB_MEL / 16, B), dim3(256), 0, s, tab, (const float*)logmel, bin_stats);
  hipLaunchKernelGGL(fbank_normalize_kernel, dim3((unsigned)((out_elems + 255) / 256)), dim3(256), 0, s, tab, (const float*)logmel,
                     (const float*)bin_stats, T_max, out);
  TRIBE_LAUNCH_CHECK();
  return 0;
}
