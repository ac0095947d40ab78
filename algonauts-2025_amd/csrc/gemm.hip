// bf16 MFMA GEMM for gfx950:  C = epi(alpha * A . B^T),  A [M,K], B [N,K], K contiguous -- the C entry points.
// No GEMM kernel lives here: tribe_gemm_bf16 resolves a launch on the host (gemm_plan.cpp) and hands it to the launch table of the
// kernel family that runs it (gemm_launch.h: gemm_8wave_nb4.hip, gemm_8wave_nb3.hip, gemm_128.hip, gemm_4wave.hip).  Beside it: the
// in-library HIP-event profile and three small helper kernels (row-norm scale, f32 <-> planes).
#include "gemm_launch.h"

#include <mutex>
#include <vector>

// ---------------------------------------------------------------------------------------------
// Optional in-library profile: HIP events recorded on the launch stream around every GEMM launch
// while enabled (bench.py brackets its timed region with tribe_prof_begin / tribe_prof_end).
// ---------------------------------------------------------------------------------------------
namespace {
struct ProfRec { hipEvent_t start, stop; int role; double flops; };
std::mutex g_prof_mu;
std::vector<ProfRec> g_prof;
size_t g_prof_used = 0;
bool g_prof_on = false;

int prof_before(int role, double flops, hipStream_t s) {
  std::lock_guard<std::mutex> lock(g_prof_mu);
  if (!g_prof_on || g_prof_used >= g_prof.size()) return -1;
  const int slot = (int)g_prof_used++;
  g_prof[slot].role = role;
  g_prof[slot].flops = flops;
  (void)hipEventRecord(g_prof[slot].start, s);
  return slot;
}
void prof_after(int slot, hipStream_t s) {
  if (slot < 0) return;
  std::lock_guard<std::mutex> lock(g_prof_mu);
  (void)hipEventRecord(g_prof[slot].stop, s);
}
}  // namespace

int tribe_internal_prof_before(int role, double flops, hipStream_t s) { return prof_before(role, flops, s); }
void tribe_internal_prof_after(int slot, hipStream_t s) { prof_after(slot, s); }

extern "C" int tribe_prof_begin(int32_t max_records) {
  std::lock_guard<std::mutex> lock(g_prof_mu);
  TRIBE_REQUIRE(max_records > 0, "tribe_prof_begin: max_records must be positive");
  while ((int)g_prof.size() < max_records) {
    ProfRec r{};
    hipError_t e = hipEventCreate(&r.start);
    if (e == hipSuccess) e = hipEventCreate(&r.stop);
    if (e != hipSuccess) { tribe_set_error("tribe_prof_begin: hipEventCreate failed: %s", hipGetErrorString(e)); return (int)e; }
    g_prof.push_back(r);
  }
  g_prof_used = 0;
  g_prof_on = true;
  return 0;
}

extern "C" int tribe_prof_end(int32_t n_roles, double* total_ms_host, int64_t* count_host, double* flops_host) {
  std::lock_guard<std::mutex> lock(g_prof_mu);
  TRIBE_REQUIRE(total_ms_host && count_host && flops_host && n_roles >= TRIBE_ROLE_COUNT, "tribe_prof_end: need %d role slots",
                TRIBE_ROLE_COUNT);
  g_prof_on = false;
  for (int i = 0; i < n_roles; ++i) { total_ms_host[i] = 0.0; count_host[i] = 0; flops_host[i] = 0.0; }
  for (size_t i = 0; i < g_prof_used; ++i) {
    hipError_t e = hipEventSynchronize(g_prof[i].stop);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, g_prof[i].start, g_prof[i].stop);
    if (e != hipSuccess) { tribe_set_error("tribe_prof_end: event query failed: %s", hipGetErrorString(e)); return (int)e; }
    total_ms_host[g_prof[i].role] += (double)ms;
    count_host[g_prof[i].role] += 1;
    flops_host[g_prof[i].role] += g_prof[i].flops;
  }
  g_prof_used = 0;
  return 0;
}

namespace {
// 16 lanes per row (each 4 partials per step, shuffle reduction): at M = 4096 one thread per row was 16 workgroups walking 48-64 partials
// serially -- 9.6 us per launch, 15 launches per forward = 1.9 % of the B = 4 step (profiles/r03_e_r1_kernel_stats.txt).
__global__ __launch_bounds__(256) void rownorm_scale_kernel(const float* __restrict__ partial, int64_t rows, int64_t n_partial,
                                                            const float* __restrict__ g, float gain_scale, float eps, float* __restrict__ scale) {
  const int sub = threadIdx.x & 15;
  const int64_t m = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  float ss = 0.f;
  if (m < rows) {
    const float* p = partial + m * n_partial;
    if ((n_partial & 3) == 0 && (((uintptr_t)partial) & 15) == 0) {
      for (int64_t i = sub * 4; i < n_partial; i += 64) {
        const float4 v = *(const float4*)(p + i);
        ss += (v.x + v.y) + (v.z + v.w);
      }
    } else {
      for (int64_t i = sub; i < n_partial; i += 16) ss += p[i];
    }
  }
  ss += __shfl_xor(ss, 1, 64);
  ss += __shfl_xor(ss, 2, 64);
  ss += __shfl_xor(ss, 4, 64);
  ss += __shfl_xor(ss, 8, 64);
  if (m < rows && sub == 0) scale[m] = g[0] * gain_scale / fmaxf(sqrtf(ss), eps);
}
}  // namespace

extern "C" int tribe_rownorm_scale_fwd(const float* partial, int64_t rows, int64_t n_partial, const float* g, float gain_scale, float eps,
                                       float* scale, void* stream) {
  TRIBE_REQUIRE(partial && g && scale && rows > 0 && n_partial > 0, "tribe_rownorm_scale_fwd: bad argument");
  hipLaunchKernelGGL(rownorm_scale_kernel, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, (hipStream_t)stream, partial, rows, n_partial, g,
                     gain_scale, eps, scale);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

// The plane format of the residual epilogues (gemm_common.h: f32_to_plane_lo / planes_to_f32) element by element: tests and debugging.
namespace {
__global__ __launch_bounds__(256) void f32_to_planes_kernel(const float* __restrict__ x, int64_t n, unsigned short* __restrict__ hi,
                                                            unsigned short* __restrict__ lo) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float v = x[i];
    hi[i] = f32_to_bf16(v);
    lo[i] = (unsigned short)f32_to_plane_lo(v);
  }
}
__global__ __launch_bounds__(256) void planes_to_f32_kernel(const unsigned short* __restrict__ hi, const unsigned short* __restrict__ lo, int64_t n,
                                                            float* __restrict__ x) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] = planes_to_f32(hi[i], lo[i]);
}
}  // namespace

extern "C" int tribe_f32_to_planes(const float* x, int64_t n, uint16_t* hi, uint16_t* lo, void* stream) {
  TRIBE_REQUIRE(x && hi && lo && n > 0, "tribe_f32_to_planes: bad argument");
  hipLaunchKernelGGL(f32_to_planes_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, x, n, hi, lo);
  TRIBE_LAUNCH_CHECK();
  return 0;
}
extern "C" int tribe_planes_to_f32(const uint16_t* hi, const uint16_t* lo, int64_t n, float* x, void* stream) {
  TRIBE_REQUIRE(x && hi && lo && n > 0, "tribe_planes_to_f32: bad argument");
  hipLaunchKernelGGL(planes_to_f32_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, hi, lo, n, x);
  TRIBE_LAUNCH_CHECK();
  return 0;
}


// ---------------------------------------------------------------------------------------------
// The C entry points. What a launch will be is resolved once, on the host, by gemm_plan.cpp (checks, kernel, tile, symbol, grid, split,
// workspace); the launch and the three queries below read that one GemmLaunch.
// ---------------------------------------------------------------------------------------------
namespace {
// compute units of the current device, asked once per device (256 where there is no device to ask); both planners count rounds on it
int device_cu_count() {
  static int cus[64] = {};
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev < 0 || dev >= 64) dev = 0;
  if (!cus[dev]) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    cus[dev] = n;
  }
  return cus[dev];
}
}  // namespace

extern "C" int tribe_gemm_bf16(const tribe_gemm_desc* d, void* stream) {
  using namespace tribe_gemm_detail;
  GemmLaunch p;
  if (gemm_resolve(d, "tribe_gemm_bf16", device_cu_count(), &p) != 0 || gemm_check_workspace(d, "tribe_gemm_bf16", p) != 0) return -1;
  // nothing below refuses the launch: a profile slot taken here always gets its stop event
  hipStream_t s = (hipStream_t)stream;
  const int role = (d->role >= 0 && d->role < TRIBE_ROLE_COUNT) ? d->role : TRIBE_ROLE_GENERIC;
  const int slot = prof_before(role, 2.0 * (double)d->M * (double)d->N * (double)d->K * (double)p.nz, s);
  const dim3 grid(p.grid_x, (unsigned)p.nz, 1);
  const int tiles_m = (int)p.tiles_m, tiles_n = (int)p.tiles_n, bf = d->c_dtype == TRIBE_BF16 ? 1 : 0;
  switch (p.kind) {
    case KIND_BIG4W: launch_4w(p.pair, grid, s, d, tiles_m, tiles_n); break;
    case KIND_BIG:
      if (d->trans_ab) launch_big4_tn(bf, grid, s, d, tiles_m, tiles_n, p.sk, p.reduce_grid_x);   // transposed operands: the 256^2 kernel only
      else if (p.bn == 192) launch_big3(p.pair, grid, s, d, tiles_m, tiles_n);
      else if (d->c_dtype >= TRIBE_F32_PLANES_OUT) launch_big4_planes(grid, s, d, tiles_m, tiles_n);
      else launch_big4(p.pair, grid, s, d, tiles_m, tiles_n);
      break;
    case KIND_RING:
      launch_ring(p.pair, grid, s, d, tiles_m, tiles_n, p.splits, p.splits > 1 ? (float*)d->stream_k_ws : nullptr);
      if (p.splits > 1) launch_splitk_epilogue(bf, s, d, p.splits, (const float*)d->stream_k_ws);
      break;
    default: launch_small(p.pair, grid, s, d, tiles_m, tiles_n); break;
  }
  prof_after(slot, s);
  TRIBE_LAUNCH_CHECK();
  return 0;
}

// the schedule itself, for inspection (tests/test_abi_and_host.py replays the kernel's decode on the host and checks that every K-step of
// every tile is covered exactly once): out = {tiles_dp, rem_units, q, workers, second_worker[0 .. 255]}; returns the grid size
extern "C" int tribe_gemm_stream_k_plan(int32_t tiles, int32_t nk, int32_t* out) {
  TRIBE_REQUIRE(tiles > 0 && nk > 0 && out != nullptr, "tribe_gemm_stream_k_plan: bad argument");
  SkSchedule sk;
  const unsigned grid = tribe_gemm_detail::plan_stream_k(tiles, nk, device_cu_count(), &sk);
  out[0] = sk.tiles_dp; out[1] = sk.rem_units; out[2] = sk.q; out[3] = sk.workers;
  for (int i = 0; i < 256; ++i) out[4 + i] = sk.second_worker[i];
  return (int)grid;
}

// The three queries read the plan the launch will read.  Their checks are lax on purpose: callers size buffers with half-filled descriptors.
extern "C" int64_t tribe_gemm_stream_k_workspace_bytes(const tribe_gemm_desc* d) {
  TRIBE_REQUIRE(d != nullptr && d->M > 0 && d->N > 0 && d->K > 0 && d->K % BK == 0, "tribe_gemm_stream_k_workspace_bytes: bad descriptor");
  return tribe_gemm_detail::gemm_plan(d, device_cu_count()).ws_need;   // 0 = not split -- also for a stream_k request whose operators the launch refuses
}

extern "C" int tribe_gemm_sumsq_slots(const tribe_gemm_desc* d) {
  TRIBE_REQUIRE(d != nullptr && d->M > 0 && d->N > 0 && d->K > 0 && d->batch1 > 0 && d->batch0 > 0, "tribe_gemm_sumsq_slots: bad descriptor");
  return (int)(d->N / tribe_gemm_detail::gemm_plan(d, device_cu_count()).sumsq_cols);
}

// which epilogue the launch of `desc` runs: 0 = the generic one (operators decided at run time), 1 = the 8-wave kernel's role-compiled one
// (epilogue_role), 2 = the one-wave-per-SIMD kernel's (epilogue_w4).  Host-side only: no GPU call.
extern "C" int tribe_gemm_epilogue_path(const tribe_gemm_desc* d) {
  TRIBE_REQUIRE(d != nullptr && d->M > 0 && d->N > 0 && d->K > 0 && d->batch1 > 0 && d->batch0 > 0, "tribe_gemm_epilogue_path: bad descriptor");
  return tribe_gemm_detail::gemm_plan(d, device_cu_count()).epilogue_path;
}

// Debug export (not in the header): what tribe_gemm_bf16 (fp8 = 0) or tribe_gemm_fp8 would launch for `d`, without launching it.
// out = {return code, kind, bm, bn, sumsq_cols, splits, pair, epilogue_path, tiles_m, tiles_n, nz, grid_x, reduce_grid_x, sk.tiles_dp,
// sk.rem_units, sk.q, sk.workers, second parts of the stream-K runs, ws_need}; all zero behind a non-zero return code (tribe_last_error).
extern "C" int tribe_debug_gemm_plan(const tribe_gemm_desc* d, int32_t fp8, int64_t* out, int32_t n) {
  using namespace tribe_gemm_detail;
  TRIBE_REQUIRE(out != nullptr && n >= 19, "tribe_debug_gemm_plan: out must hold %d entries", 19);
  GemmLaunch p{};
  int rc = fp8 ? gemm_fp8_resolve(d, "tribe_gemm_fp8", &p) : gemm_resolve(d, "tribe_gemm_bf16", device_cu_count(), &p);
  if (rc == 0 && !fp8) rc = gemm_check_workspace(d, "tribe_gemm_bf16", p);
  if (rc != 0) p = GemmLaunch{};
  const int64_t second = p.reduce_grid_x ? (int64_t)p.grid_x - p.sk.tiles_dp - p.sk.workers : 0;
  const int64_t all[19] = {rc, p.kind, p.bm, p.bn, p.sumsq_cols, p.splits, p.pair, p.epilogue_path, p.tiles_m, p.tiles_n, p.nz, p.grid_x,
                           p.reduce_grid_x, p.sk.tiles_dp, p.sk.rem_units, p.sk.q, p.sk.workers, second, p.ws_need};
  for (int i = 0; i < 19; ++i) out[i] = all[i];
  return rc;
}
