// score.hip — many candidate states scored against the resident cloud in one
// launch (include/flashsdf.h "scoring candidate states"): the cost alone, no
// gradient, no per-point output, nothing of the resident cloud's state written.
//
// A batch of B candidates is B posed models side by side in one buffer (a
// candidate's table: world planes, world vertices, the hull table, and in f64
// contexts the fp32 screening pairs — what scene_eval reads without the stage
// images, ScoreTable), written by ONE pose launch with grid.y = candidate
// (pose_impl.h pose_item, the single-state pose's arithmetic and so its bits).
//
// The score launch is a grid of (score_groups(n), B) workgroups of four waves.
// A workgroup copies candidate b's hull table into LDS (load_hull_table, as
// raycast_kernel), and its waves walk the resident cloud in resident order in
// 64-point chunks, grid-strided: wave w of group g takes the chunks 4 g + w,
// 4 (g + groups) + w, ... Each chunk is one scene_eval without a prior (any
// seed gives the same d*, bit for bit) over the chunk's precomputed bounding
// sphere. A valid lane's term is formed in fp64 from its d* as stored:
//   t = a · ρ(d*),  a = one_sided_factor(free, d*, weight)   (robust_impl.h)
// — the term robust_kernel sums into Σρ — and summed lane → wave (wave_sum) →
// workgroup (LDS, wave order) → partials[b][g]; a second small launch sums a
// candidate's partials in index order. No floating-point atomics, no in-launch
// hand-off. score_groups is a function of n alone and a candidate's workgroups
// read only its own table, so a candidate's bits depend neither on B nor on its
// place in the batch nor on how the host slices the batch.

#include "fsdf_internal.h"
#include "pose_impl.h"

#include <algorithm>

#include "sdf_device_math.h"
#include "wave_times.h"
#include "hull_sdf.h"
#include "rbf_sdf.h"
#include "scene_eval.h"
#include "robust_impl.h"

namespace fsdf {

static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

ScoreTable score_table(int precision, const LocalModel& lm) {
  const size_t tsz = precision == 64 ? sizeof(double) : sizeof(float);
  ScoreTable t;
  t.planes = 0;
  t.verts = align256(t.planes + (size_t)lm.F * 4 * tsz);
  t.rows = align256(t.verts + (size_t)lm.V * 4 * tsz);
  t.screen = align256(t.rows + (size_t)(lm.K + 1) * sizeof(HullRow));
  t.stride = precision == 64 ? align256(t.screen + (size_t)(lm.F + lm.K) * 4 * sizeof(float)) : t.screen;
  return t;
}

int score_groups(int64_t n) {
  const int64_t nc = (n + 63) / 64, per = kScoreBlock / 64;
  return (int)std::min<int64_t>(std::max<int64_t>((nc + per - 1) / per, 1), kScoreMaxGroups);
}

static size_t score_lds_bytes(const LocalModel& lm) {
  // the hull table, the waves' stages (raycast_kernel's layout), then the lanes' and the waves' sums
  return (size_t)(lm.K + 1) * sizeof(HullRow) + (size_t)(kScoreBlock / 64) * lm.stage_bytes +
         (size_t)(kScoreBlock + kScoreBlock / 64) * sizeof(double);
}

bool score_fits(const LocalModel& lm) {
  return lm.R == 0 && lm.K >= 1 && lm.K <= kMaxHulls && lm.S == lm.K && score_lds_bytes(lm) <= (size_t)kMaxLds;
}

// grid (pose workgroups, candidates): candidate b's poses [S][12] -> its table
template <typename T>
__global__ __launch_bounds__(kBlock) void score_pose_kernel(LocalModel lm, const double* __restrict__ poses,
                                                            char* __restrict__ tables, ScoreTable t) {
  const int b = blockIdx.y;
  char* tab = tables + (size_t)b * t.stride;
  pose_item<T>(lm, poses + (size_t)12 * lm.S * b, (T*)(tab + t.planes), (HullRow*)(tab + t.rows),
               (T*)(tab + t.verts), sizeof(T) == 8 ? (float*)(tab + t.screen) : nullptr, nullptr,
               (int)(blockIdx.x * blockDim.x + threadIdx.x));
}

extern __shared__ __attribute__((aligned(16))) char score_lds[];

// grid (groups, candidates). m: the model with candidate 0's table; candidate
// b's lies b · stride bytes on.
template <typename T, int SLOTS, bool CULL>
__global__ __launch_bounds__(kScoreBlock, (SLOTS == 1 ? FSDF_PASS_WAVES_PER_SIMD : (SLOTS == 2 ? 3 : 2))) void
score_kernel(const T* __restrict__ pts, int64_t n, PassModel<T> m, size_t stride, const float* __restrict__ chunk_ws,
             const double* __restrict__ conf, const int32_t* __restrict__ perm, int64_t n_surface, int kind,
             double scale, double* __restrict__ partials) {
  const int lane = threadIdx.x & 63;
  // (wave-uniform, and readfirstlane tells the compiler so: the wave's stage address and the chunk
  // loop stay out of the vector registers, which scene_eval fills to the budget — pass_kernel's note)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y;
  const size_t off = (size_t)b * stride;
  m.planes = (const T*)((const char*)m.planes + off);
  m.verts = (const T*)((const char*)m.verts + off);
  m.hull_rows = (const I4*)((const char*)m.hull_rows + off);
  if (sizeof(T) == 8) m.screen = (const float*)((const char*)m.screen + off);
  // dynamic LDS: hull table, 4 wave stages, the lanes' running sums, 4 wave sums
  HullRow* ht = (HullRow*)score_lds;
  char* stages = (char*)(ht + m.K + 1);
  T* stage = (T*)(stages + wave * m.stage_bytes);
  // (a lane's running sum lives in LDS between chunks: live in registers through scene_eval it
  // was spilled to scratch at the f64 one-slot variant's budget of 128)
  double* lsum = (double*)(stages + (kScoreBlock / 64) * m.stage_bytes);
  double* wsum = lsum + kScoreBlock;
  lsum[threadIdx.x] = 0.0;
  const float smax = load_hull_table(m, ht);
  const int64_t step = (int64_t)gridDim.x * kScoreBlock;
  for (int64_t base = (int64_t)blockIdx.x * kScoreBlock + wave * 64; base < n; base += step) {
    const int64_t i = base + lane;
    const bool valid = i < n;
    const int64_t ii = valid ? i : n - 1;
    const T px = pts[3 * ii + 0], py = pts[3 * ii + 1], pz = pts[3 * ii + 2];
    const F4* cws = chunk_ws ? (const F4*)chunk_ws + (base >> 6) : nullptr;
    T best, gx, gy, gz;
    int bk;
    scene_eval<T, SLOTS, CULL, false>(px, py, pz, valid, m, ht, smax, stage, nullptr, best, bk, gx, gy, gz, cws);
    if (valid) {
      const double d = (double)best;
      const bool free = n_surface >= 0 && robust::free_sample(perm ? (int64_t)perm[i] : i, n_surface);
      const double a = robust::one_sided_factor(free, d, conf ? conf[i] : 1.0);
      lsum[threadIdx.x] += a * robust::rho(kind, scale, d);
    }
  }
  const double acc = wave_sum(lsum[threadIdx.x]);
  if (lane == 0) wsum[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = wsum[0];
#pragma unroll
    for (int w = 1; w < kScoreBlock / 64; ++w) s += wsum[w];
    partials[(size_t)b * gridDim.x + blockIdx.x] = s;
  }
}

// cost[b] = partials[b][0] + partials[b][1] + ... in index order (a thread per candidate)
__global__ __launch_bounds__(kBlock) void score_finish_kernel(const double* __restrict__ partials, int groups, int B,
                                                              double* __restrict__ cost) {
  const int b = blockIdx.x * kBlock + threadIdx.x;
  if (b >= B) return;
  const double* p = partials + (size_t)b * groups;
  double s = p[0];
  for (int g = 1; g < groups; ++g) s += p[g];
  cost[b] = s;
}

hipError_t launch_score_pose(int precision, const LocalModel& lm, const double* d_poses, int B, void* d_tables,
                             hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (!d_poses || !d_tables || B > 65535) return hipErrorInvalidValue;
  const ScoreTable t = score_table(precision, lm);
  const int grid = (pose_items(lm) + kBlock - 1) / kBlock;
  if (precision == 64)
    hipLaunchKernelGGL(score_pose_kernel<double>, dim3(grid, B), dim3(kBlock), 0, s, lm, d_poses, (char*)d_tables, t);
  else
    hipLaunchKernelGGL(score_pose_kernel<float>, dim3(grid, B), dim3(kBlock), 0, s, lm, d_poses, (char*)d_tables, t);
  return hipGetLastError();
}

template <typename T, int SLOTS, bool CULL>
static void launch_score_v(const LocalModel& lm, const void* d_tables, const ScoreTable& t, const void* d_pts,
                           int64_t n, int B, const float* d_chunk_ws, const double* d_conf, const int32_t* d_perm,
                           int64_t n_surface, int kind, double scale, double* d_partials, hipStream_t s) {
  PassModel<T> m;
  m.K = lm.K;
  m.S = lm.S;
  m.R = 0;
  m.stage_bytes = lm.stage_bytes;
  m.planes64 = 0;  // (no stage images: hull_sdf's P64 = false layout)
  m.hull_surface = lm.hull_surface;
  m.surface_kind = lm.surface_kind;
  m.rbf_surface = nullptr;
  m.rbf_row_off = nullptr;
  m.rbf_acc_off = nullptr;
  m.rbf_rows = nullptr;
  m.face_rows = (const I4*)lm.face_rows;
  const char* tab = (const char*)d_tables;
  m.planes = (const T*)(tab + t.planes);
  m.verts = (const T*)(tab + t.verts);
  m.hull_rows = (const I4*)(tab + t.rows);
  m.screen = sizeof(T) == 8 ? (const float*)(tab + t.screen) : nullptr;
  m.image = nullptr;
  const size_t lds = score_lds_bytes(lm);
  auto kernel = score_kernel<T, SLOTS, CULL>;
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, dim3(score_groups(n), B), dim3(kScoreBlock), lds, s, (const T*)d_pts, n, m, t.stride,
                     d_chunk_ws, d_conf, d_perm, n_surface, kind, scale, d_partials);
}

template <typename T>
static void launch_score_t(bool cull, const LocalModel& lm, const void* d_tables, const ScoreTable& t,
                           const void* d_pts, int64_t n, int B, const float* d_chunk_ws, const double* d_conf,
                           const int32_t* d_perm, int64_t n_surface, int kind, double scale, double* d_partials,
                           hipStream_t s) {
#define FSDF_SCORE_LAUNCH(SLOTS)                                                                                    \
  do {                                                                                                              \
    if (cull)                                                                                                       \
      launch_score_v<T, SLOTS, true>(lm, d_tables, t, d_pts, n, B, d_chunk_ws, d_conf, d_perm, n_surface, kind,    \
                                     scale, d_partials, s);                                                        \
    else                                                                                                            \
      launch_score_v<T, SLOTS, false>(lm, d_tables, t, d_pts, n, B, d_chunk_ws, d_conf, d_perm, n_surface, kind,   \
                                      scale, d_partials, s);                                                       \
  } while (0)
  if (lm.S <= 64) FSDF_SCORE_LAUNCH(1);
  else if (lm.S <= 128) FSDF_SCORE_LAUNCH(2);
  else FSDF_SCORE_LAUNCH(4);
#undef FSDF_SCORE_LAUNCH
}

hipError_t launch_score(int precision, bool cull, const LocalModel& lm, const void* d_tables, const void* d_pts,
                        int64_t n, int B, const float* d_chunk_ws, const double* d_conf, const int32_t* d_perm,
                        int64_t n_surface, int kind, double scale, double* d_partials, double* d_cost,
                        hipStream_t s) {
  if (B <= 0) return hipSuccess;
  if (n <= 0 || B > 65535 || !score_fits(lm) || !robust::valid(kind, scale) || !d_tables || !d_pts || !d_partials ||
      !d_cost)
    return hipErrorInvalidValue;
  const ScoreTable t = score_table(precision, lm);
  if (precision == 64)
    launch_score_t<double>(cull, lm, d_tables, t, d_pts, n, B, d_chunk_ws, d_conf, d_perm, n_surface, kind, scale,
                           d_partials, s);
  else
    launch_score_t<float>(cull, lm, d_tables, t, d_pts, n, B, d_chunk_ws, d_conf, d_perm, n_surface, kind, scale,
                          d_partials, s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(score_finish_kernel, dim3((B + kBlock - 1) / kBlock), dim3(kBlock), 0, s, d_partials,
                     score_groups(n), B, d_cost);
  return hipGetLastError();
}

}  // namespace fsdf
