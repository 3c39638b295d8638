// batch.hip — gradients and Gauss-Newton moments of many candidate states
// against the resident cloud (include/flashsdf.h "gradients of candidate
// states"): per candidate the rows fsdf_eval_robust reduces at its poses —
// [S][29] (21 moments, the wrench, Σρ, Σw) or [S][8] — under the context's loss,
// weights and free-space split, nothing of the resident cloud's state written.
//
// Two designs serve this: (a) two launches per slice of candidates and a reduce,
// with a per-(candidate, point) buffer between them, or (b) one fused launch that
// keeps the lanes' carried sums in LDS. This is (a):
//   batch_eval_kernel, grid (score_groups(n), candidates): score_kernel's walk —
//     the candidate's hull table in LDS, four waves, the resident cloud in
//     64-point chunks with the resident chunk spheres, scene_eval without a
//     prior — but every valid lane stores what a pass stores for its point:
//     k* (4 B), d* (8 B) and ∇d* (24 B), widened as the pass widens them, into
//     the candidate's block of the slice buffer: k* [np] | d* [np] | ∇d* [np][3],
//     np = n rounded up to whole chunks (kBatchPointBytes · np bytes a block).
//   batch_robust_kernel, grid (robust_groups(n), candidates): robust_kernel's
//     statements (robust_body.inc) over candidate blockIdx.y's arrays.
//   batch_reduce_tiles_kernel, grid (tiles, candidates): the tile reduce's
//     statements (reduce_tiles_body.inc) over that candidate's partials.
// The fused design (b) would keep a lane's 29 carried sums (232 B per lane,
// 58 KB per workgroup) in LDS next to the hull table and the stages, and tie the
// reduction's run layout — whole contiguous runs per wave — to the evaluation's
// grid; (a) leaves both kernels what they are elsewhere, and its extra traffic
// (36 B written and read per (candidate, point)) is small against the evaluation.
// scene_eval's k*, d* and ∇d* are the pass's bit for bit with any seed, and the
// two reductions run the single launch's statements in its order, so candidate
// b's rows are fsdf_eval_robust's rows at b's poses, bit for bit, whatever the
// batch, b's place in it or the slicing. No floating-point atomics, no in-launch
// hand-off.

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

static size_t batch_eval_lds_bytes(const LocalModel& lm) {
  // the hull table, then the waves' stages (score_kernel's layout without its sums)
  return (size_t)(lm.K + 1) * sizeof(HullRow) + (size_t)(kScoreBlock / 64) * lm.stage_bytes;
}

extern __shared__ __attribute__((aligned(16))) char batch_lds[];

// grid (groups, candidates). m: the model with candidate 0's table; candidate
// b's lies b · stride bytes on, its block of out b · kBatchPointBytes · np bytes on.
template <typename T, int SLOTS, bool CULL>
__global__ __launch_bounds__(kScoreBlock, (SLOTS == 1 ? FSDF_PASS_WAVES_PER_SIMD : (SLOTS == 2 ? 3 : 2))) void
batch_eval_kernel(const T* __restrict__ pts, int64_t n, PassModel<T> m, size_t stride, const float* __restrict__ chunk_ws,
                  size_t np, char* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  // (wave-uniform, and readfirstlane tells the compiler so: score_kernel's note)
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.y;
  const size_t off = (size_t)b * stride;
  m.planes = (const T*)((const char*)m.planes + off);
  m.verts = (const T*)((const char*)m.verts + off);
  m.hull_rows = (const I4*)((const char*)m.hull_rows + off);
  if (sizeof(T) == 8) m.screen = (const float*)((const char*)m.screen + off);
  // dynamic LDS: hull table, 4 wave stages
  HullRow* ht = (HullRow*)batch_lds;
  char* stages = (char*)(ht + m.K + 1);
  T* stage = (T*)(stages + wave * m.stage_bytes);
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
    // (the point's index anew from an opaque copy of the lane: i and valid, live in registers
    // through scene_eval, were spilled to scratch at the f64 one-slot variant's budget of 128)
    int l = threadIdx.x & 63;
    asm volatile("" : "+v"(l));
    const int64_t io = base + l;
    if (io < n) {  // (io < n <= np: inside candidate b's arrays)
      char* blk = out + (size_t)b * kBatchPointBytes * np;  // (one base pointer: the SGPRs of three spilled)
      ((int32_t*)blk)[io] = bk;
      ((double*)(blk + 4 * np))[io] = (double)best;
      double* g = (double*)(blk + 12 * np) + 3 * io;
      g[0] = (double)gx;
      g[1] = (double)gy;
      g[2] = (double)gz;
    }
  }
}

extern __shared__ __attribute__((aligned(16))) double robust_tab[];  // [waves][S][LEN]

// grid (robust_groups(n), candidates), blockDim.x / 64 waves: robust_kernel over
// candidate blockIdx.y's per-point arrays (np entries apart) into its partials
// (plen doubles apart). The cloud, its weights and its permutation are shared.
template <typename T, bool MOMENTS, bool WEIGHTED, bool ONE_SIDED>
__global__ __launch_bounds__(kRobustBlock) void batch_robust_kernel(const T* __restrict__ pts,
                                                                    const char* __restrict__ points_all, int64_t n,
                                                                    int S, int run, int kind, double scale,
                                                                    double* __restrict__ partials_all,
                                                                    const double* __restrict__ conf,
                                                                    const int32_t* __restrict__ perm,
                                                                    int64_t n_surface, size_t np, size_t plen) {
  const size_t cand = blockIdx.y;
  const char* blk = points_all + cand * kBatchPointBytes * np;
  const int32_t* kstar = (const int32_t*)blk;
  const double* dstar = (const double*)(blk + 4 * np);
  const double* grad = (const double*)(blk + 12 * np);
  double* partials = partials_all + cand * plen;
#include "robust_body.inc"
}

// grid (tiles, candidates): reduce_tiles_kernel over candidate blockIdx.y's partials into its rows
__global__ __launch_bounds__(kTileBlock) void batch_reduce_tiles_kernel(const double* __restrict__ partials_all,
                                                                        int nblocks, int len,
                                                                        double* __restrict__ rows_all, size_t plen) {
  const double* partials = partials_all + (size_t)blockIdx.y * plen;
  double* accum = rows_all + (size_t)blockIdx.y * len;
#include "reduce_tiles_body.inc"
}

template <typename T, int SLOTS, bool CULL>
static void launch_batch_eval_v(const LocalModel& lm, const void* d_tables, const ScoreTable& t, const void* d_pts,
                                int64_t n, int nb, const float* d_chunk_ws, void* d_points, hipStream_t s) {
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
  const size_t lds = batch_eval_lds_bytes(lm);
  auto kernel = batch_eval_kernel<T, SLOTS, CULL>;
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  hipLaunchKernelGGL(kernel, dim3(score_groups(n), nb), dim3(kScoreBlock), lds, s, (const T*)d_pts, n, m, t.stride,
                     d_chunk_ws, batch_point_stride(n), (char*)d_points);
}

template <typename T>
static void launch_batch_eval_t(bool cull, const LocalModel& lm, const void* d_tables, const ScoreTable& t,
                                const void* d_pts, int64_t n, int nb, const float* d_chunk_ws, void* d_points,
                                hipStream_t s) {
#define FSDF_BATCH_LAUNCH(SLOTS)                                                                                  \
  do {                                                                                                            \
    if (cull)                                                                                                     \
      launch_batch_eval_v<T, SLOTS, true>(lm, d_tables, t, d_pts, n, nb, d_chunk_ws, d_points, s);   \
    else                                                                                                          \
      launch_batch_eval_v<T, SLOTS, false>(lm, d_tables, t, d_pts, n, nb, d_chunk_ws, d_points, s);  \
  } while (0)
  if (lm.S <= 64) FSDF_BATCH_LAUNCH(1);
  else if (lm.S <= 128) FSDF_BATCH_LAUNCH(2);
  else FSDF_BATCH_LAUNCH(4);
#undef FSDF_BATCH_LAUNCH
}

hipError_t launch_batch_eval(int precision, bool cull, const LocalModel& lm, const void* d_tables, const void* d_pts,
                             int64_t n, int nb, const float* d_chunk_ws, void* d_points, hipStream_t s) {
  if (nb <= 0) return hipSuccess;
  if (n <= 0 || nb > 65535 || !score_fits(lm) || !d_tables || !d_pts || !d_points)
    return hipErrorInvalidValue;
  const ScoreTable t = score_table(precision, lm);
  if (precision == 64)
    launch_batch_eval_t<double>(cull, lm, d_tables, t, d_pts, n, nb, d_chunk_ws, d_points, s);
  else
    launch_batch_eval_t<float>(cull, lm, d_tables, t, d_pts, n, nb, d_chunk_ws, d_points, s);
  return hipGetLastError();
}

hipError_t launch_batch_robust(int precision, bool moments, const void* d_pts, const void* d_points,
                               const double* d_conf, const int32_t* d_perm, int64_t n_surface,
                               int64_t n, int S, int nb, int kind, double scale, double* d_partials, double* d_rows,
                               hipStream_t s) {
  if (nb <= 0) return hipSuccess;
  if (n <= 0 || nb > 65535 || !robust_fit(S) || !robust::valid(kind, scale) || !d_pts || !d_points ||
      !d_partials || !d_rows)
    return hipErrorInvalidValue;
  // (launch_robust's grid, run, waves and LDS: functions of (n, S) alone)
  const int groups = robust_groups(n), run = (int)robust_run(n), waves = robust_waves(S), block = 64 * waves;
  const int len = moments ? kRobustLen : kRobustTail;
  const size_t lds = (size_t)waves * S * len * sizeof(double);
  const size_t np = batch_point_stride(n), plen = robust_partials_len(n, S);
#define FSDF_BATCH_ROBUST(T, M, W, O)                                                                               \
  hipLaunchKernelGGL((batch_robust_kernel<T, M, W, O>), dim3(groups, nb), dim3(block), lds, s, (const T*)d_pts,    \
                     (const char*)d_points, n, S, run, kind, scale, d_partials, d_conf, d_perm, n_surface, np, plen)
#define FSDF_BATCH_ROBUST_M(T, W, O)              \
  do {                                            \
    if (moments) FSDF_BATCH_ROBUST(T, true, W, O); \
    else FSDF_BATCH_ROBUST(T, false, W, O);        \
  } while (0)
#define FSDF_BATCH_ROBUST_W(T, O)                 \
  do {                                            \
    if (d_conf) FSDF_BATCH_ROBUST_M(T, true, O);  \
    else FSDF_BATCH_ROBUST_M(T, false, O);        \
  } while (0)
  if (precision == 64) {
    if (n_surface >= 0) FSDF_BATCH_ROBUST_W(double, true);
    else FSDF_BATCH_ROBUST_W(double, false);
  } else {
    if (n_surface >= 0) FSDF_BATCH_ROBUST_W(float, true);
    else FSDF_BATCH_ROBUST_W(float, false);
  }
#undef FSDF_BATCH_ROBUST_W
#undef FSDF_BATCH_ROBUST_M
#undef FSDF_BATCH_ROBUST
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // a candidate's partials in workgroup order (launch_reduce's grid per candidate)
  hipLaunchKernelGGL(batch_reduce_tiles_kernel, dim3((len * S + 7) / 8, nb), dim3(kTileBlock), 0, s, d_partials,
                     groups, len * S, d_rows, plen);
  return hipGetLastError();
}

}  // namespace fsdf
