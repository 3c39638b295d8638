// sdf_kernels.hip — the residual pass of Flash.jl on CDNA4 (gfx950).
//
// Reference semantics (src/Flash.jl:265-268, src/gradientdescent.jl:28-39):
//   d*(p)  = minimum(s_k(p) for k in surfaces)       first k wins ties
//   s_k(p) = gjk!(cache, pose_k, Translation(p)).signed_distance   (:238-243)
//   c      = Σ_p d*(p)^2
// restated here as the EXACT signed distance to the convex polytope conv(V_k):
//   inside / on the surface:  max_f (n_f·p − d_f)
//   outside:                  Euclidean distance to the closest boundary point
// (EnhancedGJK returns the same value outside; its penetration value inside is a
//  termination-simplex estimate and is replaced by the exact one — DESIGN.md §2).
//
// Kernel design:
//   * one lane per point; each wave owns 64 consecutive (Hilbert-ordered)
//     resident points;
//   * exact-safe culling: hulls are dropped for the whole wave from its
//     bounding sphere, then per lane by |p−c_k|−r_k against min(upper bound,
//     best so far) plus a rounding margin; a wave evaluates hull k iff any
//     lane needs it, each lane's best-first seed first;
//   * a hull evaluation stages the hull once into the wave's LDS stage; the
//     plane max is an fp32 screen (packed FMA, two faces per instruction) with
//     an exact fp64 fix-up, and the closest feature a certified descent walk;
//   * per-hull wrench sums are segmented by k* inside the wave (ballot loop +
//     DPP sums), owned in LDS rows by lane k mod 64, combined per block in
//     fixed wave order, then reduced over blocks in fixed order: the whole
//     reduction is deterministic for a given (n, grid).
//
// All arithmetic is written with explicit fma() and compiled with
// -ffp-contract=off so that oracle/flash_oracle.c reproduces every per-hull
// value bit for bit (the argmin k* must match exactly).
//
// One translation unit: the device code lives in the headers below, by concern
// (DESIGN.md §1); this file keeps the pose and per-cloud kernels and every
// launcher.

#include "fsdf_internal.h"
#include "pose_impl.h"

#include <hip/hip_ext.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sdf_device_math.h"  // fma / sqrt by precision, triangle and plane primitives, DPP wave reductions
#include "wave_times.h"       // hooks of the per-wave timeline build
#include "hull_sdf.h"         // PassModel, LDS hull table and stage, fp32 screen, closest-feature walk, hull_sdf
#include "rbf_sdf.h"          // RBF skins: field, signed distance, adjoint
#include "scene_eval.h"       // scene_eval and the chunk epilogue
#include "pass_kernels.h"     // pass_kernel, planned_pass_kernel, raycast_kernel
#include "reduce_kernels.h"   // chunk-group sums, plan, tile reduce, block order

namespace fsdf {

// (pose_item, the pose's work items: pose_impl.h)
template <typename T>
__device__ __forceinline__ void pose_body(const LocalModel& lm, const double* __restrict__ poses,
                                          T* __restrict__ planes_w, HullRow* __restrict__ hull_rows,
                                          T* __restrict__ verts_w, float* __restrict__ screen_w,
                                          I4* __restrict__ image_w) {
  pose_item<T>(lm, poses, planes_w, hull_rows, verts_w, screen_w, image_w,
               (int)(blockIdx.x * blockDim.x + threadIdx.x));
}

// Poses from global memory (uploaded by a copy), or — for up to kPoseArgMax
// surfaces — straight from the kernel arguments: the launch carries the 12·S
// doubles, each workgroup copies them into LDS, and the per-pass host-to-device
// copy (a blit kernel of its own) disappears from the step.
// skip (optional): a device flag; set, the launch does nothing (the device
// solver loop's passes after convergence, solver.hip)
template <typename T>
__global__ __launch_bounds__(kBlock) void pose_kernel(LocalModel lm, const double* __restrict__ poses,
                                                      T* __restrict__ planes_w, HullRow* __restrict__ hull_rows,
                                                      T* __restrict__ verts_w, float* __restrict__ screen_w,
                                                      I4* __restrict__ image_w, const int* __restrict__ skip) {
  if (skip && *skip) return;
  pose_body<T>(lm, poses, planes_w, hull_rows, verts_w, screen_w, image_w);
}
template <typename T>
__global__ __launch_bounds__(kBlock) void pose_kernel_args(LocalModel lm, PoseArgs pa, T* __restrict__ planes_w,
                                                           HullRow* __restrict__ hull_rows, T* __restrict__ verts_w,
                                                           float* __restrict__ screen_w, I4* __restrict__ image_w) {
  __shared__ double sp[12 * kPoseArgMax];
  for (int i = threadIdx.x; i < 12 * lm.S; i += kBlock) sp[i] = pa.v[i];
  __syncthreads();
  pose_body<T>(lm, sp, planes_w, hull_rows, verts_w, screen_w, image_w);
}

// Per-chunk bounding spheres of a resident cloud (one wave per 64 points),
// read by the pass kernel instead of recomputing them every pass. `nchunks`
// may exceed ceil(n/64) (padding to whole pass workgroups): a chunk past the
// cloud's end gets the zero-radius sphere of the last point, so a
// hull-partitioned workgroup's empty second chunk reads a defined row.
template <typename T>
__global__ __launch_bounds__(kBlock) void chunk_sphere_kernel(const T* __restrict__ pts, int64_t n, int64_t nchunks,
                                                              F4* __restrict__ out) {
  const int64_t base = ((int64_t)blockIdx.x * kBlock + threadIdx.x) & ~(int64_t)63;
  if (base >= 64 * nchunks) return;  // wave-uniform
  const int64_t i = base + (threadIdx.x & 63);
  const bool valid = i < n;
  const int64_t ii = valid ? i : n - 1;
  const WaveSphere ws = wave_sphere((float)pts[3 * ii], (float)pts[3 * ii + 1], (float)pts[3 * ii + 2], valid);
  if ((threadIdx.x & 63) == 0) out[base >> 6] = F4{ws.x, ws.y, ws.z, ws.r};
}

__global__ void to_f32_kernel(const double* __restrict__ src, float* __restrict__ dst, int64_t count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) dst[i] = (float)src[i];
}

// ---------------------------------------------------------------------------
// Launchers
// ---------------------------------------------------------------------------
// workgroups of the hull-partitioned and the one-chunk-per-wave pass
// (pass_kernel NB; 512-thread workgroups measured slower for both)
constexpr int kHpartBlock = kPassBlock;
// hpart_default_limits: models with at least kHpartFullHulls hulls use the
// M64-measured tiers, smaller ones kHpartSmall4 / kHpartSmall2 (measured on
// IRB140, C2)
constexpr int kHpartFullHulls = 32;
constexpr int64_t kHpartSmall4 = 98304;
constexpr int64_t kHpartSmall2 = 327680;
// planned pass up to (fsdf_set_plan max_points -1): above it the unplanned
// grid measured faster — M64 between 2^19 and 2^20 points, IRB140 between
// 393,216 and 2^19 (the planned reduction's extra launch outweighs a pass that
// is already short; profiles/r04/hpart_sweep_c2.jsonl)
constexpr int64_t kPlanMaxFull = 524288;
constexpr int64_t kPlanMaxSmall = 393216;
// ... and from above kPlanMinPoints: below it the unplanned 4-way tier measured
// faster for both models (2^16 points: M64 0.0644 vs 0.0662 ms, IRB140 0.0433
// vs 0.0448 — the planned reduction's second launch is not paid back)
constexpr int64_t kPlanMinPoints = 98304;
constexpr int kAliasBlock = kPassBlock;

// the aliased pass's LDS plus the hull-partitioned pass's shared per-lane bests
// (one 64-double slot row per chunk of the workgroup)
static size_t hpart_lds_bytes(const LocalModel& lm, int parts) {
  return (size_t)(kHpartBlock / 64) * lm.stage_bytes + (size_t)(lm.K + 1) * sizeof(HullRow) +
         (size_t)kHpartBlock / parts * sizeof(double);
}

// Waves per chunk of the hull-partitioned pass (pass_kernel HPART) for a cloud
// of n points, 0 = the one-wave-per-chunk pass: kHpart (4) up to the model's
// hpart4 limit, 2 up to its hpart2 limit (LocalModel; fsdf_set_partition
// overrides them per context, 0 disables a tier).
void hpart_default_limits(const LocalModel& lm, int64_t* four, int64_t* two) {
  // Measured crossovers (same-box size sweeps of every tier):
  // M64 (64 hulls) 4-way up to 196,608 points, 2-way up to 393,216
  // (profiles/r04/plan_sweeps_r04def.jsonl); IRB140 (7 hulls) 4-way up to
  // 98,304, 2-way up to 327,680 (profiles/r04/hpart_sweep_c2.jsonl: 4-way
  // best at 2^16, 2-way at 2^17..2^18, one wave from 393,216)
  if (lm.K >= kHpartFullHulls) {
    *four = 196608;
    *two = 393216;
  } else {
    *four = kHpartSmall4;
    *two = kHpartSmall2;
  }
}

int64_t planned_default_max_points(const LocalModel& lm) {
  return lm.K >= kHpartFullHulls ? kPlanMaxFull : kPlanMaxSmall;
}
int64_t planned_default_min_points() { return kPlanMinPoints; }

int hpart_parts(const LocalModel& lm, int64_t n) {
  if (!(lm.planes64 && lm.S <= 64 && lm.R == 0 && n > 0)) return 0;
  int64_t limit4, limit2;
  hpart_default_limits(lm, &limit4, &limit2);
  if (lm.hpart4_points >= 0) limit4 = lm.hpart4_points;
  if (lm.hpart2_points >= 0) limit2 = lm.hpart2_points;
  const int parts = n <= limit4 ? kHpart : (n <= limit2 ? 2 : 0);
  if (!parts) return 0;
  const int64_t per = kHpartBlock / parts;  // points per workgroup
  if ((n + per - 1) / per > kMaxBlocks) return 0;
  if (hpart_lds_bytes(lm, parts) > (size_t)kLdsPerCu * kHpartBlock / 1024) return 0;  // (4 waves per SIMD)
  return parts;
}
bool hpart_pass(const LocalModel& lm, int64_t n) { return hpart_parts(lm, n) > 0; }

static bool alias_pass(const LocalModel& lm, int64_t n) {
  return lm.planes64 && lm.S <= 64 && lm.R == 0 && n > 0 && (n + kAliasBlock - 1) / kAliasBlock <= kMaxBlocks;
}
static size_t alias_lds_bytes(const LocalModel& lm) {
  return (size_t)(kAliasBlock / 64) * lm.stage_bytes + (size_t)(lm.K + 1) * sizeof(HullRow);
}

int pass_blocks(int64_t n, const LocalModel& lm) {
  if (const int parts = hpart_parts(lm, n)) return (int)((n + kHpartBlock / parts - 1) / (kHpartBlock / parts));
  if (alias_pass(lm, n)) return (int)((n + kAliasBlock - 1) / kAliasBlock);
  int64_t b = (n + kPassBlock - 1) / kPassBlock;
  if (b < 1) b = 1;
  if (b > kMaxBlocks) b = kMaxBlocks;
  return (int)b;
}

hipError_t launch_pose(int precision, const LocalModel& lm, const double* d_poses, const PosedModel& pm,
                       hipStream_t s, const double* h_poses, const int* skip) {
  const int total = ((lm.F + lm.V + 63) & ~63) + 64 * lm.K;
  if (total == 0) return hipSuccess;  // RBF-only scene: nothing to pose
  const int grid = (total + kBlock - 1) / kBlock;
  if (h_poses) {
    PoseArgs pa;
    memcpy(pa.v, h_poses, (size_t)12 * lm.S * sizeof(double));
    if (precision == 64)
      hipLaunchKernelGGL(pose_kernel_args<double>, dim3(grid), dim3(kBlock), 0, s, lm, pa, (double*)pm.planes_w,
                         (HullRow*)pm.hull_rows, (double*)pm.verts_w, pm.screen_w, (I4*)pm.image_w);
    else
      hipLaunchKernelGGL(pose_kernel_args<float>, dim3(grid), dim3(kBlock), 0, s, lm, pa, (float*)pm.planes_w,
                         (HullRow*)pm.hull_rows, (float*)pm.verts_w, (float*)nullptr, (I4*)nullptr);
    return hipGetLastError();
  }
  if (precision == 64) {
    hipLaunchKernelGGL(pose_kernel<double>, dim3(grid), dim3(kBlock), 0, s, lm, d_poses,
                       (double*)pm.planes_w, (HullRow*)pm.hull_rows, (double*)pm.verts_w, pm.screen_w,
                       (I4*)pm.image_w, skip);
  } else {
    hipLaunchKernelGGL(pose_kernel<float>, dim3(grid), dim3(kBlock), 0, s, lm, d_poses, (float*)pm.planes_w,
                       (HullRow*)pm.hull_rows, (float*)pm.verts_w, (float*)nullptr, (I4*)nullptr, skip);
  }
  return hipGetLastError();
}

template <typename T>
static PassModel<T> pass_model(const LocalModel& lm, const PosedModel& pm) {
  PassModel<T> m;
  m.K = lm.K;
  m.S = lm.S;
  m.R = lm.R;
  m.stage_bytes = lm.stage_bytes;
  m.planes64 = lm.planes64;
  m.hull_surface = lm.hull_surface;
  m.surface_kind = lm.surface_kind;
  m.rbf_surface = lm.rbf_surface;
  m.rbf_row_off = lm.rbf_row_off;
  m.rbf_acc_off = lm.rbf_acc_off;
  m.rbf_rows = (const T*)pm.rbf_rows;
  m.face_rows = (const I4*)lm.face_rows;
  m.planes = (const T*)pm.planes_w;
  m.verts = (const T*)pm.verts_w;
  m.hull_rows = (const I4*)pm.hull_rows;
  m.screen = pm.screen_w;
  m.image = (const I4*)pm.image_w;
  return m;
}

static int slots_for(int S) { return S <= 64 ? 1 : (S <= 128 ? 2 : 4); }

size_t pass_lds_bytes(const LocalModel& lm, bool raycast, bool alias) {
  const size_t waves = (size_t)(raycast ? kBlock : kPassBlock) / 64;
  const size_t stage = waves * (size_t)lm.stage_bytes + (size_t)(lm.K + 1) * sizeof(HullRow);
  if (raycast || alias) return stage;
  const size_t red = waves * (size_t)(slots_for(lm.S) * 64 * 6 + 2) * sizeof(double);
  const size_t rbf = lm.R > 0 ? waves * kMaxRbfAcc * sizeof(double) : 0;
  return red + rbf + stage;
}

// start/stop events of the next pass launch (launch_pass; this thread only):
// hipExtLaunchKernel stamps them in the dispatch itself, where a separate
// hipEventRecord is a stream packet of its own that held the next kernel
// back by ~5-10 us (profiles/r03, step_trace)
static thread_local hipEvent_t g_pass_ev0 = nullptr, g_pass_ev1 = nullptr;

template <typename K, typename... Args>
static void launch_lds(K kernel, int grid, int block, size_t lds, hipStream_t s, Args... args) {
  if (lds > 65536) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (g_pass_ev0 || g_pass_ev1) {
    hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), (uint32_t)lds, s, g_pass_ev0, g_pass_ev1, 0u, args...);
    g_pass_ev0 = g_pass_ev1 = nullptr;
  } else {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, s, args...);
  }
}

static thread_local char g_pass_name[96] = "";
const char* last_pass_kernel() { return g_pass_name; }

template <typename T> constexpr const char* type_name();
template <> constexpr const char* type_name<double>() { return "double"; }
template <> constexpr const char* type_name<float>() { return "float"; }

// launch one pass_kernel variant and record its name (last_pass_kernel)
template <typename T, int SLOTS, bool CULL, bool RBF, bool ALIAS = false, bool HPART = false, int NB = kPassBlock,
          int NPART = kHpart>
static void launch_pass_variant(int grid, size_t lds, hipStream_t s, const T* pts, int64_t n, const PassModel<T>& m,
                                const PassOutputs& out) {
  auto b = [](bool v) { return v ? "true" : "false"; };
  snprintf(g_pass_name, sizeof g_pass_name, "pass_kernel<%s, %d, %s, %s, %s, %s, %d, %d>", type_name<T>(), SLOTS,
           b(CULL), b(RBF), b(ALIAS), b(HPART), NB, NPART);
  launch_lds(pass_kernel<T, SLOTS, CULL, RBF, ALIAS, HPART, NB, NPART>, grid, NB, lds, s, pts, n, m, out);
}

template <typename T, bool CULL, bool RBF>
static void launch_pass_t(const LocalModel& lm, const PosedModel& pm, const void* d_pts, int64_t n, int nblocks,
                          const PassOutputs& out, hipStream_t s) {
  const PassModel<T> m = pass_model<T>(lm, pm);
  const T* pts = (const T*)d_pts;
  const size_t lds = pass_lds_bytes(lm, false);
  if constexpr (!RBF) {
    // one chunk per wave: the wrench rows alias the stage (pass_kernel ALIAS)
    if (const int parts = hpart_parts(lm, n)) {
      if (parts == kHpart)
        launch_pass_variant<T, 1, CULL, false, true, true, kHpartBlock, kHpart>(nblocks, hpart_lds_bytes(lm, parts), s,
                                                                                pts, n, m, out);
      else
        launch_pass_variant<T, 1, CULL, false, true, true, kHpartBlock, 2>(nblocks, hpart_lds_bytes(lm, parts), s, pts,
                                                                           n, m, out);
      return;
    }
    if (alias_pass(lm, n) && (int64_t)nblocks * kAliasBlock >= n) {
      launch_pass_variant<T, 1, CULL, false, true, false, kAliasBlock>(nblocks, alias_lds_bytes(lm), s, pts, n, m, out);
      return;
    }
  }
  if (lm.S <= 64) launch_pass_variant<T, 1, CULL, RBF>(nblocks, lds, s, pts, n, m, out);
  else if (lm.S <= 128) launch_pass_variant<T, 2, CULL, RBF>(nblocks, lds, s, pts, n, m, out);
  else launch_pass_variant<T, 4, CULL, RBF>(nblocks, lds, s, pts, n, m, out);
}

// FSDF_BENCH_ONLY=1: A/B timing builds instantiate only the bench variant
// (f64, culled, hulls only, <= 64 surfaces); every other pass is refused.
template <typename T>
static void launch_pass_p(bool cull, const LocalModel& lm, const PosedModel& pm, const void* d_pts, int64_t n,
                          int nblocks, const PassOutputs& out, hipStream_t s) {
#if FSDF_BENCH_ONLY
  const PassModel<T> m = pass_model<T>(lm, pm);
  const int parts = hpart_parts(lm, n);
  const T* pts = (const T*)d_pts;
  if (parts == kHpart)
    launch_pass_variant<T, 1, true, false, true, true, kHpartBlock, kHpart>(nblocks, hpart_lds_bytes(lm, parts), s,
                                                                            pts, n, m, out);
  else if (parts == 2)
    launch_pass_variant<T, 1, true, false, true, true, kHpartBlock, 2>(nblocks, hpart_lds_bytes(lm, parts), s, pts, n,
                                                                       m, out);
  else if (alias_pass(lm, n) && (int64_t)nblocks * kAliasBlock >= n)
    launch_pass_variant<T, 1, true, false, true, false, kAliasBlock>(nblocks, alias_lds_bytes(lm), s, pts, n, m, out);
  else
    launch_pass_variant<T, 1, true, false>(nblocks, pass_lds_bytes(lm, false), s, pts, n, m, out);
#else
  if (lm.R > 0) {
    if (cull) launch_pass_t<T, true, true>(lm, pm, d_pts, n, nblocks, out, s);
    else launch_pass_t<T, false, true>(lm, pm, d_pts, n, nblocks, out, s);
  } else {
    if (cull) launch_pass_t<T, true, false>(lm, pm, d_pts, n, nblocks, out, s);
    else launch_pass_t<T, false, false>(lm, pm, d_pts, n, nblocks, out, s);
  }
#endif
}

hipError_t launch_pass(int precision, bool cull, const LocalModel& lm, const PosedModel& pm, const void* d_pts,
                       int64_t n, int nblocks, const PassOutputs& out, hipStream_t s, hipEvent_t ev_start,
                       hipEvent_t ev_stop) {
  // the events belong to this call only: cleared on every exit (a refused or
  // failed launch must not leave them for the next launch_lds on this thread)
  struct ClearEvents {
    ~ClearEvents() { g_pass_ev0 = g_pass_ev1 = nullptr; }
  } clear_events;
  g_pass_name[0] = 0;
  g_pass_ev0 = ev_start;
  g_pass_ev1 = ev_stop;
#if FSDF_BENCH_ONLY
  if (precision != 64 || !cull || lm.R > 0 || lm.S > 64) return hipErrorNotSupported;
  launch_pass_p<double>(cull, lm, pm, d_pts, n, nblocks, out, s);
#else
  if (precision == 64) launch_pass_p<double>(cull, lm, pm, d_pts, n, nblocks, out, s);
  else launch_pass_p<float>(cull, lm, pm, d_pts, n, nblocks, out, s);
#endif
  return hipGetLastError();
}

template <typename T, bool CULL, bool RBF>
static void launch_raycast_t(const LocalModel& lm, const PosedModel& pm, const double* origin, const double* rays,
                             int64_t n, double* depth, hipStream_t s) {
  const PassModel<T> m = pass_model<T>(lm, pm);
  const RayOrigin o{origin[0], origin[1], origin[2]};
  const int nb = (int)std::min<int64_t>((n + kBlock - 1) / kBlock, kMaxBlocks);
  const size_t lds = pass_lds_bytes(lm, true);
  if (lm.S <= 64) launch_lds(raycast_kernel<T, 1, CULL, RBF>, nb, kBlock, lds, s, o, rays, n, m, depth);
  else if (lm.S <= 128) launch_lds(raycast_kernel<T, 2, CULL, RBF>, nb, kBlock, lds, s, o, rays, n, m, depth);
  else launch_lds(raycast_kernel<T, 4, CULL, RBF>, nb, kBlock, lds, s, o, rays, n, m, depth);
}

template <typename T>
static void launch_raycast_p(bool cull, const LocalModel& lm, const PosedModel& pm, const double* origin,
                             const double* rays, int64_t n, double* depth, hipStream_t s) {
  if (lm.R > 0) {
    if (cull) launch_raycast_t<T, true, true>(lm, pm, origin, rays, n, depth, s);
    else launch_raycast_t<T, false, true>(lm, pm, origin, rays, n, depth, s);
  } else {
    if (cull) launch_raycast_t<T, true, false>(lm, pm, origin, rays, n, depth, s);
    else launch_raycast_t<T, false, false>(lm, pm, origin, rays, n, depth, s);
  }
}

hipError_t launch_raycast(int precision, bool cull, const LocalModel& lm, const PosedModel& pm, const double* origin,
                          const double* d_rays, int64_t n, double* d_depth, hipStream_t s) {
  if (n <= 0) return hipSuccess;
#if FSDF_BENCH_ONLY
  return hipErrorNotSupported;
#else
  if (precision == 64) launch_raycast_p<double>(cull, lm, pm, origin, d_rays, n, d_depth, s);
  else launch_raycast_p<float>(cull, lm, pm, origin, d_rays, n, d_depth, s);
#endif
  return hipGetLastError();
}

hipError_t launch_reduce(const double* partials, int nblocks, int len, double* d_accum, hipStream_t s,
                         const uint32_t* cost, int32_t* order, hipEvent_t ev_stop, const int* skip) {
  if (ev_stop)
    hipExtLaunchKernelGGL(reduce_tiles_kernel, dim3((len + 7) / 8), dim3(kTileBlock), 0u, s, nullptr, ev_stop, 0u,
                          partials, nblocks, len, d_accum, skip);
  else
    hipLaunchKernelGGL(reduce_tiles_kernel, dim3((len + 7) / 8), dim3(kTileBlock), 0, s, partials, nblocks, len,
                       d_accum, skip);
  if (cost) hipLaunchKernelGGL(order_kernel, dim3(1), dim3(kBlock), 0, s, cost, nblocks, order);
  return hipGetLastError();
}

// the planned pass's LDS: the hull-partitioned layout + 4 chunk start times
static size_t planned_lds_bytes(const LocalModel& lm) { return hpart_lds_bytes(lm, 1) + 4 * sizeof(uint64_t); }

bool planned_pass(const LocalModel& lm, int64_t n) {
  return lm.planes64 && lm.S <= 64 && lm.R == 0 && n > 0 && (n + 63) / 64 <= kMaxPlanChunks &&
         planned_lds_bytes(lm) <= (size_t)kLdsPerCu / 4;
}

template <typename T>
static void launch_planned_t(bool cull, const LocalModel& lm, const PosedModel& pm, const void* d_pts, int64_t n,
                             int grid, const PassOutputs& out, const ChunkOutputs& co, hipStream_t s) {
  const PassModel<T> m = pass_model<T>(lm, pm);
  auto b = [](bool v) { return v ? "true" : "false"; };
  snprintf(g_pass_name, sizeof g_pass_name, "planned_pass_kernel<%s, %s>", type_name<T>(), b(cull));
  if (cull)
    launch_lds(planned_pass_kernel<T, true>, grid, kPassBlock, planned_lds_bytes(lm), s, (const T*)d_pts, n, m, out,
               co);
  else
    launch_lds(planned_pass_kernel<T, false>, grid, kPassBlock, planned_lds_bytes(lm), s, (const T*)d_pts, n, m, out,
               co);
}

hipError_t launch_planned_pass(int precision, bool cull, const LocalModel& lm, const PosedModel& pm, const void* d_pts,
                               int64_t n, int grid, const PassOutputs& out, const ChunkOutputs& co, hipStream_t s,
                               hipEvent_t ev_start, hipEvent_t ev_stop) {
  struct ClearEvents {
    ~ClearEvents() { g_pass_ev0 = g_pass_ev1 = nullptr; }
  } clear_events;
  g_pass_name[0] = 0;
  if (precision != 64) return hipErrorNotSupported;  // (planes64: f64 contexts only)
  g_pass_ev0 = ev_start;
  g_pass_ev1 = ev_stop;
  launch_planned_t<double>(cull, lm, pm, d_pts, n, grid, out, co, s);
  return hipGetLastError();
}

hipError_t launch_reduce_chunks(const ChunkOutputs& co, int64_t nc, int S, double* partials, double* d_accum,
                                hipStream_t s, hipEvent_t ev_stop, const int* skip) {
  const int len = 1 + 6 * S;
  const int ngroups = (int)reduce_chunk_groups(nc);
  const size_t lds = (size_t)kGroupChunks * len * sizeof(double) + kGroupChunks * sizeof(I4);
  hipLaunchKernelGGL(chunk_groups_kernel, dim3(ngroups), dim3(kGroupBlock), lds, s, (const I4*)co.hdr, co.ent, co.csum,
                     co.dense, (int)nc, S, partials, ngroups, skip);
  return launch_reduce(partials, ngroups, len, d_accum, s, nullptr, nullptr, ev_stop, skip);
}

int64_t reduce_chunk_groups(int64_t nc) { return (nc + kGroupChunks - 1) / kGroupChunks; }

hipError_t launch_plan(const uint32_t* dur, int64_t nc, int n4, int n2, int32_t* order, int32_t* plan, hipStream_t s) {
  hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(kPlanBlock), 0, s, dur, (int)nc, n4, n2, order, (I4*)plan);
  return hipGetLastError();
}

hipError_t launch_chunk_spheres(int precision, const void* d_pts, int64_t n, int64_t nchunks, float* d_out,
                                hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const unsigned grid = (unsigned)((64 * nchunks + kBlock - 1) / kBlock);
  if (precision == 64)
    hipLaunchKernelGGL(chunk_sphere_kernel<double>, dim3(grid), dim3(kBlock), 0, s, (const double*)d_pts, n, nchunks,
                       (F4*)d_out);
  else
    hipLaunchKernelGGL(chunk_sphere_kernel<float>, dim3(grid), dim3(kBlock), 0, s, (const float*)d_pts, n, nchunks,
                       (F4*)d_out);
  return hipGetLastError();
}

hipError_t launch_to_f32(const double* src, float* dst, int64_t count, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  const int64_t grid = (count + kBlock - 1) / kBlock;
  hipLaunchKernelGGL(to_f32_kernel, dim3((unsigned)grid), dim3(kBlock), 0, s, src, dst, count);
  return hipGetLastError();
}

}  // namespace fsdf
