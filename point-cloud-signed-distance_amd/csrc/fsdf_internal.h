// Internal declarations shared by the kernel translation unit and the C-ABI.
// Device layouts (all per-evaluation "world" arrays are produced on the device
// by the pose kernel from the resident local model and the K poses):
//
//   local model (uploaded once by fsdf_set_model)
//     verts_l   [V][3]  f64     hull vertices, body frame
//     faces     [F][3]  i32     global vertex indices (CCW from outside)
//     planes_l  [F][4]  f64     (n, d), n·x <= d inside
//     face_hull [F]     i32     owning hull of each face
//     sphere_l  [K][4]  f64     vertex centroid (inside the hull) + radius
//     box_l     [K][8]  f64     body-frame bounding box: centre xyz, 0, half extents xyz
//                               (rounded up to f32), 0
//     face_off  [K+1]   i32     faces of hull k are [face_off[k], face_off[k+1])
//     vert_hull [V]     i32     owning hull of each vertex
//     vert_off  [K+1]   i32     vertices of hull k are [vert_off[k], vert_off[k+1])
//     face_rows [F][4]  i32     packed hull-local (v0|v1<<16, v2|n0<<16, n1|n2<<16, dup):
//                               vertex indices, the face across edge i (v_i -> v_{i+1}),
//                               dup = 1 if an earlier face of the hull has the same plane
//
//   posed model (rewritten by every evaluation; T = double or float)
//     planes_w  [F][4]  T       world plane
//     hull_rows [K+1]   96 B    the hull table (pose_impl.h HullRow): world centroid + radius
//                               and the world oriented box — (centre, 0), 3 x (body axis i,
//                               half extent i) — as f32 culling bounds, face_off[k], vert_off[k],
//                               the certificate scale max_v |v|_1 over the hull's world vertices
//                               (f64); row K: the offsets' ends and the culling-margin scale
//     verts_w   [V][4]  T       world vertices (support/optimality certificate)
//     screen_w  [F+K][4] f32    fp32 screening planes, hull-centred, in face pairs:
//                               hull k's pair j at slots face_off[k]+k+2j (32 B):
//                               (nx_a nx_b ny_a ny_b nz_a nz_b -d'_a -d'_b), a = 2j,
//                               b = 2j+1 (= a when nf is odd and j is the last pair),
//                               d' = d - n·c with c the hull's f32 sphere centre
//
//   per-block partial sums  partials [len/8][nblocks][8] f64 line tiles, len = 1+6S+Σ(4n+4)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_buffers.h"

// Every -DFSDF_... build switch of the library, with its default: four
// diagnostics (0 / 1), then the tunables. `make dev EXTRA=-D...` sets them
// (Makefile, tools/); the shipped library is the defaults. Test them with #if.
#ifndef FSDF_WAVE_TIMES
#define FSDF_WAVE_TIMES 0    // per-wave timeline with per-phase clocks in fsdf_kernel_stats (tools/wave_times.py)
#endif
#ifndef FSDF_HOST_TIMES
#define FSDF_HOST_TIMES 0    // host clocks of the solver loops, printed by fsdf_descend (tools/host_gap_probe.py)
#endif
#ifndef FSDF_SOLVER_TIMES
#define FSDF_SOLVER_TIMES 0  // per-phase clocks of the device solver step, printed by fsdf_descend
#endif
#ifndef FSDF_BENCH_ONLY
#define FSDF_BENCH_ONLY 0    // instantiate only the bench variant of the pass kernel (make dev sets it)
#endif
#ifndef FSDF_PLANE_BATCH
#define FSDF_PLANE_BATCH 8   // plane rows per LDS batch of the plane max (power of 2, >= 2)
#endif
#ifndef FSDF_SCREEN_ILP
#define FSDF_SCREEN_ILP 4    // independent 8-face batches per iteration of the fp32 screen
#endif
#ifndef FSDF_PASS_WAVES_PER_SIMD
#define FSDF_PASS_WAVES_PER_SIMD 4  // the pass kernels' occupancy target (VGPR budget 512 / w)
#endif
#ifndef FSDF_ORDER_EVERY
#define FSDF_ORDER_EVERY 16  // passes between rebuilds of the block order / the plan
#endif
#ifndef FSDF_SKIN_MOMENTS_FMA
#define FSDF_SKIN_MOMENTS_FMA 0  // skin_moments.hip: JᵀJ by v_fma_f64 inner products instead of the fp64 MFMA (A/B)
#endif
#ifndef FSDF_MAX_BLOCKS
#define FSDF_MAX_BLOCKS 16384  // pass grid cap (grid-stride beyond)
#endif

namespace fsdf {

// one-chunk-per-wave passes (pass_kernel ALIAS) keep the wrench rows in the
// wave's stage: the stage is then at least the rows + the gradient transpose
constexpr int kRedInStageMinBytes = (64 * 6 + 2) * 8 + 64 * 3 * 8;

constexpr int kBlock = 256;
constexpr int kPassBlock = 256;    // pass-kernel workgroup: 4 waves of 64
constexpr int kHullRowBytes = 96;  // a row of the posed hull table (pose_impl.h HullRow)
constexpr int kLdsPerCu = 163840;  // gfx950 LDS per CU
constexpr int kMaxLds = 163840;    // LDS a workgroup may declare (gfx950)
constexpr int kMaxHulls = 256;     // 4 accumulator slots per lane
constexpr int kMaxBlocks = FSDF_MAX_BLOCKS;  // pass grid cap (grid-stride beyond)
constexpr int kMaxRbfAccum = 512;  // Σ (4n+4) over RBF skins (= kMaxRbfAcc in the kernel)

struct LocalModel {
  int K = 0, F = 0, V = 0;   // K = convex hulls
  int S = 0, R = 0;          // surfaces (k* index space), RBF skins
  int rbf_rows = 0;          // Σ (n_centres + 1)
  int rbf_acc = 0;           // Σ (4 n_centres + 4)
  const int32_t* hull_surface = nullptr;  // [K]
  const int32_t* surface_kind = nullptr;  // [S]
  const int32_t* rbf_surface = nullptr;   // [R]
  const int32_t* rbf_row_off = nullptr;   // [R+1]
  const int32_t* rbf_acc_off = nullptr;   // [R+1]
  const double* verts_l = nullptr;
  const int32_t* faces = nullptr;
  const double* planes_l = nullptr;
  const int32_t* face_hull = nullptr;
  const double* sphere_l = nullptr;
  const double* box_l = nullptr;       // [K][8]
  const int32_t* face_off = nullptr;
  const int32_t* vert_hull = nullptr;
  const int32_t* vert_off = nullptr;
  const int32_t* face_rows = nullptr;  // [F][4]
  // per pose item (faces, then vertices) [F+V][4]: surface | nf << 16, hull,
  // face_off[hull], vert_off[hull] — one 16-B load instead of a chain of them
  const int32_t* item_meta = nullptr;
  int stage_bytes = 0;                 // per-wave LDS stage, context precision (multiple of 16)
  int planes64 = 0;                    // f64: stage the fp64 planes too (if they fit: fsdf_set_surfaces)
  // hull-partitioned pass tiers (pass_kernel HPART, hpart_parts): clouds of
  // up to hpart4_points run 4 waves per chunk, up to hpart2_points 2; -1 =
  // the model's default (hpart_default_limits), 0 = tier off (fsdf_set_partition)
  int64_t hpart4_points = -1, hpart2_points = -1;
};

// the model-dependent defaults of the two tiers (sdf_kernels.hip)
void hpart_default_limits(const LocalModel& lm, int64_t* four, int64_t* two);
// waves per chunk a pass over n points runs (4, 2; 0 = one wave per chunk)
int hpart_parts(const LocalModel& lm, int64_t n);
// the pass-kernel variant the last launch_pass on this thread dispatched
// ("pass_kernel<T, SLOTS, CULL, RBF, ALIAS, HPART, NB, NPART>", as rocprofv3
// prints it without the namespace); "" before any
const char* last_pass_kernel();

struct PosedModel {
  void* planes_w = nullptr;   // T
  void* hull_rows = nullptr;  // [K+1] HullRow (pose_impl.h)
  void* verts_w = nullptr;    // T
  float* screen_w = nullptr;  // [F+K][4] (f64 contexts; see the layout above)
  // f64 planes64 contexts: every hull's LDS stage image, [4F + K + 2V] 16-B
  // chunks; hull k at chunk 4·face_off[k] + k + 2·vert_off[k]: its screening
  // pairs (nf + 1 chunks, as in screen_w), fp64 planes (2 per face), fp64
  // vertex rows (2 per vertex), face rows (1 per face; static, written at
  // set_model). One contiguous copy stages a hull.
  void* image_w = nullptr;
  void* rbf_rows = nullptr;   // T [rbf_rows][4], per pass (fsdf_set_rbf_params)
};

struct PassOutputs {
  double* partials = nullptr;  // line tiles (pass_kernels.h pidx)
  int32_t* kstar = nullptr;    // optional, caller order
  double* d = nullptr;         // optional
  double* grad = nullptr;      // optional [n][3]
  const int32_t* perm = nullptr;  // optional: resident index -> caller index
  unsigned long long* stats = nullptr;  // optional kernel counters (fsdf_debug_stats)
  // optional cost-ordered schedule (resident-cloud passes): launch slot b runs
  // logical block order[b] (a permutation of [0, nblocks)); every logical block
  // writes its duration (100 MHz ticks) to cost[block]. Partial sums stay in
  // logical-block columns, so results do not depend on the order.
  const int32_t* order = nullptr;
  uint32_t* cost = nullptr;
  // optional [n64/64][4] f32 bounding sphere of each 64-point chunk of the
  // resident cloud (launch_chunk_spheres at set_points; pose-independent)
  const float* chunk_ws = nullptr;
  // optional [n] nearest surface of each resident point in the previous pass
  // over this cloud (hull-only scenes of <= 64 surfaces): read as the point's
  // best-first seed (a heuristic — any seed gives the same bits), rewritten by
  // this pass. prior_in is null on a cloud's first pass.
  const uint8_t* prior_in = nullptr;
  uint8_t* prior_out = nullptr;
  // optional device flag: set, the launch returns at once (the passes a
  // converged device solver loop still has queued, solver.hip)
  const int* skip = nullptr;
};

// Planned pass (pass_kernels.h planned_pass_kernel): per-chunk partial rows
// of a resident cloud (nc = ceil(n/64) chunks) and the workgroup plan.
struct ChunkOutputs {
  int32_t* hdr = nullptr;      // [nc][4] surfaces of entries 0..3 (-1: none); [c][0] == -2: dense row
  double* ent = nullptr;       // [nc][4][6] (F, M) of each entry
  double* csum = nullptr;      // [nc] Σ d² over the chunk's points
  double* dense = nullptr;     // [nc][S][6] (F, M) per surface (chunks with > 4 surfaces)
  uint32_t* dur = nullptr;     // [nc] serial-equivalent chunk durations (100 MHz ticks)
  const int32_t* plan = nullptr;  // [grid][4] workgroup plan (chunk | parts << 24, chunk, chunk, chunk), or null
  int dparts = 1;              // waves per chunk without a plan (4, 2 or 1)
  // a split chunk's wall time x (num / den) is its serial-equivalent duration
  // (the speed-up of the 4- / 2-wave split; set per model by the context:
  // pass.hip run_planned, tools/split_speedup.py)
  int r4n = 5, r4d = 2, r2n = 8, r2d = 5;
  int64_t cap = 0;             // chunks allocated: csum = ent + 24 cap, dense = ent + 25 cap (one allocation
                               // of (25 + 6 S) doubles per chunk: 1.6 KB per chunk at S = 64, i.e. 13 MB at
                               // the default 524,288-point planned window, 105 MB at kMaxPlanChunks)
};
constexpr int kPlanPartsShift = 24;
constexpr int64_t kMaxPlanChunks = 1 << 16;  // planned passes: clouds of <= 4,194,304 points per device

// a resident pass over n points of this model can run planned
bool planned_pass(const LocalModel& lm, int64_t n);
// the cloud sizes the planned pass runs by default (fsdf_set_plan max_points
// -1): min < n <= max
int64_t planned_default_max_points(const LocalModel& lm);
int64_t planned_default_min_points();
hipError_t launch_planned_pass(int precision, bool cull, const LocalModel& lm, const PosedModel& pm, const void* d_pts,
                               int64_t n, int grid, const PassOutputs& out, const ChunkOutputs& co, hipStream_t s,
                               hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// the accumulator d_accum [1 + 6S] from the chunk rows, in chunk order: 16-chunk
// group rows into `partials` (reduce_chunk_groups(nc) rows, line-tiled), then
// the unplanned pass's tile reduce over them
int64_t reduce_chunk_groups(int64_t nc);
hipError_t launch_reduce_chunks(const ChunkOutputs& co, int64_t nc, int S, double* partials, double* d_accum,
                                hipStream_t s, hipEvent_t ev_stop = nullptr, const int* skip = nullptr);
// the plan of the next passes from the chunk durations of this one
hipError_t launch_plan(const uint32_t* dur, int64_t nc, int n4, int n2, int32_t* order, int32_t* plan, hipStream_t s);

// Surfaces whose poses ride in the pose kernel's arguments (12·64 doubles =
// 6 KiB of kernarg; larger scenes upload them with a copy).
constexpr int kPoseArgMax = 64;
struct PoseArgs {
  double v[12 * kPoseArgMax];
};

// precision: 64 or 32. Points are AoS of the matching precision. h_poses (host,
// S <= kPoseArgMax) are passed by value in the launch; otherwise d_poses is read.
hipError_t launch_pose(int precision, const LocalModel& lm, const double* d_poses,
                       const PosedModel& pm, hipStream_t s, const double* h_poses = nullptr,
                       const int* skip = nullptr);

// ev_start / ev_stop (optional): timing events stamped by the pass kernel's
// dispatch itself (hipExtLaunchKernel), not by packets of their own
hipError_t launch_pass(int precision, bool cull, const LocalModel& lm, const PosedModel& pm,
                       const void* d_pts, int64_t n, int nblocks, const PassOutputs& out,
                       hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);

// origin: 3 host doubles (passed by value); d_rays [n][3] f64 unit directions.
hipError_t launch_raycast(int precision, bool cull, const LocalModel& lm, const PosedModel& pm, const double* origin,
                          const double* d_rays, int64_t n, double* d_depth, hipStream_t s);

// With cost/order: one extra workgroup also rebuilds order[] (heaviest logical
// blocks first) from this pass's costs, for the next pass of the same grid.
constexpr int kTileBlock = 1024;  // the tile reduce's workgroup (reduce_kernels.h reduce_tiles_kernel)
hipError_t launch_reduce(const double* partials, int nblocks, int len, double* d_accum,
                         hipStream_t s, const uint32_t* cost = nullptr, int32_t* order = nullptr,
                         hipEvent_t ev_stop = nullptr, const int* skip = nullptr);

// ---- second moments of the residual (moments.hip) -----------------------------
// Per surface k the 21 upper-triangle entries (row-major) of Σ w wᵀ over the
// resident points with k* = k, w = (∇d*, p × ∇d*), from the per-point k* and
// ∇d* a pass wrote in RESIDENT order. Workgroup g sums the chunks
// [g · run, (g + 1) · run), every wave a contiguous share of them into an
// [S][21] table of its own in LDS, and writes the waves' tables, summed in
// wave order, as one partial (line tiles, as the pass's); launch_reduce sums
// the partials in workgroup order. run = moments_run(n): at least
// kMomentsMinChunks, and as many as keep the grid at kMomentsMaxGroups
// workgroups (two per CU: 5.5 MB of partials for 64 surfaces) — a function of
// n alone; moments_waves(S) waves per workgroup, as many of 4, 2, 1 as have
// room for their tables in kMomentsMaxLds (4 up to 97 surfaces, 2 up to 195, 1
// up to 390).
constexpr int kMomentsLen = 21;          // entries per surface
constexpr int kMomentsBlock = 256;       // 4 waves at most
constexpr int kMomentsMinChunks = 8;     // a workgroup's run of 64-point chunks, at least (a multiple of 4)
constexpr int kMomentsMaxGroups = 512;   // workgroups, at most
constexpr int kMomentsMaxLds = 65536;    // the workgroup's tables
int moments_waves(int S);  // 0: not even one table fits
int64_t moments_run(int64_t n);
int moments_groups(int64_t n);
bool moments_fit(int S);  // the scene's table fits kMomentsMaxLds
// doubles of d_partials for a cloud of n points (>= one workgroup's)
size_t moments_partials_len(int64_t n, int S);
// n > 0, moments_fit(S). d_pts: the resident cloud (precision 64 / 32; all
// arithmetic fp64); d_moments [S][21]. A k* outside [0, S) contributes nothing.
// skip (optional): a device flag; set, both launches return at once (the
// evaluations a finished device LM frame still has queued, lm_solver.hip)
hipError_t launch_moments(int precision, const void* d_pts, const int32_t* d_kstar, const double* d_grad, int64_t n,
                          int S, double* d_partials, double* d_moments, hipStream_t s, const int* skip = nullptr);

// ---- robust point losses (robust.hip; the loss: robust_impl.h) -------------------
// Per surface k one row of kRobustLen doubles over the resident points with
// k* = k, w = w(d*), v = (∇d*, p × ∇d*): [0..20] Σ w v vᵀ (the moments' order),
// [21..26] Σ 2 w d* v (the accumulator's wrench), [27] Σ ρ(d*), [28] Σ w. From
// the per-point k*, d*, ∇d* a pass wrote in RESIDENT order. The grid, the runs
// and the reduce are the moments': run = robust_run(n) chunks per workgroup
// (at least kRobustMinChunks, at most kRobustMaxGroups workgroups: a function
// of n alone), robust_waves(S) waves per workgroup, as many of 4, 2, 1 as have
// room for their [S][29] tables in kRobustMaxLds (4 up to 70 surfaces, 2 up to
// 141, 1 up to 282). moments = false keeps the last kRobustTail entries of
// every row alone (rows of 8: wrench, Σρ, Σw), summed in the same order.
constexpr int kRobustLen = 29;           // entries per surface
constexpr int kRobustTail = 8;           // ... of which the wrench, Σρ and Σw
constexpr int kRobustBlock = 256;        // 4 waves at most
constexpr int kRobustMinChunks = 8;      // a workgroup's run of 64-point chunks, at least (a multiple of 4)
constexpr int kRobustMaxGroups = 512;    // workgroups, at most
constexpr int kRobustMaxLds = 65536;     // the workgroup's tables
int robust_waves(int S);  // 0: not even one table fits
int64_t robust_run(int64_t n);
int robust_groups(int64_t n);
bool robust_fit(int S);
// doubles of d_partials for a cloud of n points (>= one workgroup's; sized for the rows of 29)
size_t robust_partials_len(int64_t n, int S);
// n > 0, robust_fit(S), a valid loss (kind, scale: robust_impl.h). d_pts: the
// resident cloud (precision 64 / 32; all arithmetic fp64); d_rows [S][29]
// (moments) or [S][8]. A k* outside [0, S) contributes nothing. d_conf: null, or
// [n] per-point confidence weights in resident order (fp64 in either precision):
// the WEIGHTED instantiations, aw = a · w in place of w and a · ρ in place of ρ.
// n_surface >= 0: the ONE_SIDED instantiations — resident point i is a
// free-space sample iff (d_perm ? d_perm[i] : i) >= n_surface (d_perm: null, or
// the cloud's resident→caller permutation [n]) and then counts only where
// d* < 0 (robust_impl.h one_sided_factor); n_surface < 0: no split, d_perm unread.
// skip (optional): a device flag, as launch_moments'; set, both launches return
// at once (the evaluations a finished device frame still has queued). It is
// written only by a step kernel launched earlier on the same stream.
hipError_t launch_robust(int precision, bool moments, const void* d_pts, const int32_t* d_kstar, const double* d_d,
                         const double* d_grad, const double* d_conf, const int32_t* d_perm, int64_t n_surface,
                         int64_t n, int S, int kind, double scale, double* d_partials, double* d_rows,
                         hipStream_t s, const int* skip = nullptr);
// robust_rows_finish (pass.hip) on the device: from d_rows [S][29] (moments) or
// [S][8] the accumulator d_accum [1 + 6S] — [0] Σρ summed over the surfaces in
// ascending order from 0.0 by one thread, then every hull surface's wrench, 0.0
// for a surface that is no hull — and, moments, d_moments [S][21] (a hull's row
// copied, any other's 0.0): the host's bits. d_surface_kind [S]: the model's
// (LocalModel::surface_kind). Any S >= 1; one launch; skip as launch_robust's.
constexpr int kRobustAssembleBlock = 128;  // (two tiles of Σρ at the library's 256 surfaces)
hipError_t launch_robust_assemble(bool moments, const double* d_rows, const int32_t* d_surface_kind, int S,
                                  double* d_accum, double* d_moments, hipStream_t s, const int* skip = nullptr);
// ---- the RBF skins' blocks under a robust objective (robust_skin.hip) -----------
// d_blocks [lm.rbf_acc]: per skin r its block of the accumulator, Σ t j(p) over
// the resident points with k* = r's surface — rbf_adjoint's sums with the
// point's t = 2 (aw d*) (robust_impl.h wrench_scale, fp64, from the pass's d* in
// resident order) where the pass has 2s. The grid and the runs are
// launch_robust's (robust_groups, robust_run: functions of n alone), four waves
// per workgroup; d_conf, d_perm, n_surface as launch_robust's. d_rows: the RBF
// rows of the context precision (PosedModel::rbf_rows). n > 0, lm.R >= 1.
size_t robust_skin_partials_len(int64_t n, int rbf_acc);  // doubles of d_partials
hipError_t launch_robust_skin(int precision, const void* d_pts, const int32_t* d_kstar, const double* d_d,
                              const void* d_rows, const LocalModel& lm, const double* d_conf, const int32_t* d_perm,
                              int64_t n_surface, int64_t n, int kind, double scale, double* d_partials,
                              double* d_blocks, hipStream_t s);
// ---- scoring candidate states (score.hip) -----------------------------------------
// B candidates' posed models side by side: candidate b's table lies b · stride
// bytes into the buffer — world planes [F][4] T, world vertices [V][4] T, the
// hull table [K+1] HullRow and (f64) the fp32 screening pairs [F+K][4], each at
// its byte offset (multiples of 256). score_table is a function of (precision,
// model) alone.
struct ScoreTable {
  size_t stride = 0, planes = 0, verts = 0, rows = 0, screen = 0;
};
ScoreTable score_table(int precision, const LocalModel& lm);
constexpr int kScoreBlock = 256;      // 4 waves, a 64-point chunk each per round
constexpr int kScoreMaxGroups = 512;  // workgroups per candidate, at most (grid-stride beyond)
// workgroups per candidate for a cloud of n points: a function of n alone
int score_groups(int64_t n);
// hull-only scenes of up to kMaxHulls hulls whose table and stages fit a workgroup's LDS
bool score_fits(const LocalModel& lm);
// d_poses [B][S][12] -> d_tables [B] tables (pose_impl.h pose_item per candidate); B <= 65535
hipError_t launch_score_pose(int precision, const LocalModel& lm, const double* d_poses, int B, void* d_tables,
                             hipStream_t s);
// d_cost[b] = Σ_i a_i ρ(d*_b(p_i)) over the resident cloud d_pts (context
// precision; terms and sums fp64) against table b: n > 0, score_fits(lm), a
// valid loss. d_chunk_ws: null, or the resident chunk spheres; d_conf, d_perm,
// n_surface as launch_robust's. d_partials [B][score_groups(n)]. Two launches.
hipError_t launch_score(int precision, bool cull, const LocalModel& lm, const void* d_tables, const void* d_pts,
                        int64_t n, int B, const float* d_chunk_ws, const double* d_conf, const int32_t* d_perm,
                        int64_t n_surface, int kind, double scale, double* d_partials, double* d_cost,
                        hipStream_t s);
// ---- gradients and moments of many candidate states (batch.hip) ------------------
// The rows launch_robust reduces, for nb candidates at once: candidate b's posed
// table is table b of launch_score_pose's buffer. Two launches and a reduce.
// launch_batch_eval, grid (score_groups(n), nb): scene_eval of every resident
// point against table b, its k*, d* and ∇d* — what a pass writes in resident
// order, the same bits — into candidate b's block of d_points, kBatchPointBytes ·
// np bytes each: k* [np] i32 | d* [np] f64 | ∇d* [np][3] f64, np =
// batch_point_stride(n) (n rounded up to whole 64-point chunks).
// launch_batch_robust, grid (robust_groups(n), nb) then (tiles, nb):
// robust_kernel's and the tile reduce's statements per candidate (robust_body.inc,
// reduce_tiles_body.inc) over candidate b's arrays, into d_partials
// [nb][robust_partials_len(n, S)] and d_rows [nb][S · (moments ? 29 : 8)] — the
// bits launch_robust gives from the same per-point arrays. n > 0, nb <= 65535,
// score_fits(lm), robust_fit(S), a valid loss; d_conf, d_perm, n_surface as
// launch_robust's (the resident cloud's: the same for every candidate).
inline size_t batch_point_stride(int64_t n) { return (size_t)((n + 63) & ~(int64_t)63); }
constexpr size_t kBatchPointBytes = 36;
hipError_t launch_batch_eval(int precision, bool cull, const LocalModel& lm, const void* d_tables, const void* d_pts,
                             int64_t n, int nb, const float* d_chunk_ws, void* d_points, hipStream_t s);
hipError_t launch_batch_robust(int precision, bool moments, const void* d_pts, const void* d_points,
                               const double* d_conf, const int32_t* d_perm, int64_t n_surface,
                               int64_t n, int S, int nb, int kind, double scale, double* d_partials, double* d_rows,
                               hipStream_t s);
// res[i] = src[perm[i]] over n doubles (point_weights.hip: a per-point side array
// into resident order; an index outside [0, n) reads as 0)
hipError_t launch_gather_f64(const double* d_src, const int32_t* d_perm, int64_t n, double* d_res, hipStream_t s);

// ---- depth-frame ingest (depth.hip) --------------------------------------------
// A depth image of npix pixels (format FSDF_DEPTH_F64 / _F32 / _U16, device
// memory) over the pixel directions d_u [npix][3] becomes the fp64 cloud of its
// valid pixels in pixel order: s = scale · depth, valid iff finite, > 0 and in
// [near, far]; p = R (s u) + t. launch_depth_count: the count per 256-pixel
// block and their exclusive scan in place (d_counts [ceil(npix/256)]), the
// total to *d_total — two launches. launch_depth_scatter, sized by that total:
// d_xyz [total][3] and d_pix [total] (each point's pixel) — one launch.
struct DepthRange {
  double near, far, scale;
};
struct DepthPose {
  double R[9], t[3];
};
// Free-space samples (fsdf_set_free_space; `free` null: none, the launches and
// buffers above): a pixel on the stride grid with free length L (s − gap of a
// valid pixel; miss_range of a miss when that is > 0) and
// L − (samples − 1) · spacing > 0 sends `samples` points at ranges
// t = L − (j − 1) · spacing along its direction, after the valid pixels' points:
// sample j of the r-th sending pixel at n_surface + (j − 1) · m + r. The count
// then fills d_counts [2][blocks] (valid, sending), the scan runs one workgroup
// per row and writes d_total [2]; the scatter, given both totals, writes
// d_xyz / d_pix [n_surface + samples · m].
struct DepthFree {
  int32_t samples, stride, cols;
  double gap, spacing, miss_range;
};
size_t depth_format_bytes(int format);
hipError_t launch_depth_count(int format, const void* d_depth, int64_t npix, const DepthRange& r,
                              const DepthFree* free, int32_t* d_counts, int64_t* d_total, hipStream_t s);
hipError_t launch_depth_scatter(int format, const void* d_depth, const double* d_u, int64_t npix, const DepthRange& r,
                                const DepthPose& P, const DepthFree* free, int64_t n_surface, int64_t m,
                                const int32_t* d_offsets, double* d_xyz, int32_t* d_pix, hipStream_t s);
// the ingest's scan on its own (voxel.hip's head-flag counts take it too):
// d_counts [rows][nblocks], each row's exclusive prefix in place and its total
// to d_total [rows] — one workgroup per row, int32 sums (a row sums to < 2^31)
hipError_t launch_block_scan(int32_t* d_counts, int rows, int32_t nblocks, int64_t* d_total, hipStream_t s);

// ---- voxel-grid downsampling (voxel.hip) ------------------------------------------
// The grid of fsdf_set_voxel_grid: cell size h (finite, > 0) and origin o; a
// point's cell per axis is floor((x − o) / h) clamped to [−2^20, 2^20 − 1].
struct VoxelGrid {
  double size, origin[3];
};

// ---- second moments of RBF skins (skin_moments.hip) ----------------------------
// Per skin r of n centres, m = 4n + 4: M_r [m][m] = Σ_{p: k*(p) = r's surface}
// j(p) j(p)ᵀ, j the point's row in the layout of the skin's accumulator block
// (include/flashsdf.h "Gauss-Newton for RBF skins"), full, row-major, exactly
// symmetric; the skins' matrices one after the other in surface order. From
// the resident points, the pass's k* in RESIDENT order and the context's
// current RBF rows; all arithmetic fp64 (fp32 points and rows are widened).
// A unit is one 64x64 block pair (bi <= bj) of one skin; workgroup
// (unit, g) sums the chunks [g · run, (g + 1) · run) into its block on the
// fp64 matrix unit and writes it as one partial of 4096 doubles (32 KB); the
// finish launch sums a unit's partials in workgroup order and mirrors the
// block. run = skin_moments_run(n, U): at least kSkinMinChunks, and as many
// as keep U · groups <= kSkinMaxPartials — the partials take at most
// kSkinMaxPartials · 32 KB = 32 MB per context, a function of (n, the skins'
// centre counts) alone, as the grid is.
constexpr int kSkinMaxCentres = 124;     // n + 4 <= 128, the device solver's own limit
constexpr int kSkinMaxUnits = 64;        // Σ (4n + 4) <= kMaxRbfAccum: at most 64 skins, at most 64 block pairs
constexpr int kSkinBlock = 256;          // 4 waves: a 16x64 strip of the block each
constexpr int kSkinTile = 64;            // side of a unit's output block
constexpr int kSkinMinChunks = 8;        // a workgroup's run of 64-point chunks, at least (a multiple of 4)
constexpr int kSkinMaxPartials = 1024;   // partial blocks, at most (one workgroup's run is the whole cloud beyond)
struct SkinPlan {                        // (host side: a pair of launches per skin)
  int U = 0, R = 0;                      // units, skins
  int unit0[kSkinMaxUnits];              // skin r's units are [unit0[r], unit0[r + 1]): its pairs, bi-major
  int n[kSkinMaxUnits], row_off[kSkinMaxUnits], surf[kSkinMaxUnits], mom_off[kSkinMaxUnits];
  int total = 0;                         // Σ m_r²
};
// the plan of a surface list (kind [S], centres [S]); false: a skin of more
// than kSkinMaxCentres centres (or no skin at all)
bool skin_moments_plan(int S, const int32_t* kind, const int32_t* n_centers, SkinPlan* out);
int64_t skin_moments_run(int64_t n, int U);
int skin_moments_groups(int64_t n, int U);
size_t skin_moments_partials_len(int64_t n, int U);  // doubles of d_partials
// n > 0. d_rows: the RBF rows of the context precision (PosedModel::rbf_rows);
// d_moments [plan.total]. skip as launch_moments'.
hipError_t launch_skin_moments(int precision, const void* d_pts, const int32_t* d_kstar, const void* d_rows, int64_t n,
                               const SkinPlan& plan, double* d_partials, double* d_moments, hipStream_t s,
                               const int* skip = nullptr);
// the same with a factor per point, M_r = Σ aw j jᵀ (a robust objective's IRLS
// term): aw = a · w(d*) from d_d (the pass's d* in resident order), the loss,
// d_conf, d_perm and n_surface as launch_robust's, formed in fp64
hipError_t launch_skin_moments_weighted(int precision, const void* d_pts, const int32_t* d_kstar, const double* d_d,
                                        const void* d_rows, const double* d_conf, const int32_t* d_perm,
                                        int64_t n_surface, int kind, double scale, int64_t n, const SkinPlan& plan,
                                        double* d_partials, double* d_moments, hipStream_t s);

hipError_t launch_to_f32(const double* src, float* dst, int64_t count, hipStream_t s);

// per-chunk (64 points) bounding spheres of a resident cloud of the context
// precision -> d_out [ceil(n/64)][4] f32 (the pass kernel's wave culling input)
hipError_t launch_chunk_spheres(int precision, const void* d_pts, int64_t n, int64_t nchunks, float* d_out,
                                hipStream_t s);

int pass_blocks(int64_t n, const LocalModel& lm);
bool hpart_pass(const LocalModel& lm, int64_t n);

// dynamic LDS of one pass (raycast=false) / raycast workgroup for this model
size_t pass_lds_bytes(const LocalModel& lm, bool raycast, bool alias = false);

// Scratch of the per-frame spatial sort, owned by the context and grown only
// (a frame makes no allocation).
struct __attribute__((visibility("hidden"))) SortScratch {
  DevBuf<double> part;         // bbox partials [256][6] + the final box [6]
  DevBuf<uint32_t> k0;         // keys, double-buffered
  DevBuf<unsigned char> k1;    // (bytes: the alternate keys; regroup_points' priors)
  DevBuf<int32_t> i1;          // alternate index buffer
  DevBuf<unsigned char> tmp;   // rocPRIM temporary storage
  DevBuf<unsigned char> pts;   // (regroup_points) the cloud buffer the regrouped points go to
  DevBuf<uint64_t> q0, q1;     // (sort_points_keyed) composite keys, double-buffered
};

// Hilbert-order (sort.hip) the f64 AoS cloud d_src into d_dst (context
// precision) and write the permutation d_perm[resident i] = caller index
// (n < 2^31). Asynchronous on `st`.
hipError_t sort_points_spatial(const double* d_src, int64_t n, int precision, void* d_dst, int32_t* d_perm,
                              SortScratch& s, hipStream_t st);
// Regroup a resident cloud by each point's nearest surface in the last pass
// (prior[i] < 64), keeping the current (Hilbert) order within each group: a
// stable counting sort (sort.hip regroup_*_kernel, three launches). The
// regrouped points replace pts (it swaps with the scratch's buffer: read
// pts.get() anew); d_perm and prior are permuted in place. Asynchronous on `st`.
hipError_t regroup_points(DevBuf<unsigned char>& pts, int64_t n, int precision, int32_t* d_perm, uint8_t* prior,
                          SortScratch& s, hipStream_t st);
// ---- device solver iteration (solver.hip, solver_common.h) ------------------------------------
// The mechanism of a rigid scene as two device buffers built by the context
// from fsdf_set_mechanism (descend.hip build_solver_tree) — integers and doubles,
// each array at an offset — with the level schedules of the parallel FK and
// chain rule. The solver kernels copy both buffers into LDS first, so every
// later access in their level loops is an LDS access.
struct SolverTree {
  int nb = 0, nx = 0, S = 0;  // nx = nq + 3 n_deform: the whole state (x, g, divisors)
  int nq = 0;                 // joint coordinates (the deformations δ follow them in x)
  int D = 0;  // depth of the deepest body
  int H = 0;  // height levels of bodies with children: height_order[height_off[h] .. ) at height h+1
  int narrow = 0;  // every height level has <= 10 parents: the subtree sums run in one wave
  int chains = 0;  // every non-root body has <= 1 child: subtree sums along chain lists, no levels
  // one blob: the doubles [nd], then the ints [ni], padded to 16 B — copied into
  // LDS with one batch of 16-B loads per thread (one memory latency)
  const void* blob = nullptr;
  int ni = 0, nd = 0, chunks16 = 0;
  // offsets into the ints
  // path_list[path_off[b] .. path_off[b+1]): body b's ancestors from depth 1 down to b
  int parent = 0, kind = 0, qoff = 0, path_list = 0, path_off = 0, height_order = 0, height_off = 0;
  int child_off = 0, child_list = 0;  // [nb+1], children in descending index
  int surf_off = 0, surf_list = 0;    // [nb+1], surfaces in ascending index
  int surface_body = 0;               // [S]
  int chain_list = 0, chain_off = 0;  // (chains) [nb+1]: body b, its child, grandchild, ...
  // offsets into the doubles
  int axis = 0, AR = 0, At = 0, BR = 0, Bt = 0, frame_R = 0, frame_t = 0;  // frames: [S][9], [S][3]
  // RBF skins (fsdf_set_rbf_centres, in surface order) and deformations: R
  // skins of n_r centres (m_r = n_r + 4), rc = Σ n_r, rm = Σ m_r, rlu = Σ m_r²,
  // racc = Σ (4 n_r + 4) (the accumulator block after the 1 + 6S). Skin r's
  // centres start at rbf_coff[r], its m-vectors at rbf_coff[r] + 4r, its rows
  // at rbf_coff[r] + r, its accumulator block at 4 rbf_coff[r] + 4r, its LU at
  // rbf_luoff[r].
  int R = 0, n_deform = 0, rc = 0, rm = 0, rlu = 0, racc = 0;
  int rbf_n = 0, rbf_coff = 0, rbf_luoff = 0;  // ints [R], [R+1], [R+1]
  int rbf_body = 0, rbf_drow = 0;              // ints [rc]: the centre's body (-1: world) / deformation row (-1: none)
  int rbf_local = 0, rbf_values = 0;           // doubles [rc][3], [rc]
};
// One frame's solver state (device), two slots by iteration parity (a step
// launch's workgroups read slot (k & 1) while its workgroup 0 writes slot
// (k+1 & 1)): x [2][nx], the joint frames of the last FK Rb|tb [2][12 nb]
// (Rb [nb][9] then tb [nb][3] per slot); optional divisors [nx]; f = the last
// evaluation's cost / n_points; flags [3] = (done — the skip flag of the
// frame's launches —, iterations (x of the last one in slot iterations & 1),
// error: 1 FK / chain rule, 2 a non-finite pose, 3 a singular RBF system). (The next pass's posed
// model is written by the step itself: pose_impl.h.)
struct SolverState {
  double* x = nullptr;
  const double* div = nullptr;
  double *Rb = nullptr, *f = nullptr;
  int* flags = nullptr;
  // RBF / deformable scenes: what the next step's adjoint needs of this
  // step's FK and weight solve, two slots as x: rbf [2][9 nb + 3 rc + rm + rlu]
  // = the bodies' R | the centres | u | the LU factors (rows in pivoted
  // order, as the host's in-place factorization leaves them); prow [2][rm] the
  // row permutation (pivoted row i is row prow[i] of the system)
  double* rbf = nullptr;
  int32_t* prow = nullptr;
  double rate = 0.0, max_step = 0.0, tol = 0.0, n_points = 1.0, weight = 0.0;
  int limit = 0;
};
// descend_device's buffers. Device (doubles): x [2][nx] (slots by iteration
// parity) | div [nx] | Rb|tb [2][12 nb] | f | RBF scenes: the weight solve's
// state [2][9 nb + 3 rc + rm + rlu] and the row permutation [2][rm] ints; the
// flags are a buffer of their own. carve_solver_state fills st's pointers into
// d (null: none) and returns the doubles needed. Pinned (doubles): x [2][nx] |
// div [nx] | f | flags [4] (as 2 doubles): x (and the divisors) are uploaded
// from its start, and x [2][nx], f and the flags read back to their places.
inline size_t carve_solver_state(const SolverTree& T, bool divisors, double* d, SolverState* st) {
  const size_t nx = (size_t)T.nx, nb = (size_t)T.nb;
  const size_t rbf_slot = T.R > 0 ? 9 * nb + 3 * (size_t)T.rc + (size_t)T.rm + (size_t)T.rlu : 0;
  const size_t o_div = 2 * nx, o_Rb = 3 * nx, o_f = o_Rb + 24 * nb, o_rbf = o_f + 1, o_prow = o_rbf + 2 * rbf_slot;
  if (d) {
    st->x = d;
    st->div = divisors ? d + o_div : nullptr;
    st->Rb = d + o_Rb;
    st->f = d + o_f;
    if (T.R > 0) {
      st->rbf = d + o_rbf;
      st->prow = (int32_t*)(d + o_prow);
    }
  }
  return o_prow + (T.R > 0 ? (size_t)T.rm + 1 : 0);
}
struct SolverStaging {
  size_t div, f, flags;  // offsets in the pinned buffer (x at 0)
  size_t total, up;      // its doubles; the doubles uploaded from its start
};
inline SolverStaging solver_staging(int nx, bool divisors) {
  const size_t n = (size_t)nx;
  return SolverStaging{2 * n, 3 * n, 3 * n + 1, 3 * n + 3, (divisors ? 3 : 1) * n};
}
// the step's LDS (the tree, the accumulator and the work arrays, the kernels'
// static __shared__ included) fits one workgroup. nx = nq + 3 n_deform; ni, nd:
// the tree blob's ints and doubles; rbf_n [R]: the skins' centre counts
bool solver_fits(int nb, int nx, int S, int ni, int nd, int n_deform, int R, const int32_t* rbf_n);
// diagnostic builds (-DFSDF_SOLVER_TIMES=1): the last step's phase clocks (16, 100 MHz)
void solver_times(unsigned long long* out);
// FK of st.x -> Rb, tb and the first pass's posed model pm (flags zeroed by the
// caller; set on an error)
hipError_t launch_solver_init(const SolverTree& T, const SolverState& st, const LocalModel& lm,
                              const PosedModel& pm, int precision, hipStream_t s);
// one NaiveSolver iteration from the pass's accumulator, ending with the next
// pass's posed model pm (skips once flags[0] is set)
hipError_t launch_solver_step(const SolverTree& T, const SolverState& st, const double* d_accum,
                              const LocalModel& lm, const PosedModel& pm, int precision, int it_before,
                              hipStream_t s);

// ---- device Levenberg-Marquardt loop (lm_solver.hip) ------------------------------
// One frame's state of fsdf_descend_lm's device loop. The trial of evaluation k
// (0-based; the frame's start x is trial 0) lies in slot k & 1 of x [2][nq],
// its joint frames in slot k & 1 of Rb [2][12 nb] (as SolverState's); the
// accepted point — xa, f, g [nq], H [nq][nq] — and the damping lam are apart
// from them. flags [4] = (done: the skip flag of the frame's launches,
// evaluations counted, error: 1 FK / chain rule / motion rows, 2 a non-finite
// pose, unused). mu / x_ref [nq]: the prior's weights and reference
// (fsdf_set_lm_prior), mu null: no prior.
struct LmState {
  double *x = nullptr, *Rb = nullptr;
  double *xa = nullptr, *f = nullptr, *lam = nullptr, *g = nullptr, *H = nullptr;
  const double *mu = nullptr, *x_ref = nullptr;
  int* flags = nullptr;
  double max_step = 0.0, tol = 0.0, n_points = 1.0, weight = 0.0;
  int limit = 0;
};
// descend_lm_device's buffer, device and pinned alike (doubles): x [2][nq] |
// x_ref [nq] | mu [nq] | lam | flags [4] (as 2 doubles) | f | xa [nq] | g [nq] |
// H [nq][nq] | Rb|tb [2][12 nb]. carve_lm_state fills ls's pointers into d
// (null: none; mu only with a prior) and returns the spans: the first `up`
// doubles are uploaded (x_ref, mu, lam at these offsets), and `back` doubles
// from lam are read back in one copy — lam | flags (at b_flags) | f (b_f) | xa
// (b_xa).
struct LmSpans {
  size_t need, up, back;
  size_t ref, mu, lam;
  static constexpr size_t b_flags = 1, b_f = 3, b_xa = 4;
};
inline LmSpans carve_lm_state(int nb, int nq_, bool prior, double* d, LmState* ls) {
  const size_t nq = (size_t)nq_;
  const size_t o_ref = 2 * nq, o_mu = 3 * nq, o_lam = 4 * nq, o_flags = o_lam + 1, o_f = o_flags + 2, o_xa = o_f + 1,
               o_g = o_xa + nq, o_H = o_g + nq, o_Rb = o_H + nq * nq;
  if (d) {
    ls->x = d;
    ls->x_ref = d + o_ref;
    ls->mu = prior ? d + o_mu : nullptr;
    ls->lam = d + o_lam;
    ls->flags = (int*)(d + o_flags);
    ls->f = d + o_f;
    ls->xa = d + o_xa;
    ls->g = d + o_g;
    ls->H = d + o_H;
    ls->Rb = d + o_Rb;
  }
  return LmSpans{o_Rb + 24 * (size_t)nb, o_f, nq + 4, o_ref, o_mu, o_lam};
}
// the LM step's LDS (its carve and the kernel's static __shared__) fits one
// workgroup's 64 KB, nq one wave (the factorisation owns a row per lane), and
// the LM pose kernel's LDS (the tree blob of ni ints and nd doubles, the rigid
// step's carve, its static __shared__) fits too
bool lm_solver_fits(int nb, int nq, int S, int ni, int nd);
// diagnostic builds (-DFSDF_SOLVER_TIMES=1): solver_times for the LM step's launches
void lm_solver_times(unsigned long long* out);
// After evaluation it_before (0-based) — its pass, reduce and moments: the
// trial's wrapped objective (+ prior), accept / reject, on acceptance the
// Gauss-Newton matrix at the trial, the end conditions in the host loop's
// order, the damped step (degenerate factorisations raise the damping inside
// the launch) and the next trial into slot (it_before + 1) & 1. One workgroup.
// x, f, the count and the damping equal fsdf_lm_minimize's bit for bit.
hipError_t launch_lm_step(const SolverTree& T, const LmState& ls, const double* d_accum, const double* d_moments,
                          int it_before, hipStream_t s);
// FK of the trial in `slot`, its joint frames into that slot and the next
// pass's posed model pm (solver_init_kernel's work for a later trial; skips
// once flags[0] is set)
hipError_t launch_lm_pose(const SolverTree& T, const LmState& ls, const LocalModel& lm, const PosedModel& pm,
                          int precision, int slot, hipStream_t s);

// Exchanged spatial shards (fsdf_set_points_keyed_device): the bounding box
// (lo xyz, hi xyz; a device pointer into the scratch) of a device f64 cloud,
// the 30-bit curve keys of a cloud in a given device box (the keys
// sort_points_spatial orders by), and a resident cloud ordered by (key,
// whole-cloud index) with perm = those indices (< 2^31) — the order a shard of
// the whole cloud's sort_points_spatial order has. Asynchronous on `st`.
hipError_t cloud_box(const double* d_src, int64_t n, SortScratch& s, hipStream_t st, double** d_box);
// Seeds carried from one cloud to the next (sort.hip): a kVoxDim^3 grid of
// uint8 k* over a box fixed per context (lo, cells per unit length inv)
constexpr int kVoxDim = 64;
struct VoxBox {
  double lo[3] = {0, 0, 0}, inv[3] = {0, 0, 0};
};
// every point of a resident cloud (context precision) writes its prior k* (< 64) into its voxel
hipError_t vox_scatter(int precision, const void* d_pts, int64_t n, const uint8_t* d_prior, const VoxBox& b,
                       uint8_t* d_grid, hipStream_t st);
// every point's prior from its voxel (0xFF outside the box or in an empty voxel)
hipError_t vox_gather(int precision, const void* d_pts, int64_t n, const VoxBox& b, const uint8_t* d_grid,
                      uint8_t* d_prior, hipStream_t st);
hipError_t curve_keys(const double* d_src, int64_t n, const double* d_box, uint32_t* d_keys, hipStream_t st);
hipError_t sort_points_keyed(const double* d_src, const uint32_t* d_keys, const int64_t* d_index, int64_t n,
                             int precision, void* d_dst, int32_t* d_perm, SortScratch& s, hipStream_t st);

// d_out[i] = d_perm[i] as int64 (fsdf_get_permutation's layout)
hipError_t widen_permutation(const int32_t* d_perm, int64_t n, int64_t* d_out, hipStream_t st);

}  // namespace fsdf
