// ctx.h — the context behind include/flashsdf.h, shared by the host-side
// translation units: capi.hip (context, model, queries), cloud.hip (resident
// cloud), point_weights.hip (its per-point confidence weights), voxel.hip (its
// voxel-grid downsampling), pass.hip (the
// residual pass), iterate.hip (mechanism, one iteration), descend.hip (the
// solver loops).
//
// The context owns its device and pinned memory in the buffers of
// device_buffers.h (see the rule there: a pointer is read with get() after the
// reserve for that use). LocalModel, PosedModel and ChunkOutputs are views of
// them, filled where the buffers are reserved.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <string>
#include <utility>
#include <vector>

#include "device_buffers.h"
#include "flashsdf.h"
#include "fsdf_internal.h"
#if FSDF_HOST_TIMES
#include <chrono>
#endif

constexpr int kOrderEvery = FSDF_ORDER_EVERY;
constexpr int kPoseRing = 8;

// (the context's types and the functions shared by its translation units are
// internal: not exported)
#pragma GCC visibility push(hidden)
// device arrays of the local model (fsdf::LocalModel is their view) and the
// buffers sized by it
struct ModelBuffers {
  fsdf::DevBuf<double> verts_l, planes_l, sphere_l, box_l;
  fsdf::DevBuf<int32_t> faces, face_hull, face_off, vert_hull, vert_off, face_rows, hull_surface, item_meta,
      surface_kind, rbf_surface, rbf_row_off, rbf_acc_off;
  fsdf::DevBuf<double> rbf64;  // per-pass RBF rows (f64)
  fsdf::DevBuf<double> poses, accum;
};
// storage of one fsdf::PosedModel (T arrays in bytes)
struct PosedBuffers {
  fsdf::DevBuf<unsigned char> verts_w, hull_rows, planes_w, image_w;
  fsdf::DevBuf<float> screen_w;
};
// storage of fsdf::ChunkOutputs and the plan kernel's scratch
struct ChunkBuffers {
  fsdf::DevBuf<int32_t> hdr;
  fsdf::DevBuf<double> rows;  // ent | csum | dense: one allocation
  fsdf::DevBuf<uint32_t> dur;
  fsdf::DevBuf<int32_t> plan_order;
};
// a resident cloud: points (precision-typed AoS, bytes), resident i -> caller
// index (sorted / ranged clouds; none: the resident order is the caller's),
// [ceil(n/64)][4] bounding sphere per 64-point chunk
struct ResidentCloud {
  fsdf::DevBuf<unsigned char> pts;
  fsdf::DevBuf<int32_t> perm;
  fsdf::DevBuf<float> chunk_ws;
};

// the voxel-grid stage (voxel.hip): the (key, index) pairs double-buffered — the
// sorted pairs are k0 / i0 —, rocPRIM's temporary storage, the head-flag counts
// [2][blocks] and totals {m, dropped} with their pinned read-back, each voxel's
// first sorted position; then the lists kept for fsdf_get_voxels /
// fsdf_get_voxel_of_point, the weights and a depth frame's pixel list and cloud
struct VoxelBuffers {
  fsdf::DevBuf<uint64_t> k0, k1;
  fsdf::DevBuf<int32_t> i0, i1, counts, start;
  fsdf::DevBuf<unsigned char> tmp;
  fsdf::DevBuf<int64_t> total;
  fsdf::PinnedBuf<int64_t> h_total;
  fsdf::DevBuf<double> xyz;                     // [m][3] centroids
  fsdf::DevBuf<int32_t> count, cell, first;     // [m], [m][3], [m]
  fsdf::DevBuf<int32_t> of_point;               // [n_in]
  fsdf::DevBuf<double> weights;                 // [m + tail] (double)count, then 1.0 per free-space sample
  fsdf::DevBuf<int32_t> pix;                    // [m + tail] a depth frame's pixel list (swapped into depth_pix)
  fsdf::DevBuf<double> cloud;                   // [m + tail][3] a depth frame's centroids, then its samples
};

struct fsdf_ctx {
  int device = 0;
  int precision = 64;
  int sort_points = 0;
  int cull = 1;
  int out_order = FSDF_ORDER_CALLER;
  // streams and events ahead of the buffers: destroyed after them
  fsdf::Stream own_stream;
  hipStream_t stream = nullptr;  // own_stream or the caller's (fsdf_set_stream)
  fsdf::Stream copy_stream;
  fsdf::Event ev_prefetch;
  fsdf::Event pose_ev[kPoseRing], rbf_ev[kPoseRing];
  std::vector<fsdf::Event> prof_ev;  // pass-kernel timing (fsdf_profile_pass): triples
  std::string err;
  std::string pass_kernel;  // the pass-kernel variant of the last pass (fsdf_pass_kernel_name)

  // local model
  fsdf::LocalModel lm;
  ModelBuffers model;
  fsdf::PinnedBuf<double> h_rbf[kPoseRing];  // pinned staging ring for RBF rows (own slots and events,
                                             // independent of the pose ring: poses of <= 64
                                             // surfaces never touch theirs)
  std::vector<int32_t> h_surface_kind, h_n_centers;  // host copy of the surface list (set_surfaces)
  int rbf_slot = 0;
  bool rbf_ready = false;
  // posed model: rewritten by every pass's pose kernel (pose_model) or by the
  // device solver's step, in order on the context stream
  fsdf::PosedModel pm;
  PosedBuffers posed;
  fsdf::DevBuf<float> rbf32;  // the per-pass RBF rows of f32 contexts (pm.rbf_rows)
  // poses: pinned ring + device copy (model.poses)
  fsdf::PinnedBuf<double> h_poses[kPoseRing];
  int pose_slot = 0;
  // pinned read-back of the accumulator (fetch): a pageable destination makes
  // the D2H copy go through the runtime's staging buffer
  fsdf::PinnedBuf<double> h_acc;
  // resident cloud
  int64_t n = 0;
  ResidentCloud cur;
  fsdf::DevBuf<uint8_t> prior;       // [n] each resident point's nearest surface in the last pass (seed hint)
  bool prior_ok = false;             // prior is readable as seeds: every byte a surface of the model or 0xFF
                                     // (none) — written by a pass over the resident cloud, or gathered from
                                     // the previous cloud's voxels (finish_resident); the pass's prior_in
  bool prior_pass = false;           // ... and a pass over the current resident cloud wrote every byte (each
                                     // its point's k* < 64, never 0xFF): what the regroup groups by and the
                                     // next cloud's seeds are carried from
  // regroup (fsdf_regroup_points): mode (fsdf_set_regroup), whether the
  // resident cloud has been regrouped since its set_points, whether its first
  // iteration pass is still to come (the auto regroup follows that pass), and
  // the shape of the last resident pass (the auto rule's input)
  int regroup_mode = FSDF_REGROUP_AUTO;
  bool regrouped = false;
  bool regroup_pending = false;
  int last_pass_shape = 0;           // 0 none, 1 one wave per chunk, 2 hull-partitioned tiers, 3 planned
  fsdf::SortScratch sort;            // per-frame sort scratch (grown only)
  fsdf::DevBuf<double> staging;      // host-source clouds land here first
  // the next frame's cloud, copied ahead on a stream of its own (fsdf_prefetch_points)
  fsdf::DevBuf<double> prefetch;
  int64_t prefetch_n = -1;           // -1: none pending
  // a prefetch is queued on the next pass's launch (its host-side work then
  // overlaps that pass instead of delaying the frame's first launch): the
  // caller's cloud, whether it is still to be issued, and the issue's result
  const double* prefetch_src = nullptr;
  bool prefetch_deferred = false;
  int prefetch_rc = 0;
  // ... and its resident form, sorted there too (swapped in by fsdf_set_points_prefetched)
  bool prefetch_sorted = false;
  ResidentCloud next;
  fsdf::SortScratch sort_next;
  // seeds carried from one cloud to the next (a voxel grid of the last pass's k*)
  fsdf::DevBuf<uint8_t> vox_grid;
  bool vox_ok = false, seed_pending = false;
  fsdf::VoxBox vox;
  bool ranged = false;               // the resident cloud is a range of a larger one (fsdf_set_points_range)
  fsdf::DevBuf<unsigned char> range_pts;  // fsdf_set_points_range: the whole cloud, sorted (scratch)
  fsdf::DevBuf<int32_t> range_perm;
  // work
  fsdf::DevBuf<double> partials;
  // cost-ordered schedule of resident-cloud passes (fsdf::PassOutputs::order)
  fsdf::DevBuf<uint32_t> block_cost;  // [kMaxBlocks]
  // the one-wave grid's heaviest-first block orders, one per layout of a frame's
  // cloud: [0] its Hilbert order (the frame's first pass), [1] regrouped (the
  // rest of the frame) — each rebuilt from the costs of a pass in its layout, so
  // a frame's passes run the order the previous frame left for the same layout
  fsdf::DevBuf<int32_t> block_order[2];  // [kMaxBlocks]
  int order_nblocks[2] = {0, 0};  // grid the order was built for (0: none yet)
  int order_age[2] = {0, 0};      // passes since the order was rebuilt
  // planned pass (fsdf::planned_pass_kernel): per-chunk partial rows, chunk
  // durations and the workgroup plan built from them (fsdf_set_plan)
  fsdf::ChunkOutputs co;             // view of chunk, [co.cap] chunks
  ChunkBuffers chunk;
  int co_s = 0;                      // surfaces the dense rows of co were sized for
  fsdf::DevBuf<int32_t> plan;        // [grid][4]
  int plan_grid = 0;                 // workgroups of the current plan (0: none — the default shape)
  int64_t plan_nc = -1;              // chunks the plan was built for
  int plan_age = 0;                  // planned passes since the plan was rebuilt
  int plan_enable = 1;
  double plan_f4 = -1.0, plan_f2 = -1.0;  // shares of the chunks split over 4 / 2 waves (< 0: default counts)
  int wave_slots = 0;                // device wave slots at the pass's occupancy (0: not queried yet)
  int64_t plan_max_points = -1;      // planned pass up to this cloud size (per device; -1: the model's default)
  fsdf::DevBuf<int32_t> kstar;       // per-point outputs (fsdf_eval, fsdf_skin, fsdf_raycast)
  fsdf::DevBuf<double> d, grad;
  // second moments of the residual (fsdf_eval_moments, fsdf_value_gradient_hessian;
  // moments.hip): the workgroups' partials, the [S][21] sums, their pinned read-back
  fsdf::DevBuf<double> moments_partials, moments;
  fsdf::PinnedBuf<double> h_moments;
  // second moments of the RBF skins (fsdf_eval_skin_moments, fsdf_value_gradient_hessian with
  // fsdf_set_lm_skins; skin_moments.hip): the workgroups' partial blocks, the skins' [m][m]
  // matrices one after the other, their pinned read-back
  fsdf::DevBuf<double> skin_partials, skin_moments;
  fsdf::PinnedBuf<double> h_skin_moments;
  std::vector<fsdf::Event> skin_ev;  // skin-moments timing (fsdf_profile_pass): pairs around its launches
  size_t skin_ev_used = 0;
  // robust point loss (fsdf_set_loss: a context setting, kept over model and cloud swaps) and the
  // buffers of its reduction (fsdf_eval_robust and the iteration entry points with a loss;
  // robust.hip): the workgroups' partials, the [S][29] (or [S][8]) rows, their pinned read-back
  int loss_kind = FSDF_LOSS_SQUARE;
  double loss_scale = 0.0;
  fsdf::DevBuf<double> robust_partials, robust_rows;
  fsdf::PinnedBuf<double> h_robust;
  std::vector<double> robust_accum, robust_moments;  // the accumulator (fsdf_eval's layout) and moments [S][21] from the rows
  // the device solver loops on a robust objective (fsdf_set_robust_loops: a context setting like
  // robust_skins, off by default; descend.hip): the accumulator [1 + 6S] and moments [S][21]
  // assembled from the rows on the device (robust.hip robust_assemble_kernel), which the step
  // kernels read in place of the pass's least-squares accumulator and the moments kernel's sums
  int robust_loops = 0;
  fsdf::DevBuf<double> robust_dev_accum, robust_dev_moments;
  // robust objectives on RBF skins and deformations (fsdf_set_robust_skins: a context setting like
  // lm_skins; robust_skin.hip): the workgroups' partials, the skins' blocks [rbf_acc], their pinned
  // read-back. The weighted skin moments reuse skin_partials / skin_moments / h_skin_moments.
  int robust_skins = 0;
  fsdf::DevBuf<double> robust_skin_partials, robust_skin_blocks;
  fsdf::PinnedBuf<double> h_robust_skin;
  // per-point confidence weights (fsdf_set_point_weights; point_weights.hip): they belong to the
  // resident cloud (every new one clears them). conf_src [n] in the caller's order, conf_res [n]
  // in resident order (sorted clouds: gathered through cur.perm; conf_stale: the layout changed
  // since, regather before the next robust launch). A cloud with no permutation reads conf_src.
  fsdf::DevBuf<double> conf_src, conf_res;
  bool conf_set = false, conf_stale = false;
  // depth frames (fsdf_set_sensor, fsdf_set_depth_*; cloud.hip over depth.hip): the sensor — a
  // context setting like the loss — as one direction per pixel, sensor_u [rows·cols][3]
  // (sensor_rows == 0: none); the frame's raw image (host sources land here), the per-block
  // counts / offsets, the pinned total; depth_pix [n] each caller point's pixel, valid while
  // depth_cloud says the resident cloud came from a depth frame. The frame's fp64 cloud is
  // written to `staging`.
  int sensor_rows = 0, sensor_cols = 0, sensor_kind = 0;
  fsdf::DevBuf<double> sensor_u;
  fsdf::DevBuf<unsigned char> depth_raw;
  fsdf::DevBuf<int32_t> depth_counts, depth_pix;
  fsdf::DevBuf<int64_t> depth_total;
  fsdf::PinnedBuf<int64_t> h_depth_total;
  bool depth_cloud = false;
  // free space (fsdf_set_free_split, fsdf_set_free_space; robust.hip ONE_SIDED, depth.hip): free_split
  // is the resident cloud's n_surface — caller points [free_split, n) are free-space samples — and
  // belongs to the cloud like the weights (-1: none; every new cloud clears it). The samples a depth
  // frame sends are a context setting like the sensor (free_samples 0: off); a frame with them on
  // reads two totals back (depth_total / h_depth_total [2], depth_counts [2][blocks]).
  int64_t free_split = -1;
  int free_samples = 0, free_stride = 1;
  double free_gap = 0.0, free_spacing = 0.0, free_miss = 0.0;
  // voxel grid (fsdf_set_voxel_grid, fsdf_set_points_voxel, depth frames; voxel.hip): the grid is a
  // context setting like the sensor (vox_size 0: off). voxel_cloud says the resident cloud came
  // through it: `voxel` then holds its lists — vox_m voxels of vox_n_in input points, vox_dropped
  // of them non-finite —, which belong to the cloud like a depth frame's pixel list.
  double vox_size = 0.0, vox_origin[3] = {0.0, 0.0, 0.0};
  int vox_weights = FSDF_VOXEL_COUNT;
  bool voxel_cloud = false;
  int64_t vox_m = 0, vox_n_in = 0, vox_dropped = 0;
  VoxelBuffers voxel;
  // scoring candidate states (fsdf_score_poses, fsdf_score_states; score_api.hip over score.hip): the
  // batch's poses [B][S][12] and costs [B] on the device and pinned, one slice's posed tables and
  // partials; buffers of their own — a scoring call writes nothing any other call reads. Timing
  // (fsdf_score_time): a pair of events per profiled call, created on first use.
  fsdf::DevBuf<double> score_poses, score_partials, score_cost;
  fsdf::DevBuf<unsigned char> score_tables;
  fsdf::PinnedBuf<double> h_score_poses, h_score_cost;
  std::vector<fsdf::Event> score_ev;
  size_t score_ev_used = 0;
  // gradients and moments of candidate states (fsdf_batch_robust_poses, fsdf_batch_states and the
  // lockstep loops over them; batch_api.hip over batch.hip): the batch's poses [B][S][12] and rows
  // [B][S · 29] on the device and pinned, one slice's posed tables, per-point blocks (k*, d*, ∇d* per
  // (candidate, point)) and partials; buffers of these calls alone, grown only — a call writes
  // nothing any other call reads. Timing (fsdf_batch_time) as the scoring calls'.
  fsdf::DevBuf<double> batch_poses, batch_partials, batch_rows;
  fsdf::DevBuf<unsigned char> batch_tables, batch_points;
  fsdf::PinnedBuf<double> h_batch_poses, h_batch_rows;
  std::vector<fsdf::Event> batch_ev;
  size_t batch_ev_used = 0;
  // query scratch (fsdf_skin)
  fsdf::DevBuf<unsigned char> q;
  fsdf::DevBuf<double> q64;
  bool profiling = false;
  size_t prof_used = 0;             // events recorded (3 per pass)
  fsdf::DevBuf<unsigned long long> stats;  // fsdf_kernel_stats
  bool stats_on = false;
  // mechanism of fsdf_set_mechanism (host arrays; fsdf_value_and_gradient)
  struct Mechanism {
    int nb = 0, nq = 0;
    std::vector<int32_t> parent, kind, qoff, surface_body;
    std::vector<double> axis, AR, At, BR, Bt, frame_R, frame_t;
    std::vector<double> R, t, Rb, tb, poses, work;  // scratch
    std::vector<double> gn_work;                    // fsdf_gauss_newton_matrix's (fsdf_value_gradient_hessian)
    std::vector<double> skin_L, skin_work, gn_hull; // fsdf_rbf_state_map's L and scratch, the hulls' [nq][nq] (lm_skins)
    // RBF surfaces (fsdf_set_rbf_centres), in surface order; n == 0: undeclared
    struct Rbf {
      int n_sp = 0, n = 0;
      std::vector<int32_t> body, drow, piv;
      std::vector<double> local, values, centres, u, lu, G, work;
    };
    std::vector<Rbf> rbf;
    int n_deform = 0;
    double weight = 10.0;  // default_deformation_cost_weight (src/gradientdescent.jl:7)
    std::vector<double> rows, body_wrench, x_prepared;
    // the x of the last two fsdf_eval_state_device passes (their accumulators
    // may still be in flight): fsdf_state_gradient accepts only these (or the
    // last prepared x) and refuses any other with FSDF_ERR_STATE
    std::vector<double> x_pass[2];
    int x_pass_next = 0;
  } mech;
  int lm_skins = 0;                  // fsdf_set_lm_skins: the second-order solver serves skins and deformations
  int lm_solver_device = 0;          // fsdf_set_lm_solver: 0 host loop (default), 1 device where it fits, 2 required
  std::vector<double> lm_prior;      // fsdf_set_lm_prior: fsdf_descend_lm's prior weights (empty: none)
  // device solver loop of fsdf_descend (solver.hip): the mechanism's device
  // arrays (built on the first device descend after fsdf_set_mechanism) and
  // one frame's state; pinned staging for x / divisors in and x, f, flags out
  int solver_device = 1;             // fsdf_set_solver: 1 device where possible (default), 0 host loop,
                                     // 2 device required; 3 / 4: as 1 / 2 with RBF
                                     // and deformable scenes admitted
  bool solver_tree_ok = false;
  fsdf::SolverTree stree;
  fsdf::DevBuf<double> stree_blob;   // the tree blob (fsdf::SolverTree::blob)
  fsdf::DevBuf<double> solver;       // x | div | Rb | tb | poses | f (descend_device), or descend_lm_device's state
  fsdf::DevBuf<int> solver_flags;
  fsdf::PinnedBuf<double> h_solver;  // pinned: x | div | f | flags (as doubles)
};

static inline int fail(fsdf_ctx* c, int code, const char* fmt, ...) {
  if (c) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    c->err = buf;
  }
  return code;
}

#define HIPCHECK(ctx, expr)                                                                             \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) return fail((ctx), FSDF_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

static inline int accum_len(const fsdf_ctx* c) { return 1 + 6 * c->lm.S + c->lm.rbf_acc; }
static inline size_t point_bytes(const fsdf_ctx* c) { return c->precision == 64 ? sizeof(double) : sizeof(float); }

// file-local functions that cross the translation units
// cloud.hip
int adopt_points_device(fsdf_ctx* c, const double* d_src, int64_t n, fsdf::DevBuf<unsigned char>& dst);
int prefetch_issue(fsdf_ctx* c);
// pass.hip
int pose_model(fsdf_ctx* c, const double* poses, bool posed = false);
int run_pass(fsdf_ctx* c, const double* poses, const void* d_pts, int64_t n, double* d_accum, int32_t* d_kstar,
             double* d_d, double* d_grad, const int32_t* d_perm, bool schedule, bool posed = false,
             const int* skip = nullptr);
int ensure_outputs(fsdf_ctx* c, int64_t n);
int ensure_host_acc(fsdf_ctx* c, int len);
// (the pass with k*, ∇d* in resident order, then the moments: h_acc and h_moments in flight;
// what: kMomentsRigid the hulls' of a rigid scene, kMomentsAll the hulls' and the skins'
// (h_skin_moments) of any scene, kMomentsSkins the skins' alone)
enum { kMomentsRigid = 0, kMomentsAll = 1, kMomentsSkins = 2 };
int run_pass_moments(fsdf_ctx* c, const double* poses, const char* who, int what = kMomentsRigid);
// (the pass with k*, d*, ∇d* in resident order, then the robust launch: the rows [S][29] (moments)
// or [S][8] to h_robust, in flight; hull-only scenes — with fsdf_set_robust_skins also scenes with
// RBF skins and deformations: the skins' blocks (robust_skin.hip) to h_robust_skin and — moments —
// their weighted second moments to h_skin_moments. robust_rows_finish, after the
// synchronisation: robust_accum (fsdf_eval's layout, Σρ summed in surface order, a skin's wrench
// 0.0, then the skins' blocks) and — moments — robust_moments from the rows (a skin's row zero))
int run_pass_robust(fsdf_ctx* c, const double* poses, const char* who, bool moments);
void robust_rows_finish(fsdf_ctx* c, bool moments);
// point_weights.hip: the weights in resident order for a robust launch (null: none set), regathered
// on the context stream when the layout changed since; whether the iteration calls take the robust path
int point_weights_resident(fsdf_ctx* c, const double** d_conf_out);
// voxel.hip: d_xyz [n][3] (device, fp64) through the context's grid into c->voxel (one sizing
// synchronisation; the caller synchronised the stream before); then the weights [vox_m + tail]
// — the counts, 1.0 per tail point — and, from a depth frame's pixel list, c->voxel.pix; and the
// counts as the resident cloud's weights under FSDF_VOXEL_COUNT
int voxel_downsample(fsdf_ctx* c, const double* d_xyz, int64_t n, const char* who);
int voxel_finish(fsdf_ctx* c, int64_t tail, const int32_t* d_pix_in);
int voxel_set_weights(fsdf_ctx* c);
static inline bool robust_objective(const fsdf_ctx* c) {
  return c->loss_kind != FSDF_LOSS_SQUARE || c->conf_set || c->free_split >= 0;
}
int fetch(fsdf_ctx* c, int64_t n, double* cost_out, double* accum_out, int32_t* kstar_out, double* d_out,
          double* grad_out, bool want_pp);
// iterate.hip (the solver loops of descend.hip run on them)
// after an iteration pass: the new cloud's first one regroups it when the auto rule says so
int iteration_regroup(fsdf_ctx* c);
// the host halves of one CostFunctor iteration at x around a pass: prepare = FK, RBF centres +
// weight solve + rows upload, surface poses; finish = RBF adjoint, chain rule, regularizer
int iteration_prepare(fsdf_ctx* c, const double* x, const char* who, bool upload = true);
int iteration_finish(fsdf_ctx* c, const double* x, const double* accum, double* cost_out, double* grad_out,
                     const char* who);

// diagnostic builds (-DFSDF_HOST_TIMES=1): host-side clocks of the host solver
// loop's iterations — prepare (FK, poses), launches, the wait, the chain rule —
// summed by fsdf_value_and_gradient (iterate.hip) and printed by fsdf_descend
// (descend.hip, stderr), to split the GPU's idle gap between iterations into
// host work and synchronisation latency
#if FSDF_HOST_TIMES
extern double g_host_t[8];
extern long g_host_n;
static inline double host_now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
#define HOST_STAMP(i) const double ht_##i = host_now_us()
#else
#define HOST_STAMP(i)
#endif
#pragma GCC visibility pop
