// pass.hip — one residual pass of a context (pose -> pass -> reduce): the
// partial sums, the pose ring, the planned pass and its plan, the per-point
// outputs and their read-back, fsdf_eval / fsdf_eval_device, the permutation
// getters, and the pass followed by the second-moments reduction
// (run_pass_moments, fsdf_eval_moments) or by the sums of a robust point loss
// (fsdf_set_loss, run_pass_robust, fsdf_eval_robust; on scenes with RBF skins
// behind fsdf_set_robust_skins, fsdf_eval_robust_skins).

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.h"
#include "robust_impl.h"

// default plan composition: chunks split over 4 / 2 waves (fsdf_set_plan shares < 0)
static constexpr int64_t kPlanDefault4 = 96, kPlanDefault2 = 192;

static int ensure_partials(fsdf_ctx* c, int nblocks) {
  // (rounded up to whole 8-entry tiles: FSDF_PARTIALS_LAYOUT 2)
  const size_t need = (size_t)((accum_len(c) + 7) & ~7) * nblocks;
  HIPCHECK(c, c->partials.reserve(need));
  return FSDF_OK;
}

static int upload_poses(fsdf_ctx* c, const double* poses, hipStream_t st) {
  for (int i = 0; i < 12 * c->lm.S; ++i)
    if (!std::isfinite(poses[i])) return fail(c, FSDF_ERR_ARG, "poses: entry %d is not finite", i);
  if (c->lm.S <= fsdf::kPoseArgMax) return FSDF_OK;  // they ride in the pose kernel's arguments
  const int s = c->pose_slot;
  c->pose_slot = (s + 1) % kPoseRing;
  HIPCHECK(c, hipEventSynchronize(c->pose_ev[s]));  // slot free once its last copy ran
  memcpy(c->h_poses[s].get(), poses, (size_t)c->lm.S * 12 * sizeof(double));
  HIPCHECK(c, hipMemcpyAsync(c->model.poses.get(), c->h_poses[s].get(), (size_t)c->lm.S * 12 * sizeof(double),
                             hipMemcpyHostToDevice, st));
  HIPCHECK(c, hipEventRecord(c->pose_ev[s], st));
  return FSDF_OK;
}

// Pose the model for one pass into c->pm, in order on the context stream.
// (Posing into a second buffer on a stream of its own, to overlap the previous
// pass's tail and reduce, measured slower: the cross-stream event waits cost
// more than the overlap saves, +10 us per step on M64.)
// posed: the model is already posed on the device (the device solver loop's
// step poses the next pass's model itself, solver.hip): no pose launch.
int pose_model(fsdf_ctx* c, const double* poses, bool posed) {
  if (posed) return FSDF_OK;
  int rc = upload_poses(c, poses, c->stream);
  if (rc) return rc;
  HIPCHECK(c, fsdf::launch_pose(c->precision, c->lm, c->model.poses.get(), c->pm, c->stream,
                                c->lm.S <= fsdf::kPoseArgMax ? poses : nullptr));
  return FSDF_OK;
}

static int ensure_chunk_outputs(fsdf_ctx* c, int64_t nc) {
  if (c->co.cap >= nc && c->co_s >= c->lm.S) return FSDF_OK;
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  c->co = fsdf::ChunkOutputs();
  c->chunk = ChunkBuffers();  // (all four anew, at this cloud's chunk count)
  c->plan_nc = -1;
  HIPCHECK(c, c->chunk.hdr.reserve((size_t)nc * 4));
  // one allocation: entries [nc][24] | Σ d² [nc] | dense rows [nc][S][6] (sized by the surface count:
  // (25 + 6 S) doubles per chunk, 1.6 KB at S = 64 — per context, so two in flight hold it twice)
  HIPCHECK(c, c->chunk.rows.reserve((size_t)nc * (24 + 1 + 6 * (size_t)c->lm.S)));
  c->co_s = c->lm.S;
  HIPCHECK(c, c->chunk.dur.reserve((size_t)nc));
  HIPCHECK(c, c->chunk.plan_order.reserve((size_t)nc));
  c->co.hdr = c->chunk.hdr.get();
  c->co.ent = c->chunk.rows.get();
  c->co.csum = c->co.ent + (size_t)nc * 24;
  c->co.dense = c->co.ent + (size_t)nc * 25;
  c->co.dur = c->chunk.dur.get();
  c->co.cap = nc;
  return FSDF_OK;
}

// the plan's composition for nc chunks: n4 chunks over 4 waves, n2 over 2,
// the rest one wave each. The heaviest `plan_f4` / `plan_f2` shares are split,
// and at least as many chunks over 4 waves as the device's idle wave slots
// allow (slots - nc, 3 extra waves per split chunk): a strong-scaling shard
// that leaves slots free splits its heavy third, a full machine only its tail.
static int wave_slots(fsdf_ctx* c) {
  if (c->wave_slots == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus <= 0)
      cus = 256;
    c->wave_slots = cus * 4 * 4;  // 4 SIMDs x 4 waves (the pass's register budget)
  }
  return c->wave_slots;
}

static void plan_shape(fsdf_ctx* c, int64_t nc, int* n4, int* n2) {
  wave_slots(c);
  const int64_t spare = std::max<int64_t>(0, (int64_t)c->wave_slots - nc);
  // default (shares < 0): fixed counts — the heavy tail that outlasts the rest
  // of a pass is ~100 chunks at 2^18 and at 2^19 points alike (measured)
  const int64_t want4 = c->plan_f4 < 0 ? kPlanDefault4 : llround(c->plan_f4 * (double)nc);
  const int64_t want2 = c->plan_f2 < 0 ? kPlanDefault2 : llround(c->plan_f2 * (double)nc);
  const int64_t a = std::min<int64_t>(nc, std::max<int64_t>(want4, spare / 3));
  *n4 = (int)a;
  *n2 = (int)std::min<int64_t>(nc - a, want2);
}

// The planned pass of a resident cloud: per-chunk partial rows, the
// two-level chunk reduction (16-chunk groups, then the tile reduce), and a
// plan rebuilt from this pass's chunk durations on the first pass of a cloud
// and then every kOrderEvery passes.
static int run_planned(fsdf_ctx* c, const fsdf::PosedModel& P, const void* d_pts, int64_t n, double* d_accum,
                       fsdf::PassOutputs& out, const fsdf::Event* pe, const int* skip) {
  const int64_t nc = (n + 63) / 64;
  int rc = ensure_chunk_outputs(c, nc);
  if (rc) return rc;
  rc = ensure_partials(c, (int)std::max<int64_t>(fsdf::pass_blocks(n, c->lm), fsdf::reduce_chunk_groups(nc)));
  if (rc) return rc;
  out.partials = c->partials.get();
  out.cost = nullptr;
  out.order = nullptr;
  fsdf::ChunkOutputs co = c->co;
  // the split speed-ups behind the serial-equivalent durations (plan order,
  // fsdf_chunk_costs, the shard rebalance): M64-class scenes (>= 32 hulls)
  // measured 1.82-1.87x at 4 waves and 1.28-1.33x at 2 (tools/split_speedup.py,
  // profiles/r05/split_speedup.jsonl); IRB140-class measurements scattered
  // (4-way 1.22-1.53x) and their plan ran slower with them (profiles/r05/
  // keyed_plan), so those keep round 4's 5/2 and 8/5
  if (c->lm.K >= 32) {
    co.r4n = 15; co.r4d = 8; co.r2n = 4; co.r2d = 3;
  }
  const bool planned = c->plan_nc == nc && c->plan_grid > 0;
  co.plan = planned ? c->plan.get() : nullptr;
  const int dparts = fsdf::hpart_parts(c->lm, n);
  co.dparts = dparts ? dparts : 1;
  const int grid = planned ? c->plan_grid : (int)((nc * co.dparts + 3) / 4);
  HIPCHECK(c, fsdf::launch_planned_pass(c->precision, c->cull != 0, c->lm, P, d_pts, n, grid, out, co, c->stream,
                                        pe ? (hipEvent_t)pe[0] : nullptr, pe ? (hipEvent_t)pe[1] : nullptr));
  c->pass_kernel = fsdf::last_pass_kernel();
  HIPCHECK(c, fsdf::launch_reduce_chunks(co, nc, c->lm.S, c->partials.get(), d_accum, c->stream,
                                         pe ? (hipEvent_t)pe[2] : nullptr, skip));
  if (!planned || ++c->plan_age >= kOrderEvery) {
    int n4, n2;
    plan_shape(c, nc, &n4, &n2);
    const int64_t g = n4 + (n2 + 1) / 2 + (nc - n4 - n2 + 3) / 4;
    if (c->plan.capacity() < (size_t)g * 4) HIPCHECK(c, hipStreamSynchronize(c->stream));
    HIPCHECK(c, c->plan.reserve((size_t)g * 4));
    HIPCHECK(c, fsdf::launch_plan(c->co.dur, nc, n4, n2, c->chunk.plan_order.get(), c->plan.get(), c->stream));
    c->plan_grid = (int)g;
    c->plan_nc = nc;
    c->plan_age = 0;
  }
  return FSDF_OK;
}

// schedule: resident-cloud passes (repeated over the same cloud) launch their
// workgroups heaviest-first by the previous pass's durations
// posed / skip: the device solver loop's pass — its model posed by the
// previous step (pose_model), its done flag
static int run_pass_impl(fsdf_ctx* c, const double* poses, const void* d_pts, int64_t n, double* d_accum,
                         int32_t* d_kstar, double* d_d, double* d_grad, const int32_t* d_perm, bool schedule,
                         bool posed, const int* skip) {
  if (c->lm.R > 0 && !c->rbf_ready)
    return fail(c, FSDF_ERR_STATE, "eval: the scene has RBF surfaces: call fsdf_set_rbf_params first");
  int rc = pose_model(c, poses, posed);
  if (rc) return rc;
  const bool resident = d_pts == c->cur.pts.get() && n == c->n;
  const int nblocks = fsdf::pass_blocks(n, c->lm);
  rc = ensure_partials(c, nblocks);
  if (rc) return rc;
  fsdf::PassOutputs out;
  out.partials = c->partials.get();
  out.kstar = d_kstar;
  out.d = d_d;
  out.grad = d_grad;
  out.perm = d_perm;
  out.stats = c->stats_on ? c->stats.get() : nullptr;
  out.skip = skip;
  out.chunk_ws = resident ? c->cur.chunk_ws.get() : nullptr;  // resident cloud only
  // the previous pass's nearest surfaces as seeds (resident cloud, hull-only
  // scenes of <= 64 surfaces; fsdf_internal.h PassOutputs::prior_in); marked
  // written (prior_ok, prior_pass) once the pass is launched — stream-ordered, the next
  // pass reads what this one writes
  const bool prior = resident && n > 0 && c->prior.capacity() >= (size_t)n && c->lm.R == 0 && c->lm.S <= 64;
  out.prior_out = prior ? c->prior.get() : nullptr;
  out.prior_in = prior && c->prior_ok ? c->prior.get() : nullptr;
  // planned window: (default min, model's default max], or (0, max_points] when set
  const int64_t plan_max = c->plan_max_points >= 0 ? c->plan_max_points : fsdf::planned_default_max_points(c->lm);
  const int64_t plan_min = c->plan_max_points >= 0 ? 0 : fsdf::planned_default_min_points();
  if (schedule && n > plan_min && c->plan_enable && n <= plan_max && c->precision == 64 &&
      fsdf::planned_pass(c->lm, n)) {
    const bool prof = c->profiling && c->prof_used + 3 <= c->prof_ev.size();
    const fsdf::Event* pe = prof ? &c->prof_ev[c->prof_used] : nullptr;
    rc = run_planned(c, c->pm, d_pts, n, d_accum, out, pe, skip);
    if (rc) return rc;
    if (prior) c->prior_ok = c->prior_pass = true;
    if (resident) c->last_pass_shape = 3;
    if (prof) c->prof_used += 3;
    return FSDF_OK;
  }
  const int ol = c->regrouped ? 1 : 0;  // (the layout's block order)
  if (schedule && n > 0) {
    HIPCHECK(c, c->block_cost.reserve(fsdf::kMaxBlocks));
    HIPCHECK(c, c->block_order[0].reserve(fsdf::kMaxBlocks));
    HIPCHECK(c, c->block_order[1].reserve(fsdf::kMaxBlocks));
    out.cost = c->block_cost.get();
    out.order = c->order_nblocks[ol] == nblocks ? c->block_order[ol].get() : nullptr;
  }
  if (n > 0) {
    // profiling: the pass kernel's start / end and the reduce's end, stamped
    // by the dispatches themselves (no packets of their own between kernels)
    const bool prof = c->profiling && c->prof_used + 3 <= c->prof_ev.size();
    const fsdf::Event* pe = prof ? &c->prof_ev[c->prof_used] : nullptr;
    HIPCHECK(c, fsdf::launch_pass(c->precision, c->cull != 0, c->lm, c->pm, d_pts, n, nblocks, out, c->stream,
                                  pe ? (hipEvent_t)pe[0] : nullptr, pe ? (hipEvent_t)pe[1] : nullptr));
    c->pass_kernel = fsdf::last_pass_kernel();
    if (prior) c->prior_ok = c->prior_pass = true;
    if (resident) c->last_pass_shape = fsdf::hpart_pass(c->lm, n) ? 2 : 1;
    if (prof) c->prof_used += 3;
    // the order is rebuilt on the first scheduled pass of a grid and then every
    // kOrderEvery passes (the heavy blocks of a cloud stay heavy from pass to
    // pass; the rebuild is a ~7 us single-workgroup sort on the reduce launch)
    const bool rebuild = out.cost && (c->order_nblocks[ol] != nblocks || ++c->order_age[ol] >= kOrderEvery);
    HIPCHECK(c, fsdf::launch_reduce(c->partials.get(), nblocks, accum_len(c), d_accum, c->stream,
                                    rebuild ? out.cost : nullptr, rebuild ? c->block_order[ol].get() : nullptr,
                                    pe ? (hipEvent_t)pe[2] : nullptr, skip));
    if (rebuild) {
      c->order_nblocks[ol] = nblocks;
      c->order_age[ol] = 0;
    }
  } else {
    HIPCHECK(c, hipMemsetAsync(d_accum, 0, (size_t)accum_len(c) * sizeof(double), c->stream));
  }
  return FSDF_OK;
}

// A pass, then a prefetch still to be issued (fsdf_prefetch_points): its copy,
// sort launches and their host-side cost go behind this pass, which the device
// is already running (profiles/r06/prefetch_defer/). Its result waits for
// fsdf_set_points_prefetched.
int run_pass(fsdf_ctx* c, const double* poses, const void* d_pts, int64_t n, double* d_accum, int32_t* d_kstar,
             double* d_d, double* d_grad, const int32_t* d_perm, bool schedule, bool posed, const int* skip) {
  const int rc = run_pass_impl(c, poses, d_pts, n, d_accum, d_kstar, d_d, d_grad, d_perm, schedule, posed, skip);
  if (!rc && c->prefetch_deferred) c->prefetch_rc = prefetch_issue(c);
  return rc;
}

// per-point outputs of resident-cloud passes: scattered to caller order through
// the sort permutation, or written in resident order (coalesced)
// (a ranged cloud, fsdf_set_points_range: always resident order — its
// permutation names indices of the WHOLE cloud, beyond the outputs' length)
static const int32_t* out_perm(const fsdf_ctx* c) {
  return c->out_order == FSDF_ORDER_RESIDENT || c->ranged ? nullptr : c->cur.perm.get();
}

static int get_perm(fsdf_ctx* c, int64_t* out, bool device) {
  if (!c) return FSDF_ERR_ARG;
  if (c->n > 0 && !out) return fail(c, FSDF_ERR_ARG, "get_permutation: null output");
  HIPCHECK(c, hipSetDevice(c->device));
  if (c->n == 0) return FSDF_OK;
  if (const int32_t* d_perm = c->cur.perm.get()) {
    std::vector<int32_t> p32;
    if (device) {
      HIPCHECK(c, fsdf::widen_permutation(d_perm, c->n, out, c->stream));
    } else {
      p32.resize((size_t)c->n);
      HIPCHECK(c, hipMemcpyAsync(p32.data(), d_perm, (size_t)c->n * sizeof(int32_t), hipMemcpyDeviceToHost,
                                 c->stream));
    }
    HIPCHECK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < p32.size(); ++i) out[i] = p32[i];
  } else if (device) {
    std::vector<int64_t> id((size_t)c->n);
    for (int64_t i = 0; i < c->n; ++i) id[(size_t)i] = i;
    HIPCHECK(c, hipMemcpy(out, id.data(), (size_t)c->n * sizeof(int64_t), hipMemcpyHostToDevice));
  } else {
    for (int64_t i = 0; i < c->n; ++i) out[i] = i;
  }
  return FSDF_OK;
}

extern "C" int fsdf_get_permutation(fsdf_ctx* c, int64_t* perm_out) { return get_perm(c, perm_out, false); }
extern "C" int fsdf_get_permutation_device(fsdf_ctx* c, int64_t* d_perm_out) { return get_perm(c, d_perm_out, true); }

extern "C" int fsdf_eval_device(fsdf_ctx* c, const double* poses, double* d_accum, int32_t* d_kstar, double* d_d,
                                double* d_grad) {
  if (!c) return FSDF_ERR_ARG;
  if (c->lm.S == 0) return fail(c, FSDF_ERR_STATE, "eval: no model (call fsdf_set_model first)");
  if (!poses || !d_accum) return fail(c, FSDF_ERR_ARG, "eval_device: poses and d_accum are required");
  HIPCHECK(c, hipSetDevice(c->device));
  return run_pass(c, poses, c->cur.pts.get(), c->n, d_accum, d_kstar, d_d, d_grad, out_perm(c), true);
}

int ensure_outputs(fsdf_ctx* c, int64_t n) {
  HIPCHECK(c, c->kstar.reserve((size_t)n));
  HIPCHECK(c, c->d.reserve((size_t)n));
  HIPCHECK(c, c->grad.reserve((size_t)std::max<int64_t>(n, 1) * 3));
  return FSDF_OK;
}

int ensure_host_acc(fsdf_ctx* c, int len) {
  HIPCHECK(c, c->h_acc.reserve((size_t)len));
  return FSDF_OK;
}

int fetch(fsdf_ctx* c, int64_t n, double* cost_out, double* accum_out, int32_t* kstar_out, double* d_out,
                 double* grad_out, bool want_pp) {
  const int len = accum_len(c);
  int rc = ensure_host_acc(c, len);
  if (rc) return rc;
  double* acc = c->h_acc.get();
  HIPCHECK(c, hipMemcpyAsync(acc, c->model.accum.get(), len * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (want_pp && n > 0) {
    if (kstar_out)
      HIPCHECK(c, hipMemcpyAsync(kstar_out, c->kstar.get(), n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (d_out) HIPCHECK(c, hipMemcpyAsync(d_out, c->d.get(), n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (grad_out)
      HIPCHECK(c, hipMemcpyAsync(grad_out, c->grad.get(), n * 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  if (cost_out) *cost_out = acc[0];
  if (accum_out) memcpy(accum_out, acc, len * sizeof(double));
  return FSDF_OK;
}

extern "C" int fsdf_eval(fsdf_ctx* c, const double* poses, double* cost_out, double* accum_out, int32_t* kstar_out,
                         double* d_out, double* grad_out) {
  if (!c) return FSDF_ERR_ARG;
  if (c->lm.S == 0) return fail(c, FSDF_ERR_STATE, "eval: no model (call fsdf_set_model first)");
  if (!poses) return fail(c, FSDF_ERR_ARG, "eval: poses required");
  HIPCHECK(c, hipSetDevice(c->device));
  const bool want_pp = kstar_out || d_out || grad_out;
  if (want_pp) {
    int rc = ensure_outputs(c, c->n);
    if (rc) return rc;
  }
  int rc = run_pass(c, poses, c->cur.pts.get(), c->n, c->model.accum.get(), want_pp ? c->kstar.get() : nullptr,
                    want_pp ? c->d.get() : nullptr, want_pp ? c->grad.get() : nullptr, out_perm(c), true);
  if (rc) return rc;
  return fetch(c, c->n, cost_out, accum_out, kstar_out, d_out, grad_out, want_pp);
}

// One pass over the resident cloud and the per-surface second moments of its
// residual (moments.hip), for fsdf_eval_moments and
// fsdf_value_gradient_hessian: the accumulator goes to c->h_acc (stored by the
// reduction itself, as fsdf_value_and_gradient's), the moments [S][21] to
// c->h_moments, both in flight on the context stream when this returns — the
// caller synchronises, and regroups (if it does) after this, so the moments
// read the layout the pass ran on.
// The order here is the rule of device_buffers.h made structural: (1) every
// buffer the pass's per-point outputs and the moments touch is reserved; (2)
// only then are their pointers read with get(), into locals; (3) the launches
// take those locals. No context buffer is named as an argument of a call that
// may reserve. A cloud of no points launches no moments kernel: zero moments.
// what (ctx.h): kMomentsRigid is the above and refuses other scenes;
// kMomentsAll serves any scene (fsdf_set_lm_skins) and adds the RBF skins' own
// second moments (skin_moments.hip) into c->h_skin_moments, from the same k*
// and the rows the pass read; kMomentsSkins leaves the hulls' out
// (fsdf_eval_skin_moments).
int run_pass_moments(fsdf_ctx* c, const double* poses, const char* who, int what) {
  const int S = c->lm.S;
  if (what == kMomentsRigid && (c->lm.R > 0 || c->mech.n_deform > 0))
    return fail(c, FSDF_ERR_STATE, "%s: the second moments are defined for rigid scenes (no RBF skin, no deformation)",
                who);
  const bool hulls = what != kMomentsSkins, skins = what != kMomentsRigid && c->lm.R > 0;
  if (hulls && !fsdf::moments_fit(S))
    return fail(c, FSDF_ERR_STATE, "%s: the moments table of %d surfaces (%zu bytes) does not fit %d bytes of LDS", who,
                S, (size_t)S * fsdf::kMomentsLen * sizeof(double), fsdf::kMomentsMaxLds);
  fsdf::SkinPlan plan;
  if (skins && !fsdf::skin_moments_plan(S, c->h_surface_kind.data(), c->h_n_centers.data(), &plan))
    return fail(c, FSDF_ERR_STATE, "%s: the skin moments serve skins of at most %d centres (n + 4 <= 128)", who,
                fsdf::kSkinMaxCentres);
  const int64_t n = c->n;
  const size_t mlen = (size_t)S * fsdf::kMomentsLen, slen = skins ? (size_t)plan.total : 0;
  // (1) reserve
  int rc = ensure_outputs(c, n);
  if (rc) return rc;
  rc = ensure_host_acc(c, accum_len(c));
  if (rc) return rc;
  if (hulls) {
    HIPCHECK(c, c->moments_partials.reserve(fsdf::moments_partials_len(n, S)));
    HIPCHECK(c, c->moments.reserve(mlen));
    HIPCHECK(c, c->h_moments.reserve(mlen));
  }
  if (skins) {
    HIPCHECK(c, c->skin_partials.reserve(fsdf::skin_moments_partials_len(n, plan.U)));
    HIPCHECK(c, c->skin_moments.reserve(slen));
    HIPCHECK(c, c->h_skin_moments.reserve(slen));
  }
  // (2) read the pointers
  const void* d_pts = c->cur.pts.get();
  int32_t* d_kstar = c->kstar.get();
  double* d_grad = c->grad.get();
  double* d_partials = c->moments_partials.get();
  double* d_moments = c->moments.get();
  double* h_moments = c->h_moments.get();
  double* d_skin_partials = c->skin_partials.get();
  double* d_skin_moments = c->skin_moments.get();
  double* h_skin_moments = c->h_skin_moments.get();
  double* d_acc_host = nullptr;
  HIPCHECK(c, hipHostGetDevicePointer((void**)&d_acc_host, c->h_acc.get(), 0));
  // (3) launch: the pass with k* and ∇d* in resident order (no permutation), the moments, their read-back
  rc = run_pass(c, poses, d_pts, n, d_acc_host, d_kstar, nullptr, d_grad, nullptr, true);
  if (rc) return rc;
  if (n == 0) {
    if (hulls) memset(h_moments, 0, mlen * sizeof(double));
    if (skins) memset(h_skin_moments, 0, slen * sizeof(double));
    return FSDF_OK;
  }
  if (hulls) {
    HIPCHECK(c, fsdf::launch_moments(c->precision, d_pts, d_kstar, d_grad, n, S, d_partials, d_moments, c->stream));
    HIPCHECK(c, hipMemcpyAsync(h_moments, d_moments, mlen * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  if (skins) {  // (the rows the pass just read: fsdf_set_rbf_params' last, in order on the stream)
    // (profiling: a pair of events around the skins' launches, fsdf_skin_moments_time)
    const bool prof = c->profiling && c->skin_ev_used + 2 <= c->skin_ev.size();
    if (prof) HIPCHECK(c, hipEventRecord(c->skin_ev[c->skin_ev_used], c->stream));
    HIPCHECK(c, fsdf::launch_skin_moments(c->precision, d_pts, d_kstar, c->pm.rbf_rows, n, plan, d_skin_partials,
                                          d_skin_moments, c->stream));
    if (prof) {
      HIPCHECK(c, hipEventRecord(c->skin_ev[c->skin_ev_used + 1], c->stream));
      c->skin_ev_used += 2;
    }
    HIPCHECK(c, hipMemcpyAsync(h_skin_moments, d_skin_moments, slen * sizeof(double), hipMemcpyDeviceToHost,
                               c->stream));
  }
  return FSDF_OK;
}

extern "C" int fsdf_eval_moments(fsdf_ctx* c, const double* poses, double* cost_out, double* accum_out,
                                 double* moments_out) {
  if (!c) return FSDF_ERR_ARG;
  if (c->lm.S == 0) return fail(c, FSDF_ERR_STATE, "eval_moments: no model (call fsdf_set_model first)");
  if (!poses || !moments_out) return fail(c, FSDF_ERR_ARG, "eval_moments: poses and moments_out are required");
  HIPCHECK(c, hipSetDevice(c->device));
  const int rc = run_pass_moments(c, poses, "eval_moments");
  if (rc) return rc;
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  const double* acc = c->h_acc.get();
  if (cost_out) *cost_out = acc[0];
  if (accum_out) memcpy(accum_out, acc, (size_t)accum_len(c) * sizeof(double));
  memcpy(moments_out, c->h_moments.get(), (size_t)c->lm.S * fsdf::kMomentsLen * sizeof(double));
  return FSDF_OK;
}

// fsdf_eval's pass and the second moments of the scene's RBF skins
// (skin_moments.hip), at the rows of the last fsdf_set_rbf_params.
extern "C" int fsdf_eval_skin_moments(fsdf_ctx* c, const double* poses, double* cost_out, double* accum_out,
                                      double* moments_out) {
  if (!c) return FSDF_ERR_ARG;
  if (c->lm.S == 0) return fail(c, FSDF_ERR_STATE, "eval_skin_moments: no model (call fsdf_set_surfaces first)");
  if (!poses || !moments_out) return fail(c, FSDF_ERR_ARG, "eval_skin_moments: poses and moments_out are required");
  if (c->lm.R == 0) return fail(c, FSDF_ERR_STATE, "eval_skin_moments: the scene has no RBF skin");
  HIPCHECK(c, hipSetDevice(c->device));
  const int rc = run_pass_moments(c, poses, "eval_skin_moments", kMomentsSkins);
  if (rc) return rc;
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  const double* acc = c->h_acc.get();
  if (cost_out) *cost_out = acc[0];
  if (accum_out) memcpy(accum_out, acc, (size_t)accum_len(c) * sizeof(double));
  size_t total = 0;
  for (int k = 0; k < c->lm.S; ++k)
    if (c->h_n_centers[k] > 0) total += (size_t)(4 * c->h_n_centers[k] + 4) * (size_t)(4 * c->h_n_centers[k] + 4);
  memcpy(moments_out, c->h_skin_moments.get(), total * sizeof(double));
  return FSDF_OK;
}

extern "C" int fsdf_skin_moments_time(fsdf_ctx* c, double* total_ms, int64_t* launches) {
  if (!c || !total_ms || !launches) return FSDF_ERR_ARG;
  HIPCHECK(c, hipSetDevice(c->device));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  double t = 0.0;
  for (size_t i = 0; i + 1 < c->skin_ev_used; i += 2) {
    float ms = 0.f;
    HIPCHECK(c, hipEventElapsedTime(&ms, c->skin_ev[i], c->skin_ev[i + 1]));
    t += ms;
  }
  *total_ms = t;
  *launches = (int64_t)(c->skin_ev_used / 2);
  c->skin_ev_used = 0;
  return FSDF_OK;
}

// ---- robust point losses (robust.hip, robust_impl.h) ---------------------------------
extern "C" int fsdf_set_loss(fsdf_ctx* c, int32_t kind, double scale) {
  if (!c) return FSDF_ERR_ARG;
  if (kind != FSDF_LOSS_SQUARE && kind != FSDF_LOSS_HUBER && kind != FSDF_LOSS_TUKEY)
    return fail(c, FSDF_ERR_ARG, "set_loss: unknown kind %d", kind);
  if (!fsdf::robust::valid(kind, scale))
    return fail(c, FSDF_ERR_ARG, "set_loss: the scale of a Huber or Tukey loss must be finite and > 0 (got %g)", scale);
  c->loss_kind = kind;
  c->loss_scale = kind == FSDF_LOSS_SQUARE ? 0.0 : scale;
  return FSDF_OK;
}

extern "C" int fsdf_set_loss_ref(fsdf_ctx* c, int32_t kind, const double* scale) {
  return fsdf_set_loss(c, kind, scale ? *scale : 0.0);
}

extern "C" int fsdf_get_loss(const fsdf_ctx* c, int32_t* kind_out, double* scale_out) {
  if (!c) return FSDF_ERR_ARG;
  if (kind_out) *kind_out = c->loss_kind;
  if (scale_out) *scale_out = c->loss_scale;
  return FSDF_OK;
}

// One pass over the resident cloud and the per-surface sums of the context's
// loss (robust.hip), for fsdf_eval_robust and the iteration entry points with
// a loss set: the rows go to c->h_robust, in flight on the context stream when
// this returns — the caller synchronises (and regroups, if it does, after
// this: the launch reads the layout the pass ran on), then robust_rows_finish.
// The order is run_pass_moments': (1) reserve every buffer the per-point
// outputs and the rows touch; (2) read their pointers into locals; (3) launch
// with the locals. A cloud of no points launches no robust kernel: zero rows.
// The pass's own least-squares accumulator goes to the context's device
// accumulator and is not read.
// With fsdf_set_robust_skins, scenes with RBF skins and deformations too: robust_kernel gives Σρ, Σw and
// the hull surfaces' wrenches and moments for every k*; the skins' blocks come from a launch of
// their own (robust_skin.hip) into h_robust_skin and — moments — their weighted second moments
// Σ aw j jᵀ (skin_moments.hip's factor variant) into h_skin_moments, all from the same k*, d* and
// the rows the pass read.
int run_pass_robust(fsdf_ctx* c, const double* poses, const char* who, bool moments) {
  const int S = c->lm.S;
  if ((c->lm.R > 0 || c->mech.n_deform > 0) && !c->robust_skins)
    return fail(c, FSDF_ERR_STATE, "%s: a robust loss%s serves hull-only scenes (no RBF skin, no deformation)", who,
                c->free_split >= 0 ? " or a free-space split (fsdf_set_free_split)" : "");
  const bool skins = c->lm.R > 0;
  fsdf::SkinPlan plan;
  if (skins && moments && !fsdf::skin_moments_plan(S, c->h_surface_kind.data(), c->h_n_centers.data(), &plan))
    return fail(c, FSDF_ERR_STATE, "%s: the skin moments serve skins of at most %d centres (n + 4 <= 128)", who,
                fsdf::kSkinMaxCentres);
  if (!fsdf::robust_fit(S))
    return fail(c, FSDF_ERR_STATE,
                "%s: the robust table of %d surfaces (%zu bytes) does not fit %d bytes of LDS (at most 282 surfaces)",
                who, S, (size_t)S * fsdf::kRobustLen * sizeof(double), fsdf::kRobustMaxLds);
  const int64_t n = c->n;
  const size_t rlen = (size_t)S * (moments ? fsdf::kRobustLen : fsdf::kRobustTail);
  // (1) reserve
  int rc = ensure_outputs(c, n);
  if (rc) return rc;
  HIPCHECK(c, c->robust_partials.reserve(fsdf::robust_partials_len(n, S)));
  HIPCHECK(c, c->robust_rows.reserve((size_t)S * fsdf::kRobustLen));
  HIPCHECK(c, c->h_robust.reserve((size_t)S * fsdf::kRobustLen));
  const size_t blen = skins ? (size_t)c->lm.rbf_acc : 0, slen = skins && moments ? (size_t)plan.total : 0;
  if (skins) {
    HIPCHECK(c, c->robust_skin_partials.reserve(fsdf::robust_skin_partials_len(n, c->lm.rbf_acc)));
    HIPCHECK(c, c->robust_skin_blocks.reserve(blen));
    HIPCHECK(c, c->h_robust_skin.reserve(blen));
  }
  if (slen) {
    HIPCHECK(c, c->skin_partials.reserve(fsdf::skin_moments_partials_len(n, plan.U)));
    HIPCHECK(c, c->skin_moments.reserve(slen));
    HIPCHECK(c, c->h_skin_moments.reserve(slen));
  }
  // (2) read the pointers
  const void* d_pts = c->cur.pts.get();
  int32_t* d_kstar = c->kstar.get();
  double* d_d = c->d.get();
  double* d_grad = c->grad.get();
  double* d_partials = c->robust_partials.get();
  double* d_rows = c->robust_rows.get();
  double* h_rows = c->h_robust.get();
  double* d_accum = c->model.accum.get();
  double* d_skin_bpartials = c->robust_skin_partials.get();
  double* d_skin_blocks = c->robust_skin_blocks.get();
  double* h_skin_blocks = c->h_robust_skin.get();
  double* d_skin_partials = c->skin_partials.get();
  double* d_skin_moments = c->skin_moments.get();
  double* h_skin_moments = c->h_skin_moments.get();
  // (the per-point weights in resident order, regathered when the layout changed since; null: none set)
  const double* d_conf = nullptr;
  rc = point_weights_resident(c, &d_conf);
  if (rc) return rc;
  // (3) launch: the pass with k*, d* and ∇d* in resident order (no permutation), the robust sums, their read-back
  rc = run_pass(c, poses, d_pts, n, d_accum, d_kstar, d_d, d_grad, nullptr, true);
  if (rc) return rc;
  if (n == 0) {
    HIPCHECK(c, hipStreamSynchronize(c->stream));  // (an earlier read-back into the rows)
    memset(h_rows, 0, rlen * sizeof(double));
    if (skins) memset(h_skin_blocks, 0, blen * sizeof(double));
    if (slen) memset(h_skin_moments, 0, slen * sizeof(double));
    return FSDF_OK;
  }
  // (a split: the one-sided instantiations, which read the resident→caller permutation — null: the
  // resident order is the caller's)
  HIPCHECK(c, fsdf::launch_robust(c->precision, moments, d_pts, d_kstar, d_d, d_grad, d_conf, c->cur.perm.get(),
                                  c->free_split, n, S, c->loss_kind, c->loss_scale, d_partials, d_rows, c->stream));
  HIPCHECK(c, hipMemcpyAsync(h_rows, d_rows, rlen * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (skins) {  // (the rows the pass just read: fsdf_set_rbf_params' last, in order on the stream)
    HIPCHECK(c, fsdf::launch_robust_skin(c->precision, d_pts, d_kstar, d_d, c->pm.rbf_rows, c->lm, d_conf,
                                         c->cur.perm.get(), c->free_split, n, c->loss_kind, c->loss_scale,
                                         d_skin_bpartials, d_skin_blocks, c->stream));
    HIPCHECK(c, hipMemcpyAsync(h_skin_blocks, d_skin_blocks, blen * sizeof(double), hipMemcpyDeviceToHost,
                               c->stream));
  }
  if (slen) {
    HIPCHECK(c, fsdf::launch_skin_moments_weighted(c->precision, d_pts, d_kstar, d_d, c->pm.rbf_rows, d_conf,
                                                   c->cur.perm.get(), c->free_split, c->loss_kind, c->loss_scale, n,
                                                   plan, d_skin_partials, d_skin_moments, c->stream));
    HIPCHECK(c, hipMemcpyAsync(h_skin_moments, d_skin_moments, slen * sizeof(double), hipMemcpyDeviceToHost,
                               c->stream));
  }
  return FSDF_OK;
}

// the accumulator in fsdf_eval's layout (Σρ summed in surface order from 0.0, then every surface's
// wrench) and — moments — the [S][21] moments, from the rows read back
void robust_rows_finish(fsdf_ctx* c, bool moments) {
  const int S = c->lm.S, len = moments ? fsdf::kRobustLen : fsdf::kRobustTail, m0 = len - fsdf::kRobustTail;
  const double* rows = c->h_robust.get();
  // (a rigid scene's accumulator is [1 + 6S]; a skin's wrench stays 0.0, as the pass leaves it)
  c->robust_accum.assign((size_t)accum_len(c), 0.0);
  double cost = 0.0;
  for (int k = 0; k < S; ++k) {
    const double* r = rows + (size_t)len * k;
    cost += r[m0 + 6];
    if (c->h_surface_kind[k] != FSDF_SURFACE_HULL) continue;
    for (int i = 0; i < 6; ++i) c->robust_accum[(size_t)1 + 6 * (size_t)k + i] = r[m0 + i];
  }
  c->robust_accum[0] = cost;
  if (c->lm.R > 0)
    memcpy(c->robust_accum.data() + 1 + 6 * (size_t)S, c->h_robust_skin.get(), (size_t)c->lm.rbf_acc * sizeof(double));
  if (moments) {
    c->robust_moments.resize((size_t)S * fsdf::kMomentsLen);
    for (int k = 0; k < S; ++k)
      if (c->h_surface_kind[k] == FSDF_SURFACE_HULL)
        memcpy(c->robust_moments.data() + (size_t)fsdf::kMomentsLen * k, rows + (size_t)len * k,
               fsdf::kMomentsLen * sizeof(double));
      else  // (a skin's points have no hull moments)
        memset(c->robust_moments.data() + (size_t)fsdf::kMomentsLen * k, 0, fsdf::kMomentsLen * sizeof(double));
  }
}

extern "C" int fsdf_eval_robust(fsdf_ctx* c, const double* poses, double* cost_out, double* accum_out,
                                double* moments_out, double* weight_out) {
  if (!c) return FSDF_ERR_ARG;
  if (c->lm.S == 0) return fail(c, FSDF_ERR_STATE, "eval_robust: no model (call fsdf_set_model first)");
  if (!poses) return fail(c, FSDF_ERR_ARG, "eval_robust: poses required");
  HIPCHECK(c, hipSetDevice(c->device));
  if (c->lm.R > 0)
    return fail(c, FSDF_ERR_STATE, "eval_robust: hull-only scenes (the scene has an RBF skin)%s",
                c->free_split >= 0 ? "; a free-space split is set (fsdf_set_free_split)" : "");
  const bool moments = moments_out != nullptr;
  const int rc = run_pass_robust(c, poses, "eval_robust", moments);
  if (rc) return rc;
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  robust_rows_finish(c, moments);
  const int S = c->lm.S, len = moments ? fsdf::kRobustLen : fsdf::kRobustTail;
  if (cost_out) *cost_out = c->robust_accum[0];
  if (accum_out) memcpy(accum_out, c->robust_accum.data(), c->robust_accum.size() * sizeof(double));
  if (moments) memcpy(moments_out, c->robust_moments.data(), c->robust_moments.size() * sizeof(double));
  if (weight_out)
    for (int k = 0; k < S; ++k) weight_out[k] = c->h_robust.get()[(size_t)len * k + len - 1];
  return FSDF_OK;
}

// fsdf_eval_robust without its synchronisation and read-back: the pass, the
// robust launch and the rows' assembly on the device (robust.hip
// robust_assemble_kernel: robust_rows_finish's arithmetic) into the caller's
// device buffers, all in order on the context stream. The order is
// run_pass_robust's: reserve, read the pointers, launch. A cloud of no points
// launches no robust kernel: zeros.
extern "C" int fsdf_eval_robust_device(fsdf_ctx* c, const double* poses, double* d_accum, double* d_moments) {
  if (!c) return FSDF_ERR_ARG;
  if (c->lm.S == 0) return fail(c, FSDF_ERR_STATE, "eval_robust_device: no model (call fsdf_set_model first)");
  if (!poses || !d_accum) return fail(c, FSDF_ERR_ARG, "eval_robust_device: poses and d_accum are required");
  HIPCHECK(c, hipSetDevice(c->device));
  if (c->lm.R > 0 || c->mech.n_deform > 0)
    return fail(c, FSDF_ERR_STATE, "eval_robust_device: hull-only scenes (the scene has an RBF skin or a deformation)%s",
                c->free_split >= 0 ? "; a free-space split is set (fsdf_set_free_split)" : "");
  const int S = c->lm.S;
  if (!fsdf::robust_fit(S))
    return fail(c, FSDF_ERR_STATE,
                "eval_robust_device: the robust table of %d surfaces (%zu bytes) does not fit %d bytes of LDS (at most "
                "282 surfaces)", S, (size_t)S * fsdf::kRobustLen * sizeof(double), fsdf::kRobustMaxLds);
  const bool moments = d_moments != nullptr;
  const int64_t n = c->n;
  // (1) reserve
  int rc = ensure_outputs(c, n);
  if (rc) return rc;
  HIPCHECK(c, c->robust_partials.reserve(fsdf::robust_partials_len(n, S)));
  HIPCHECK(c, c->robust_rows.reserve((size_t)S * fsdf::kRobustLen));
  // (2) read the pointers
  const void* d_pts = c->cur.pts.get();
  int32_t* d_kstar = c->kstar.get();
  double* d_d = c->d.get();
  double* d_grad = c->grad.get();
  double* d_partials = c->robust_partials.get();
  double* d_rows = c->robust_rows.get();
  double* d_ls = c->model.accum.get();  // (the pass's own least-squares accumulator: not read)
  const double* d_conf = nullptr;
  rc = point_weights_resident(c, &d_conf);
  if (rc) return rc;
  // (3) launch
  rc = run_pass(c, poses, d_pts, n, d_ls, d_kstar, d_d, d_grad, nullptr, true);
  if (rc) return rc;
  if (n == 0) {
    HIPCHECK(c, hipMemsetAsync(d_accum, 0, ((size_t)1 + 6 * (size_t)S) * sizeof(double), c->stream));
    if (moments) HIPCHECK(c, hipMemsetAsync(d_moments, 0, (size_t)S * fsdf::kMomentsLen * sizeof(double), c->stream));
    return FSDF_OK;
  }
  HIPCHECK(c, fsdf::launch_robust(c->precision, moments, d_pts, d_kstar, d_d, d_grad, d_conf, c->cur.perm.get(),
                                  c->free_split, n, S, c->loss_kind, c->loss_scale, d_partials, d_rows, c->stream));
  HIPCHECK(c, fsdf::launch_robust_assemble(moments, d_rows, c->lm.surface_kind, S, d_accum, d_moments, c->stream));
  return FSDF_OK;
}

// ---- the device solver loops on a robust objective (descend.hip) --------------------------
extern "C" int fsdf_set_robust_loops(fsdf_ctx* c, int32_t enable) {
  if (!c) return FSDF_ERR_ARG;
  if (enable != 0 && enable != 1) return fail(c, FSDF_ERR_ARG, "set_robust_loops: enable %d", enable);
  c->robust_loops = enable;
  return FSDF_OK;
}

extern "C" int fsdf_get_robust_loops(const fsdf_ctx* c, int32_t* enable_out) {
  if (!c || !enable_out) return FSDF_ERR_ARG;
  *enable_out = c->robust_loops;
  return FSDF_OK;
}

// ---- robust objectives on RBF skins and deformations (robust_skin.hip) --------------------
extern "C" int fsdf_set_robust_skins(fsdf_ctx* c, int32_t enable) {
  if (!c) return FSDF_ERR_ARG;
  if (enable != 0 && enable != 1) return fail(c, FSDF_ERR_ARG, "set_robust_skins: enable %d", enable);
  c->robust_skins = enable;
  return FSDF_OK;
}

extern "C" int fsdf_get_robust_skins(const fsdf_ctx* c, int32_t* enable_out) {
  if (!c || !enable_out) return FSDF_ERR_ARG;
  *enable_out = c->robust_skins;
  return FSDF_OK;
}

extern "C" int fsdf_eval_robust_skins(fsdf_ctx* c, const double* poses, double* cost_out, double* accum_out,
                                      double* moments_out, double* skin_moments_out, double* weight_out) {
  if (!c) return FSDF_ERR_ARG;
  if (c->lm.S == 0) return fail(c, FSDF_ERR_STATE, "eval_robust_skins: no model (call fsdf_set_surfaces first)");
  if (!poses) return fail(c, FSDF_ERR_ARG, "eval_robust_skins: poses required");
  if (!c->robust_skins)
    return fail(c, FSDF_ERR_STATE, "eval_robust_skins: robust objectives on skins are off (fsdf_set_robust_skins)");
  HIPCHECK(c, hipSetDevice(c->device));
  const bool moments = moments_out != nullptr || skin_moments_out != nullptr;
  const int rc = run_pass_robust(c, poses, "eval_robust_skins", moments);
  if (rc) return rc;
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  robust_rows_finish(c, moments);
  const int S = c->lm.S, len = moments ? fsdf::kRobustLen : fsdf::kRobustTail;
  if (cost_out) *cost_out = c->robust_accum[0];
  if (accum_out) memcpy(accum_out, c->robust_accum.data(), c->robust_accum.size() * sizeof(double));
  if (moments_out) memcpy(moments_out, c->robust_moments.data(), c->robust_moments.size() * sizeof(double));
  if (skin_moments_out && c->lm.R > 0) {
    size_t total = 0;
    for (int k = 0; k < S; ++k)
      if (c->h_n_centers[k] > 0) total += (size_t)(4 * c->h_n_centers[k] + 4) * (size_t)(4 * c->h_n_centers[k] + 4);
    memcpy(skin_moments_out, c->h_skin_moments.get(), total * sizeof(double));
  }
  if (weight_out)
    for (int k = 0; k < S; ++k) weight_out[k] = c->h_robust.get()[(size_t)len * k + len - 1];
  return FSDF_OK;
}
