// score_api.hip — the context side of scoring candidate states
// (include/flashsdf.h "scoring candidate states"; kernels: score.hip):
// fsdf_score_poses, fsdf_score_states, fsdf_score_time.
//
// A call is read-only on the context: it uses buffers of its own (ctx.h
// score_*), reads the resident cloud, its chunk spheres, permutation, weights
// and split, and the loss — and writes none of them, nor the seeds, the plan,
// the block orders, the regroup state or the posed model of the passes. The
// mechanism's scratch is left alone too: fsdf_score_states runs the forward
// kinematics into vectors of its own.
//
// The batch's posed tables can be large (several hundred candidates of a
// 64-hull model: tens of megabytes), so the batch is walked in slices of
// kScoreSliceBytes of tables (the environment variable FSDF_SCORE_SLICE_BYTES
// overrides the budget; at least one candidate per slice). A candidate's bits
// do not depend on the slicing (score.hip).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "ctx.h"
#include "kin_impl.h"
#include "robust_impl.h"

static constexpr size_t kScoreSliceBytes = (size_t)64 << 20;
static constexpr int kScoreMaxSlice = 65535;  // (grid.y)
static constexpr size_t kScoreEvents = 2 * 256;

static size_t slice_budget() {
  const char* e = getenv("FSDF_SCORE_SLICE_BYTES");
  if (!e || !*e) return kScoreSliceBytes;
  char* end = nullptr;
  const unsigned long long v = strtoull(e, &end, 10);
  return (end && *end == 0 && v > 0) ? (size_t)v : kScoreSliceBytes;
}

// the checks the two entry points share, after their argument checks
static int score_ready(fsdf_ctx* c, const char* who) {
  if (c->lm.S == 0) return fail(c, FSDF_ERR_STATE, "%s: no model (call fsdf_set_model first)", who);
  if (c->lm.R > 0 || c->mech.n_deform > 0)
    return fail(c, FSDF_ERR_STATE, "%s: scoring serves hull-only rigid scenes (no RBF skin, no deformation)", who);
  if (!fsdf::score_fits(c->lm))
    return fail(c, FSDF_ERR_STATE, "%s: the scene's hull table and stages do not fit a workgroup's LDS", who);
  if (!c->cur.pts.get()) return fail(c, FSDF_ERR_STATE, "%s: no cloud (call fsdf_set_points first)", who);
  if (c->ranged)
    return fail(c, FSDF_ERR_STATE, "%s: scoring serves a whole resident cloud (not a ranged or keyed one)", who);
  if (c->prefetch_n >= 0 || c->prefetch_deferred)
    return fail(c, FSDF_ERR_STATE, "%s: a prefetched cloud is pending (call fsdf_set_points_prefetched first)", who);
  return FSDF_OK;
}

// poses [B][S][12] (host), every check passed -> cost_out [B]
static int score_poses_impl(fsdf_ctx* c, const double* poses, int32_t B, double* cost_out, const char* who) {
  const int S = c->lm.S;
  const int64_t n = c->n;
  if (n == 0) {  // an empty cloud: exact zeros
    for (int32_t b = 0; b < B; ++b) cost_out[b] = 0.0;
    return FSDF_OK;
  }
  HIPCHECK(c, hipSetDevice(c->device));
  // (earlier work on the stream: a growing reserve below frees what a queued launch may read — the
  // weights' gather among them; and the scoring buffers' last users are done)
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  // the candidates whose poses are finite go to the device, in order; the others' cost is NaN
  const size_t plen = (size_t)12 * S;
  HIPCHECK(c, c->h_score_poses.reserve((size_t)B * plen));
  std::vector<int32_t> where((size_t)B);
  int32_t Bf = 0;
  for (int32_t b = 0; b < B; ++b) {
    const double* P = poses + (size_t)b * plen;
    bool finite = true;
    for (size_t i = 0; i < plen && finite; ++i) finite = std::isfinite(P[i]);
    where[(size_t)b] = finite ? Bf : -1;
    if (finite) memcpy(c->h_score_poses.get() + (size_t)Bf++ * plen, P, plen * sizeof(double));
  }
  if (Bf > 0) {
    const fsdf::ScoreTable t = fsdf::score_table(c->precision, c->lm);
    const int groups = fsdf::score_groups(n);
    const int slice =
        (int)std::min<size_t>(std::max<size_t>(slice_budget() / t.stride, 1), (size_t)std::min(Bf, kScoreMaxSlice));
    // (1) reserve, (2) read the pointers, (3) launch (device_buffers.h)
    HIPCHECK(c, c->score_poses.reserve((size_t)Bf * plen));
    HIPCHECK(c, c->score_tables.reserve((size_t)slice * t.stride));
    HIPCHECK(c, c->score_partials.reserve((size_t)slice * groups));
    HIPCHECK(c, c->score_cost.reserve((size_t)Bf));
    HIPCHECK(c, c->h_score_cost.reserve((size_t)Bf));
    const bool prof = c->profiling;
    if (prof && c->score_ev.empty()) {
      c->score_ev.resize(kScoreEvents);
      for (auto& e : c->score_ev) HIPCHECK(c, e.create(hipEventDisableSystemFence));
    }
    const bool stamp = prof && c->score_ev_used + 2 <= c->score_ev.size();
    const double* d_conf = nullptr;
    const int rc = point_weights_resident(c, &d_conf);  // (regathers stale weights, as any robust launch would)
    if (rc) return rc;
    double* d_poses = c->score_poses.get();
    unsigned char* d_tables = c->score_tables.get();
    double* d_partials = c->score_partials.get();
    double* d_cost = c->score_cost.get();
    double* h_cost = c->h_score_cost.get();
    HIPCHECK(c, hipMemcpyAsync(d_poses, c->h_score_poses.get(), (size_t)Bf * plen * sizeof(double),
                               hipMemcpyHostToDevice, c->stream));
    if (stamp) HIPCHECK(c, hipEventRecord(c->score_ev[c->score_ev_used], c->stream));
    for (int32_t b0 = 0; b0 < Bf; b0 += slice) {
      const int nb = std::min<int32_t>(slice, Bf - b0);
      HIPCHECK(c, fsdf::launch_score_pose(c->precision, c->lm, d_poses + (size_t)b0 * plen, nb, d_tables, c->stream));
      HIPCHECK(c, fsdf::launch_score(c->precision, c->cull != 0, c->lm, d_tables, c->cur.pts.get(), n, nb,
                                     c->cur.chunk_ws.get(), d_conf, c->cur.perm.get(), c->free_split, c->loss_kind,
                                     c->loss_scale, d_partials, d_cost + b0, c->stream));
    }
    if (stamp) {
      HIPCHECK(c, hipEventRecord(c->score_ev[c->score_ev_used + 1], c->stream));
      c->score_ev_used += 2;
    }
    HIPCHECK(c, hipMemcpyAsync(h_cost, d_cost, (size_t)Bf * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHECK(c, hipStreamSynchronize(c->stream));
  }
  for (int32_t b = 0; b < B; ++b)
    cost_out[b] = where[(size_t)b] >= 0 ? c->h_score_cost.get()[where[(size_t)b]]
                                        : std::numeric_limits<double>::quiet_NaN();
  (void)who;
  return FSDF_OK;
}

extern "C" int fsdf_score_poses(fsdf_ctx* c, const double* poses, int32_t B, double* cost_out) {
  if (!c) return FSDF_ERR_ARG;
  if (B < 0) return fail(c, FSDF_ERR_ARG, "score_poses: B = %d", B);
  if (B == 0) return FSDF_OK;
  if (!poses || !cost_out) return fail(c, FSDF_ERR_ARG, "score_poses: null argument");
  const int rc = score_ready(c, "score_poses");
  if (rc) return rc;
  return score_poses_impl(c, poses, B, cost_out, "score_poses");
}

extern "C" int fsdf_score_states(fsdf_ctx* c, const double* x, int32_t B, double* cost_out) {
  if (!c) return FSDF_ERR_ARG;
  if (B < 0) return fail(c, FSDF_ERR_ARG, "score_states: B = %d", B);
  if (B == 0) return FSDF_OK;
  if (!x || !cost_out) return fail(c, FSDF_ERR_ARG, "score_states: null argument");
  const auto& M = c->mech;
  if (M.nb == 0) return fail(c, FSDF_ERR_STATE, "score_states: no mechanism (call fsdf_set_mechanism)");
  int rc = score_ready(c, "score_states");
  if (rc) return rc;
  const int S = c->lm.S;
  if ((int)M.surface_body.size() != S)
    return fail(c, FSDF_ERR_STATE, "score_states: mechanism registered for another surface list (call fsdf_set_mechanism)");
  // forward kinematics and surface poses per candidate (iteration_prepare's rigid part, quaternion
  // blocks normalised inside), into vectors of this call: the mechanism's scratch and its record of
  // prepared states stay as they are
  const size_t nb = (size_t)M.nb;
  std::vector<double> R(9 * nb), t(3 * nb), Rb(9 * nb), tb(3 * nb), poses((size_t)B * 12 * S);
  for (int32_t b = 0; b < B; ++b) {
    rc = fsdf_tree_transforms(M.nb, M.parent.data(), M.kind.data(), M.qoff.data(), M.axis.data(), M.AR.data(),
                              M.At.data(), M.BR.data(), M.Bt.data(), x + (size_t)b * M.nq, R.data(), t.data(),
                              Rb.data(), tb.data());
    if (rc) return fail(c, rc, "score_states: forward kinematics of candidate %d (bad configuration)", b);
    for (int k = 0; k < S; ++k) {
      double* P = poses.data() + ((size_t)b * S + k) * 12;
      const int body = M.surface_body[k];
      if (body < 0) {
        for (int i = 0; i < 12; ++i) P[i] = (i % 4 == 0 && i < 9) ? 1.0 : 0.0;
        continue;
      }
      fsdf::kin::surface_pose(R.data() + 9 * body, t.data() + 3 * body, M.frame_R.data() + 9 * k,
                              M.frame_t.data() + 3 * k, P);
    }
  }
  return score_poses_impl(c, poses.data(), B, cost_out, "score_states");
}

extern "C" int fsdf_score_time(fsdf_ctx* c, double* total_ms, int64_t* launches) {
  if (!c || !total_ms || !launches) return FSDF_ERR_ARG;
  HIPCHECK(c, hipSetDevice(c->device));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  double t = 0.0;
  for (size_t i = 0; i + 1 < c->score_ev_used; i += 2) {
    float ms = 0.f;
    HIPCHECK(c, hipEventElapsedTime(&ms, c->score_ev[i], c->score_ev[i + 1]));
    t += ms;
  }
  *total_ms = t;
  *launches = (int64_t)(c->score_ev_used / 2);
  c->score_ev_used = 0;
  return FSDF_OK;
}
