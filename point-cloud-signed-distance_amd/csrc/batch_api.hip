// batch_api.hip — the context side of the gradients and Gauss-Newton moments
// of many candidate states (include/flashsdf.h "gradients of candidate states";
// kernels: batch.hip): fsdf_batch_robust_poses, fsdf_batch_states, the lockstep
// solver loops fsdf_descend_lm_batch and fsdf_descend_batch (and their _ref forms), fsdf_batch_time.
//
// A call is read-only on the context, as the scoring calls are (score_api.hip):
// it uses buffers of its own (ctx.h batch_*), reads the resident cloud, its chunk
// spheres, permutation, weights and split, and the loss — and writes none of
// them, nor the seeds, the plan, the block orders, the regroup state, the posed
// model of the passes, the mechanism's scratch or its record of prepared states:
// the forward kinematics, the chain rule and the Gauss-Newton matrix run on
// vectors of the call.
//
// A candidate costs its posed table, its per-point block (36 B a point), its
// partials and its rows, so the batch is walked in slices of kBatchSliceBytes of
// them (the environment variable FSDF_BATCH_SLICE_BYTES overrides the budget; at
// least one candidate per slice). A candidate's bits do not depend on the
// slicing (batch.hip).
//
// The loops are host loops around one batched evaluation per round — the
// candidates still running, compacted in ascending index order — and apply
// fsdf_lm_minimize's (gauss_newton.cpp) and fsdf_descend's host loop's
// (descend.hip) statements per candidate: one synchronisation per round for the
// whole batch.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "ctx.h"
#include "kin_impl.h"
#include "robust_impl.h"

static constexpr size_t kBatchSliceBytes = (size_t)256 << 20;
static constexpr int kBatchMaxSlice = 65535;  // (grid.y)
static constexpr size_t kBatchEvents = 2 * 256;

static size_t batch_slice_budget() {
  const char* e = getenv("FSDF_BATCH_SLICE_BYTES");
  if (!e || !*e) return kBatchSliceBytes;
  char* end = nullptr;
  const unsigned long long v = strtoull(e, &end, 10);
  return (end && *end == 0 && v > 0) ? (size_t)v : kBatchSliceBytes;
}

// the checks the entry points share, after their argument checks (the scoring calls', and the
// robust table's)
static int batch_ready(fsdf_ctx* c, const char* who) {
  if (c->lm.S == 0) return fail(c, FSDF_ERR_STATE, "%s: no model (call fsdf_set_model first)", who);
  if (c->lm.R > 0 || c->mech.n_deform > 0)
    return fail(c, FSDF_ERR_STATE, "%s: the batched calls serve hull-only rigid scenes (no RBF skin, no deformation)",
                who);
  if (!fsdf::score_fits(c->lm))
    return fail(c, FSDF_ERR_STATE, "%s: the scene's hull table and stages do not fit a workgroup's LDS", who);
  if (!fsdf::robust_fit(c->lm.S))
    return fail(c, FSDF_ERR_STATE, "%s: the robust table of %d surfaces does not fit %d bytes of LDS", who, c->lm.S,
                fsdf::kRobustMaxLds);
  if (!c->cur.pts.get()) return fail(c, FSDF_ERR_STATE, "%s: no cloud (call fsdf_set_points first)", who);
  if (c->ranged)
    return fail(c, FSDF_ERR_STATE, "%s: the batched calls serve a whole resident cloud (not a ranged or keyed one)",
                who);
  if (c->prefetch_n >= 0 || c->prefetch_deferred)
    return fail(c, FSDF_ERR_STATE, "%s: a prefetched cloud is pending (call fsdf_set_points_prefetched first)", who);
  return FSDF_OK;
}

// where[b] = 0 where every entry of candidate b's poses [S][12] is finite, -1 elsewhere
static void finite_candidates(const double* poses, int32_t B, size_t plen, std::vector<int32_t>& where) {
  where.assign((size_t)B, 0);
  for (int32_t b = 0; b < B; ++b)
    for (size_t i = 0; i < plen; ++i)
      if (!std::isfinite(poses[(size_t)b * plen + i])) {
        where[(size_t)b] = -1;
        break;
      }
}

// poses [B][S][12] (host), every check passed, n > 0 -> the candidates' rows in c->h_batch_rows:
// where[b] >= 0: candidate b's rows are rows where[b] (of S · 29 or S · 8 doubles), -1: a pose of
// b's is not finite (no rows)
static int batch_rows(fsdf_ctx* c, const double* poses, int32_t B, bool moments, std::vector<int32_t>& where) {
  const int S = c->lm.S;
  const int64_t n = c->n;
  HIPCHECK(c, hipSetDevice(c->device));
  // (earlier work on the stream: a growing reserve below frees what a queued launch may read — the
  // weights' gather among them; and these buffers' last users are done)
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  const size_t plen = (size_t)12 * S;
  HIPCHECK(c, c->h_batch_poses.reserve((size_t)B * plen));
  where.assign((size_t)B, -1);
  int32_t Bf = 0;
  for (int32_t b = 0; b < B; ++b) {
    const double* P = poses + (size_t)b * plen;
    bool finite = true;
    for (size_t i = 0; i < plen && finite; ++i) finite = std::isfinite(P[i]);
    if (!finite) continue;
    where[(size_t)b] = Bf;
    memcpy(c->h_batch_poses.get() + (size_t)Bf++ * plen, P, plen * sizeof(double));
  }
  if (Bf == 0) return FSDF_OK;
  const fsdf::ScoreTable t = fsdf::score_table(c->precision, c->lm);
  const size_t rlen = (size_t)S * (moments ? fsdf::kRobustLen : fsdf::kRobustTail);
  const size_t np = fsdf::batch_point_stride(n), parts = fsdf::robust_partials_len(n, S);
  // a candidate's share of the slice budget: table, per-point block, partials, rows
  const size_t per = t.stride + fsdf::kBatchPointBytes * np + (parts + (size_t)S * fsdf::kRobustLen) * sizeof(double);
  const int slice =
      (int)std::min<size_t>(std::max<size_t>(batch_slice_budget() / per, 1), (size_t)std::min(Bf, kBatchMaxSlice));
  // (1) reserve, (2) read the pointers, (3) launch (device_buffers.h)
  HIPCHECK(c, c->batch_poses.reserve((size_t)Bf * plen));
  HIPCHECK(c, c->batch_tables.reserve((size_t)slice * t.stride));
  HIPCHECK(c, c->batch_points.reserve((size_t)slice * fsdf::kBatchPointBytes * np));
  HIPCHECK(c, c->batch_partials.reserve((size_t)slice * parts));
  HIPCHECK(c, c->batch_rows.reserve((size_t)Bf * rlen));
  HIPCHECK(c, c->h_batch_rows.reserve((size_t)Bf * rlen));
  const bool prof = c->profiling;
  if (prof && c->batch_ev.empty()) {
    c->batch_ev.resize(kBatchEvents);
    for (auto& e : c->batch_ev) HIPCHECK(c, e.create(hipEventDisableSystemFence));
  }
  const double* d_conf = nullptr;
  const int rc = point_weights_resident(c, &d_conf);  // (regathers stale weights, as any robust launch would)
  if (rc) return rc;
  double* d_poses = c->batch_poses.get();
  unsigned char* d_tables = c->batch_tables.get();
  unsigned char* d_points = c->batch_points.get();
  double* d_partials = c->batch_partials.get();
  double* d_rows = c->batch_rows.get();
  double* h_rows = c->h_batch_rows.get();
  HIPCHECK(c, hipMemcpyAsync(d_poses, c->h_batch_poses.get(), (size_t)Bf * plen * sizeof(double),
                             hipMemcpyHostToDevice, c->stream));
  for (int32_t b0 = 0; b0 < Bf; b0 += slice) {
    const int nb = std::min<int32_t>(slice, Bf - b0);
    // (profiling: a pair of events around every slice's launches — fsdf_batch_time counts slices)
    const bool stamp = prof && c->batch_ev_used + 2 <= c->batch_ev.size();
    if (stamp) HIPCHECK(c, hipEventRecord(c->batch_ev[c->batch_ev_used], c->stream));
    HIPCHECK(c, fsdf::launch_score_pose(c->precision, c->lm, d_poses + (size_t)b0 * plen, nb, d_tables, c->stream));
    HIPCHECK(c, fsdf::launch_batch_eval(c->precision, c->cull != 0, c->lm, d_tables, c->cur.pts.get(), n, nb,
                                        c->cur.chunk_ws.get(), d_points, c->stream));
    HIPCHECK(c, fsdf::launch_batch_robust(c->precision, moments, c->cur.pts.get(), d_points, d_conf, c->cur.perm.get(),
                                          c->free_split, n, S, nb, c->loss_kind, c->loss_scale, d_partials,
                                          d_rows + (size_t)b0 * rlen, c->stream));
    if (stamp) {
      HIPCHECK(c, hipEventRecord(c->batch_ev[c->batch_ev_used + 1], c->stream));
      c->batch_ev_used += 2;
    }
  }
  HIPCHECK(c, hipMemcpyAsync(h_rows, d_rows, (size_t)Bf * rlen * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  return FSDF_OK;
}

// robust_rows_finish's (pass.hip) arithmetic on one candidate's rows: accum [1 + 6S] (Σρ summed in
// surface order from 0.0, then every hull surface's wrench), moments [S][21] (null: none)
static void batch_assemble(const fsdf_ctx* c, const double* rows, bool moments, double* accum, double* mom) {
  const int S = c->lm.S, len = moments ? fsdf::kRobustLen : fsdf::kRobustTail, m0 = len - fsdf::kRobustTail;
  for (int i = 0; i < 1 + 6 * S; ++i) accum[i] = 0.0;
  double cost = 0.0;
  for (int k = 0; k < S; ++k) {
    const double* r = rows + (size_t)len * k;
    cost += r[m0 + 6];
    if (c->h_surface_kind[k] != FSDF_SURFACE_HULL) continue;
    for (int i = 0; i < 6; ++i) accum[(size_t)1 + 6 * (size_t)k + i] = r[m0 + i];
  }
  accum[0] = cost;
  if (!moments || !mom) return;
  for (int k = 0; k < S; ++k) {
    if (c->h_surface_kind[k] == FSDF_SURFACE_HULL)
      memcpy(mom + (size_t)fsdf::kMomentsLen * k, rows + (size_t)len * k, fsdf::kMomentsLen * sizeof(double));
    else
      memset(mom + (size_t)fsdf::kMomentsLen * k, 0, fsdf::kMomentsLen * sizeof(double));
  }
}

extern "C" int fsdf_batch_robust_poses(fsdf_ctx* c, const double* poses, int32_t B, double* accum_out,
                                       double* moments_out, double* weight_out) {
  if (!c) return FSDF_ERR_ARG;
  if (B < 0) return fail(c, FSDF_ERR_ARG, "batch_robust_poses: B = %d", B);
  if (B == 0) return FSDF_OK;
  if (!poses || !accum_out) return fail(c, FSDF_ERR_ARG, "batch_robust_poses: null argument");
  int rc = batch_ready(c, "batch_robust_poses");
  if (rc) return rc;
  const int S = c->lm.S;
  const size_t alen = (size_t)1 + 6 * (size_t)S, mlen = (size_t)S * fsdf::kMomentsLen;
  const bool moments = moments_out != nullptr;
  const int len = moments ? fsdf::kRobustLen : fsdf::kRobustTail;
  std::vector<int32_t> where;
  std::vector<double> zero_rows;
  if (c->n == 0) {  // an empty cloud: exact zeros (a non-finite candidate still gets its NaNs)
    finite_candidates(poses, B, (size_t)12 * S, where);
    zero_rows.assign((size_t)S * len, 0.0);
  } else {
    rc = batch_rows(c, poses, B, moments, where);
    if (rc) return rc;
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int32_t b = 0; b < B; ++b) {
    double* a = accum_out + (size_t)b * alen;
    double* m = moments ? moments_out + (size_t)b * mlen : nullptr;
    double* w = weight_out ? weight_out + (size_t)b * S : nullptr;
    if (where[(size_t)b] < 0) {  // a non-finite pose: NaN outputs
      for (size_t i = 0; i < alen; ++i) a[i] = nan;
      if (m)
        for (size_t i = 0; i < mlen; ++i) m[i] = nan;
      if (w)
        for (int k = 0; k < S; ++k) w[k] = nan;
      continue;
    }
    const double* rows = c->n == 0 ? zero_rows.data() : c->h_batch_rows.get() + (size_t)where[(size_t)b] * S * len;
    batch_assemble(c, rows, moments, a, m);
    if (w)
      for (int k = 0; k < S; ++k) w[k] = rows[(size_t)len * k + len - 1];
  }
  return FSDF_OK;
}

// fsdf_batch_states after its argument checks: per candidate the forward kinematics and surface
// poses of fsdf_score_states, the rows, then robust_iteration's (iterate.hip) host half — the
// accumulator's chain rule (iteration_finish's rigid statements) and, hess_out given, the
// Gauss-Newton matrix with its factor 2 — on vectors of this call
static int batch_states(fsdf_ctx* c, const double* x, int32_t B, double* cost_out, double* grad_out, double* hess_out,
                        const char* who) {
  const auto& M = c->mech;
  if (M.nb == 0) return fail(c, FSDF_ERR_STATE, "%s: no mechanism (call fsdf_set_mechanism)", who);
  int rc = batch_ready(c, who);
  if (rc) return rc;
  const int S = c->lm.S, nq = M.nq;
  if ((int)M.surface_body.size() != S)
    return fail(c, FSDF_ERR_STATE, "%s: mechanism registered for another surface list (call fsdf_set_mechanism)", who);
  const size_t nb = (size_t)M.nb;
  std::vector<double> R(9 * nb), t(3 * nb), Rb((size_t)B * 9 * nb), tb((size_t)B * 3 * nb),
      poses((size_t)B * 12 * S);
  for (int32_t b = 0; b < B; ++b) {
    rc = fsdf_tree_transforms(M.nb, M.parent.data(), M.kind.data(), M.qoff.data(), M.axis.data(), M.AR.data(),
                              M.At.data(), M.BR.data(), M.Bt.data(), x + (size_t)b * nq, R.data(), t.data(),
                              Rb.data() + (size_t)b * 9 * nb, tb.data() + (size_t)b * 3 * nb);
    if (rc) return fail(c, rc, "%s: forward kinematics of candidate %d (bad configuration)", who, b);
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
  const bool moments = hess_out != nullptr;
  const int len = moments ? fsdf::kRobustLen : fsdf::kRobustTail;
  const size_t rlen = (size_t)S * len;
  std::vector<int32_t> where((size_t)B, 0);
  std::vector<double> zero_rows;
  if (c->n == 0) {  // (an empty cloud: zero rows, the same host half; a non-finite candidate still gets its NaNs)
    finite_candidates(poses.data(), B, (size_t)12 * S, where);
    zero_rows.assign(rlen, 0.0);
  } else {
    rc = batch_rows(c, poses.data(), B, moments, where);
    if (rc) return rc;
  }
  std::vector<double> accum((size_t)1 + 6 * (size_t)S), mom(moments ? (size_t)S * fsdf::kMomentsLen : 0),
      work(6 * nb), gn_work(moments ? (size_t)36 * nb + (size_t)6 * nq : 0);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int32_t b = 0; b < B; ++b) {
    double* g = grad_out + (size_t)b * nq;
    double* H = moments ? hess_out + (size_t)b * nq * nq : nullptr;
    if (where[(size_t)b] < 0) {  // a non-finite pose: NaN outputs
      cost_out[b] = nan;
      for (int i = 0; i < nq; ++i) g[i] = nan;
      if (H)
        for (size_t i = 0; i < (size_t)nq * nq; ++i) H[i] = nan;
      continue;
    }
    const double* rows = c->n == 0 ? zero_rows.data() : c->h_batch_rows.get() + (size_t)where[(size_t)b] * rlen;
    batch_assemble(c, rows, moments, accum.data(), moments ? mom.data() : nullptr);
    const double* xb = x + (size_t)b * nq;
    const double* Rbb = Rb.data() + (size_t)b * 9 * nb;
    const double* tbb = tb.data() + (size_t)b * 3 * nb;
    for (int i = 0; i < nq; ++i) g[i] = 0.0;
    rc = fsdf_config_gradient(M.nb, M.parent.data(), M.kind.data(), M.qoff.data(), M.axis.data(), Rbb, tbb, xb, S,
                              M.surface_body.data(), accum.data() + 1, nullptr, work.data(), g);
    if (rc) return fail(c, rc, "%s: chain rule of candidate %d", who, b);
    const double reg = 0.0;  // (no deformation: iteration_finish's regulariser sum is empty)
    cost_out[b] = accum[0] + M.weight * reg;
    if (!H) continue;
    rc = fsdf_gauss_newton_matrix(M.nb, M.parent.data(), M.kind.data(), M.qoff.data(), M.axis.data(), Rbb, tbb, xb, S,
                                  M.surface_body.data(), mom.data(), nq, gn_work.data(), H);
    if (rc) return fail(c, rc, "%s: Gauss-Newton matrix of candidate %d", who, b);
    for (size_t i = 0; i < (size_t)nq * nq; ++i) H[i] = 2.0 * H[i];
  }
  return FSDF_OK;
}

extern "C" int fsdf_batch_states(fsdf_ctx* c, const double* x, int32_t B, double* cost_out, double* grad_out,
                                 double* hess_out) {
  if (!c) return FSDF_ERR_ARG;
  if (B < 0) return fail(c, FSDF_ERR_ARG, "batch_states: B = %d", B);
  if (B == 0) return FSDF_OK;
  if (!x || !cost_out || !grad_out) return fail(c, FSDF_ERR_ARG, "batch_states: null argument");
  return batch_states(c, x, B, cost_out, grad_out, hess_out, "batch_states");
}

// the opening checks of the two loops (descend_checks', descend.hip)
static int batch_loop_checks(fsdf_ctx* c, const char* who, const double* x, int32_t B, int32_t iteration_limit,
                             double gain, double max_step, double n_points) {
  if (B < 0) return fail(c, FSDF_ERR_ARG, "%s: B = %d", who, B);
  if (B == 0) return FSDF_OK;
  if (!x || iteration_limit < 0 || !(n_points > 0.0) || !std::isfinite(gain) || !(max_step >= 0.0))
    return fail(c, FSDF_ERR_ARG, "%s: bad arguments", who);
  if (c->mech.nb == 0) return fail(c, FSDF_ERR_STATE, "%s: no mechanism (call fsdf_set_mechanism)", who);
  return batch_ready(c, who);
}

// fsdf_lm_minimize (gauss_newton.cpp) for B candidates in lockstep, statement for statement per
// candidate, over fsdf_descend_lm's wrapped objective (lm_objective, descend.hip: ÷ n_points, the
// prior of fsdf_set_lm_prior about each candidate's own start): a round advances every running
// candidate to its next evaluation — the end conditions, the damped step, the raises of a
// degenerate factorisation — and then evaluates the trials of all of them in one fsdf_batch_states
extern "C" int fsdf_descend_lm_batch(fsdf_ctx* c, double* x, int32_t B, int32_t iteration_limit, double damping,
                                     double max_step, double tolerance, double n_points, double* value_out,
                                     int32_t* iterations_out, double* damping_out) {
  if (!c) return FSDF_ERR_ARG;
  int rc = batch_loop_checks(c, "descend_lm_batch", x, B, iteration_limit, damping, max_step, n_points);
  if (rc || B == 0) return rc;
  const int nq = c->mech.nq;
  const size_t n = (size_t)nq, nn = n * n;
  const bool prior = !c->lm_prior.empty();
  if (prior && (int)c->lm_prior.size() != nq)
    return fail(c, FSDF_ERR_STATE, "descend_lm_batch: the prior has %d weights, the mechanism %d coordinates",
                (int)c->lm_prior.size(), nq);
  const double* mu = prior ? c->lm_prior.data() : nullptr;
  const std::vector<double> x_ref(x, x + (size_t)B * n);  // each candidate's own start
  std::vector<double> g((size_t)B * n), H((size_t)B * nn), xt((size_t)B * n), lam((size_t)B, damping),
      f((size_t)B, NAN), step(n), step_work(nn + n);
  std::vector<int32_t> it((size_t)B, 0);
  std::vector<char> running((size_t)B, iteration_limit > 0);
  // the compacted evaluation: the trials, their outputs, the candidates they belong to
  std::vector<double> ex((size_t)B * n), ef((size_t)B), eg((size_t)B * n), eH((size_t)B * nn);
  std::vector<int32_t> who;
  auto finish = [&](int status) {
    for (int32_t b = 0; b < B; ++b) {
      if (value_out) value_out[b] = f[(size_t)b];
      if (iterations_out) iterations_out[b] = it[(size_t)b];
      if (damping_out) damping_out[b] = lam[(size_t)b];
    }
    return status;
  };
  // lm_objective's statements on evaluation j of the compacted batch, candidate b
  auto wrap = [&](size_t j, int32_t b) {
    double* gj = eg.data() + j * n;
    double* Hj = eH.data() + j * nn;
    if (!mu) {
      ef[j] = ef[j] / n_points;
      for (int i = 0; i < nq; ++i) gj[i] = gj[i] / n_points;
      for (size_t i = 0; i < nn; ++i) Hj[i] = Hj[i] / n_points;
      return;
    }
    const double* xj = ex.data() + j * n;
    const double* xr = x_ref.data() + (size_t)b * n;
    double r = 0.0;
    for (int i = 0; i < nq; ++i) {
      const double e = xj[i] - xr[i];
      r += mu[i] * (e * e);
      gj[i] = gj[i] / n_points + (2.0 * mu[i]) * e;
    }
    ef[j] = ef[j] / n_points + r;
    for (int i = 0; i < nq; ++i)
      for (int k = 0; k < nq; ++k) {
        const size_t at = (size_t)i * n + k;
        Hj[at] = i == k ? Hj[at] / n_points + 2.0 * mu[i] : Hj[at] / n_points;
      }
  };
  bool first = true;
  for (;;) {
    who.clear();
    for (int32_t b = 0; b < B; ++b) {
      if (!running[(size_t)b]) continue;
      double* xb = x + (size_t)b * n;
      if (first) {  // the evaluation at the start x
        memcpy(ex.data() + who.size() * n, xb, n * sizeof(double));
        who.push_back(b);
        continue;
      }
      const double* gb = g.data() + (size_t)b * n;
      const double* Hb = H.data() + (size_t)b * nn;
      double& lb = lam[(size_t)b];
      bool trial = false;
      while (it[(size_t)b] < iteration_limit) {
        double nrm2 = 0.0;
        for (int i = 0; i < nq; ++i) nrm2 += gb[i] * gb[i];
        if (sqrt(nrm2) < tolerance) break;
        const int st = fsdf_lm_step(nq, Hb, gb, lb, max_step, step_work.data(), step.data());
        if (st == FSDF_ERR_DEGENERATE) {  // more damping, no evaluation
          lb *= 10.0;
          if (lb > 1e12) break;
          continue;
        }
        if (st) return finish(fail(c, st, "descend_lm_batch: the damped step of candidate %d", b));
        double* xtb = xt.data() + (size_t)b * n;
        for (int i = 0; i < nq; ++i) xtb[i] = xb[i] + step[i];
        memcpy(ex.data() + who.size() * n, xtb, n * sizeof(double));
        who.push_back(b);
        trial = true;
        break;
      }
      if (!trial) running[(size_t)b] = 0;
    }
    if (who.empty()) break;
    rc = batch_states(c, ex.data(), (int32_t)who.size(), ef.data(), eg.data(), eH.data(), "descend_lm_batch");
    if (rc) return finish(rc);
    for (size_t j = 0; j < who.size(); ++j) {
      const int32_t b = who[j];
      wrap(j, b);
      ++it[(size_t)b];
      double* xb = x + (size_t)b * n;
      double* gb = g.data() + (size_t)b * n;
      double* Hb = H.data() + (size_t)b * nn;
      double& lb = lam[(size_t)b];
      if (first) {
        f[(size_t)b] = ef[j];
        memcpy(gb, eg.data() + j * n, n * sizeof(double));
        memcpy(Hb, eH.data() + j * nn, nn * sizeof(double));
        continue;
      }
      if (ef[j] < f[(size_t)b]) {
        f[(size_t)b] = ef[j];
        memcpy(xb, ex.data() + j * n, n * sizeof(double));
        memcpy(gb, eg.data() + j * n, n * sizeof(double));
        memcpy(Hb, eH.data() + j * nn, nn * sizeof(double));
        lb = 1e-12 > lb / 10.0 ? 1e-12 : lb / 10.0;
      } else {
        lb *= 10.0;
        if (lb > 1e12) running[(size_t)b] = 0;
      }
    }
    first = false;
  }
  return finish(FSDF_OK);
}

// fsdf_descend's host loop (descend.hip: the NaiveSolver rule) for B candidates in lockstep: a
// round evaluates the candidates still running in one fsdf_batch_states without moments, then
// applies the loop's statements to each — f = c / n, g = (∂c/∂x / n) ./ divisors, stop when
// |g| < tolerance, else x += clamp(−rate g, ±max_step)
extern "C" int fsdf_descend_batch(fsdf_ctx* c, double* x, int32_t B, int32_t iteration_limit, double rate,
                                  double max_step, double tolerance, const double* divisors, double n_points,
                                  double* value_out, int32_t* iterations_out) {
  if (!c) return FSDF_ERR_ARG;
  int rc = batch_loop_checks(c, "descend_batch", x, B, iteration_limit, rate, max_step, n_points);
  if (rc || B == 0) return rc;
  const int ns = c->mech.nq;
  const size_t n = (size_t)ns;
  std::vector<double> f((size_t)B, 0.0), ex((size_t)B * n), ef((size_t)B), eg((size_t)B * n);
  std::vector<int32_t> it((size_t)B, 0), who;
  std::vector<char> running((size_t)B, 1);
  auto finish = [&](int status) {
    for (int32_t b = 0; b < B; ++b) {
      if (value_out) value_out[b] = f[(size_t)b];
      if (iterations_out) iterations_out[b] = it[(size_t)b];
    }
    return status;
  };
  for (;;) {
    who.clear();
    for (int32_t b = 0; b < B; ++b) {
      if (!running[(size_t)b] || it[(size_t)b] >= iteration_limit) continue;
      memcpy(ex.data() + who.size() * n, x + (size_t)b * n, n * sizeof(double));
      who.push_back(b);
    }
    if (who.empty()) break;
    rc = batch_states(c, ex.data(), (int32_t)who.size(), ef.data(), eg.data(), nullptr, "descend_batch");
    if (rc) return finish(rc);
    for (size_t j = 0; j < who.size(); ++j) {
      const int32_t b = who[j];
      double* xb = x + (size_t)b * n;
      double* g = eg.data() + j * n;
      ++it[(size_t)b];
      f[(size_t)b] = ef[j] / n_points;
      double nrm2 = 0.0;
      for (int i = 0; i < ns; ++i) {
        double gi = g[i] / n_points;
        if (divisors) gi = gi / divisors[i];
        g[i] = gi;
        nrm2 += gi * gi;
      }
      if (std::sqrt(nrm2) < tolerance) {
        running[(size_t)b] = 0;
        continue;
      }
      for (int i = 0; i < ns; ++i) xb[i] = xb[i] + std::min(std::max(-rate * g[i], -max_step), max_step);
    }
  }
  return finish(FSDF_OK);
}

// the two loops with every floating-point scalar read through a pointer (include/flashsdf.h: for
// bindings that pass them by reference, as fsdf_set_loss_ref)
extern "C" int fsdf_descend_lm_batch_ref(fsdf_ctx* c, double* x, int32_t B, int32_t iteration_limit,
                                         const double* params, double* value_out, int32_t* iterations_out,
                                         double* damping_out) {
  if (!c) return FSDF_ERR_ARG;
  if (!params) return fail(c, FSDF_ERR_ARG, "descend_lm_batch_ref: null parameters");
  return fsdf_descend_lm_batch(c, x, B, iteration_limit, params[0], params[1], params[2], params[3], value_out,
                               iterations_out, damping_out);
}

extern "C" int fsdf_descend_batch_ref(fsdf_ctx* c, double* x, int32_t B, int32_t iteration_limit,
                                      const double* params, const double* divisors, double* value_out,
                                      int32_t* iterations_out) {
  if (!c) return FSDF_ERR_ARG;
  if (!params) return fail(c, FSDF_ERR_ARG, "descend_batch_ref: null parameters");
  return fsdf_descend_batch(c, x, B, iteration_limit, params[0], params[1], params[2], divisors, params[3], value_out,
                            iterations_out);
}

extern "C" int fsdf_batch_time(fsdf_ctx* c, double* total_ms, int64_t* launches) {
  if (!c || !total_ms || !launches) return FSDF_ERR_ARG;
  HIPCHECK(c, hipSetDevice(c->device));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  double t = 0.0;
  for (size_t i = 0; i + 1 < c->batch_ev_used; i += 2) {
    float ms = 0.f;
    HIPCHECK(c, hipEventElapsedTime(&ms, c->batch_ev[i], c->batch_ev[i + 1]));
    t += ms;
  }
  *total_ms = t;
  *launches = (int64_t)(c->batch_ev_used / 2);
  c->batch_ev_used = 0;
  return FSDF_OK;
}
