// iterate.hip — iterations of a registered mechanism: fsdf_set_mechanism, RBF
// centres and deformations, the host halves of one CostFunctor iteration
// (FK, weight solve, chain rule) around a pass, the same with the Gauss-Newton
// Hessian (fsdf_value_gradient_hessian; with fsdf_set_lm_skins also for scenes
// with RBF skins and deformations) and its Levenberg-Marquardt loop
// (fsdf_descend_lm, with the prior of fsdf_set_lm_prior, on the host or —
// fsdf_set_lm_solver — on the device), and the solver loops of fsdf_descend on
// the host and on the device (solver.hip).

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.h"
#include "kin_impl.h"

// after an iteration pass (value_and_gradient, eval_state_device, descend):
// the new cloud's first one regroups it when the auto rule says so
static int iteration_regroup(fsdf_ctx* c) {
  if (!c->regroup_pending) return FSDF_OK;
  c->regroup_pending = false;
  if (c->regroup_mode != FSDF_REGROUP_AUTO) return FSDF_OK;
  return fsdf_regroup_auto(c, nullptr);
}

extern "C" int fsdf_set_mechanism(fsdf_ctx* c, int32_t nb, const int32_t* parent, const int32_t* kind,
                                  const int32_t* qoff, const double* axis, const double* AR, const double* At,
                                  const double* BR, const double* Bt, int32_t nq, const int32_t* surface_body,
                                  const double* frame_R, const double* frame_t) {
  if (!c) return FSDF_ERR_ARG;
  if (c->lm.S == 0) return fail(c, FSDF_ERR_STATE, "set_mechanism: set the surfaces first");
  if (nb < 1 || nq < 0 || !parent || !kind || !qoff || !axis || !AR || !At || !BR || !Bt || !surface_body ||
      !frame_R || !frame_t)
    return fail(c, FSDF_ERR_ARG, "set_mechanism: bad arguments");
  const int S = c->lm.S;
  for (int b = 1; b < nb; ++b) {
    if (parent[b] < 0 || parent[b] >= b) return fail(c, FSDF_ERR_ARG, "set_mechanism: bodies not in topological order");
    if (kind[b] < 0 || kind[b] > 2) return fail(c, FSDF_ERR_ARG, "set_mechanism: joint kind %d", kind[b]);
    const int width = kind[b] == 1 ? 1 : (kind[b] == 2 ? 7 : 0);
    if (width && (qoff[b] < 0 || qoff[b] + width > nq)) return fail(c, FSDF_ERR_ARG, "set_mechanism: q offset");
  }
  for (int k = 0; k < S; ++k)
    if (surface_body[k] < -1 || surface_body[k] >= nb) return fail(c, FSDF_ERR_ARG, "set_mechanism: surface body");
  auto& M = c->mech;
  M.nb = nb;
  M.nq = nq;
  M.parent.assign(parent, parent + nb);
  M.kind.assign(kind, kind + nb);
  M.qoff.assign(qoff, qoff + nb);
  M.surface_body.assign(surface_body, surface_body + S);
  M.axis.assign(axis, axis + 3 * nb);
  M.AR.assign(AR, AR + 9 * nb);
  M.At.assign(At, At + 3 * nb);
  M.BR.assign(BR, BR + 9 * nb);
  M.Bt.assign(Bt, Bt + 3 * nb);
  M.frame_R.assign(frame_R, frame_R + 9 * S);
  M.frame_t.assign(frame_t, frame_t + 3 * S);
  M.R.resize(9 * nb);
  M.t.resize(3 * nb);
  M.Rb.resize(9 * nb);
  M.tb.resize(3 * nb);
  M.poses.resize(12 * S);
  M.work.resize(6 * nb);
  M.rbf.clear();  // centre declarations name bodies of the previous tree
  M.x_prepared.clear();
  c->lm_prior.clear();  // (weights per coordinate of the previous tree)
  c->solver_tree_ok = false;
  return FSDF_OK;
}

extern "C" int fsdf_set_rbf_centres(fsdf_ctx* c, int32_t surface, int32_t n_sp, const int32_t* body_sp,
                                    const double* local_sp, const int32_t* deform_row_sp, int32_t n_sk,
                                    const int32_t* body_sk, const double* local_sk) {
  if (!c) return FSDF_ERR_ARG;
  auto& M = c->mech;
  if (M.nb == 0) return fail(c, FSDF_ERR_STATE, "set_rbf_centres: call fsdf_set_mechanism first");
  const int S = c->lm.S;
  if (surface < 0 || surface >= S || c->h_surface_kind[surface] != FSDF_SURFACE_RBF)
    return fail(c, FSDF_ERR_ARG, "set_rbf_centres: surface %d is not an RBF surface", surface);
  if (n_sp < 0 || n_sk < 0 || n_sp + n_sk != c->h_n_centers[surface] || (n_sp && (!body_sp || !local_sp)) ||
      (n_sk && (!body_sk || !local_sk)))
    return fail(c, FSDF_ERR_ARG, "set_rbf_centres: surface %d has %d centres, got %d + %d", surface,
                c->h_n_centers[surface], n_sp, n_sk);
  int r = 0;
  for (int k = 0; k < surface; ++k) r += c->h_surface_kind[k] == FSDF_SURFACE_RBF;
  M.rbf.resize(c->lm.R);
  auto& D = M.rbf[r];
  const int n = n_sp + n_sk;
  D.n_sp = n_sp;
  D.n = n;
  D.body.resize(n);
  D.drow.assign(n, -1);
  D.local.resize(3 * n);
  D.values.resize(n);
  for (int j = 0; j < n; ++j) {
    const bool sp = j < n_sp;
    const int b = sp ? body_sp[j] : body_sk[j - n_sp];
    if (b < -1 || b >= M.nb) return fail(c, FSDF_ERR_ARG, "set_rbf_centres: centre %d body %d", j, b);
    D.body[j] = b;
    if (sp && deform_row_sp) D.drow[j] = deform_row_sp[j];
    if (D.drow[j] < -1) return fail(c, FSDF_ERR_ARG, "set_rbf_centres: centre %d deformation row", j);
    const double* p = sp ? local_sp + 3 * j : local_sk + 3 * (j - n_sp);
    for (int i = 0; i < 3; ++i) D.local[3 * j + i] = p[i];
    D.values[j] = sp ? 0.0 : -1.0;  // src/Flash.jl:208-211
  }
  D.centres.resize(3 * n);
  D.u.resize(n + 4);
  D.lu.resize((size_t)(n + 4) * (n + 4));
  D.piv.resize(n + 4);
  D.G.resize(3 * n);
  D.work.resize(n + 4);
  c->solver_tree_ok = false;  // (the device loop's tree holds the centres)
  return FSDF_OK;
}

extern "C" int fsdf_set_deformations(fsdf_ctx* c, int32_t n_deform, double weight) {
  if (!c) return FSDF_ERR_ARG;
  if (n_deform < 0 || !std::isfinite(weight)) return fail(c, FSDF_ERR_ARG, "set_deformations: bad arguments");
  c->mech.n_deform = n_deform;
  c->mech.weight = weight;
  c->solver_tree_ok = false;  // (the device loop's state length)
  return FSDF_OK;
}

// The host halves of one CostFunctor iteration at x (fsdf_value_and_gradient
// and its device-split form fsdf_eval_state_device + fsdf_state_gradient):
// prepare = FK, RBF centres + weight solve + rows upload, surface poses;
// finish = RBF adjoint, chain rule, regularizer from an accumulator.
// upload = false: the host part only (FK, RBF centres + weight solve, surface
// poses into c->mech) — fsdf_state_gradient re-prepares an earlier x so the
// chain rule runs on that pass's solve (pipelined passes, flash/distributed.py)
static int iteration_prepare(fsdf_ctx* c, const double* x, const char* who, bool upload = true) {
  auto& M = c->mech;
  if (M.nb == 0) return fail(c, FSDF_ERR_STATE, "%s: no mechanism (call fsdf_set_mechanism)", who);
  if ((int)M.surface_body.size() != c->lm.S || (int)M.poses.size() != 12 * c->lm.S)
    return fail(c, FSDF_ERR_STATE, "%s: mechanism registered for another surface list (call fsdf_set_mechanism)", who);
  const int R = c->lm.R;
  if (R > 0) {
    bool all = (int)M.rbf.size() == R;
    for (int r = 0; all && r < R; ++r) all = M.rbf[r].n > 0;
    if (!all) return fail(c, FSDF_ERR_STATE, "%s: declare every RBF surface's centres (fsdf_set_rbf_centres)", who);
    for (const auto& D : M.rbf)
      for (int j = 0; j < D.n; ++j)
        if (D.drow[j] >= M.n_deform)
          return fail(c, FSDF_ERR_STATE, "%s: deformation row %d >= %d (fsdf_set_deformations)", who, D.drow[j],
                      M.n_deform);
  }
  HIPCHECK(c, hipSetDevice(c->device));
  // forward kinematics (quaternion blocks normalized inside: normalize!, src/gradientdescent.jl:30)
  int rc = fsdf_tree_transforms(M.nb, M.parent.data(), M.kind.data(), M.qoff.data(), M.axis.data(), M.AR.data(),
                                M.At.data(), M.BR.data(), M.Bt.data(), x, M.R.data(), M.t.data(), M.Rb.data(),
                                M.tb.data());
  if (rc) return fail(c, rc, "%s: forward kinematics (bad configuration)", who);
  const double* delta = x + M.nq;
  // RBF skins: centres c = R_b (p + δ) + t_b, the weight solve, the rows
  // (flash/rbf.py solve / rows)
  if (R > 0) {
    M.rows.clear();
    for (auto& D : M.rbf) {
      for (int j = 0; j < D.n; ++j) {
        double p[3] = {D.local[3 * j], D.local[3 * j + 1], D.local[3 * j + 2]};
        if (D.drow[j] >= 0)
          for (int i = 0; i < 3; ++i) p[i] += delta[3 * D.drow[j] + i];
        const int b = D.body[j];
        for (int i = 0; i < 3; ++i)
          D.centres[3 * j + i] = b < 0 ? p[i]
                                       : (M.R[9 * b + 3 * i] * p[0] + M.R[9 * b + 3 * i + 1] * p[1] +
                                          M.R[9 * b + 3 * i + 2] * p[2]) + M.t[3 * b + i];
      }
      rc = fsdf_rbf_solve(D.n, D.centres.data(), D.values.data(), D.u.data(), D.lu.data(), D.piv.data());
      if (rc) return fail(c, rc, "%s: singular RBF system", who);
      for (int j = 0; j < D.n; ++j) {
        M.rows.insert(M.rows.end(), D.centres.begin() + 3 * j, D.centres.begin() + 3 * j + 3);
        M.rows.push_back(D.u[j]);
      }
      M.rows.insert(M.rows.end(), D.u.begin() + D.n, D.u.end());
    }
    if (upload) {
      rc = fsdf_set_rbf_params(c, M.rows.data(), (int64_t)M.rows.size());
      if (rc) return rc;
    }
  }
  // surface poses T_world_body · T_body_geometry (identity for surfaces without
  // a body; kin_impl.h, the device solver's arithmetic too)
  const int S = c->lm.S;
  for (int k = 0; k < S; ++k) {
    double* P = M.poses.data() + 12 * k;
    const int b = M.surface_body[k];
    if (b < 0) {
      for (int i = 0; i < 12; ++i) P[i] = (i % 4 == 0 && i < 9) ? 1.0 : 0.0;
      continue;
    }
    fsdf::kin::surface_pose(M.R.data() + 9 * b, M.t.data() + 3 * b, M.frame_R.data() + 9 * k,
                            M.frame_t.data() + 3 * k, P);
  }
  M.x_prepared.assign(x, x + M.nq + 3 * M.n_deform);
  return FSDF_OK;
}

static int iteration_finish(fsdf_ctx* c, const double* x, const double* accum, double* cost_out, double* grad_out,
                            const char* who) {
  auto& M = c->mech;
  const int R = c->lm.R, S = c->lm.S;
  const double* delta = x + M.nq;
  for (int i = 0; i < M.nq + 3 * M.n_deform; ++i) grad_out[i] = 0.0;
  // RBF chain (flash/rbf.py chain): G_j = ∂c/∂c_j through the solve -> body
  // wrenches (F, M about the world origin; δc = -(ω·M + v·F)) and ∂c/∂δ
  if (R > 0) {
    M.body_wrench.assign(6 * M.nb, 0.0);
    const double* block = accum + 1 + 6 * S;
    for (auto& D : M.rbf) {
      const int rc = fsdf_rbf_adjoint(D.n, D.centres.data(), D.u.data(), D.lu.data(), D.piv.data(), block,
                                      D.G.data(), D.work.data());
      if (rc) return fail(c, rc, "%s: RBF adjoint", who);
      block += 4 * D.n + 4;
      for (int j = 0; j < D.n; ++j) {
        const double* G = D.G.data() + 3 * j;
        const double* cj = D.centres.data() + 3 * j;
        const int b = D.body[j];
        if (b >= 0) {
          double* w = M.body_wrench.data() + 6 * b;
          w[0] -= G[0];
          w[1] -= G[1];
          w[2] -= G[2];
          w[3] -= cj[1] * G[2] - cj[2] * G[1];
          w[4] -= cj[2] * G[0] - cj[0] * G[2];
          w[5] -= cj[0] * G[1] - cj[1] * G[0];
        }
        if (D.drow[j] >= 0) {  // c_j = R_b (p_j + δ_j) + t_b
          double* gd = grad_out + M.nq + 3 * D.drow[j];
          for (int i = 0; i < 3; ++i)
            gd[i] += b < 0 ? G[i] : (M.R[9 * b + i] * G[0] + M.R[9 * b + 3 + i] * G[1] + M.R[9 * b + 6 + i] * G[2]);
        }
      }
    }
  }
  const int rc = fsdf_config_gradient(M.nb, M.parent.data(), M.kind.data(), M.qoff.data(), M.axis.data(),
                                      M.Rb.data(), M.tb.data(), x, S, M.surface_body.data(), accum + 1,
                                      R > 0 ? M.body_wrench.data() : nullptr, M.work.data(), grad_out);
  if (rc) return fail(c, rc, "%s: chain rule", who);
  // the deformation regularizer weight Σ|δ|^2 (src/gradientdescent.jl:33-37)
  double reg = 0.0;
  for (int i = 0; i < 3 * M.n_deform; ++i) {
    reg += delta[i] * delta[i];
    grad_out[M.nq + i] += 2.0 * M.weight * delta[i];
  }
  *cost_out = accum[0] + M.weight * reg;
  return FSDF_OK;
}

// diagnostic builds (-DFSDF_HOST_TIMES=1): host-side clocks of the host solver
// loop's iterations — prepare (FK, poses), launches, the wait, the chain rule —
// summed here and printed by fsdf_descend (stderr), to split the GPU's idle
// gap between iterations into host work and synchronisation latency
#if FSDF_HOST_TIMES
#include <chrono>
static double g_host_t[8];
static long g_host_n;
static inline double host_now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
#define HOST_STAMP(i) const double ht_##i = host_now_us()
#else
#define HOST_STAMP(i)
#endif

extern "C" int fsdf_value_and_gradient(fsdf_ctx* c, const double* x, double* cost_out, double* grad_out) {
  if (!c) return FSDF_ERR_ARG;
  HOST_STAMP(0);
  if (!x || !cost_out || !grad_out) return fail(c, FSDF_ERR_ARG, "value_and_gradient: null argument");
  int rc = iteration_prepare(c, x, "value_and_gradient");
  if (rc) return rc;
  auto& M = c->mech;
  // the reduction stores the accumulator straight into pinned host memory (no
  // D2H copy command before the sync: the full iteration is 1.5 to 2.5 us
  // faster than with the pinned copy, profiles/r02/experiments/r02zc)
  rc = ensure_host_acc(c, accum_len(c));
  if (rc) return rc;
  double* d_acc_host = nullptr;
  HIPCHECK(c, hipHostGetDevicePointer((void**)&d_acc_host, c->h_acc.get(), 0));
  HOST_STAMP(1);
  rc = run_pass(c, M.poses.data(), c->cur.pts.get(), c->n, d_acc_host, nullptr, nullptr, nullptr, nullptr, true);
  if (rc) return rc;
  HOST_STAMP(2);
  rc = iteration_regroup(c);  // (stream-ordered after the pass: the sync below covers it)
  if (rc) return rc;
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  HOST_STAMP(3);
  rc = iteration_finish(c, x, c->h_acc.get(), cost_out, grad_out, "value_and_gradient");
#if FSDF_HOST_TIMES
  HOST_STAMP(4);
  g_host_t[0] += ht_1 - ht_0;  // prepare
  g_host_t[1] += ht_2 - ht_1;  // pose + pass + reduce launches
  g_host_t[2] += ht_3 - ht_2;  // wait (device work + wake-up)
  g_host_t[3] += ht_4 - ht_3;  // chain rule
  ++g_host_n;
#endif
  return rc;
}

// fsdf_value_and_gradient with the Gauss-Newton Hessian 2 JᵀJ of the same pass
// (rigid scenes; others below, behind fsdf_set_lm_skins): the pass also writes k* and ∇d* in resident order, the
// moments launch (moments.hip) reduces them per surface, and
// fsdf_gauss_newton_matrix contracts them with that pass's FK. The auto
// regroup is queued after the moments launch: they read the layout the pass
// ran on.
extern "C" int fsdf_value_gradient_hessian(fsdf_ctx* c, const double* x, double* cost_out, double* grad_out,
                                           double* hess_out) {
  if (!c) return FSDF_ERR_ARG;
  if (!x || !cost_out || !grad_out || !hess_out)
    return fail(c, FSDF_ERR_ARG, "value_gradient_hessian: null argument");
  const bool rigid = c->lm.R == 0 && c->mech.n_deform == 0;
  if (!rigid && !c->lm_skins)
    return fail(c, FSDF_ERR_STATE,
                "value_gradient_hessian: the Gauss-Newton matrix is defined for rigid scenes (no RBF skin, no "
                "deformation)");
  int rc = iteration_prepare(c, x, "value_gradient_hessian");
  if (rc) return rc;
  auto& M = c->mech;
  rc = run_pass_moments(c, M.poses.data(), "value_gradient_hessian", rigid ? kMomentsRigid : kMomentsAll);
  if (rc) return rc;
  rc = iteration_regroup(c);  // (stream-ordered after the pass and the moments: the sync below covers it)
  if (rc) return rc;
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  rc = iteration_finish(c, x, c->h_acc.get(), cost_out, grad_out, "value_gradient_hessian");
  if (rc) return rc;
  const int nq = M.nq;
  M.gn_work.resize((size_t)36 * M.nb + (size_t)6 * nq);
  if (rigid) {
    rc = fsdf_gauss_newton_matrix(M.nb, M.parent.data(), M.kind.data(), M.qoff.data(), M.axis.data(), M.Rb.data(),
                                  M.tb.data(), x, c->lm.S, M.surface_body.data(), c->h_moments.get(), nq,
                                  M.gn_work.data(), hess_out);
    if (rc) return fail(c, rc, "value_gradient_hessian: Gauss-Newton matrix");
    for (size_t i = 0; i < (size_t)nq * nq; ++i) hess_out[i] = 2.0 * hess_out[i];
    return FSDF_OK;
  }
  // skins and deformations (fsdf_set_lm_skins): A = A_hulls in the nq block +
  // Σ_r L_r M_r L_rᵀ over the nx = nq + 3 n_deform coordinates, H = 2 A +
  // 2 weight I on the deformations (the regulariser is a sum of squares too)
  const int nx = nq + 3 * M.n_deform, S = c->lm.S;
  double* hm = c->h_moments.get();
  for (int k = 0; k < S; ++k)  // (a skin's points have no hull moments)
    if (c->h_surface_kind[k] != FSDF_SURFACE_HULL)
      for (int e = 0; e < fsdf::kMomentsLen; ++e) hm[(size_t)fsdf::kMomentsLen * k + e] = 0.0;
  M.gn_hull.resize((size_t)nq * nq);
  rc = fsdf_gauss_newton_matrix(M.nb, M.parent.data(), M.kind.data(), M.qoff.data(), M.axis.data(), M.Rb.data(),
                                M.tb.data(), x, S, M.surface_body.data(), hm, nq, M.gn_work.data(), M.gn_hull.data());
  if (rc) return fail(c, rc, "value_gradient_hessian: Gauss-Newton matrix");
  for (size_t i = 0; i < (size_t)nx * nx; ++i) hess_out[i] = 0.0;
  for (int i = 0; i < nq; ++i)
    for (int j = 0; j < nq; ++j) hess_out[(size_t)i * nx + j] = M.gn_hull[(size_t)i * nq + j];
  const double* sm = c->h_skin_moments.get();
  for (auto& D : M.rbf) {
    const int m = 4 * D.n + 4;
    M.skin_L.resize((size_t)nx * m);
    M.skin_work.resize(std::max((size_t)8 * D.n + 8 + (size_t)12 * M.nb + nx, (size_t)nx * m));
    rc = fsdf_rbf_state_map(M.nb, M.parent.data(), M.kind.data(), M.qoff.data(), M.axis.data(), M.R.data(),
                            M.Rb.data(), M.tb.data(), x, nq, D.n, D.centres.data(), D.u.data(), D.lu.data(),
                            D.piv.data(), D.body.data(), D.drow.data(), M.n_deform, M.skin_work.data(),
                            M.skin_L.data());
    if (!rc) rc = fsdf_gauss_newton_add(nx, m, M.skin_L.data(), sm, M.skin_work.data(), hess_out);
    if (rc) return fail(c, rc, "value_gradient_hessian: the skins' Gauss-Newton term");
    sm += (size_t)m * m;
  }
  for (size_t i = 0; i < (size_t)nx * nx; ++i) hess_out[i] = 2.0 * hess_out[i];
  for (int i = nq; i < nx; ++i) hess_out[(size_t)i * nx + i] += 2.0 * M.weight;
  return FSDF_OK;
}

// fsdf_lm_minimize (gauss_newton.cpp) over fsdf_value_gradient_hessian with
// estimate_state's wrapped cost (c / n, ∂c/∂x / n, H / n) and, when one is set,
// the prior on the frame's start state: the host loop, one synchronization
// per evaluation.
namespace {
struct LmObjective {
  fsdf_ctx* c;
  int nq;
  double n_points;
  const double* mu;     // fsdf_set_lm_prior's weights [nq], or null: no prior
  const double* x_ref;  // the x handed to fsdf_descend_lm (the frame's warm start)
};
int lm_objective(void* user, const double* x, double* f, double* g, double* H) {
  const LmObjective& o = *(const LmObjective*)user;
  double cost = 0.0;
  const int rc = fsdf_value_gradient_hessian(o.c, x, &cost, g, H);
  if (rc) return rc;
  if (!o.mu) {
    *f = cost / o.n_points;
    for (int i = 0; i < o.nq; ++i) g[i] = g[i] / o.n_points;
    for (size_t i = 0; i < (size_t)o.nq * o.nq; ++i) H[i] = H[i] / o.n_points;
    return FSDF_OK;
  }
  // the prior Σ mu_i (x_i − x̄_i)^2 on the wrapped objective, in the one
  // operation order flash.tracking.state_prior restates (the same bits)
  double r = 0.0;
  for (int i = 0; i < o.nq; ++i) {
    const double e = x[i] - o.x_ref[i];
    r += o.mu[i] * (e * e);
    g[i] = g[i] / o.n_points + (2.0 * o.mu[i]) * e;
  }
  *f = cost / o.n_points + r;
  for (int i = 0; i < o.nq; ++i)
    for (int j = 0; j < o.nq; ++j) {
      const size_t at = (size_t)i * o.nq + j;
      H[at] = i == j ? H[at] / o.n_points + 2.0 * o.mu[i] : H[at] / o.n_points;
    }
  return FSDF_OK;
}
}  // namespace

extern "C" int fsdf_set_lm_prior(fsdf_ctx* c, const double* weight, int32_t n) {
  if (!c) return FSDF_ERR_ARG;
  if (n < 0) return fail(c, FSDF_ERR_ARG, "set_lm_prior: n %d", n);
  if (!weight || n == 0) {
    c->lm_prior.clear();
    return FSDF_OK;
  }
  for (int i = 0; i < n; ++i)
    if (!(weight[i] >= 0.0) || !std::isfinite(weight[i]))
      return fail(c, FSDF_ERR_ARG, "set_lm_prior: weight %d is negative or not finite", i);
  c->lm_prior.assign(weight, weight + n);
  return FSDF_OK;
}

extern "C" int fsdf_set_lm_solver(fsdf_ctx* c, int32_t device_loop) {
  if (!c) return FSDF_ERR_ARG;
  if (device_loop < 0 || device_loop > 2) return fail(c, FSDF_ERR_ARG, "set_lm_solver: mode %d", device_loop);
  c->lm_solver_device = device_loop;
  return FSDF_OK;
}

extern "C" int fsdf_set_lm_skins(fsdf_ctx* c, int32_t enable) {
  if (!c) return FSDF_ERR_ARG;
  if (enable != 0 && enable != 1) return fail(c, FSDF_ERR_ARG, "set_lm_skins: enable %d", enable);
  c->lm_skins = enable;
  return FSDF_OK;
}

static int build_solver_tree(fsdf_ctx* c);

// fsdf_descend_lm with every evaluation on the device (solver.hip, "the device
// Levenberg-Marquardt loop"): solver_init (FK of x -> the first posed model),
// then per evaluation pass (k*, ∇d* in resident order) -> reduce -> moments ->
// their reduce -> LM step -> FK + pose of the next trial, all enqueued up
// front; one read-back of x, f, the count, the damping and the flags. The
// same bits as fsdf_lm_minimize over lm_objective.
// The rule of device_buffers.h, as run_pass_moments: (1) every buffer the
// frame hands to a launch is reserved — per-point outputs, moments and their
// partials, the solver state with the accepted g and H, the pinned staging;
// (2) their pointers are read into locals; (3) the launches take the locals.
// The cloud pointer alone is read again after the first evaluation's regroup,
// which swaps the resident cloud's buffer (sort.hip regroup_points).
static int descend_lm_device(fsdf_ctx* c, double* x, int32_t iteration_limit, double damping, double max_step,
                             double tolerance, double n_points, double* value_out, int32_t* iterations_out,
                             double* damping_out) {
  auto& M = c->mech;
  const int nq = M.nq, nb = M.nb, S = c->lm.S;
  const int64_t n = c->n;
  const bool prior = !c->lm_prior.empty();
  const fsdf::SolverTree& T = c->stree;
  if (damping_out) *damping_out = damping;  // (fsdf_lm_minimize's first line: also what a failed first evaluation leaves)
  // device: x [2][nq] | x_ref [nq] | mu [nq] | lam | flags [4] (as 2 doubles) | f | xa [nq] | g [nq] |
  // H [nq][nq] | Rb|tb [2][12 nb]; uploaded: the first 4 nq + 3, read back: lam | flags | f | xa
  const size_t o_ref = 2 * (size_t)nq, o_mu = 3 * (size_t)nq, o_lam = 4 * (size_t)nq, o_flags = o_lam + 1,
               o_f = o_flags + 2, o_xa = o_f + 1, o_g = o_xa + nq, o_H = o_g + nq, o_Rb = o_H + (size_t)nq * nq,
               need = o_Rb + 24 * (size_t)nb;
  const size_t up = o_f, back = (size_t)nq + 4;
  // (1) reserve
  int rc = ensure_outputs(c, n);
  if (rc) return rc;
  HIPCHECK(c, c->moments_partials.reserve(fsdf::moments_partials_len(n, S)));
  HIPCHECK(c, c->moments.reserve((size_t)S * fsdf::kMomentsLen));
  if (c->solver.capacity() < need) HIPCHECK(c, hipStreamSynchronize(c->stream));  // (an earlier frame's launches)
  HIPCHECK(c, c->solver.reserve(need));
  HIPCHECK(c, c->h_solver.reserve(up + back));
  // (2) read the pointers
  const void* d_pts = c->cur.pts.get();
  int32_t* d_kstar = c->kstar.get();
  double* d_grad = c->grad.get();
  double* d_partials = c->moments_partials.get();
  double* d_moments = c->moments.get();
  double* d_accum = c->model.accum.get();
  double* d = c->solver.get();
  double* h = c->h_solver.get();
  HIPCHECK(c, hipStreamSynchronize(c->stream));  // (the pinned staging of an earlier frame is free)
  memset(h, 0, up * sizeof(double));
  memcpy(h, x, (size_t)nq * sizeof(double));  // (trial 0)
  memcpy(h + o_ref, x, (size_t)nq * sizeof(double));
  if (prior) memcpy(h + o_mu, c->lm_prior.data(), (size_t)nq * sizeof(double));
  h[o_lam] = damping;
  fsdf::LmState ls;
  ls.x = d;
  ls.x_ref = d + o_ref;
  ls.mu = prior ? d + o_mu : nullptr;
  ls.lam = d + o_lam;
  ls.flags = (int*)(d + o_flags);
  ls.f = d + o_f;
  ls.xa = d + o_xa;
  ls.g = d + o_g;
  ls.H = d + o_H;
  ls.Rb = d + o_Rb;
  ls.max_step = max_step;
  ls.tol = tolerance;
  ls.n_points = n_points;
  ls.weight = M.weight;
  ls.limit = iteration_limit;
  fsdf::SolverState st;  // (solver_init's view: x0 in slot 0 -> Rb, tb and the first posed model)
  st.x = ls.x;
  st.Rb = ls.Rb;
  st.f = ls.f;
  st.flags = ls.flags;
  // (3) enqueue
  HIPCHECK(c, hipMemcpyAsync(d, h, up * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIPCHECK(c, fsdf::launch_solver_init(T, st, c->lm, c->pm, c->precision, c->stream));
  for (int it = 0; it < iteration_limit; ++it) {
    rc = run_pass(c, nullptr, d_pts, n, d_accum, d_kstar, nullptr, d_grad, nullptr, true, true, ls.flags);
    if (rc) return rc;
    HIPCHECK(c, fsdf::launch_moments(c->precision, d_pts, d_kstar, d_grad, n, S, d_partials, d_moments, c->stream,
                                     ls.flags));
    if (it == 0) {  // (after the moments launch: they read the layout the pass ran on)
      rc = iteration_regroup(c);
      if (rc) return rc;
      d_pts = c->cur.pts.get();
    }
    HIPCHECK(c, fsdf::launch_lm_step(T, ls, d_accum, d_moments, it, c->stream));
    if (it + 1 < iteration_limit)
      HIPCHECK(c, fsdf::launch_lm_pose(T, ls, c->lm, c->pm, c->precision, (it + 1) & 1, c->stream));
  }
  double* hb = h + up;  // lam | flags | f | xa
  HIPCHECK(c, hipMemcpyAsync(hb, ls.lam, back * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  int flags[4];
  memcpy(flags, hb + 1, sizeof flags);
#if FSDF_SOLVER_TIMES
  {
    unsigned long long tt[16];
    fsdf::solver_times(tt);
    fprintf(stderr, "LM step phases of evaluation 5 (10 ns):");
    for (int i = 1; i < 10; ++i) fprintf(stderr, " %lld", (long long)(tt[i] - tt[0]));
    fprintf(stderr, "\n");
  }
#endif
  if (iterations_out) *iterations_out = flags[1];
  if (flags[1] > 0) {  // (as the host loop: x the last accepted point, also when a later evaluation failed)
    memcpy(x, hb + 4, (size_t)nq * sizeof(double));
    if (damping_out) *damping_out = hb[0];
    if (value_out) *value_out = hb[3];
  }
  if (flags[2] == 2) return fail(c, FSDF_ERR_ARG, "descend_lm: poses not finite (configuration diverged)");
  if (flags[2]) return fail(c, FSDF_ERR_ARG, "value_gradient_hessian: forward kinematics (bad configuration)");
  return FSDF_OK;
}

extern "C" int fsdf_descend_lm(fsdf_ctx* c, double* x, int32_t iteration_limit, double damping, double max_step,
                               double tolerance, double n_points, double* value_out, int32_t* iterations_out,
                               double* damping_out) {
  if (!c) return FSDF_ERR_ARG;
  if (iterations_out) *iterations_out = 0;
  if (!x || iteration_limit < 0 || !(n_points > 0.0) || !std::isfinite(damping) || !(max_step >= 0.0))
    return fail(c, FSDF_ERR_ARG, "descend_lm: bad arguments");
  if (c->mech.nb == 0) return fail(c, FSDF_ERR_STATE, "descend_lm: no mechanism (call fsdf_set_mechanism)");
  const bool rigid = c->lm.R == 0 && c->mech.n_deform == 0;
  if (!rigid && !c->lm_skins)
    return fail(c, FSDF_ERR_STATE, "descend_lm: rigid scenes only (no RBF skin, no deformation)");
  const auto& Mc = c->mech;
  if ((int)Mc.surface_body.size() != c->lm.S || (int)Mc.poses.size() != 12 * c->lm.S)
    return fail(c, FSDF_ERR_STATE,
                "descend_lm: mechanism registered for another surface list (call fsdf_set_mechanism)");
  // (the state: the joint coordinates, then — fsdf_set_lm_skins — the deformations)
  const int nq = c->mech.nq + 3 * c->mech.n_deform;
  const bool prior = !c->lm_prior.empty();
  if (prior && (int)c->lm_prior.size() != nq)
    return fail(c, FSDF_ERR_STATE, "descend_lm: the prior has %d weights, the mechanism %d coordinates",
                (int)c->lm_prior.size(), nq);
  if (!rigid && c->lm_solver_device == 2)
    return fail(c, FSDF_ERR_STATE, "descend_lm: the device loop was required (fsdf_set_lm_solver 2) but the scene "
                                   "has RBF skins / deformations (their loop runs on the host)");
  // the device loop (fsdf_set_lm_solver 1 / 2): a finite damping > 0 (the
  // step's raises of a degenerate factorisation are then bounded), resident
  // points, the moments table and both solver kernels' carves within their LDS
  if (rigid && c->lm_solver_device && iteration_limit > 0) {
    const bool required = c->lm_solver_device == 2;
    if (required && !(damping > 0.0))
      return fail(c, FSDF_ERR_ARG, "descend_lm: the device loop needs a damping > 0");
    bool device_loop = damping > 0.0 && c->n > 0 && fsdf::moments_fit(c->lm.S);
    if (device_loop) {
      HIPCHECK(c, hipSetDevice(c->device));
      if (!c->solver_tree_ok) {
        const int rc = build_solver_tree(c);
        if (rc) return rc;
      }
      device_loop = fsdf::solver_fits(Mc.nb, nq, c->lm.S, c->stree.ni, c->stree.nd, 0, 0, nullptr) &&
                    fsdf::lm_solver_fits(Mc.nb, nq, c->lm.S);
    }
    if (required && !device_loop)
      return fail(c, FSDF_ERR_STATE, "descend_lm: the device loop was required (fsdf_set_lm_solver 2) but the scene %s",
                  c->n == 0 ? "has no resident points" : "does not fit the solver kernels' LDS");
    if (device_loop)
      return descend_lm_device(c, x, iteration_limit, damping, max_step, tolerance, n_points, value_out,
                               iterations_out, damping_out);
  }
  const std::vector<double> x_ref(x, x + (prior ? nq : 0));
  LmObjective o{c, nq, n_points, prior ? c->lm_prior.data() : nullptr, prior ? x_ref.data() : nullptr};
  std::vector<double> work((size_t)3 * nq * nq + (size_t)5 * nq + 1);
  return fsdf_lm_minimize(lm_objective, &o, nq, x, iteration_limit, damping, max_step, tolerance, work.data(),
                          value_out, iterations_out, damping_out);
}

// The solver loop of estimate_state (src/tracking.jl:16-26 with the
// NaiveSolver restated in flash/tracking.py) around fsdf_value_and_gradient,
// without a host-language round trip per iteration: f = c/n, g = (∂c/∂x / n)
// ./ divisors; stop when |g| < tolerance; else x += clamp(-rate g, ±max_step).
// The device arrays of the mechanism for the solver step (solver.hip) and
// the level schedules of its parallel FK (bodies by depth) and subtree sums
// (parents by height, children in descending index: the host's reverse
// topological loop adds them in that order).
static int build_solver_tree(fsdf_ctx* c) {
  auto& M = c->mech;
  const int nb = M.nb, S = c->lm.S;
  std::vector<int> depth(nb, 0), height(nb, 0), nchild(nb, 0);
  for (int b = 1; b < nb; ++b) depth[b] = depth[M.parent[b]] + 1;
  for (int b = nb - 1; b >= 1; --b) {
    const int p = M.parent[b];
    height[p] = std::max(height[p], height[b] + 1);
    ++nchild[p];
  }
  int D = 0, H = 0;
  for (int b = 1; b < nb; ++b) {
    D = std::max(D, depth[b]);
    if (nchild[b]) H = std::max(H, height[b]);
  }
  std::vector<int32_t> iv;  // parent | kind | qoff | depth_order | depth_off | height_order | height_off |
                            // child_off | child_list | surf_off | surf_list | surface_body
  auto put = [&](const std::vector<int32_t>& v) {
    const size_t at = iv.size();
    iv.insert(iv.end(), v.begin(), v.end());
    return at;
  };
  // dord / doff: every body's path from the root, its ancestors of depth 1 .. its own
  // (the device composes a body's chain in registers, one thread per body)
  std::vector<int32_t> dord, doff(1, 0), hord, hoff(1, 0), coff(1, 0), clist, soff(1, 0), slist;
  dord.reserve((size_t)nb * (size_t)(D + 1));
  for (int b = 0; b < nb; ++b) {
    std::vector<int32_t> path;
    for (int a = b; a > 0; a = M.parent[a]) path.push_back(a);
    dord.insert(dord.end(), path.rbegin(), path.rend());
    doff.push_back((int32_t)dord.size());
  }
  int widest = 0;  // the most parents at one height: the subtree sums run in one wave when 6x that fits
  // chains: every body but the root has at most one child (IRB140, M64's arms): body b's
  // subtree is the list b, child, grandchild, ... (dlist / dof), summed in one thread
  bool chains = true;
  for (int b = 1; b < nb; ++b) chains = chains && nchild[b] <= 1;
  std::vector<int32_t> dlist, dof(1, 0);
  if (chains) {
    std::vector<int32_t> child(nb, -1);
    for (int b = 1; b < nb; ++b)
      if (M.parent[b] > 0) child[M.parent[b]] = b;
    for (int b = 0; b < nb; ++b) {
      for (int a = b; b > 0 && a >= 0; a = child[a]) dlist.push_back(a);
      dof.push_back((int32_t)dlist.size());
    }
  }
  for (int h = 1; h <= H; ++h) {
    for (int b = 1; b < nb; ++b)
      if (nchild[b] && height[b] == h) hord.push_back(b);
    widest = std::max(widest, (int)hord.size() - hoff.back());
    hoff.push_back((int32_t)hord.size());
  }
  for (int p = 0; p < nb; ++p) {
    for (int b = nb - 1; b > p; --b)
      if (M.parent[b] == p) clist.push_back(b);
    coff.push_back((int32_t)clist.size());
    for (int k = 0; k < S; ++k)
      if (M.surface_body[k] == p) slist.push_back(k);
    soff.push_back((int32_t)slist.size());
  }
  // RBF skins (declared ones; fsdf_descend takes the device loop only with all of them declared)
  std::vector<int32_t> rn, rcoff(1, 0), rluoff(1, 0), rbody, rdrow;
  std::vector<double> rlocal, rvalues;
  for (const auto& D : M.rbf) {
    rn.push_back(D.n);
    rcoff.push_back(rcoff.back() + D.n);
    rluoff.push_back(rluoff.back() + (D.n + 4) * (D.n + 4));
    rbody.insert(rbody.end(), D.body.begin(), D.body.end());
    rdrow.insert(rdrow.end(), D.drow.begin(), D.drow.end());
    rlocal.insert(rlocal.end(), D.local.begin(), D.local.end());
    rvalues.insert(rvalues.end(), D.values.begin(), D.values.end());
  }
  const size_t o_parent = put(M.parent), o_kind = put(M.kind), o_qoff = put(M.qoff), o_dord = put(dord),
               o_doff = put(doff), o_hord = put(hord), o_hoff = put(hoff), o_coff = put(coff), o_clist = put(clist),
               o_soff = put(soff), o_slist = put(slist), o_sb = put(M.surface_body), o_dlist = put(dlist),
               o_dof = put(dof), o_rn = put(rn), o_rcoff = put(rcoff), o_rluoff = put(rluoff), o_rbody = put(rbody),
               o_rdrow = put(rdrow);
  std::vector<double> dv;
  auto putd = [&](const std::vector<double>& v) {
    const size_t at = dv.size();
    dv.insert(dv.end(), v.begin(), v.end());
    return at;
  };
  const size_t o_axis = putd(M.axis), o_AR = putd(M.AR), o_At = putd(M.At), o_BR = putd(M.BR), o_Bt = putd(M.Bt),
               o_FR = putd(M.frame_R), o_Ft = putd(M.frame_t), o_rlocal = putd(rlocal), o_rvalues = putd(rvalues);
  HIPCHECK(c, hipStreamSynchronize(c->stream));  // (a previous frame's steps may still read the old arrays)
  c->stree_blob.reset();
  const size_t bytes = dv.size() * sizeof(double) + iv.size() * sizeof(int32_t);
  const size_t chunks = (bytes + 15) / 16;
  std::vector<char> blob(chunks * 16, 0);
  memcpy(blob.data(), dv.data(), dv.size() * sizeof(double));
  memcpy(blob.data() + dv.size() * sizeof(double), iv.data(), iv.size() * sizeof(int32_t));
  HIPCHECK(c, c->stree_blob.reserve(std::max<size_t>(blob.size(), 16) / sizeof(double)));
  HIPCHECK(c, hipMemcpy(c->stree_blob.get(), blob.data(), blob.size(), hipMemcpyHostToDevice));
  fsdf::SolverTree& T = c->stree;
  T.nb = nb;
  T.nx = M.nq + 3 * M.n_deform;
  T.nq = M.nq;
  T.S = S;
  T.R = (int)rn.size();
  T.n_deform = M.n_deform;
  T.rc = rcoff.back();
  T.rm = T.rc + 4 * T.R;
  T.rlu = rluoff.back();
  T.racc = 4 * T.rc + 4 * T.R;
  T.rbf_n = (int)o_rn;
  T.rbf_coff = (int)o_rcoff;
  T.rbf_luoff = (int)o_rluoff;
  T.rbf_body = (int)o_rbody;
  T.rbf_drow = (int)o_rdrow;
  T.rbf_local = (int)o_rlocal;
  T.rbf_values = (int)o_rvalues;
  T.D = D;
  T.H = H;
  T.blob = c->stree_blob.get();
  T.ni = (int)iv.size();
  T.nd = (int)dv.size();
  T.chunks16 = (int)chunks;
  T.parent = (int)o_parent;
  T.kind = (int)o_kind;
  T.qoff = (int)o_qoff;
  T.path_list = (int)o_dord;
  T.path_off = (int)o_doff;
  T.narrow = 6 * widest <= 64;
  T.chains = chains;
  T.chain_list = (int)o_dlist;
  T.chain_off = (int)o_dof;
  T.height_order = (int)o_hord;
  T.height_off = (int)o_hoff;
  T.child_off = (int)o_coff;
  T.child_list = (int)o_clist;
  T.surf_off = (int)o_soff;
  T.surf_list = (int)o_slist;
  T.surface_body = (int)o_sb;
  T.axis = (int)o_axis;
  T.AR = (int)o_AR;
  T.At = (int)o_At;
  T.BR = (int)o_BR;
  T.Bt = (int)o_Bt;
  T.frame_R = (int)o_FR;
  T.frame_t = (int)o_Ft;
  c->solver_tree_ok = true;
  return FSDF_OK;
}

// fsdf_descend for rigid scenes, every iteration on the device: solver_init
// (FK of x0 -> poses), then per iteration pose -> pass -> reduce -> solver
// step, all enqueued up front; one read-back of x, f and the count at the end.
// Bit-identical to the host loop below (solver.hip).
static int descend_device(fsdf_ctx* c, double* x, int32_t iteration_limit, double rate, double max_step,
                          double tolerance, const double* divisors, double n_points, double* value_out,
                          int32_t* iterations_out) {
  auto& M = c->mech;
  const int nx = M.nq + 3 * M.n_deform, nb = M.nb;  // (the state: joint coordinates, then the deformations)
  HIPCHECK(c, hipSetDevice(c->device));
  if (!c->solver_tree_ok) {
    const int rc = build_solver_tree(c);
    if (rc) return rc;
  }
  // device: x [2][nx] (slots by iteration parity) | div [nx] | Rb|tb [2][12 nb] | f | RBF scenes: the
  // weight solve's state [2][9 nb + 3 rc + rm + rlu] and row permutation [2][rm] ints; flags [4] int
  const fsdf::SolverTree& T = c->stree;
  const size_t rbf_slot = T.R > 0 ? 9 * (size_t)nb + 3 * (size_t)T.rc + (size_t)T.rm + (size_t)T.rlu : 0;
  const size_t need = (size_t)3 * nx + 24 * (size_t)nb + 1 + 2 * rbf_slot + (T.R > 0 ? (size_t)T.rm + 1 : 0);
  if (c->solver.capacity() < need) HIPCHECK(c, hipStreamSynchronize(c->stream));
  HIPCHECK(c, c->solver.reserve(need));
  HIPCHECK(c, c->solver_flags.reserve(4));
  // pinned: x [2][nx] | div [nx] | f | flags [4] (as 2 doubles)
  HIPCHECK(c, c->h_solver.reserve((size_t)3 * nx + 3));
  double* h = c->h_solver.get();
  double* d_solver = c->solver.get();
  HIPCHECK(c, hipStreamSynchronize(c->stream));  // (the pinned staging of an earlier frame is free)
  memcpy(h, x, (size_t)nx * sizeof(double));  // (slot 0)
  if (divisors) memcpy(h + 2 * nx, divisors, (size_t)nx * sizeof(double));
  HIPCHECK(c, hipMemcpyAsync(d_solver, h, (size_t)(divisors ? 3 : 1) * nx * sizeof(double),
                             hipMemcpyHostToDevice, c->stream));
  fsdf::SolverState st;
  st.x = d_solver;
  st.div = divisors ? d_solver + 2 * nx : nullptr;
  st.Rb = d_solver + 3 * nx;
  st.f = st.Rb + 24 * nb;
  if (T.R > 0) {
    st.rbf = st.f + 1;
    st.prow = (int32_t*)(st.rbf + 2 * rbf_slot);
  }
  st.flags = c->solver_flags.get();
  st.rate = rate;
  st.max_step = max_step;
  st.tol = tolerance;
  st.n_points = n_points;
  st.weight = M.weight;
  st.limit = iteration_limit;
  HIPCHECK(c, hipMemsetAsync(st.flags, 0, 4 * sizeof(int), c->stream));
  // (the init and every step pose the next pass's model, c->pm, themselves:
  // the passes below launch no pose kernel)
  HIPCHECK(c, fsdf::launch_solver_init(c->stree, st, c->lm, c->pm, c->precision, c->stream));
  // (the init wrote the first pass's RBF rows; as it was again on every return but a frame's good end)
  struct RbfReady {
    fsdf_ctx* c;
    bool was, keep;
    ~RbfReady() {
      if (!keep) c->rbf_ready = was;
    }
  } rbf_rows{c, c->rbf_ready, false};
  if (T.R > 0) c->rbf_ready = true;
  HOST_STAMP(0);
  for (int it = 0; it < iteration_limit; ++it) {
    int rc = run_pass(c, nullptr, c->cur.pts.get(), c->n, c->model.accum.get(), nullptr, nullptr, nullptr, nullptr,
                      true, true, st.flags);
    if (rc) return rc;
    if (it == 0) {
      rc = iteration_regroup(c);
      if (rc) return rc;
    }
    HIPCHECK(c, fsdf::launch_solver_step(c->stree, st, c->model.accum.get(), c->lm, c->pm, c->precision, it,
                                         c->stream));
  }
  HOST_STAMP(1);
  HIPCHECK(c, hipMemcpyAsync(h, st.x, (size_t)2 * nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipMemcpyAsync(h + 3 * nx, st.f, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipMemcpyAsync(h + 3 * nx + 1, st.flags, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
#if FSDF_HOST_TIMES
  HOST_STAMP(2);
  fprintf(stderr, "device loop: enqueue %.1f us (%d iterations), then wait %.1f us\n", ht_1 - ht_0, iteration_limit,
          ht_2 - ht_1);
#endif
  int flags[4];
  memcpy(flags, h + 3 * nx + 1, sizeof flags);
#if FSDF_SOLVER_TIMES
  {
    unsigned long long tt[16];
    fsdf::solver_times(tt);
    fprintf(stderr, "solver step phases (10 ns):");
    for (int i = 1; i < 10; ++i) fprintf(stderr, " %lld", (long long)(tt[i] - tt[0]));
    fprintf(stderr, "\n");
  }
#endif
  memcpy(x, h + (size_t)(flags[1] & 1) * nx, (size_t)nx * sizeof(double));  // (the last iteration's slot)
  if (iterations_out) *iterations_out = flags[1];
  // (the steps wrote the passes' RBF rows themselves: those of the last posed x are on the device)
  rbf_rows.keep = !flags[2];
  if (flags[2] == 3) return fail(c, FSDF_ERR_DEGENERATE, "value_and_gradient: singular RBF system");
  if (flags[2] == 2) return fail(c, FSDF_ERR_ARG, "descend: poses not finite (configuration diverged)");
  if (flags[2]) return fail(c, FSDF_ERR_ARG, "descend: forward kinematics / chain rule (bad configuration)");
  if (value_out) *value_out = h[3 * nx];
  return FSDF_OK;
}

extern "C" int fsdf_set_solver(fsdf_ctx* c, int32_t device_loop) {
  if (!c) return FSDF_ERR_ARG;
  if (device_loop < 0 || device_loop > 4) return fail(c, FSDF_ERR_ARG, "set_solver: mode %d", device_loop);
  c->solver_device = device_loop;
  return FSDF_OK;
}

extern "C" int fsdf_descend(fsdf_ctx* c, double* x, int32_t iteration_limit, double rate, double max_step,
                            double tolerance, const double* divisors, double n_points, double* value_out,
                            int32_t* iterations_out) {
  if (!c) return FSDF_ERR_ARG;
  if (iterations_out) *iterations_out = 0;
  if (!x || iteration_limit < 0 || !(n_points > 0.0) || !std::isfinite(rate) || !(max_step >= 0.0))
    return fail(c, FSDF_ERR_ARG, "descend: bad arguments");
  if (c->mech.nb == 0) return fail(c, FSDF_ERR_STATE, "descend: no mechanism (call fsdf_set_mechanism)");
  const auto& Mc = c->mech;
  if ((int)Mc.surface_body.size() != c->lm.S || (int)Mc.poses.size() != 12 * c->lm.S)
    return fail(c, FSDF_ERR_STATE, "descend: mechanism registered for another surface list (call fsdf_set_mechanism)");
  // rigid scenes (no RBF skin, no deformation) iterate on the device when the
  // mechanism's tree and the step's work arrays fit the step's LDS (M64's 65
  // bodies: ~45 KB); scenes with RBF skins or deformations too in modes 3 / 4
  // (fsdf_set_solver), their skins' LU factors and work arrays counted. A
  // scene whose skins are not all declared, or name a deformation row that
  // does not exist, takes the host loop, which reports it.
  const bool rigid = c->lm.R == 0 && Mc.n_deform == 0;
  const bool required = c->solver_device == 2 || c->solver_device == 4;
  bool declared = (int)Mc.rbf.size() == c->lm.R || c->lm.R == 0;
  for (const auto& D : Mc.rbf) {
    declared = declared && D.n > 0;
    for (int j = 0; j < D.n; ++j) declared = declared && D.drow[j] < Mc.n_deform;
  }
  bool device_loop = c->solver_device && iteration_limit > 0 && (rigid || (c->solver_device >= 3 && declared)) &&
                     c->n > 0;
  if (device_loop && !c->solver_tree_ok) {
    HIPCHECK(c, hipSetDevice(c->device));
    const int rc = build_solver_tree(c);
    if (rc) return rc;
  }
  if (device_loop) {
    std::vector<int32_t> rbf_n;
    for (const auto& D : Mc.rbf) rbf_n.push_back(D.n);
    device_loop = fsdf::solver_fits(Mc.nb, Mc.nq + 3 * Mc.n_deform, c->lm.S, c->stree.ni, c->stree.nd, Mc.n_deform,
                                    (int)rbf_n.size(), rbf_n.data());
  }
  if (required && iteration_limit > 0 && !device_loop && (rigid || c->solver_device == 2 || declared))
    return fail(c, FSDF_ERR_STATE, "descend: the device loop was required (fsdf_set_solver %d) but the scene %s",
                c->solver_device,
                c->solver_device == 2 && !rigid ? "has RBF skins / deformations" :
                c->n == 0 ? "has no resident points" : "does not fit the solver step's LDS");
  if (device_loop)
    return descend_device(c, x, iteration_limit, rate, max_step, tolerance, divisors, n_points, value_out,
                          iterations_out);
  const int ns = c->mech.nq + 3 * c->mech.n_deform;
  std::vector<double> g(ns);
  double f = 0.0;
  int it = 0;
#if FSDF_HOST_TIMES
  for (double& v : g_host_t) v = 0.0;
  g_host_n = 0;
  const double ht_start = host_now_us();
#endif
  while (it < iteration_limit) {
    double cost = 0.0;
    const int rc = fsdf_value_and_gradient(c, x, &cost, g.data());
    if (rc) return rc;
    ++it;
    if (iterations_out) *iterations_out = it;
    f = cost / n_points;
    double nrm2 = 0.0;
    for (int i = 0; i < ns; ++i) {
      double gi = g[i] / n_points;
      if (divisors) gi = gi / divisors[i];
      g[i] = gi;
      nrm2 += gi * gi;
    }
    if (std::sqrt(nrm2) < tolerance) break;
    for (int i = 0; i < ns; ++i) x[i] = x[i] + std::min(std::max(-rate * g[i], -max_step), max_step);
  }
#if FSDF_HOST_TIMES
  if (g_host_n > 0) {
    const double span = host_now_us() - ht_start, k = (double)g_host_n;
    fprintf(stderr, "host loop per iteration (us): prepare %.2f launches %.2f wait %.2f chain %.2f total %.2f (%ld)\n",
            g_host_t[0] / k, g_host_t[1] / k, g_host_t[2] / k, g_host_t[3] / k, span / k, g_host_n);
  }
#endif
  if (value_out) *value_out = f;
  return FSDF_OK;
}

extern "C" int fsdf_eval_state_device(fsdf_ctx* c, const double* x, double* d_accum) {
  if (!c) return FSDF_ERR_ARG;
  if (!x || !d_accum) return fail(c, FSDF_ERR_ARG, "eval_state_device: null argument");
  int rc = iteration_prepare(c, x, "eval_state_device");
  if (rc) return rc;
  rc = run_pass(c, c->mech.poses.data(), c->cur.pts.get(), c->n, d_accum, nullptr, nullptr, nullptr, nullptr, true);
  if (rc) return rc;
  rc = iteration_regroup(c);
  if (rc) return rc;
  auto& M = c->mech;
  M.x_pass[M.x_pass_next] = M.x_prepared;
  M.x_pass_next ^= 1;
  return FSDF_OK;
}

extern "C" int fsdf_state_gradient(fsdf_ctx* c, const double* x, const double* accum, double* cost_out,
                                   double* grad_out) {
  if (!c) return FSDF_ERR_ARG;
  if (!x || !accum || !cost_out || !grad_out) return fail(c, FSDF_ERR_ARG, "state_gradient: null argument");
  auto& M = c->mech;
  const size_t nx = (size_t)M.nq + 3 * (size_t)M.n_deform;
  // the chain rule runs on the FK / weight solve of the pass that produced
  // accum; for an x other than the last prepared one (a pipelined earlier
  // pass) that host part is redone — the same arithmetic, the same bits
  if (M.nb == 0) return fail(c, FSDF_ERR_STATE, "state_gradient: no mechanism (call fsdf_set_mechanism)");
  auto same = [&](const std::vector<double>& v) {
    return v.size() == nx && memcmp(v.data(), x, nx * sizeof(double)) == 0;
  };
  if (!same(M.x_prepared)) {
    // an earlier pass of the ring: its FK / weight solve is redone (the same
    // arithmetic, the same bits); any other x cannot belong to an accumulator
    // of this context
    if (!same(M.x_pass[0]) && !same(M.x_pass[1]))
      return fail(c, FSDF_ERR_STATE,
                  "state_gradient: x is not the configuration of either of this context's last two "
                  "eval_state_device passes (nor the last prepared one)");
    const int rc = iteration_prepare(c, x, "state_gradient", false);
    if (rc) return rc;
  }
  return iteration_finish(c, x, accum, cost_out, grad_out, "state_gradient");
}
