// iterate.hip — one iteration of a registered mechanism: fsdf_set_mechanism, RBF
// centres and deformations, the host halves of one CostFunctor iteration
// (FK, weight solve, chain rule) around a pass, the same with the Gauss-Newton
// Hessian (fsdf_value_gradient_hessian; with fsdf_set_lm_skins also for scenes
// with RBF skins and deformations), and the device-split form
// (fsdf_eval_state_device, fsdf_state_gradient). The solver loops over them
// are in descend.hip.

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.h"
#include "kin_impl.h"

// after an iteration pass (value_and_gradient, eval_state_device, descend):
// the new cloud's first one regroups it when the auto rule says so
int iteration_regroup(fsdf_ctx* c) {
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
int iteration_prepare(fsdf_ctx* c, const double* x, const char* who, bool upload) {
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

int iteration_finish(fsdf_ctx* c, const double* x, const double* accum, double* cost_out, double* grad_out,
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

#if FSDF_HOST_TIMES
double g_host_t[8];  // (ctx.h: the host loop's clocks, printed by fsdf_descend)
long g_host_n;
#endif

// The Gauss-Newton matrix of a scene with skins and deformations (fsdf_set_lm_skins), from the hulls'
// moments hm [S][21] (a skin's row zero) and the skins' second moments sm: A = A_hulls in the nq
// block + Σ_r L_r M_r L_rᵀ over the nx = nq + 3 n_deform coordinates, H = 2 A + 2 weight I on the
// deformations (the regulariser is a sum of squares too, and is not robustified)
static int skins_hessian(fsdf_ctx* c, const double* x, const double* hm, const double* sm, double* hess_out,
                         const char* who) {
  auto& M = c->mech;
  const int nq = M.nq, nx = nq + 3 * M.n_deform, S = c->lm.S;
  M.gn_work.resize((size_t)36 * M.nb + (size_t)6 * nq);
  M.gn_hull.resize((size_t)nq * nq);
  int rc = fsdf_gauss_newton_matrix(M.nb, M.parent.data(), M.kind.data(), M.qoff.data(), M.axis.data(), M.Rb.data(),
                                    M.tb.data(), x, S, M.surface_body.data(), hm, nq, M.gn_work.data(),
                                    M.gn_hull.data());
  if (rc) return fail(c, rc, "%s: Gauss-Newton matrix", who);
  for (size_t i = 0; i < (size_t)nx * nx; ++i) hess_out[i] = 0.0;
  for (int i = 0; i < nq; ++i)
    for (int j = 0; j < nq; ++j) hess_out[(size_t)i * nx + j] = M.gn_hull[(size_t)i * nq + j];
  for (auto& D : M.rbf) {
    const int m = 4 * D.n + 4;
    M.skin_L.resize((size_t)nx * m);
    M.skin_work.resize(std::max((size_t)8 * D.n + 8 + (size_t)12 * M.nb + nx, (size_t)nx * m));
    rc = fsdf_rbf_state_map(M.nb, M.parent.data(), M.kind.data(), M.qoff.data(), M.axis.data(), M.R.data(),
                            M.Rb.data(), M.tb.data(), x, nq, D.n, D.centres.data(), D.u.data(), D.lu.data(),
                            D.piv.data(), D.body.data(), D.drow.data(), M.n_deform, M.skin_work.data(),
                            M.skin_L.data());
    if (!rc) rc = fsdf_gauss_newton_add(nx, m, M.skin_L.data(), sm, M.skin_work.data(), hess_out);
    if (rc) return fail(c, rc, "%s: the skins' Gauss-Newton term", who);
    sm += (size_t)m * m;
  }
  for (size_t i = 0; i < (size_t)nx * nx; ++i) hess_out[i] = 2.0 * hess_out[i];
  for (int i = nq; i < nx; ++i) hess_out[(size_t)i * nx + i] += 2.0 * M.weight;
  return FSDF_OK;
}

// With a loss other than SQUARE set (fsdf_set_loss), per-point weights
// (fsdf_set_point_weights) or a free-space split (fsdf_set_free_split; both
// also under SQUARE): the same iteration on the
// robust objective Σρ(d*) — the pass with k*, d*, ∇d* in resident order, the
// robust launch (robust.hip) in place of the pass's own sums, and the same
// chain rule on the accumulator assembled from its rows. The auto regroup is
// queued after the robust launch: it reads the layout the pass ran on. Rigid
// scenes only — with fsdf_set_robust_skins scenes with RBF skins and deformations too: the skins'
// blocks come from robust_skin.hip, the Hessian (fsdf_set_lm_skins as well) from the robust hull
// moments and the weighted skin moments through the non-rigid branch's own arithmetic.
// hess_out null: the rows without the moments (the same (c, g) bits).
static int robust_iteration(fsdf_ctx* c, const double* x, double* cost_out, double* grad_out, double* hess_out,
                            const char* who) {
  const bool rigid = c->lm.R == 0 && c->mech.n_deform == 0;
  if (!rigid && !c->robust_skins)
    return fail(c, FSDF_ERR_STATE,
                "%s: the loss set by fsdf_set_loss (kind %d)%s%s serves rigid scenes (no RBF skin, no deformation)", who,
                c->loss_kind, c->conf_set ? " and the weights of fsdf_set_point_weights" : "",
                c->free_split >= 0 ? " and the free-space split of fsdf_set_free_split" : "");
  if (!rigid && hess_out && !c->lm_skins)
    return fail(c, FSDF_ERR_STATE,
                "%s: the Gauss-Newton matrix is defined for rigid scenes (no RBF skin, no deformation); "
                "fsdf_set_lm_skins serves the others", who);
  int rc = iteration_prepare(c, x, who);
  if (rc) return rc;
  auto& M = c->mech;
  const bool moments = hess_out != nullptr;
  rc = run_pass_robust(c, M.poses.data(), who, moments);
  if (rc) return rc;
  rc = iteration_regroup(c);  // (stream-ordered after the pass and the robust launch: the sync below covers it)
  if (rc) return rc;
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  robust_rows_finish(c, moments);
  rc = iteration_finish(c, x, c->robust_accum.data(), cost_out, grad_out, who);
  if (rc || !moments) return rc;
  if (!rigid)  // (robust_moments: a skin's row zero; h_skin_moments: Σ aw j jᵀ, or untouched with no skin)
    return skins_hessian(c, x, c->robust_moments.data(), c->h_skin_moments.get(), hess_out, who);
  const int nq = M.nq;
  M.gn_work.resize((size_t)36 * M.nb + (size_t)6 * nq);
  rc = fsdf_gauss_newton_matrix(M.nb, M.parent.data(), M.kind.data(), M.qoff.data(), M.axis.data(), M.Rb.data(),
                                M.tb.data(), x, c->lm.S, M.surface_body.data(), c->robust_moments.data(), nq,
                                M.gn_work.data(), hess_out);
  if (rc) return fail(c, rc, "%s: Gauss-Newton matrix", who);
  for (size_t i = 0; i < (size_t)nq * nq; ++i) hess_out[i] = 2.0 * hess_out[i];
  return FSDF_OK;
}

static int robust_value_and_gradient(fsdf_ctx* c, const double* x, double* cost_out, double* grad_out) {
  return robust_iteration(c, x, cost_out, grad_out, nullptr, "value_and_gradient");
}

extern "C" int fsdf_value_and_gradient(fsdf_ctx* c, const double* x, double* cost_out, double* grad_out) {
  if (!c) return FSDF_ERR_ARG;
  HOST_STAMP(0);
  if (!x || !cost_out || !grad_out) return fail(c, FSDF_ERR_ARG, "value_and_gradient: null argument");
  if (robust_objective(c)) return robust_value_and_gradient(c, x, cost_out, grad_out);
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
  if (robust_objective(c))
    return robust_iteration(c, x, cost_out, grad_out, hess_out, "value_gradient_hessian");
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
  // skins and deformations (fsdf_set_lm_skins)
  double* hm = c->h_moments.get();
  for (int k = 0; k < c->lm.S; ++k)  // (a skin's points have no hull moments)
    if (c->h_surface_kind[k] != FSDF_SURFACE_HULL)
      for (int e = 0; e < fsdf::kMomentsLen; ++e) hm[(size_t)fsdf::kMomentsLen * k + e] = 0.0;
  return skins_hessian(c, x, hm, c->h_skin_moments.get(), hess_out, "value_gradient_hessian");
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
