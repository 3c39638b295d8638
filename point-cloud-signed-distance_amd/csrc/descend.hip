// descend.hip — the solver loops over the iterations of iterate.hip:
// fsdf_descend (estimate_state's NaiveSolver loop) on the host or — the tree
// of build_solver_tree, descend_device — with every iteration on the device
// (solver.hip), and fsdf_descend_lm (Levenberg-Marquardt over
// fsdf_value_gradient_hessian, with the prior of fsdf_set_lm_prior) on the host
// or — fsdf_set_lm_solver, descend_lm_device — on the device (lm_solver.hip).

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ctx.h"

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
  // The blob: the doubles, then the ints, each array appended where its offset
  // is written into T (SolverTree, fsdf_internal.h).
  fsdf::SolverTree T;
  std::vector<int32_t> iv;
  std::vector<double> dv;
  auto ints = [&](int& at, const std::vector<int32_t>& v) {
    at = (int)iv.size();
    iv.insert(iv.end(), v.begin(), v.end());
  };
  auto doubles = [&](int& at, const std::vector<double>& v) {
    at = (int)dv.size();
    dv.insert(dv.end(), v.begin(), v.end());
  };
  ints(T.parent, M.parent);
  ints(T.kind, M.kind);
  ints(T.qoff, M.qoff);
  ints(T.path_list, dord);
  ints(T.path_off, doff);
  ints(T.height_order, hord);
  ints(T.height_off, hoff);
  ints(T.child_off, coff);
  ints(T.child_list, clist);
  ints(T.surf_off, soff);
  ints(T.surf_list, slist);
  ints(T.surface_body, M.surface_body);
  ints(T.chain_list, dlist);
  ints(T.chain_off, dof);
  ints(T.rbf_n, rn);
  ints(T.rbf_coff, rcoff);
  ints(T.rbf_luoff, rluoff);
  ints(T.rbf_body, rbody);
  ints(T.rbf_drow, rdrow);
  doubles(T.axis, M.axis);
  doubles(T.AR, M.AR);
  doubles(T.At, M.At);
  doubles(T.BR, M.BR);
  doubles(T.Bt, M.Bt);
  doubles(T.frame_R, M.frame_R);
  doubles(T.frame_t, M.frame_t);
  doubles(T.rbf_local, rlocal);
  doubles(T.rbf_values, rvalues);
  T.nb = nb;
  T.nx = M.nq + 3 * M.n_deform;
  T.nq = M.nq;
  T.S = S;
  T.D = D;
  T.H = H;
  T.narrow = 6 * widest <= 64;
  T.chains = chains;
  T.R = (int)rn.size();
  T.n_deform = M.n_deform;
  T.rc = rcoff.back();
  T.rm = T.rc + 4 * T.R;
  T.rlu = rluoff.back();
  T.racc = 4 * T.rc + 4 * T.R;
  T.ni = (int)iv.size();
  T.nd = (int)dv.size();
  const size_t bytes = dv.size() * sizeof(double) + iv.size() * sizeof(int32_t);
  const size_t chunks = (bytes + 15) / 16;
  T.chunks16 = (int)chunks;
  std::vector<char> blob(chunks * 16, 0);
  memcpy(blob.data(), dv.data(), dv.size() * sizeof(double));
  memcpy(blob.data() + dv.size() * sizeof(double), iv.data(), iv.size() * sizeof(int32_t));
  HIPCHECK(c, hipStreamSynchronize(c->stream));  // (a previous frame's steps may still read the old arrays)
  c->stree_blob.reset();
  HIPCHECK(c, c->stree_blob.reserve(std::max<size_t>(blob.size(), 16) / sizeof(double)));
  HIPCHECK(c, hipMemcpy(c->stree_blob.get(), blob.data(), blob.size(), hipMemcpyHostToDevice));
  T.blob = c->stree_blob.get();
  c->stree = T;
  c->solver_tree_ok = true;
  return FSDF_OK;
}

// the opening checks of fsdf_descend and fsdf_descend_lm (gain: the rate / the
// damping; rigid_only: the scene has skins or deformations the loop does not serve)
static int descend_checks(fsdf_ctx* c, const char* who, const double* x, int32_t iteration_limit, double gain,
                          double max_step, double n_points, bool rigid_only) {
  if (!x || iteration_limit < 0 || !(n_points > 0.0) || !std::isfinite(gain) || !(max_step >= 0.0))
    return fail(c, FSDF_ERR_ARG, "%s: bad arguments", who);
  if (c->mech.nb == 0) return fail(c, FSDF_ERR_STATE, "%s: no mechanism (call fsdf_set_mechanism)", who);
  if (rigid_only)
    return fail(c, FSDF_ERR_STATE, "%s: rigid scenes only (no RBF skin, no deformation)%s", who,
                c->free_split >= 0 ? "; a free-space split is set (fsdf_set_free_split)" : "");
  if ((int)c->mech.surface_body.size() != c->lm.S || (int)c->mech.poses.size() != 12 * c->lm.S)
    return fail(c, FSDF_ERR_STATE, "%s: mechanism registered for another surface list (call fsdf_set_mechanism)", who);
  return FSDF_OK;
}

// fsdf_descend for rigid scenes, every iteration on the device: solver_init
// (FK of x0 -> poses), then per iteration pose -> pass -> reduce -> solver
// step, all enqueued up front; one read-back of x, f and the count at the end.
// Bit-identical to the host loop below (solver.hip).
// Under a robust objective (fsdf_set_robust_loops, rigid scenes): pose -> pass
// (k*, d*, ∇d*) -> reduce -> robust sums -> their reduce -> assembly -> solver
// step; the regrouped layout's permutation and weights are read again after the
// first evaluation's regroup, where the host loop's next evaluation gets them.
static int descend_device(fsdf_ctx* c, double* x, int32_t iteration_limit, double rate, double max_step,
                          double tolerance, const double* divisors, double n_points, double* value_out,
                          int32_t* iterations_out) {
  auto& M = c->mech;
  const int nx = M.nq + 3 * M.n_deform;  // (the state: joint coordinates, then the deformations)
  HIPCHECK(c, hipSetDevice(c->device));
  if (!c->solver_tree_ok) {
    const int rc = build_solver_tree(c);
    if (rc) return rc;
  }
  // (the layouts of the device state and the pinned staging: fsdf_internal.h, next to SolverState)
  const fsdf::SolverTree& T = c->stree;
  const size_t need = fsdf::carve_solver_state(T, divisors != nullptr, nullptr, nullptr);
  const fsdf::SolverStaging hs = fsdf::solver_staging(nx, divisors != nullptr);
  if (c->solver.capacity() < need) HIPCHECK(c, hipStreamSynchronize(c->stream));
  HIPCHECK(c, c->solver.reserve(need));
  HIPCHECK(c, c->solver_flags.reserve(4));
  HIPCHECK(c, c->h_solver.reserve(hs.total));
  // A robust objective (fsdf_set_robust_loops; fsdf_descend admits rigid scenes alone): the pass
  // also writes k*, d*, ∇d* in resident order, the robust launch (robust.hip, rows of 8) sums
  // them and the assembly writes the accumulator the step reads — in place of the pass's own,
  // which still goes to c->model.accum. The rule of device_buffers.h: reserved here, the
  // pointers read below, the launches take the locals.
  const bool robust = robust_objective(c);
  const int64_t n = c->n;
  const int S = c->lm.S;
  if (robust) {
    const int rc = ensure_outputs(c, n);
    if (rc) return rc;
    HIPCHECK(c, c->robust_partials.reserve(fsdf::robust_partials_len(n, S)));
    HIPCHECK(c, c->robust_rows.reserve((size_t)S * fsdf::kRobustLen));
    HIPCHECK(c, c->robust_dev_accum.reserve((size_t)1 + 6 * (size_t)S));
  }
  int32_t* d_kstar = robust ? c->kstar.get() : nullptr;
  double* d_d = robust ? c->d.get() : nullptr;
  double* d_grad = robust ? c->grad.get() : nullptr;
  double* d_rpartials = c->robust_partials.get();
  double* d_rows = c->robust_rows.get();
  double* d_step_accum = robust ? c->robust_dev_accum.get() : c->model.accum.get();
  const int32_t* d_perm = c->cur.perm.get();
  // (the per-point weights in resident order, regathered when the layout changed since; null: none set)
  const double* d_conf = nullptr;
  if (robust) {
    const int rc = point_weights_resident(c, &d_conf);
    if (rc) return rc;
  }
  double* h = c->h_solver.get();
  double* d_solver = c->solver.get();
  HIPCHECK(c, hipStreamSynchronize(c->stream));  // (the pinned staging of an earlier frame is free)
  memcpy(h, x, (size_t)nx * sizeof(double));  // (slot 0)
  if (divisors) memcpy(h + hs.div, divisors, (size_t)nx * sizeof(double));
  HIPCHECK(c, hipMemcpyAsync(d_solver, h, hs.up * sizeof(double), hipMemcpyHostToDevice, c->stream));
  fsdf::SolverState st;
  fsdf::carve_solver_state(T, divisors != nullptr, d_solver, &st);
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
    int rc = run_pass(c, nullptr, c->cur.pts.get(), c->n, c->model.accum.get(), d_kstar, d_d, d_grad, nullptr,
                      true, true, st.flags);
    if (rc) return rc;
    if (robust) {  // (before the regroup: the launch reads the layout the pass ran on)
      HIPCHECK(c, fsdf::launch_robust(c->precision, false, c->cur.pts.get(), d_kstar, d_d, d_grad, d_conf, d_perm,
                                      c->free_split, n, S, c->loss_kind, c->loss_scale, d_rpartials, d_rows,
                                      c->stream, st.flags));
      HIPCHECK(c, fsdf::launch_robust_assemble(false, d_rows, c->lm.surface_kind, S, d_step_accum, nullptr,
                                               c->stream, st.flags));
    }
    if (it == 0) {
      rc = iteration_regroup(c);
      if (rc) return rc;
      if (robust) {  // (the regrouped layout's permutation and weights, as the host loop's next evaluation)
        d_perm = c->cur.perm.get();
        rc = point_weights_resident(c, &d_conf);
        if (rc) return rc;
      }
    }
    HIPCHECK(c, fsdf::launch_solver_step(c->stree, st, d_step_accum, c->lm, c->pm, c->precision, it, c->stream));
  }
  HOST_STAMP(1);
  HIPCHECK(c, hipMemcpyAsync(h, st.x, (size_t)2 * nx * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipMemcpyAsync(h + hs.f, st.f, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipMemcpyAsync(h + hs.flags, st.flags, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
#if FSDF_HOST_TIMES
  HOST_STAMP(2);
  fprintf(stderr, "device loop: enqueue %.1f us (%d iterations), then wait %.1f us\n", ht_1 - ht_0, iteration_limit,
          ht_2 - ht_1);
#endif
  int flags[4];
  memcpy(flags, h + hs.flags, sizeof flags);
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
  if (value_out) *value_out = h[hs.f];
  return FSDF_OK;
}

extern "C" int fsdf_set_solver(fsdf_ctx* c, int32_t device_loop) {
  if (!c) return FSDF_ERR_ARG;
  if (device_loop < 0 || device_loop > 4) return fail(c, FSDF_ERR_ARG, "set_solver: mode %d", device_loop);
  c->solver_device = device_loop;
  return FSDF_OK;
}

// The solver loop of estimate_state (src/tracking.jl:16-26 with the
// NaiveSolver restated in flash/tracking.py) around fsdf_value_and_gradient,
// without a host-language round trip per iteration: f = c/n, g = (∂c/∂x / n)
// ./ divisors; stop when |g| < tolerance; else x += clamp(-rate g, ±max_step).
extern "C" int fsdf_descend(fsdf_ctx* c, double* x, int32_t iteration_limit, double rate, double max_step,
                            double tolerance, const double* divisors, double n_points, double* value_out,
                            int32_t* iterations_out) {
  if (!c) return FSDF_ERR_ARG;
  if (iterations_out) *iterations_out = 0;
  if (const int rc = descend_checks(c, "descend", x, iteration_limit, rate, max_step, n_points, false)) return rc;
  const auto& Mc = c->mech;
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
  // A loss other than SQUARE (fsdf_set_loss) is served by the host loop alone
  // (the device step reads the pass's least-squares accumulator).
  // Per-point weights (fsdf_set_point_weights) and a free-space split (fsdf_set_free_split) likewise.
  // fsdf_set_robust_loops admits them to the device loop on hull-only rigid scenes whose robust
  // table fits (descend_device: the robust launch and the assembly feed the step); scenes with RBF
  // skins or deformations keep the host loop under a robust objective (modes 3 / 4 as well).
  const bool loss = robust_objective(c);
  // (robust_fit holds up to 282 surfaces and fsdf_set_surfaces admits 256: with that limit the
  // table always fits, and the refusal that names it below is not reachable today)
  const bool robust_dev = loss && c->robust_loops && rigid && fsdf::robust_fit(c->lm.S);
  if (loss && !robust_dev && c->robust_loops && required && iteration_limit > 0)
    return fail(c, FSDF_ERR_STATE,
                "descend: the device loop was required (fsdf_set_solver %d) under a robust objective "
                "(fsdf_set_robust_loops) but the scene %s",
                c->solver_device,
                !rigid ? "has RBF skins / deformations (the robust device loops serve hull-only rigid scenes)" :
                         "has more surfaces than the robust table's LDS holds (at most 282)");
  if (loss && !robust_dev && required && iteration_limit > 0)
    return fail(c, FSDF_ERR_STATE,
                "descend: the device loop was required (fsdf_set_solver %d) but %s (the host loop serves it)",
                c->solver_device,
                c->free_split >= 0 ? "a free-space split is set (fsdf_set_free_split)" :
                c->conf_set ? "per-point weights are set (fsdf_set_point_weights)" :
                c->loss_kind == FSDF_LOSS_HUBER ? "a loss is set (fsdf_set_loss kind 1)" :
                                                  "a loss is set (fsdf_set_loss kind 2)");
  bool device_loop = c->solver_device && iteration_limit > 0 && (rigid || (c->solver_device >= 3 && declared)) &&
                     c->n > 0 && (!loss || robust_dev);
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

// fsdf_descend_lm with every evaluation on the device (lm_solver.hip): solver_init (FK of x -> the first posed model),
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
// Under a robust objective (fsdf_set_robust_loops): the pass also writes d*, the
// robust launch (robust.hip, rows of 29) stands where the moments launch does,
// and the assembly writes an accumulator and moments of the robust path's own,
// which the unchanged step reads; the pass's least-squares accumulator still
// goes to c->model.accum and is not read. After the regroup the permutation
// and the weights are read again too (point_weights_resident enqueues the
// regather of stale weights): where the host loop's next evaluation gets them.
static int descend_lm_device(fsdf_ctx* c, double* x, int32_t iteration_limit, double damping, double max_step,
                             double tolerance, double n_points, double* value_out, int32_t* iterations_out,
                             double* damping_out) {
  auto& M = c->mech;
  const int nq = M.nq, nb = M.nb, S = c->lm.S;
  const int64_t n = c->n;
  const bool prior = !c->lm_prior.empty();
  const fsdf::SolverTree& T = c->stree;
  if (damping_out) *damping_out = damping;  // (fsdf_lm_minimize's first line: also what a failed first evaluation leaves)
  // (the layout of the state, its uploaded and read-back spans: fsdf_internal.h, next to LmState)
  const fsdf::LmSpans sp = fsdf::carve_lm_state(nb, nq, prior, nullptr, nullptr);
  const size_t need = sp.need, up = sp.up, back = sp.back;
  // (1) reserve
  int rc = ensure_outputs(c, n);
  if (rc) return rc;
  HIPCHECK(c, c->moments_partials.reserve(fsdf::moments_partials_len(n, S)));
  HIPCHECK(c, c->moments.reserve((size_t)S * fsdf::kMomentsLen));
  const bool robust = robust_objective(c);
  if (robust) {
    HIPCHECK(c, c->robust_partials.reserve(fsdf::robust_partials_len(n, S)));
    HIPCHECK(c, c->robust_rows.reserve((size_t)S * fsdf::kRobustLen));
    HIPCHECK(c, c->robust_dev_accum.reserve((size_t)1 + 6 * (size_t)S));
    HIPCHECK(c, c->robust_dev_moments.reserve((size_t)S * fsdf::kMomentsLen));
  }
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
  double* d_d = robust ? c->d.get() : nullptr;
  double* d_rpartials = c->robust_partials.get();
  double* d_rows = c->robust_rows.get();
  // (what the step reads: the robust path's own pair, or the pass's accumulator and the moments kernel's sums)
  double* d_step_accum = robust ? c->robust_dev_accum.get() : d_accum;
  double* d_step_moments = robust ? c->robust_dev_moments.get() : d_moments;
  const int32_t* d_perm = c->cur.perm.get();
  // (the per-point weights in resident order, regathered when the layout changed since; null: none set)
  const double* d_conf = nullptr;
  if (robust) {
    rc = point_weights_resident(c, &d_conf);
    if (rc) return rc;
  }
  double* d = c->solver.get();
  double* h = c->h_solver.get();
  HIPCHECK(c, hipStreamSynchronize(c->stream));  // (the pinned staging of an earlier frame is free)
  memset(h, 0, up * sizeof(double));
  memcpy(h, x, (size_t)nq * sizeof(double));  // (trial 0)
  memcpy(h + sp.ref, x, (size_t)nq * sizeof(double));
  if (prior) memcpy(h + sp.mu, c->lm_prior.data(), (size_t)nq * sizeof(double));
  h[sp.lam] = damping;
  fsdf::LmState ls;
  fsdf::carve_lm_state(nb, nq, prior, d, &ls);
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
    rc = run_pass(c, nullptr, d_pts, n, d_accum, d_kstar, d_d, d_grad, nullptr, true, true, ls.flags);
    if (rc) return rc;
    if (robust) {
      HIPCHECK(c, fsdf::launch_robust(c->precision, true, d_pts, d_kstar, d_d, d_grad, d_conf, d_perm, c->free_split,
                                      n, S, c->loss_kind, c->loss_scale, d_rpartials, d_rows, c->stream, ls.flags));
      HIPCHECK(c, fsdf::launch_robust_assemble(true, d_rows, c->lm.surface_kind, S, d_step_accum, d_step_moments,
                                               c->stream, ls.flags));
    } else {
      HIPCHECK(c, fsdf::launch_moments(c->precision, d_pts, d_kstar, d_grad, n, S, d_partials, d_moments, c->stream,
                                       ls.flags));
    }
    if (it == 0) {  // (after the moments / robust launch: they read the layout the pass ran on)
      rc = iteration_regroup(c);
      if (rc) return rc;
      d_pts = c->cur.pts.get();
      if (robust) {
        d_perm = c->cur.perm.get();
        rc = point_weights_resident(c, &d_conf);
        if (rc) return rc;
      }
    }
    HIPCHECK(c, fsdf::launch_lm_step(T, ls, d_step_accum, d_step_moments, it, c->stream));
    if (it + 1 < iteration_limit)
      HIPCHECK(c, fsdf::launch_lm_pose(T, ls, c->lm, c->pm, c->precision, (it + 1) & 1, c->stream));
  }
  double* hb = h + up;  // lam | flags | f | xa
  HIPCHECK(c, hipMemcpyAsync(hb, ls.lam, back * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHECK(c, hipStreamSynchronize(c->stream));
  int flags[4];
  memcpy(flags, hb + sp.b_flags, sizeof flags);
#if FSDF_SOLVER_TIMES
  {
    unsigned long long tt[16];
    fsdf::lm_solver_times(tt);
    fprintf(stderr, "LM step phases of evaluation 5 (10 ns):");
    for (int i = 1; i < 10; ++i) fprintf(stderr, " %lld", (long long)(tt[i] - tt[0]));
    fprintf(stderr, "\n");
  }
#endif
  if (iterations_out) *iterations_out = flags[1];
  if (flags[1] > 0) {  // (as the host loop: x the last accepted point, also when a later evaluation failed)
    memcpy(x, hb + sp.b_xa, (size_t)nq * sizeof(double));
    if (damping_out) *damping_out = hb[0];
    if (value_out) *value_out = hb[sp.b_f];
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
  const bool rigid = c->lm.R == 0 && c->mech.n_deform == 0;
  if (const int rc = descend_checks(c, "descend_lm", x, iteration_limit, damping, max_step, n_points,
                                    !rigid && !c->lm_skins))
    return rc;
  const auto& Mc = c->mech;
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
  // A loss other than SQUARE (fsdf_set_loss): the host loop alone (mode 1 takes it, mode 2 is refused).
  // Per-point weights (fsdf_set_point_weights) and a free-space split (fsdf_set_free_split) likewise.
  // fsdf_set_robust_loops admits them on hull-only rigid scenes whose robust table fits
  // (descend_lm_device: the robust launch and the assembly feed the step).
  const bool loss = robust_objective(c);
  // (a non-rigid scene in the required mode was refused above; robust_fit cannot fail under
  // fsdf_set_surfaces' limit of 256 surfaces, so the refusal below is not reachable today)
  const bool robust_dev = loss && c->robust_loops && rigid && fsdf::robust_fit(c->lm.S);
  if (loss && !robust_dev && c->robust_loops && c->lm_solver_device == 2)
    return fail(c, FSDF_ERR_STATE,
                "descend_lm: the device loop was required (fsdf_set_lm_solver 2) under a robust objective "
                "(fsdf_set_robust_loops) but the scene has more surfaces than the robust table's LDS holds (at most 282)");
  if (loss && !robust_dev && c->lm_solver_device == 2)
    return fail(c, FSDF_ERR_STATE, "descend_lm: the device loop was required (fsdf_set_lm_solver 2) but %s "
                                   "(loss kind %d: the host loop serves it)",
                c->free_split >= 0 ? "a free-space split is set (fsdf_set_free_split)" :
                c->conf_set ? "per-point weights are set (fsdf_set_point_weights)" : "a loss is set (fsdf_set_loss)",
                c->loss_kind);
  if (rigid && c->lm_solver_device && iteration_limit > 0 && (!loss || robust_dev)) {
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
                    fsdf::lm_solver_fits(Mc.nb, nq, c->lm.S, c->stree.ni, c->stree.nd);
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
