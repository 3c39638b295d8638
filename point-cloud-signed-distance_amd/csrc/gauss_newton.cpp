// gauss_newton.cpp — host side of the second-order tracking solver (no device):
// the Gauss-Newton matrix of the mechanism from the per-surface second moments
// of the residual, one damped (Levenberg-Marquardt) step, and the loop over it
// (fsdf_lm_minimize); for RBF skins the term L M Lᵀ of one skin
// (fsdf_gauss_newton_add).
//
// For a point p on a surface of body b, ∂d*(p)/∂x_i = s_i · w_p, with w_p =
// (∇d*, p × ∇d*) and s_i the motion row of joint coordinate i — the row the
// chain rule (kin_impl.h joint_gradient) contracts a wrench with — when i's
// joint is b's or an ancestor's, and 0 otherwise. s_i depends on the joint
// alone, so with M_k = Σ w wᵀ per surface
//
//   A = JᵀJ = Σ_k S_b(k) M_k S_b(k)ᵀ,   A_ij = s_iᵀ C_deeper(i, j) s_j
//
// where C_b sums M_k over the surfaces of b's subtree and deeper(i, j) is the
// deeper of the two joints' bodies when one is the other's ancestor (A_ij = 0
// when neither is): per-body sums, subtree sums (children before parents),
// then every coordinate against the coordinates on its path to the root.

#include <math.h>
#include <stdint.h>

#include "flashsdf.h"
#include "gn_impl.h"

// The per-element arithmetic is gn_impl.h's (the device LM loop, lm_solver.hip,
// runs the same functions in parallel): here the sequential loops over it.
using fsdf::gn::joint_rows;
using fsdf::gn::joint_width;

extern "C" int fsdf_gauss_newton_matrix(int32_t nb, const int32_t* parent, const int32_t* kind, const int32_t* qoff,
                                        const double* axis, const double* Rb, const double* tb, const double* q,
                                        int32_t nsurf, const int32_t* surface_body, const double* moments, int32_t nq,
                                        double* work, double* A_out) {
  if (nb < 1 || nq < 0 || !parent || !kind || !qoff || !axis || !Rb || !tb || !q || !work || (nq > 0 && !A_out) ||
      nsurf < 0 || (nsurf > 0 && (!surface_body || !moments)))
    return FSDF_ERR_ARG;
  double* C = work;                        // [nb][36] subtree moment sums
  double* rows = work + (size_t)36 * nb;   // [nq][6] motion rows by coordinate
  for (size_t i = 0; i < (size_t)36 * nb; ++i) C[i] = 0.0;
  for (size_t i = 0; i < (size_t)6 * nq; ++i) rows[i] = 0.0;
  for (size_t i = 0; i < (size_t)nq * nq; ++i) A_out[i] = 0.0;
  for (int k = 0; k < nsurf; ++k) {
    const int b = surface_body[k];
    if (b < 0) continue;
    if (b >= nb) return FSDF_ERR_ARG;
    const double* M = moments + 21 * k;
    double* Cb = C + 36 * b;
    int e = 0;
    for (int i = 0; i < 6; ++i)
      for (int j = i; j < 6; ++j, ++e) {
        Cb[6 * i + j] += M[e];
        if (j != i) Cb[6 * j + i] += M[e];
      }
  }
  for (int b = nb - 1; b >= 1; --b) {
    const int p = parent[b];
    if (p < 0 || p >= b) return FSDF_ERR_ARG;  // topological order required
    for (int j = 0; j < 36; ++j) C[36 * p + j] += C[36 * b + j];
  }
  for (int b = 1; b < nb; ++b) {
    const int w = joint_width(kind[b]);
    if (kind[b] < 0 || kind[b] > 2 || (w && (qoff[b] < 0 || qoff[b] + w > nq))) return FSDF_ERR_ARG;
    if (w && !joint_rows(kind[b], axis + 3 * b, Rb + 9 * b, tb + 3 * b, q + qoff[b], rows + 6 * qoff[b]))
      return FSDF_ERR_ARG;
  }
  for (int b = 1; b < nb; ++b) {
    const int wb = joint_width(kind[b]);
    const double* Cb = C + 36 * b;
    for (int dj = 0; dj < wb; ++dj) {
      const int cj = qoff[b] + dj;
      const double* sj = rows + 6 * cj;
      double u[6];
      for (int i = 0; i < 6; ++i) u[i] = fsdf::gn::moment_row(Cb, sj, i);
      for (int a = b; a >= 1; a = parent[a]) {
        const int wa = a == b ? dj + 1 : joint_width(kind[a]);  // own joint: the upper triangle, mirrored
        for (int di = 0; di < wa; ++di) {
          const int ci = qoff[a] + di;
          const double* si = rows + 6 * ci;
          const double s = fsdf::gn::row_dot(si, u);
          A_out[(size_t)ci * nq + cj] = s;
          A_out[(size_t)cj * nq + ci] = s;
        }
      }
    }
  }
  return FSDF_OK;
}

// A += L M Lᵀ for one RBF skin (L from fsdf_rbf_state_map, M its second
// moment, skin_moments.hip): T = L M, then the upper triangle of T Lᵀ is added
// to A's and mirrored, so A is exactly symmetric whatever rounding M carries.
extern "C" int fsdf_gauss_newton_add(int32_t nx, int32_t m, const double* L, const double* M, double* work,
                                     double* A) {
  if (nx < 0 || m < 0 || ((nx > 0 && m > 0) && (!L || !M || !work)) || (nx > 0 && !A)) return FSDF_ERR_ARG;
  double* T = work;  // [nx][m]
  for (int i = 0; i < nx; ++i)
    for (int k = 0; k < m; ++k) {
      double s = 0.0;
      for (int l = 0; l < m; ++l) s += L[(size_t)i * m + l] * M[(size_t)l * m + k];
      T[(size_t)i * m + k] = s;
    }
  for (int i = 0; i < nx; ++i)
    for (int j = i; j < nx; ++j) {
      double s = 0.0;
      for (int k = 0; k < m; ++k) s += T[(size_t)i * m + k] * L[(size_t)j * m + k];
      const double a = A[(size_t)i * nx + j] + s;
      A[(size_t)i * nx + j] = a;
      A[(size_t)j * nx + i] = a;
    }
  return FSDF_OK;
}

extern "C" int fsdf_lm_step(int32_t n, const double* H, const double* g, double lambda, double max_step, double* work,
                            double* dx_out) {
  if (n < 0 || (n > 0 && (!H || !g || !work || !dx_out))) return FSDF_ERR_ARG;
  double* L = work;                    // [n][n], lower triangle
  double* y = work + (size_t)n * n;    // [n]
  double hmax = 0.0;
  for (int i = 0; i < n; ++i) hmax = fsdf::gn::diag_max(hmax, H[(size_t)i * n + i]);
  const double floor_d = 1e-12 * hmax;
  for (int j = 0; j < n; ++j) {
    // max(H_jj, 1e-12 max H) (a NaN H_jj meets the pivot test)
    double p = fsdf::gn::damped_diagonal(H[(size_t)j * n + j], lambda, floor_d);
    for (int k = 0; k < j; ++k) p = fsdf::gn::minus_product(p, L[(size_t)j * n + k], L[(size_t)j * n + k]);
    if (fsdf::gn::bad_pivot(p)) return FSDF_ERR_DEGENERATE;
    const double ljj = sqrt(p);
    L[(size_t)j * n + j] = ljj;
    for (int i = j + 1; i < n; ++i) {
      double s = H[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) s = fsdf::gn::minus_product(s, L[(size_t)i * n + k], L[(size_t)j * n + k]);
      L[(size_t)i * n + j] = s / ljj;
    }
  }
  for (int i = 0; i < n; ++i) {  // L y = g
    double s = g[i];
    for (int k = 0; k < i; ++k) s = fsdf::gn::minus_product(s, L[(size_t)i * n + k], y[k]);
    y[i] = s / L[(size_t)i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {  // Lᵀ z = y
    double s = y[i];
    for (int k = i + 1; k < n; ++k) s = fsdf::gn::minus_product(s, L[(size_t)k * n + i], y[k]);
    y[i] = s / L[(size_t)i * n + i];
  }
  for (int i = 0; i < n; ++i)
    if (!isfinite(y[i])) return FSDF_ERR_DEGENERATE;
  for (int i = 0; i < n; ++i) dx_out[i] = fsdf::gn::clamped_step(y[i], max_step);
  return FSDF_OK;
}

// flash.tracking.LevenbergMarquardt.optimize, operation for operation (the
// same bits): |g| summed in index order; a degenerate step raises lambda
// without an evaluation; a trial is accepted only when ft < f (a NaN ft is
// rejected); lambda / 10 down to 1e-12 on acceptance, x 10 up to 1e12 on
// rejection, the loop ending once it passes 1e12.
// work: g | H | xt | gt | Ht | step | fsdf_lm_step's n^2 + n
extern "C" int fsdf_lm_minimize(fsdf_vgh_fn fn, void* user, int32_t n, double* x, int32_t iteration_limit,
                                double damping, double max_step, double tolerance, double* work, double* value_out,
                                int32_t* iterations_out, double* damping_out) {
  if (iterations_out) *iterations_out = 0;
  if (damping_out) *damping_out = damping;
  if (!fn || n < 0 || iteration_limit < 0 || (n > 0 && !x) || !work) return FSDF_ERR_ARG;
  const size_t nn = (size_t)n * n;
  double* g = work;
  double* H = g + n;
  double* xt = H + nn;
  double* gt = xt + n;
  double* Ht = gt + n;
  double* step = Ht + nn;
  double* step_work = step + n;
  double lam = damping, f = NAN;
  int it = 0;
  if (iteration_limit > 0) {
    const int rc = fn(user, x, &f, g, H);
    if (rc) return rc;
    it = 1;
    if (iterations_out) *iterations_out = it;
  }
  while (it < iteration_limit) {
    double nrm2 = 0.0;
    for (int i = 0; i < n; ++i) nrm2 += g[i] * g[i];
    if (sqrt(nrm2) < tolerance) break;
    const int st = fsdf_lm_step(n, H, g, lam, max_step, step_work, step);
    if (st == FSDF_ERR_DEGENERATE) {  // more damping, no evaluation
      lam *= 10.0;
      if (lam > 1e12) break;
      continue;
    }
    if (st) return st;
    for (int i = 0; i < n; ++i) xt[i] = x[i] + step[i];
    double ft = NAN;
    const int rc = fn(user, xt, &ft, gt, Ht);
    if (rc) {
      if (damping_out) *damping_out = lam;
      if (value_out) *value_out = f;
      return rc;
    }
    ++it;
    if (iterations_out) *iterations_out = it;
    if (ft < f) {
      f = ft;
      for (int i = 0; i < n; ++i) {
        x[i] = xt[i];
        g[i] = gt[i];
      }
      for (size_t i = 0; i < nn; ++i) H[i] = Ht[i];
      lam = 1e-12 > lam / 10.0 ? 1e-12 : lam / 10.0;
    } else {
      lam *= 10.0;
      if (lam > 1e12) break;
    }
  }
  if (damping_out) *damping_out = lam;
  if (value_out) *value_out = f;
  return FSDF_OK;
}
