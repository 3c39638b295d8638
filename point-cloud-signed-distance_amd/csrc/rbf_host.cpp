// Host side of the RBF interpolating skins around the GPU pass
// (src/Flash.jl:143-213: SpatialFields.InterpolatingSurface(points, values,
// XCubed(), true) over the posed surface points, value 0, and skeleton
// points, value -1):
//   fsdf_rbf_solve    the per-pass weight solve [A P; Pᵀ 0][w; a; b] = [v; 0],
//                     A_ij = |c_i - c_j|^3, P_i = (1, c_iᵀ), by LU with partial
//                     pivoting (kept for the adjoint);
//   fsdf_rbf_adjoint  the pass's RBF accumulator block (λ = Σ 2s ∂s/∂(w,a,b),
//                     E_j = Σ 2s ∂s/∂c_j) -> G_j = ∂c/∂c_j through the solve:
//                     μ = M⁻ᵀλ (M is symmetric), ∂(w,a,b)/∂c_j by implicit
//                     differentiation of M u = rhs.
//   fsdf_rbf_state_map  the linear map L from a skin's accumulator block to the
//                     state gradient (the Gauss-Newton term L M Lᵀ of the skin).
// flash/rbf.py solve / chain / state_map are the numpy twins the tests compare with.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "flashsdf.h"
#include "rbf_impl.h"  // the arithmetic, shared with the device solver step (solver_rbf.h)

using namespace fsdf::rbf;

extern "C" int fsdf_rbf_solve(int32_t n, const double* centres, const double* values, double* u, double* lu,
                              int32_t* piv) {
  if (n < 1 || !centres || !values || !u || !lu || !piv) return FSDF_ERR_ARG;
  const int m = n + 4;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) lu[i * m + j] = matrix_entry(n, centres, i, j);
  if (!lu_factor(m, lu, piv)) return FSDF_ERR_DEGENERATE;
  for (int i = 0; i < m; ++i) u[i] = rhs_entry(n, values, i);
  lu_solve(m, lu, piv, u);
  for (int i = 0; i < m; ++i)
    if (!std::isfinite(u[i])) return FSDF_ERR_DEGENERATE;
  return FSDF_OK;
}

extern "C" int fsdf_rbf_adjoint(int32_t n, const double* centres, const double* u, const double* lu,
                                const int32_t* piv, const double* block, double* G, double* work) {
  if (n < 1 || !centres || !u || !lu || !piv || !block || !G || !work) return FSDF_ERR_ARG;
  const int m = n + 4;
  double* mu = work;  // μ = M⁻ᵀ λ = M⁻¹ λ (M symmetric)
  std::memcpy(mu, block, (size_t)m * sizeof(double));
  lu_solve(m, lu, piv, mu);
  const double* E = block + m;
  for (int j = 0; j < n; ++j)
    for (int c = 0; c < 3; ++c) G[3 * j + c] = adjoint_entry(n, centres, u, mu, E, j, c, nullptr);
  return FSDF_OK;
}

// One skin's map from its accumulator block to the state gradient, column by
// column: the unit block e_k through fsdf_rbf_adjoint, the body wrenches and
// ∂/∂δ as fsdf_value_and_gradient forms them (iterate.hip iteration_finish),
// and fsdf_config_gradient — the gradient's own code, so L is its map by
// construction. flash/rbf.py state_map is the numpy twin.
extern "C" int fsdf_rbf_state_map(int32_t nb, const int32_t* parent, const int32_t* kind, const int32_t* qoff,
                                  const double* axis, const double* R, const double* Rb, const double* tb,
                                  const double* q, int32_t nq, int32_t n, const double* centres, const double* u,
                                  const double* lu, const int32_t* piv, const int32_t* body, const int32_t* drow,
                                  int32_t n_deform, double* work, double* L_out) {
  if (nb < 1 || nq < 0 || n < 1 || n_deform < 0 || !parent || !kind || !qoff || !axis || !R || !Rb || !tb || !q ||
      !centres || !u || !lu || !piv || !body || !work || !L_out)
    return FSDF_ERR_ARG;
  for (int j = 0; j < n; ++j)
    if (body[j] < -1 || body[j] >= nb || (drow && (drow[j] < -1 || drow[j] >= n_deform))) return FSDF_ERR_ARG;
  for (int b = 1; b < nb; ++b) {  // (the chain rule writes g at the joints' coordinates)
    const int width = kind[b] == 1 ? 1 : (kind[b] == 2 ? 7 : 0);
    if (kind[b] < 0 || kind[b] > 2 || (width && (qoff[b] < 0 || qoff[b] + width > nq))) return FSDF_ERR_ARG;
  }
  const int m = 4 * n + 4, nx = nq + 3 * n_deform;
  double* block = work;               // [4n+4]
  double* G = block + m;              // [n][3]
  double* adj = G + 3 * n;            // [n+4]
  double* wrench = adj + n + 4;       // [nb][6]
  double* cg = wrench + 6 * nb;       // [nb][6] fsdf_config_gradient's scratch
  double* g = cg + 6 * nb;            // [nx]
  for (int k = 0; k < m; ++k) block[k] = 0.0;
  for (int k = 0; k < m; ++k) {
    block[k] = 1.0;
    int rc = fsdf_rbf_adjoint(n, centres, u, lu, piv, block, G, adj);
    block[k] = 0.0;
    if (rc) return rc;
    for (int i = 0; i < 6 * nb; ++i) wrench[i] = 0.0;
    for (int i = 0; i < nx; ++i) g[i] = 0.0;
    for (int j = 0; j < n; ++j) {
      const double* Gj = G + 3 * j;
      const double* cj = centres + 3 * j;
      const int b = body[j];
      if (b >= 0) {
        double* w = wrench + 6 * b;
        w[0] -= Gj[0];
        w[1] -= Gj[1];
        w[2] -= Gj[2];
        w[3] -= cj[1] * Gj[2] - cj[2] * Gj[1];
        w[4] -= cj[2] * Gj[0] - cj[0] * Gj[2];
        w[5] -= cj[0] * Gj[1] - cj[1] * Gj[0];
      }
      if (drow && drow[j] >= 0) {  // c_j = R_b (p_j + δ_j) + t_b
        double* gd = g + nq + 3 * drow[j];
        for (int i = 0; i < 3; ++i)
          gd[i] += b < 0 ? Gj[i] : (R[9 * b + i] * Gj[0] + R[9 * b + 3 + i] * Gj[1] + R[9 * b + 6 + i] * Gj[2]);
      }
    }
    rc = fsdf_config_gradient(nb, parent, kind, qoff, axis, Rb, tb, q, 0, nullptr, nullptr, wrench, cg, g);
    if (rc) return rc;
    for (int i = 0; i < nx; ++i) L_out[(size_t)i * m + k] = g[i];
  }
  return FSDF_OK;
}
