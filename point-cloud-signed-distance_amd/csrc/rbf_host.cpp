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
// flash/rbf.py solve / chain are the numpy twins the tests compare with.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "flashsdf.h"
#include "rbf_impl.h"  // the arithmetic, shared with the device solver step (solver.hip)

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
