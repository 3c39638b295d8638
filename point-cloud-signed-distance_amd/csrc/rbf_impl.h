// rbf_impl.h — the arithmetic of the RBF skins' per-pass weight solve and its
// adjoint, shared by the host (rbf_host.cpp fsdf_rbf_solve / fsdf_rbf_adjoint)
// and the device solver step (solver_rbf.h), as kin_impl.h shares the FK. Every
// function is one entry's / one row's / one centre's work with a fixed
// operation order, so the host's sequential loops and the device's
// workgroup-parallel ones produce the same bits (both are built with
// -ffp-contract=off; device sqrt and division are correctly rounded).
//
// The system (src/Flash.jl:143-213 through SpatialFields.InterpolatingSurface
// with XCubed and a linear polynomial): M u = rhs, M = [A P; Pᵀ 0] (m = n + 4),
// A_ij = |c_i - c_j|^3, P_i = (1, c_iᵀ), u = (w, a, b), rhs = (values, 0).
// PA = LU with partial pivoting: the host swaps rows in place (lu_factor); the
// device keeps the rows where they are, swaps a row map, searches the pivot
// across a wave's lanes (the same index: solver_rbf.h rbf_factor) and applies
// lu_multiplier / lu_eliminate / subst_term per entry.
#pragma once
#include <math.h>
#include <stdint.h>

#include "kin_impl.h"  // FSDF_HD

namespace fsdf {
namespace rbf {

// M[i][j] of the m x m system over n centres (m = n + 4)
FSDF_HD double matrix_entry(int n, const double* centres, int i, int j) {
  if (i >= n && j >= n) return 0.0;
  if (i < n && j < n) {
    const double* ci = centres + 3 * i;
    const double* cj = centres + 3 * j;
    const double dx = ci[0] - cj[0], dy = ci[1] - cj[1], dz = ci[2] - cj[2];
    const double r = sqrt(dx * dx + dy * dy + dz * dz);
    return r * r * r;
  }
  // P_c of the centre: (1, c)
  const int c = i < n ? j - n : i - n, k = i < n ? i : j;
  return c == 0 ? 1.0 : centres[3 * k + c - 1];
}

// the right-hand side: the centres' values, then four zeros
FSDF_HD double rhs_entry(int n, const double* values, int i) { return i < n ? values[i] : 0.0; }

// Step k's pivot: the first row i >= k of the largest |A[i][k]| under a strict
// >, from |A[k][k]| (a NaN there stays; a NaN below is never taken). Returns
// -1 for a singular or non-finite column.
FSDF_HD int lu_pivot(int m, const double* A, int k) {
  int p = k;
  double best = fabs(A[k * m + k]);
  for (int i = k + 1; i < m; ++i) {
    const double v = fabs(A[i * m + k]);
    if (v > best) {
      best = v;
      p = i;
    }
  }
  if (!(best > 0.0) || !isfinite(best)) return -1;
  return p;
}

// Step k on row i > k: the multiplier l = a_ik / a_kk as a_ik * (1 / a_kk),
// then a_ij -= l a_kj (skipped for l == 0, which keeps a non-finite a_kj out)
FSDF_HD double lu_multiplier(double a_ik, double inv_kk) { return a_ik * inv_kk; }
FSDF_HD double lu_eliminate(double a_ij, double l, double a_kj) { return l != 0.0 ? a_ij - l * a_kj : a_ij; }

// In-place LU with partial pivoting of the row-major m x m matrix A
// (PA = LU, unit lower L below the diagonal, U on and above it), rows swapped
// in place; piv[k] = the row swapped with k. Returns false if singular.
FSDF_HD bool lu_factor(int m, double* A, int32_t* piv) {
  for (int k = 0; k < m; ++k) {
    const int p = lu_pivot(m, A, k);
    if (p < 0) return false;
    piv[k] = p;
    if (p != k)
      for (int j = 0; j < m; ++j) {
        const double t = A[k * m + j];
        A[k * m + j] = A[p * m + j];
        A[p * m + j] = t;
      }
    const double inv = 1.0 / A[k * m + k];
    for (int i = k + 1; i < m; ++i) {
      const double l = lu_multiplier(A[i * m + k], inv);
      A[i * m + k] = l;
      for (int j = k + 1; j < m; ++j) A[i * m + j] = lu_eliminate(A[i * m + j], l, A[k * m + j]);
    }
  }
  return true;
}

// One term of a substitution row: s - l_ij b_j (forward: j < i ascending from
// s = b_i; backward: j > i ascending from s = b_i, then s / u_ii)
FSDF_HD double subst_term(double s, double a_ij, double b_j) { return s - a_ij * b_j; }

// Solves A x = b in place with the factorization of lu_factor.
FSDF_HD void lu_solve(int m, const double* LU, const int32_t* piv, double* b) {
  for (int k = 0; k < m; ++k)
    if (piv[k] != k) {
      const double t = b[k];
      b[k] = b[piv[k]];
      b[piv[k]] = t;
    }
  for (int i = 1; i < m; ++i) {
    double s = b[i];
    for (int j = 0; j < i; ++j) s = subst_term(s, LU[i * m + j], b[j]);
    b[i] = s;
  }
  for (int i = m - 1; i >= 0; --i) {
    double s = b[i];
    for (int j = i + 1; j < m; ++j) s = subst_term(s, LU[i * m + j], b[j]);
    b[i] = s / LU[i * m + i];
  }
}

// The adjoint's pair factor 3 |c_j - c_i| (∇φ(d) = 3 |d| d)
FSDF_HD double adjoint_r3(const double* centres, int j, int i) {
  const double* cj = centres + 3 * j;
  const double* ci = centres + 3 * i;
  const double d[3] = {cj[0] - ci[0], cj[1] - ci[1], cj[2] - ci[2]};
  return 3.0 * sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
}

// Component c of G_j = ∂cost/∂c_j through the solve: E_j - (w_j Σ_i μw_i g_ji +
// μw_j Σ_i w_i g_ji + μw_j b + w_j μb), g_ji = 3 |c_j - c_i| (c_j - c_i), both
// sums over i ascending. u = (w, a, b), mu = M⁻¹λ likewise; r3_j: optional
// row j of the pair factors (adjoint_r3), computed here when null.
FSDF_HD double adjoint_entry(int n, const double* centres, const double* u, const double* mu, const double* E, int j,
                             int c, const double* r3_j) {
  const double *w = u, *b = u + n + 1, *mw = mu, *mb = mu + n + 1;
  const double cjc = centres[3 * j + c];
  double sm = 0.0, sw = 0.0;
  for (int i = 0; i < n; ++i) {
    const double r3 = r3_j ? r3_j[i] : adjoint_r3(centres, j, i);
    const double g = r3 * (cjc - centres[3 * i + c]);
    sm += mw[i] * g;
    sw += w[i] * g;
  }
  const double term = w[j] * sm + mw[j] * sw + mw[j] * b[c] + w[j] * mb[c];
  return E[3 * j + c] - term;
}

}  // namespace rbf
}  // namespace fsdf
