// gn_impl.h — the per-element arithmetic of the Gauss-Newton matrix and of the
// damped (Levenberg-Marquardt) step, shared by the host entry points
// (gauss_newton.cpp fsdf_gauss_newton_matrix / fsdf_lm_step) and the device LM
// loop (lm_solver.hip lm_step_kernel). As kin_impl.h: every function is one
// element's work with a fixed operation order, so the host's sequential loops
// and the device's parallel ones give the same bits (-ffp-contract=off in both
// translation units; device sqrt and division are correctly rounded).
//
// The matrix (gauss_newton.cpp's head comment): per body the moments of its
// surfaces in surface order, subtree sums with the children added in
// descending index, u_j = C_b s_j for every coordinate j of body b, and
// A_ij = s_i · u_j for every coordinate i of b's path to the root.
// The step: D_ii = max(H_ii, 1e-12 max H), Cholesky of H + lambda D with every
// L_ij subtracting L_ik L_jk for k ascending (a multiply, then a subtract),
// L y = g with k ascending per row, Lᵀ z = y with k ascending from i + 1.
#pragma once
#include "kin_impl.h"

namespace fsdf {
namespace gn {

FSDF_HD int joint_width(int kind) { return kind == 1 ? 1 : (kind == 2 ? 7 : 0); }

// slot of (i, j) in a surface's 21 upper-triangle moments (row-major: 00 01 .. 05 11 .. 55)
FSDF_HD int tri_index(int i, int j) {
  const int a = i < j ? i : j, b = i < j ? j : i;
  return 6 * a - (a * (a - 1)) / 2 + (b - a);
}

// The motion rows of body b's joint, rows [width][6]: g_i = rows_i · (F, M) is
// joint_gradient's entry i, the same expressions in the same order (revolute
// ω = Rb·axis, v = tb × ω, row = −(v, ω); quaternion-floating: the four
// rotation columns through E(q̂) with the normalization projection 1/|q| at
// the caller's un-normalised q, then the translation columns −(Rb e_j, 0)).
// (Inputs into locals before the first output is written: kin_impl.h.)
FSDF_HD bool joint_rows(int kind, const double* a_, const double* R_, const double* o_, const double* q_,
                        double* rows) {
  if (kind != 1 && kind != 2) return kind == 0;
  double a[3], R[9], o[3], q[7];
  kin::load(a_, a, 3);
  kin::load(R_, R, 9);
  kin::load(o_, o, 3);
  if (kind == 1) {
    double w[3], v[3];
    for (int i = 0; i < 3; ++i) w[i] = R[3 * i] * a[0] + R[3 * i + 1] * a[1] + R[3 * i + 2] * a[2];
    v[0] = o[1] * w[2] - o[2] * w[1];
    v[1] = o[2] * w[0] - o[0] * w[2];
    v[2] = o[0] * w[1] - o[1] * w[0];
    for (int i = 0; i < 3; ++i) {
      rows[i] = -v[i];
      rows[3 + i] = -w[i];
    }
    return true;
  }
  kin::load(q_, q, 7);
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (!(nrm > 0)) return false;
  const double W = q[0] / nrm, X = q[1] / nrm, Y = q[2] / nrm, Z = q[3] / nrm;
  const double E[3][4] = {{-X, W, -Z, Y}, {-Y, Z, W, -X}, {-Z, -Y, X, W}};
  double org[3];  // world origin of the frame after the joint
  for (int i = 0; i < 3; ++i) org[i] = (R[3 * i] * q[4] + R[3 * i + 1] * q[5] + R[3 * i + 2] * q[6]) + o[i];
  for (int j = 0; j < 4; ++j) {
    double w[3], v[3];
    for (int i = 0; i < 3; ++i)
      w[i] = R[3 * i] * (2.0 * E[0][j]) + R[3 * i + 1] * (2.0 * E[1][j]) + R[3 * i + 2] * (2.0 * E[2][j]);
    v[0] = org[1] * w[2] - org[2] * w[1];
    v[1] = org[2] * w[0] - org[0] * w[2];
    v[2] = org[0] * w[1] - org[1] * w[0];
    for (int i = 0; i < 3; ++i) {
      rows[6 * j + i] = -v[i] / nrm;
      rows[6 * j + 3 + i] = -w[i] / nrm;
    }
  }
  for (int j = 0; j < 3; ++j) {
    double* r = rows + 6 * (4 + j);
    r[0] = -R[j];
    r[1] = -R[3 + j];
    r[2] = -R[6 + j];
    r[3] = r[4] = r[5] = 0.0;
  }
  return true;
}

// entry i of u = C_b s (C_b [6][6] a body's subtree moments, s a motion row): j ascending from 0.0
FSDF_HD double moment_row(const double* Cb, const double* s, int i) {
  double v = 0.0;
  for (int j = 0; j < 6; ++j) v += Cb[6 * i + j] * s[j];
  return v;
}
// A_ij = s_i · u_j: j ascending from 0.0
FSDF_HD double row_dot(const double* si, const double* u) {
  double v = 0.0;
  for (int j = 0; j < 6; ++j) v += si[j] * u[j];
  return v;
}

// ---- the damped step -----------------------------------------------------------
// max_j H_jj over the positive diagonal entries (a NaN is never the larger), one entry at a time
FSDF_HD double diag_max(double hmax, double hjj) { return hjj > hmax ? hjj : hmax; }
// the pivot of column j before its subtractions: H_jj + lambda max(H_jj, floor_d); a NaN H_jj
// stays one (it meets the pivot test)
FSDF_HD double damped_diagonal(double hjj, double lambda, double floor_d) {
  const double dj = hjj > floor_d ? hjj : floor_d;
  return hjj != hjj ? hjj : hjj + lambda * dj;
}
// s − a b: one term of a factorisation or substitution sum (a multiply, then a subtract)
FSDF_HD double minus_product(double s, double a, double b) { return s - a * b; }
FSDF_HD bool bad_pivot(double p) { return !(p > 0.0) || !isfinite(p); }
// clamp(−y, ±max_step)
FSDF_HD double clamped_step(double y, double max_step) {
  const double s = -y;
  const double lo = s < -max_step ? -max_step : s;
  return max_step < lo ? max_step : lo;
}

}  // namespace gn
}  // namespace fsdf
