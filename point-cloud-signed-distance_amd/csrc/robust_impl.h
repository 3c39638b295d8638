// robust_impl.h — the robust point losses (include/flashsdf.h "robust point
// losses"): the one definition of the weight w(d) = ρ′(d) / (2d) and of ρ(d),
// shared by the device reduction (robust.hip robust_kernel) and the host entry
// points (pass.hip fsdf_set_loss). As gn_impl.h and kin_impl.h: every function
// is one point's work with a fixed operation order (-ffp-contract=off in every
// translation unit; device division is correctly rounded), so a host
// restatement gives the same bits. flash/robust.py restates the same order in
// numpy. All arithmetic fp64.
//
//   SQUARE (0)  w = 1, ρ = d²
//   HUBER  (1)  |d| <= c: w = 1, ρ = d²; else w = c / |d|, ρ = 2c|d| − c²
//               (|d| <= c is tested first: d = 0 never divides)
//   TUKEY  (2)  u = d / c; |d| < c: w = (1 − u²)², ρ = (c²/3)(1 − (1 − u²)³),
//               evaluated as (c²/3) u² (3 − u² (3 − u²)): a point near the
//               surface keeps ρ's relative accuracy (the expanded form loses
//               it to 1 − (1 − u²)³'s cancellation); else w = 0 exactly, ρ = c²/3
#pragma once
#include <math.h>
#include <stdint.h>

#include "kin_impl.h"

namespace fsdf {
namespace robust {

constexpr int kSquare = 0, kHuber = 1, kTukey = 2;

// a loss the library serves: a known kind, and for Huber / Tukey a finite scale > 0
FSDF_HD bool valid(int kind, double c) {
  if (kind == kSquare) return true;
  if (kind != kHuber && kind != kTukey) return false;
  return c > 0.0 && c <= 1.79769313486231570815e308;  // (finite; a NaN fails the first test)
}

FSDF_HD double weight(int kind, double c, double d) {
  const double a = fabs(d);
  if (kind == kHuber) return a <= c ? 1.0 : c / a;
  if (kind == kTukey) {
    if (!(a < c)) return 0.0;
    const double u = d / c, t = 1.0 - u * u;
    return t * t;
  }
  return 1.0;
}

FSDF_HD double rho(int kind, double c, double d) {
  const double a = fabs(d);
  if (kind == kHuber) return a <= c ? d * d : (2.0 * c) * a - c * c;
  if (kind == kTukey) {
    const double third = (c * c) / 3.0;
    if (!(a < c)) return third;
    const double u = d / c, q = u * u;
    return third * (q * (3.0 - q * (3.0 - q)));  // = third (1 − (1 − q)³), without its cancellation near d = 0
  }
  return d * d;
}

// the factor of v = (∇d*, p × ∇d*) in a point's wrench 2 w d · v
FSDF_HD double wrench_scale(double w, double d) { return 2.0 * (w * d); }

// Free-space samples (include/flashsdf.h "free space"): caller points
// [n_surface, n) are positions known to be empty, penalised only where the
// model covers them. one_sided_factor is the point's factor a in the weighted
// arithmetic above (a · w, a · ρ): the caller's weight (1.0 without weights)
// for a surface observation and for a sample with d* < 0, exactly 0.0 for a
// sample the model does not cover (a NaN d* fails the test) — that point stays
// in the sums as zero terms, as a weight-0 point does.
FSDF_HD bool free_sample(int64_t caller_index, int64_t n_surface) { return caller_index >= n_surface; }
FSDF_HD bool one_sided_gate(double d) { return d < 0.0; }
FSDF_HD double one_sided_factor(bool free, double d, double a) { return !free || one_sided_gate(d) ? a : 0.0; }

}  // namespace robust
}  // namespace fsdf
