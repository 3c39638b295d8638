"""Robust point losses for the cost and the Levenberg-Marquardt solver.

A loss is (kind, scale c > 0), given by its weight w(d) = ρ′(d) / (2d) with
ρ(d) = d² near zero (include/flashsdf.h "robust point losses"):

  Huber(c)   |d| <= c: w = 1, ρ = d²;  else w = c/|d|, ρ = 2c|d| − c²
  Tukey(c)   u = d/c;  |d| < c: w = (1 − u²)², ρ = (c²/3)(1 − (1 − u²)³),
             evaluated as (c²/3) u² (3 − u² (3 − u²)): no cancellation near 0;
             else w = 0 exactly, ρ = c²/3

`weight` and `rho` are numpy twins of csrc/robust_impl.h, in its operation
order; they keep the dtype of `d` (float64 by default; a test may call them in
numpy.longdouble). The library evaluates them on the device
(csrc/robust.hip); pass a loss to CostFunctor / estimate_state / Tracker /
track (`loss=`), or to Context.set_loss. None means least squares.
"""
from __future__ import annotations

import numpy as np

SQUARE, HUBER, TUKEY = 0, 1, 2


def _residuals(d):
    d = np.asarray(d)
    return d if np.issubdtype(d.dtype, np.floating) else d.astype(np.float64)


class _Loss:
    kind = SQUARE
    name = "square"

    def __init__(self, scale: float):
        scale = float(scale)
        if not (np.isfinite(scale) and scale > 0.0):
            raise ValueError(f"{type(self).__name__}: the scale must be finite and > 0, got {scale!r}")
        self.scale = scale

    def __repr__(self):
        return f"{type(self).__name__}({self.scale!r})"

    def __eq__(self, other):
        return type(other) is type(self) and other.scale == self.scale

    def __hash__(self):
        return hash((type(self).__name__, self.scale))


class Huber(_Loss):
    """Quadratic up to |d| = scale, linear beyond: a far point pulls with a
    constant force."""
    kind = HUBER
    name = "huber"

    def weight(self, d):
        d = _residuals(d)
        c, a = d.dtype.type(self.scale), np.abs(d)
        far = a > c
        return np.where(far, c / np.where(far, a, 1), d.dtype.type(1))

    def rho(self, d):
        d = _residuals(d)
        c, a = d.dtype.type(self.scale), np.abs(d)
        return np.where(a <= c, d * d, (2 * c) * a - c * c)


class Tukey(_Loss):
    """Tukey's biweight: a point beyond |d| = scale has no influence at all."""
    kind = TUKEY
    name = "tukey"

    def weight(self, d):
        d = _residuals(d)
        c = d.dtype.type(self.scale)
        with np.errstate(over="ignore"):  # (a huge |d| is beyond c: its t is not used)
            u = d / c
            t = 1 - u * u
        return np.where(np.abs(d) < c, t * t, d.dtype.type(0))

    def rho(self, d):
        d = _residuals(d)
        c = d.dtype.type(self.scale)
        third = (c * c) / 3
        with np.errstate(over="ignore"):  # (a huge |d| is beyond c: its q is not used)
            u = d / c
            q = u * u
            # 1 − (1 − q)³ = q (3 − q (3 − q)): no cancellation near d = 0
            inside = third * (q * (3 - q * (3 - q)))
        return np.where(np.abs(d) < c, inside, third)


def parse(spec):
    """'huber:0.02' / 'tukey:0.05' -> the loss; None, '' or 'square' -> None."""
    if spec is None or isinstance(spec, _Loss):
        return spec
    name, _, scale = str(spec).partition(":")
    name = name.strip().lower()
    if name in ("", "none", "square"):
        return None
    kinds = {"huber": Huber, "tukey": Tukey}
    if name not in kinds or not scale:
        raise ValueError(f"loss {spec!r}: expected huber:SCALE or tukey:SCALE")
    return kinds[name](float(scale))


def _point_factors(dd, loss, weights, one_sided, who):
    """(aw, a·ρ) per point in the dtype of dd, formed as csrc/robust.hip forms
    them: w = w(d) and ρ of `loss` (None: 1, d²), a = weights (None: 1) through
    the one-sided gate (one_sided: True for a free-space sample, which keeps
    its a only where d < 0 and gets exactly 0 elsewhere), one product aw."""
    t = dd.dtype.type
    w = np.ones_like(dd) if loss is None else loss.weight(dd)
    rho = dd * dd if loss is None else loss.rho(dd)
    a = None
    if weights is not None:
        a = np.asarray(weights, dd.dtype)
        if a.shape != dd.shape:
            raise ValueError(f"{who}: {a.shape} weights for {dd.shape} points")
    if one_sided is not None:
        free = np.asarray(one_sided)
        if free.dtype != np.bool_ or free.shape != dd.shape:
            raise ValueError(f"{who}: one_sided is a boolean mask per point, got {free.dtype} {free.shape}")
        a = np.where(~free | (dd < 0), np.ones_like(dd) if a is None else a, t(0))
    if a is not None:
        w, rho = a * w, a * rho
    return w, rho


def weighted_sums(points, kstar, d, grad, n_surfaces, loss=None, weights=None, one_sided=None):
    """The per-surface sums of the (weighted) robust objective in plain numpy,
    from per-point outputs (include/flashsdf.h "per-point confidence
    weights"): with a = weights (None: 1), w = w(d) and ρ of `loss` (None:
    w = 1, ρ = d²), v = (∇d, p × ∇d) and aw = a · w, over the points with
    k* = k:
        cost [S] Σ a ρ;  wrench [S, 6] Σ 2 (aw d) v;  moments [S, 21] Σ aw v vᵀ
        (upper triangle, row-major);  W [S] Σ aw.
    The per-point factors are formed as csrc/robust.hip forms them (one product
    aw, wrench scale 2 (aw d), a · ρ); the sums are numpy's, in the dtype of `d`
    (float64 by default; a test may pass numpy.longdouble).
    one_sided: a boolean mask per point, True for a free-space sample
    (include/flashsdf.h "free space"): such a point counts only where d < 0.
    The gate is formed as the kernel forms it (csrc/robust_impl.h
    one_sided_factor): its factor a becomes exactly 0 where the gate is shut,
    and the weighted arithmetic follows."""
    dd = _residuals(d)
    t = dd.dtype.type
    P, G = np.asarray(points, dd.dtype), np.asarray(grad, dd.dtype)
    k = np.asarray(kstar)
    w, rho = _point_factors(dd, loss, weights, one_sided, "weighted_sums")
    v = np.concatenate([G, np.cross(P, G)], axis=1)
    term = v * (t(2) * (w * dd))[:, None]
    iu = np.triu_indices(6)
    S = int(n_surfaces)
    cost, wrench = np.zeros(S, dd.dtype), np.zeros((S, 6), dd.dtype)
    moments, W = np.zeros((S, 21), dd.dtype), np.zeros(S, dd.dtype)
    for s in np.unique(k):
        if s < 0 or s >= S:
            continue
        sel = k == s
        cost[s], wrench[s], W[s] = rho[sel].sum(), term[sel].sum(0), w[sel].sum()
        moments[s] = np.einsum("ni,nj->ij", v[sel] * w[sel, None], v[sel])[iu]
    return cost, wrench, moments, W


def _skins(solves_or_rows):
    """[(surface, centres [n, 3], u [n + 4])]: of flash.rbf.solve's RbfSolves
    (their .surface, .centres, .u), or of (surface, rows [n + 1, 4]) pairs —
    a skin's rows as set_rbf_params takes them (centre and weight per centre,
    then (a, b))."""
    out = []
    for r in solves_or_rows:
        if hasattr(r, "centres"):
            out.append((int(r.surface), np.asarray(r.centres), np.asarray(r.u)))
        else:
            surface, rows = r
            rows = np.asarray(rows)
            out.append((int(surface), rows[:-1, :3], np.concatenate([rows[:-1, 3], rows[-1]])))
    return out


def weighted_skin_blocks(points, kstar, d, solves_or_rows, loss=None, weights=None, one_sided=None,
                         dtype=np.float64):
    """The RBF skins' blocks of the accumulator under the (weighted) robust
    objective in plain numpy (include/flashsdf.h "robust objectives on skins"):
    per skin Σ 2 (aw d) j over the points with k* = the skin's surface, j the
    point's row of flash.rbf.skin_jacobian (the block's layout) and aw as
    weighted_sums forms it. With no loss, weights or mask: Σ 2 d j, the pass's
    own block. Returns one [4n + 4] array per skin, in the order given.
    dtype: the arithmetic's (np.longdouble measures float64's own rounding)."""
    from . import rbf
    dd = np.asarray(d, dtype)
    P, k = np.asarray(points, dtype).reshape(-1, 3), np.asarray(kstar)
    aw, _ = _point_factors(dd, loss, weights, one_sided, "weighted_skin_blocks")
    t = dd.dtype.type(2) * (aw * dd)
    out = []
    for surface, C, u in _skins(solves_or_rows):
        sel = k == surface
        J = rbf.skin_jacobian(C, u, P[sel], dtype=dtype)
        out.append((J * t[sel, None]).sum(0))
    return out


def weighted_skin_moments(points, kstar, d, solves_or_rows, loss=None, weights=None, one_sided=None,
                          dtype=np.float64):
    """The skins' weighted second moments Σ aw j jᵀ — the Gauss-Newton (IRLS)
    term of the robust objective on a skin, as weighted_skin_blocks: one
    [4n + 4, 4n + 4] array per skin. With no loss, weights or mask: Σ j jᵀ
    (csrc/skin_moments.hip)."""
    from . import rbf
    dd = np.asarray(d, dtype)
    P, k = np.asarray(points, dtype).reshape(-1, 3), np.asarray(kstar)
    aw, _ = _point_factors(dd, loss, weights, one_sided, "weighted_skin_moments")
    out = []
    for surface, C, u in _skins(solves_or_rows):
        sel = k == surface
        J = rbf.skin_jacobian(C, u, P[sel], dtype=dtype)
        out.append((J * aw[sel, None]).T @ J)
    return out
