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
