"""Per-point confidence weights on the CPU (include/flashsdf.h "per-point
confidence weights"): depth_noise_weights, the weighted robust objective
Σ a ρ(d*) with its wrench and moments over the CPU oracle
(flash.robust.weighted_sums), what a zero weight does to the seed-41 drift
case of tests/test_lm_prior.py, and the way tracking._optimize hands weights to
the functor."""
import types

import numpy as np
import pytest

from gn_helpers import OracleCost

# err123 of the seed-41 case after 10 LM evaluations with weight 0 on the cloud's synthetic
# outliers and interior points (test_zero_weights_are_the_cloud_without_those_points; the GPU
# twin tests/test_gpu_point_weights.py reproduces it to four digits). Least squares: 0.1114,
# Huber(0.02): 0.0135 (tests/test_robust_loss.py).
ORACLE_WEIGHTS_ERR123 = 0.0117
LEAST_SQUARES_ERR123 = 0.1114


# ---- 1. depth_noise_weights ----------------------------------------------------------------

def test_depth_noise_weights():
    import flash
    from flash import depthsensors
    assert flash.depth_noise_weights is depthsensors.depth_noise_weights
    r = np.random.default_rng(3)
    origin, axis = np.array([0.2, -1.0, 0.5]), np.array([0.0, 3.0, 4.0])  # (|axis| = 5: any length)
    unit = axis / 5.0
    # a point at range z0 along the axis, anywhere across it: exactly 1
    across = np.cross(unit, [1.0, 0.0, 0.0])
    at_z0 = origin + 0.4 * unit + np.outer([0.0, 0.3, -2.0], across)
    z_at = (at_z0 - origin) @ unit
    w = flash.depth_noise_weights(at_z0, origin, axis)
    assert (np.abs(w - 1.0) <= 4 * 0.0019 / 0.0012 * (z_at - 0.4) ** 2 + 1e-15).all() and w[0] == 1.0
    # monotone decreasing beyond z0
    z = np.linspace(0.4, 6.0, 400)
    w = flash.depth_noise_weights(origin + np.outer(z, unit), origin, axis)
    assert w[0] == pytest.approx(1.0, abs=1e-15) and (np.diff(w) < 0).all() and (w > 0).all()
    # values against the formula in longdouble, defaults and other parameters
    pts = r.uniform(-3, 3, (500, 3))
    for kw in ({}, {"sigma0": 0.002, "k": 0.004, "z0": 0.7}, {"k": 0.0}):
        s0, k, z0 = (np.longdouble(kw.get(n, dflt)) for n, dflt in (("sigma0", 0.0012), ("k", 0.0019), ("z0", 0.4)))
        zl = (pts.astype(np.longdouble) - origin.astype(np.longdouble)) @ (axis.astype(np.longdouble) / 5)
        want = (s0 / (s0 + k * (zl - z0) ** 2)) ** 2
        got = flash.depth_noise_weights(pts, origin, axis, **kw)
        assert got.dtype == np.float64 and got.shape == (500,)
        # (|d ln w / dz| = 4 k dz / (σ0 + k dz²) <= 2 sqrt(k / σ0) < 3 here; z carries at most
        # ~6 u |p − o| <= 2^-47 absolute with |p − o| < 8 (the difference, the dot product), so
        # 3 · 2^-47 of the weight, relative, plus the formula's own seven roundings: < 2^-44)
        assert (np.abs(got - want) <= 2.0 ** -44 * want).all(), float((np.abs(got - want) / want).max())
    assert np.array_equal(flash.depth_noise_weights(pts, origin, axis, k=0.0), np.ones(500))
    # bad shapes and parameters raise
    for bad in (np.zeros(3), np.zeros((4, 2)), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError):
            flash.depth_noise_weights(bad, origin, axis)
    for o, a in ((np.zeros(2), axis), (origin, np.zeros((1, 3))), (origin, np.zeros(3))):
        with pytest.raises(ValueError):
            flash.depth_noise_weights(pts, o, a)
    with pytest.raises(ValueError):
        flash.depth_noise_weights(pts, origin, axis, sigma0=0.0)
    assert flash.depth_noise_weights(np.zeros((0, 3)), origin, axis).shape == (0,)


# ---- 2. the weighted objective over the CPU oracle -------------------------------------------

class WeightedOracleCost(OracleCost):
    """OracleCost with a loss and per-point weights, through
    flash.robust.weighted_sums: c = Σ a ρ(d*), the wrench Σ 2 a w d* v and the
    moments Σ a w v vᵀ."""

    def __init__(self, m, pts, loss=None, weights=None):
        super().__init__(m, pts)
        self.loss, self.weights = loss, weights

    def _sums(self, x):
        from flash.robust import weighted_sums
        d, k, g = self.per_point(x)
        return weighted_sums(self.pts, k, d, g, len(self.sb), self.loss, self.weights)

    def value_and_gradient(self, x):
        x = np.asarray(x, np.float64)
        cost, wrench, _, _ = self._sums(x)
        mech = self.m.mechanism
        bw = np.zeros((mech.num_bodies, 6))
        np.add.at(bw, self.sb, wrench)
        return float(cost.sum()), mech.config_gradient_numpy(x, bw)

    def __call__(self, x):
        x = np.asarray(x, np.float64)
        cost, wrench, mom, _ = self._sums(x)
        mech = self.m.mechanism
        bw = np.zeros((mech.num_bodies, 6))
        np.add.at(bw, self.sb, wrench)
        return float(cost.sum()), mech.config_gradient_numpy(x, bw), 2.0 * mech.gauss_newton_matrix_numpy(x, self.sb, mom)


def seed41_case():
    """tests/test_lm_prior.py's seed-41 drift case (IRB140, 3,000 points of
    synthetic.depth_cloud at its defaults) and, per point of the cloud, whether
    it is one of the cloud's synthetic outliers (10 % uniform in the padded
    box) or interior points (5 %): depth_cloud(order="generated") draws the
    same points and lists surface samples, box samples and interior points in
    that order; the default raster order only permutes them."""
    from flash import Models, synthetic
    m = Models.irb140()
    q_true, q0 = synthetic.perturbed_configuration(m, 41)
    pts = synthetic.depth_cloud(m, q_true, 3000, seed=42)
    gen = synthetic.depth_cloud(m, q_true, 3000, seed=42, order="generated")
    n_surf = int(round(0.85 * 3000))
    label = {row.tobytes(): i >= n_surf for i, row in enumerate(gen)}
    assert len(label) == 3000
    off_surface = np.array([label[row.tobytes()] for row in pts])
    assert off_surface.sum() == 3000 - n_surf == 450
    return m, pts, np.asarray(q_true, np.float64), np.asarray(q0, np.float64), off_surface


@pytest.fixture(scope="module")
def case(oracle_mod):
    return seed41_case()


def seed41_weights(n=3000):
    """Uniform in [0, 2], about one in ten exactly 0 (the GPU tests' recipe)."""
    r = np.random.default_rng(4141)
    a = r.uniform(0.0, 2.0, n)
    a[r.random(n) < 0.1] = 0.0
    return a


def test_weighted_sums_without_weights_or_loss_are_the_oracle_cost(case):
    m, pts, _, q0, _ = case
    plain, w = OracleCost(m, pts), WeightedOracleCost(m, pts, None, np.ones(len(pts)))
    a, b = plain(q0), w(q0)
    assert abs(a[0] - b[0]) <= 1e-13 * a[0] and np.allclose(a[1], b[1], rtol=0, atol=1e-12 * np.abs(a[1]).max())
    assert np.allclose(a[2], b[2], rtol=0, atol=1e-12 * np.abs(a[2]).max())
    quarter = WeightedOracleCost(m, pts, None, np.full(len(pts), 0.25))(q0)
    assert quarter[0] == 0.25 * b[0] and np.array_equal(quarter[1], 0.25 * b[1]) and np.array_equal(quarter[2], 0.25 * b[2])


@pytest.mark.parametrize("spec", ["huber:0.02", "tukey:0.05", "square"])
def test_weighted_gradient_matches_central_differences(case, spec):
    """∂(Σ a ρ)/∂x by the chain rule on the weighted wrench against central
    differences of Σ a ρ itself: the step (h = 1e-6) and tolerance
    (|g − g_fd|_∞ <= 1e-7 |g|_∞) of tests/test_robust_loss.py's unweighted
    case — the weights are constants of the objective."""
    from flash import robust
    m, pts, _, q0, _ = case
    oc = WeightedOracleCost(m, pts, robust.parse(spec), seed41_weights())
    c, g = oc.value_and_gradient(q0)
    h, eye = 1e-6, np.eye(len(q0))
    g_fd = np.array([(oc.value_and_gradient(q0 + h * e)[0] - oc.value_and_gradient(q0 - h * e)[0]) / (2 * h)
                     for e in eye])
    err, scale = float(np.abs(g - g_fd).max()), float(np.abs(g).max())
    print(f"seed 41 {spec} weighted: c {c:.6f} |g|_inf {scale:.4f} |g - g_fd|_inf {err:.2e}")
    assert scale > 0 and err <= 1e-7 * scale, (err, scale)


# ---- 3. weight 0 removes a point; oracle weights against least squares -------------------------

def _lm(oc, q0, n):
    from flash.tracking import LevenbergMarquardt, state_prior

    def vgh(x):
        c, g, H = oc(x)
        return c / n, g / n, H / n

    s = LevenbergMarquardt(len(q0), damping=1e-3, max_step=0.5, iteration_limit=10, gradient_convergence_tolerance=0.0)
    x, _ = s.optimize(state_prior(vgh, q0, 1e-3), q0)
    assert s.iterations == 10
    return x


def test_zero_weights_are_the_cloud_without_those_points(case):
    """tests/test_robust_loss.py's conditions (10 LM evaluations, damping 1e-3,
    max_step 0.5, tolerance 0, prior μ = 1e-3, c / N with N = 3,000 in both
    runs) with weight 0 on the cloud's synthetic outliers and interior points,
    1 elsewhere: the state LM reaches on the cloud with those points deleted,
    to 1e-9 in every joint — only the summation order differs. Its err123 is
    ORACLE_WEIGHTS_ERR123, below the unweighted least-squares run's 0.1114
    (DESIGN.md §7)."""
    m, pts, q_true, q0, off = case
    a = np.where(off, 0.0, 1.0)
    x_w = _lm(WeightedOracleCost(m, pts, None, a), q0, 3000.0)
    x_d = _lm(WeightedOracleCost(m, pts[~off], None, None), q0, 3000.0)
    err = float(np.abs(x_w - q_true)[:3].max())
    print(f"seed 41: zero weights vs deletion |dx|_inf {np.abs(x_w - x_d).max():.2e}; err123 {err:.4f} "
          f"(least squares {LEAST_SQUARES_ERR123}, start {np.abs(q0 - q_true)[:3].max():.4f})")
    assert np.abs(x_w - x_d).max() <= 1e-9
    assert abs(err - ORACLE_WEIGHTS_ERR123) <= 5e-5, err
    assert err < LEAST_SQUARES_ERR123


# ---- 4. tracking._optimize hands the weights to the functor -----------------------------------

def test_optimize_hands_the_weights_to_the_functor():
    """_optimize(..., weights=) sets the functor's weights (after its loss)
    before the native loop is entered; without weights= the functor is left as
    it is."""
    from flash.robust import Huber
    from flash.tracking import LevenbergMarquardt, NaiveSolver, _optimize
    calls = []

    def descend_lm(x, limit, damping, max_step, tol, n, prior_weight=None, device_loop=None):
        calls.append(("descend_lm", prior_weight, device_loop))
        return x + 1.0, 0.5, 3, 1e-5

    def descend(x, limit, rate, max_step, tol, div, n):
        calls.append(("descend", limit, n))
        return x - 1.0, 0.25, 2

    cost = types.SimpleNamespace(_native=True, rigid=True, value_gradient_hessian=None, descend_lm=descend_lm,
                                 descend=descend, set_loss=lambda loss: calls.append(("set_loss", loss)),
                                 set_point_weights=lambda w: calls.append(("set_point_weights", w)))
    w = np.linspace(0.0, 1.0, 12)
    solver = LevenbergMarquardt(3, iteration_limit=7, prior_weight=1e-3, device_loop=True)
    x = _optimize(cost, 12, np.zeros(3), None, solver, weights=w)
    assert np.array_equal(x, np.ones(3)) and solver.iterations == 3
    assert [c[0] for c in calls] == ["set_point_weights", "descend_lm"] and calls[0][1] is w
    del calls[:]
    x = _optimize(cost, 12, np.zeros(3), None, NaiveSolver(3, iteration_limit=5), loss=Huber(0.02), weights=w)
    assert np.array_equal(x, -np.ones(3))
    assert [c[0] for c in calls] == ["set_loss", "set_point_weights", "descend"] and calls[2] == ("descend", 5, 12)
    del calls[:]
    _optimize(cost, 12, np.zeros(3), None, solver)
    assert calls == [("descend_lm", 1e-3, True)]


def test_frame_weights_take_an_array_or_a_callable():
    from flash.tracking import _frame_weights
    pts = np.arange(12.0).reshape(4, 3)
    assert _frame_weights(None, pts) is None
    assert np.array_equal(_frame_weights([1, 0, 2, 1], pts), [1.0, 0.0, 2.0, 1.0])
    assert np.array_equal(_frame_weights(lambda p: p[:, 2], pts), pts[:, 2])
