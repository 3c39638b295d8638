"""CPU: robust objectives on RBF skins and deformations, host side (no GPU):
the numpy twins of the skins' robust blocks and weighted second moments
(flash/robust.py weighted_skin_blocks, weighted_skin_moments) against the
oracle's accumulator block and against central differences of the twin
objective, what a Huber loss buys on a cluttered deformable scene, and the
plumbing of `robust_skins` through CostFunctor and estimate_state / Tracker.

A skin's block under Σ a ρ(d*) is Σ 2 (aw d*) j and its Gauss-Newton term
Σ aw j jᵀ, aw = a · w(d*), w = ρ′/2d (include/flashsdf.h "robust objectives on
skins")."""
import types

import numpy as np
import pytest

from test_skin_gauss_newton import _build, _cloud, _fd_check, _solves

H_FD = 1e-6


class RobustTwinCost:
    """x -> (c, ∂c/∂x, H) of a one-skin scene under a robust objective: the
    oracle skin's d = s, c = Σ a ρ(s) + weight |δ|², the gradient
    L Σ 2 (aw s) j + 2 weight δ and the twin IRLS Gauss-Newton Hessian."""

    def __init__(self, m, pts, loss=None, weights=None, one_sided=None, weight=10.0):
        self.m, self.pts, self.weight = m, np.ascontiguousarray(pts, np.float64), weight
        self.loss, self.weights, self.one_sided = loss, weights, one_sided
        self.nq = m.mechanism.num_positions

    def __call__(self, x, hessian=True, gradient=True):
        import rbf as orbf  # oracle/rbf.py
        from flash import rbf, robust
        x = np.asarray(x, np.float64)
        r = _solves(self.m, x)[0]
        s = orbf.skin(r.centres, r.u, self.pts)[0]
        k = np.full(len(s), r.surface)
        _, arho = robust._point_factors(s, self.loss, self.weights, self.one_sided, "twin")
        delta = x[self.nq:]
        c = float(arho.sum()) + self.weight * float(delta @ delta)
        if not gradient:  # (central differences need the value alone)
            return c, None, None
        block = robust.weighted_skin_blocks(self.pts, k, s, [r], self.loss, self.weights, self.one_sided)[0]
        g = rbf.state_map(self.m, x, r) @ block
        g[self.nq:] += 2.0 * self.weight * delta
        if not hessian:
            return c, g, None
        M = robust.weighted_skin_moments(self.pts, k, s, [r], self.loss, self.weights, self.one_sided)
        return c, g, rbf.gauss_newton(self.m, x, [r], M, None, self.weight)


@pytest.mark.parametrize("name", ["beanbag", "squishable", "two_link_arm"])
def test_plain_blocks_are_the_oracle_accumulator_block(name, oracle_mod):
    """No loss, no weights, no split: Σ 2 d j, the skin block of OracleModel.cost_accum
    (test_skin_gauss_newton.py's tolerance for the same sums)."""
    import flash
    import rbf as orbf  # oracle/rbf.py
    from flash import rbf, robust
    m, x = _build(name)
    r = _solves(m, x)[0]
    pts = _cloud(r.centres, 50, 3)
    s = orbf.skin(r.centres, r.u, pts)[0]
    k = np.full(len(pts), r.surface)
    block = robust.weighted_skin_blocks(pts, k, s, [r])[0]
    om = oracle_mod.OracleModel.from_manipulator(m)
    nq = m.mechanism.num_positions
    poses = flash.core.surface_poses(m, m.mechanism.normalize(x[:nq]))
    want = om.cost_accum(poses, pts, rbf.rows([r]))[1 + 6 * len(m.surfaces):]
    assert np.allclose(block, want, rtol=1e-9, atol=1e-9 * np.abs(want).max()), np.abs(block - want).max()
    # the rows form of the same skin, and weights ≡ 1 / a Huber that never bends: the same bits
    rows = rbf.rows([r])
    assert np.array_equal(robust.weighted_skin_blocks(pts, k, s, [(r.surface, rows)])[0], block)
    assert np.array_equal(robust.weighted_skin_blocks(pts, k, s, [r], robust.Huber(1e30), np.ones(len(pts)))[0], block)
    # the moments without a factor are Σ j jᵀ (to the matrix product's own summation order)
    J = rbf.skin_jacobian(r.centres, r.u, pts)
    M, want = robust.weighted_skin_moments(pts, k, s, [r])[0], J.T @ J
    assert np.allclose(M, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    # points of another surface contribute nothing
    k2 = k.copy()
    k2[::2] = r.surface + 1
    half = robust.weighted_skin_blocks(pts, k2, s, [r])[0]
    assert np.array_equal(half, robust.weighted_skin_blocks(pts[1::2], k[1::2], s[1::2], [r])[0])


def _objectives(n, scale):
    from flash.robust import Huber, Tukey
    w = np.random.default_rng(8).uniform(0.0, 2.0, n)
    w[::7] = 0.0
    free = np.zeros(n, bool)
    free[n // 2:] = True
    return {"huber": dict(loss=Huber(scale)), "tukey": dict(loss=Tukey(3.0 * scale)),
            "weights": dict(weights=w), "huber+weights": dict(loss=Huber(scale), weights=w),
            "one_sided": dict(one_sided=free), "tukey+weights+one_sided": dict(loss=Tukey(3.0 * scale), weights=w,
                                                                             one_sided=free)}


@pytest.mark.parametrize("name", ["beanbag", "squishable", "two_link_arm"])
def test_twin_gradient_matches_central_differences(name, oracle_mod):
    """The robust twin objective's gradient against central differences at h and
    2h (test_skin_gauss_newton.py _fd_check: 10 x their disagreement + 1e-9 max)."""
    import rbf as orbf  # oracle/rbf.py
    m, x = _build(name)
    r = _solves(m, x)[0]
    pts = _cloud(r.centres, 120, 4)
    s = orbf.skin(r.centres, r.u, pts)[0]
    scale = float(np.median(np.abs(s)))  # (half the points beyond Huber's bend)
    for what, kw in _objectives(len(pts), scale).items():
        cost = RobustTwinCost(m, pts, **kw)
        c, g, _ = cost(x, hessian=False)

        def fd(h):
            out = np.empty_like(g)
            for i in range(len(x)):
                e = np.zeros(len(x))
                e[i] = h
                out[i] = (cost(x + e, gradient=False)[0] - cost(x - e, gradient=False)[0]) / (2 * h)
            return out

        f1, f2 = fd(H_FD), fd(2 * H_FD)
        print(f"{name} {what}: c {c:.4e}, |g| {np.linalg.norm(g):.3e}, max |g - fd| {np.abs(g - f1).max():.3e}")
        _fd_check(g, f1, f2, (name, what))


def _payoff_scene(n=1500, n_clutter=225):
    """squishable at its zero state: n points projected onto the skin, and the
    slab the clutter is drawn in (beyond the centres' box in x)."""
    import flash
    import rbf as orbf  # oracle/rbf.py
    from flash import Models
    m = Models.squishable()
    nq = m.mechanism.num_positions
    x_true = np.zeros(flash.num_states(m))
    x_true[:nq] = m.mechanism.zero_configuration()
    r = _solves(m, x_true)[0]
    pts = _cloud(r.centres, n, 21)
    for _ in range(30):  # Newton projection onto the zero set of the oracle skin
        s, gs = orbf.skin(r.centres, r.u, pts)
        step = -(s / (gs * gs).sum(1))[:, None] * gs
        nrm = np.linalg.norm(step, axis=1, keepdims=True)
        pts = pts + step * np.minimum(1.0, 0.2 / np.maximum(nrm, 1e-300))
    lo, hi = r.centres.min(0), r.centres.max(0)
    return m, x_true, pts, lo, hi


def payoff_cloud(pts, lo, hi, seed, n_clutter=225):
    """The surface points with N(0, 0.002 L) noise and 15 % clutter, uniform in
    the slab x ∈ [x_max + 0.05 L, x_max + 0.35 L], y and z inside the centres'
    box; L the centres' largest extent. Drawn from default_rng(seed + 100)."""
    L = float((hi - lo).max())
    rg = np.random.default_rng(seed + 100)
    noisy = pts + rg.normal(0.0, 0.002 * L, pts.shape)
    clutter = lo + (hi - lo) * rg.random((n_clutter, 3))
    clutter[:, 0] = hi[0] + 0.05 * L + 0.30 * L * rg.random(n_clutter)
    return np.concatenate([noisy, clutter]), L


def payoff_errors(m, x_true, x):
    """(translation error, max |δ|) of a solution against the true zero state."""
    nq = m.mechanism.num_positions
    e = next(e for e in m.mechanism.edges[1:] if e.joint.kind == "quaternion_floating")
    t = slice(e.q_offset + 4, e.q_offset + 7)
    return float(np.linalg.norm(x[t] - x_true[t])), float(np.abs(x[nq:] - x_true[nq:]).max())


@pytest.mark.parametrize("seed", [12, 7, 19])
def test_huber_halves_the_error_of_least_squares_on_the_cluttered_squishable(seed, oracle_mod):
    """LevenbergMarquardt, 30 evaluations on the twin objective / N: Huber(0.0075)'s
    translation error and max |δ| are each below half of least squares'."""
    from flash.robust import Huber
    from flash.tracking import LevenbergMarquardt
    m, x_true, pts, lo, hi = _payoff_scene()
    cloud, L = payoff_cloud(pts, lo, hi, seed)
    assert abs(L - 0.36997) < 1e-4 and len(cloud) == 1725
    x0 = x_true + np.random.default_rng(seed).normal(0.0, 0.03, len(x_true))
    n = float(len(cloud))
    out = {}
    for what, loss in (("least squares", None), ("huber", Huber(0.0075))):
        cost = RobustTwinCost(m, cloud, loss=loss)

        def vgh(x):
            c, g, H = cost(x)
            return c / n, g / n, H / n

        solver = LevenbergMarquardt(len(x0), iteration_limit=30)
        x, f = solver.optimize(vgh, x0)
        out[what] = payoff_errors(m, x_true, x)
        print(f"seed {seed} {what}: f {f:.4e} after {solver.iterations} evaluations, translation error "
              f"{out[what][0]:.4f}, max |delta| {out[what][1]:.4f}")
    (t_ls, d_ls), (t_h, d_h) = out["least squares"], out["huber"]
    assert t_h < 0.5 * t_ls, (t_h, t_ls)
    assert d_h < 0.5 * d_ls, (d_h, d_ls)


# ---- plumbing ------------------------------------------------------------------------------

def test_optimize_turns_robust_skins_on_before_the_loss():
    from flash.robust import Huber
    from flash.tracking import LevenbergMarquardt, NaiveSolver, _optimize
    calls = []

    def descend(x, limit, rate, max_step, tol, div, n):
        calls.append(("descend", limit, n))
        return x - 1.0, 0.25, 2

    def descend_lm(x, limit, damping, max_step, tol, n, prior_weight=None, device_loop=None):
        calls.append(("descend_lm",))
        return x + 1.0, 0.5, 3, 1e-5

    cost = types.SimpleNamespace(_native=True, rigid=False, skin_hessian=False, value_gradient_hessian=None,
                                 descend=descend, descend_lm=descend_lm,
                                 set_loss=lambda loss: calls.append(("set_loss", loss)),
                                 set_point_weights=lambda w: calls.append(("set_point_weights", len(w))),
                                 set_robust_skins=lambda on: calls.append(("set_robust_skins", on)),
                                 set_skin_hessian=lambda on: calls.append(("set_skin_hessian", on)))
    loss = Huber(0.02)
    _optimize(cost, 12, np.zeros(3), None, NaiveSolver(3, iteration_limit=5), loss=loss, weights=np.ones(12),
              robust_skins=True)
    assert calls == [("set_robust_skins", True), ("set_loss", loss), ("set_point_weights", 12), ("descend", 5, 12)]
    del calls[:]
    _optimize(cost, 12, np.zeros(3), None, LevenbergMarquardt(3, skins=True), loss=loss, robust_skins=True)
    assert calls == [("set_robust_skins", True), ("set_loss", loss), ("set_skin_hessian", True), ("descend_lm",)]
    del calls[:]
    _optimize(cost, 12, np.zeros(3), None, NaiveSolver(3, iteration_limit=5), loss=loss)  # (the functor as it is)
    assert calls == [("set_loss", loss), ("descend", 5, 12)]


def test_estimate_state_and_tracker_forward_robust_skins(monkeypatch):
    from flash import tracking
    from flash.robust import Huber
    made = []

    class FakeCost:
        _native, rigid, n_points = True, False, 4

        def __init__(self, manipulator, pts, device=0, precision=64, robust_skins=False):
            self.robust_skins, self.calls = robust_skins, []
            made.append(self)

        def set_robust_skins(self, on):
            self.calls.append(("set_robust_skins", on))

        def set_loss(self, loss):
            self.calls.append(("set_loss", loss))

        def set_sensed_points(self, pts):
            pass

        def descend(self, x, *a):
            return x, 0.0, 1

    monkeypatch.setattr(tracking, "CostFunctor", FakeCost)
    solver = tracking.NaiveSolver(3, iteration_limit=1)
    loss = Huber(0.01)
    tracking.estimate_state(None, np.zeros((4, 3)), np.zeros(3), solver=solver, loss=loss, robust_skins=True)
    assert made[-1].robust_skins is True and made[-1].calls == [("set_robust_skins", True), ("set_loss", loss)]
    tracking.estimate_state(None, np.zeros((4, 3)), np.zeros(3), solver=solver, loss=loss)
    assert made[-1].robust_skins is False and made[-1].calls == [("set_loss", loss)]
    state = types.SimpleNamespace()
    monkeypatch.setattr(tracking, "flatten", lambda s: np.zeros(3))
    monkeypatch.setattr(tracking, "unflatten", lambda s, x: None)
    tr = tracking.Tracker(None, state, solver, loss=loss, robust_skins=True)
    assert made[-1].robust_skins is True and tr.robust_skins is True
    tr.step(np.zeros((4, 3)))
    assert made[-1].calls == [("set_robust_skins", True), ("set_loss", loss)]
    xs, tr = tracking.track(None, [np.zeros((4, 3))], state, solver, loss=loss, robust_skins=True)
    assert made[-1].robust_skins is True and len(xs) == 1
    xs, tr = tracking.track(None, [np.zeros((4, 3))], state, solver, loss=loss)
    assert made[-1].robust_skins is False and made[-1].calls == [("set_loss", loss)]


def test_functor_refuses_a_non_rigid_scene_without_the_switch():
    """CostFunctor.set_loss / set_point_weights / set_free_split on a native scene
    with a skin: NotImplementedError as before, accepted once robust_skins is on."""
    from flash.gradientdescent import CostFunctor
    from flash.robust import Huber
    seen = []
    ctx = types.SimpleNamespace(loss=None, robust_skins=False,
                                set_loss=lambda loss: seen.append(("set_loss", loss)),
                                set_point_weights=lambda w: seen.append(("set_point_weights", None if w is None else len(w))),
                                set_free_split=lambda n: seen.append(("set_free_split", n)))

    def set_robust_skins(on):
        ctx.robust_skins = on
        seen.append(("set_robust_skins", on))

    ctx.set_robust_skins = set_robust_skins
    cf = CostFunctor.__new__(CostFunctor)
    cf._native, cf.rigid, cf.robust_skins, cf.ctx, cf.n_points, cf.n_surface = True, False, False, ctx, 10, 10
    cf.loss = cf.point_weights = None
    cf._ensure_resident = lambda: None
    with pytest.raises(NotImplementedError):
        cf.set_loss(Huber(0.1))
    with pytest.raises(NotImplementedError):
        cf.set_point_weights(np.ones(10))
    with pytest.raises(NotImplementedError):
        cf.set_free_split(5)
    assert seen == [] and cf.loss is None and cf.n_surface == 10
    cf.set_robust_skins(True)
    cf.set_loss(Huber(0.1))
    cf.set_point_weights(np.ones(10))
    cf.set_free_split(5)
    assert seen == [("set_robust_skins", True), ("set_loss", Huber(0.1)), ("set_point_weights", 10),
                    ("set_free_split", 5)]
    assert cf.loss == Huber(0.1) and cf.n_surface == 5
    # a scene that is not native-capable has no switch to turn
    cf2 = CostFunctor.__new__(CostFunctor)
    cf2._native = False
    with pytest.raises(NotImplementedError):
        cf2.set_robust_skins(True)
