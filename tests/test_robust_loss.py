"""Robust point losses on the CPU (flash.robust, csrc/robust_impl.h's numpy
twins): the loss functions themselves, the robust objective Σρ(d*) with its
IRLS wrench and moments over the CPU oracle, what the loss does to the drift
cases of tests/test_lm_prior.py, and the way tracking._optimize hands a loss
to the functor."""
import types

import numpy as np
import pytest

from gn_helpers import IU, OracleCost, point_vectors

SCALES = (0.02, 0.05, 0.125, 3.0)


def _losses():
    from flash.robust import Huber, Tukey
    return [cls(c) for cls in (Huber, Tukey) for c in SCALES]


# ---- 1. the twins ---------------------------------------------------------------------

def test_exported_from_the_package():
    import flash
    from flash import robust
    assert flash.Huber is robust.Huber and flash.Tukey is robust.Tukey
    assert (robust.Huber(0.1).kind, robust.Tukey(0.1).kind) == (1, 2)
    assert robust.parse("huber:0.02") == robust.Huber(0.02) and robust.parse("tukey:0.05") == robust.Tukey(0.05)
    assert robust.parse(None) is None and robust.parse("square") is None
    with pytest.raises(ValueError):
        robust.parse("cauchy:1")


@pytest.mark.parametrize("loss", _losses(), ids=repr)
def test_rho_is_continuous_and_its_derivative_is_2wd(loss):
    """ρ is continuous at c (one ulp of ρ(c) either side: ρ′ is bounded by 2c);
    w(0) = 1 and ρ(0) = 0; ρ′ = 2 w d against central differences of ρ in
    longdouble (h = 1e-6 c: truncation h² ρ‴/6 <= 1e-11 relative to ρ′'s scale
    2c, rounding 2^-64 ρ / h ~ 1e-13) at 1e-7 relative — at points on both
    sides of c, both signs, none within h of the kink."""
    c = loss.scale
    for side in (-1.0, 1.0):
        at, below, above = (loss.rho(np.array([side * v]))[0] for v in (c, np.nextafter(c, 0), np.nextafter(c, 2 * c)))
        assert abs(at - below) <= 4 * np.spacing(at) + 2 * c * np.spacing(c)
        assert abs(at - above) <= 4 * np.spacing(at) + 2 * c * np.spacing(c)
    zero = np.zeros(1)
    assert loss.weight(zero)[0] == 1.0 and loss.rho(zero)[0] == 0.0
    assert loss.weight(np.float64(0.0)) == 1.0
    u = np.array([1e-3, 0.1, 0.5, 0.9, 0.999, 1.001, 1.5, 4.0, 100.0])
    d = np.concatenate([u, -u]).astype(np.longdouble) * np.longdouble(c)
    h = np.longdouble(1e-6) * np.longdouble(c)
    w, fd = loss.weight(d), (loss.rho(d + h) - loss.rho(d - h)) / (2 * h)
    assert w.dtype == np.longdouble and fd.dtype == np.longdouble  # (dtype-preserving)
    assert loss.weight(d.astype(np.float64)).dtype == np.float64
    err = np.abs(2 * w * d - fd)
    assert (err <= 1e-7 * np.maximum(np.abs(fd), 2 * c * 1e-3)).all(), float(err.max())
    assert (w >= 0).all() and (w <= 1).all()
    # near zero the loss is the square, to Tukey's next term d⁴/c² and a few ulps of d²
    # (ρ keeps its relative accuracy there: no 1 − (1 − u²)³ cancellation)
    small = np.array([1e-9, -1e-7, 1e-3]) * c
    assert (np.abs(loss.rho(small) - small * small) <= small ** 4 / c ** 2 + 2.0 ** -50 * small * small).all()


@pytest.mark.parametrize("c", SCALES)
def test_tukey_rejects_exactly_beyond_its_scale(c):
    from flash.robust import Tukey
    t = Tukey(c)
    d = np.array([c, -c, np.nextafter(c, 2 * c), 2 * c, -17.0 * c, 1e300])
    assert np.array_equal(t.weight(d), np.zeros(6))
    assert np.array_equal(t.rho(d), np.full(6, (c * c) / 3))
    inside = np.array([np.nextafter(c, 0), -0.5 * c])
    assert (t.weight(inside) >= 0).all() and t.weight(inside)[1] == (1 - 0.25) ** 2
    assert (t.rho(inside) <= (c * c) / 3 + 2 * np.spacing((c * c) / 3)).all()  # (to rounding, one ulp below c)


@pytest.mark.parametrize("c", SCALES)
def test_huber_is_the_square_up_to_its_scale(c):
    from flash.robust import Huber
    hub = Huber(c)
    d = np.array([0.0, 0.5 * c, -c, c])
    assert np.array_equal(hub.weight(d), np.ones(4)) and np.array_equal(hub.rho(d), d * d)
    far = np.array([2 * c, -4 * c])
    assert np.array_equal(hub.weight(far), [0.5, 0.25])
    assert np.allclose(hub.rho(far), [3 * c * c, 7 * c * c], rtol=1e-15)


@pytest.mark.parametrize("bad", [0.0, -0.02, float("nan"), float("inf")])
def test_bad_scales_raise(bad):
    from flash.robust import Huber, Tukey
    for cls in (Huber, Tukey):
        with pytest.raises(ValueError):
            cls(bad)


# ---- 2. the robust objective over the CPU oracle ------------------------------------------

class RobustOracleCost(OracleCost):
    """OracleCost with a loss: c = Σρ(d*), the wrench Σ 2 w d* v and the moments
    Σ w v vᵀ with the twin's w (the IRLS model of include/flashsdf.h "robust
    point losses"); loss None is OracleCost itself."""

    def __init__(self, m, pts, loss=None):
        super().__init__(m, pts)
        self.loss = loss

    def _weights(self, d):
        return np.ones_like(d) if self.loss is None else self.loss.weight(d)

    def value_and_gradient(self, x):
        x = np.asarray(x, np.float64)
        d, k, g = self.per_point(x)
        mech = self.m.mechanism
        wrench = point_vectors(self.pts, g) * (2.0 * self._weights(d) * d)[:, None]
        bw = np.zeros((mech.num_bodies, 6))
        np.add.at(bw, self.sb[k], wrench)
        cost = float(d @ d) if self.loss is None else float(self.loss.rho(d).sum())
        return cost, mech.config_gradient_numpy(x, bw), (d, k, g)

    def __call__(self, x):
        c, gq, (d, k, g) = self.value_and_gradient(x)
        v, w = point_vectors(self.pts, g), self._weights(d)
        mom = np.zeros((len(self.sb), 21))
        for s in range(len(self.sb)):
            sel = k == s
            mom[s] = ((v[sel] * w[sel, None]).T @ v[sel])[IU]
        return c, gq, 2.0 * self.m.mechanism.gauss_newton_matrix_numpy(x, self.sb, mom)


@pytest.fixture(scope="module", params=[41, 7, 19])
def drift_scene(request, oracle_mod):
    """tests/test_lm_prior.py's drift cases: IRB140, 3,000 points of
    synthetic.depth_cloud at its defaults (10 % box outliers, 5 % interior)."""
    from flash import Models, synthetic
    seed = request.param
    m = Models.irb140()
    q_true, q0 = synthetic.perturbed_configuration(m, seed)
    pts = synthetic.depth_cloud(m, q_true, 3000, seed=seed + 1)
    return seed, m, pts, np.asarray(q_true, np.float64), np.asarray(q0, np.float64)


@pytest.mark.parametrize("spec", ["huber:0.02", "tukey:0.05"])
def test_robust_gradient_matches_central_differences(drift_scene, spec):
    """∂(Σρ)/∂x by the chain rule on the robust wrench against central
    differences of Σρ itself (h = 1e-6): |g − g_fd|_∞ <= 1e-7 |g|_∞ at the
    cases' starts. ρ is C¹ (ρ″ jumps at c for Huber): the difference's
    truncation is O(h² |ρ‴|) away from the kinks and O(h) ρ″-jump on the few
    points within h·|∇d| of one — measured 1e-10 .. 1e-9 relative."""
    from flash import robust
    seed, m, pts, _, q0 = drift_scene
    oc = RobustOracleCost(m, pts, robust.parse(spec))
    c, g, _ = oc.value_and_gradient(q0)
    h, eye = 1e-6, np.eye(len(q0))
    g_fd = np.array([(oc.value_and_gradient(q0 + h * e)[0] - oc.value_and_gradient(q0 - h * e)[0]) / (2 * h)
                     for e in eye])
    err, scale = float(np.abs(g - g_fd).max()), float(np.abs(g).max())
    print(f"seed {seed} {spec}: c {c:.6f} |g|_inf {scale:.4f} |g - g_fd|_inf {err:.2e}")
    assert scale > 0 and err <= 1e-7 * scale, (err, scale)


def test_robust_oracle_without_a_loss_is_the_oracle_cost(drift_scene):
    _, m, pts, _, q0 = drift_scene
    plain, robust_none = OracleCost(m, pts), RobustOracleCost(m, pts, None)
    a, b = plain(q0), robust_none(q0)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    assert np.allclose(a[2], b[2], rtol=0, atol=1e-12 * np.abs(a[2]).max())


# ---- 3. what the loss does to the drift cases -----------------------------------------------

def test_huber_with_the_prior_recovers_the_observed_joints(drift_scene):
    """10 LM evaluations, damping 1e-3, max_step 0.5, tolerance 0, prior
    μ = 1e-3 about the start, which is 0.07 – 0.12 rad off on joints 1–3
    (err123 = max |q − q_true| over them). The cloud's 10 % box outliers bias
    the least-squares solution; Huber(0.02) bounds their pull.

    Measured (seed: least squares err123 -> Huber 0.02 err123; c/N at the end
    least squares / Huber):
      41: 0.1114 -> 0.0135; 1.03e-2 / 1.27e-3
       7: 0.0851 -> 0.0269; 9.8e-3 / 1.26e-3
      19: 0.0335 -> 0.0152; 1.20e-2 / 1.38e-3
    Conditions: Huber err123 <= 0.03 and <= half the least-squares run's, whose
    own err123 >= 0.03 is the negative control."""
    from flash.robust import Huber
    from flash.tracking import LevenbergMarquardt, state_prior
    seed, m, pts, q_true, q0 = drift_scene
    n = float(len(pts))

    def run(loss):
        oc = RobustOracleCost(m, pts, loss)

        def vgh(x):
            c, g, H = oc(x)
            return c / n, g / n, H / n

        s = LevenbergMarquardt(len(q0), damping=1e-3, max_step=0.5, iteration_limit=10,
                               gradient_convergence_tolerance=0.0)
        x, f = s.optimize(state_prior(vgh, q0, 1e-3), q0)
        assert s.iterations == 10
        return float(np.abs(x - q_true)[:3].max()), vgh(x)[0]

    e_ls, f_ls = run(None)
    e_hub, f_hub = run(Huber(0.02))
    print(f"seed {seed}: start err123 {np.abs(q0 - q_true)[:3].max():.4f}; least squares {e_ls:.4f} (c/N {f_ls:.3e}); "
          f"Huber 0.02 {e_hub:.4f} (c/N {f_hub:.3e})")
    assert e_ls >= 0.03, e_ls  # (the negative control)
    assert e_hub <= 0.03, e_hub
    assert e_hub <= 0.5 * e_ls, (e_hub, e_ls)


# ---- 4. tracking._optimize hands the loss to the functor -----------------------------------

def test_optimize_hands_the_loss_to_the_functor():
    """_optimize(..., loss=) sets the functor's loss before the native loop is
    entered (the stand-in of test_optimize_hands_prior_and_loop_to_the_native_path
    with a set_loss); without loss= the functor is left as it is."""
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
                                 descend=descend, set_loss=lambda loss: calls.append(("set_loss", loss)))
    loss = Huber(0.02)
    solver = LevenbergMarquardt(3, iteration_limit=7, prior_weight=1e-3, device_loop=True)
    x = _optimize(cost, 12, np.zeros(3), None, solver, loss=loss)
    assert np.array_equal(x, np.ones(3)) and solver.iterations == 3
    assert calls == [("set_loss", loss), ("descend_lm", 1e-3, True)]
    del calls[:]
    x = _optimize(cost, 12, np.zeros(3), None, NaiveSolver(3, iteration_limit=5), loss=loss)
    assert np.array_equal(x, -np.ones(3)) and calls == [("set_loss", loss), ("descend", 5, 12)]
    del calls[:]
    _optimize(cost, 12, np.zeros(3), None, solver)
    assert calls == [("descend_lm", 1e-3, True)]


def test_optimize_callback_sees_the_functors_cost_with_a_loss():
    """With a callback the Python loop runs over the functor's
    value_gradient_hessian — the robust one once set_loss ran — and the
    callback gets its raw cost."""
    from flash.robust import Tukey
    from flash.tracking import LevenbergMarquardt, _optimize

    class StandIn:
        _native = True
        loss = None

        def set_loss(self, loss):
            self.loss = loss

        def value_gradient_hessian(self, x):
            s = 1.0 if self.loss is None else 0.5
            return s * float(x @ x), s * 2.0 * x, s * 2.0 * np.eye(len(x))

    cost, seen = StandIn(), []
    solver = LevenbergMarquardt(3, iteration_limit=4, gradient_convergence_tolerance=0.0)
    x0 = np.array([0.3, -0.2, 0.1])
    _optimize(cost, 10, x0, lambda x, c: seen.append((x.copy(), c)), solver, loss=Tukey(0.05))
    assert cost.loss == Tukey(0.05) and len(seen) == solver.iterations == 4
    assert all(c == 0.5 * float(x @ x) for x, c in seen)
