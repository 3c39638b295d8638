"""The prior on the frame's start state (flash.tracking.state_prior,
LevenbergMarquardt(prior_weight=...), fsdf_set_lm_prior's arithmetic) on the
CPU: its derivatives, the bit-identical Python and native loops over the
wrapped objective, and the drift of weakly observed joints it stops."""
import types

import numpy as np
import pytest

from gn_helpers import OracleCost, convergence_case


def _toy(x):
    """A smooth objective with a dense Hessian."""
    x = np.asarray(x, np.float64)
    A = np.array([[2.0, 0.3, -0.1], [0.3, 1.5, 0.2], [-0.1, 0.2, 0.8]])
    f = float(0.5 * x @ A @ x + np.sin(x[0]) * x[2])
    g = A @ x + np.array([np.cos(x[0]) * x[2], 0.0, np.sin(x[0])])
    H = A.copy()
    H[0, 0] += -np.sin(x[0]) * x[2]
    H[0, 2] += np.cos(x[0])
    H[2, 0] += np.cos(x[0])
    return f, g, H


def test_state_prior_matches_central_differences():
    from flash.tracking import state_prior
    x_ref = np.array([0.3, -0.2, 0.7])
    mu = np.array([1e-3, 0.0, 2.5])
    F = state_prior(_toy, x_ref, mu)
    x = np.array([0.45, 0.1, 0.2])
    f0, g0, H0 = _toy(x)
    f, g, H = F(x)
    # f − r is the wrapped f exactly: r added once, summed in index order from 0.0
    r = 0.0
    for m, e in zip(mu, x - x_ref):
        r += float(m) * (float(e) * float(e))
    assert f == f0 + r and r > 0.0
    assert np.isclose(r, float(mu @ (x - x_ref) ** 2), rtol=1e-14)
    # r's gradient and Hessian against central differences of r itself
    def prior(v):
        return F(v)[0] - _toy(v)[0]
    h = 1e-5
    eye = np.eye(3)
    g_fd = np.array([(prior(x + h * eye[i]) - prior(x - h * eye[i])) / (2 * h) for i in range(3)])
    assert np.allclose(g - g0, g_fd, rtol=1e-6, atol=1e-10)
    assert np.array_equal(g, g0 + (2.0 * mu) * (x - x_ref))
    # (r is quadratic: its second difference is exact up to rounding, ~1e-16 |F| / k^2 = 1e-10 at k = 1e-3)
    k = 1e-3
    d2 = np.array([(prior(x + k * eye[i]) - 2 * prior(x) + prior(x - k * eye[i])) / k ** 2 for i in range(3)])
    assert np.allclose(np.diag(H - H0), d2, rtol=1e-6, atol=1e-8)
    assert np.array_equal(np.diag(H), np.diag(H0) + 2.0 * mu)
    off = ~np.eye(3, dtype=bool)
    assert np.array_equal(H[off], H0[off])
    # the whole wrapped objective: gradient against central differences of F
    gF = np.array([(F(x + h * eye[i])[0] - F(x - h * eye[i])[0]) / (2 * h) for i in range(3)])
    assert np.allclose(g, gF, rtol=1e-6, atol=1e-9)
    # a scalar weight is one weight per coordinate
    fs, gs, Hs = state_prior(_toy, x_ref, 0.5)(x)
    fv, gv, Hv = state_prior(_toy, x_ref, np.full(3, 0.5))(x)
    assert fs == fv and np.array_equal(gs, gv) and np.array_equal(Hs, Hv)


def test_state_prior_none_is_the_objective_itself():
    from flash.tracking import state_prior
    out = (1.5, np.arange(3.0), np.eye(3))
    F = state_prior(lambda x: out, np.zeros(3), None)
    got = F(np.ones(3))
    assert got is out
    with pytest.raises(ValueError):
        state_prior(_toy, np.zeros(3), -1.0)
    with pytest.raises(ValueError):
        state_prior(_toy, np.zeros(3), np.array([0.0, np.nan, 1.0]))


@pytest.fixture(scope="module")
def oracle_objective(oracle_mod):
    """x -> (c/n, g/n, H/n) of the convergence case over the CPU oracle, each x
    evaluated once, and the start (tests/test_lm_loop.py's)."""
    m, pts, _, q0 = convergence_case()
    oc = OracleCost(m, pts)
    n = float(len(pts))
    seen = {}

    def vgh(x):
        key = np.asarray(x, np.float64).tobytes()
        if key not in seen:
            c, g, H = oc(x)
            seen[key] = (c / n, g / n, H / n)
        return seen[key]

    return vgh, q0


@pytest.mark.parametrize("mu", [1e-3, np.array([0.0, 1e-3, 0.0, 2e-2, 5e-3, 1e-1])], ids=["scalar", "vector"])
def test_python_and_native_loops_match_with_prior(oracle_objective, mu):
    """LevenbergMarquardt.optimize and fsdf_lm_minimize over the same
    state_prior-wrapped oracle objective: x, f, evaluations and the final
    damping bit for bit — and not the run without the prior."""
    from flash._lib import lm_minimize
    from flash.tracking import LevenbergMarquardt, state_prior
    vgh, q0 = oracle_objective
    F = state_prior(vgh, q0, mu)
    solver = LevenbergMarquardt(len(q0), iteration_limit=6, gradient_convergence_tolerance=0.0)
    x_py, f_py = solver.optimize(F, q0)
    x, f, its, lam = lm_minimize(F, q0, 6, solver.damping, solver.max_step, 0.0)
    assert its == solver.iterations == 6
    assert np.array_equal(x, x_py) and f == f_py and lam == solver.final_damping
    plain = LevenbergMarquardt(len(q0), iteration_limit=6, gradient_convergence_tolerance=0.0)
    x_plain, _ = plain.optimize(vgh, q0)
    assert not np.array_equal(x, x_plain) and not np.array_equal(x, q0)


# ---- the drift of weakly observed joints (IRB140, 3,000 noisy points) ----------

@pytest.fixture(scope="module", params=[41, 7, 19])
def drift_case(request, oracle_mod):
    from flash import Models, synthetic
    seed = request.param
    m = Models.irb140()
    q_true, q0 = synthetic.perturbed_configuration(m, seed)
    pts = synthetic.depth_cloud(m, q_true, 3000, seed=seed + 1)
    oc = OracleCost(m, pts)
    n = float(len(pts))
    seen = {}

    def vgh(x):
        key = np.asarray(x, np.float64).tobytes()
        if key not in seen:
            c, g, H = oc(x)
            seen[key] = (c / n, g / n, H / n)
        return seen[key]

    return vgh, np.asarray(q_true, np.float64), np.asarray(q0, np.float64)


def test_prior_stops_the_drift(drift_case):
    """4 evaluations, damping 1e-3, max_step 0.5, tolerance 0. Without the
    prior Gauss-Newton pushes the wrist joints >= 0.5 rad off (measured 1.07,
    1.39, 1.52 rad for seeds 41, 7, 19); with mu = 1e-3 the state stays within
    0.2 rad of the truth (measured 0.112, 0.114, 0.033) and within a quarter of
    the run without, and the cost still ends below the start's."""
    from flash.tracking import LevenbergMarquardt, state_prior
    vgh, q_true, q0 = drift_case

    def run(weight):
        s = LevenbergMarquardt(len(q0), damping=1e-3, max_step=0.5, iteration_limit=4,
                               gradient_convergence_tolerance=0.0)
        x, _ = s.optimize(state_prior(vgh, q0, weight), q0)
        return x, float(np.max(np.abs(x - q_true)))

    _, err_plain = run(None)
    x, err = run(1e-3)
    print(f"start {np.max(np.abs(q0 - q_true)):.3f} plain {err_plain:.3f} prior {err:.3f} "
          f"c/N {vgh(x)[0]:.6f} start c/N {vgh(q0)[0]:.6f}")
    assert err_plain >= 0.5  # (the negative control)
    assert err <= 0.2 and err <= 0.25 * err_plain
    assert vgh(x)[0] < vgh(q0)[0]


class _StandIn:
    """A native rigid functor as tracking._optimize sees one (no descend_lm:
    the Python loop)."""
    _native = True

    def __init__(self, n):
        self.A = np.diag(np.arange(1.0, n + 1.0))

    def value_gradient_hessian(self, x):
        return float(x @ self.A @ x), 2.0 * self.A @ x, 2.0 * self.A


def test_optimize_applies_the_prior_on_the_callback_path():
    """_optimize wraps (c/n, g/n, H/n) in state_prior about the warm start; the
    callback still sees the raw cost once per evaluation."""
    from flash.tracking import LevenbergMarquardt, _optimize, state_prior
    cost = _StandIn(4)
    x0 = np.linspace(-0.3, 0.4, 4)
    mu = np.array([0.0, 0.5, 0.0, 2.0])
    seen = []
    solver = LevenbergMarquardt(4, iteration_limit=5, gradient_convergence_tolerance=0.0, prior_weight=mu)
    x = _optimize(cost, 10, x0, lambda xs, c: seen.append((xs.copy(), c)), solver)
    assert solver.iterations == len(seen) == 5
    assert all(c == float(xs @ cost.A @ xs) for xs, c in seen)
    ref = LevenbergMarquardt(4, iteration_limit=5, gradient_convergence_tolerance=0.0)
    bowl = _StandIn(4)
    x_ref, _ = ref.optimize(state_prior(lambda v: tuple(t / 10 for t in bowl.value_gradient_hessian(v)), x0, mu), x0)
    assert np.array_equal(x, x_ref)
    plain = LevenbergMarquardt(4, iteration_limit=5, gradient_convergence_tolerance=0.0)
    assert not np.array_equal(x, _optimize(_StandIn(4), 10, x0, None, plain))


def test_optimize_hands_prior_and_loop_to_the_native_path():
    """Without a callback a native functor's descend_lm gets the solver's
    prior_weight and device_loop."""
    from flash.tracking import LevenbergMarquardt, _optimize
    got = {}

    def descend_lm(x, limit, damping, max_step, tol, n, prior_weight=None, device_loop=None):
        got.update(prior_weight=prior_weight, device_loop=device_loop, limit=limit, n=n)
        return x + 1.0, 0.5, 3, 1e-5

    cost = types.SimpleNamespace(_native=True, rigid=True, value_gradient_hessian=None, descend_lm=descend_lm)
    solver = LevenbergMarquardt(3, iteration_limit=7, prior_weight=1e-3, device_loop="require")
    x = _optimize(cost, 12, np.zeros(3), None, solver)
    assert np.array_equal(x, np.ones(3)) and solver.iterations == 3 and solver.final_damping == 1e-5
    assert got == dict(prior_weight=1e-3, device_loop="require", limit=7, n=12)
