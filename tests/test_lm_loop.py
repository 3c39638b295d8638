"""The native Levenberg-Marquardt loop fsdf_lm_minimize (host only, no GPU)
against flash.tracking.LevenbergMarquardt.optimize, which it restates operation
for operation, and the solver's way through tracking._optimize."""
import types

import numpy as np
import pytest

from gn_helpers import OracleCost, convergence_case


@pytest.fixture(scope="module")
def oracle_objective(oracle_mod):
    """x -> (c/n, g/n, H/n) of the convergence case over the CPU oracle, each x
    evaluated once (both loops visit the same points), and the start."""
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


@pytest.mark.parametrize("tolerance", [0.0, None])
def test_lm_minimize_matches_python_loop(oracle_objective, tolerance):
    """Same x, f, evaluations and final damping, bit for bit: iteration_limit 6
    with tolerance 0, and with a tolerance between the gradient norms of the
    accepted points, which stops the loop early."""
    from flash._lib import lm_minimize
    from flash.tracking import LevenbergMarquardt
    vgh, q0 = oracle_objective
    if tolerance is None:
        # |g| at the points the full run accepts falls from the start's; a
        # tolerance just above the third accepted point's stops both loops there
        norms = []

        def rec(x):
            f, g, H = vgh(x)
            norms.append((f, float(np.sqrt(sum(float(v) * float(v) for v in g)))))
            return f, g, H

        LevenbergMarquardt(len(q0), iteration_limit=6, gradient_convergence_tolerance=0.0).optimize(rec, q0)
        best, accepted = np.inf, []
        for f, nrm in norms:
            if f < best:
                best = f
                accepted.append(nrm)
        assert len(accepted) >= 3
        tolerance = accepted[2] * 1.000001
    solver = LevenbergMarquardt(len(q0), iteration_limit=6, gradient_convergence_tolerance=tolerance)
    x_py, f_py = solver.optimize(vgh, q0)
    x, f, its, lam = lm_minimize(vgh, q0, 6, solver.damping, solver.max_step, tolerance)
    assert its == solver.iterations and (its < 6) == (tolerance > 0)
    assert np.array_equal(x, x_py) and f == f_py and lam == solver.final_damping
    assert not np.array_equal(x, q0)


def test_lm_minimize_zero_iterations():
    from flash._lib import lm_minimize
    x0 = np.array([1.0, -2.0])
    x, f, its, lam = lm_minimize(lambda x: pytest.fail("no evaluation expected"), x0, 0, 1e-3, 0.5, 0.0)
    assert np.array_equal(x, x0) and f is None and its == 0 and lam == 1e-3


def test_lm_minimize_objective_status_ends_the_loop():
    """A nonzero return of the objective ends the loop with that status; x is
    the last accepted point."""
    from flash import _lib
    calls = []

    def vgh(x):
        calls.append(x.copy())
        if len(calls) == 3:
            return 7
        return float(x @ x), 2.0 * x, 2.0 * np.eye(len(x))

    with pytest.raises(_lib.FlashNativeError) as e:
        _lib.lm_minimize(vgh, np.array([3.0, -4.0, 0.5]), 10, 1e-3, 0.5, 0.0)
    assert e.value.status == 7 and len(calls) == 3
    # the raw entry point: x holds the last accepted point, the count the evaluations made
    n = 3
    x = np.array([3.0, -4.0, 0.5])
    seen = []

    def raw(_user, px, pf, pg, pH):
        xs = np.ctypeslib.as_array(px, (n,)).copy()
        seen.append(xs)
        if len(seen) == 3:
            return 7
        pf[0] = float(xs @ xs)
        np.ctypeslib.as_array(pg, (n,))[:] = 2.0 * xs
        np.ctypeslib.as_array(pH, (n, n))[:] = 2.0 * np.eye(n)
        return 0

    import ctypes
    cb = _lib.VGH_FN(raw)
    work = np.empty(3 * n * n + 5 * n)
    f, its, lam = ctypes.c_double(0.0), ctypes.c_int32(0), ctypes.c_double(0.0)
    st = _lib.load().fsdf_lm_minimize(ctypes.cast(cb, ctypes.c_void_p), None, n, _lib.ptr(x), 10, 1e-3, 0.5, 0.0,
                                      _lib.ptr(work), ctypes.byref(f), ctypes.byref(its), ctypes.byref(lam))
    assert st == 7 and its.value == 2
    assert np.array_equal(x, seen[1]) and f.value == float(seen[1] @ seen[1])


def test_lm_minimize_always_degenerate_hessian():
    """H = 0: every step is degenerate, the damping rises tenfold without an
    evaluation until it passes 1e12 — one evaluation in all."""
    from flash._lib import lm_minimize
    from flash.tracking import LevenbergMarquardt
    calls = []

    def vgh(x):
        calls.append(1)
        return 1.0, np.ones(4), np.zeros((4, 4))

    x0 = np.arange(4.0)
    x, f, its, lam = lm_minimize(vgh, x0, 30, 1e-3, 0.5, 0.0)
    assert len(calls) == 1 and its == 1 and lam > 1e12 and f == 1.0 and np.array_equal(x, x0)
    solver = LevenbergMarquardt(4, iteration_limit=30, gradient_convergence_tolerance=0.0)
    solver.optimize(vgh, x0)
    assert solver.final_damping == lam and solver.iterations == 1


def test_lm_minimize_python_exception_is_raised_again():
    from flash._lib import lm_minimize

    def vgh(x):
        raise KeyError("objective")

    with pytest.raises(KeyError):
        lm_minimize(vgh, np.zeros(2), 5, 1e-3, 0.5, 0.0)


class _StandIn:
    """A native rigid functor as tracking._optimize sees one: a quadratic bowl."""
    _native = True

    def __init__(self, n):
        self.A = np.diag(np.arange(1.0, n + 1.0))
        self.evaluations = 0

    def value_gradient_hessian(self, x):
        self.evaluations += 1
        return float(x @ self.A @ x), 2.0 * self.A @ x, 2.0 * self.A


def test_optimize_runs_lm_with_callback_once_per_evaluation():
    from flash.tracking import LevenbergMarquardt, _optimize
    cost = _StandIn(5)
    x0 = np.linspace(-0.3, 0.4, 5)
    seen = []
    solver = LevenbergMarquardt(5, iteration_limit=8, gradient_convergence_tolerance=1e-9)
    x = _optimize(cost, 10, x0, lambda x, c: seen.append((x.copy(), c)), solver)
    assert solver.iterations == cost.evaluations == len(seen) >= 2
    assert all(c == float(xs @ cost.A @ xs) for xs, c in seen)
    assert np.array_equal(seen[0][0], x0)
    assert float(x @ cost.A @ x) < 1e-6 * float(x0 @ cost.A @ x0)
    # the objective handed to the solver is (c/n, g/n, H/n)
    ref = LevenbergMarquardt(5, iteration_limit=8, gradient_convergence_tolerance=1e-9)
    bowl = _StandIn(5)
    x_ref, _ = ref.optimize(lambda v: tuple(t / 10 for t in bowl.value_gradient_hessian(v)), x0)
    assert np.array_equal(x, x_ref)


def test_optimize_still_refuses_non_rigid_or_non_native():
    from flash.tracking import LevenbergMarquardt, _optimize
    for cost in (types.SimpleNamespace(_native=False, value_gradient_hessian=None),
                 types.SimpleNamespace(_native=True, rigid=False, value_gradient_hessian=None),
                 types.SimpleNamespace(_native=True)):
        with pytest.raises(NotImplementedError):
            _optimize(cost, 10, np.zeros(6), None, LevenbergMarquardt(6))
