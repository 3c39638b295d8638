"""Host side of the second-order tracking solver (no GPU): the Gauss-Newton
matrix fsdf_gauss_newton_matrix against its numpy twin and against finite
differences of the CPU oracle, its algebraic properties, the damped step
fsdf_lm_step, and the Levenberg-Marquardt loop's convergence over the oracle.

The cost is c = Σ_p d*(p)², so with J = ∂d*/∂x the Gauss-Newton Hessian is
2 JᵀJ, and JᵀJ = Σ_k S_b(k) M_k S_b(k)ᵀ from the per-surface second moments
M_k = Σ w wᵀ, w = (∇d*, p × ∇d*) (include/flashsdf.h)."""
import numpy as np
import pytest

from gn_helpers import (OracleCost, convergence_case, floating_scene, moments_numpy, random_psd_moments,
                        surface_bodies)


def _scene(name):
    """(manipulator, x): x un-normalised where the scene has quaternions."""
    from flash import Models, synthetic
    if name == "floating":
        m, _, x0 = floating_scene(100)
        x0[0:4] = np.array([0.9, 0.1, -0.2, 0.3]) * 1.3  # base quaternion: rotated, |q| != 1
        return m, x0
    m = Models.irb140() if name == "irb140" else Models.arm_grid()
    return m, np.asarray(synthetic.perturbed_configuration(m, 41)[1], np.float64)


@pytest.mark.parametrize("name", ["irb140", "floating", "m64"])
def test_native_matrix_matches_numpy_twin(name):
    m, x = _scene(name)
    sb = surface_bodies(m)
    mom = random_psd_moments(len(sb), 7)
    A = m.mechanism.gauss_newton_matrix(x, sb, mom)
    T = m.mechanism.gauss_newton_matrix_numpy(x, sb, mom)
    assert np.linalg.norm(T) > 0
    assert np.linalg.norm(A - T) <= 1e-12 * np.linalg.norm(T), np.linalg.norm(A - T) / np.linalg.norm(T)


@pytest.mark.parametrize("name", ["irb140", "floating", "m64"])
def test_matrix_properties(name):
    """Symmetric (exactly), positive semi-definite for PSD moments, and for
    quaternion joints A q̂ = 0: the rows carry the (I − q̂q̂ᵀ)/|q| projection."""
    m, x = _scene(name)
    sb = surface_bodies(m)
    A = m.mechanism.gauss_newton_matrix(x, sb, random_psd_moments(len(sb), 8))
    assert np.array_equal(A, A.T)
    ev = np.linalg.eigvalsh(A)
    assert ev[-1] > 0 and ev[0] >= -1e-12 * ev[-1], ev[0] / ev[-1]
    if name == "floating":
        mech = m.mechanism
        quats = [e.q_offset for e in mech.edges[1:] if e.joint.kind == "quaternion_floating"]
        assert len(quats) == 2
        for o in quats:
            v = np.zeros(len(x))
            v[o:o + 4] = x[o:o + 4] / np.linalg.norm(x[o:o + 4])
            assert np.linalg.norm(A @ v) <= 1e-12 * np.linalg.norm(A), np.linalg.norm(A @ v) / np.linalg.norm(A)


def test_matrix_matches_finite_differences(irb, oracle_mod):
    """A from the oracle's per-point ∇d* and k* against Σ J_fdᵀ J_fd with J_fd
    the central differences (h = 1e-6) of the oracle's d*(p) in each joint.
    Points whose k* differs at q ± h are left out (at most 1 %)."""
    from flash import synthetic
    m = irb
    q_true, q = synthetic.perturbed_configuration(m, 41)
    pts = synthetic.depth_cloud(m, q_true, 1000, seed=42)
    oc = OracleCost(m, pts)
    d0, k0, g0 = oc.per_point(q)
    h = 1e-6
    nq = len(q)
    J = np.empty((len(pts), nq))
    keep = np.ones(len(pts), bool)
    for i in range(nq):
        e = np.zeros(nq)
        e[i] = h
        dp, kp, _ = oc.per_point(q + e)
        dm, km, _ = oc.per_point(q - e)
        keep &= (kp == k0) & (km == k0)
        J[:, i] = (dp - dm) / (2 * h)
    left_out = int((~keep).sum())
    assert left_out <= 0.01 * len(pts), left_out
    A_fd = J[keep].T @ J[keep]
    mom = moments_numpy(pts[keep], g0[keep], k0[keep], len(oc.sb))
    for A in (m.mechanism.gauss_newton_matrix(q, oc.sb, mom), m.mechanism.gauss_newton_matrix_numpy(q, oc.sb, mom)):
        err = np.linalg.norm(A - A_fd) / np.linalg.norm(A_fd)
        print(f"finite differences: {left_out} points left out, relative error {err:.3e}")
        assert err <= 1e-6, err


# ---- fsdf_lm_step ----------------------------------------------------------------
def _spd(n, seed):
    r = np.random.default_rng(seed)
    B = r.normal(size=(n, n + 3))
    return B @ B.T, r.normal(size=n)


@pytest.mark.parametrize("n,lam", [(1, 0.0), (6, 1e-3), (20, 10.0), (48, 1e-6)])
def test_lm_step_matches_numpy_solve(n, lam):
    from flash._lib import lm_step
    H, g = _spd(n, n)
    D = np.maximum(np.diag(H), 1e-12 * np.diag(H).max())
    ref = -np.linalg.solve(H + lam * np.diag(D), g)
    st, dx = lm_step(H, g, lam, 1e30)
    assert st == 0
    assert np.linalg.norm(dx - ref) <= 1e-10 * np.linalg.norm(ref)
    # the clamp, component-wise
    cap = 0.5 * np.abs(ref).max()
    st, dc = lm_step(H, g, lam, cap)
    assert st == 0 and np.array_equal(dc, np.clip(dx, -cap, cap))
    if n > 1:
        assert (np.abs(dx) > cap).any() and (np.abs(dc) == cap).any()


def test_lm_step_degenerate():
    from flash._lib import lm_step
    H, g = _spd(5, 3)
    Hi = H.copy()
    Hi[2, 2] = -Hi[2, 2] - 1.0  # indefinite
    assert lm_step(Hi, g, 1e-3, 0.5) == (5, None)
    Hn = H.copy()
    Hn[3, 1] = Hn[1, 3] = np.nan
    assert lm_step(Hn, g, 1e-3, 0.5) == (5, None)
    Hn = H.copy()
    Hn[4, 4] = np.nan
    assert lm_step(Hn, g, 1e-3, 0.5) == (5, None)
    assert lm_step(np.zeros((3, 3)), np.zeros(3), 1.0, 0.5) == (5, None)


def test_lm_step_zero_row_gives_zero_step():
    """A coordinate the cost does not see (zero row and column, zero gradient
    entry): the floor on D keeps the factorisation going and its step is 0."""
    from flash._lib import lm_step
    H, g = _spd(6, 9)
    H[2, :] = H[:, 2] = 0.0
    g[2] = 0.0
    st, dx = lm_step(H, g, 1e-3, 1e30)
    assert st == 0 and dx[2] == 0.0
    keep = np.arange(6) != 2
    Hk = H[np.ix_(keep, keep)]
    ref = -np.linalg.solve(Hk + 1e-3 * np.diag(np.diag(Hk)), g[keep])
    assert np.linalg.norm(dx[keep] - ref) <= 1e-10 * np.linalg.norm(ref)


# ---- convergence over the oracle ---------------------------------------------------
def test_lm_converges_on_oracle(oracle_mod):
    """Within 6 evaluations LM reaches f <= 1.01 f(q_true) and f <= NaiveSolver's
    f after 30 (rate 0.1, max_step 0.5, tolerance 0)."""
    from flash.tracking import LevenbergMarquardt, NaiveSolver
    m, pts, q_true, q0 = convergence_case()
    oc = OracleCost(m, pts)
    n = float(len(pts))
    f_true = oc.value_and_gradient(q_true)[0] / n

    lm_f = []

    def vgh(x):
        c, g, H = oc(x)
        lm_f.append(c / n)
        return c / n, g / n, H / n

    solver = LevenbergMarquardt(len(q0), iteration_limit=6, gradient_convergence_tolerance=0.0)
    _, f_lm = solver.optimize(vgh, q0)
    assert solver.iterations <= 6 and f_lm == min(lm_f)

    naive_f = []

    def vg(x):
        c, g, _ = oc.value_and_gradient(x)
        naive_f.append(c / n)
        return c / n, g / n

    NaiveSolver(len(q0), rate=0.1, max_step=0.5, iteration_limit=30, gradient_convergence_tolerance=0.0).optimize(vg, q0)
    assert len(naive_f) == 30
    print(f"LM f by evaluation {['%.4e' % v for v in lm_f]}; f(q_true) {f_true:.4e}; naive after 30 {naive_f[-1]:.4e}")
    assert f_lm <= 1.01 * f_true, (f_lm, f_true)
    assert f_lm <= naive_f[-1], (f_lm, naive_f[-1])


def test_estimate_state_refuses_levenberg_marquardt_for_now():
    """The tracking entry points have no Gauss-Newton Hessian to hand the solver
    yet: they say so instead of running it on a two-value objective."""
    import types
    import flash
    from flash.tracking import LevenbergMarquardt, _optimize
    assert flash.LevenbergMarquardt is LevenbergMarquardt
    with pytest.raises(NotImplementedError):
        _optimize(types.SimpleNamespace(_native=False), 10, np.zeros(6), None, LevenbergMarquardt(6))
