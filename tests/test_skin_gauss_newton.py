"""CPU: the Gauss-Newton matrix of scenes with RBF skins and deformations, host
side (no GPU): the per-point rows of a skin (flash/rbf.py skin_jacobian) against
central differences of the oracle skin and against the oracle's accumulator
block, the map to state space (state_map) against the gradient's own chain and
against central differences through the weight solve, the native
fsdf_rbf_state_map / fsdf_gauss_newton_add against those twins, and
Levenberg-Marquardt over the twin objective on the deformable squishable.

A skin point's row j(p) has m = 4n + 4 entries in the layout of the skin's
accumulator block (∂s/∂w [n], ∂s/∂a, ∂s/∂b [3], ∂s/∂c [n][3], coefficients
fixed for the last); the block is Σ 2 s j, the skin's second moment Σ j jᵀ,
∂s/∂x = L j and H = 2 (A_hulls + Σ_r L_r M_r L_rᵀ) + 2 weight I on δ
(include/flashsdf.h "Gauss-Newton for RBF skins")."""
import numpy as np
import pytest

H_FD = 1e-5


def _build(name):
    """(manipulator, x): x off the zero configuration in every entry — bodies
    moved, quaternions not normalised, non-zero deformations."""
    import flash
    from flash import Models
    if name == "two_link_arm+beanbag":
        bag = Models.beanbag()
        bag.mechanism.body_names[1] = "beanbag_body"  # (the arm has a "body1" of its own)
        m = Models.merge(Models.two_link_arm(), bag)
    else:
        m = getattr(Models, name)()
    nq = m.mechanism.num_positions
    r = np.random.default_rng(5)
    x = np.zeros(flash.num_states(m))
    x[:nq] = m.mechanism.zero_configuration() + 0.05 * r.normal(size=nq)
    x[nq:] = 0.02 * r.normal(size=len(x) - nq)
    for e in m.mechanism.edges[1:]:
        if e.joint.kind == "quaternion_floating":
            x[e.q_offset:e.q_offset + 4] *= 1.2
    return m, x


def _solves(m, x):
    from flash import rbf
    nq = m.mechanism.num_positions
    return rbf.solve(m, m.mechanism.normalize(x[:nq]), x[nq:])


def _cloud(centres, n, seed):
    """Random points in the centres' box padded by 0.3."""
    r = np.random.default_rng(seed)
    lo, hi = centres.min(0) - 0.3, centres.max(0) + 0.3
    return lo + (hi - lo) * r.random((n, 3))


def _fd_check(got, fd1, fd2, what):
    """Central differences at h and 2h calibrate the tolerance: 10 x their
    disagreement elementwise, plus 1e-9 max|got|."""
    tol = 10.0 * np.abs(fd1 - fd2) + 1e-9 * np.abs(got).max()
    bad = np.abs(got - fd1) > tol
    assert not bad.any(), (what, int(bad.sum()), float(np.abs(got - fd1).max()), float(tol.min()))


@pytest.mark.parametrize("name", ["beanbag", "squishable", "two_link_arm"])
def test_skin_jacobian_against_central_differences(name, oracle_mod):
    import rbf as orbf  # oracle/rbf.py (numpy restatement)
    from flash import rbf
    m, x = _build(name)
    r = _solves(m, x)[0]
    C, u, n = r.centres, r.u, r.n
    pts = _cloud(C, 50, 3)
    J = rbf.skin_jacobian(C, u, pts)
    assert J.shape == (50, 4 * n + 4)

    def fd(h):
        out = np.empty_like(J)
        for k in range(n + 4):  # in u = (w, a, b)
            e = np.zeros(n + 4)
            e[k] = h
            out[:, k] = (orbf.skin(C, u + e, pts)[0] - orbf.skin(C, u - e, pts)[0]) / (2 * h)
        for k in range(3 * n):  # in the centres, u fixed
            e = np.zeros(3 * n)
            e[k] = h
            e = e.reshape(n, 3)
            out[:, n + 4 + k] = (orbf.skin(C + e, u, pts)[0] - orbf.skin(C - e, u, pts)[0]) / (2 * h)
        return out

    _fd_check(J, fd(H_FD), fd(2 * H_FD), name)
    # Σ 2 s j is the skin's block of the oracle's accumulator (tests/test_gpu_rbf.py's tolerance for the same sums)
    import flash
    om = oracle_mod.OracleModel.from_manipulator(m)
    nq = m.mechanism.num_positions
    poses = flash.core.surface_poses(m, m.mechanism.normalize(x[:nq]))
    acc = om.cost_accum(poses, pts, rbf.rows([r]))
    s = orbf.skin(C, u, pts)[0]
    block = (2.0 * s[:, None] * J).sum(0)
    want = acc[1 + 6 * len(m.surfaces):]
    assert np.allclose(block, want, rtol=1e-9, atol=1e-9 * np.abs(want).max()), np.abs(block - want).max()


def _gradient_of_block(m, x, solve_r, block):
    """chain + config_gradient on one skin's block: the gradient's own code."""
    from flash import rbf
    mech = m.mechanism
    nq = mech.num_positions
    nd = m.num_deformations()
    wrench, gdef = rbf.chain(m, mech.normalize(x[:nq]), [solve_r], block, nd)
    return np.concatenate([mech.config_gradient(x[:nq], wrench), gdef])


@pytest.mark.parametrize("name", ["beanbag", "two_link_arm", "two_link_arm+beanbag"])
def test_state_map(name, oracle_mod):
    """L j(p) against central differences of s(p; x) through centres -> fit ->
    skin, and L @ block against chain + config_gradient on that block to 1e-12
    relative. The second check needs chain's adjoint arithmetic in
    np.longdouble: two_link_arm's 46-centre skin (cond(M) = 7.7e4) has centre
    forces of norm 7.8e4 cancelling into a wrench of 15, which in float64 left
    1.7e-12 between the two sides; it is 2.2e-15 now (beanbag 1.5e-16)."""
    import rbf as orbf  # oracle/rbf.py
    from flash import rbf
    from flash.core import InterpolatingGeometry
    m, x = _build(name)
    nq = m.mechanism.num_positions
    solves = _solves(m, x)
    skins = [s for s in m.surfaces if isinstance(s, InterpolatingGeometry)]
    assert len(solves) == len(skins) == (2 if "+" in name else 1)
    rg = np.random.default_rng(9)
    rel = []
    for r, surf in zip(solves, skins):
        L = rbf.state_map(m, x, r)
        assert L.shape == (len(x), 4 * r.n + 4)
        block = rg.normal(size=4 * r.n + 4)
        want = _gradient_of_block(m, x, r, block)
        rel.append(np.linalg.norm(L @ block - want) / np.linalg.norm(want))
        print(f"{name} surface {r.surface}: |L block - gradient| / |gradient| = {rel[-1]:.3e}")
        # ∂s(p; x)/∂x = L j(p), against central differences through centres -> fit -> skin
        pts = _cloud(r.centres, 12, 4)
        got = rbf.skin_jacobian(r.centres, r.u, pts) @ L.T  # [N, nx]

        def s_of(xx):
            C, v = orbf.surface_centres(m, xx[:nq], xx[nq:], surf)
            return orbf.skin(C, orbf.fit(C, v)[0], pts)[0]

        def fd(h):
            out = np.empty_like(got)
            for k in range(len(x)):
                e = np.zeros(len(x))
                e[k] = h
                out[:, k] = (s_of(x + e) - s_of(x - e)) / (2 * h)
            return out

        _fd_check(got, fd(H_FD), fd(2 * H_FD), (name, r.surface))
    assert max(rel) <= 1e-12, rel


def _native_state_map(lib, m, x, r):
    """fsdf_rbf_state_map on the FK of the caller's x and fsdf_rbf_solve's factors."""
    mech = m.mechanism
    nq, nb, nd = mech.num_positions, mech.num_bodies, m.num_deformations()
    P = mech._kinematic_plan()
    q = np.ascontiguousarray(x[:nq], np.float64)
    R, t, Rb, tb = (np.ascontiguousarray(a) for a in mech.body_transform_arrays(q))
    n = r.n
    surf = m.surfaces[r.surface]
    C = np.ascontiguousarray(r.centres, np.float64)
    v = np.concatenate([np.zeros(len(surf.surface_points)), -np.ones(len(surf.skeleton_points))])
    u, lu, piv = np.empty(n + 4), np.empty((n + 4) ** 2), np.empty(n + 4, np.int32)
    assert lib.fsdf_rbf_solve(n, C.ctypes.data, v.ctypes.data, u.ctypes.data, lu.ctypes.data, piv.ctypes.data) == 0
    body = np.ascontiguousarray(r.bodies, np.int32)
    drow = np.ascontiguousarray(r.deform_rows, np.int32)
    nx = nq + 3 * nd
    work = np.empty(8 * n + 8 + 12 * nb + nx)
    L = np.empty((nx, 4 * n + 4))
    nat = P["native_ptrs"]
    args = [nb, nat[0], nat[1], nat[2], nat[3], R.ctypes.data, Rb.ctypes.data, tb.ctypes.data, q.ctypes.data, nq, n,
            C.ctypes.data, u.ctypes.data, lu.ctypes.data, piv.ctypes.data, body.ctypes.data, drow.ctypes.data, nd,
            work.ctypes.data, L.ctypes.data]
    keep = (R, Rb, tb, q, C, u, lu, piv, body, drow, work)
    return L, args, keep


@pytest.mark.parametrize("name", ["beanbag", "squishable", "two_link_arm", "two_link_arm+beanbag"])
def test_native_state_map_and_add_match_the_twins(name):
    from flash import _lib, rbf
    lib = _lib.load()
    m, x = _build(name)
    nx = len(x)
    A = np.zeros((nx, nx))
    A_twin = np.zeros((nx, nx))
    for r in _solves(m, x):
        L, args, _keep = _native_state_map(lib, m, x, r)
        assert lib.fsdf_rbf_state_map(*args) == 0
        T = rbf.state_map(m, x, r)
        scale = np.abs(T).max()
        assert scale > 0
        assert np.allclose(L, T, rtol=1e-9, atol=1e-9 * scale), np.abs(L - T).max() / scale
        mm = 4 * r.n + 4
        J = rbf.skin_jacobian(r.centres, r.u, _cloud(r.centres, 300, 6))
        M = np.ascontiguousarray(J.T @ J)
        work = np.empty(nx * mm)
        assert lib.fsdf_gauss_newton_add(nx, mm, L.ctypes.data, M.ctypes.data, work.ctypes.data, A.ctypes.data) == 0
        A_twin += T @ M @ T.T
    scale = np.abs(A_twin).max()
    assert np.allclose(A, A_twin, rtol=1e-9, atol=1e-9 * scale), np.abs(A - A_twin).max() / scale
    assert np.array_equal(A, A.T)
    ev = np.linalg.eigvalsh(A)
    assert ev[-1] > 0 and ev[0] >= -1e-9 * ev[-1], ev[0] / ev[-1]


def test_native_bad_arguments():
    from flash import _lib
    lib = _lib.load()
    m, x = _build("beanbag")
    r = _solves(m, x)[0]
    L, args, _keep = _native_state_map(lib, m, x, r)
    assert lib.fsdf_rbf_state_map(*args) == 0
    for i, bad in ((0, 0), (10, 0), (5, None), (11, None), (19, None), (17, -1)):
        a = list(args)
        a[i] = bad
        assert _lib.STATUS_NAMES[lib.fsdf_rbf_state_map(*a)] == "FSDF_ERR_ARG", i
    a = list(args)
    rows = np.full(r.n, 99, np.int32)  # a deformation row beyond n_deform
    a[16] = rows.ctypes.data
    assert _lib.STATUS_NAMES[lib.fsdf_rbf_state_map(*a)] == "FSDF_ERR_ARG"
    nx, mm = L.shape
    M, work, A = np.eye(mm), np.empty(nx * mm), np.zeros((nx, nx))
    ok = [nx, mm, L.ctypes.data, M.ctypes.data, work.ctypes.data, A.ctypes.data]
    assert lib.fsdf_gauss_newton_add(*ok) == 0
    for i, bad in ((0, -1), (1, -1), (2, None), (3, None), (4, None), (5, None)):
        a = list(ok)
        a[i] = bad
        assert _lib.STATUS_NAMES[lib.fsdf_gauss_newton_add(*a)] == "FSDF_ERR_ARG", i


class TwinCost:
    """x -> (c, ∂c/∂x, H) of a one-skin scene: the oracle skin's cost, the
    gradient L Σ 2 s j + 2 w δ and the twin Gauss-Newton Hessian."""

    def __init__(self, m, pts, weight=10.0):
        self.m, self.pts, self.weight = m, np.ascontiguousarray(pts, np.float64), weight
        self.nq = m.mechanism.num_positions

    def __call__(self, x):
        import rbf as orbf  # oracle/rbf.py
        from flash import rbf
        x = np.asarray(x, np.float64)
        r = _solves(self.m, x)[0]
        s = orbf.skin(r.centres, r.u, self.pts)[0]
        J = rbf.skin_jacobian(r.centres, r.u, self.pts)
        delta = x[self.nq:]
        c = float(s @ s) + self.weight * float(delta @ delta)
        g = rbf.state_map(self.m, x, r) @ (2.0 * s @ J)
        g[self.nq:] += 2.0 * self.weight * delta
        return c, g, rbf.gauss_newton(self.m, x, [r], [J.T @ J], None, self.weight)


def test_lm_on_the_twin_objective_squishable(oracle_mod):
    """Within 30 evaluations LevenbergMarquardt ends at or below
    NaiveSolver(rate 0.1, max_step 0.5) after 30, from the same start."""
    import flash
    import rbf as orbf  # oracle/rbf.py
    from flash import Models
    from flash.tracking import LevenbergMarquardt, NaiveSolver
    m = Models.squishable()
    nq = m.mechanism.num_positions
    x_true = np.zeros(flash.num_states(m))
    x_true[:nq] = m.mechanism.zero_configuration()
    r = _solves(m, x_true)[0]
    pts = _cloud(r.centres, 2000, 21)
    for _ in range(30):  # Newton projection onto the zero set of the oracle skin
        s, gs = orbf.skin(r.centres, r.u, pts)
        step = -(s / (gs * gs).sum(1))[:, None] * gs
        nrm = np.linalg.norm(step, axis=1, keepdims=True)
        pts = pts + step * np.minimum(1.0, 0.2 / np.maximum(nrm, 1e-300))
    print(f"cloud: max |s| at x_true {np.abs(orbf.skin(r.centres, r.u, pts)[0]).max():.3e}")
    x0 = x_true + np.random.default_rng(12).normal(0.0, 0.03, len(x_true))
    cost = TwinCost(m, pts)
    n = float(len(pts))
    lm_f, naive_f = [], []

    def vgh(x):
        c, g, H = cost(x)
        lm_f.append(c / n)
        return c / n, g / n, H / n

    def vg(x):
        c, g, _ = cost(x)
        naive_f.append(c / n)
        return c / n, g / n

    solver = LevenbergMarquardt(len(x0), iteration_limit=30, gradient_convergence_tolerance=0.0)
    _, f_lm = solver.optimize(vgh, x0)
    NaiveSolver(len(x0), rate=0.1, max_step=0.5, iteration_limit=30,
                gradient_convergence_tolerance=0.0).optimize(vg, x0)
    print("LM f by evaluation", ["%.4e" % v for v in lm_f])
    print("naive f by iteration", ["%.4e" % v for v in naive_f])
    assert solver.iterations <= 30 and len(naive_f) == 30
    assert f_lm == min(lm_f)
    assert f_lm <= naive_f[-1], (f_lm, naive_f[-1])
