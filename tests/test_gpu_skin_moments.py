"""GPU: the second moments of RBF skins on the device (csrc/skin_moments.hip,
fsdf_eval_skin_moments) against Σ j jᵀ of the numpy twin (flash/rbf.py
skin_jacobian), and the second-order solver on scenes with skins and
deformations behind fsdf_set_lm_skins: fsdf_value_gradient_hessian against the
twin Gauss-Newton Hessian, fsdf_descend_lm against the Python loop bit for bit,
estimate_state end to end.

Tolerance of the moments and of H: max(1e-9, 100 ε) relative to the largest
entry, ε the twin's own float64-versus-np.longdouble disagreement on the same
inputs (at most 1,000 points), printed by each test."""
import numpy as np
import pytest

from test_gpu_solver_rbf import _build, _scene, _sphere_skin

pytestmark = pytest.mark.gpu

# 1, around one 64-point chunk, 549 = one workgroup's run of 8 chunks and a second workgroup, 4000 = 8 workgroups
COUNTS = (1, 63, 64, 65, 549, 4000)


def _ctx(m, precision=64):
    from flash import _lib
    from flash.core import ConvexGeometry
    c = _lib.Context(device=0, precision=precision)
    c.set_surfaces([("hull", (s.hull.vertices, s.hull.faces, s.hull.planes)) if isinstance(s, ConvexGeometry)
                    else ("rbf", len(s.surface_points) + len(s.skeleton_points)) for s in m.surfaces])
    return c


def _posed(m, x):
    """(poses, solves, rows) of the scene at x."""
    from flash import rbf
    from flash.core import surface_poses
    nq = m.mechanism.num_positions
    qn = m.mechanism.normalize(x[:nq])
    solves = rbf.solve(m, qn, x[nq:])
    return surface_poses(m, qn), solves, rbf.rows(solves)


def _twin_moment(C, u, pts):
    """(Σ j jᵀ in float64, ε: its disagreement with np.longdouble on at most 1,000 of the points)."""
    from flash import rbf
    J = rbf.skin_jacobian(C, u, pts)
    M = J.T @ J
    sub = pts[:1000]
    if len(sub) == 0:
        return M, 0.0
    J64 = J[:len(sub)]
    Jl = rbf.skin_jacobian(C, u, sub, dtype=np.longdouble)
    Ml = Jl.T @ Jl
    eps = float(np.abs(J64.T @ J64 - Ml).max() / np.abs(Ml).max())
    return M, eps


def _box_cloud(solves, n, seed):
    C = np.concatenate([r.centres for r in solves])
    r = np.random.default_rng(seed)
    lo, hi = C.min(0) - 0.3, C.max(0) + 0.3
    return lo + (hi - lo) * r.random((n, 3))


def _scene_at(name):
    if name.startswith("sphere"):  # (sphereN: N centres, the skeleton point among them)
        return _sphere_skin(int(name[6:]) - 1), np.array([0.2])
    return _build(name)


@pytest.mark.parametrize("name,precision,m_rows", [
    ("beanbag", 64, (32,)), ("beanbag", 32, (32,)),  # under one block
    ("squishable", 64, (56,)),
    ("two_link_arm", 64, (188,)),                     # three blocks, the last partial
    ("sphere71", 64, (288,)),
    ("sphere124", 64, (500,)),                        # the limit n + 4 = 128
    ("irb_and_squishable", 64, (56,)),                # hull points masked
    ("two_link_arm+beanbag", 64, (188, 32)),          # two skins
])
def test_skin_moments_match_the_twin(name, precision, m_rows):
    from flash import synthetic
    m, x = _scene_at(name)
    poses, solves, rows = _posed(m, x)
    assert tuple(4 * r.n + 4 for r in solves) == m_rows
    c = _ctx(m, precision)
    c.set_rbf_params(rows)
    if precision == 32:  # (the context works on its fp32 points and rows, widened)
        rows = rows.astype(np.float32).astype(np.float64)
    big = synthetic.skin_cloud(m, x, max(COUNTS), seed=11) if name == "irb_and_squishable" else \
        _box_cloud(solves, max(COUNTS), 11)
    for n in COUNTS:
        pts = big[:n]
        c.set_points(pts)
        cost, acc, Ms = c.eval_skin_moments(poses)
        cost2, acc2, Ms2 = c.eval_skin_moments(poses)
        _, acc_e, (k, _, _) = c.eval(poses, per_point=True)
        assert cost == cost2 and np.array_equal(acc, acc2) and np.array_equal(acc, acc_e)
        if precision == 32:
            pts = pts.astype(np.float32).astype(np.float64)
        if name == "irb_and_squishable" and n == max(COUNTS):
            assert (k == solves[0].surface).any() and (k != solves[0].surface).any()
        row0 = 0
        for r, M, M2 in zip(solves, Ms, Ms2):
            C, u = rows[row0:row0 + r.n, :3], np.concatenate([rows[row0:row0 + r.n, 3], rows[row0 + r.n]])
            row0 += r.n + 1
            want, eps = _twin_moment(C, u, pts[k == r.surface])
            assert M.shape == want.shape
            assert np.array_equal(M, M.T)
            assert np.array_equal(M, M2)  # two runs, the same bits
            if not (k == r.surface).any():
                assert not M.any()
                continue
            scale = np.abs(want).max()
            tol = max(1e-9, 100.0 * eps)
            err = np.abs(M - want).max() / scale
            print(f"{name} f{precision} n={n} m={len(M)}: err {err:.3e}, eps {eps:.3e}, tol {tol:.3e}")
            assert err <= tol, (n, err, tol)
    c.close()


def test_skin_of_125_centres_is_refused():
    from flash._lib import FlashNativeError
    m, x = _scene_at("sphere125")
    poses, solves, rows = _posed(m, x)
    c = _ctx(m)
    c.set_rbf_params(rows)
    c.set_points(_box_cloud(solves, 100, 1))
    c.eval(poses)  # (the pass itself serves the skin)
    with pytest.raises(FlashNativeError) as e:
        c.eval_skin_moments(poses)
    assert e.value.status == 3
    c.close()


def test_no_point_on_the_skin_and_no_point_at_all():
    """Points on the robot's hulls, none nearest to the skin: exact zeros; so
    does an empty cloud. A scene without a skin is refused."""
    from flash import Models, synthetic
    from flash._lib import FlashNativeError
    m, x = _build("irb_and_squishable")
    poses, solves, rows = _posed(m, x)
    c = _ctx(m)
    c.set_rbf_params(rows)
    verts = np.concatenate([v for v, _ in synthetic.world_hulls(m, x[:m.mechanism.num_positions])[:3]])
    c.set_points(verts)
    _, _, (k, _, _) = c.eval(poses, per_point=True)
    assert (k != solves[0].surface).all()
    _, _, Ms = c.eval_skin_moments(poses)
    assert len(Ms) == 1 and Ms[0].shape == (56, 56) and not Ms[0].any()
    c.set_points(np.zeros((0, 3)))
    cost, _, Ms = c.eval_skin_moments(poses)
    assert cost == 0.0 and not Ms[0].any()
    c.close()
    irb = Models.irb140()
    c = _ctx(irb)
    c.set_points(np.zeros((4, 3)))
    with pytest.raises(FlashNativeError) as e:
        c.eval_skin_moments(np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (len(irb.surfaces), 1)))
    assert e.value.status == 3
    c.close()


@pytest.mark.parametrize("name", ["squishable", "irb_and_squishable", "two_link_arm+beanbag"])
def test_value_gradient_hessian_with_the_switch(name):
    from flash import rbf
    from flash._lib import FlashNativeError
    from flash.core import ConvexGeometry
    from flash.gradientdescent import CostFunctor
    from gn_helpers import moments_numpy
    m, pts, x0 = _scene(name)
    cf = CostFunctor(m, pts, skin_hessian=True)
    c, g, H = cf.value_gradient_hessian(x0)
    c2, g2 = cf.value_and_gradient(x0)
    assert c == c2 and np.array_equal(g, g2)
    nx, nq = len(x0), m.mechanism.num_positions
    assert H.shape == (nx, nx) and np.array_equal(H, H.T)
    assert (np.diag(H)[nq:] >= 2.0 * cf.weight).all()
    # the twin: Σ j jᵀ per skin over the device's k*, the hulls' moments from the device's ∇d*
    k, d, grad = cf.per_point(x0)
    _, solves, _ = _posed(m, x0)
    Ms, eps = [], 0.0
    for r in solves:
        M, e = _twin_moment(r.centres, r.u, pts[k == r.surface])
        Ms.append(M)
        eps = max(eps, e)
    hull = moments_numpy(pts, grad, k, len(m.surfaces))
    for s, surf in enumerate(m.surfaces):
        if not isinstance(surf, ConvexGeometry):
            hull[s] = 0.0
    want = rbf.gauss_newton(m, x0, solves, Ms, hull, cf.weight)
    err = np.abs(H - want).max() / np.abs(want).max()
    tol = max(1e-9, 100.0 * eps)
    print(f"{name}: H err {err:.3e}, eps {eps:.3e}, tol {tol:.3e}")
    assert err <= tol, (err, tol)
    # the switch off, on a fresh context: today's refusal
    cf2 = CostFunctor(_build(name)[0], pts[:200])
    with pytest.raises(FlashNativeError) as e:
        cf2.ctx.value_gradient_hessian(x0)
    assert e.value.status == 3
    with pytest.raises(FlashNativeError) as e:
        cf2.ctx.descend_lm(x0, 2, 1e-3, 0.5, 0.0, 200.0)
    assert e.value.status == 3
    cf.set_skin_hessian(False)  # (the scene's engine is shared with other tests: as it was)


@pytest.mark.parametrize("name", ["squishable", "irb_and_squishable"])
@pytest.mark.parametrize("prior", [None, 1e-3])
def test_descend_lm_equals_the_python_loop(name, prior):
    from flash._lib import FlashNativeError
    from flash.gradientdescent import CostFunctor
    from flash.tracking import LevenbergMarquardt, state_prior
    m, pts, x0 = _scene(name)
    cf = CostFunctor(m, pts, skin_hessian=True)
    n = float(len(pts))
    limit = 8
    got = cf.descend_lm(x0, limit, 1e-3, 0.5, 1e-6, n, prior_weight=prior)

    def wrapped(x):
        c, g, H = cf.ctx.value_gradient_hessian(x)
        return c / n, g / n, H / n

    solver = LevenbergMarquardt(len(x0), iteration_limit=limit, skins=True)
    x, f = solver.optimize(state_prior(wrapped, x0, prior), x0)
    assert got[2] == solver.iterations and got[3] == solver.final_damping
    assert got[1] == f and np.array_equal(got[0], x)
    assert got[2] > 1 and f < wrapped(x0)[0]
    # mode 1 takes the host loop: the same bits; mode 2 refuses the scene
    same = cf.descend_lm(x0, limit, 1e-3, 0.5, 1e-6, n, prior_weight=prior, device_loop=True)
    assert same[1:] == got[1:] and np.array_equal(same[0], got[0])
    with pytest.raises(FlashNativeError) as e:
        cf.descend_lm(x0, limit, 1e-3, 0.5, 1e-6, n, prior_weight=prior, device_loop="require")
    assert e.value.status == 3
    if prior is not None:  # a prior of nq weights no longer fits the nx coordinates
        with pytest.raises(FlashNativeError) as e:
            cf.descend_lm(x0, limit, 1e-3, 0.5, 1e-6, n, prior_weight=np.full(m.mechanism.num_positions, prior))
        assert e.value.status == 3
    cf.set_skin_hessian(False)  # (the scene's engine is shared with other tests: as it was)


def test_estimate_state_squishable_end_to_end():
    import flash
    from flash.gradientdescent import CostFunctor
    from flash.tracking import LevenbergMarquardt, estimate_state
    m, pts, x0 = _scene("squishable")
    with pytest.raises(NotImplementedError):  # the default solver settings refuse the scene as before
        estimate_state(m, pts, x0, solver=LevenbergMarquardt(len(x0)))
    solver = LevenbergMarquardt(len(x0), skins=True)
    x_lm = estimate_state(m, pts, x0, solver=solver)
    x_naive = estimate_state(m, pts, x0)
    cf = CostFunctor(m, pts)
    c_lm, c_naive, c0 = cf(x_lm), cf(x_naive), cf(x0)
    print(f"squishable, 4000 points: cost at start {c0:.6e}, LevenbergMarquardt(skins) {c_lm:.6e} after "
          f"{solver.iterations} evaluations, default solver {c_naive:.6e}")
    m.engine().set_lm_skins(False)  # (estimate_state's cost turned it on: the shared engine as it was)
    assert flash.num_states(m) == len(x_lm)
    assert c_lm <= c_naive, (c_lm, c_naive)
