"""CPU: tests/skin_ref.py against itself (its complex-step gradient against
central differences of its own cost, its fit against the values at the centres,
the reference project's one numeric test), and the native host pieces of the
RBF chain that have CPU entry points — fsdf_rbf_solve, fsdf_rbf_adjoint,
fsdf_tree_transforms and fsdf_config_gradient (csrc/rbf_host.cpp,
csrc/kinematics.cpp; rbf_host.cpp instantiates csrc/rbf_impl.h, which the device
solver step shares) — against it on every shape of skin_ref.SHAPES.

Every comparison with the reference is held to max(1e-9, 100 · precision_gap)
of the largest entry (tests/test_gpu_skin_moments.py's convention);
precision_gap is the reference's own disagreement between complex128 and
clongdouble. The sums between fsdf_rbf_adjoint and fsdf_config_gradient (centre
forces to body wrenches, Rᵀ G per deformation row) run inside fsdf_* calls that
need a context; here they are restated in numpy from iterate.hip's
iteration_finish, so this file checks the native solve, adjoint, kinematics and
chain rule, and a numpy twin of the sums between them. The device's own sums
are held to the same reference by tests/test_gpu_solver_rbf_shapes.py."""
import numpy as np
import pytest

import skin_ref

SHAPES = list(skin_ref.SHAPES) + [f"sphere{skin_ref.MMAX_N}"]
# The central differences' step: a difference quotient of c carries ε c / h of rounding, and the rule's
# floor is 1e-9 max|g|; on the one-coordinate spheres c = 37 and max|g| = 0.7 near their optimum, so h
# must exceed 2.2e-16 · 37 / 7e-10 = 1.2e-5 — 1e-4 leaves a factor of 8, and its truncation error is what the
# rule's other term, the disagreement of h and 2h, measures.
H_FD = 1e-4


def test_kat_beanbag():
    """The reference project's only numeric test of a skin: beanbag at its
    default state, s(100, 0, 0) ≈ 99 at rtol 2e-2 (oracle/rbf.py's header)."""
    import flash
    from flash import Models
    m = Models.beanbag()
    x = np.zeros(flash.num_states(m))
    x[:7] = m.mechanism.zero_configuration()
    obj = skin_ref.SkinObjective(m, np.array([[100.0, 0.0, 0.0]]))
    (C, u), = obj.fits(x, np.clongdouble)
    s = float(skin_ref.field_ref(C[None], u[None], obj.pts)[0, 0].real)
    print(f"beanbag s(100, 0, 0) = {s:.6f}")
    assert abs(s - 99.0) <= 2e-2 * 99.0
    assert abs(s - 98.893) < 1e-3  # (the figure oracle/rbf.py's header records)


@pytest.mark.parametrize("shape", SHAPES)
def test_shape_is_what_its_name_says(shape):
    """System sizes, a start off the zero state in every entry the shape
    allows, quaternion norms in 0.9 .. 1.1, non-zero δ; scene() itself asserts
    that at most 0.1 % of the cloud was dropped as tied."""
    m, pts, x0 = skin_ref.scene(shape)
    sizes = tuple(len(s[1]) + 4 for s in skin_ref.skins_of(m))
    assert sizes == skin_ref.SHAPES.get(shape, (skin_ref.MMAX_N + 4,))
    assert 0.999 * skin_ref.POINTS <= len(pts) <= skin_ref.POINTS
    mech = m.mechanism
    for e in mech.edges[1:]:
        if e.joint.kind == "quaternion_floating":
            assert 0.9 <= np.linalg.norm(x0[e.q_offset:e.q_offset + 4]) <= 1.1
        elif e.joint.kind == "revolute":
            assert (x0[e.q_offset] == 0.0) == shape.startswith("lattice")
    assert np.all(x0[mech.num_positions:] != 0.0)
    assert (x0.size > mech.num_positions) == (m.num_deformations() > 0)


@pytest.mark.parametrize("shape", SHAPES)
def test_fit_reproduces_the_values(shape):
    """M u = (v, 0) in clongdouble: the field takes the centres' values and the
    weights are orthogonal to the polynomials, to 1e-13."""
    obj, x0 = skin_ref.objective(shape), skin_ref.scene(shape)[2]
    for (_, _, _, _, values), (C, u) in zip(obj.skins, obj.fits(x0, np.clongdouble)):
        res = np.sum(skin_ref.system_ref(C) * u[None, :], axis=1) - np.concatenate([values, np.zeros(4)])
        assert float(np.abs(res).max()) <= 1e-13, float(np.abs(res).max())


@pytest.mark.parametrize("shape", SHAPES)
def test_gradient_against_central_differences(shape):
    """The complex-step gradient against central differences of the
    reference's own c(x) at h and 2h, k* held at x0's: within 10 x their
    disagreement plus 1e-9 max|g| (tests/test_skin_gauss_newton.py's rule).
    Points inside a hull are left out: there d* is the largest plane value,
    which has a kink wherever two faces tie, and a single point within h of one
    puts an error of 2 d* Δn / 2 into the difference quotient at any h."""
    obj, x0 = skin_ref.objective(shape), np.array(skin_ref.scene(shape)[2])
    d, k, _ = obj.assign(x0)
    smooth = ~np.isin(k, obj.hulls) | (d > 1e-3)
    assert smooth.sum() >= 0.5 * len(d)
    obj = skin_ref.SkinObjective(obj.m, obj.pts[smooth], obj.weight)
    c, g = obj(x0)
    k = obj.assign(x0)[1]
    assert abs(obj.value(x0, k) - c) <= 1e-12 * c

    def fd(h):
        out = np.empty_like(g)
        for i in range(x0.size):
            e = np.zeros(x0.size)
            e[i] = h
            out[i] = (obj.value(x0 + e, k) - obj.value(x0 - e, k)) / (2 * h)
        return out

    fd1, fd2 = fd(H_FD), fd(2 * H_FD)
    tol = 10.0 * np.abs(fd1 - fd2) + 1e-9 * np.abs(g).max()
    err = np.abs(g - fd1)
    print(f"{shape}: worst |g - fd| / tolerance {float((err / tol).max()):.3e}, max|g| {np.abs(g).max():.3e}")
    assert np.all(err <= tol), (int(np.argmax(err / tol)), float((err / tol).max()))


def _native_chain(m, pts, x, weight):
    """(u per skin, c, g) of the host's chain at x: fsdf_tree_transforms, the
    centres, fsdf_rbf_solve, the CPU oracle's accumulator at those rows,
    fsdf_rbf_adjoint, the wrench sums of iteration_finish (numpy, in its
    order), fsdf_config_gradient."""
    import oracle
    from flash import _lib
    lib = _lib.load()
    mech = m.mechanism
    nq, nb = mech.num_positions, mech.num_bodies
    R, t, _, _ = mech.body_transform_arrays(x[:nq])
    delta = x[nq:]
    solves, rows = [], []
    for _, body, local, drow, values in skin_ref.skins_of(m):
        n = len(body)
        C = np.empty((n, 3))
        for j in range(n):
            p = local[j] + (delta[3 * drow[j]:3 * drow[j] + 3] if drow[j] >= 0 else 0.0)
            C[j] = p if body[j] < 0 else R[body[j]] @ p + t[body[j]]
        u, lu, piv = np.empty(n + 4), np.empty((n + 4) ** 2), np.empty(n + 4, np.int32)
        v = np.ascontiguousarray(values)
        assert lib.fsdf_rbf_solve(n, C.ctypes.data, v.ctypes.data, u.ctypes.data, lu.ctypes.data, piv.ctypes.data) == 0
        solves.append((body, drow, C, u, lu, piv))
        rows += [np.hstack([C, u[:n, None]]), u[n:][None]]
    om = oracle.OracleModel.from_manipulator(m)
    S = len(m.surfaces)
    hull = [not hasattr(s, "skeleton_points") for s in m.surfaces]
    poses = np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (S, 1))
    for k, s in enumerate(m.surfaces):
        if hull[k]:
            poses[k, :9] = (R[s.body] @ s.frame.R).ravel()
            poses[k, 9:] = R[s.body] @ s.frame.t + t[s.body]
    acc = om.cost_accum(poses, pts, np.ascontiguousarray(np.concatenate(rows)))
    wrench, gd, off = np.zeros((nb, 6)), np.zeros(delta.size), 1 + 6 * S
    for body, drow, C, u, lu, piv in solves:
        n = len(body)
        block = np.ascontiguousarray(acc[off:off + 4 * n + 4])
        off += 4 * n + 4
        G, work = np.empty(3 * n), np.empty(n + 4)
        assert lib.fsdf_rbf_adjoint(n, C.ctypes.data, u.ctypes.data, lu.ctypes.data, piv.ctypes.data, block.ctypes.data,
                                    G.ctypes.data, work.ctypes.data) == 0
        G = G.reshape(n, 3)
        for j in range(n):
            b = body[j]
            if b >= 0:
                wrench[b, :3] -= G[j]
                wrench[b, 3:] -= np.cross(C[j], G[j])
            if drow[j] >= 0:
                gd[3 * drow[j]:3 * drow[j] + 3] += G[j] if b < 0 else R[b].T @ G[j]
    sb = np.array([s.body if h else -1 for s, h in zip(m.surfaces, hull)], np.int32)
    gq = mech.config_gradient(x[:nq], wrench, sb, np.ascontiguousarray(acc[1:1 + 6 * S]))
    g = np.concatenate([gq, gd + 2.0 * weight * delta])
    return [s[3] for s in solves], acc[0] + weight * float(delta @ delta), g


@pytest.mark.parametrize("shape", SHAPES)
def test_native_host_chain_against_the_reference(shape):
    """The weights u of fsdf_rbf_solve against the reference's fit in
    clongdouble, and the host chain's cost and whole-state gradient against the
    reference's, each within max(1e-9, 100 · precision_gap) of the largest
    entry. Prints the gap and the systems' condition numbers."""
    m, pts, x0 = skin_ref.scene(shape)
    obj, x0 = skin_ref.objective(shape), np.array(x0)
    gap, bound = skin_ref.precision_gap(shape), skin_ref.bound_of(shape)
    cond = skin_ref.condition_numbers(shape)
    us, c, g = _native_chain(m, pts, x0, obj.weight)
    c_ref, g_ref = obj(x0)
    eu = max(float(np.abs(u - ur.real.astype(np.float64)).max() / np.abs(ur.real).max())
             for u, (_, ur) in zip(us, obj.fits(x0, np.clongdouble)))
    ec = abs(c - c_ref) / c_ref
    eg = float(np.abs(g - g_ref).max() / np.abs(g_ref).max())
    print(f"{shape}: precision_gap {gap:.2e}, cond {max(cond):.2e}; u {eu:.2e}, c {ec:.2e}, g {eg:.2e} "
          f"of bound {bound:.1e}")
    assert eu <= bound and ec <= bound and eg <= bound, (eu, ec, eg, bound)


@pytest.mark.parametrize("shape", SHAPES)
def test_rate_table(shape):
    """skin_ref.RATES holds what reference_rate's rule gives: the rate passes
    (half of the coordinates unclipped in each of the reference's first four
    iterations, with and without divisors; the fourth step at least 1 % of the
    first), and twice the rate does not, or the rate is 64."""
    rate = skin_ref.rate_of(shape)
    assert skin_ref.rate_holds(shape, rate)
    assert rate == 64.0 or not skin_ref.rate_holds(shape, 2.0 * rate)
