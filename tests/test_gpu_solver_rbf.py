"""GPU: the device solver loop of fsdf_descend on scenes with RBF skins and
deformations (csrc/solver.hip, csrc/solver_rbf.h with csrc/rbf_impl.h;
fsdf_set_solver modes 3 "all" and 4 "require-all").

The step does on the device what the host loop does around every pass — the
adjoint of the skins' weight solve, the body wrenches, the deformation
gradient and regularizer, then after the step's FK the new centres, the
(n+4)x(n+4) LU and the weight solve — with the host's arithmetic in the host's
order of additions, so x, f and the iteration count equal the host loop's bit
for bit. No tolerance: a difference is an operation done in another order."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (tolerance, limit, rate, divisors?) of tests/test_gpu_solver.py's rigid test
ARGS = ((0.0, 7, 0.5, False), (1e-3, 40, 2.0, True), (1e30, 5, 1.0, False))


def _build(name):
    """(manipulator, x_true) of a scene: x_true the zero configuration with the
    scene's own placements, no deformation."""
    import flash
    from flash import Models
    if name == "irb_and_squishable":
        m, x = Models.irb_and_squishable()
        return m, np.asarray(x, np.float64)
    if name == "sphere71":
        return _sphere_skin(70), np.array([0.2])
    if name == "two_link_arm+beanbag":
        bag = Models.beanbag()
        bag.mechanism.body_names[1] = "beanbag_body"  # (the arm has a "body1" of its own)
        m = Models.merge(Models.two_link_arm(), bag)
    else:
        m = getattr(Models, name)()
    x = np.zeros(flash.num_states(m))
    x[:m.mechanism.num_positions] = m.mechanism.zero_configuration()
    return m, x


_SCENES = {}


def _scene(name):
    """The scene, a 4,000-point cloud around its skins at x_true, and a start x0
    off it in every entry: bodies translated and turned, quaternions slightly
    unnormalised, non-zero deformations. Built once per scene."""
    if name not in _SCENES:
        from flash import synthetic
        m, x_true = _build(name)
        pts = synthetic.skin_cloud(m, x_true, 4000, seed=11)
        x0 = x_true + np.random.default_rng(12).normal(0.0, 0.03, len(x_true))
        _SCENES[name] = (m, pts, x0)
    return _SCENES[name]


def _both(cf, modes, x0, limit, rate, tol, div, n):
    res = []
    for mode in modes:
        cf.ctx.set_solver(mode)
        res.append(cf.descend(x0, limit, rate, 0.05, tol, div, n))
    cf.ctx.set_solver(True)  # (the default)
    return res


def _assert_same(a, b):
    (xa, fa, ia), (xb, fb, ib) = a, b
    assert ia == ib, (ia, ib)
    assert fa == fb, (fa, fb)
    assert np.array_equal(xa, xb), np.abs(xa - xb).max()


@pytest.mark.parametrize("name,precision,nx", [
    ("beanbag", 64, 25), ("beanbag", 32, 25),  # one quaternion body, 7 centres, 6 deformation rows: m = 11
    ("squishable", 64, 43),                    # m = 17
    ("two_link_arm", 64, 2),                   # a rigid skin on two revolute bodies: body wrenches, m = 50
    ("irb_and_squishable", 64, 63), ("irb_and_squishable", 32, 63),  # hulls + skin + table in one step
    ("two_link_arm+beanbag", 64, 27),          # two skins: the block and deformation row offsets
    ("sphere71", 64, 1),                       # m = 75: two rows per lane in the pivot search and the solves
])
def test_rbf_device_loop_bit_identical_to_host_loop(name, precision, nx):
    from flash.gradientdescent import CostFunctor
    m, pts, x0 = _scene(name)
    assert len(x0) == nx
    cf = CostFunctor(m, pts, precision=precision)
    div = np.linspace(1.0, 1.5, nx)
    for tol, limit, rate, with_div in ARGS:
        host, dev, opt = _both(cf, (False, "require-all", "all"), x0, limit, rate, tol, div if with_div else None,
                               float(len(pts)))
        _assert_same(host, dev)
        # ("all" decides as "require-all" does — one condition in fsdf_descend — and only falls back where that fails)
        _assert_same(host, opt)
        xb, fb, ib = dev
        if tol == 0.0:
            assert ib == limit
        if tol == 1e30:  # converged at the first evaluation: x untouched
            assert ib == 1 and np.array_equal(xb, x0)


def _sphere_skin(n=100):
    """A rigid skin of n distinct points on a sphere and one skeleton point on
    one revolute body. n = 100: m = 105, whose LU alone (88 KB) exceeds the
    step's LDS; n = 70: m = 75 fits (a 45 KB LU)."""
    from flash.core import Manipulator, RigidInterpolatingSkin
    from flash.mechanism import Mechanism, Revolute
    mech = Mechanism("world")
    body = mech.attach(0, Revolute([0, 0, 1], "joint1"), None, "body1")
    k = np.arange(n) + 0.5
    phi, th = np.arccos(1.0 - 2.0 * k / n), np.pi * (1.0 + 5.0 ** 0.5) * k
    p = 0.5 * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1) + [0.6, 0.0, 0.0]
    return Manipulator(mech, [RigidInterpolatingSkin([(body, q) for q in p], [(body, [0.6, 0.0, 0.0])])])


def test_skin_too_large_for_the_step():
    """"require-all" refuses the scene (FSDF_ERR_STATE); "all" falls back to
    the host loop: its x, f and count exactly."""
    from flash import synthetic
    from flash._lib import FlashNativeError
    from flash.gradientdescent import CostFunctor
    m = _sphere_skin()
    pts = synthetic.skin_cloud(m, np.array([0.2]), 3000, seed=3)
    cf = CostFunctor(m, pts)
    x0 = np.array([0.25])
    cf.ctx.set_solver("require-all")
    with pytest.raises(FlashNativeError):
        cf.descend(x0, 3, 1.0, 0.05, 0.0, None, float(len(pts)))
    host, dev = _both(cf, (False, "all"), x0, 3, 1.0, 0.0, None, float(len(pts)))
    _assert_same(host, dev)


def test_singular_system_fails_as_on_the_host():
    """Beanbag with δ_0 = (2, 0, 0): centre 0 = (-1, 0, 0) + δ_0 lies exactly on
    centre 1 = (1, 0, 0) (identity pose), two equal rows — fsdf_rbf_solve
    reports FSDF_ERR_DEGENERATE for these centres on the CPU. Both loops raise,
    and the context stays usable."""
    from flash._lib import FlashNativeError
    from flash.gradientdescent import CostFunctor
    m, pts, x0 = _scene("beanbag")
    _, bad = _build("beanbag")
    bad[7:10] = (2.0, 0.0, 0.0)
    cf = CostFunctor(m, pts)
    for mode in (False, "require-all"):
        cf.ctx.set_solver(mode)
        with pytest.raises(FlashNativeError):
            cf.descend(bad, 3, 1.0, 0.05, 0.0, None, float(len(pts)))
        x, f, its = cf.descend(x0, 2, 1.0, 0.05, 0.0, None, float(len(pts)))
        assert its == 2 and np.isfinite(f)
    cf.ctx.set_solver(True)


def test_default_mode_keeps_rbf_scenes_on_the_host_loop():
    """set_solver(True) (mode 1, the default) on an RBF scene: the host loop's
    result bit for bit (mode 2's refusal: tests/test_gpu_solver.py)."""
    from flash.gradientdescent import CostFunctor
    m, pts, x0 = _scene("squishable")
    cf = CostFunctor(m, pts)
    host, default = _both(cf, (False, True), x0, 4, 0.5, 0.0, None, float(len(pts)))
    _assert_same(host, default)
