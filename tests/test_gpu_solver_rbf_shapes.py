"""GPU: the RBF half of the device solver step (csrc/solver_rbf.h with
csrc/rbf_impl.h; fsdf_set_solver mode 4 "require-all") on the skin shape family
of tests/skin_ref.py — every form of its shape-dependent code: W = m − 1 against
16 working waves (m = 8, 16, 17), the second row per lane on either side of
m = 64 (63 .. 66) and at the largest system the step accepts, exact ties in the
pivot column (the lattices), the second round of the per-wave skin loops (17
skins), skins of different sizes in one scene, centres on the world (b < 0), two
deformable skins with a hull between them, a deformable skin below a revolute
chain, and hulls, a skin and the table in one step.

Two checks per shape, as tests/test_gpu_solver_shapes.py makes them for rigid
scenes. The device loop equals the host loop bit for bit (x, f, the iteration
count). And — not a self-comparison, and the only check that sees an error in
the shared rbf_impl.h — every step of the device loop's own trajectory equals
the step of skin_ref's independent reference (complex-step gradient through
FK, centres, the weight solve and the field) taken from the device's previous
iterate, within max(1e-9, 100 · precision_gap) where the rigid test has 1e-9.
Every device run is under "require-all": a silent fall-back to the host loop
would fail."""
import numpy as np
import pytest

import mech_ref
import skin_ref
import test_gpu_solver_shapes as rigid

pytestmark = pytest.mark.gpu

SHAPES = list(skin_ref.SHAPES)
FSDF_ERR_STATE = 3
STEPS = 4
MODE = "require-all"


def _functor(shape, precision=64):
    from flash.gradientdescent import CostFunctor
    m, pts, x0 = skin_ref.scene(shape)
    return CostFunctor(m, pts, precision=precision), m, pts, np.array(x0)


def _bit_identical(shape, precision=64):
    """The three settings of test_gpu_solver_shapes._bit_identical at the shape's rate."""
    cf, m, pts, x0 = _functor(shape, precision)
    rigid._bit_identical(cf, x0, float(len(pts)), skin_ref.rate_of(shape), f"{shape} fp{precision}", MODE)


def _steps_match_reference(shape):
    """test_gpu_solver_shapes._steps_match_reference against skin_ref's
    objective, its fixed 1e-9 replaced by r = max(1e-9, 100 · precision_gap):
    f_k = c_ref(x_{k-1}) / N at r relative; x_k − x_{k-1} = naive_step_ref at
    x_{k-1} within r of the largest unclipped step plus 4 ulp of |x|; a
    component whose unclipped step is within r relative of ±max_step need only
    lie inside the clip. At least half of the coordinates are unclipped in
    every iteration. Returns the worst (f, step) figures, each over its bound."""
    cf, m, pts, x0 = _functor(shape)
    ref, r, rate = skin_ref.objective(shape), skin_ref.bound_of(shape), skin_ref.rate_of(shape)
    n, nx, ms = float(len(pts)), len(x0), skin_ref.MAX_STEP
    div = mech_ref.divisors_of(nx)
    cf.ctx.set_solver(MODE)
    prev, worst_f, worst_x = x0, 0.0, 0.0
    try:
        for k in range(1, STEPS + 1):
            xk, fk, its = cf.descend(x0, k, rate, ms, 0.0, div, n)
            assert its == k
            c, g = ref(prev)
            ef = abs(fk - c / n) / abs(c / n)
            step, raw = mech_ref.naive_step_ref(g / n, rate, ms, div)
            ulps = 4.0 * np.spacing(np.maximum(np.abs(prev), np.abs(xk)))
            bound = r * np.abs(raw).max() + ulps
            got = xk - prev
            edge = np.abs(np.abs(raw) - ms) <= r * ms
            excess = np.where(edge, np.maximum(np.abs(got) - (ms + ulps), 0.0) / bound, np.abs(got - step) / bound)
            free = int(np.count_nonzero(np.abs(raw) < ms * (1 - 1e-9)))
            print(f"{shape} step {k}: f rel err / bound {ef / r:.2e}, step err / bound {excess.max():.2e}, "
                  f"max |step| {np.abs(got).max():.3e}, unclipped {free} of {nx}, bound {r:.1e}")
            assert 2 * free >= nx
            assert ef <= r, (k, fk, c / n)
            assert excess.max() <= 1.0, (k, int(np.argmax(excess)), got[np.argmax(excess)], step[np.argmax(excess)])
            worst_f, worst_x = max(worst_f, ef / r), max(worst_x, float(excess.max()))
            prev = xk
    finally:
        cf.ctx.set_solver(True)
    assert not np.array_equal(prev, x0)
    return worst_f, worst_x


@pytest.mark.parametrize("shape", SHAPES)
def test_device_loop_bit_identical_to_host_loop(shape):
    _bit_identical(shape)


@pytest.mark.parametrize("shape", skin_ref.FP32_SHAPES)
def test_device_loop_bit_identical_in_an_fp32_context(shape):
    _bit_identical(shape, precision=32)


@pytest.mark.parametrize("shape", SHAPES)
def test_device_steps_match_the_reference(shape):
    _steps_match_reference(shape)


def _probe(n):
    """A functor of sphere{n} over a few random points: enough to ask whether the step accepts the scene."""
    from flash.gradientdescent import CostFunctor
    m, _ = skin_ref._manipulator(f"sphere{n}")
    pts = np.random.default_rng(n).uniform(-0.5, 1.5, (64, 3))
    return CostFunctor(m, pts), m, pts


def test_mmax_boundary():
    """The largest single skin the step accepts, its centres stepped down from
    100 by one: every larger one is refused by "require-all" with
    FSDF_ERR_STATE and "does not fit" (n + 1 the last of them), and run by the
    host loop under "all", bit for bit; the accepted n is skin_ref.MMAX_N (the
    step's LDS carve and stage_rbf's eight loads per thread at capacity), and
    both checks above hold there."""
    from flash._lib import FlashNativeError
    n = 100
    while n > 64:
        cf, m, pts = _probe(n)
        x0, npts = np.array([0.1]), float(len(pts))
        cf.ctx.set_solver(MODE)
        try:
            cf.descend(x0, 1, 1.0, skin_ref.MAX_STEP, 0.0, None, npts)
            break
        except FlashNativeError as e:
            assert e.status == FSDF_ERR_STATE and "does not fit" in str(e)
            if n in (100, skin_ref.MMAX_N + 1):  # ("all" on a refused scene: the host loop's bits)
                (xa, fa, ia), (xb, fb, ib) = rigid._both(cf, "all", x0, 3, 1.0, skin_ref.MAX_STEP, 0.0, None, npts)
                assert ia == ib == 3 and fa == fb and np.array_equal(xa, xb) and not np.array_equal(xb, x0)
        finally:
            cf.ctx.set_solver(True)
            m.invalidate()
        n -= 1
    print(f"largest skin the device loop accepts: {n} centres, m = {n + 4}")
    assert n == skin_ref.MMAX_N, n
    shape = f"sphere{n}"
    _bit_identical(shape)
    _steps_match_reference(shape)


def test_singular_lattice_fails_as_on_the_host():
    """lattice13 with deformable corners and δ_0 = (0.5, 0, 0): corner 0 lies
    exactly on corner 4 at every angle (the same body, p_0 + δ_0 == p_4 bit for
    bit), two equal rows. Both loops raise, and the context stays usable."""
    from flash._lib import FlashNativeError
    cf, m, pts, x0 = _functor("lattice13_soft")
    bad = x0.copy()
    bad[1:] = 0.0
    bad[1:4] = (0.5, 0.0, 0.0)
    n = float(len(pts))
    for mode in (False, MODE):
        cf.ctx.set_solver(mode)
        try:
            with pytest.raises(FlashNativeError):
                cf.descend(bad, 3, 1.0, skin_ref.MAX_STEP, 0.0, None, n)
            x, f, its = cf.descend(x0, 2, 1.0, skin_ref.MAX_STEP, 0.0, None, n)
            assert its == 2 and np.isfinite(f) and not np.array_equal(x, x0)
        finally:
            cf.ctx.set_solver(True)
