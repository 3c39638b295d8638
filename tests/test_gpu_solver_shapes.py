"""GPU: the NaiveSolver device loop (csrc/solver.hip, solver_common.h,
kin_impl.h) on the shape family of tests/mech_ref.py — every form of the
step's shape-dependent code: |g|² by readlane and by thread 0 (nx = 63, 64, 65,
70), the chain walk's groups of four with every remainder, the narrow and the
wide subtree sums on either side of their boundary (10 and 11 parents at a
height), more than 64 surfaces, quaternion joints below rotated revolute
parents with non-identity joint frames, kin::sincos at its branch points, and
the step's LDS at capacity and beyond.

Two checks per shape. The device loop equals the host loop bit for bit (x, f,
the iteration count). And — not a self-comparison — every step of the device
loop's own trajectory equals the step of mech_ref's independent reference
(complex-step kinematics, the CPU oracle's per-point values, plain sums) taken
from the device's previous iterate: iterations 2 and later are where a stale
joint frame, a wrong slot parity, a wrong subtree order or a wrong quaternion
row would show."""
import numpy as np
import pytest

import mech_ref

pytestmark = pytest.mark.gpu

CASES = mech_ref.all_cases()
IDS = [mech_ref.case_id(c) for c in CASES]
FSDF_ERR_STATE = 3
STEPS = 4


def _functor(case, precision=64):
    from flash.gradientdescent import CostFunctor
    m, pts, x0 = mech_ref.scene(*case)
    return CostFunctor(m, pts, precision=precision), m, pts, np.array(x0)


def _both(cf, device_mode, *args):
    res = []
    for mode in (False, device_mode):
        cf.ctx.set_solver(mode)
        res.append(cf.descend(*args))
    cf.ctx.set_solver(True)  # (the default)
    return res


def _bit_identical(cf, x0, n, rate, label, device_mode="require"):
    """tests/test_gpu_solver.py's three settings at the shape's rate: a run that
    never stops; one with divisors and a tolerance just above |g| at the host
    loop's third iterate, which stops there or earlier; one converged at the
    first evaluation, whose f is the cost of the device's FK at x0."""
    div = mech_ref.divisors_of(len(x0))
    cf.ctx.set_solver(False)
    x3, _, its = cf.descend(x0, 3, rate, mech_ref.MAX_STEP, 0.0, div, n)
    assert its == 3
    g = cf.value_and_gradient(x3)[1] / n / div
    tol3 = float(np.sqrt(sum(float(v) * float(v) for v in g))) * 1.000001
    for tol, limit, div_ in ((0.0, 7, None), (tol3, 8, div), (1e30, 5, None)):
        (xa, fa, ia), (xb, fb, ib) = _both(cf, device_mode, x0, limit, rate, mech_ref.MAX_STEP, tol, div_, n)
        print(f"{label} tolerance {tol:.3e}: iterations {ia}, f {fa!r}")
        assert ia == ib, (ia, ib)
        assert fa == fb, (fa, fb)
        assert np.array_equal(xa, xb), np.abs(xa - xb).max()
        if tol == 0.0:
            assert ib == limit and not np.array_equal(xb, x0)
        elif tol == 1e30:
            assert ib == 1 and np.array_equal(xb, x0)
            assert fb == cf.value_and_gradient(x0)[0] / n
        else:
            assert 1 <= ib < limit


def _steps_match_reference(cf, m, pts, x0, rate, label):
    """f_k = c_ref(x_{k-1}) / N at 1e-9 relative (RTOL_SUM: the sums differ in
    order, the poses in their last bits) and x_k − x_{k-1} = naive_step_ref at
    x_{k-1} within 1e-9 of the largest unclipped step plus 4 ulp of |x|; a
    component whose unclipped step is within 1e-9 relative of ±max_step need
    only lie inside the clip. At least half of the coordinates are unclipped in
    every iteration. Returns the worst (f, step) figures, each over its bound."""
    ref = mech_ref.ObjectiveRef(m, pts)
    n, nx, ms = float(len(pts)), len(x0), mech_ref.MAX_STEP
    div = mech_ref.divisors_of(nx)
    cf.ctx.set_solver("require")
    prev, worst_f, worst_x = x0, 0.0, 0.0
    try:
        for k in range(1, STEPS + 1):
            xk, fk, its = cf.descend(x0, k, rate, ms, 0.0, div, n)
            assert its == k
            c, g, _, _ = ref(prev)
            ef = abs(fk - c / n) / abs(c / n)
            step, raw = mech_ref.naive_step_ref(g / n, rate, ms, div)
            ulps = 4.0 * np.spacing(np.maximum(np.abs(prev), np.abs(xk)))
            bound = 1e-9 * np.abs(raw).max() + ulps
            got = xk - prev
            edge = np.abs(np.abs(raw) - ms) <= 1e-9 * ms
            excess = np.where(edge, np.maximum(np.abs(got) - (ms + ulps), 0.0) / bound, np.abs(got - step) / bound)
            free = int(np.count_nonzero(np.abs(raw) < ms * (1 - 1e-9)))
            print(f"{label} step {k}: f rel err {ef:.2e}, step err / bound {excess.max():.2e}, "
                  f"max |step| {np.abs(got).max():.3e}, unclipped {free} of {nx}")
            assert 2 * free >= nx
            assert ef <= 1e-9, (k, fk, c / n)
            assert excess.max() <= 1.0, (k, int(np.argmax(excess)), got[np.argmax(excess)], step[np.argmax(excess)])
            worst_f, worst_x = max(worst_f, ef), max(worst_x, float(excess.max()))
            prev = xk
    finally:
        cf.ctx.set_solver(True)
    assert not np.array_equal(prev, x0)
    return worst_f, worst_x


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_loop_bit_identical_to_host_loop(case):
    cf, m, pts, x0 = _functor(case)
    _bit_identical(cf, x0, float(len(pts)), mech_ref.rate_of(case), mech_ref.case_id(case))


def test_device_loop_bit_identical_in_an_fp32_context():
    cf, m, pts, x0 = _functor(("mixed", 0), precision=32)
    _bit_identical(cf, x0, float(len(pts)), mech_ref.rate_of(("mixed", 0)), "mixed-0 fp32")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_steps_match_the_reference(case):
    cf, m, pts, x0 = _functor(case)
    _steps_match_reference(cf, m, pts, x0, mech_ref.rate_of(case), mech_ref.case_id(case))


def test_scene_that_does_not_fit():
    """star_too_large (120 arms: 1 + 6S + 12nb + 2nx = 2413 > 2048 staged
    doubles): mode "require" is refused with FSDF_ERR_STATE and says why; the
    default mode runs the host loop (x, f and the count bit for bit)."""
    from flash._lib import FlashNativeError
    cf, m, pts, x0 = _functor(("star_too_large", 0))
    n = float(len(pts))
    cf.ctx.set_solver("require")
    with pytest.raises(FlashNativeError) as e:
        cf.descend(x0, 3, 64.0, mech_ref.MAX_STEP, 0.0, None, n)
    assert e.value.status == FSDF_ERR_STATE and "does not fit" in str(e.value)
    (xa, fa, ia), (xb, fb, ib) = _both(cf, True, x0, 3, 64.0, mech_ref.MAX_STEP, 0.0, None, n)
    assert ia == ib == 3 and fa == fb and np.array_equal(xa, xb) and not np.array_equal(xb, x0)


def test_largest_star_that_fits():
    """The arm count stepped down from 120 in sixes until "require" accepts:
    the step's carve at capacity (72 arms by solver_fits's formula, about 62 of
    the 64 KB). Both checks above at that size."""
    from flash._lib import FlashNativeError
    from flash.gradientdescent import CostFunctor
    arms = 120
    while arms > 64:
        m, pts, x0 = mech_ref.scene(f"star{arms}", 0, n=256)
        cf = CostFunctor(m, pts)
        cf.ctx.set_solver("require")
        try:
            cf.descend(np.array(x0), 1, 1.0, mech_ref.MAX_STEP, 0.0, None, float(len(pts)))
            break
        except FlashNativeError as e:
            assert e.status == FSDF_ERR_STATE and "does not fit" in str(e)
        finally:
            cf.ctx.set_solver(True)
            m.invalidate()
        arms -= 6
    print(f"largest star the device loop accepts: {arms} arms")
    assert 66 <= arms < 120
    case = (f"star{arms}", 0)
    cf, m, pts, x0 = _functor(case)
    _bit_identical(cf, x0, float(len(pts)), mech_ref.DEFAULT_RATE, case[0])
    _steps_match_reference(cf, m, pts, x0, mech_ref.DEFAULT_RATE, case[0])
