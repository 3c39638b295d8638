"""GPU: the Levenberg-Marquardt device loop (csrc/lm_solver.hip, gn_impl.h) on
the shape family of tests/mech_ref.py with at most 64 coordinates — one
coordinate, a full wave of Cholesky rows (float9_r1: nq = 64), the narrow and
wide subtree sums, quaternion joints below rotated revolute parents — against
the host loop bit for bit, its refusal beyond 64 coordinates, and its first
trial against mech_ref's independent reference (the damped step solved in
np.longdouble from the complex-step Jacobian)."""
import numpy as np
import pytest

import mech_ref

pytestmark = pytest.mark.gpu

CASES = [c for c in mech_ref.all_cases() if c[0] not in mech_ref.OVER_64]
IDS = [mech_ref.case_id(c) for c in CASES]
WEIGHT = 10.0  # (the regularizer's weight register_native passes: rigid scenes have no deformation)
FSDF_ERR_STATE = 3
# shapes whose host run on the noisy cloud rejects trials (1 to 7 of its 7; one-coordinate shapes and most
# `angles` triples accept them all, and are compared on the accept branch alone)
REJECTING = ("chain_2", "chain_3", "chain_4", "chain_5", "chain_8", "chain_9", "wide10", "wide11", "float9_r0",
             "float9_r1", "mixed")


def _fresh(m):
    from flash import _lib
    from flash.gradientdescent import register_native
    ctx = _lib.Context(device=0, precision=64, sort_points=True)
    ctx.set_surfaces([("hull", (s.hull.vertices, s.hull.faces, s.hull.planes)) for s in m.surfaces])
    register_native(m, ctx, WEIGHT)
    return ctx


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and a[3] == b[3]


def _both(ctx, device_mode, *args):
    res = []
    for mode in (False, device_mode):
        ctx.set_lm_solver(mode)
        res.append(ctx.descend_lm(*args))
    ctx.set_lm_solver(False)
    return res


def _rejections(ctx, x0, n, limit, damping):
    """Trials the Python loop over the context's value_gradient_hessian (the
    host loop's bits, tests/test_gpu_moments.py) rejects."""
    from flash.tracking import LevenbergMarquardt
    fs = []

    def vgh(x):
        c, g, H = ctx.value_gradient_hessian(x)
        fs.append(c / n)
        return c / n, g / n, H / n

    LevenbergMarquardt(len(x0), damping=damping, iteration_limit=limit,
                       gradient_convergence_tolerance=0.0).optimize(vgh, x0)
    best, rejected = np.inf, 0
    for f in fs:
        if f < best:
            best = f
        else:
            rejected += 1
    return rejected


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_loop_equals_host_loop(case):
    """x, f, the evaluations and the final damping of the required device loop
    equal the host loop's: limit 6 at damping 1e-3, and limit 8 at damping 1e-9
    on a noisy cloud (sigma 2 cm, 20 % outliers), where trials are rejected."""
    m, pts, x0 = mech_ref.scene(*case)
    _, noisy, _ = mech_ref.scene(*case, noisy=True)
    x0 = np.array(x0)
    ctx = _fresh(m)
    try:
        ctx.set_points(pts)
        n = float(len(pts))
        ctx.value_and_gradient(x0)  # (the cloud's first pass: both loops start from the same layout)
        host, dev = _both(ctx, "require", x0, 6, 1e-3, 0.5, 0.0, n)
        print(f"{mech_ref.case_id(case)} limit 6: evaluations {host[2]}, f {host[1]:.6e}, damping {host[3]:.1e}")
        assert _same(host, dev), (host, dev)
        assert host[2] == 6 and not np.array_equal(host[0], x0)
        ctx.set_points(noisy)
        n = float(len(noisy))
        ctx.value_and_gradient(x0)
        rejected = _rejections(ctx, x0, n, 8, 1e-9)
        host, dev = _both(ctx, "require", x0, 8, 1e-9, 0.5, 0.0, n)
        print(f"{mech_ref.case_id(case)} noisy: evaluations {host[2]}, rejected {rejected}, damping {host[3]:.1e}")
        assert _same(host, dev), (host, dev)
        assert host[2] == 8
        if case[0] in REJECTING:
            assert rejected > 0  # (the reject branch is compared)
    finally:
        ctx.close()


@pytest.mark.parametrize("shape", ["float9_r2", "float10"])
def test_over_the_coordinate_limit(shape):
    """nq = 65 and 70: "require" is refused with FSDF_ERR_STATE; the default
    device mode runs the host loop, bit for bit."""
    from flash._lib import FlashNativeError
    m, pts, x0 = mech_ref.scene(shape)
    x0 = np.array(x0)
    assert x0.size > 64
    ctx = _fresh(m)
    try:
        ctx.set_points(pts)
        n = float(len(pts))
        ctx.value_and_gradient(x0)
        ctx.set_lm_solver("require")
        with pytest.raises(FlashNativeError) as e:
            ctx.descend_lm(x0, 3, 1e-3, 0.5, 0.0, n)
        assert e.value.status == FSDF_ERR_STATE and "does not fit" in str(e.value)
        host, dev = _both(ctx, True, x0, 4, 1e-3, 0.5, 0.0, n)
        assert _same(host, dev), (host, dev)
        assert host[2] == 4 and not np.array_equal(host[0], x0)
    finally:
        ctx.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_first_trial_matches_the_reference(case):
    """Damping 1, two evaluations. An accepted trial: x − x0 equals
    lm_trial_ref within (nq + 1) · 1e-9 · max |step| — the Jacobi-scaled
    H + λD at λ = 1 has its eigenvalues in [1, nq + 1], and the matrix and the
    gradient are sums good to 1e-9 — and f equals c_ref(x_1) / N at 1e-9. A
    rejected one: x is x0 bit for bit. The reference accepts on every chain_k
    and mixed shape (tests/test_mech_ref.py), so those must accept here."""
    m, pts, x0 = mech_ref.scene(*case)
    x0 = np.array(x0)
    nq, n = x0.size, float(len(pts))
    ref = mech_ref.ObjectiveRef(m, pts)
    ctx = _fresh(m)
    try:
        ctx.set_points(pts)
        ctx.set_lm_solver("require")
        x, f, its, lam = ctx.descend_lm(x0, 2, 1.0, 0.5, 0.0, n)
    finally:
        ctx.close()
    assert its == 2
    c0, g, _, H = ref(x0)
    if np.array_equal(x, x0):
        print(f"{mech_ref.case_id(case)}: the first trial was rejected (f stays {f:.6e})")
        assert abs(f - c0 / n) <= 1e-9 * c0 / n and lam == 10.0
        assert not (case[0].startswith("chain_") or case[0] == "mixed")
        return
    step, _ = mech_ref.lm_trial_ref(H / n, g / n, 1.0, 0.5)
    err = float(np.abs((x - x0) - step).max())
    bound = (nq + 1) * 1e-9 * float(np.abs(step).max())
    c1 = ref.value(x)
    ef = abs(f - c1 / n) / (c1 / n)
    print(f"{mech_ref.case_id(case)}: LM trial err / bound {err / bound:.2e} (max |step| {np.abs(step).max():.3e}), "
          f"f rel err {ef:.2e}")
    assert lam == 0.1 and f < c0 / n
    assert err <= bound
    assert ef <= 1e-9
