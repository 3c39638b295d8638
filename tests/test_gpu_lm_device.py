"""GPU: the device-resident Levenberg-Marquardt loop (fsdf_set_lm_solver,
csrc/lm_solver.hip lm_step_kernel / lm_pose_kernel) against fsdf_descend_lm's host
loop — x, f, the evaluation count and the final damping bit for bit, with and
without the prior of fsdf_set_lm_prior — its refusals, its buffer discipline
and its way through estimate_state."""
import numpy as np
import pytest

from gn_helpers import convergence_case, floating_scene

pytestmark = pytest.mark.gpu

WEIGHT = 10.0  # (the regularizer's weight register_native passes: rigid scenes have no deformation)


def _specs(m):
    return [("hull", (s.hull.vertices, s.hull.faces, s.hull.planes)) for s in m.surfaces]


def _load_model(ctx, m):
    from flash.gradientdescent import register_native
    ctx.set_surfaces(_specs(m))
    register_native(m, ctx, WEIGHT)


def _fresh(m):
    from flash import _lib
    ctx = _lib.Context(device=0, precision=64, sort_points=True)
    _load_model(ctx, m)
    return ctx


def _prior(nq):
    """A vector prior, zero on every third coordinate."""
    return np.where(np.arange(nq) % 3 == 0, 0.0, 1e-3) * (1.0 + np.arange(nq) % 4)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and a[3] == b[3]


@pytest.fixture(scope="module")
def scenes():
    """name -> (manipulator, cloud, start, (noisy cloud, its start))."""
    from flash import Models, synthetic
    out = {}
    m, pts, _, q0 = convergence_case()
    q_true, q_near = synthetic.perturbed_configuration(m, 41)
    out["irb140"] = (m, pts, q0, (synthetic.depth_cloud(m, q_true, 3000, seed=42), np.asarray(q_near, np.float64)))
    m, pts, x0 = floating_scene(20000)
    out["floating"] = (m, pts, x0, (pts, x0))  # (sigma 2 mm and 10 % box outliers already)
    m = Models.arm_grid()
    q_true, q0 = synthetic.perturbed_configuration(m, 31)
    q0 = np.asarray(q0, np.float64)
    big = synthetic.depth_cloud(m, q_true, 300000, seed=32)  # (at its defaults: sigma 5 mm, 10 % box outliers)
    out["m64_65536"] = (m, big[:65536], q0, (big[:65536], q0))
    out["m64_300000"] = (m, big, q0, (big, q0))
    return out


def _python_trace(ctx, x0, mu, n, limit, damping):
    """The Python loop over the context's value_gradient_hessian (the host
    loop's bits, tests/test_gpu_moments.py): (f, |g|) per evaluation."""
    from flash.tracking import LevenbergMarquardt, state_prior
    trace = []

    def vgh(x):
        c, g, H = ctx.value_gradient_hessian(x)
        return c / n, g / n, H / n

    F = state_prior(vgh, x0, mu)

    def rec(x):
        f, g, H = F(x)
        trace.append((f, float(np.sqrt(sum(float(v) * float(v) for v in g)))))
        return f, g, H

    s = LevenbergMarquardt(len(x0), damping=damping, iteration_limit=limit, gradient_convergence_tolerance=0.0)
    s.optimize(rec, x0)
    best, accepted = np.inf, []
    for f, nrm in trace:
        if f < best:
            best = f
            accepted.append(nrm)
    return trace, accepted


@pytest.mark.parametrize("with_prior", [False, True], ids=["plain", "prior"])
@pytest.mark.parametrize("scene", ["irb140", "floating", "m64_65536", "m64_300000"])
def test_device_loop_equals_host_loop(scenes, scene, with_prior):
    """Five settings per scene, each on both loops: (limit 6, tolerance 0); (30,
    just above the third accepted point's |g|): an early stop; (5, 1e30): one
    evaluation; a noisy cloud at damping 1e-9, limit 8, where the host run
    rejects trials (IRB140: 3 of 8 accepted, the floating scene 3-6, M64 at
    65,536 points 5-6); and the same cloud, damping and limit warm-started at
    that run's end point, as the next frame of a sequence would be: Gauss-Newton
    steps at a converged point fit the noise and are rejected (M64 at 300,000
    points: 2-3 of 8 accepted). Every scene asserts a rejection from its host
    run in the last setting. The fourth setting's host run on M64 at 300,000
    points accepts all 8 trials from every start tried (sigma 0.05 to 0.3 rad,
    with and without a prior: a cloud that large determines every joint), so
    there that setting compares the bits and the fifth asserts the rejection;
    on the other scenes both do."""
    m, pts, x0, (noisy, x0_noisy) = scenes[scene]
    nq = len(x0)
    mu = _prior(nq) if with_prior else None
    ctx = _fresh(m)
    try:
        ctx.set_lm_prior(mu)

        def both(x, limit, damping, tol, n):
            res = []
            for mode in (False, "require"):
                ctx.set_lm_solver(mode)
                res.append(ctx.descend_lm(x, limit, damping, 0.5, tol, n))
            ctx.set_lm_solver(False)
            return res

        ctx.set_points(pts)
        n = float(len(pts))
        ctx.value_and_gradient(x0)  # (the cloud's first pass: both loops start from the same layout)
        host, dev = both(x0, 6, 1e-3, 0.0, n)
        print(f"{scene} prior={with_prior} limit 6: evaluations {host[2]}, f {host[1]:.6e}, damping {host[3]:.1e}")
        assert _same(host, dev), (host, dev)
        assert host[2] == 6 and not np.array_equal(host[0], x0)
        # a tolerance just above the third accepted point's |g|: both loops stop there
        _, accepted = _python_trace(ctx, x0, mu, n, 6, 1e-3)
        assert len(accepted) >= 3
        host, dev = both(x0, 30, 1e-3, accepted[2] * 1.000001, n)
        assert _same(host, dev), (host, dev)
        assert host[2] < 30
        # converged at the start: one evaluation, x untouched, f = c / N (the prior is 0 at its reference)
        host, dev = both(x0, 5, 1e-3, 1e30, n)
        assert _same(host, dev), (host, dev)
        assert dev[2] == 1 and np.array_equal(dev[0], x0)
        assert dev[1] == ctx.value_gradient_hessian(x0)[0] / n
        # a noisy cloud at a tiny damping: rejected trials
        if noisy is not pts:
            ctx.set_points(noisy)
            ctx.value_and_gradient(x0_noisy)
        n = float(len(noisy))
        trace, accepted = _python_trace(ctx, x0_noisy, mu, n, 8, 1e-9)
        host, dev = both(x0_noisy, 8, 1e-9, 0.0, n)
        print(f"{scene} prior={with_prior} noisy: evaluations {host[2]}, accepted {len(accepted)}, "
              f"damping {host[3]:.1e}")
        assert host[2] == len(trace) == 8
        if scene != "m64_300000":
            assert len(trace) > len(accepted)  # (a rejected trial: the reject branch is compared)
        assert _same(host, dev), (host, dev)
        # warm-started at that run's end point (the prior's reference is then that point)
        x1 = host[0].copy()
        ctx.value_and_gradient(x1)
        trace, accepted = _python_trace(ctx, x1, mu, n, 8, 1e-9)
        host, dev = both(x1, 8, 1e-9, 0.0, n)
        print(f"{scene} prior={with_prior} warm start: evaluations {host[2]}, accepted {len(accepted)}, "
              f"damping {host[3]:.1e}")
        assert host[2] == len(trace) > len(accepted)  # (on every scene: a rejected trial)
        assert _same(host, dev), (host, dev)
    finally:
        ctx.close()


# At this damping the host runs below reject trials: `comb` 4 of 8 in its first
# frame and 7 in the warm-started one; `hand` from the scene's own start accepts
# all 16 with the prior (each frame's reference moves with it), so its start is
# this much further off (rad, seed 7): 4 of the second frame's 8 rejected with
# the prior, 6 without.
BRANCHING_DAMPING = 1e-9
BRANCHING_START_SIGMA = {"hand": 0.15, "comb": 0.0}


@pytest.mark.parametrize("with_prior", [False, True], ids=["plain", "prior"])
@pytest.mark.parametrize("scene", ["hand", "comb"])
def test_device_loop_equals_host_loop_on_branching_trees(scene, with_prior):
    """Trees that branch below the root (gn_helpers.branching_scene): the
    chain rule's level-ordered subtree sums and the matrix entries' ancestor
    walks between coordinates of different branches (and, in `hand`, through a
    body without coordinates), which no set of chains runs. Two frames of 8
    evaluations on both loops — from the perturbed start, then warm-started at
    that frame's end point, where Gauss-Newton steps fit the noise — x, f, the
    evaluations and the damping bit for bit; the host runs reject a trial."""
    from gn_helpers import branching_scene
    m, pts, x0 = branching_scene(scene)
    x0 = x0 + np.random.default_rng(7).normal(0.0, 1.0, len(x0)) * BRANCHING_START_SIGMA[scene]
    mu = _prior(len(x0)) if with_prior else None
    n = float(len(pts))
    ctx = _fresh(m)
    try:
        ctx.set_lm_prior(mu)
        ctx.set_points(pts)
        for frame in ("start", "warm start"):
            ctx.value_and_gradient(x0)  # (the cloud's first pass: both loops start from the same layout)
            trace, accepted = _python_trace(ctx, x0, mu, n, 8, BRANCHING_DAMPING)
            res = []
            for mode in (False, "require"):
                ctx.set_lm_solver(mode)
                res.append(ctx.descend_lm(x0, 8, BRANCHING_DAMPING, 0.5, 0.0, n))
            ctx.set_lm_solver(False)
            host, dev = res
            print(f"{scene} prior={with_prior} {frame}: evaluations {host[2]}, accepted {len(accepted)}, "
                  f"f {host[1]:.6e}, damping {host[3]:.1e}")
            assert host[2] == len(trace) == 8
            assert _same(host, dev), (host, dev)
            if frame == "start":
                assert not np.array_equal(host[0], x0)
            else:
                assert len(trace) > len(accepted)  # (a rejected trial: the reject branch is compared)
            x0 = host[0].copy()
    finally:
        ctx.close()


def test_bookkeeping_after_a_device_frame(scenes):
    """The returned f is the wrapped objective at the returned x, and the
    context evaluates as a fresh one right after a device frame."""
    m, pts, x0, _ = scenes["irb140"]
    n = float(len(pts))
    mu = _prior(len(x0))
    ctx, fresh = _fresh(m), _fresh(m)
    try:
        for c in (ctx, fresh):
            c.set_points(pts)
            c.value_and_gradient(x0)
        ctx.set_lm_solver("require")
        ctx.set_lm_prior(mu)
        x, f, its, lam = ctx.descend_lm(x0, 6, 1e-3, 0.5, 0.0, n)
        c, g, H = ctx.value_gradient_hessian(x)
        F = c / n + float(mu @ (x - x0) ** 2)
        assert abs(f - F) <= 1e-9 * abs(F), (f, F)
        c2, g2, H2 = fresh.value_gradient_hessian(x)
        assert abs(c - c2) <= 1e-9 * abs(c2)
        assert np.linalg.norm(g - g2) <= 1e-9 * np.linalg.norm(g2)
        assert np.linalg.norm(H - H2) <= 1e-9 * np.linalg.norm(H2)
    finally:
        ctx.close()
        fresh.close()


def test_refusals(scenes):
    from flash import Models, _lib
    from flash.gradientdescent import CostFunctor, flatten
    m, pts, x0, _ = scenes["irb140"]
    bare = _lib.Context(device=0)
    try:
        with pytest.raises(ValueError):  # a scalar weight before the mechanism: no coordinate count to repeat it to
            bare.set_lm_prior(1e-3)
    finally:
        bare.close()
    ctx = _fresh(m)
    try:
        with pytest.raises(_lib.FlashNativeError) as e:
            ctx.set_lm_solver(3)
        assert e.value.status == 1
        ctx.set_lm_solver("require")
        with pytest.raises(_lib.FlashNativeError) as e:  # no resident points
            ctx.descend_lm(x0, 3, 1e-3, 0.5)
        assert e.value.status == 3
        ctx.set_points(pts[:500])
        with pytest.raises(_lib.FlashNativeError) as e:  # damping 0
            ctx.descend_lm(x0, 3, 0.0, 0.5)
        assert e.value.status == 1
        with pytest.raises(_lib.FlashNativeError) as e:
            ctx.set_lm_prior(np.array([0.0, -1e-3, 0.0, 0.0, 0.0, 0.0]))
        assert e.value.status == 1
        with pytest.raises(_lib.FlashNativeError) as e:
            ctx.set_lm_prior(np.array([0.0, np.inf, 0.0, 0.0, 0.0, 0.0]))
        assert e.value.status == 1
        ctx.set_lm_prior(np.full(5, 1e-3))  # a wrong length: refused by the next descend, on either loop
        for mode in ("require", False):
            ctx.set_lm_solver(mode)
            with pytest.raises(_lib.FlashNativeError) as e:
                ctx.descend_lm(x0, 3, 1e-3, 0.5)
            assert e.value.status == 3
        ctx.set_lm_prior(None)
        ctx.set_lm_solver("require")
        x, f, its, lam = ctx.descend_lm(x0, 3, 1e-3, 0.5, 0.0, 500.0)
        assert its == 3
    finally:
        ctx.close()
    # an RBF / deformable scene: mode 2 refuses, mode 1 fails as the host loop does
    ms = Models.irb_and_squishable()[0]
    cf = CostFunctor(ms, np.zeros((10, 3)) + 0.3)
    xs = flatten(cf.state)
    for mode in ("require", True, False):
        cf.ctx.set_lm_solver(mode)
        with pytest.raises(_lib.FlashNativeError) as e:
            cf.ctx.descend_lm(xs, 3, 1e-3, 0.5)
        assert e.value.status == 3
    cf.ctx.set_lm_solver(False)


def test_zero_quaternion_fails_on_both_loops(scenes):
    from flash import _lib
    m, pts, x0, _ = scenes["floating"]
    ctx = _fresh(m)
    try:
        ctx.set_points(pts[:2000])
        bad = x0.copy()
        bad[13:17] = 0.0
        for mode in (False, "require"):
            ctx.set_lm_solver(mode)
            with pytest.raises(_lib.FlashNativeError) as e:
                ctx.descend_lm(bad, 4, 1e-3, 0.5, 0.0, 2000.0)
            assert e.value.status == 1
        res = []
        for mode in (False, "require"):  # the context works afterwards
            ctx.set_lm_solver(mode)
            res.append(ctx.descend_lm(x0, 4, 1e-3, 0.5, 0.0, 2000.0))
        assert _same(*res) and res[0][2] == 4
    finally:
        ctx.close()


def _table_scene():
    from flash import Models, synthetic
    m = Models.table()
    x_true = np.array(m.mechanism.zero_configuration(), np.float64)
    x_true[4:7] = (0.4, 0.0, 0.6)
    pts = synthetic.depth_cloud(m, x_true, 500, seed=9, sigma=0.002)
    x0 = x_true.copy()
    x0[:4] = [0.998, 0.03, -0.02, 0.01]
    x0[4:7] += 0.02
    return m, pts, x0


def test_device_frame_is_a_fresh_contexts_first_call(scenes):
    """descend_lm on the device loop as the very first call of a context: every
    buffer the frame touches is reserved by the frame itself."""
    m, pts, x0, _ = scenes["irb140"]
    res = []
    for mode in ("require", False):
        ctx = _fresh(m)
        try:
            ctx.set_lm_solver(mode)
            ctx.set_points(pts)
            res.append(ctx.descend_lm(x0, 5, 1e-3, 0.5, 0.0, float(len(pts))))
        finally:
            ctx.close()
    assert _same(*res) and res[0][2] == 5


def test_buffers_follow_cloud_sizes_and_a_model_swap():
    """One context walked through 1,000 -> 65,573 -> 64 points and a model swap
    (IRB140 -> one floating box), every frame on the device loop; each step
    against the host loop of a fresh context, bit for bit."""
    from flash import Models, synthetic
    irb = Models.irb140()
    q_true, q0 = synthetic.perturbed_configuration(irb, 41, sigma=0.1)
    q0 = np.asarray(q0, np.float64)
    pool = synthetic.depth_cloud(irb, q_true, 65573, seed=44)
    table, tpts, tx0 = _table_scene()
    steps = [(irb, pool[:1000], q0), (irb, pool, q0), (irb, pool[:64], q0), (table, tpts, tx0)]
    walked = _fresh(irb)
    walked.set_lm_solver("require")
    try:
        model = irb
        for k, (m, pts, x0) in enumerate(steps):
            if m is not model:
                _load_model(walked, m)
                model = m
            mu = None if k % 2 == 0 else np.full(len(x0), 1e-3)
            walked.set_points(pts)
            walked.set_lm_prior(mu)
            dev = walked.descend_lm(x0, 5, 1e-3, 0.5, 0.0, float(len(pts)))
            fresh = _fresh(m)
            try:
                fresh.set_points(pts)
                fresh.set_lm_prior(mu)
                host = fresh.descend_lm(x0, 5, 1e-3, 0.5, 0.0, float(len(pts)))
            finally:
                fresh.close()
            assert _same(host, dev), (k, host, dev)
            assert dev[2] >= 1 and not np.array_equal(dev[0], x0)
    finally:
        walked.close()


def test_estimate_state_on_the_device_loop(scenes):
    from flash.tracking import LevenbergMarquardt, estimate_state
    m, pts, x0, _ = scenes["irb140"]
    n = len(x0)
    dev = LevenbergMarquardt(n, iteration_limit=6, device_loop=True, prior_weight=1e-3)
    x_dev = estimate_state(m, pts, x0, solver=dev)
    host = LevenbergMarquardt(n, iteration_limit=6, device_loop=False, prior_weight=1e-3)
    x_host = estimate_state(m, pts, x0, solver=host)
    assert np.array_equal(x_dev, x_host)
    assert dev.iterations == host.iterations >= 1 and dev.final_damping == host.final_damping
    seen = []
    cb = LevenbergMarquardt(n, iteration_limit=6, device_loop=True, prior_weight=1e-3)
    x_cb = estimate_state(m, pts, x0, callback=lambda x, c: seen.append(c), solver=cb)
    assert np.array_equal(x_cb, x_host) and len(seen) == cb.iterations == host.iterations
    # a solver's device_loop and prior hold for its call alone: the mode chosen on the context stays
    m.engine().set_lm_solver(True)
    plain = LevenbergMarquardt(n, iteration_limit=6)
    assert not np.array_equal(estimate_state(m, pts, x0, solver=plain), x_host)
    assert m.engine().lm_solver_mode == 1
    m.engine().set_lm_solver(False)


@pytest.mark.parametrize("seed", [41, 7, 19])
def test_prior_stops_the_drift_on_the_device_loop(seed):
    """tests/test_lm_prior.py's drift case, the with-prior half: IRB140, 3,000
    noisy points, 4 evaluations, mu = 1e-3, on the device loop: within 0.2 rad
    of the truth."""
    from flash import Models, synthetic
    from flash.gradientdescent import CostFunctor
    from flash.tracking import LevenbergMarquardt, _optimize
    m = Models.irb140()
    q_true, q0 = synthetic.perturbed_configuration(m, seed)
    pts = synthetic.depth_cloud(m, q_true, 3000, seed=seed + 1)
    cf = CostFunctor(m, pts)
    solver = LevenbergMarquardt(len(q0), damping=1e-3, max_step=0.5, iteration_limit=4,
                                gradient_convergence_tolerance=0.0, prior_weight=1e-3, device_loop="require")
    x = _optimize(cf, len(pts), np.asarray(q0, np.float64), None, solver)
    err = float(np.max(np.abs(x - np.asarray(q_true, np.float64))))
    print(f"seed {seed}: max |x - q_true| {err:.3f} rad after {solver.iterations} evaluations")
    assert solver.iterations == 4 and err <= 0.2
