"""GPU: robust objectives on the device-resident solver loops
(fsdf_set_robust_loops; csrc/robust.hip robust_assemble_kernel and the skip flag,
csrc/descend.hip) and fsdf_eval_robust_device.

The criterion throughout is bit identity (np.array_equal, ==) between the
device loop and the host loop of the same build on the same context state; the
host loop itself is held to the Python loops and the CPU oracle elsewhere
(tests/test_gpu_robust.py, test_gpu_point_weights.py, test_gpu_free_space.py).
The device side always runs in the required modes (device_loop="require",
set_solver("require")): a silent fallback to the host loop is an error there,
not a pass.

Sizes: 37 points are one partial chunk; 513 are two robust workgroups, the
second holding one point (a workgroup's run is kRobustMinChunks = 8 chunks of
64); 3000 is the drift cloud of tests/test_gpu_robust.py."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, rng

pytestmark = pytest.mark.gpu

ERR_STATE = 3
LM = dict(damping=1e-3, max_step=0.5)


def _drift(n, seed=41):
    from flash import Models, synthetic
    m = Models.irb140()
    q_true, q0 = synthetic.perturbed_configuration(m, seed)
    return m, synthetic.depth_cloud(m, q_true, n, seed=seed + 1), np.asarray(q_true, np.float64), np.asarray(q0, np.float64)


def _m64():
    from flash import Models
    z = np.load(os.path.join(GOLDEN, "m64_2k.npz"))
    return Models.arm_grid(), z["points"], z["poses"], np.asarray(z["q"], np.float64)


def _objectives(n):
    """name -> (loss, weights, n_surface): the five objectives of the loops' tests."""
    from flash.robust import Huber, Tukey
    a = rng(911).uniform(0.25, 2.0, n)
    split = (2 * n) // 3
    assert 0 < split < n
    return {"huber": (Huber(0.02), None, None), "tukey": (Tukey(0.05), None, None), "weights": (None, a, None),
            "split": (None, None, split), "all": (Huber(0.02), a, split)}


def _functor(m, pts, loss=None, weights=None, split=None, precision=64, loops=True):
    from flash.gradientdescent import CostFunctor
    cf = CostFunctor(m, pts, precision=precision, loss=loss, robust_loops=loops)
    if weights is not None:
        cf.set_point_weights(weights)
    if split is not None:
        cf.set_free_split(split)
    return cf


def _outcome(call):
    """What a loop call gives: its result tuple as one flat array, or the status it was refused with."""
    from flash._lib import FlashNativeError
    try:
        out = call()
    except FlashNativeError as e:
        return ("error", e.status)
    return ("ok", np.concatenate([np.ravel(np.asarray(v, np.float64)) for v in out]))


def _same(a, b):
    return a[0] == b[0] and (np.array_equal(a[1], b[1]) if a[0] == "ok" else a[1] == b[1])


def _lm_pair(cf, q0, limit, tol, n, mu):
    host = _outcome(lambda: cf.descend_lm(q0, limit, LM["damping"], LM["max_step"], tol, n, prior_weight=mu,
                                          device_loop=False))
    dev = _outcome(lambda: cf.descend_lm(q0, limit, LM["damping"], LM["max_step"], tol, n, prior_weight=mu,
                                         device_loop="require"))
    return host, dev


def _naive_pair(cf, q0, limit, tol, n, div=None, rate=0.1):
    try:
        cf.ctx.set_solver(False)
        host = _outcome(lambda: cf.descend(q0, limit, rate, 0.5, tol, div, n))
        cf.ctx.set_solver("require")
        dev = _outcome(lambda: cf.descend(q0, limit, rate, 0.5, tol, div, n))
    finally:
        cf.ctx.set_solver(True)
    return host, dev


# ---- 1. the assembly alone ------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["irb140", "m64"])
def test_eval_robust_device_gives_eval_robusts_bits(scene):
    """fsdf_eval_robust_device into torch tensors against fsdf_eval_robust's accum
    and moments: Huber, Tukey, weights under SQUARE, a split under SQUARE, all
    three; with the moments and with d_moments = NULL (the rows of 8)."""
    import torch
    import flash
    from flash import _lib
    if scene == "irb140":
        m, pts, _, q0 = _drift(3000)
        poses = flash.hull_poses(m, q0)
    else:
        m, pts, poses, _ = _m64()
    S = len(m.surfaces)
    c = _lib.Context(device=0, sort_points=True)
    dev = torch.device("cuda", 0)
    try:
        c.set_surfaces([("hull", (s.hull.vertices, s.hull.faces, s.hull.planes)) for s in m.surfaces])
        c.set_points(pts)
        for name, (loss, a, split) in _objectives(len(pts)).items():
            c.set_loss(loss)
            c.set_point_weights(a)
            c.set_free_split(len(pts) if split is None else split)
            cost, accum, mom, _ = c.eval_robust(poses)
            accum8 = c.eval_robust(poses, moments=False)[1]
            # (filled with NaN: every entry must be written)
            d_acc = torch.full((1 + 6 * S,), float("nan"), dtype=torch.float64, device=dev)
            d_mom = torch.full((S, 21), float("nan"), dtype=torch.float64, device=dev)
            d_acc8 = torch.full((1 + 6 * S,), float("nan"), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            c.eval_robust_device(poses, d_acc.data_ptr(), d_mom.data_ptr())
            c.eval_robust_device(poses, d_acc8.data_ptr())
            c.synchronize()
            assert np.array_equal(d_acc.cpu().numpy(), accum), (scene, name)
            assert np.array_equal(d_mom.cpu().numpy(), mom), (scene, name)
            assert np.array_equal(d_acc8.cpu().numpy(), accum8), (scene, name)
            assert accum[0] == cost and np.abs(mom).max() > 0, (scene, name)
    finally:
        c.close()


def test_assembly_with_more_surfaces_than_a_workgroup_has_threads():
    """256 surfaces, the library's limit: the assembly's workgroup is kRobustAssembleBlock = 128
    threads, so Σρ takes a second tile and the copies more than one workgroup."""
    import torch
    from flash import _lib
    from flash.robust import Huber
    from test_gpu_shapes import _cloud, _poses, _random_hull
    r = rng(914)
    K = 256
    hulls = [_random_hull(r, int(r.integers(8, 40))) for _ in range(K)]
    poses = _poses(r, K, spread=0.6)
    pts = _cloud(r, poses, 5000, spread=0.08)
    c = _lib.Context(device=0, sort_points=True)
    dev = torch.device("cuda", 0)
    try:
        c.set_surfaces([("hull", h) for h in hulls])
        c.set_points(pts)
        c.set_loss(Huber(0.02))
        cost, accum, mom, _ = c.eval_robust(poses)
        accum8 = c.eval_robust(poses, moments=False)[1]
        d_acc = torch.full((1 + 6 * K,), float("nan"), dtype=torch.float64, device=dev)
        d_mom = torch.full((K, 21), float("nan"), dtype=torch.float64, device=dev)
        d_acc8 = torch.full((1 + 6 * K,), float("nan"), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        c.eval_robust_device(poses, d_acc.data_ptr(), d_mom.data_ptr())
        c.eval_robust_device(poses, d_acc8.data_ptr())
        c.synchronize()
        assert np.array_equal(d_acc.cpu().numpy(), accum) and np.array_equal(d_mom.cpu().numpy(), mom)
        assert np.array_equal(d_acc8.cpu().numpy(), accum8)
        assert (np.abs(mom[128:]).max(axis=1) > 0).any()  # (points nearest to a surface of the second tile)
    finally:
        c.close()


# ---- 2. the LM loop ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", [37, 513, 3000])
def test_lm_device_loop_equals_the_host_loop(n):
    """(x, f, evaluations, final damping) of descend_lm on the device with the
    switch on against the host loop, per objective, with and without a prior; at
    3000 points also (limit, tol) = (30, 1e-4), whose evaluations after
    convergence are the skipped launches."""
    m, pts, _, q0 = _drift(n)
    early = []
    for name, (loss, a, split) in _objectives(n).items():
        cf = _functor(m, pts, loss, a, split)
        cf.value_and_gradient(q0)  # (the cloud's first pass and its regroup: one layout for both loops)
        for mu in (None, 1e-3):
            for limit, tol in ((6, 0.0), (30, 1e-4)) if n == 3000 else ((6, 0.0),):
                host, dev = _lm_pair(cf, q0, limit, tol, n, mu)
                assert host[0] == "ok" and _same(host, dev), (n, name, mu, limit, host, dev)
                its = int(host[1][-2])
                assert 1 <= its <= limit
                if n == 3000:  # (the loop moved: the comparison is not of two untouched starts)
                    assert not np.array_equal(host[1][:len(q0)], q0), (n, name)
                if limit == 30:
                    early.append(its)
        cf.set_robust_loops(False)
    if n == 3000:
        print(f"LM evaluations under (30, 1e-4): {early}")
        assert min(early) < 30  # (a frame done early: its queued evaluations ran the skip path)


@pytest.mark.parametrize("name", ["huber", "all"])
def test_lm_device_loop_on_m64(name):
    m, pts, _, q = _m64()
    loss, a, split = _objectives(len(pts))[name]
    cf = _functor(m, pts, loss, a, split)
    cf.value_and_gradient(q)
    for mu in (None, 1e-3):
        host, dev = _lm_pair(cf, q, 6, 0.0, len(pts), mu)
        assert host[0] == "ok" and _same(host, dev), (name, mu, host, dev)
    cf.set_robust_loops(False)


def test_lm_device_loop_in_an_fp32_context():
    m, pts, _, q0 = _drift(3000)
    loss, a, split = _objectives(len(pts))["all"]
    cf = _functor(m, pts, loss, a, split, precision=32)
    cf.value_and_gradient(q0)
    for limit, tol in ((6, 0.0), (30, 1e-4)):
        host, dev = _lm_pair(cf, q0, limit, tol, len(pts), 1e-3)
        assert host[0] == "ok" and _same(host, dev), (limit, host, dev)
    cf.set_robust_loops(False)


# ---- 3. the NaiveSolver loop --------------------------------------------------------------------

def _midway_tolerance(cf, q0, limit, n, rate=0.1):
    """A tolerance the host loop meets first at an evaluation j + 1 with 1 <= j < limit − 1: half way
    between |g| at that evaluation and the least |g| before it, along NaiveSolver's own trajectory."""
    from flash.tracking import NaiveSolver
    norms = []

    def vg(x):
        c, g = cf.value_and_gradient(x)
        norms.append(float(np.linalg.norm(g / n)))
        return c / n, g / n

    NaiveSolver(len(q0), rate=rate, max_step=0.5, iteration_limit=limit,
                gradient_convergence_tolerance=0.0).optimize(vg, q0)
    for j in range(1, limit - 1):
        if norms[j] < min(norms[:j]):
            return 0.5 * (norms[j] + min(norms[:j])), j + 1
    raise AssertionError(f"no evaluation lowers |g|: {norms}")


@pytest.mark.parametrize("n", [37, 513, 3000])
def test_naive_device_loop_equals_the_host_loop(n):
    m, pts, _, q0 = _drift(n)
    for name, (loss, a, split) in _objectives(n).items():
        cf = _functor(m, pts, loss, a, split)
        cf.value_and_gradient(q0)
        host, dev = _naive_pair(cf, q0, 8, 0.0, n)
        assert host[0] == "ok" and _same(host, dev), (n, name, host, dev)
        assert int(host[1][-1]) == 8 and not np.array_equal(host[1][:len(q0)], q0)
        if n == 3000:
            tol, stop = _midway_tolerance(cf, q0, 8, n)
            assert tol > 0.0
            host, dev = _naive_pair(cf, q0, 8, tol, n)
            assert host[0] == "ok" and _same(host, dev), (n, name, tol, host, dev)
            assert int(host[1][-1]) == stop < 8, (name, tol, host)  # (the steps after it were skipped)
        cf.set_robust_loops(False)


def test_naive_device_loop_with_divisors():
    m, pts, _, q0 = _drift(3000)
    loss, a, split = _objectives(len(pts))["all"]
    cf = _functor(m, pts, loss, a, split)
    cf.value_and_gradient(q0)
    div = np.linspace(0.5, 2.0, len(q0))
    host, dev = _naive_pair(cf, q0, 6, 0.0, len(pts), div)
    assert host[0] == "ok" and _same(host, dev), (host, dev)
    plain = _naive_pair(cf, q0, 6, 0.0, len(pts))[1]
    assert not _same(plain, dev)  # (the divisors act)
    cf.set_robust_loops(False)


# ---- 4. the regroup inside the loop ---------------------------------------------------------------

@pytest.mark.parametrize("loop", ["lm", "naive"])
def test_the_first_evaluations_regroup_inside_the_loop(loop):
    """A fresh functor whose first evaluation happens inside the loop, on a cloud the auto rule
    regroups after it (tests/test_gpu_point_weights.py's recipe): evaluation 0 reads the Hilbert
    layout's weights and permutation, the later ones the regrouped layout's — as the host loop's."""
    from flash import Models
    from flash.gradientdescent import CostFunctor
    _, pts, _, q0 = _drift(4000)
    n = len(pts)
    a = rng(912).uniform(0.25, 2.0, n)  # (distinct per point: a stale gather shows)
    assert len(np.unique(a)) == n
    split = (3 * n) // 4
    out = {}
    for side in ("device", "host"):
        cf = CostFunctor(Models.irb140(), np.zeros((0, 3)), robust_loops=(side == "device"))
        ctx = cf.ctx
        ctx.set_plan(False)
        ctx.set_partition(0, 0)  # every pass one wave per chunk: the auto rule regroups
        ctx.set_regroup(True)
        cf.set_sensed_points(pts)
        cf.set_point_weights(a)
        cf.set_free_split(split)
        before = ctx.permutation()
        assert np.array_equal(ctx.point_weights(), a[before])
        if loop == "lm":
            out[side] = _outcome(lambda: cf.descend_lm(q0, 6, LM["damping"], LM["max_step"], 0.0, n, prior_weight=1e-3,
                                                       device_loop="require" if side == "device" else False))
        else:
            try:
                ctx.set_solver("require" if side == "device" else False)
                out[side] = _outcome(lambda: cf.descend(q0, 6, 0.1, 0.5, 0.0, None, n))
            finally:
                ctx.set_solver(True)
        after = ctx.permutation()
        assert not np.array_equal(after, before), side  # (regrouped by the loop's first evaluation)
        assert np.array_equal(ctx.point_weights(), a[after]), side
        assert ctx.get_free_split() == split
        cf.set_robust_loops(False)
    assert out["host"][0] == "ok" and _same(out["host"], out["device"]), out


# ---- 5. edges -------------------------------------------------------------------------------------

def test_edges():
    from flash.robust import Huber, Tukey
    m, pts, _, q0 = _drift(3000)
    n = len(pts)
    # a weight of exactly 0 on a tenth of the points
    a = rng(913).uniform(0.25, 2.0, n)
    a[::10] = 0.0
    cf = _functor(m, pts, Huber(0.02), a)
    cf.value_and_gradient(q0)
    for pair in (_lm_pair(cf, q0, 6, 0.0, n, 1e-3), _naive_pair(cf, q0, 6, 0.0, n)):
        assert pair[0][0] == "ok" and _same(*pair), pair
    # iteration_limit = 1
    for pair in (_lm_pair(cf, q0, 1, 0.0, n, None), _naive_pair(cf, q0, 1, 0.0, n)):
        assert pair[0][0] == "ok" and _same(*pair), pair
    # free-space samples that all lie outside the model: their terms are zero
    far = pts[:500] + np.array([0.0, 0.0, 5.0])
    cf = _functor(m, np.concatenate([pts, far]), Huber(0.02), None, n)
    cf.value_and_gradient(q0)
    assert (cf.per_point(q0)[1][n:] > 0).all()  # (k*, d*, ∇d*: every sample's d* is positive)
    for pair in (_lm_pair(cf, q0, 6, 0.0, n + 500, None), _naive_pair(cf, q0, 6, 0.0, n + 500)):
        assert pair[0][0] == "ok" and _same(*pair), pair
    # Tukey with every point beyond the scale: all-zero rows, a degenerate factorisation in the step
    cf = _functor(m, pts + np.array([0.0, 0.0, 5.0]), Tukey(0.05))
    c, g, H = cf.value_gradient_hessian(q0)
    assert not g.any() and not H.any() and c > 0
    # (fsdf_lm_minimize: g = 0 is not below a tolerance of 0.0, so the step is tried. Without a
    # prior H = 0 and every factorisation is degenerate: the damping is raised past 1e12 with no
    # further evaluation and the loop ends after its first, at the start. With the prior H = 2 mu I
    # and g = 0: the step is zero, each trial repeats f, none is accepted, all six evaluations are made.)
    for mu, evaluations in ((None, 1), (1e-3, 6)):
        host, dev = _lm_pair(cf, q0, 6, 0.0, n, mu)
        assert host[0] == "ok" and _same(host, dev), (mu, host, dev)
        assert int(host[1][-2]) == evaluations and np.array_equal(host[1][:len(q0)], q0), (mu, host)
        assert host[1][-1] > LM["damping"]  # (raised, on both sides to the same value)
    pair = _naive_pair(cf, q0, 6, 0.0, n)
    assert pair[0][0] == "ok" and _same(*pair), pair
    cf.set_robust_loops(False)


# ---- 6. through the front end -----------------------------------------------------------------------

def test_estimate_state_on_a_depth_frame_with_free_space_a_grid_and_a_loss():
    """The pipeline for a real camera — DepthFrame with FreeSpace → VoxelGrid (its counts are point
    weights) → Huber → LevenbergMarquardt with a prior — on the device loop against the host loop."""
    import flash
    from flash import Models, VoxelGrid
    from flash.depthsensors import DepthFrame, FreeSpace, Kinect, raycast_depths
    from flash.geometry import Transform, angle_axis
    from flash.robust import Huber
    from flash.tracking import LevenbergMarquardt, estimate_state
    q_true = np.array([0.3, -0.2, 0.25, 0.1, -0.15, 0.2])
    x0 = q_true + np.array([0.08, -0.06, 0.07, 0.05, -0.04, 0.06])
    sensor = Kinect(96, 128)
    tf = Transform(angle_axis(np.pi / 2, [1, 0, 0]), np.array([0.0, 1.0, 0.45]))
    m = Models.irb140()
    state = flash.ManipulatorState(m)
    state.q[:] = q_true
    depth = raycast_depths(flash.skin(state), sensor, tf)
    frame = DepthFrame(depth, sensor, tf, free_space=FreeSpace(samples=2, stride=3))

    def run(device_loop, loops):
        s = LevenbergMarquardt(len(x0), damping=1e-3, max_step=0.5, iteration_limit=10,
                               gradient_convergence_tolerance=0.0, prior_weight=1e-3, device_loop=device_loop)
        x = estimate_state(Models.irb140(), frame, x0, solver=s, loss=Huber(0.02), voxel=VoxelGrid(0.03),
                           robust_loops=loops)
        return x, s.iterations, s.final_damping

    x_dev, its_dev, lam_dev = run("require", True)
    x_host, its_host, lam_host = run(False, False)
    assert np.array_equal(x_dev, x_host) and (its_dev, lam_dev) == (its_host, lam_host)
    # (the loops ran and moved: the comparison above is not of two untouched starts; how well a Huber
    # run recovers the joints is the next test's matter)
    assert its_host == 10 and not np.array_equal(x_host, x0)
    print(f"depth frame, free space, grid, Huber: err123 {np.abs(x0 - q_true)[:3].max():.4f} -> "
          f"{np.abs(x_host - q_true)[:3].max():.4f} in {its_host} evaluations")
    with pytest.raises(Exception) as e:  # (without the switch the required device loop is refused, as before)
        run("require", False)
    assert getattr(e.value, "status", None) == ERR_STATE


@pytest.mark.parametrize("seed", [41, 7, 19])
def test_estimate_state_with_huber_on_the_device_loop_recovers_the_observed_joints(seed):
    """tests/test_gpu_robust.py's drift cases with the Huber run on the device loop: the same bounds
    (Huber err123 <= 0.03 and <= half the least-squares run's, whose err123 >= 0.03)."""
    from flash.robust import Huber
    from flash.tracking import LevenbergMarquardt, estimate_state
    m, pts, q_true, q0 = _drift(3000, seed)

    def solver(device_loop):
        return LevenbergMarquardt(len(q0), damping=1e-3, max_step=0.5, iteration_limit=10,
                                  gradient_convergence_tolerance=0.0, prior_weight=1e-3, device_loop=device_loop)

    s_ls, s_host, s_dev = solver(False), solver(False), solver("require")
    x_ls = estimate_state(m, pts, q0, solver=s_ls)
    x_host = estimate_state(m, pts, q0, solver=s_host, loss=Huber(0.02))
    x_dev = estimate_state(m, pts, q0, solver=s_dev, loss=Huber(0.02), robust_loops=True)
    m.engine().set_robust_loops(False)
    assert s_dev.iterations == s_host.iterations == 10
    assert np.array_equal(x_dev, x_host) and s_dev.final_damping == s_host.final_damping
    e_ls, e_hub = (float(np.abs(x - q_true)[:3].max()) for x in (x_ls, x_dev))
    print(f"seed {seed}: err123 least squares {e_ls:.4f}, Huber 0.02 on the device loop {e_hub:.4f}")
    assert e_ls >= 0.03, e_ls  # (the negative control)
    assert e_hub <= 0.03, e_hub
    assert e_hub <= 0.5 * e_ls, (e_hub, e_ls)


# ---- 7. the switch ------------------------------------------------------------------------------------

def test_the_switch():
    from flash import Models
    from flash._lib import FlashNativeError
    from flash.gradientdescent import CostFunctor
    from flash.robust import Huber
    _, pts, _, q0 = _drift(3000)
    n = len(pts)

    def calls(cf):
        out = [cf.value_and_gradient(q0), cf.value_gradient_hessian(q0), cf.descend(q0, 4, 0.1, 0.5, 0.0, None, n),
               cf.descend_lm(q0, 4, 1e-3, 0.5, 0.0, n), cf.descend_lm(q0, 4, 1e-3, 0.5, 0.0, n, device_loop=True)]
        return [np.concatenate([np.ravel(np.asarray(v, np.float64)) for v in o]) for o in out]

    never = CostFunctor(Models.irb140(), pts, loss=Huber(0.02))
    assert never.ctx.get_robust_loops() is False  # (the default)
    never.value_and_gradient(q0)  # (the cloud's first pass and its regroup)
    want = calls(never)
    # off: the required modes are refused, as they were
    with pytest.raises(FlashNativeError) as e:
        never.descend_lm(q0, 6, 1e-3, 0.5, 0.0, n, device_loop="require")
    assert e.value.status == ERR_STATE and "loss" in str(e.value)
    try:
        never.ctx.set_solver("require")
        with pytest.raises(FlashNativeError) as e:
            never.descend(q0, 5, 0.1, 0.5, 0.0, None, n)
        assert e.value.status == ERR_STATE and "loss" in str(e.value)
    finally:
        never.ctx.set_solver(True)
    # on, used, and off again: every call gives the bits of the context that never had it on
    had = CostFunctor(Models.irb140(), pts, loss=Huber(0.02), robust_loops=True)
    assert had.ctx.get_robust_loops() is True
    had.value_and_gradient(q0)
    on = calls(had)
    had.descend_lm(q0, 3, 1e-3, 0.5, 0.0, n, device_loop="require")
    for a, b in zip(on, want):  # (on: the loops that may take the device give the host loop's bits)
        assert np.array_equal(a, b)
    had.set_robust_loops(False)
    assert had.ctx.get_robust_loops() is False
    for a, b in zip(calls(had), want):
        assert np.array_equal(a, b)
    with pytest.raises(FlashNativeError) as e:
        had.descend_lm(q0, 6, 1e-3, 0.5, 0.0, n, device_loop="require")
    assert e.value.status == ERR_STATE
    # values other than 0 / 1 are refused and leave the switch as it was
    had.ctx.set_robust_loops(True)
    assert had.ctx._lib.fsdf_set_robust_loops(had.ctx._ctx, 2) == 1 and had.ctx.get_robust_loops() is True
    assert had.ctx._lib.fsdf_set_robust_loops(had.ctx._ctx, -1) == 1 and had.ctx.get_robust_loops() is True
    had.ctx.set_robust_loops(False)


def test_a_scene_with_a_skin_keeps_the_host_loop():
    """With the switch on, a scene with an RBF skin under a robust objective is still refused by the
    required modes, with a reason that names skins; the other modes run the host loop."""
    from flash._lib import FlashNativeError
    from flash.gradientdescent import CostFunctor
    from flash.robust import Huber
    from test_gpu_solver_rbf import _scene
    m, pts, x0 = _scene("beanbag")
    n = float(len(pts))
    cf = CostFunctor(m, pts, loss=Huber(0.02), robust_skins=True, robust_loops=True)
    try:
        assert cf.ctx.get_robust_loops()
        cf.value_and_gradient(x0)
        cf.ctx.set_solver(False)
        want = cf.descend(x0, 4, 0.1, 0.5, 0.0, None, n)
        for mode in (True, "all"):
            cf.ctx.set_solver(mode)
            got = cf.descend(x0, 4, 0.1, 0.5, 0.0, None, n)
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
        for mode in ("require", "require-all"):
            cf.ctx.set_solver(mode)
            with pytest.raises(FlashNativeError) as e:
                cf.descend(x0, 4, 0.1, 0.5, 0.0, None, n)
            assert e.value.status == ERR_STATE and "skins" in str(e.value), str(e.value)
    finally:
        cf.ctx.set_solver(True)
        cf.ctx.set_loss(None)
        cf.ctx.set_robust_skins(False)
        cf.ctx.set_robust_loops(False)
