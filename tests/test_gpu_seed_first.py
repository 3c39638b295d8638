"""GPU: the seed-first path of scene_eval changes no bit.

A wave all of whose valid lanes carry a usable prior (PassOutputs::prior_in)
skips Phase A's candidate loop, evaluates the priors first and then culls ONCE
at wave level against the lanes' bests. Every case here runs seeded passes on a
warm context and compares cost, accumulator, k*, d* and ∇d* bit for bit with a
cold context's first (unseeded) pass at the same configuration: an unsorted
context given the warm context's resident cloud (pts[permutation()]), so that
chunks, pass shape and summation order are the same and only the seeds differ.
The pass shapes are forced through fsdf_set_plan / fsdf_set_partition, the
clouds are small.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, rng

pytestmark = pytest.mark.gpu

N_ODD = 4133  # 65 chunks: no multiple of 64 or 256, more than one workgroup
SIZES = (1, 63, 64, 65, N_ODD)
SHAPES = ("grid", "planned", "planned_regroup", "planned_range")


def _hulls(manip):
    return [(s.hull.vertices, s.hull.faces, s.hull.planes) for s in manip.convex_surfaces()]


def _shape(ctx, shape):
    if shape == "grid":  # one wave per chunk, pass_kernel
        ctx.set_plan(False)
        ctx.set_partition(0, 0)
    elif shape == "mixed":  # planned: a tenth of the chunks asked over 4 waves, a tenth over 2
        ctx.set_plan(True, 0.1, 0.1, 1 << 30)
    else:  # planned pass at every size: a quarter of the chunks asked over 4 waves, half over 2
        ctx.set_plan(True, 0.25, 0.5, 1 << 30)  # (clouds this small: the plan splits every chunk 4 ways)


@pytest.fixture
def make_ctx():
    from flash import _lib
    made = []

    def make(hulls, shape, precision=64, cull=True, sort_points=True):
        c = _lib.Context(device=0, precision=precision, cull=cull, sort_points=sort_points)
        c.set_model(hulls)
        _shape(c, shape)
        made.append(c)
        return c
    yield make
    for c in made:
        c.close()


@pytest.fixture(scope="module")
def m64_case(m64):
    """M64 cloud and a tracking sequence of poses (shared, read-only)."""
    import flash
    from flash import synthetic
    qt, qe = synthetic.perturbed_configuration(m64, 1301)
    pts = synthetic.depth_cloud(m64, qt, N_ODD + 41, seed=1302, order="shuffled")
    track = [flash.hull_poses(m64, qe + d) for d in (0.0, 2e-3, -3e-3)]
    stale = [flash.hull_poses(m64, qe + d) for d in (0.0, 0.3, 0.0)]
    return _hulls(m64), pts, track, stale


def _same(got, want):
    (c1, a1, (k1, d1, g1)), (c0, a0, (k0, d0, g0)) = got, want
    assert c1 == c0, (c1, c0)
    assert np.array_equal(a1, a0), np.abs(a1 - a0).max()
    assert np.array_equal(k1, k0), np.nonzero(k1 != k0)[0][:10]
    assert np.array_equal(d1, d0), np.abs(d1 - d0).max()
    assert np.array_equal(g1, g0), np.abs(g1 - g0).max()


def _warm_vs_cold(make_ctx, hulls, pts, poses, shape, precision=64, regroup_after=None, rng_=None, stats_out=None):
    """Passes at `poses` on one warm context (resident-order outputs) against a
    cold first pass each; returns the warm runs and the resident clouds used."""
    warm = make_ctx(hulls, shape, precision=precision)
    if rng_ is None:
        warm.set_points(pts)
    else:
        warm.set_points_range(pts, *rng_)
    warm.set_output_order(True)
    cold = make_ctx(hulls, shape, precision=precision, sort_points=False)
    runs, clouds = [], []
    for j, p in enumerate(poses):
        if stats_out is not None:
            warm.kernel_stats(True)
        got = warm.eval(p, per_point=True)
        if stats_out is not None:
            stats_out.append(warm.kernel_stats(False))
        assert warm.pass_kernel_name().startswith("planned_pass_kernel") == (shape != "grid" and precision == 64)
        resident = pts[warm.permutation()]
        cold.set_points(resident)  # a new cloud: no prior
        _same(got, cold.eval(p, per_point=True))
        runs.append(got)
        clouds.append(resident)
        if regroup_after == j:
            warm.regroup_points()
    return runs, clouds


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n", SIZES)
def test_seeded_passes_change_no_bits(m64_case, make_ctx, shape, n):
    """Tracking passes (every prior valid, nearly all right) on the one-wave
    grid, the planned pass (at these sizes the plan splits every chunk 4 ways:
    a lane's prior can lie outside its wave's part, and that wave falls back;
    test_seed_first_path_in_planned_pass mixes the chunk shapes), the same
    after fsdf_regroup_points and on a ranged cloud."""
    hulls, pts, track, _ = m64_case
    kw = {}
    if shape == "planned_regroup":
        kw["regroup_after"] = 0
    if shape == "planned_range":
        kw["rng_"] = (7, 7 + n)
        cloud = pts[: n + 41]
    else:
        cloud = pts[:n]
    _warm_vs_cold(make_ctx, hulls, cloud, track + track[:1], shape.split("_")[0], **kw)


@pytest.mark.parametrize("shape", ["grid", "planned"])
def test_stale_seeds(m64_case, make_ctx, oracle_mod, m64, shape):
    """q, then every joint + 0.3 rad (most priors wrong, the lane's ub loose),
    then back: each pass equals a cold pass; the first configuration also
    equals the oracle."""
    hulls, pts, _, stale = m64_case
    runs, clouds = _warm_vs_cold(make_ctx, hulls, pts[:N_ODD], stale, shape)
    changed = np.count_nonzero(runs[0][2][0] != runs[1][2][0])
    assert changed > N_ODD // 10, changed  # many priors of the second and third pass are wrong
    om = oracle_mod.OracleModel.from_manipulator(m64)
    od, ok, og = om.skin(stale[2], clouds[2])
    _, acc, (k, d, g) = runs[2]
    assert np.array_equal(k, ok) and np.array_equal(d, od) and np.array_equal(g, og)
    oacc = om.cost_accum(stale[2], clouds[2])
    assert np.allclose(acc, oacc, rtol=1e-9, atol=1e-9 * np.abs(oacc).max())


def test_ties_against_the_seed(make_ctx):
    """Two identical hulls A < B. Pass 1: A far away, every prior becomes B.
    Pass 2: both posed identically — every point ties, and k* must be A though
    the seed is B. Pass 3: A away again."""
    from flash import _lib
    r = rng(1311)
    hull = _lib.convex_hull(r.normal(size=(60, 3)) * np.array([0.2, 0.12, 0.08]))
    eye = [1.0, 0, 0, 0, 1, 0, 0, 0, 1]
    near, far = np.array(eye + [0.1, -0.2, 0.3]), np.array(eye + [40.0, 0.0, 0.0])
    poses = [np.stack([far, near]), np.stack([near, near]), np.stack([far, near])]
    pts = hull[0][r.integers(0, len(hull[0]), 1500)] * r.uniform(0.2, 1.6, (1500, 1)) + near[9:]
    pts += r.normal(size=pts.shape) * 0.01
    runs, _ = _warm_vs_cold(make_ctx, [hull, hull], pts, poses, "grid")
    assert (runs[0][2][0] == 1).all() and (runs[1][2][0] == 0).all() and (runs[2][2][0] == 1).all()


@pytest.mark.parametrize("shape", ["grid", "planned"])
def test_irb140(irb, make_ctx, oracle_mod, shape):
    """7 hulls: the box term of the best-first seed (K < kSeedBoxMaxHulls) is on
    the fallback path only."""
    import flash
    from flash import synthetic
    qt, qe = synthetic.perturbed_configuration(irb, 1321)
    pts = synthetic.depth_cloud(irb, qt, N_ODD, seed=1322, order="shuffled")
    poses = [flash.hull_poses(irb, qe + d) for d in (0.0, 2e-3, 0.3, 0.0)]
    runs, clouds = _warm_vs_cold(make_ctx, _hulls(irb), pts, poses, shape)
    om = oracle_mod.OracleModel.from_manipulator(irb)
    od, ok, og = om.skin(poses[1], clouds[1])
    _, acc, (k, d, g) = runs[1]
    assert np.array_equal(k, ok) and np.array_equal(d, od) and np.array_equal(g, og)
    oacc = om.cost_accum(poses[1], clouds[1])
    assert np.allclose(acc, oacc, rtol=1e-9, atol=1e-9 * np.abs(oacc).max())


def test_fp32_context(m64_case, make_ctx, oracle_mod, m64):
    """An f32 context of M64: seeded passes equal cold ones, and the fp32
    oracle bit for bit (as test_gpu_fp32_exact.py compares)."""
    hulls, pts, track, stale = m64_case
    poses = track + stale[1:]
    runs, clouds = _warm_vs_cold(make_ctx, hulls, pts[:N_ODD], poses, "grid", precision=32)
    od, ok, og = oracle_mod.OracleModel.from_manipulator(m64).skin(poses[1], clouds[1], precision=32)
    _, _, (k, d, g) = runs[1]
    assert np.array_equal(k, ok) and np.array_equal(d, od) and np.array_equal(g, og)


def test_cull_off_and_rbf_unchanged(m64_case, make_ctx):
    """cull=False and an RBF scene take no seeds: repeated passes still run and
    equal a fresh context's (and the culled result / the golden k*)."""
    from flash import Models, _lib
    from flash.core import ConvexGeometry
    hulls, pts, track, _ = m64_case
    cloud = pts[:N_ODD]
    culled = make_ctx(hulls, "grid", sort_points=False)
    culled.set_points(cloud)
    brute = make_ctx(hulls, "grid", cull=False, sort_points=False)
    brute.set_points(cloud)
    brute.kernel_stats(True)
    for p in track:
        want = culled.eval(p, per_point=True)
        culled.set_points(cloud)
        got = brute.eval(p, per_point=True)
        for x, y in zip(got[2], want[2]):
            assert np.array_equal(x, y)
    assert brute.kernel_stats(False)["seed_first_waves"] == 0
    z = np.load(os.path.join(GOLDEN, "c3_beanbag.npz"))
    surfaces = [("hull", (s.hull.vertices, s.hull.faces, s.hull.planes)) if isinstance(s, ConvexGeometry)
                else ("rbf", len(s.surface_points) + len(s.skeleton_points)) for s in Models.beanbag().surfaces]
    outs = []
    for _ in range(2):
        c = _lib.Context(device=0)
        try:
            c.set_surfaces(surfaces)
            c.set_points(z["points"])
            c.set_rbf_params(z["rbf_rows"])
            outs.append([c.eval(z["poses"], per_point=True) for _ in range(1 + len(outs))])
        finally:
            c.close()
    for run in outs[1]:
        _same(run, outs[0][0])
    assert np.array_equal(outs[0][0][2][0], z["kstar"])


def test_seed_first_path_is_taken(m64_case, make_ctx):
    """Work counters of the seeded passes over the regrouped M64 cloud (one-wave
    grid) against a cold pass over the same resident cloud: every wave takes the
    seed-first path, evaluations per wave do not rise, and the candidates left
    by the wave-level cull fall."""
    hulls, pts, track, _ = m64_case
    cloud = pts[:N_ODD]
    warm = make_ctx(hulls, "grid")
    warm.set_points(cloud)
    warm.eval(track[0])
    warm.regroup_points()
    resident = cloud[warm.permutation()]
    cold = make_ctx(hulls, "grid", sort_points=False)
    for p in track[1:]:
        warm.kernel_stats(True)
        warm.eval(p)
        sw = warm.kernel_stats(False)
        cold.set_points(resident)
        cold.kernel_stats(True)
        cold.eval(p)
        sc = cold.kernel_stats(False)
        print("seeded", sw, "\ncold  ", sc)
        waves = (N_ODD + 63) // 64
        assert sw["wave_iters"] == sc["wave_iters"] == waves
        assert sc["seed_first_waves"] == 0 and sw["seed_first_waves"] == waves
        assert sw["hull_evals"] <= sc["hull_evals"]
        assert sw["wave_candidates"] < sc["wave_candidates"]



def test_seed_first_path_in_planned_pass(m64, make_ctx):
    """A planned pass that mixes one-wave, 2-way and 4-way chunks needs a cloud
    of more chunks than a third of the device's idle wave slots (the plan splits
    chunks 4 ways while slots are free): 102,437 points, a tenth of the chunks
    asked 4-way and a tenth 2-way. Seeded passes equal cold ones bit for bit; the
    one-wave chunks take the seed-first path, and the waves of a split chunk
    whose part does not hold every lane's prior fall back — some waves, not
    all, are counted, so a silent fallback of the planned kernel would show."""
    import flash
    from flash import synthetic
    n = 102437
    qt, qe = synthetic.perturbed_configuration(m64, 1331)
    pts = synthetic.depth_cloud(m64, qt, n, seed=1332, order="shuffled")
    poses = [flash.hull_poses(m64, qe + d) for d in (0.0, 2e-3, -3e-3, 0.0)]
    stats = []
    _warm_vs_cold(make_ctx, _hulls(m64), pts, poses, "mixed", stats_out=stats)
    chunks = (n + 63) // 64
    for st in stats[2:]:  # (the first pass is unseeded, the second still runs the size tier's shape)
        print("planned seeded", st)
        assert chunks < st["wave_iters"] < 4 * chunks  # one-wave and split chunks
        assert 0 < st["seed_first_waves"] < st["wave_iters"]
