"""The resident order — Hilbert keys, bounding box, the sort by (key, caller
index), the keyed shard order and the regroup by nearest surface (csrc/sort.hip
and its callers in csrc/cloud.hip) — held to the numpy twins of curve_ref.py.
Every comparison is on integers or bits.

The library is built with -ffp-contract=off and without fast-math, so the
twin's fp64 subtraction, division and product are the device's."""
import numpy as np
import pytest

from conftest import rng
from curve_ref import box_of, cells_of, hilbert_decode, hilbert_encode, keys_of

pytestmark = pytest.mark.gpu

DYADIC = np.array([0.0, 0.0, 0.0, 1024.0, 1024.0, 1024.0])
TOP = 1 << 30


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _model(name):
    from flash import Models
    return {"irb140": Models.irb140, "arm_grid": Models.arm_grid}[name]()


def _spec(m):
    return [(s.hull.vertices, s.hull.faces, s.hull.planes) for s in m.convex_surfaces()]


def _sorted_perm(pts):
    """The whole cloud's resident order: by key in the cloud's own box, ties by caller index."""
    return np.argsort(keys_of(pts, box_of(pts)), kind="stable")


@pytest.fixture(scope="module")
def contexts():
    """Contexts by (model, precision, role), made once and reused: their
    buffers and scratch grow and shrink from case to case, as in a session."""
    from flash import _lib
    made = {}

    def get(model, precision=64, role="a", sort_points=True):
        key = (model, precision, role, sort_points)
        if key not in made:
            c = _lib.Context(device=0, precision=precision, sort_points=sort_points)
            if model:
                c.set_model(_spec(_model(model)))
            made[key] = c
        return made[key]

    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def scenes():
    """Per model: (poses a, poses b, the posed model's box grown by 0.1, the
    world centroid of every surface's vertices at poses a)."""
    import flash
    from flash import synthetic
    made = {}

    def get(name):
        if name not in made:
            m = _model(name)
            _, qe = synthetic.perturbed_configuration(m, 1201)
            pa, pb = flash.hull_poses(m, qe), flash.hull_poses(m, qe + 2e-3)
            world = [s.hull.vertices @ p[:9].reshape(3, 3).T + p[9:] for s, p in zip(m.convex_surfaces(), pa)]
            allv = np.concatenate(world)
            made[name] = (pa, pb, (allv.min(0) - 0.1, allv.max(0) + 0.1), np.stack([w.mean(0) for w in world]))
        return made[name]

    return get


def _box_cloud(scene, n, seed):
    lo, hi = scene[2]
    return rng(seed).uniform(lo, hi, size=(n, 3))


# ---- keys ---------------------------------------------------------------------

def _device_keys(ctx, pts, box):
    import torch
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = len(pts)
    d_pts = _dev(pts)
    d_keys = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    ctx.curve_keys_device(d_pts.data_ptr(), n, box, d_keys.data_ptr())
    return d_keys.cpu().numpy().view(np.uint32).astype(np.int64)


KEY_SIZES = [1, 255, 256, 257, 5000]


@pytest.mark.parametrize("n", KEY_SIZES)
def test_keys_at_cell_centres(contexts, n):
    """A point at the centre of cell hilbert_decode(h) of the dyadic box has
    key h: the first and the last 4,096 keys and random ones."""
    ctx = contexts(None, sort_points=False)
    i = np.arange(n)
    for h in (i % 4096, TOP - 1 - (i % 4096), rng(40 + n).integers(0, TOP, n)):
        got = _device_keys(ctx, hilbert_decode(h) + 0.5, DYADIC)
        assert np.array_equal(got, h), np.flatnonzero(got != h)[:10]


@pytest.mark.parametrize("n", KEY_SIZES)
def test_keys_follow_the_quantisation(contexts, n):
    """Device keys equal keys_of: points on cell boundaries of the dyadic box
    (p = c; c = 1024 = hi clamps to 1023), points outside it (u in [-2, 3]), a
    box that is no power of two, and boxes degenerate on one, two and three
    axes (also hi < lo)."""
    ctx = contexts(None, sort_points=False)
    r = rng(50 + n)
    # cell boundaries
    c = r.integers(0, 1025, size=(n, 3))
    c[0] = (1024, 0, 1024)
    got = _device_keys(ctx, c.astype(np.float64), DYADIC)
    assert np.array_equal(got, hilbert_encode(np.minimum(c, 1023)))
    assert np.array_equal(got, keys_of(c, DYADIC))
    # outside
    p = r.uniform(-2048.0, 3072.0, size=(n, 3))
    want = keys_of(p, DYADIC)
    assert np.array_equal(_device_keys(ctx, p, DYADIC), want)
    if n >= 255:
        cells = cells_of(p, DYADIC)
        assert (cells == 0).any() and (cells == 1023).any() and ((cells > 0) & (cells < 1023)).any()
    # a box that is no power of two; lo and hi themselves among the points
    lo, ext = np.array([-0.37, 1.6, 0.21]), np.array([1.3, 0.7, 2.9])
    box = np.concatenate([lo, lo + ext])
    p = lo + ext * r.uniform(-0.2, 1.2, size=(n, 3))
    p[0] = box[:3]
    p[-1] = box[3:]
    assert np.array_equal(_device_keys(ctx, p, box), keys_of(p, box))
    # degenerate axes: ext = 0 and ext < 0 give cell 0
    for axes in ((0,), (2,), (0, 1), (1, 2), (0, 1, 2)):
        for gap in (0.0, -0.5):
            b = box.copy()
            b[[3 + a for a in axes]] = b[list(axes)] + gap
            want = keys_of(p, b)
            assert np.array_equal(cells_of(p, b)[:, list(axes)], np.zeros((n, len(axes)), np.int64))
            assert np.array_equal(_device_keys(ctx, p, b), want), (axes, gap)


def test_keys_refuse_a_box_that_is_not_finite(contexts):
    from flash._lib import FlashNativeError
    ctx = contexts(None, sort_points=False)
    p = rng(60).uniform(size=(16, 3))
    for j in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            box = np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
            box[j] = bad
            with pytest.raises(FlashNativeError) as e:
                _device_keys(ctx, p, box)
            assert e.value.status == 1


# ---- bounding box -------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 65535, 65536, 65537, 65793])
def test_cloud_box(contexts, n):
    """fsdf_cloud_box_device equals the per-axis minimum and maximum exactly;
    above 65,536 points the 256 workgroups of 256 lanes grid-stride. Every
    axis's extreme at the first point, at the last and at index 65536."""
    ctx = contexts(None, sort_points=False)
    base = rng(70 + n).normal(size=(n, 3))
    assert not np.any((base == 0.0) & np.signbit(base))
    clouds = [base]
    for pos in (0, n - 1, 65536):
        if pos >= n:
            continue
        for extreme in (np.array([-50.0, -60.0, -70.0]), np.array([50.0, 60.0, 70.0])):
            p = base.copy()
            p[pos] = extreme
            clouds.append(p)
    for p in clouds:
        got = ctx.cloud_box_device(_dev(p).data_ptr(), n)
        assert np.array_equal(got, box_of(p)), (got, box_of(p))


def test_cloud_box_of_no_points(contexts):
    got = contexts(None, sort_points=False).cloud_box_device(0, 0)
    assert np.array_equal(got, [np.inf] * 3 + [-np.inf] * 3)


# ---- the sorted order ------------------------------------------------------------

def _clouds(n, seed):
    r = rng(seed)
    rand = r.normal(size=(n, 3)) * np.array([0.4, 0.7, 0.2]) + np.array([0.3, -0.1, 0.9])
    lattice = np.floor(r.uniform(0.0, 4.0, size=(n, 3))) * 0.25 + 0.125  # 64 distinct points: heavy ties
    planar = rand.copy()
    planar[:, 2] = 0.3
    one = np.tile(rand[:1], (n, 1))
    return {"random": rand, "lattice": lattice, "planar": planar, "one-point": one}


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000, 65537])
def test_sorted_order(contexts, precision, n):
    """fsdf_set_points of a sorting context: permutation() is the stable
    argsort of the twin's keys in the cloud's own box — by key, ties (whole
    lattice cells, a degenerate axis, one repeated point) by caller index."""
    ctx = contexts("irb140", precision)
    for name, pts in _clouds(n, 80 + n).items():
        ctx.set_points(pts)
        got = ctx.permutation()
        assert np.array_equal(got, _sorted_perm(pts)), name


@pytest.mark.parametrize("precision", [64, 32])
def test_points_move_with_their_indices(contexts, scenes, oracle_mod, precision):
    """Resident-order k*, d*, ∇d* equal the oracle's at the permutation: the
    gather moved each point with its index."""
    scene = scenes("irb140")
    om = oracle_mod.OracleModel.from_manipulator(_model("irb140"))
    ctx = contexts("irb140", precision)
    pts = _box_cloud(scene, 1000, 90)
    ctx.set_points(pts)
    perm = ctx.permutation()
    assert np.array_equal(perm, _sorted_perm(pts))
    ctx.set_output_order(True)
    try:
        _, _, (k, d, g) = ctx.eval(scene[0], per_point=True)
    finally:
        ctx.set_output_order(False)
    od, ok, og = om.skin(scene[0], pts[perm], precision=precision)
    assert np.array_equal(k, ok) and np.array_equal(d, od) and np.array_equal(g, og)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n", [257, 65537])
def test_sorted_order_of_a_prefetched_cloud(contexts, scenes, precision, n):
    """fsdf_prefetch_points + fsdf_set_points_prefetched: the same order, with
    the sort issued by the set call (no pass between) and behind a pass."""
    scene = scenes("irb140")
    ctx = contexts("irb140", precision)
    a, b = _clouds(n, 100 + n)["lattice"], _box_cloud(scene, n + 3, 101 + n)
    ctx.prefetch_points(a)
    ctx.set_points_prefetched()
    assert np.array_equal(ctx.permutation(), _sorted_perm(a))
    ctx.prefetch_points(b)
    ctx.eval(scene[0])  # (the prefetch is issued behind this pass, on the copy stream)
    assert np.array_equal(ctx.permutation(), _sorted_perm(a))
    ctx.set_points_prefetched()
    assert np.array_equal(ctx.permutation(), _sorted_perm(b))


@pytest.mark.parametrize("precision", [64, 32])
def test_sorted_order_of_a_depth_frame(contexts, precision):
    """A depth frame on a sorting context: the order of the frame's cloud
    (the numpy twin flash.depthsensors.depth_points gives its bits)."""
    from flash.depthsensors import Kinect, depth_points
    from flash.geometry import Transform, angle_axis
    ctx = contexts("irb140", precision)
    rays = Kinect(37, 53).rays
    r = rng(110)
    img = r.uniform(0.9, 2.5, size=(37, 53))
    img[r.uniform(size=img.shape) < 0.3] = np.nan
    tf = Transform(angle_axis(2.0, [1.0, 0.2, -0.1]), np.array([0.1, 1.6, 0.6]))
    pts, pix = depth_points(img, rays, tf, 0.8, 2.6, 1.0, "range")
    ctx.set_sensor(rays, "range")
    try:
        assert ctx.set_depth(img, tf, 0.8, 2.6, 1.0) == len(pts) > 1000
        assert np.array_equal(ctx.depth_pixels(), pix)
        assert np.array_equal(ctx.permutation(), _sorted_perm(pts))
    finally:
        ctx.set_sensor(None)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n", [65, 5000])
def test_range_is_a_slice_of_the_whole_order(contexts, precision, n):
    """fsdf_set_points_range(pts, b, e): permutation() == whole_perm[b:e]."""
    ctx = contexts("irb140", precision)
    for name, pts in _clouds(n, 120 + n).items():
        whole = _sorted_perm(pts)
        for b, e in ((0, n), (n // 3 + 1, n - 7), (n // 2, n // 2 + 1)):
            ctx.set_points_range(pts, b, e)
            assert np.array_equal(ctx.permutation(), whole[b:e]), (name, b, e)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("n", [1, 257, 5000])
def test_keyed_order(contexts, scenes, oracle_mod, precision, n):
    """fsdf_set_points_keyed_device, given the twin's keys and a shuffled
    slice of a larger cloud: the whole-cloud indices ordered by (key, index) —
    equal keys with distinct indices among them (lattice points) — and the
    points moved with them (outputs equal the oracle's at the permutation)."""
    scene = scenes("irb140")
    ctx = contexts("irb140", precision)
    r = rng(130 + n)
    lo, hi = scene[2]
    whole = _box_cloud(scene, 3 * n + 5, 131 + n)
    snap = r.uniform(size=len(whole)) < 0.5  # half the cloud on a 4 x 4 x 4 lattice of the box
    whole[snap] = lo + (hi - lo) * (np.floor(r.uniform(0.0, 4.0, size=(int(snap.sum()), 3))) * 0.25 + 0.125)
    keys = keys_of(whole, box_of(whole))
    idx = r.permutation(len(whole))[:n]
    d_pts, d_keys, d_idx = _dev(whole[idx]), _dev(keys[idx].astype(np.uint32).view(np.int32)), _dev(idx.astype(np.int64))
    ctx.set_points_keyed_device(d_pts.data_ptr(), d_keys.data_ptr(), d_idx.data_ptr(), n)
    want = idx[np.lexsort((idx, keys[idx]))]
    if n >= 257:
        assert len(np.unique(keys[idx])) < n  # (ties that the index breaks)
    perm = ctx.permutation()
    assert np.array_equal(perm, want)
    _, _, (k, d, g) = ctx.eval(scene[0], per_point=True)  # (a ranged cloud: resident order)
    od, ok, og = oracle_mod.OracleModel.from_manipulator(_model("irb140")).skin(scene[0], whole[perm],
                                                                                 precision=precision)
    assert np.array_equal(k, ok) and np.array_equal(d, od) and np.array_equal(g, og)


# ---- regroup ---------------------------------------------------------------------

def _regroup_against_twin(ctx, plain, pts, pa, pb, one_surface=False):
    """set_points, a pass at pa, the regroup: perm1 == perm0[stable argsort of
    the pass's resident-order k*]; then a pass at pb gives an unregrouped
    context's per-point bits at perm1."""
    ctx.set_points(pts)
    ctx.set_output_order(True)
    perm0 = ctx.permutation()
    _, _, (ka, _, _) = ctx.eval(pa, per_point=True)
    assert ka.min() >= 0 and ka.max() < 64
    if one_surface:
        assert np.all(ka == ka[0])
    ctx.regroup_points()
    perm1 = ctx.permutation()
    want = perm0[np.argsort(ka, kind="stable")]
    assert np.array_equal(perm1, want), np.flatnonzero(perm1 != want)[:10]
    plain.set_points(pts)
    plain.set_output_order(False)
    _, _, (kb, db, gb) = plain.eval(pb, per_point=True)  # caller order
    _, _, (k1, d1, g1) = ctx.eval(pb, per_point=True)
    ctx.set_output_order(False)
    assert np.array_equal(k1, kb[perm1]) and np.array_equal(d1, db[perm1]) and np.array_equal(g1, gb[perm1])
    return ka


# one window of 4,096 points and its ragged ends, a cloud under one wave, and
# a cloud whose 64 * ceil(n / 4096) counts cross a scan super-tile (16 x 1,024
# counts): n > 2^20
REGROUP_SIZES = [1, 63, 64, 65, 4095, 4096, 4097, 8193, (1 << 20) + 4101]


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("model", ["arm_grid", "irb140"])
@pytest.mark.parametrize("n", REGROUP_SIZES)
def test_regroup_matches_the_twin(contexts, scenes, model, precision, n):
    """fsdf_regroup_points is the stable counting sort of the resident cloud by
    the last pass's k*: 64 surfaces (arm_grid) and 7 (irb140: most of the 64
    groups empty), both precisions, uniform points in a box around the model.

    The seed bytes: every pass of a hull-only scene of <= 64 surfaces writes
    them through emit_chunk — the 4- and 2-way hull-partitioned tiers (their
    part 0), the planned pass and the one-wave grid alike — so whichever shape
    fsdf_get_partition names for n, the default path is the one under test."""
    scene = scenes(model)
    ctx, plain = contexts(model, precision), contexts(model, precision, "plain")
    assert ctx.get_partition(n)[2] in (4, 2, 0)
    ka = _regroup_against_twin(ctx, plain, _box_cloud(scene, n, 140 + n % 1000), scene[0], scene[1])
    if n >= 4095:  # (some hulls are nowhere the nearest: 48 to 56 groups of arm_grid, 6 of irb140)
        groups = len(np.unique(ka))
        assert groups > 32 if model == "arm_grid" else 1 < groups <= 7
    if n > 1 << 20:
        # the counts lie surface-major, [64][windows]: those past the first
        # super-tile are surface 63's from window 130 on, and only a surface
        # with points there shows a lost carry
        nwin = -(-n // 4096)
        first = 16 * 1024 - 63 * nwin
        assert 64 * nwin > 16 * 1024 and 0 < first < nwin
        if model == "arm_grid":
            assert np.count_nonzero(ka[first * 4096:] == 63) > 1000


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("model", ["arm_grid", "irb140"])
def test_regroup_on_the_one_wave_grid(contexts, scenes, model, precision):
    """The same at a small size with the hull-partitioned tiers and the planned
    pass switched off (fsdf_set_partition, fsdf_set_plan): the one-wave-per-chunk
    pass wrote the seed bytes."""
    from flash import _lib
    scene = scenes(model)
    ctx = _lib.Context(device=0, precision=precision, sort_points=True)
    try:
        ctx.set_model(_spec(_model(model)))
        ctx.set_plan(False)
        ctx.set_partition(0, 0)
        assert ctx.get_partition(4097)[2] == 0
        _regroup_against_twin(ctx, contexts(model, precision, "plain"), _box_cloud(scene, 4097, 150), scene[0],
                              scene[1])
    finally:
        ctx.close()


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("model", ["arm_grid", "irb140"])
def test_regroup_of_a_single_group(contexts, scenes, model, precision):
    """Every point nearest the same surface (a tight cluster at one hull's
    centroid): one group, the regroup leaves the order as it is."""
    scene = scenes(model)
    ctx, plain = contexts(model, precision), contexts(model, precision, "plain")
    j = 3
    pts = scene[3][j] + 1e-4 * rng(160).normal(size=(4097, 3))
    ka = _regroup_against_twin(ctx, plain, pts, scene[0], scene[1], one_surface=True)
    assert ka[0] == j


def test_regroup_refuses_65_surfaces():
    """More than 64 surfaces: no seed bytes, FSDF_ERR_STATE, the order stays."""
    from flash import _lib
    from flash._lib import FlashNativeError
    from test_gpu_shapes import _cloud, _poses, _random_hull
    r = rng(765)
    hulls = [_random_hull(r, int(r.integers(8, 40))) for _ in range(65)]
    poses = _poses(r, 65, spread=0.6)
    pts = _cloud(r, poses, 4097, spread=0.08)
    ctx = _lib.Context(device=0, sort_points=True)
    try:
        ctx.set_model(hulls)
        ctx.set_points(pts)
        perm0 = ctx.permutation()
        assert np.array_equal(perm0, _sorted_perm(pts))
        ctx.eval(poses)
        with pytest.raises(FlashNativeError) as e:
            ctx.regroup_points()
        assert e.value.status == 3
        assert ctx.regroup_auto() is False
        assert np.array_equal(ctx.permutation(), perm0)
    finally:
        ctx.close()


@pytest.mark.parametrize("precision", [64, 32])
def test_regroup_needs_a_pass_over_this_cloud(scenes, precision):
    """set_points(A), a pass, set_points(B): B's seed bytes are hints gathered
    from A's voxels (0xFF where none), not B's nearest surfaces. The regroup
    refuses (FSDF_ERR_STATE) and leaves the order; the next pass gives the bits
    of a context that never asked; after it the regroup follows the twin."""
    from flash import _lib
    from flash._lib import FlashNativeError
    scene = scenes("irb140")
    pa, pb = scene[0], scene[1]
    A, B = _box_cloud(scene, 5000, 170), _box_cloud(scene, 5003, 171)
    spec = _spec(_model("irb140"))
    ctx, never = (_lib.Context(device=0, precision=precision, sort_points=True) for _ in range(2))
    try:
        for c in (ctx, never):
            c.set_model(spec)
            c.set_output_order(True)
            c.set_points(A)
            c.eval(pa)
            c.set_points(B)
        perm0 = ctx.permutation()
        assert np.array_equal(perm0, _sorted_perm(B))
        assert ctx.regroup_auto() is False
        with pytest.raises(FlashNativeError) as e:
            ctx.regroup_points()
        assert e.value.status == 3
        assert np.array_equal(ctx.permutation(), perm0)
        c1, acc1, (k1, d1, g1) = ctx.eval(pb, per_point=True)
        c0, acc0, (k0, d0, g0) = never.eval(pb, per_point=True)
        assert c1 == c0 and np.array_equal(acc1, acc0)
        assert np.array_equal(k1, k0) and np.array_equal(d1, d0) and np.array_equal(g1, g0)
        ctx.regroup_points()  # a pass over B has run
        perm1 = ctx.permutation()
        assert np.array_equal(perm1, perm0[np.argsort(k1, kind="stable")])
        _, _, (k2, d2, g2) = ctx.eval(pa, per_point=True)
        _, _, (k3, d3, g3) = never.eval(pa, per_point=True)
        pos0 = np.empty(len(B), np.int64)
        pos0[perm0] = np.arange(len(B))
        at = pos0[perm1]  # regrouped position -> Hilbert position
        assert np.array_equal(k2, k3[at]) and np.array_equal(d2, d3[at]) and np.array_equal(g2, g3[at])
    finally:
        ctx.close()
        never.close()
