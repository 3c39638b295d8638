"""GPU: voxel-grid downsampling on the device (include/flashsdf.h "voxel grid";
csrc/voxel.hip) against its numpy twin flash.depthdata.voxel_downsample bit for
bit; everything downstream of the centroids identical to a context fed the
twin's centroids and counts; depth frames and free-space samples through the
grid; the switch off and the refusals; the objective the weighted centroids
approximate; and the grow-only buffers of one context through large and small
voxel frames. Every comparison is exact equality unless it says otherwise."""
import numpy as np
import pytest

from conftest import rng

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 3
CONFIGS = {"f64": (64, False), "f64-sorted": (64, True), "f32": (32, False), "f32-sorted": (32, True)}
# the empty cloud, one point, a wave boundary, a count-block boundary, several blocks with a ragged tail
SMALL = (0, 1, 63, 64, 65, 255, 256, 257, 1125)
ONE_VOXEL = 4097                 # the one-lane fold over a whole cloud
TWO_TILES = 262145 + 1031        # 1,029 count blocks of 256: a second tile of the head-flag scan
NEAR, FAR = 0.8, 2.6


def _hulls(m):
    return [(s.hull.vertices, s.hull.faces, s.hull.planes) for s in m.surfaces]


@pytest.fixture(scope="module")
def scenes(irb, m64):
    """name -> (hull specs, poses, a cloud of 4,097 points near the model)."""
    import flash
    from flash import synthetic
    out = {}
    for name, m, seed in (("irb140", irb, 21), ("m64", m64, 31)):
        q_true, q_eval = synthetic.perturbed_configuration(m, seed)
        out[name] = (_hulls(m), flash.hull_poses(m, q_eval), synthetic.depth_cloud(m, q_true, 4097, seed=seed + 1))
    return out


@pytest.fixture(scope="module")
def contexts(scenes):
    """(config, k) -> the k-th IRB140 context of that configuration, made once."""
    from flash import _lib
    made = {}

    def get(config, k=0):
        if (config, k) not in made:
            precision, sort = CONFIGS[config]
            c = _lib.Context(device=0, precision=precision, sort_points=sort)
            c.set_model(scenes["irb140"][0])
            made[(config, k)] = c
        return made[(config, k)]

    yield get
    for c in made.values():
        c.close()


def _status(call, status, names=()):
    from flash import _lib
    with pytest.raises(_lib.FlashNativeError) as e:
        call()
    assert e.value.status == status, e.value
    for word in names:
        assert word in str(e.value), e.value


def _cases():
    """(label, points, grid) over the sizes and the grids of the stage."""
    from flash import VoxelGrid
    out = []
    for n in SMALL:
        r = rng(100 + n)
        # every point its own voxel: a shuffled lattice of spacing 2 h, both signs of the cells
        lattice = np.stack(np.unravel_index(np.arange(n), (11, 11, 11)), axis=1) - 5.0
        out.append((f"own-{n}", (lattice * 0.02 + 0.003)[r.permutation(n)], VoxelGrid(0.01)))
        # about three points per cell, around a non-zero origin
        side = max(n / 3.0, 1.0) ** (1.0 / 3.0) * 0.05
        out.append((f"three-{n}", r.uniform(-side / 2, side / 2, size=(n, 3)) + [0.3, -0.2, 0.9],
                    VoxelGrid(0.05, (0.3, -0.2, 0.9))))
        # points exactly on cell faces, k h for k of both signs
        k = r.integers(-6, 7, size=(n, 3))
        out.append((f"faces-{n}", k * 0.1, VoxelGrid(0.1)))
        # negative cells only
        out.append((f"negative-{n}", -r.uniform(0.5, 0.9, size=(n, 3)), VoxelGrid(0.03, weights="unit")))
        # clamped cells: beyond 2^20 cells each way, and the overflow of x − o
        far = r.choice([-3e3, 2e3, 1e300, -1e300, 0.01], size=(n, 3))
        out.append((f"clamped-{n}", far + r.uniform(0, 1e-3, size=(n, 3)), VoxelGrid(1e-3)))
        # dropped points: the first, the last, every other one
        for where in ("first", "last", "alternating"):
            p = r.uniform(-0.2, 0.2, size=(n, 3))
            sel = {"first": slice(0, 1), "last": slice(max(n - 1, 0), n), "alternating": slice(0, n, 2)}[where]
            p[sel, r.integers(0, 3)] = (np.nan, np.inf, -np.inf)[n % 3]
            out.append((f"dropped-{where}-{n}", p, VoxelGrid(0.04)))
    r = rng(7)
    out.append(("one-voxel", r.uniform(0.0, 0.999, size=(ONE_VOXEL, 3)) + [3.0, -2.0, 1.0], VoxelGrid(1.0)))
    p = r.uniform(-1.0, 1.0, size=(TWO_TILES, 3)) * [1.0, 0.7, 0.4]
    p[r.integers(0, TWO_TILES, size=500)] = np.nan
    out.append(("two-tiles", p, VoxelGrid(0.02)))
    return out


@pytest.fixture(scope="module")
def cases():
    """The cases with the twin's outputs, computed once."""
    from flash.depthdata import voxel_downsample
    return [(label, pts, grid, voxel_downsample(pts, grid)) for label, pts, grid in _cases()]


def _check_voxels(ctx, pts, grid, twin, label):
    xyz, count, cell, first, vop, dropped = twin
    m = len(xyz)
    assert ctx.n == m == ctx._num_points(), label
    gx, gc, gcell, n_in, gdrop = ctx.get_voxels()
    assert (n_in, gdrop) == (len(pts), dropped), label
    assert np.array_equal(gx.view(np.uint64), xyz.view(np.uint64)), label
    assert np.array_equal(gc, count) and np.array_equal(gcell, cell), label
    assert np.array_equal(ctx.get_voxel_of_point(), vop), label
    w = ctx.point_weights()
    if grid.weights == "count" and m > 0:
        assert np.array_equal(w, count.astype(np.float64)[ctx.permutation()]), label
    else:
        assert w is None, label


@pytest.mark.parametrize("config", list(CONFIGS))
def test_bits_against_the_twin(contexts, cases, config):
    import torch
    ctx = contexts(config)
    seen = set()
    for label, pts, grid, twin in cases:
        ctx.set_voxel_grid(grid)
        assert ctx.get_voxel_grid() == (grid.size, grid.origin, grid.mode)
        assert ctx.set_points_voxel(pts) == len(twin[0]), label
        _check_voxels(ctx, pts, grid, twin, label + " (host)")
        t = torch.from_numpy(np.ascontiguousarray(pts)).to("cuda:0")
        torch.cuda.synchronize()
        ctx.set_points(np.zeros((3, 3)))  # (another cloud in between: nothing of the host run is left to pass for it)
        assert ctx.set_points_voxel_device(t.data_ptr() if len(pts) else 0, len(pts)) == len(twin[0]), label
        _check_voxels(ctx, pts, grid, twin, label + " (device)")
        seen.add((label.split("-")[0], len(pts), len(twin[0]), twin[5], int(twin[1].max()) if len(twin[1]) else 0))
    # what the cases are there for: (kind, n, m, dropped, largest cell)
    assert all(("own", n, n, 0, min(n, 1)) in seen for n in SMALL)
    assert ("one", ONE_VOXEL, 1, 0, ONE_VOXEL) in seen
    assert any(k == "two" and n == TWO_TILES and m > 1024 * 256 // 3 and d > 0 for k, n, m, d, _ in seen)
    assert any(k == "three" and n == 1125 and 2 <= big and m < n for k, n, m, _, big in seen)
    assert any(k == "clamped" and 0 < m < n for k, n, m, _, _ in seen)
    assert any(k == "dropped" and d == (n + 1) // 2 and n > 1 for k, n, _, d, _ in seen)
    ctx.set_voxel_grid(None)


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("scene", ["irb140", "m64"])
def test_everything_downstream_is_identical(scenes, scene, config):
    """A context fed set_points_voxel(P) against one fed set_points(twin xyz) and
    set_point_weights(twin count): permutation, k*, d*, ∇d*, the robust rows."""
    from flash import VoxelGrid, _lib
    from flash.depthdata import voxel_downsample
    from flash.robust import Huber
    specs, poses, pts = scenes[scene]
    precision, sort = CONFIGS[config]
    # (about two points per cell on either cloud: IRB140's 4,097 points span 1 m, M64's 4 m)
    grid = VoxelGrid({"irb140": 0.03, "m64": 0.08}[scene], (0.01, -0.02, 0.005))
    xyz, count, *_ = voxel_downsample(pts, grid)
    assert len(pts) / 8 < len(xyz) < len(pts) / 1.5 and count.max() > 2
    a, b = (_lib.Context(device=0, precision=precision, sort_points=sort) for _ in range(2))
    try:
        for c in (a, b):
            c.set_model(specs)
        a.set_voxel_grid(grid)
        a.set_points_voxel(pts)
        b.set_points(xyz)
        b.set_point_weights(count.astype(np.float64))
        assert np.array_equal(a.permutation(), b.permutation())
        ra, rb = a.eval(poses, per_point=True), b.eval(poses, per_point=True)
        assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1])
        assert all(np.array_equal(u, v) for u, v in zip(ra[2], rb[2]))
        for loss in (None, Huber(0.02)):
            for c in (a, b):
                c.set_loss(loss)
            ua, ub = a.eval_robust(poses), b.eval_robust(poses)
            assert ua[0] == ub[0] and all(np.array_equal(u, v) for u, v in zip(ua[1:], ub[1:]))
        assert np.array_equal(a.point_weights(), b.point_weights())
    finally:
        a.close()
        b.close()


# ---- depth frames -------------------------------------------------------------------------------

def _image(fmt, shape, pattern):
    n = shape[0] * shape[1]
    r = rng(13 * n + len(pattern))
    valid = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "random": r.uniform(size=n) < 0.6}[pattern]
    if fmt == np.uint16:
        img = r.integers(int(NEAR * 1000) + 1, int(FAR * 1000), size=n).astype(np.uint16)
        bad, scale = np.array([0, 100, 2601, 65535], np.uint16), 0.001
    else:
        img = r.uniform(NEAR * 1.01, FAR * 0.99, size=n).astype(fmt)
        bad, scale = np.array([np.nan, 0.0, -1.5, np.inf, 0.5 * NEAR, 2.0 * FAR], fmt), 1.0
    img[~valid] = bad[np.arange((~valid).sum()) % len(bad)]
    return img.reshape(shape), scale


def _tform():
    from flash.geometry import Transform, angle_axis
    return Transform(angle_axis(2.0, [1.0, 0.2, -0.1]), np.array([0.1, 1.6, 0.6]))


def _same_pass(a, b, poses):
    ra, rb = a.eval(poses, per_point=True), b.eval(poses, per_point=True)
    assert ra[0] == rb[0] and np.array_equal(ra[1], rb[1])
    assert all(np.array_equal(u, v) for u, v in zip(ra[2], rb[2]))
    assert np.array_equal(a.permutation(), b.permutation())


@pytest.mark.parametrize("config", ["f64", "f64-sorted", "f32-sorted"])
@pytest.mark.parametrize("shape", [(1, 1), (5, 13), (37, 53), (120, 160)], ids=lambda s: "%dx%d" % s)
def test_depth_frames_through_the_grid(contexts, scenes, shape, config):
    """set_depth_{f64, f32, u16} with a grid equals set_points_voxel of
    depth_points' output; with free space on it equals the twin's centroids
    followed by the twin's samples, with split m, weights [count..., 1...] and
    the pixel list of the voxels' first points."""
    from flash import VoxelGrid
    from flash.depthdata import voxel_downsample
    from flash.depthsensors import DepthFrame, DepthSensor, FreeSpace, Kinect, depth_points
    from flash.robust import Huber
    a, b = contexts(config, 0), contexts(config, 1)
    poses = scenes["irb140"][1]
    rays = Kinect(*shape).rays if shape != (1, 1) else np.array([[[0.1, -0.2, 1.0]]])
    tf = _tform()
    grid = VoxelGrid(0.12, (0.0, 0.05, 0.0))
    a.set_sensor(rays, "range")
    thinned = False
    for fmt in (np.float64, np.float32, np.uint16):
        for pattern in ("all", "none", "random"):
            img, scale = _image(fmt, shape, pattern)
            pts, pix = depth_points(img, rays, tf, NEAR, FAR, scale)
            twin = voxel_downsample(pts, grid)
            a.set_free_space(None)
            a.set_voxel_grid(grid)
            b.set_voxel_grid(grid)
            assert a.set_depth(img, tf, NEAR, FAR, scale) == len(twin[0])
            b.set_points_voxel(pts)
            _check_voxels(a, pts, grid, twin, f"{fmt.__name__} {pattern}")
            assert np.array_equal(a.depth_pixels(), pix[twin[3]])
            assert a.get_free_split() is None
            _same_pass(a, b, poses)
            assert (a.point_weights() is None and len(twin[0]) == 0) or \
                np.array_equal(a.point_weights(), b.point_weights())
            thinned |= 0 < len(twin[0]) < len(pts)
            for J in (1, 2):
                fs = FreeSpace(J, 2, 0.02, 0.05, 1.2)
                frame = DepthFrame(img, DepthSensor(rays), tf, NEAR, FAR, scale, free_space=fs)
                vp, vpix, vw = frame.voxel_points(grid)
                m = len(twin[0])
                a.set_free_space(fs)
                assert a.set_depth(img, tf, NEAR, FAR, scale) == len(vp)
                vox = a.get_voxels()
                assert np.array_equal(vox[0], twin[0]) and np.array_equal(vox[1], twin[1])
                assert vox[3:] == (len(pts), 0)
                assert np.array_equal(a.depth_pixels(), vpix)
                assert a.get_free_split() == (m if m < len(vp) else None)
                b.set_points(vp)
                b.set_free_split(m)
                if len(vp):
                    b.set_point_weights(vw)
                    assert np.array_equal(a.point_weights(), vw[a.permutation()])
                _same_pass(a, b, poses)
                if len(vp):
                    for c in (a, b):
                        c.set_loss(Huber(0.02) if J == 2 else None)
                    ua, ub = a.eval_robust(poses), b.eval_robust(poses)
                    assert ua[0] == ub[0] and all(np.array_equal(u, v) for u, v in zip(ua[1:], ub[1:]))
                    for c in (a, b):
                        c.set_loss(None)
    assert thinned or shape == (1, 1)
    for c in (a, b):
        c.set_free_space(None)
        c.set_voxel_grid(None)


# ---- the switch off, refusals, life cycle ----------------------------------------------------------

def test_switched_off_and_refusals(contexts, scenes):
    from flash import VoxelGrid
    from flash.depthsensors import Kinect
    a, b = contexts("f64-sorted", 0), contexts("f64-sorted", 1)   # (b never hears of the grid here)
    b.set_voxel_grid(None)
    poses, pts = scenes["irb140"][1], scenes["irb140"][2][:900]
    shape = (37, 53)
    rays = Kinect(*shape).rays
    img, scale = _image(np.float32, shape, "random")
    for c in (a, b):
        c.set_sensor(rays, "range")
        c.set_free_space(None)
    # a grid set and turned off again: a depth frame and set_points as before
    a.set_voxel_grid(VoxelGrid(0.1))
    a.set_voxel_grid(None)
    assert a.get_voxel_grid() is None
    assert a.set_depth(img, _tform(), NEAR, FAR, scale) == b.set_depth(img, _tform(), NEAR, FAR, scale)
    assert np.array_equal(a.depth_pixels(), b.depth_pixels())
    _same_pass(a, b, poses)
    assert a.point_weights() is None
    _status(a.get_voxels, ERR_STATE, ("voxel grid",))
    _status(a.get_voxel_of_point, ERR_STATE, ("voxel grid",))
    _status(lambda: a.set_points_voxel(pts), ERR_STATE, ("voxel grid", "fsdf_set_voxel_grid"))
    assert a._num_points() == b._num_points()  # (refused: the resident cloud stays)
    # with a grid set, plain set_points ignores it
    a.set_voxel_grid(VoxelGrid(0.1))
    a.set_points(pts)
    b.set_points(pts)
    _same_pass(a, b, poses)
    _status(a.get_voxels, ERR_STATE, ("voxel grid",))
    # bad arguments: FSDF_ERR_ARG, and the earlier setting stays
    lib, h = a._lib, a._ctx
    keep = a.get_voxel_grid()
    origin = np.zeros(3)
    for size in (-0.1, np.nan, np.inf, -np.inf):
        assert lib.fsdf_set_voxel_grid(h, size, None, 1) == ERR_ARG
    for bad in (np.array([np.nan, 0.0, 0.0]), np.array([0.0, np.inf, 0.0])):
        assert lib.fsdf_set_voxel_grid(h, 0.1, bad.ctypes.data, 1) == ERR_ARG
    for mode in (-1, 2, 7):
        assert lib.fsdf_set_voxel_grid(h, 0.2, origin.ctypes.data, mode) == ERR_ARG
    assert a.get_voxel_grid() == keep == (0.1, (0.0, 0.0, 0.0), 1)
    assert lib.fsdf_set_points_voxel(h, None, 5) == ERR_ARG and lib.fsdf_set_points_voxel(h, None, -1) == ERR_ARG
    assert a._num_points() == len(pts)
    # by reference, as the Julia binding passes it
    import ctypes
    size = ctypes.c_double(0.25)
    assert lib.fsdf_set_voxel_grid_ref(h, ctypes.byref(size), None, 0) == 0
    assert a.get_voxel_grid() == (0.25, (0.0, 0.0, 0.0), 0)
    assert lib.fsdf_set_voxel_grid_ref(h, None, None, 0) == 0 and a.get_voxel_grid() is None
    # a voxel cloud, then a plain one: the lists end
    a.set_voxel_grid(VoxelGrid(0.1))
    m = a.set_points_voxel(pts)
    assert 0 < m < len(pts) and a.voxel_sizes() == (m, len(pts), 0)
    a.set_points(pts[:10])
    _status(a.get_voxels, ERR_STATE, ("voxel grid",))
    assert a.point_weights() is None
    # the caller's weights replace the counts
    a.set_points_voxel(pts)
    w = rng(3).uniform(0.5, 1.5, size=m)
    a.set_point_weights(w)
    assert np.array_equal(a.point_weights(), w[a.permutation()])
    assert np.array_equal(a.get_voxels()[1].sum(), len(pts))  # (the lists stay)
    a.set_voxel_grid(None)


# ---- the objective it approximates --------------------------------------------------------------------

def _close(u, v):
    """The project's bar for sums that differ only in their order: 1e-9 relative, entries below 1
    against 1 (tests/test_gpu_buffer_reuse.py test_regroup_after_reuse)."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    return bool(np.all(np.abs(u - v) <= 1e-9 * np.maximum(np.abs(v), 1.0)))


@pytest.fixture(scope="module")
def doubled(scenes):
    """Distinct points, each present once or twice ((p + p) / 2 == p exactly), shuffled; and a grid so
    fine that only duplicates share a cell, its 2^20 cells each way still covering the cloud."""
    from flash import VoxelGrid
    from flash.depthdata import voxel_downsample
    base = scenes["irb140"][2][:1500]
    full = np.concatenate([base, base[::2]])[rng(17).permutation(2250)]
    grid = VoxelGrid(2e-6, tuple(base.mean(axis=0)))
    xyz, count, *_ = voxel_downsample(full, grid)
    assert len(xyz) == 1500 and sorted(set(count.tolist())) == [1, 2] and np.abs(base - base.mean(axis=0)).max() < 2.0
    assert set(map(tuple, xyz)) == set(map(tuple, base))  # (the centroids are the distinct points, bit for bit)
    return full, grid


@pytest.mark.parametrize("sort_points", [False, True])
def test_count_weights_give_the_full_clouds_objective(scenes, doubled, sort_points):
    from flash import _lib
    from flash.robust import Huber, Tukey
    specs, poses, _ = scenes["irb140"]
    full, grid = doubled
    a, b = (_lib.Context(device=0, sort_points=sort_points) for _ in range(2))
    try:
        for c in (a, b):
            c.set_model(specs)
        a.set_voxel_grid(grid)
        assert a.set_points_voxel(full) == 1500
        b.set_points(full)
        for loss in (None, Huber(0.02), Tukey(0.05)):
            for c in (a, b):
                c.set_loss(loss)
            (ca, acc_a, mom_a, w_a), (cb, acc_b, mom_b, w_b) = a.eval_robust(poses), b.eval_robust(poses)
            assert cb > 0 and abs(ca - cb) <= 1e-9 * cb, (loss, ca, cb)
            assert _close(acc_a, acc_b), (loss, np.abs(acc_a - acc_b).max())
            assert _close(mom_a.ravel(), mom_b.ravel()) and _close(w_a, w_b)
    finally:
        a.close()
        b.close()


def test_count_weights_through_value_gradient_hessian(irb, doubled):
    from flash.gradientdescent import CostFunctor
    from flash.robust import Huber, Tukey
    full, grid = doubled
    x = 0.1 * np.arange(irb.mechanism.num_positions) - 0.2
    for loss in (None, Huber(0.02), Tukey(0.05)):
        fv = CostFunctor(irb, full, loss=loss, voxel=grid)
        assert fv.n_points == 1500 and fv.n_divisor == len(full)
        cv, gv, Hv = fv.value_gradient_hessian(x)
        ff = CostFunctor(irb, full, loss=loss)
        cf, gf, Hf = ff.value_gradient_hessian(x)
        assert cf > 0 and abs(cv - cf) <= 1e-9 * cf
        assert np.all(np.abs(gv - gf) <= 1e-9 * np.abs(gf).max())
        assert np.all(np.abs(Hv - Hf) <= 1e-9 * np.abs(Hf).max())


# ---- buffer reuse --------------------------------------------------------------------------------------

def test_buffers_through_large_and_small_voxel_frames(scenes):
    """One context: a large voxel frame, a small one, a plain cloud, a large one again; after each,
    what a fresh context gives."""
    from flash import VoxelGrid, _lib
    from flash.depthsensors import FreeSpace, Kinect
    specs, poses, pts = scenes["irb140"]
    grid = VoxelGrid(0.1)

    def fresh():
        c = _lib.Context(device=0, sort_points=True)
        c.set_model(specs)
        return c

    def frame(shape, fs):
        rays = Kinect(*shape).rays
        img, scale = _image(np.uint16, shape, "random")

        def load(c):
            c.set_sensor(rays, "range")
            c.set_free_space(fs)
            c.set_voxel_grid(grid)
            c.set_depth(img, _tform(), NEAR, FAR, scale)
        return load

    def voxel_cloud(p):
        def load(c):
            c.set_voxel_grid(grid)
            c.set_points_voxel(p)
        return load

    steps = [(frame((120, 160), FreeSpace(2, 3, 0.02, 0.05, 1.2)), True),
             (frame((5, 13), None), True),
             (voxel_cloud(pts[:70]), True),
             (lambda c: c.set_points(pts[:333]), False),
             (voxel_cloud(pts), True),
             (frame((120, 160), FreeSpace(1, 2, 0.02, 0.05, 0.0)), True)]
    ctx = fresh()
    try:
        for load, voxel in steps:
            load(ctx)
            ref = fresh()
            try:
                load(ref)
                assert ctx.n == ref.n
                _same_pass(ctx, ref, poses)
                wa, wb = ctx.point_weights(), ref.point_weights()
                assert (wa is None and wb is None) or np.array_equal(wa, wb)
                assert ctx.get_free_split() == ref.get_free_split()
                if voxel:
                    for u, v in zip(ctx.get_voxels(), ref.get_voxels()):
                        assert np.array_equal(u, v)
                    assert np.array_equal(ctx.get_voxel_of_point(), ref.get_voxel_of_point())
                else:
                    _status(ctx.get_voxels, ERR_STATE)
            finally:
                ref.close()
    finally:
        ctx.close()
