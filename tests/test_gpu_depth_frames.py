"""Depth-frame ingest on the device (fsdf_set_sensor, fsdf_set_depth_*,
fsdf_get_depth_pixels; csrc/depth.hip) against its numpy twin
flash.depthsensors.depth_points: the same pixels and, through a pass, the same
bits as a context fed the twin's points — identical input bits and identical
caller order make everything downstream identical."""
import numpy as np
import pytest

from conftest import rng

pytestmark = pytest.mark.gpu

# where compaction can go wrong: one pixel, under a wave, one wave exactly, a
# second wave of one pixel, one workgroup exactly, a second workgroup of one
# pixel, several workgroups with a ragged tail, more blocks (1,200) than one
# scan tile (1,024)
SHAPES = [(1, 1), (1, 63), (8, 8), (5, 13), (16, 16), (1, 257), (37, 53), (480, 640)]
CONFIGS = {"f64": (64, False), "f64-sorted": (64, True), "f32-sorted": (32, True)}
PATTERNS = ("all", "none", "first", "last", "alternating", "random", "runs")
NEAR, FAR = 0.8, 2.6


def _mask(pattern, n):
    i = np.arange(n)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "first":
        return i == 0
    if pattern == "last":
        return i == n - 1
    if pattern == "alternating":
        return i % 2 == 0
    if pattern == "random":
        return rng(n).uniform(size=n) < 0.5
    # valid runs that start and stop exactly at multiples of 64 and of 256
    return ((i // 64) % 3 == 1) | ((i // 256) % 2 == 1)


def _image(fmt, shape, pattern):
    """(image, scale): valid pixels inside [NEAR, FAR] after the scale, the
    others cycling through every way of being invalid."""
    n = shape[0] * shape[1]
    valid = _mask(pattern, n)
    r = rng(7 * n + len(pattern))
    if fmt == np.uint16:
        img = r.integers(int(NEAR * 1000) + 1, int(FAR * 1000), size=n).astype(np.uint16)
        bad = np.array([0, 100, 799, 2601, 65535], np.uint16)
        scale = 0.001
    else:
        img = r.uniform(NEAR * 1.01, FAR * 0.99, size=n).astype(fmt)
        bad = np.array([np.nan, 0.0, -1.5, np.inf, -np.inf, 0.5 * NEAR, 2.0 * FAR], fmt)
        scale = 1.0
    img[~valid] = bad[np.arange((~valid).sum()) % len(bad)]
    return img.reshape(shape), scale


@pytest.fixture(scope="module")
def scene(irb):
    import flash
    q = 0.1 * np.arange(irb.mechanism.num_positions)
    hulls = [(s.hull.vertices, s.hull.faces, s.hull.planes) for s in irb.surfaces]
    return hulls, flash.hull_poses(irb, q)


@pytest.fixture(scope="module")
def contexts(scene):
    """Per configuration a pair: one fed depth frames, one fed the twin's points."""
    from flash import _lib
    made = {}

    def get(name):
        if name not in made:
            precision, sort = CONFIGS[name]
            pair = []
            for _ in range(2):
                c = _lib.Context(device=0, precision=precision, sort_points=sort)
                c.set_model(scene[0])
                pair.append(c)
            made[name] = pair
        return made[name]

    yield get
    for pair in made.values():
        for c in pair:
            c.close()


def _tform():
    from flash.geometry import Transform, angle_axis
    return Transform(angle_axis(2.0, [1.0, 0.2, -0.1]), np.array([0.1, 1.6, 0.6]))


def _same_pass(a, b, poses):
    ca, acc_a, (ka, da, ga) = a.eval(poses, per_point=True)
    cb, acc_b, (kb, db, gb) = b.eval(poses, per_point=True)
    assert np.array_equal(ka, kb) and np.array_equal(da, db) and np.array_equal(ga, gb)
    assert np.array_equal(acc_a, acc_b) and ca == cb
    return ca


def _check_frame(a, b, poses, img, rays, tf, kind, scale, near=NEAR, far=FAR):
    from flash.depthsensors import depth_points
    pts, pix = depth_points(img, rays, tf, near, far, scale, kind)
    n = a.set_depth(img, tf, near, far, scale)
    assert n == len(pix) == a.n
    got = a.depth_pixels()
    assert got.dtype == np.int32 and np.array_equal(got, pix)
    b.set_points(pts)
    cost = _same_pass(a, b, poses)
    if n == 0:
        assert cost == 0.0
    return pts, pix


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_bit_parity_with_the_twin(contexts, scene, shape, config):
    from flash.depthsensors import Kinect
    a, b = contexts(config)
    rays = Kinect(*shape).rays if shape != (1, 1) else np.array([[[0.1, -0.2, 1.0]]])
    tf = _tform()
    for kind in ("range", "z"):
        a.set_sensor(rays, kind)
        assert a.sensor() == (shape[0], shape[1], kind)
        for fmt in (np.float64, np.float32, np.uint16):
            for pattern in PATTERNS:
                img, scale = _image(fmt, shape, pattern)
                _, pix = _check_frame(a, b, scene[1], img, rays, tf, kind, scale)
                assert np.array_equal(pix, np.flatnonzero(_mask(pattern, img.size)))


def test_identity_pose_and_default_range(contexts, scene):
    """pose and range NULL: the identity and {0, +inf, 1}."""
    from flash import _lib
    from flash.depthsensors import Kinect, depth_points
    a, b = contexts("f64-sorted")
    rays = Kinect(9, 14).rays
    img, _ = _image(np.float64, (9, 14), "random")
    a.set_sensor(rays, "range")
    pts, pix = depth_points(img, rays, None)
    _lib.check(a._lib.fsdf_set_depth_f64(a._ctx, _lib.ptr(img), None, None), a._ctx, "set_depth_f64")
    a.n = a._num_points()
    assert np.array_equal(a.depth_pixels(), pix)
    b.set_points(pts)
    _same_pass(a, b, scene[1])


def test_raycast_loop(irb):
    """IRB140 seen by Kinect(41, 41) (tests/test_gpu_depth.py's pose): the
    raycast depths go straight back in as a frame, and tracking from the frame
    returns the bits of tracking from its points."""
    import flash
    from flash.depthsensors import DepthFrame, Kinect, raycast_depths
    from flash.geometry import Transform, angle_axis
    from flash.tracking import LevenbergMarquardt, estimate_state
    sensor = Kinect(41, 41)
    tf = Transform(angle_axis(np.pi / 2, [1, 0, 0]), np.array([0.0, 1.5, 0.5]))
    state = flash.ManipulatorState(irb)
    d = raycast_depths(flash.skin(state), sensor, tf)
    frame = DepthFrame(d, sensor, tf)
    ctx = irb.engine()
    ctx.set_sensor(sensor.rays, "range")
    assert ctx.set_depth(d, tf) == (~np.isnan(d)).sum() > 50
    assert np.array_equal(ctx.depth_pixels(), np.flatnonzero(~np.isnan(d).ravel()))
    pts, pix = frame.points()
    assert np.array_equal(pix, ctx.depth_pixels())
    assert np.abs(flash.skin(state)(pts)).max() < 1e-2  # (the hits lie on the skin)
    x0 = state.q + 0.05 * np.cos(np.arange(len(state.q)))
    n = flash.num_states(irb)
    for make in (lambda: None, lambda: LevenbergMarquardt(n, iteration_limit=4)):
        xf = estimate_state(irb, frame, x0, solver=make())
        xp = estimate_state(irb, pts, x0, solver=make())
        assert np.array_equal(xf, xp) and not np.array_equal(xf, x0)
    # a weights callable sees the frame's points
    seen = []

    def weights(p):
        seen.append(p)
        return np.ones(len(p))

    xw = estimate_state(irb, frame, x0, weights=weights)
    assert len(seen) == 1 and np.array_equal(seen[0], pts)
    assert np.array_equal(xw, estimate_state(irb, pts, x0, weights=np.ones(len(pts))))


def test_tracker_takes_frames(irb):
    import flash
    from flash.depthsensors import DepthFrame, Kinect, raycast_depths
    from flash.geometry import Transform, angle_axis
    from flash.tracking import Tracker, track
    sensor = Kinect(24, 24)
    tf = Transform(angle_axis(np.pi / 2, [1, 0, 0]), np.array([0.0, 1.5, 0.5]))
    state = flash.ManipulatorState(irb)
    frames = []
    for k in range(3):
        state.q[:] = 0.05 * k
        frames.append(DepthFrame(raycast_depths(flash.skin(state), sensor, tf), sensor, tf))
    xs_f, tr = track(irb, frames, state=flash.ManipulatorState(irb))
    by_points = Tracker(irb, flash.ManipulatorState(irb))  # (frame by frame, no prefetch: as frames go)
    xs_p = np.array([by_points.step(f.points()[0]) for f in frames])
    assert np.array_equal(xs_f, xs_p)
    assert tr.cost._points is None  # (nothing asked for the host points)


def test_weights_lifecycle(contexts, scene):
    from flash.depthsensors import Kinect
    a, _ = contexts("f64-sorted")
    shape = (37, 53)
    rays = Kinect(*shape).rays
    a.set_sensor(rays, "range")
    img, scale = _image(np.float32, shape, "random")
    a.set_depth(img, _tform(), NEAR, FAR, scale)
    w_img = rng(5).uniform(0.1, 1.0, size=shape)
    w = w_img.ravel()[a.depth_pixels()]
    a.set_point_weights(w)
    assert np.array_equal(a.point_weights(), w[a.permutation()])
    # the next frame clears them
    a.set_depth(img, _tform(), NEAR, FAR, scale)
    assert a.point_weights() is None


def test_errors_keep_the_resident_cloud(scene):
    from flash import _lib
    from flash.depthsensors import Kinect
    a = _lib.Context(device=0, sort_points=True)
    a.set_model(scene[0])
    pts = rng(9).uniform(-0.5, 0.5, size=(300, 3)) + [0.0, 0.0, 0.5]
    a.set_points(pts)
    before = a.eval(scene[1], per_point=True)
    img, _ = _image(np.float64, (8, 8), "all")

    def refused(status, call):
        with pytest.raises(_lib.FlashNativeError) as e:
            call()
        assert e.value.status == status
        assert a._num_points() == 300
        after = a.eval(scene[1], per_point=True)
        assert all(np.array_equal(x, y) for x, y in zip(after[2], before[2]))

    refused(3, lambda: a.set_depth(img))  # no sensor: FSDF_ERR_STATE
    refused(3, a.depth_pixels)            # fsdf_set_points' cloud has no pixels
    rays = Kinect(8, 8).rays
    for bad, kind in ((np.full((8, 8, 3), np.nan), "range"), (np.zeros((8, 8, 3)), "range"), (-rays, "z")):
        refused(1, lambda: a.set_sensor(bad, kind))
    assert a.sensor() is None
    a.set_sensor(rays, "range")
    refused(1, lambda: a.set_sensor(np.zeros((8, 8, 3)), "range"))
    assert a.sensor() == (8, 8, "range")  # (the earlier sensor stays)
    nan_pose = np.concatenate([np.eye(3).ravel(), [0.0, np.nan, 0.0]])
    refused(1, lambda: a.set_depth(img, nan_pose))
    refused(1, lambda: a.set_depth(img, None, 2.0, 1.0))
    refused(1, lambda: a.set_depth(img, None, np.nan, 1.0))
    for scale in (0.0, -1.0, np.inf, np.nan):
        refused(1, lambda: a.set_depth(img, None, 0.0, 1.0, scale))
    with pytest.raises(TypeError):
        a.set_depth(img.astype(np.int32))
    # a depth frame, then fsdf_set_points: the pixel list is gone
    assert a.set_depth(img, None, NEAR, FAR) == 64
    assert len(a.depth_pixels()) == 64
    a.set_points(pts)
    refused(3, a.depth_pixels)
    # the sensor is a context setting: it survives the cloud swap, and clears on request
    assert a.sensor() == (8, 8, "range")
    a.set_sensor(None)
    refused(3, lambda: a.set_depth(img))
    a.close()


def test_two_functors_displace_each_other(irb):
    from flash.depthsensors import DepthFrame, Kinect
    from flash.gradientdescent import CostFunctor
    sensor = Kinect(20, 30)
    img, _ = _image(np.float64, (20, 30), "random")
    frame = DepthFrame(img, sensor, _tform(), NEAR, FAR)
    cloud = rng(11).uniform(-0.4, 0.4, size=(500, 3)) + [0.0, 0.0, 0.6]
    x = 0.1 * np.arange(irb.mechanism.num_positions)
    f_depth = CostFunctor(irb, frame)
    c_depth = f_depth(x)
    f_array = CostFunctor(irb, cloud)  # (displaces the frame)
    c_array = f_array(x)
    assert c_depth != c_array
    assert f_depth(x) == c_depth and f_depth.n_points == len(frame.points()[1])
    assert f_array(x) == c_array and f_array.n_points == 500
    assert f_depth(x) == c_depth
    assert np.array_equal(f_depth.depth_pixels(), frame.points()[1])
    assert np.array_equal(f_depth.sensed_points, frame.points()[0])
    assert c_depth == CostFunctor(irb, frame.points()[0])(x)


def test_sizes_grow_and_shrink_and_runs_repeat(contexts, scene):
    """One context through a small, a larger and a smaller sensor again (the
    grow-only buffers), and one frame twice: identical resident points and pix."""
    from flash.depthsensors import Kinect
    a, b = contexts("f64")
    tf = _tform()
    for shape in ((16, 16), (61, 67), (5, 13)):
        rays = Kinect(*shape).rays
        a.set_sensor(rays, "range")
        img, scale = _image(np.uint16, shape, "random")
        _check_frame(a, b, scene[1], img, rays, tf, "range", scale)
    # (an unsorted f64 context: FSDF_ORDER_CALLER d* and grad name the resident points)
    shape = (61, 67)
    rays = Kinect(*shape).rays
    a.set_sensor(rays, "z")
    img, scale = _image(np.float32, shape, "runs")
    runs = []
    for _ in range(2):
        a.set_depth(img, tf, NEAR, FAR, scale)
        runs.append((a.depth_pixels(), a.eval(scene[1], per_point=True)))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert all(np.array_equal(x, y) for x, y in zip(runs[0][1][2], runs[1][1][2]))


@pytest.mark.parametrize("fmt", [np.float64, np.float32, np.uint16], ids=["f64", "f32", "u16"])
def test_device_source(contexts, scene, fmt):
    import torch
    from flash.depthsensors import Kinect
    a, b = contexts("f64-sorted")
    shape = (37, 53)
    rays = Kinect(*shape).rays
    tf = _tform()
    img, scale = _image(fmt, shape, "random")
    for c in (a, b):
        c.set_sensor(rays, "range")
    a.set_depth(img, tf, NEAR, FAR, scale)
    t = torch.from_numpy(img.view(np.int16) if fmt == np.uint16 else img).to("cuda:0")
    torch.cuda.synchronize()
    assert b.set_depth_device(t.data_ptr(), fmt, tf, NEAR, FAR, scale) == a.n
    assert np.array_equal(a.depth_pixels(), b.depth_pixels())
    _same_pass(a, b, scene[1])
    from flash import _lib
    with pytest.raises(_lib.FlashNativeError) as e:
        b.set_depth_device(t.data_ptr(), 7, tf)
    assert e.value.status == 1
