"""GPU: tracking through a voxel grid (estimate_state / Tracker / track
`voxel=`; include/flashsdf.h "voxel grid"). IRB140 seen by Kinect(96, 128) from
1 m: a depth image raycast on the device at q_true, a start off by a fixed
perturbation, LevenbergMarquardt on the host loop under a Huber loss, once on
the full frame and once through VoxelGrid(H).

The joint error is taken over joints 1-3. A noise-free cloud of the arm does
not determine the wrist (the LM prior's entry: H_ii / N of 6e-5 ..
3e-9 for joints 4-6 against 1e-2 .. 7e-2 for joints 1-3); on the CPU-composed
run of this scene joint 6 ends 0.5 rad from q_true on the FULL frame, at a cost
within rounding of the minimum.

Chosen on the CPU twin before any device run (oracle raycast of the same scene,
3,698 points): H = 0.03 keeps 610 voxels (16 %), the centroids lie up to 8.0 mm
inside the surface (corners and edges; h²/8R on the convex faces), the
CPU-composed voxel run ends 2.3e-3 rad from q_true on joints 1-3 where the full
frame ends 7e-6, and the start state's cost c/N is 1.020 times the full
frame's (h = 0.02: 1.014, 0.04: 1.073, 0.05: 1.186). The test recomputes each of
these on the frame it raycasts."""
import numpy as np
import pytest

from test_free_space import OneSidedOracleCost

pytestmark = pytest.mark.gpu

H = 0.03
START = np.array([0.08, -0.06, 0.07, 0.05, -0.04, 0.06])
Q_TRUE = np.array([0.3, -0.2, 0.25, 0.1, -0.15, 0.2])
DETERMINED = slice(0, 3)


def _loss():
    from flash.robust import Huber
    return Huber(0.02)


def _lm(n, limit=30):
    from flash.tracking import LevenbergMarquardt
    return LevenbergMarquardt(n, iteration_limit=limit, gradient_convergence_tolerance=0.0)


@pytest.fixture(scope="module")
def scene(irb, oracle_mod):
    """(frame, its points, the grid, the twin's voxels, the centroids' largest
    |d*| at q_true, the CPU-composed voxel run's solution)."""
    import flash
    from flash import VoxelGrid
    from flash.depthdata import voxel_downsample
    from flash.depthsensors import DepthFrame, Kinect, raycast_depths
    from flash.geometry import Transform, angle_axis
    sensor = Kinect(96, 128)
    tf = Transform(angle_axis(np.pi / 2, [1, 0, 0]), np.array([0.0, 1.0, 0.45]))
    state = flash.ManipulatorState(irb)
    state.q[:] = Q_TRUE
    frame = DepthFrame(raycast_depths(flash.skin(state), sensor, tf), sensor, tf)
    pts, _ = frame.points()
    grid = VoxelGrid(H)
    xyz, count, *_ = voxel_downsample(pts, grid)
    # the offset of the centroids: inside a convex surface by about h²/8R, more at edges and corners
    offset = float(np.abs(OneSidedOracleCost(irb, xyz, len(xyz)).per_point(Q_TRUE)[0]).max())
    # the loop composed on the CPU (oracle, flash.robust.weighted_sums, flash/mechanism.py) on the
    # weighted centroids: the joint error that offset explains
    oc = OneSidedOracleCost(irb, xyz, len(xyz), loss=_loss(), weights=count.astype(np.float64))
    n = float(count.sum())
    costs = []

    def f(x):
        c, g, Hm = oc(x)
        costs.append(c)
        return c / n, g / n, Hm / n

    x_cpu, _ = _lm(len(Q_TRUE)).optimize(f, Q_TRUE + START)
    full0 = OneSidedOracleCost(irb, pts, len(pts), loss=_loss())(Q_TRUE + START)[0] / len(pts)
    return frame, pts, grid, (xyz, count), offset, x_cpu, (costs[0] / n, full0)


def test_voxel_run_tracks_as_the_full_frame_does(irb, scene):
    from flash.tracking import estimate_state
    frame, pts, grid, (xyz, count), offset, x_cpu, (cpu_vox0, cpu_full0) = scene
    n = len(Q_TRUE)
    x0 = Q_TRUE + START
    assert len(pts) > 2000 and 4 * len(xyz) <= len(pts), (len(xyz), len(pts))
    seen = {"full": [], "voxel": []}
    x_full = estimate_state(irb, frame, x0, solver=_lm(n), loss=_loss(), callback=lambda x, c: seen["full"].append(c))
    x_vox = estimate_state(irb, frame, x0, solver=_lm(n), loss=_loss(), voxel=grid,
                           callback=lambda x, c: seen["voxel"].append(c))
    err0 = float(np.abs(START[DETERMINED]).max())
    e_full = float(np.abs(x_full - Q_TRUE)[DETERMINED].max())
    e_vox = float(np.abs(x_vox - Q_TRUE)[DETERMINED].max())
    bias = float(np.abs(x_cpu - Q_TRUE)[DETERMINED].max())
    # the costs the solver works with: c / N, N the frame's size in both runs (Σ count = n)
    assert count.sum() == len(pts)
    f_full, f_vox = seen["full"][0] / len(pts), seen["voxel"][0] / float(count.sum())
    print(f"voxel tracking: {len(pts)} points -> {len(xyz)} voxels at h = {H}; centroid offset {offset:.2e} m; joint "
          f"error (joints 1-3) start {err0:.3f}, full frame {e_full:.2e}, voxel {e_vox:.2e}, CPU-composed voxel run "
          f"{bias:.2e}; start cost c/N full {f_full:.6e}, voxel {f_vox:.6e} (ratio {f_vox / f_full:.4f}; CPU twin "
          f"{cpu_vox0 / cpu_full0:.4f})")
    # the reference run recovers the pose: without this the comparison below could pass vacuously
    assert e_full < 0.25 * err0
    # the voxel run: at most twice the full frame's error plus what the centroids' offset explains
    assert offset < H  # (a centroid lies within its cell of the surface)
    assert e_vox <= 2.0 * e_full + bias
    # the start state's cost within 10 % of the full frame's (confirmed on the CPU twin: 1.020)
    assert abs(cpu_vox0 / cpu_full0 - 1.0) <= 0.10
    assert abs(f_vox - f_full) <= 0.10 * f_full


def test_tracker_and_track_give_estimate_states_bits(irb, scene):
    import flash
    from flash import VoxelGrid
    from flash.depthsensors import DepthFrame
    from flash.tracking import Tracker, estimate_state, track
    frame, pts, grid, (xyz, count), *_ = scene
    n = len(Q_TRUE)
    x0 = Q_TRUE + START
    loss = _loss()

    def state0():
        s = flash.ManipulatorState(irb)
        s.q[:] = x0
        return s

    x_es = estimate_state(irb, frame, x0, solver=_lm(n, 6), loss=loss, voxel=grid)
    assert not np.array_equal(x_es, x0)
    # the grid does not stay behind on the manipulator's shared context: the next depth image
    # handed to it directly is not thinned
    assert irb.engine().get_voxel_grid() is None
    # the frame's points through the grid: the same centroids, the same bits
    assert np.array_equal(estimate_state(irb, pts, x0, solver=_lm(n, 6), loss=loss, voxel=grid), x_es)
    tr = Tracker(irb, state0(), _lm(n, 6), loss=loss, voxel=grid)
    assert np.array_equal(tr.step(frame), x_es)
    assert tr.cost.n_points == len(xyz) and tr.cost.n_divisor == len(pts)
    # a second frame warm-started from the first's solution, and a step's own grid
    frame2 = DepthFrame(frame.depth + 0.001, frame.sensor, frame.tform)
    xs, tr2 = track(irb, [frame, frame2], state=state0(), solver=_lm(n, 6), loss=loss, voxel=grid)
    assert np.array_equal(xs[0], x_es)
    assert np.array_equal(xs[1], estimate_state(irb, frame2, xs[0], solver=_lm(n, 6), loss=loss, voxel=grid))
    assert getattr(tr2.cost, "_prefetched", None) is None  # (no prefetch with a grid)
    tr3 = Tracker(irb, state0(), _lm(n, 6), loss=loss)
    assert np.array_equal(tr3.step(frame, voxel=grid), x_es)
    assert np.array_equal(tr3.step(frame), estimate_state(irb, frame, x_es, solver=_lm(n, 6), loss=loss))
    # a weights callable sees the resident points, centroids first, and multiplies the counts
    got = []

    def ones(p):
        got.append(p)
        return np.ones(len(p))

    assert np.array_equal(estimate_state(irb, frame, x0, solver=_lm(n, 6), loss=loss, voxel=grid, weights=ones), x_es)
    assert len(got) == 1 and np.array_equal(got[0], frame.voxel_points(grid)[0]) and np.array_equal(got[0], xyz)
    # "unit": every centroid counts 1 and N is the resident count
    unit = VoxelGrid(H, weights="unit")
    x_unit = estimate_state(irb, frame, x0, solver=_lm(n, 6), loss=loss, voxel=unit)
    assert np.array_equal(x_unit, estimate_state(irb, xyz, x0, solver=_lm(n, 6), loss=loss))
    assert not np.array_equal(x_unit, x_es)
