"""The free-space term on the CPU (include/flashsdf.h "free space"): the numpy
twin of the depth frame's free-space samples (flash.depthsensors.FreeSpace,
free_space_points), the one-sided gate of flash.robust.weighted_sums, the
gradient of Σ_surface d*² + Σ_free min(d*, 0)² over the CPU oracle against
central differences, and a scene the surface term alone cannot move
(free_space_scene; tests/test_gpu_free_space.py holds the device to the same
conditions)."""
import numpy as np
import pytest

from gn_helpers import OracleCost, floating_scene

NEAR, FAR = 0.5, 3.0


# ---- 1. the twin ------------------------------------------------------------------------------

def _rays(rows, cols):
    from flash.depthsensors import Kinect
    return Kinect(rows, cols).rays if (rows, cols) != (1, 1) else np.array([[[0.1, -0.2, 1.0]]])


def _tform():
    from flash.geometry import Transform, angle_axis
    return Transform(angle_axis(2.0, [1.0, 0.2, -0.1]), np.array([0.1, 1.6, 0.6]))


def hand_image(rows, cols, seed=0):
    """Every kind of pixel in one image: valid returns all over [NEAR, FAR], returns closer
    than any (J − 1) · spacing used here reaches, and — cycling — NaN, 0, negative, +inf,
    −inf, beyond far (misses) and too near."""
    r = np.random.default_rng(100 * rows + cols + seed)
    n = rows * cols
    img = r.uniform(NEAR, FAR, n)
    kinds = r.integers(0, 4, n)  # 0, 1: valid; 2: close to NEAR; 3: not valid
    img[kinds == 2] = r.uniform(NEAR, NEAR + 0.06, (kinds == 2).sum())
    bad = np.array([np.nan, 0.0, -1.5, np.inf, -np.inf, 2.0 * FAR, 0.5 * NEAR, 0.01 * NEAR])
    img[kinds == 3] = bad[np.arange((kinds == 3).sum()) % len(bad)]
    return img.reshape(rows, cols)


def expected_sending(img, stride, J, gap, spacing, miss_range, near=NEAR, far=FAR, scale=1.0):
    """(valid [npix], sending [npix], L [npix]) by a per-pixel Python loop: the rule as the
    header states it, written independently of the twin's array code."""
    rows, cols = img.shape
    valid, send, L = np.zeros(img.size, bool), np.zeros(img.size, bool), np.zeros(img.size)
    for i, raw in enumerate(img.reshape(-1)):
        s = np.float64(scale) * np.float64(raw)
        valid[i] = bool(np.isfinite(s) and s > 0.0 and near <= s <= far)
        if (i // cols) % stride or (i % cols) % stride:
            continue
        if valid[i]:
            L[i] = s - np.float64(gap)
        elif miss_range > 0.0 and not (s > 0.0 and s < near):
            L[i] = miss_range
        else:
            continue
        send[i] = L[i] - np.float64(J - 1) * np.float64(spacing) > 0.0
    return valid, send, L


@pytest.mark.parametrize("kind", ["range", "z"])
@pytest.mark.parametrize("shape,stride", [((1, 1), 1), ((3, 5), 2), ((7, 10), 3), ((17, 31), 1), ((8, 13), 2)])
def test_twin_properties(shape, stride, kind):
    from flash.depthsensors import DepthFrame, FreeSpace, Kinect, depth_points, free_space_points, pixel_directions
    rays, tf = _rays(*shape), _tform()
    u = pixel_directions(rays, kind)
    for img in (hand_image(*shape), np.full(shape, 1.5), np.full(shape, np.nan), np.full(shape, 0.1 * NEAR)):
        base_pts, base_pix = depth_points(img, rays, tf, NEAR, FAR, 1.0, kind)
        for J, gap, spacing, miss in ((1, 0.0, 0.0, 0.0), (2, 0.02, 0.05, 0.0), (3, 0.02, 0.3, 2.0), (16, 0.01, 0.04, 0.7)):
            fs = FreeSpace(J, stride, gap, spacing, miss)
            pts, pix = free_space_points(img, rays, tf, NEAR, FAR, 1.0, kind, fs)
            valid, send, L = expected_sending(img, stride, J, gap, spacing, miss)
            n_surface, m = int(valid.sum()), int(send.sum())
            # the count; the observed points first, unchanged
            assert len(pts) == len(pix) == n_surface + J * m and pix.dtype == np.int32
            assert np.array_equal(pts[:n_surface], base_pts) and np.array_equal(pix[:n_surface], base_pix)
            # j-major, then pixel row-major
            sp = np.flatnonzero(send)
            assert np.array_equal(pix[n_surface:], np.tile(sp, J))
            assert (sp // shape[1] % stride == 0).all() and (sp % shape[1] % stride == 0).all()
            # every sample on its pixel's ray at t = L − (j − 1) spacing, t_1 = L exactly; in front of a return
            R, t0 = np.asarray(tf.R), np.asarray(tf.t)
            for j in range(J):
                blk = pts[n_surface + j * m: n_surface + (j + 1) * m]
                t = L[sp] - np.float64(j) * np.float64(spacing)
                assert (t > 0).all()
                cam = (blk - t0) @ R  # (Rᵀ (p − t): back in the camera frame)
                assert np.allclose(cam, t[:, None] * u[sp], rtol=0, atol=1e-12)
                if kind == "range":
                    rng_ = np.linalg.norm(blk - t0, axis=1)
                    assert np.allclose(rng_, t, rtol=0, atol=1e-12)
                    s = img.reshape(-1)[sp]
                    ret = valid[sp]
                    assert (rng_[ret] <= s[ret] - gap + 1e-12).all()
                if j == 0:
                    # t_1 = s − gap exactly: the twin's own arithmetic on that range
                    want = np.empty_like(blk)
                    c = [L[sp] * u[sp, a] for a in range(3)]
                    for a in range(3):
                        want[:, a] = ((R[a, 0] * c[0] + R[a, 1] * c[1]) + R[a, 2] * c[2]) + t0[a]
                    assert np.array_equal(blk, want)
                    assert np.array_equal(L[sp][valid[sp]], img.reshape(-1)[sp][valid[sp]] - np.float64(gap))
            # misses send only with miss_range > 0; too-near pixels never; short returns never
            s_all = img.reshape(-1)
            with np.errstate(invalid="ignore"):
                too_near = (s_all > 0) & (s_all < NEAR)
            assert not send[too_near].any()
            if miss == 0.0:
                assert not send[~valid].any()
            else:
                on_grid = (np.arange(img.size) // shape[1] % stride == 0) & (np.arange(img.size) % shape[1] % stride == 0)
                assert np.array_equal(send[~valid & ~too_near & on_grid],
                                      np.full((~valid & ~too_near & on_grid).sum(), miss - (J - 1) * spacing > 0))
            with np.errstate(invalid="ignore"):
                short = valid & (s_all - gap - (J - 1) * spacing <= 0)
            assert not send[short].any()
            # the frame's points() are the twin's
            f_pts, f_pix = DepthFrame(img, Kinect(*shape) if shape != (1, 1) else type("S", (), {"rays": rays})(), tf,
                                      NEAR, FAR, 1.0, kind, fs).points()
            assert np.array_equal(f_pts, pts) and np.array_equal(f_pix, pix)
    assert np.array_equal(free_space_points(img, rays, tf, NEAR, FAR, 1.0, kind, None)[0], base_pts)


def test_twin_cases_by_hand():
    """1 x 1 as valid, miss and too near; returns closer than (J − 1) · spacing; u16 with a scale."""
    from flash.depthsensors import FreeSpace, free_space_points
    rays = _rays(1, 1)
    fs = FreeSpace(3, 1, 0.2, 0.2, 0.0)
    for depth, n in ((1.0, 1 + 3), (np.nan, 0), (0.2, 0), (0.55, 1)):  # (0.55 − 0.2 − 0.4 > 0 fails: no samples)
        pts, pix = free_space_points(np.array([[depth]]), rays, None, NEAR, FAR, 1.0, "range", fs)
        assert len(pts) == n and (pix == 0).all()
    fs = FreeSpace(3, 1, 0.1, 0.2, 1.0)
    for depth, n in ((1.0, 4), (np.nan, 3), (np.inf, 3), (-1.0, 3), (0.0, 3), (2 * FAR, 3), (0.2, 0)):
        pts, _ = free_space_points(np.array([[depth]]), rays, None, NEAR, FAR, 1.0, "range", fs)
        assert len(pts) == n, depth
    pts, _ = free_space_points(np.array([[np.nan]]), rays, None, NEAR, FAR, 1.0, "range", fs)
    assert np.allclose(np.linalg.norm(pts, axis=1), [1.0, 0.8, 0.6], rtol=0, atol=1e-15)
    img = np.array([[1000, 0, 100, 65535]], np.uint16)  # (valid; a miss; too near; beyond far: a miss)
    pts, pix = free_space_points(img, _rays(1, 4), None, NEAR, FAR, 0.001, "z", FreeSpace(2, 1, 0.0, 0.25, 0.5))
    assert np.array_equal(pix, [0, 0, 1, 3, 0, 1, 3])
    assert np.array_equal(pts[:, 2], [1.0, 1.0, 0.5, 0.5, 0.75, 0.25, 0.25])  # (kind "z": t is the camera z)


def test_free_space_argument_checks():
    import flash
    from flash.depthsensors import DepthFrame, FreeSpace, Kinect
    assert flash.FreeSpace is FreeSpace
    f = FreeSpace(4, 2, 0.02, 0.05, 1.5)
    assert (f.samples, f.stride) == (4, 2) and np.array_equal(f.lengths, [0.02, 0.05, 1.5])
    assert FreeSpace(1, 1, 0.0, 0.0, 0.0).samples == 1  # (one sample needs no spacing)
    assert f == FreeSpace(4, 2, 0.02, 0.05, 1.5) and hash(f) == hash(FreeSpace(4, 2, 0.02, 0.05, 1.5))
    for bad in (dict(samples=0), dict(samples=17), dict(samples=-1), dict(samples=2.5), dict(samples=True),
                dict(stride=0), dict(stride=-2), dict(stride=1.5), dict(gap=-1e-9), dict(gap=np.nan),
                dict(gap=np.inf), dict(spacing=-0.1), dict(spacing=np.nan), dict(spacing=0.0, samples=2),
                dict(miss_range=-1.0), dict(miss_range=np.nan), dict(miss_range=np.inf)):
        with pytest.raises(ValueError):
            FreeSpace(**bad)
    assert DepthFrame(np.ones((2, 2)), Kinect(2, 2)).free_space is None


# ---- 2. the gate of weighted_sums -----------------------------------------------------------

@pytest.mark.parametrize("spec", ["square", "huber:0.02", "tukey:0.05"])
def test_weighted_sums_one_sided_is_a_gate_on_the_weights(spec):
    from flash import robust
    from flash.robust import weighted_sums
    r = np.random.default_rng(17)
    n, S = 4000, 5
    pts, grad = r.normal(size=(n, 3)), r.normal(size=(n, 3))
    grad /= np.linalg.norm(grad, axis=1, keepdims=True)
    d = r.normal(scale=0.04, size=n)
    d[::97] = 0.0  # (d = 0 is outside the gate)
    k = r.integers(-1, S + 1, n)
    mask = r.random(n) < 0.5
    a = r.uniform(0.0, 2.0, n)
    loss = robust.parse(spec)
    gate = np.where(mask, d < 0, True).astype(np.float64)  # host-made
    assert 0.2 * n < (gate == 0).sum() < 0.3 * n
    for weights in (None, a):
        got = weighted_sums(pts, k, d, grad, S, loss, weights, one_sided=mask)
        want = weighted_sums(pts, k, d, grad, S, loss, gate if weights is None else weights * gate)
        assert all(np.array_equal(u, v) for u, v in zip(got, want))
        assert not np.array_equal(got[0], weighted_sums(pts, k, d, grad, S, loss, weights)[0])
    none = weighted_sums(pts, k, d, grad, S, loss, a, one_sided=np.zeros(n, bool))
    assert all(np.array_equal(u, v) for u, v in zip(none, weighted_sums(pts, k, d, grad, S, loss, a)))
    # under SQUARE the samples' cost is Σ min(d, 0)²
    if loss is None:
        cost = weighted_sums(pts, k, d, grad, S, None, None, one_sided=np.ones(n, bool))[0]
        ok = (k >= 0) & (k < S)
        assert cost.sum() == pytest.approx((np.minimum(d[ok], 0.0) ** 2).sum(), rel=1e-13)
    with pytest.raises(ValueError):
        weighted_sums(pts, k, d, grad, S, loss, None, one_sided=np.ones(n))
    with pytest.raises(ValueError):
        weighted_sums(pts, k, d, grad, S, loss, None, one_sided=np.ones(n - 1, bool))


# ---- 3. the gradient against central differences ---------------------------------------------

class OneSidedOracleCost(OracleCost):
    """OracleCost of a split cloud — points [n_surface, n) are free-space samples — through
    flash.robust.weighted_sums(one_sided=) and the host chain rule and Gauss-Newton twin of
    flash/mechanism.py: x -> (c, ∂c/∂x, 2A)."""

    def __init__(self, m, pts, n_surface, loss=None, weights=None):
        super().__init__(m, pts)
        self.loss, self.weights = loss, weights
        self.free = np.arange(len(self.pts)) >= n_surface

    def sums(self, x, free_only=False):
        from flash.robust import weighted_sums
        d, k, g = self.per_point(x)
        a = self.weights
        if free_only:
            a = self.free.astype(np.float64) if a is None else a * self.free
        return weighted_sums(self.pts, k, d, g, len(self.sb), self.loss, a, one_sided=self.free)

    def value_and_gradient(self, x):
        return self(x)[:2]

    def __call__(self, x):
        x = np.asarray(x, np.float64)
        cost, wrench, mom, _ = self.sums(x)
        mech = self.m.mechanism
        bw = np.zeros((mech.num_bodies, 6))
        np.add.at(bw, self.sb, wrench)
        return float(cost.sum()), mech.config_gradient_numpy(x, bw), 2.0 * mech.gauss_newton_matrix_numpy(x, self.sb, mom)


def mixed_sign_cloud(m, pts, x, n_surface):
    """pts with its tail [n_surface, n) moved along ∇d* at x to the level sets d* = ∓1 cm,
    alternately, and 2 mm off them: free-space samples of both signs. Returns (cloud, d* of the
    moved tail at x)."""
    oc = OracleCost(m, pts)
    d, _, g = oc.per_point(x)
    out = np.array(pts, np.float64)
    tail = np.arange(n_surface, len(pts))
    level = np.where(tail % 2 == 0, -0.01, 0.01)
    out[tail] = pts[tail] - (d[tail] - level)[:, None] * g[tail]
    # (a point that was nearest to an edge or a vertex lands, moved inward along ∇d*, exactly on
    # the ridge between two faces, where d* has a kink and a central difference averages the two
    # sides: 2 mm in a random direction takes every sample off the ridges and keeps its sign)
    out[tail] += np.random.default_rng(len(pts)).uniform(-0.002, 0.002, (len(tail), 3))
    return out, OracleCost(m, out).per_point(x)[0][tail]


def _split_case(name):
    from flash import Models, synthetic
    if name == "floating":
        m, pts, x = floating_scene(3000)
        x[0:4] = np.array([0.9, 0.1, -0.2, 0.3]) * 1.3  # (base quaternion: rotated, |q| != 1)
    else:
        m = Models.irb140()
        q_true, x = synthetic.perturbed_configuration(m, 41)
        pts, x = synthetic.depth_cloud(m, q_true, 3000, seed=42), np.asarray(x, np.float64)
    n_surface = 1700
    cloud, d_free = mixed_sign_cloud(m, pts, x, n_surface)
    return m, cloud, x, n_surface, d_free


@pytest.mark.parametrize("name", ["irb140", "floating"])
def test_split_gradient_matches_central_differences(oracle_mod, name):
    """∂/∂x of Σ_surface d*² + Σ_free min(d*, 0)² by the chain rule on the one-sided wrench
    against central differences of the cost itself: the step (h = 1e-6) and tolerance
    (|g − g_fd|_∞ <= 1e-7 |g|_∞) of tests/test_point_weights.py on IRB140, its scene. The
    gate adds no kink: min(d*, 0)² is C¹, a sample whose d* changes sign inside the step
    contributes O(h²) to the difference. The floating scene is not in that file; its step is
    the h = 1e-7 that tests/test_gpu_point_weights.py and tests/test_gpu_robust.py use for it,
    under the same tolerance: at 1e-6 a surface point of this start changes its nearest hull
    inside the step, where d*² itself has a kink, and the plain least-squares cost with no
    split misses the tolerance by the same 1.9e-2 in the same entry — at 1e-7 both pass. The
    rounding of the difference, about 2^-52 c / h = 5e-8, stays below 1e-7 |g|_∞ = 8e-6."""
    m, cloud, x, n_surface, d_free = _split_case(name)
    n_free = len(cloud) - n_surface
    neg, pos = int((d_free < 0).sum()), int((d_free > 0).sum())
    assert 4 * neg >= n_free and 4 * pos >= n_free, (neg, pos, n_free)
    oc = OneSidedOracleCost(m, cloud, n_surface)
    c, g = oc.value_and_gradient(x)
    # the cost is what it says
    d = oc.per_point(x)[0]
    want = (d[:n_surface] ** 2).sum() + (np.minimum(d[n_surface:], 0.0) ** 2).sum()
    assert c == pytest.approx(want, rel=1e-12)
    h, eye = (1e-7 if name == "floating" else 1e-6), np.eye(len(x))
    g_fd = np.array([(oc.value_and_gradient(x + h * e)[0] - oc.value_and_gradient(x - h * e)[0]) / (2 * h) for e in eye])
    err, scale = float(np.abs(g - g_fd).max()), float(np.abs(g).max())
    print(f"{name} split {n_surface}/{len(cloud)} (free: {neg} inside, {pos} outside): c {c:.6f} |g|_inf {scale:.4f} "
          f"|g - g_fd|_inf {err:.2e}")
    assert scale > 0 and err <= 1e-7 * scale, (err, scale)
    # the free part alone has a gradient of its own
    free_only = OneSidedOracleCost(m, cloud[n_surface:], 0)
    assert np.abs(free_only.value_and_gradient(x)[1]).max() > 0


# ---- 4. what it buys: a body in front of what the camera saw ------------------------------------

def free_space_scene():
    """tests/test_gpu_free_space.py's scene, chosen on the CPU (test_what_it_buys_on_the_cpu):
    the floating table and a second floating box B, taller than wide (its side faces are
    nearest for most interior points), under Kinect(24, 32) looking down. The frame is a
    raycast of the scene with B far outside the view; the estimate has the table at its true
    pose and B between camera and table, overlapping one side of the view. Returns
    (manipulator, x_true, x_start, sensor, tform, FreeSpace, B's state slice)."""
    from flash import Models
    from flash.core import ConvexGeometry, Manipulator
    from flash.depthsensors import FreeSpace, Kinect
    from flash.geometry import Transform, angle_axis
    from flash.mechanism import Mechanism, QuaternionFloating
    m = Models.table(width=TABLE_HALF_WIDTH)
    mech = Mechanism("world")
    b = mech.attach(0, QuaternionFloating("blocker_floating"), None, "blocker_body")
    blocker = Manipulator(mech, [ConvexGeometry(Models.box_hull(BLOCKER_HALF), b, Transform(np.eye(3), np.zeros(3)),
                                                "blocker")])
    Models.merge(m, blocker)
    x = np.array(m.mechanism.zero_configuration(), np.float64)
    rt = m.mechanism.q_range(m.mechanism.body_index("table_body"))
    rb = m.mechanism.q_range(m.mechanism.body_index("blocker_body"))
    x[rt.start + 4: rt.start + 7] = TABLE_AT
    x_true, x_start = x.copy(), x.copy()
    x_true[rb.start + 4: rb.start + 7] = BLOCKER_AWAY
    x_start[rb.start + 4: rb.start + 7] = BLOCKER_START
    sensor = Kinect(24, 32)
    tform = Transform(angle_axis(np.pi, [1.0, 0.0, 0.0]), np.array(CAMERA_AT))  # (z down)
    return m, x_true, x_start, sensor, tform, FreeSpace(FREE_SAMPLES, 1, 0.02, FREE_SPACING, 0.0), slice(rb.start, rb.stop)


# B: 0.16 x 0.16 x 0.40 m; spacing 0.08 = half its smallest extent; 12 samples reach 0.02 + 11 · 0.08 =
# 0.90 m up from the table top, past B's top
BLOCKER_HALF = (0.08, 0.08, 0.20)
TABLE_HALF_WIDTH = 0.6  # (the view at the table top, 1.2 m below the camera, is 1.21 x 1.45 m)
TABLE_AT = (0.0, 0.0, 0.0)
CAMERA_AT = (0.0, 0.0, 1.25)
BLOCKER_AWAY = (5.0, 5.0, 0.0)
BLOCKER_START = (0.22, 0.05, 0.65)
FREE_SAMPLES, FREE_SPACING = 12, 0.08
# the CPU run's free-space cost Σ_free min(d*, 0)² at the start and after 20 LM evaluations
# (test_what_it_buys_on_the_cpu prints them)
CPU_FREE_COST = (2.130602e-01, 0.0)


def lm_accepted_costs(vgh, x0, n, limit=20):
    """LevenbergMarquardt.optimize over vgh / n, and the costs it accepted in order."""
    from flash.tracking import LevenbergMarquardt
    seen = []

    def f(x):
        c, g, H = vgh(x)
        seen.append(c)
        return c / n, g / n, H / n

    s = LevenbergMarquardt(len(x0), iteration_limit=limit, gradient_convergence_tolerance=0.0)
    x, _ = s.optimize(f, x0)
    accepted = [seen[0]]
    for c in seen[1:]:
        if c < accepted[-1]:
            accepted.append(c)
    return x, seen, accepted


def test_what_it_buys_on_the_cpu(oracle_mod):
    """The loop composed from the oracle, weighted_sums and flash/mechanism.py on
    free_space_scene: (a) without free space B's seven gradient entries are exactly 0.0;
    (b) with it the start has >= 32 samples with d* < 0, B's translation gradient is nonzero,
    the accepted costs decrease, and the free-space cost at least halves within 20
    evaluations."""
    from flash.depthsensors import DepthFrame
    m, x_true, x_start, sensor, tform, fs, sl = free_space_scene()
    om_depth = _oracle_raycast(m, x_true, sensor, tform)
    frame = DepthFrame(om_depth, sensor, tform, free_space=None)
    pts, _ = frame.points()
    assert len(pts) > 100
    plain = OneSidedOracleCost(m, pts, len(pts))
    c, g = plain.value_and_gradient(x_start)
    assert (g[sl] == 0.0).all()  # (a): exactly zero for B
    frame = DepthFrame(om_depth, sensor, tform, free_space=fs)
    cloud, _ = frame.points()
    n_surface = frame.n_surface()
    assert n_surface == len(pts) and len(cloud) > n_surface
    oc = OneSidedOracleCost(m, cloud, n_surface)
    d = oc.per_point(x_start)[0]
    assert int((d[n_surface:] < 0).sum()) >= 32
    c, g = oc.value_and_gradient(x_start)
    assert np.abs(g[sl.start + 4: sl.stop]).max() > 0
    free0 = float(oc.sums(x_start, free_only=True)[0].sum())
    x, seen, accepted = lm_accepted_costs(oc, x_start, len(cloud))
    free1 = float(oc.sums(x, free_only=True)[0].sum())
    print(f"free-space scene (CPU): n {len(cloud)} ({n_surface} observed), inside at start "
          f"{int((d[n_surface:] < 0).sum())}, cost {seen[0]:.6e} -> {accepted[-1]:.6e}, free-space cost {free0:.6e} -> "
          f"{free1:.6e} in {len(seen)} evaluations")
    assert all(b < a for a, b in zip(accepted, accepted[1:])) and len(accepted) >= 3 and len(seen) <= 20
    assert free1 <= 0.5 * free0
    assert free0 == pytest.approx(CPU_FREE_COST[0], rel=1e-6) and free1 <= CPU_FREE_COST[1] + 1e-12
    assert np.array_equal(x[:sl.start], x_start[:sl.start]) or np.abs(x[:sl.start] - x_start[:sl.start]).max() < 1e-6


def _oracle_raycast(m, x, sensor, tform):
    """The depth image of the scene at x by the CPU: per ray the first hit of the posed hulls
    (slab clipping against every hull's planes), NaN for a miss."""
    import flash
    mech = m.mechanism
    poses = flash.hull_poses(m, mech.normalize(x))
    rays = sensor.rays.reshape(-1, 3) @ np.asarray(tform.R).T
    rays = rays / np.linalg.norm(rays, axis=1, keepdims=True)
    o = np.asarray(tform.t, np.float64)
    best = np.full(len(rays), np.inf)
    for s, pose in zip(m.surfaces, np.asarray(poses).reshape(-1, 12)):
        R, t = pose[:9].reshape(3, 3), pose[9:]
        nrm = s.hull.planes[:, :3] @ R.T  # world normals; plane: n_w · p <= off + n_w · t
        off = s.hull.planes[:, 3] + nrm @ t
        den = rays @ nrm.T
        num = off - nrm @ o
        with np.errstate(divide="ignore", invalid="ignore"):
            tt = num[None, :] / den
        t_in = np.where(den < 0, tt, -np.inf).max(1)
        t_out = np.where(den > 0, tt, np.inf).min(1)
        outside_parallel = ((den == 0) & (num[None, :] < 0)).any(1)
        hit = (t_in <= t_out) & (t_in > 0) & ~outside_parallel
        best = np.where(hit & (t_in < best), t_in, best)
    return np.where(np.isfinite(best), best, np.nan).reshape(sensor.rays.shape[:2])
