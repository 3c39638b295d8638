"""GPU: the free-space term (include/flashsdf.h "free space") — the ONE_SIDED
instantiations of csrc/robust.hip against the weighted ones bit for bit and
against the numpy twin, the split's life cycle and refusals, the free-space
samples of a depth frame (csrc/depth.hip) against flash.depthsensors
.free_space_points bit for bit, the solver loops over the split objective, and
the scene of tests/test_free_space.py that the surface term alone cannot move."""
import numpy as np
import pytest

from conftest import rng
from test_free_space import (CPU_FREE_COST, free_space_scene, lm_accepted_costs)
from test_gpu_moments import _context, _hull_specs, _vgh_scene
from test_gpu_point_weights import _reference, _weights
from test_gpu_robust import DIAG, EPS, RUN_POINTS, _losses
from gn_helpers import IU

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 3
# around the chunk; three workgroups with a ragged tail; 65 chunks in nine workgroups
SIZES = (1, 63, 64, 65, 2 * RUN_POINTS + 101, 4097)


def _mixed(pts, d, g, seed):
    """pts moved along ∇d* to the level sets d* = ∓1 cm, alternately, and 2 mm off them in a
    random direction: a cloud of both signs wherever it is split."""
    level = np.where(np.arange(len(pts)) % 2 == 0, -0.01, 0.01)
    return pts - (d - level)[:, None] * g + rng(seed).uniform(-0.002, 0.002, pts.shape)


@pytest.fixture(scope="module")
def pools():
    """name -> (surface specs, poses, a pool of 4,097 points of both signs of d*)."""
    import flash
    from flash import Models, synthetic
    out = {}
    for name, m, seed in (("irb140", Models.irb140(), 21), ("m64", Models.arm_grid(), 31)):
        q_true, q_eval = synthetic.perturbed_configuration(m, seed)
        specs, poses = _hull_specs(m), flash.hull_poses(m, q_eval)
        pts = synthetic.depth_cloud(m, q_true, 4097, seed=seed + 1)
        ctx = _context(specs, 64, False)
        try:
            ctx.set_points(pts)
            _, _, (k, d, g) = ctx.eval(poses, per_point=True)
        finally:
            ctx.close()
        out[name] = (specs, poses, _mixed(pts, d, g, seed))
    return out


def _same(u, v):
    return u[0] == v[0] and all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(u[1:], v[1:]))


def _splits(n):
    return sorted({s for s in (0, 1, 37, n // 2 + 5, n - 1) if 0 <= s < n})


def _one_sided_against_weighted(ctx, poses, n, d, r, label, splits=None, losses=None):
    """For every split, loss and row length: eval_robust with the split set returns the bits of
    the weighted path given a_i = 1 for surface points and for free points with d* < 0, else 0;
    with caller weights b also set, those of the weights b · a. d: d* in caller order."""
    idx = np.arange(n)
    b = _weights(r, n)
    seen_gate = False
    for split in (_splits(n) if splits is None else splits):
        a = np.where((idx < split) | (d < 0), 1.0, 0.0)
        seen_gate = seen_gate or (a == 0).any()
        for loss in (_losses() if losses is None else losses):
            ctx.set_loss(loss)
            for moments in (True, False):
                for caller, eff in ((None, a), (b, b * a)):
                    ctx.set_free_split(split)
                    assert ctx.get_free_split() == split
                    ctx.set_point_weights(caller)
                    got = ctx.eval_robust(poses, moments=moments)
                    ctx.set_free_split(None)
                    assert ctx.get_free_split() is None
                    ctx.set_point_weights(eff)
                    want = ctx.eval_robust(poses, moments=moments)
                    assert _same(got, want), (label, split, loss, moments, caller is not None)
    ctx.set_point_weights(None)
    return seen_gate


# ---- 1. the one-sided kernel against the weighted kernel, bit for bit ---------------------------

@pytest.mark.parametrize("sort_points", [False, True])
@pytest.mark.parametrize("scene,precision", [("irb140", 64), ("irb140", 32), ("m64", 64), ("m64", 32)])
def test_one_sided_rows_are_the_weighted_rows_bit_for_bit(pools, scene, precision, sort_points):
    surfaces, poses, pool = pools[scene]
    ctx = _context(surfaces, precision, sort_points)
    r = rng(1101)
    gated = False
    try:
        for step, n in enumerate(SIZES):
            pts = pool[7 * step:7 * step + n] if n < len(pool) else pool
            ctx.set_points(pts)
            assert ctx.get_free_split() is None
            _, _, (_, d, _) = ctx.eval(poses, per_point=True)  # (caller order: the order of the split)
            if n > 100:
                assert (d < 0).sum() > n // 4 and (d > 0).sum() > n // 4
            label = f"{scene} f{precision} sorted={sort_points} n={n}"
            gated |= _one_sided_against_weighted(ctx, poses, n, d, r, label)
            if sort_points and n > 1000:
                # after a regroup: another resident order, the permutation read anew
                perm = ctx.permutation()
                ctx.eval_robust(poses)
                ctx.regroup_points()
                assert not np.array_equal(ctx.permutation(), perm)
                ctx.set_free_split(n // 2 + 5)
                before = ctx.get_free_split()
                _one_sided_against_weighted(ctx, poses, n, d, r, label + " regrouped", splits=(n // 2 + 5, 1))
                assert before == n // 2 + 5
        assert gated
    finally:
        ctx.close()


# ---- 2. the rows against the numpy twin ---------------------------------------------------------

@pytest.mark.parametrize("sort_points", [False, True])
@pytest.mark.parametrize("scene,precision", [("irb140", 64), ("irb140", 32), ("m64", 64)])
def test_one_sided_rows_match_the_numpy_twin(pools, scene, precision, sort_points):
    """eval_robust with a split against flash.robust.weighted_sums(one_sided=) in longdouble,
    under the bounds of tests/test_gpu_point_weights.py::test_weighted_rows_match_per_point_outputs
    (its docstring) with a · gate as the weight."""
    from flash.robust import weighted_sums
    surfaces, poses, pool = pools[scene]
    S = len(surfaces)
    ctx = _context(surfaces, precision, sort_points)
    r = rng(1102)
    f64 = lambda v: np.asarray(v, np.float64)  # noqa: E731
    try:
        for n in (65, 2 * RUN_POINTS + 101, 4097):
            pts = pool[:n]
            ctx.set_points(pts)
            _, _, (k, d, g) = ctx.eval(poses, per_point=True)
            P = pts.astype(np.float32) if precision == 32 else pts
            split = n // 2 + 5
            free = np.arange(n) >= split
            for loss in _losses():
                for caller in (None, _weights(r, n)):
                    ctx.set_loss(loss)
                    ctx.set_point_weights(caller)
                    ctx.set_free_split(split)
                    cost, accum, M, W = ctx.eval_robust(poses)
                    rc, rf, rm, rw = weighted_sums(P, k, np.asarray(d, np.longdouble), g, S, loss, caller, one_sided=free)
                    assert rc.dtype == np.longdouble
                    a_eff = np.where(~free | (d < 0), 1.0 if caller is None else caller, 0.0)
                    R, F, A, sr, mr, sw, cnt = _reference(P, k, d, g, S, loss, a_eff)
                    L = np.sqrt((np.asarray(P, np.float64) ** 2).sum(1)).max()
                    D, amax = float(np.abs(d).max()), float(np.max(a_eff))
                    s = np.array([1.0, 1.0, 1.0, L, L, L])
                    b_m = EPS * cnt[:, None] * (np.sqrt(f64(R[:, DIAG])[:, IU[0]] * f64(R[:, DIAG])[:, IU[1]]) +
                                                amax * s[IU[0]] * s[IU[1]])
                    b_f = EPS * cnt[:, None] * (f64(A) + 2.0 * amax * D * s[None, :])
                    b_r = EPS * cnt * (f64(sr) + amax * f64(mr))
                    b_w = EPS * cnt * (f64(sw) + amax)
                    b_c = float(b_r.sum()) + S * 2.0 ** -52 * float(sr.sum())
                    wrench = accum[1:].reshape(S, 6)
                    label = (scene, precision, sort_points, n, loss, caller is not None)
                    assert (f64(np.abs(np.asarray(M, np.longdouble) - rm)) <= b_m).all(), label
                    assert (f64(np.abs(np.asarray(wrench, np.longdouble) - rf)) <= b_f).all(), label
                    assert (f64(np.abs(np.asarray(W, np.longdouble) - rw)) <= b_w).all(), label
                    assert float(abs(np.longdouble(cost) - rc.sum())) <= b_c, label
    finally:
        ctx.close()


# ---- 3. the split at the end --------------------------------------------------------------------

def test_split_at_the_end():
    """n_surface == n clears the split: with no loss and no weights the iteration calls return
    the least-squares bits of a context that never had one (the pass's own sums, not the robust
    reduction's). Under a loss, a split that gates nothing out — every free point has d* < 0 —
    runs the one-sided kernel and returns the bits of the robust path without a split."""
    from flash import _lib
    from flash.gradientdescent import register_native
    from flash.robust import Huber
    m, pts, x = _vgh_scene("irb140")
    n = len(pts)
    ctx = _lib.Context(device=0, precision=64, sort_points=True)
    try:
        ctx.set_surfaces(_hull_specs(m))
        register_native(m, ctx, 10)
        ctx.set_regroup(False)
        ctx.set_points(pts)
        c0, g0 = ctx.value_and_gradient(x)
        c1, g1, H1 = ctx.value_gradient_hessian(x)
        ctx.set_free_split(n // 3)
        cs, gs = ctx.value_and_gradient(x)
        assert cs < c0  # (the split objective: free points outside the model cost nothing)
        for clear in (n, -1, None):
            ctx.set_free_split(n // 3)
            ctx.set_free_split(clear)
            assert ctx.get_free_split() is None
            c, g = ctx.value_and_gradient(x)
            c2, g2, H2 = ctx.value_gradient_hessian(x)
            assert c == c0 and np.array_equal(g, g0)
            assert c2 == c1 and np.array_equal(g2, g1) and np.array_equal(H2, H1)
        # under a loss: the one-sided kernel with every gate open
        import flash
        poses = flash.hull_poses(m, m.mechanism.normalize(x))
        _, _, (k, d, g) = ctx.eval(poses, per_point=True)
        inside = pts - (d + 0.01)[:, None] * g
        ctx.set_points(inside)
        _, _, (_, d_in, _) = ctx.eval(poses, per_point=True)
        assert (d_in < 0).all()
        for loss in (Huber(0.02), None):
            ctx.set_loss(loss)
            ctx.set_point_weights(np.ones(n) if loss is None else None)  # (SQUARE: the robust path through the weights)
            plain = ctx.eval_robust(poses)
            vgh = ctx.value_gradient_hessian(x)
            for split in (0, 1, n - 1):
                ctx.set_free_split(split)
                assert ctx.get_free_split() == split
                assert _same(ctx.eval_robust(poses), plain)
                got = ctx.value_gradient_hessian(x)
                assert got[0] == vgh[0] and np.array_equal(got[1], vgh[1]) and np.array_equal(got[2], vgh[2])
            ctx.set_free_split(None)
    finally:
        ctx.close()


# ---- 4. ingest parity ----------------------------------------------------------------------------

NEAR, FAR = 0.8, 2.6
CONFIGS = {"f64": (64, False), "f64-sorted": (64, True), "f32-sorted": (32, True)}
PATTERNS = ("all", "none", "miss", "checkerboard", "near-band", "short")


def _image(fmt, shape, pattern):
    """(image, scale). all: every pixel valid; none: every pixel too near (no point, no
    sample); miss: every pixel a miss, cycling through its kinds; checkerboard: valid and miss
    alternate in both directions; near-band: the middle rows too near, the others valid;
    short: returns at NEAR + 1 .. 60 mm, closer than the 0.9 that 16 samples span."""
    rows, cols = shape
    n = rows * cols
    r = rng(11 * n + len(pattern))
    ii, jj = np.divmod(np.arange(n), cols)
    if fmt == np.uint16:
        img = r.integers(int(NEAR * 1000) + 1, int(FAR * 1000), size=n).astype(np.uint16)
        miss = np.array([0, 2601, 65535], np.uint16)
        near, scale = np.uint16(300), 0.001
        short = (int(NEAR * 1000) + 1 + np.arange(n) % 60).astype(np.uint16)
    else:
        img = r.uniform(NEAR * 1.01, FAR * 0.99, size=n).astype(fmt)
        miss = np.array([np.nan, 0.0, -1.5, np.inf, -np.inf, 2.0 * FAR], fmt)
        near, scale = fmt(0.5 * NEAR), 1.0
        short = (NEAR + 0.001 * (1 + np.arange(n) % 60)).astype(fmt)
    if pattern == "none":
        img[:] = near
    elif pattern == "miss":
        img[:] = miss[np.arange(n) % len(miss)]
    elif pattern == "checkerboard":
        sel = (ii + jj) % 2 == 1
        img[sel] = miss[np.arange(sel.sum()) % len(miss)]
    elif pattern == "near-band":
        img[(ii >= rows // 3) & (ii <= (2 * rows) // 3)] = near
    elif pattern == "short":
        img[:] = short
    return img.reshape(shape), scale


@pytest.fixture(scope="module")
def pairs(irb):
    """Per configuration a pair: one fed depth frames, one fed the twin's points and the split."""
    import flash
    from flash import _lib
    hulls = [(s.hull.vertices, s.hull.faces, s.hull.planes) for s in irb.surfaces]
    poses = flash.hull_poses(irb, 0.1 * np.arange(irb.mechanism.num_positions))
    made = {}

    def get(name):
        if name not in made:
            precision, sort = CONFIGS[name]
            pair = []
            for _ in range(2):
                c = _lib.Context(device=0, precision=precision, sort_points=sort)
                c.set_model(hulls)
                pair.append(c)
            made[name] = pair
        return made[name] + [poses]

    yield get
    for pair in made.values():
        for c in pair:
            c.close()


def _tform():
    from flash.geometry import Transform, angle_axis
    return Transform(angle_axis(2.0, [1.0, 0.2, -0.1]), np.array([0.1, 1.6, 0.6]))


def _check_free_frame(a, b, poses, img, rays, tf, kind, scale, fs, loss):
    """Context a fed the frame with free space on, b fed the twin's points and the split: the
    same pixels, permutation, k*, d*, ∇d* and robust rows. Returns (n_surface, n)."""
    from flash.depthsensors import depth_points, free_space_points
    pts, pix = free_space_points(img, rays, tf, NEAR, FAR, scale, kind, fs)
    n_surface = len(depth_points(img, rays, tf, NEAR, FAR, scale, kind)[1])
    a.set_free_space(fs)
    n = a.set_depth(img, tf, NEAR, FAR, scale)
    assert n == len(pix) == a.n
    got = a.depth_pixels()
    assert got.dtype == np.int32 and np.array_equal(got, pix)
    assert a.get_free_split() == (n_surface if n_surface < n else None)
    b.set_points(pts)
    b.set_free_split(n_surface)
    assert b.get_free_split() == a.get_free_split()
    assert np.array_equal(a.permutation(), b.permutation())
    ca, acc_a, (ka, da, ga) = a.eval(poses, per_point=True)
    cb, acc_b, (kb, db, gb) = b.eval(poses, per_point=True)
    assert np.array_equal(ka, kb) and np.array_equal(da, db) and np.array_equal(ga, gb)
    assert np.array_equal(acc_a, acc_b) and ca == cb
    for c in (a, b):
        c.set_loss(loss)
    assert _same(a.eval_robust(poses), b.eval_robust(poses))
    return n_surface, n


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("shape,stride", [((1, 1), 1), ((3, 5), 2), ((17, 31), 1), ((70, 70), 3)],
                         ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "s%d" % v)
def test_ingest_bit_parity_with_the_twin(pairs, shape, stride, config):
    from flash.depthsensors import FreeSpace, Kinect
    from flash.robust import Huber
    a, b, poses = pairs(config)
    rays = Kinect(*shape).rays if shape != (1, 1) else np.array([[[0.1, -0.2, 1.0]]])
    tf = _tform()
    sent = set()
    for kind in ("range", "z"):
        a.set_sensor(rays, kind)
        for fmt in (np.float64, np.float32, np.uint16):
            for pattern in PATTERNS:
                img, scale = _image(fmt, shape, pattern)
                for J, miss in ((1, 1.3), (2, 0.0), (16, 1.1)):
                    fs = FreeSpace(J, stride, 0.02, 0.06, miss)  # (J = 16 reaches 0.9 back from the return)
                    n_surface, n = _check_free_frame(a, b, poses, img, rays, tf, kind, scale, fs,
                                                     Huber(0.02) if J == 2 else None)
                    assert (n - n_surface) % J == 0
                    sent.add((pattern, J, n_surface > 0, n > n_surface))
    # what each pattern is there for
    assert ("all", 16, True, True) in sent and ("none", 16, False, False) in sent
    assert ("miss", 16, False, True) in sent and ("miss", 2, False, False) in sent
    assert ("short", 1, True, True) in sent and ("short", 16, True, False) in sent
    if shape != (1, 1):
        assert ("checkerboard", 16, True, True) in sent and ("near-band", 2, True, True) in sent
    a.set_free_space(None)


def test_ingest_parity_over_a_second_scan_tile(pairs):
    """520 x 520: 1,057 count blocks, a second tile of the scan for both rows of counts."""
    from flash.depthsensors import FreeSpace, Kinect
    a, b, poses = pairs("f32-sorted")
    shape = (520, 520)
    rays = Kinect(*shape).rays
    a.set_sensor(rays, "range")
    img, scale = _image(np.float32, shape, "checkerboard")
    n_surface, n = _check_free_frame(a, b, poses, img, rays, _tform(), "range", scale, FreeSpace(1, 1, 0.02, 0.05, 1.3),
                                     None)
    assert n_surface == 520 * 520 // 2 and n == n_surface + 520 * 520  # (every pixel sends its one sample)
    a.set_free_space(None)


# ---- 5. life cycle and refusals -----------------------------------------------------------------

def test_life_cycle(pools):
    import torch
    from flash import _lib
    from flash.depthsensors import FreeSpace, Kinect
    from flash.robust import Huber
    surfaces, poses, pool = pools["irb140"]
    n = 1000
    pts = pool[:n]
    ctx = _context(surfaces, 64, sort_points=True)
    lib, raw = ctx._lib, ctx._ctx
    try:
        ctx.set_loss(Huber(0.02))
        ctx.set_points(pts)
        plain = ctx.eval_robust(poses)
        # a split beyond the cloud: refused, the earlier one stays
        ctx.set_free_split(400)
        split = ctx.eval_robust(poses)
        assert split[0] < plain[0]
        assert lib.fsdf_set_free_split(raw, n + 1) == ERR_ARG and ctx.get_free_split() == 400
        assert _same(ctx.eval_robust(poses), split)
        # ignored by the least-squares queries
        ls = ctx.eval(poses)
        ctx.set_free_split(None)
        assert ctx.eval(poses)[0] == ls[0] and _same(ctx.eval_robust(poses), plain)
        # cleared by every call that makes another cloud resident
        t = torch.from_numpy(pts).to("cuda:0")
        torch.cuda.synchronize()

        def prefetched():
            ctx.prefetch_points(pts)
            ctx.eval_robust(poses)
            ctx.set_points_prefetched()

        for swap in (lambda: ctx.set_points(pts), lambda: ctx.set_points_device(t.data_ptr(), n), prefetched,
                     lambda: ctx.set_points_range(pool[:3000], 7, 7 + n)):
            ctx.set_points(pts)
            ctx.set_free_split(400)
            assert ctx.get_free_split() == 400
            swap()
            assert ctx.get_free_split() is None
        # a ranged cloud refuses a split, by name
        with pytest.raises(_lib.FlashNativeError) as e:
            ctx.set_free_split(400)
        assert e.value.status == ERR_STATE and "split" in str(e.value) and ctx.get_free_split() is None
        # the setting: bad arguments keep the earlier one
        fs = FreeSpace(3, 2, 0.02, 0.05, 1.2)
        assert ctx.get_free_space() is None
        ctx.set_free_space(fs)
        assert ctx.get_free_space() == (3, 2, 0.02, 0.05, 1.2)
        ok = np.array([0.02, 0.05, 1.2])
        for samples, stride, lengths in ((-1, 1, ok), (17, 1, ok), (3, 0, ok), (3, -1, ok), (3, 1, [np.nan, 0.05, 0.0]),
                                         (3, 1, [-0.1, 0.05, 0.0]), (3, 1, [0.02, 0.0, 0.0]), (3, 1, [0.02, -1.0, 0.0]),
                                         (3, 1, [0.02, 0.05, np.nan]), (3, 1, [0.02, 0.05, -1.0]),
                                         (3, 1, [0.02, 0.05, np.inf])):
            assert lib.fsdf_set_free_space(raw, samples, stride, _lib.ptr(np.array(lengths, np.float64))) == ERR_ARG
            assert ctx.get_free_space() == (3, 2, 0.02, 0.05, 1.2)
        assert lib.fsdf_set_free_space(raw, 3, 1, None) == ERR_ARG
        # it survives frames; a frame sets the split itself; weights are one per resident point
        shape = (17, 31)
        rays = Kinect(*shape).rays
        ctx.set_sensor(rays, "range")
        img, scale = _image(np.float32, shape, "checkerboard")
        for _ in range(2):
            nn = ctx.set_depth(img, _tform(), NEAR, FAR, scale)
            ns = ctx.get_free_split()
            assert ns == (17 * 31 + 1) // 2 and nn > ns and (nn - ns) % 3 == 0
            assert ctx.get_free_space() == (3, 2, 0.02, 0.05, 1.2)
        w_img = rng(5).uniform(0.1, 1.0, size=shape)
        w = w_img.ravel()[ctx.depth_pixels()]
        assert len(w) == nn
        assert lib.fsdf_set_point_weights(raw, _lib.ptr(w), ns) == ERR_ARG
        ctx.set_point_weights(w)
        assert np.array_equal(ctx.point_weights(), w[ctx.permutation()]) and ctx.get_free_split() == ns
        framed = ctx.eval_robust(poses)
        # a frame that errs keeps the resident cloud, its split and the setting
        with pytest.raises(_lib.FlashNativeError):
            ctx.set_depth(img, _tform(), 2.0, 1.0, scale)
        assert ctx.get_free_split() == ns and ctx._num_points() == nn and _same(ctx.eval_robust(poses), framed)
        # free space off: the frame clears the split
        ctx.set_free_space(None)
        assert ctx.get_free_space() is None
        assert ctx.set_depth(img, _tform(), NEAR, FAR, scale) == ns and ctx.get_free_split() is None
    finally:
        ctx.close()


def test_refusals_name_the_split():
    from flash import Models, _lib
    from flash.gradientdescent import CostFunctor, flatten
    m = Models.irb_and_squishable()[0]
    cf = CostFunctor(m, np.zeros((10, 3)) + 0.3)
    x = flatten(cf.state)
    with pytest.raises(NotImplementedError):
        cf.set_free_split(5)
    assert cf.n_surface == 10
    cf.ctx.set_free_split(5)  # (behind the functor's back: the library refuses the calls itself)
    try:
        for call in (lambda: cf.ctx.value_and_gradient(x), lambda: cf.ctx.value_gradient_hessian(x),
                     lambda: cf.ctx.descend(x, 2, 0.1, 0.5), lambda: cf.ctx.descend_lm(x, 2, 1e-3, 0.5)):
            with pytest.raises(_lib.FlashNativeError) as e:
                call()
            assert e.value.status == ERR_STATE and "split" in str(e.value), str(e.value)
    finally:
        cf.ctx.set_free_split(None)
    assert np.isfinite(cf.value_and_gradient(x)[0])
    # a rigid scene: the required device loops are refused by name, modes 1 run the host loop (the same bits)
    m, pts, q0 = _vgh_scene("irb140")
    n = len(pts)
    cf = CostFunctor(m, pts)
    cf.set_free_split(n // 2)
    assert cf.n_surface == n // 2 and cf.ctx.get_free_split() == n // 2
    cf.value_and_gradient(q0)
    with pytest.raises(_lib.FlashNativeError) as e:
        cf.descend_lm(q0, 6, 1e-3, 0.5, 0.0, n, device_loop="require")
    assert e.value.status == ERR_STATE and "split" in str(e.value)
    host = cf.descend_lm(q0, 6, 1e-3, 0.5, 0.0, n, device_loop=False)
    mode1 = cf.descend_lm(q0, 6, 1e-3, 0.5, 0.0, n, device_loop=True)
    assert np.array_equal(host[0], mode1[0]) and host[1:] == mode1[1:]
    try:
        cf.ctx.set_solver("require")
        with pytest.raises(_lib.FlashNativeError) as e:
            cf.descend(q0, 5, 0.1, 0.5, 0.0, None, n)
        assert e.value.status == ERR_STATE and "split" in str(e.value)
        cf.ctx.set_solver(False)
        host = cf.descend(q0, 5, 0.1, 0.5, 0.0, None, n)
        cf.ctx.set_solver(True)
        mode1 = cf.descend(q0, 5, 0.1, 0.5, 0.0, None, n)
        assert np.array_equal(host[0], mode1[0]) and host[1:] == mode1[1:]
    finally:
        cf.ctx.set_solver(True)
    # the split leaves with the cloud
    cf.set_sensed_points(pts)
    assert cf.n_surface == n and cf.ctx.get_free_split() is None


# ---- 6. the loops ---------------------------------------------------------------------------------

def _split_functor(loss=None):
    """(functor, q0, n) of IRB140 on a cloud whose tail [1700, 3000) are samples of both signs."""
    from flash.gradientdescent import CostFunctor
    m, pts, q0 = _vgh_scene("irb140")
    cf = CostFunctor(m, pts, loss=loss)
    _, d, g = cf.per_point(q0)
    cloud = np.array(pts)
    cloud[1700:] = _mixed(pts[1700:], d[1700:], g[1700:], 1106)
    cf.set_sensed_points(cloud)
    cf.set_free_split(1700)
    d = cf.per_point(q0)[1][1700:]
    assert 4 * (d < 0).sum() >= len(d) and 4 * (d > 0).sum() >= len(d)
    return cf, q0, len(cloud)


@pytest.mark.parametrize("spec", ["huber:0.02", "square"])
def test_loops_with_a_split_match_the_python_loops(spec):
    """tests/test_gpu_point_weights.py::test_loops_with_weights_match_the_python_loops with a
    split in place of the weights: fsdf_descend and fsdf_descend_lm are NaiveSolver.optimize and
    LevenbergMarquardt.optimize over the functor, the same bits, with and without a prior."""
    from flash import robust
    from flash.tracking import LevenbergMarquardt, NaiveSolver, state_prior
    cf, q0, n = _split_functor(robust.parse(spec))
    cf.value_and_gradient(q0)  # (the cloud's first pass: the same layout for every loop)

    def vg(x):
        c, g = cf.value_and_gradient(x)
        return c / n, g / n

    def vgh(x):
        c, g, H = cf.value_gradient_hessian(x)
        return c / n, g / n, H / n

    naive = NaiveSolver(len(q0), rate=0.1, max_step=0.5, iteration_limit=5, gradient_convergence_tolerance=0.0)
    x_py, f_py = naive.optimize(vg, q0)
    x, f, its = cf.descend(q0, 5, 0.1, 0.5, 0.0, None, n)
    assert its == naive.iterations == 5 and np.array_equal(x, x_py) and f == f_py
    for mu in (None, 1e-3):
        for limit, tol in ((6, 0.0), (30, 1e-4)):
            solver = LevenbergMarquardt(len(q0), iteration_limit=limit, gradient_convergence_tolerance=tol)
            x_py, f_py = solver.optimize(state_prior(vgh, q0, mu), q0)
            x, f, its, lam = cf.descend_lm(q0, limit, solver.damping, solver.max_step, tol, n, prior_weight=mu)
            assert its == solver.iterations and lam == solver.final_damping, (mu, limit)
            assert np.array_equal(x, x_py) and f == f_py, (mu, limit)
    assert not np.array_equal(x, q0)


def test_split_gradient_on_the_device_matches_central_differences():
    """The device's gradient of the split objective against central differences of its cost, as
    tests/test_gpu_point_weights.py::test_value_gradient_hessian_with_weights checks the weighted
    one (h = 1e-6, tolerance 2^-49 n c / h + 1e-7 |g|_∞); (c, g) the same bits from both calls."""
    cf, q0, n = _split_functor()
    cf.value_and_gradient(q0)
    c0, g0 = cf.value_and_gradient(q0)
    c, g, H = cf.value_gradient_hessian(q0)
    assert c == c0 and np.array_equal(g, g0) and np.array_equal(H, H.T)
    h, eye = 1e-6, np.eye(len(q0))
    g_fd = np.array([(cf(q0 + h * e) - cf(q0 - h * e)) / (2 * h) for e in eye])
    err, tol = float(np.abs(g - g_fd).max()), EPS * n * c / h + 1e-7 * float(np.abs(g).max())
    print(f"irb140 split on the device: c {c:.6f} |g|_inf {np.abs(g).max():.4f} |g - g_fd|_inf {err:.2e} (tolerance {tol:.2e})")
    assert err <= tol, (err, tol)


# ---- 7. what it buys -----------------------------------------------------------------------------

def test_what_it_buys():
    """tests/test_free_space.py's scene on the device: the frame is the raycast of the table
    with the box B far outside the view; the estimate has B between camera and table.
    (a) Without free space B's seven gradient entries are exactly 0.0 and estimate_state leaves
    its states bit-unchanged. (b) With free space the start has at least 32 samples with
    d* < 0, B's translation gradient is nonzero, the LM host loop's accepted costs decrease, and
    the free-space cost Σ_free min(d*, 0)² is at most half its start within 20 evaluations —
    the conditions the CPU run meets (CPU_FREE_COST)."""
    import flash
    from flash.depthsensors import DepthFrame, raycast_depths
    from flash.gradientdescent import CostFunctor, unflatten
    from flash.tracking import estimate_state
    m, x_true, x_start, sensor, tform, fs, sl = free_space_scene()
    state = flash.ManipulatorState(m)
    unflatten(state, x_true)
    depth = raycast_depths(flash.skin(state), sensor, tform)
    assert (~np.isnan(depth)).sum() > 500
    # (a)
    cf = CostFunctor(m, DepthFrame(depth, sensor, tform))
    assert cf.n_surface == cf.n_points == (~np.isnan(depth)).sum()
    g = cf.value_and_gradient(x_start)[1]
    assert (g[sl] == 0.0).all()
    x = estimate_state(m, DepthFrame(depth, sensor, tform), x_start)
    assert np.array_equal(x[sl], x_start[sl])
    # (b)
    frame = DepthFrame(depth, sensor, tform, free_space=fs)
    cf = CostFunctor(m, frame)
    ns, n = cf.n_surface, cf.n_points
    assert ns == (~np.isnan(depth)).sum() and n > ns and (n - ns) % fs.samples == 0
    assert np.array_equal(cf.depth_pixels(), frame.points()[1])

    def free_cost(x):
        d = cf.per_point(x)[1]
        return int((d[ns:] < 0).sum()), float((np.minimum(d[ns:], 0.0) ** 2).sum())

    inside, free0 = free_cost(x_start)
    assert inside >= 32
    c, g = cf.value_and_gradient(x_start)
    assert np.abs(g[sl.start + 4: sl.stop]).max() > 0
    x, seen, accepted = lm_accepted_costs(cf.value_gradient_hessian, x_start, n)
    x_native, f_native, its, _ = cf.descend_lm(x_start, 20, 1e-3, 0.5, 0.0, n)
    assert its == len(seen) <= 20 and np.array_equal(x_native, x) and f_native == accepted[-1] / n
    _, free1 = free_cost(x)
    print(f"free-space scene (GPU): n {n} ({ns} observed), inside at start {inside}, cost {seen[0]:.6e} -> "
          f"{accepted[-1]:.6e}, free-space cost {free0:.6e} -> {free1:.6e} in {len(seen)} evaluations "
          f"(CPU: {CPU_FREE_COST[0]:.6e} -> {CPU_FREE_COST[1]:.6e})")
    assert all(b < a for a, b in zip(accepted, accepted[1:])) and len(accepted) >= 3
    assert free1 <= 0.5 * free0
    # estimate_state takes the frame as it is: N is the resident point count, samples included
    from flash.tracking import LevenbergMarquardt
    s = LevenbergMarquardt(len(x_start), iteration_limit=20, gradient_convergence_tolerance=0.0)
    # (a functor of its own: its first pass may run another layout, so to rounding)
    assert np.abs(estimate_state(m, frame, x_start, solver=s) - x).max() <= 1e-9
