"""GPU: a context's device buffers are grown, kept and exchanged as clouds and
models come and go. Whatever a long-lived context held before, it evaluates
exactly as a fresh context given only the final model and cloud does (every
comparison is exact equality unless stated)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

# around the 64-point chunk and the 4-chunk padding of the chunk-sphere array; grow, shrink, grow
SIZES = (0, 1, 63, 64, 65, 255, 257, 1025, 64, 0, 257)


@pytest.fixture(scope="module")
def irb_scene():
    """IRB140: hull specs, poses, and a pool of points the clouds are cut from."""
    import flash
    from flash import Models, synthetic
    m = Models.irb140()
    q_true, q_eval = synthetic.perturbed_configuration(m, 21)
    pool = synthetic.depth_cloud(m, q_true, 4096, seed=22)
    hulls = [("hull", (s.hull.vertices, s.hull.faces, s.hull.planes)) for s in m.surfaces]
    return hulls, flash.hull_poses(m, q_eval), pool


@pytest.fixture(scope="module")
def rbf_scene():
    """BASELINE config 5 (IRB140 and a squishable RBF skin): surfaces, poses, rows, points."""
    from flash import Models
    from flash.core import ConvexGeometry
    z = np.load(os.path.join(GOLDEN, "c5_scene.npz"))
    m = Models.irb_and_squishable()[0]
    surfaces = [("hull", (s.hull.vertices, s.hull.faces, s.hull.planes)) if isinstance(s, ConvexGeometry)
                else ("rbf", len(s.surface_points) + len(s.skeleton_points)) for s in m.surfaces]
    return surfaces, z["poses"], z["rbf_rows"], z["points"][:700]


def _context(surfaces, precision=64, sort_points=False, rbf_rows=None):
    from flash import _lib
    c = _lib.Context(device=0, precision=precision, sort_points=sort_points)
    c.set_surfaces(surfaces)
    if rbf_rows is not None:
        c.set_rbf_params(rbf_rows)
    return c


def _assert_same(got, want):
    (c0, a0, p0), (c1, a1, p1) = got, want
    assert c0 == c1 and np.array_equal(a0, a1)
    for u, v in zip(p0, p1):
        assert np.array_equal(u, v)


def _cloud(pool, step, n):
    """Other points at every step: a stale buffer cannot pass for the new cloud."""
    return pool[97 * step:97 * step + n]


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("sort_points", [True, False])
def test_grow_shrink_grow(irb_scene, precision, sort_points):
    """One context walks set_points through SIZES, then the same walk through
    prefetch_points / set_points_prefetched (the current and the next cloud's
    buffers swap while their capacities differ), then through set_points_range
    with a range smaller than the cloud. After every step the pass with
    per-point outputs equals a fresh context's."""
    hulls, poses, pool = irb_scene
    ctx = _context(hulls, precision, sort_points)

    def check(load, n):
        load(ctx)
        assert ctx.n == n
        ref = _context(hulls, precision, sort_points)
        load(ref)
        _assert_same(ctx.eval(poses, True), ref.eval(poses, True))
        assert np.array_equal(ctx.permutation(), ref.permutation())
        ref.close()

    for step, n in enumerate(SIZES):
        check(lambda c: c.set_points(_cloud(pool, step, n)), n)

    def prefetched(pts):
        def load(c):
            c.prefetch_points(pts)
            if c is ctx and len(pts) % 2:
                c.eval(poses)  # (a pass of the current frame issues the copy and sort behind it)
            c.set_points_prefetched()
        return load
    for step, n in enumerate(SIZES):
        check(prefetched(_cloud(pool, 11 + step, n)), n)
    for step, n in enumerate(SIZES):
        whole = _cloud(pool, 22 + step, n + 41)
        check(lambda c: c.set_points_range(whole, 7, 7 + n), n)
    ctx.close()


@pytest.mark.parametrize("precision", [64, 32])
def test_model_replaced_in_place(irb_scene, rbf_scene, precision):
    """set_surfaces on one context: hull-only, an RBF scene (in an f32 context its
    f32 rows are a buffer apart from the f64 ones), hull-only with fewer hulls;
    each followed by set_points and a pass equal to a fresh context's. The
    partition limits set before the first model are still reported after the last."""
    hulls, poses, pool = irb_scene
    surfaces, rbf_poses, rbf_rows, rbf_pts = rbf_scene
    ctx = _context(hulls, precision, sort_points=True)
    ctx.set_partition(1234, 5678)
    stages = ((hulls, None, poses, pool[:1000]),
              (surfaces, rbf_rows, rbf_poses, rbf_pts),
              (hulls[:3], None, poses[:3], pool[1000:1300]))
    for i, (surf, rows, P, pts) in enumerate(stages):
        if i:
            ctx.set_surfaces(surf)
        if rows is not None:
            ctx.set_rbf_params(rows)
        ctx.set_points(pts)
        ref = _context(surf, precision, sort_points=True, rbf_rows=rows)
        ref.set_points(pts)
        _assert_same(ctx.eval(P, True), ref.eval(P, True))
        ref.close()
    assert ctx.get_partition(0)[:2] == (1234, 5678)
    ctx.close()


def test_regroup_after_reuse(irb_scene):
    """A sorted context that has held a larger cloud loads a smaller one: pass,
    fsdf_regroup_points (the cloud buffer swaps with the sort scratch's), pass.
    Per-point outputs before and after are equal; the accumulator differs in
    rounding only (1e-9 relative, the bound of test_gpu_solver.py::
    test_auto_regroup_descend_matches_unregrouped for regrouped against
    unregrouped sums). A larger cloud then grows the buffer that came back from
    the scratch."""
    hulls, poses, pool = irb_scene
    ctx = _context(hulls, 64, sort_points=True)
    ctx.set_points(pool[:1025])
    ctx.eval(poses)
    small, large = pool[1100:1400], pool[1500:3700]
    ctx.set_points(small)
    c0, a0, p0 = ctx.eval(poses, True)
    perm0 = ctx.permutation()
    ctx.regroup_points()
    c1, a1, p1 = ctx.eval(poses, True)
    assert np.array_equal(np.sort(ctx.permutation()), np.sort(perm0))
    for u, v in zip(p0, p1):
        assert np.array_equal(u, v)
    assert abs(c1 - c0) <= 1e-9 * abs(c0)
    assert np.all(np.abs(a1 - a0) <= 1e-9 * np.maximum(np.abs(a0), 1.0)), np.abs(a1 - a0).max()
    ref = _context(hulls, 64, sort_points=True)
    ref.set_points(small)
    _assert_same((c0, a0, p0), ref.eval(poses, True))
    ctx.set_points(large)
    ref.set_points(large)
    want = ref.eval(poses, True)
    _assert_same(ctx.eval(poses, True), want)
    ctx.regroup_points()  # (and back: the scratch now holds the first exchange's buffer)
    for u, v in zip(ctx.eval(poses, True)[2], want[2]):
        assert np.array_equal(u, v)
    ref.close()
    ctx.close()


def test_create_and_destroy(irb_scene):
    """Eight contexts in turn, at most two alive at once, each with a model, a
    cloud and one pass: the last one's results equal the first's."""
    hulls, poses, pool = irb_scene
    results, prev = [], None
    for _ in range(8):
        c = _context(hulls, 64, sort_points=True)
        if prev is not None:
            prev.close()
        c.set_points(pool[:777])
        results.append(c.eval(poses, True))
        prev = c
    prev.close()
    _assert_same(results[-1], results[0])
