"""Voxel-grid downsampling on the CPU (flash.depthdata.voxel_downsample, the
numpy twin of csrc/voxel.hip; flash.VoxelGrid): the twin against an independent
restatement in plain Python — math.floor, a dict keyed by cell, sequential
float adds: no code shared with the twin —, bit for bit; the properties of the
definition (include/flashsdf.h "voxel grid"); and the grid's validation."""
import math

import numpy as np
import pytest

from conftest import rng

LO, HI = -(1 << 20), (1 << 20) - 1


def _plain(points, size, origin):
    """The definition over Python floats (IEEE doubles): per point the cell by
    math.floor of the quotient, clamped; cells kept in a dict with their members
    in input order; voxels sorted by (cz, cy, cx) — the key's order; the
    centroid by sequential adds, then one division."""
    cells, dropped, where = {}, 0, []
    for i, p in enumerate(points):
        x = [float(v) for v in p]
        if not all(math.isfinite(v) for v in x):
            dropped += 1
            where.append(None)
            continue
        c = []
        for v, o in zip(x, origin):
            t = (v - o) / size
            q = LO if t < LO else (HI if t > HI else math.floor(t))  # (t may be ±inf: x − o overflowed)
            c.append(min(max(int(q), LO), HI))
        c = tuple(c)
        cells.setdefault(c, []).append(i)
        where.append(c)
    order = sorted(cells, key=lambda c: (c[2], c[1], c[0]))
    xyz, count, first = [], [], []
    for c in order:
        members = cells[c]
        acc = [float(v) for v in points[members[0]]]
        for i in members[1:]:
            acc = [a + float(v) for a, v in zip(acc, points[i])]
        xyz.append([a / float(len(members)) for a in acc])
        count.append(len(members))
        first.append(members[0])
    rank = {c: v for v, c in enumerate(order)}
    vop = [-1 if c is None else rank[c] for c in where]
    return (np.array(xyz, np.float64).reshape(-1, 3), np.array(count, np.int32),
            np.array(order, np.int32).reshape(-1, 3), np.array(first, np.int64), np.array(vop, np.int32), dropped)


def _same(points, grid):
    from flash.depthdata import voxel_downsample
    got = voxel_downsample(points, grid)
    want = _plain(np.asarray(points, np.float64).reshape(-1, 3), grid.size, grid.origin)
    names = ("xyz", "count", "cell", "first", "voxel_of_point")
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape, name
        if name == "xyz":
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), name  # (bits: −0.0 and 0.0 differ)
        else:
            assert np.array_equal(g, w), name
    assert got[5] == want[5]
    assert got[1].dtype == np.int32 and got[2].dtype == np.int32 and got[4].dtype == np.int32
    return got


def _properties(points, grid, out):
    """What the definition promises, checked on the twin's output."""
    xyz, count, cell, first, vop, dropped = out
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n, m = len(p), len(xyz)
    assert count.sum() == n - dropped and (count >= 1).all()
    assert dropped == (~np.isfinite(p).all(axis=1)).sum()
    key = ((cell[:, 2].astype(np.int64) + (1 << 20)) << 42) | ((cell[:, 1].astype(np.int64) + (1 << 20)) << 21) | \
        (cell[:, 0].astype(np.int64) + (1 << 20))
    assert (np.diff(key) > 0).all()  # strictly ascending: one voxel per cell, in key order
    assert (vop[~np.isfinite(p).all(axis=1)] == -1).all()
    for v in range(m):
        members = np.flatnonzero(vop == v)
        assert len(members) == count[v] and first[v] == members.min()
    # voxel_of_point agrees with the cells: every kept point's own cell is its voxel's
    h, o = grid.size, np.array(grid.origin)
    kept = np.flatnonzero(vop >= 0)
    with np.errstate(over="ignore"):
        own = np.clip(np.floor((p[kept] - o) / h), LO, HI).astype(np.int32)
    assert np.array_equal(own, cell[vop[kept]])
    # a centroid lies in its cell's closed box widened by 4 ulp of the coordinate (cells that are
    # not clamped: a clamped cell collects everything beyond it)
    inner = ((cell > LO) & (cell < HI)).all(axis=1)
    lo_edge, hi_edge = o + cell * h, o + (cell + 1.0) * h
    slack = 4.0 * np.spacing(np.maximum(np.abs(xyz), np.maximum(np.abs(lo_edge), np.abs(hi_edge))))
    assert (xyz[inner] >= (lo_edge - slack)[inner]).all() and (xyz[inner] <= (hi_edge + slack)[inner]).all()


@pytest.mark.parametrize("seed", range(4))
def test_random_clouds(seed):
    from flash import VoxelGrid
    r = rng(seed)
    n = (1, 17, 400, 2500)[seed]
    pts = r.normal(size=(n, 3)) * [0.6, 0.3, 1.1] + [0.2, -0.1, 0.8]
    for h in (0.01, 0.07, 0.5, 10.0):
        grid = VoxelGrid(h)
        _properties(pts, grid, _same(pts, grid))


def test_points_on_cell_faces():
    """x = k · h for k of both signs: floor against truncation, and the
    quotient's rounding ((k · h) / h is not always k)."""
    from flash import VoxelGrid
    for h in (0.1, 0.005, 1.0 / 3.0, 0.7):
        k = np.arange(-40, 41)
        pts = np.stack([k * h, (k[::-1] + 0.5) * h, np.nextafter(k * h, -np.inf)], axis=1)
        grid = VoxelGrid(h)
        out = _same(pts, grid)
        _properties(pts, grid, out)
        pts = np.stack([k * h, np.zeros(len(k)), np.zeros(len(k))], axis=1)
        out = _same(pts, grid)
        _properties(pts, grid, out)
        # negative coordinates floor down: −h/2 lies in cell −1, not 0
        cells = _same(np.array([[-0.5 * h, 0.5 * h, -1.5 * h]]), grid)[2]
        assert cells.tolist() == [[-1, 0, -2]]


def test_nonzero_origin():
    from flash import VoxelGrid
    pts = rng(5).uniform(-1.0, 1.0, size=(700, 3))
    for origin in ((0.013, -0.4, 7.0), (-1.0, -1.0, -1.0), (1e6, 0.0, -1e-9)):
        grid = VoxelGrid(0.05, origin)
        _properties(pts, grid, _same(pts, grid))
    # the grid is anchored at the origin: shifting both by a whole number of cells keeps the cells' contents
    a = _same(pts, VoxelGrid(0.25, (0.0, 0.0, 0.0)))
    b = _same(pts + 0.5, VoxelGrid(0.25, (0.5, 0.5, 0.5)))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4])


def test_clamped_cells():
    from flash import VoxelGrid
    h = 1e-3
    far = (1 << 20) * h
    pts = np.array([[far * 4, 0, 0], [far * 9, 0, 0], [-far * 3, 0, 0], [-far * 8, 0, 0], [far - h / 2, 0, 0],
                    [-far + h / 2, 0, 0], [1e300, -1e300, 1.7e308], [far, far, far], [-far, -far, -far],
                    [np.nextafter(-far, -np.inf), 0, 0]], np.float64)
    grid = VoxelGrid(h)
    out = _same(pts, grid)
    _properties(pts, grid, out)
    cell = out[2][out[4]]
    assert cell[0, 0] == cell[1, 0] == HI and cell[2, 0] == cell[3, 0] == LO  # the far points share the last cells
    assert cell[4, 0] == HI and cell[5, 0] == LO
    assert cell[6].tolist() == [HI, LO, HI]
    assert cell[7].tolist() == [HI, HI, HI] and cell[8].tolist() == [LO, LO, LO] and cell[9, 0] == LO
    # x − o overflows to ±inf for a finite point: still a finite point, clamped
    out = _same(np.array([[1.7e308, -1.7e308, 0.0]]), VoxelGrid(1.0, (-1.7e308, 1.7e308, 0.0)))
    assert out[2].tolist() == [[HI, LO, 0]] and out[5] == 0


def test_non_finite_points_are_dropped():
    from flash import VoxelGrid
    pts = rng(6).uniform(-0.3, 0.3, size=(40, 3))
    pts[0, 1] = np.nan
    pts[7] = [np.inf, 0.0, 0.0]
    pts[8] = [0.0, -np.inf, 0.0]
    pts[39, 2] = np.nan
    pts[20] = [np.nan, np.inf, -np.inf]
    grid = VoxelGrid(0.1)
    out = _same(pts, grid)
    _properties(pts, grid, out)
    assert out[5] == 5 and (out[4][[0, 7, 8, 20, 39]] == -1).all() and (np.delete(out[4], [0, 7, 8, 20, 39]) >= 0).all()
    # every point dropped, and the alternating pattern
    allbad = np.full((9, 3), np.nan)
    out = _same(allbad, grid)
    assert len(out[0]) == 0 and out[5] == 9 and (out[4] == -1).all()
    alt = rng(7).uniform(-0.3, 0.3, size=(64, 3))
    alt[::2, 0] = np.inf
    out = _same(alt, grid)
    _properties(alt, grid, out)
    assert out[5] == 32


def test_duplicates():
    from flash import VoxelGrid
    base = rng(8).uniform(-0.5, 0.5, size=(50, 3))
    pts = np.concatenate([base, base[::2], base[::5], base[:1]])[rng(9).permutation(50 + 25 + 10 + 1)]
    grid = VoxelGrid(1e-6)  # (only duplicates share a cell; 2^20 cells each way still cover the cloud)
    out = _same(pts, grid)
    _properties(pts, grid, out)
    assert len(out[0]) == 50 and out[1].sum() == 86
    # (p + p) / 2 == p exactly: the twice-present points' centroids are the points
    twice = out[1] == 2
    assert twice.any() and np.array_equal(out[0][twice], pts[out[3][twice]])


def test_empty_cloud():
    from flash import VoxelGrid
    out = _same(np.zeros((0, 3)), VoxelGrid(0.1))
    assert out[0].shape == (0, 3) and out[1].shape == (0,) and out[2].shape == (0, 3) and out[3].shape == (0,)
    assert out[4].shape == (0,) and out[5] == 0


def test_left_fold_order():
    """The centroid's bits are the input-order left fold's: a cell whose sum
    depends on the order of its adds."""
    from flash import VoxelGrid
    from flash.depthdata import voxel_downsample
    pts = np.array([[1e16, 0.5, 0.5], [1.0, 0.5, 0.5], [-1e16, 0.5, 0.5], [1.0, 0.5, 0.5]])
    grid = VoxelGrid(1e17, (-5e16, 0.0, 0.0))
    out = _same(pts, grid)
    assert out[1].tolist() == [4]
    assert out[0][0, 0] == (((1e16 + 1.0) + -1e16) + 1.0) / 4.0 == 0.25  # (the exact mean is 0.5)
    back = voxel_downsample(pts[[1, 3, 0, 2]], grid)
    assert back[0][0, 0] == (((1.0 + 1.0) + 1e16) + -1e16) / 4.0 == 0.5  # (another input order: another fold)


def test_frame_voxel_points_is_twin_of_twin():
    from flash import VoxelGrid
    from flash.depthdata import voxel_downsample
    from flash.depthsensors import DepthFrame, FreeSpace, Kinect
    sensor = Kinect(12, 16)
    depth = rng(10).uniform(0.9, 2.0, size=(12, 16))
    depth[rng(11).uniform(size=(12, 16)) < 0.2] = np.nan
    grid = VoxelGrid(0.08, (0.01, 0.02, 0.03))
    for fs in (None, FreeSpace(samples=2, stride=3)):
        frame = DepthFrame(depth, sensor, None, 0.5, 3.0, free_space=fs)
        pts, pix = frame.points()
        ns = frame.n_surface()
        xyz, count, _, first, _, dropped = voxel_downsample(pts[:ns], grid)
        vp, vpix, vw = frame.voxel_points(grid)
        assert dropped == 0 and len(xyz) < ns
        assert np.array_equal(vp, np.concatenate([xyz, pts[ns:]]))
        assert np.array_equal(vpix, np.concatenate([pix[:ns][first], pix[ns:]]))
        assert np.array_equal(vw, np.concatenate([count.astype(float), np.ones(len(pts) - ns)]))
        assert np.array_equal(frame.points()[0], pts)  # (points() stays the frame without a grid)


def test_voxel_grid_validation():
    import flash
    from flash import VoxelGrid
    g = VoxelGrid(0.05)
    assert g.size == 0.05 and g.origin == (0.0, 0.0, 0.0) and g.weights == "count" and g.mode == 1
    g = VoxelGrid(2, origin=np.array([1, 2, 3]), weights="unit")
    assert g.size == 2.0 and g.origin == (1.0, 2.0, 3.0) and g.mode == 0
    assert isinstance(g.size, float) and all(isinstance(v, float) for v in g.origin)
    assert flash.VoxelGrid is flash.DepthData.VoxelGrid and "VoxelGrid" in flash.__all__
    with pytest.raises(Exception):
        g.size = 1.0  # frozen
    for bad in (0.0, -0.1, np.nan, np.inf, -np.inf, True, "x", None):
        with pytest.raises(ValueError):
            VoxelGrid(bad)
    for bad in ((0.0, 0.0), (0.0, 0.0, 0.0, 0.0), (np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), "abc", None):
        with pytest.raises(ValueError):
            VoxelGrid(0.1, origin=bad)
    for bad in ("counts", "", None, 1):
        with pytest.raises(ValueError):
            VoxelGrid(0.1, weights=bad)
