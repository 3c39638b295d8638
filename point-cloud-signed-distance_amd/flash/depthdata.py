"""module Flash.DepthData (src/depthdata.jl) — point-cloud ingest.

read_point_cloud(file) (:19-30): line 1 is the camera origin "x, y, z"; every
following line is "x, y, z, r, g, b" (comma separated, readdlm). Returns a
PointCloud (camera_origin, positions [n,3], colors [n,3]). As in the
reference, rows without colour columns are an error (:27 indexes columns 4-6;
box_on_table_points.txt is xyz-only and fails there too). LCMGL rendering
(:32-46) is out of scope.
"""
from __future__ import annotations

import io
import os
from dataclasses import dataclass

import numpy as np


@dataclass
class PointCloud:
    camera_origin: np.ndarray
    positions: np.ndarray  # [n,3] float64
    colors: np.ndarray     # [n,3] float64 (RGB in [0,1])

    def __repr__(self):
        o = ", ".join(repr(float(v)) for v in self.camera_origin)
        return f"PointCloud with origin: [{o}] containing {len(self.positions)} points"

    def __len__(self):
        return len(self.positions)


def read_point_cloud(file) -> PointCloud:
    """Path or text file object -> PointCloud."""
    if isinstance(file, (str, os.PathLike)):
        with open(file) as f:
            return read_point_cloud(f)
    origin_line = file.readline()
    origin = np.array([float(c) for c in origin_line.split(",")[:3]], np.float64)
    rest = file.read()
    data = np.loadtxt(io.StringIO(rest), delimiter=",", dtype=np.float64, ndmin=2) if rest.strip() else np.zeros((0, 6))
    if data.shape[1] < 6:
        raise ValueError(f"read_point_cloud: rows have {data.shape[1]} columns, expected x,y,z,r,g,b")
    return PointCloud(origin, np.ascontiguousarray(data[:, :3]), np.ascontiguousarray(data[:, 3:6]))


def subsample(points: np.ndarray, step: int = 200) -> np.ndarray:
    """msg[:points][1:200:end] (examples/irb_and_squishable.ipynb cell 12)."""
    return np.ascontiguousarray(np.asarray(points)[::step])


@dataclass(frozen=True)
class VoxelGrid:
    """A world-anchored voxel grid that thins a cloud before the solver sees it
    (fsdf_set_voxel_grid; not in the reference, which takes every 200th point):
    one centroid per occupied cell of side `size` (finite, > 0; the units of the
    points), cells counted from `origin`. weights "count": the cell's population
    becomes the centroid's point weight, so Σ a ρ(d*) approximates the full
    cloud's objective; "unit": every centroid counts 1. estimate_state, Tracker,
    track and CostFunctor take it as `voxel=`; voxel_downsample is the
    arithmetic."""
    size: float
    origin: tuple = (0.0, 0.0, 0.0)
    weights: str = "count"

    WEIGHT_MODES = {"unit": 0, "count": 1}  # FSDF_VOXEL_UNIT, FSDF_VOXEL_COUNT

    def __post_init__(self):
        try:
            size = float(self.size)
        except (TypeError, ValueError):
            raise ValueError(f"VoxelGrid: size must be a number, got {self.size!r}") from None
        if isinstance(self.size, bool) or not (np.isfinite(size) and size > 0.0):
            raise ValueError(f"VoxelGrid: size must be finite and > 0, got {self.size!r}")
        try:
            origin = tuple(float(v) for v in np.asarray(self.origin, np.float64).reshape(-1))
        except (TypeError, ValueError):
            raise ValueError(f"VoxelGrid: origin must be 3 numbers, got {self.origin!r}") from None
        if len(origin) != 3 or not all(np.isfinite(v) for v in origin):
            raise ValueError(f"VoxelGrid: origin must be 3 finite numbers, got {self.origin!r}")
        if self.weights not in self.WEIGHT_MODES:
            raise ValueError(f"VoxelGrid: weights must be 'count' or 'unit', got {self.weights!r}")
        object.__setattr__(self, "size", size)
        object.__setattr__(self, "origin", origin)

    @property
    def mode(self) -> int:
        """FSDF_VOXEL_UNIT / FSDF_VOXEL_COUNT as fsdf_set_voxel_grid takes it."""
        return self.WEIGHT_MODES[self.weights]


VOXEL_CELL_MIN, VOXEL_CELL_MAX = -(1 << 20), (1 << 20) - 1


def voxel_downsample(points, grid: VoxelGrid):
    """The voxel centroids of a cloud -> (xyz [m, 3], count [m] int32, cell
    [m, 3] int32, first [m], voxel_of_point [n] int32, dropped): the numpy twin
    of fsdf_set_points_voxel (csrc/voxel.hip), the same bits. Per point and
    axis, in float64: q = floor((x − o) / h), the cell is q clamped to
    [−2^20, 2^20 − 1]; key = (c_z + 2^20) << 42 | (c_y + 2^20) << 21 |
    (c_x + 2^20). A point with a non-finite coordinate is dropped (counted in
    `dropped`, voxel_of_point −1). Voxels come in ascending key order, their
    points in ascending input index (a stable argsort of the keys); first[v] is
    the lowest input index in voxel v. The centroid is the left fold
    acc = p_first; acc = acc + p_next; ... in that order, then
    acc / float64(count) — vectorised as: round j adds the j-th member of every
    voxel that has one."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    n = len(p)
    h, o = np.float64(grid.size), np.array(grid.origin, np.float64)
    finite = np.isfinite(p).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor((p - o) / h)
    q = np.where(finite[:, None], np.clip(q, VOXEL_CELL_MIN, VOXEL_CELL_MAX), 0.0)
    u = (q.astype(np.int64) + (1 << 20)).astype(np.uint64)
    keys = (u[:, 2] << np.uint64(42)) | (u[:, 1] << np.uint64(21)) | u[:, 0]
    keys[~finite] = np.uint64(0xFFFFFFFFFFFFFFFF)
    order = np.argsort(keys, kind="stable")
    kept = int(finite.sum())
    order, ks = order[:kept], keys[order[:kept]]  # (the dropped points' keys sort last)
    head = np.ones(kept, bool)
    head[1:] = ks[1:] != ks[:-1]
    start = np.flatnonzero(head)
    m = len(start)
    count = np.diff(np.append(start, kept)).astype(np.int32)
    first = order[start]
    acc = p[first].copy()
    for j in range(1, int(count.max()) if m else 0):
        sel = np.flatnonzero(count > j)
        acc[sel] = acc[sel] + p[order[start[sel] + j]]
    xyz = acc / count.astype(np.float64)[:, None]
    kv = ks[start]
    mask = np.uint64(0x1FFFFF)
    cell = np.stack([(kv & mask), ((kv >> np.uint64(21)) & mask), ((kv >> np.uint64(42)) & mask)],
                    axis=1).astype(np.int64) - (1 << 20)
    voxel_of_point = np.full(n, -1, np.int32)
    voxel_of_point[order] = np.repeat(np.arange(m, dtype=np.int32), count)
    return xyz, count, cell.astype(np.int32).reshape(m, 3), first.astype(np.int64), voxel_of_point, n - kept


def kinect_to_pointcloud(x, y, z, num: int | None = None, utime: int = 0) -> dict:
    """The message conversion of convert_kinect_log_data.py:11-31 on arrays.

    A kinect.pointcloud_t (KINECT_POINTS_REDUCED) interleaves positions and
    colours in its x/y/z arrays: even indices are xyz, odd indices rgb. The
    bot_core.pointcloud_t it becomes holds n_points = num // 2 points
    (x[i], y[i], z[i]) for even i, and n_channels = 3 channels "r", "g", "b"
    whose values are x[i], y[i], z[i] for odd i. Returns that message as a dict
    (utime, n_points, points [n,3] f32, n_channels, channel_names, channels
    [3,n] f32). LCM wire encoding is out of scope: the lcmtypes are not part of
    the reference."""
    x, y, z = (np.asarray(v, np.float32) for v in (x, y, z))
    num = len(x) if num is None else int(num)
    pts = np.stack([x[0:num:2], y[0:num:2], z[0:num:2]], axis=1)
    chans = np.stack([v[1:num:2] for v in (x, y, z)])
    return {"utime": int(utime), "n_points": num // 2, "points": np.ascontiguousarray(pts), "n_channels": 3,
            "channel_names": ["r", "g", "b"], "channels": np.ascontiguousarray(chans)}


def pointcloud_positions(msg: dict, step: int = 200) -> np.ndarray:
    """[n,3] float64 positions of a bot_core.pointcloud_t dict, subsampled as
    msg[:points][1:200:end] (examples/irb_and_squishable.ipynb cell 12)."""
    return subsample(np.asarray(msg["points"], np.float64), step)
