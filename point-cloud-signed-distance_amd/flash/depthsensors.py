"""module Flash.DepthSensors (src/depthsensors.jl) — synthetic depth on the GPU.

  generateKinectRays(rows, cols, vfov, hfov)   :10-30  (camera-frame unit rays)
  Kinect(rows, cols, vfov, hfov)               :54
  rays_in_world(sensor, tform)                 :83-86
  raycast_depths(surface, sensor, tform)       :88-97  (doRaycast per ray, :56-81)
  raycast_points(surface, sensor, tform)       :99-113 (row-major, NaN rays dropped)
  raycast(state, sensor, tform)                :115-118
The per-ray secant march runs in raycast_kernel (fsdf_raycast), one lane per
ray, on the same scene SDF as the residual pass. LCMGL drawing (:36-52,
:120-135) is out of scope.

DepthFrame / depth_points (the reverse direction, a camera's frame coming in):
the depth image over the sensor's fixed rays and the sensor pose, which the
device back-projects and compacts itself (Context.set_sensor / set_depth,
csrc/depth.hip) in the order and arithmetic of raycast_points (:99-113);
depth_points is its numpy twin, bit for bit.

FreeSpace / free_space_points (not in the reference): what a depth image says
beyond its returns — the ray up to each return is empty, and a pixel with no
return saw nothing within range. A DepthFrame with `free_space` set sends
samples along its rays after the observed points (fsdf_set_free_space), which
the robust reduction penalises only where the model covers them
(include/flashsdf.h "free space"); free_space_points is the numpy twin.

depth_noise_weights (not in the reference): per-point confidence weights from
a structured-light sensor's axial noise model, for estimate_state / Tracker /
track (`weights=`).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .core import ManipulatorState, SceneSkin, skin
from .geometry import Transform


def generate_kinect_rays(rows: int, cols: int, vertical_fov: float = 0.4682, horizontal_fov: float = 0.5449):
    """[rows, cols, 3] unit rays. As in the reference, x uses tan(vertical_fov)/cx
    and y tan(horizontal_fov)/cy (the names are swapped there; kept)."""
    cx, cy = (cols + 1) / 2.0, (rows + 1) / 2.0
    tv, th = np.tan(vertical_fov), np.tan(horizontal_fov)
    v, u = np.meshgrid(np.arange(1, rows + 1), np.arange(1, cols + 1), indexing="ij")
    r = np.stack([(u - cx) * tv / cx, (v - cy) * th / cy, np.ones_like(u, dtype=np.float64)], axis=-1)
    return r / np.linalg.norm(r, axis=-1, keepdims=True)


@dataclass
class DepthSensor:
    rays: np.ndarray  # [rows, cols, 3], camera frame


def Kinect(rows: int, cols: int, vertical_fov: float = 0.4682, horizontal_fov: float = 0.5449) -> DepthSensor:
    return DepthSensor(generate_kinect_rays(rows, cols, vertical_fov, horizontal_fov))


def rays_in_world(sensor: DepthSensor, tform: Transform) -> np.ndarray:
    return sensor.rays @ tform.R.T


def raycast_depths(surface: SceneSkin, sensor: DepthSensor, tform: Transform) -> np.ndarray:
    """[rows, cols] depths (NaN = miss)."""
    rw = rays_in_world(sensor, tform)
    rw = rw / np.linalg.norm(rw, axis=-1, keepdims=True)  # normalize(rays[i]) (:93)
    d = surface.raycast(tform.t, rw.reshape(-1, 3))
    return d.reshape(sensor.rays.shape[:2])


def raycast_points(surface: SceneSkin, sensor: DepthSensor, tform: Transform) -> np.ndarray:
    """World points of every hit, row-major (:99-113)."""
    d = raycast_depths(surface, sensor, tform)
    hit = ~np.isnan(d)
    r = sensor.rays / np.linalg.norm(sensor.rays, axis=-1, keepdims=True)
    return tform.apply(d[hit][:, None] * r[hit])


def raycast(state: ManipulatorState, sensor: DepthSensor, tform: Transform, device: int = 0) -> np.ndarray:
    return raycast_points(skin(state, device), sensor, tform)


def pixel_directions(sensor_rays, kind: str = "range") -> np.ndarray:
    """One direction u per pixel [rows·cols, 3] as fsdf_set_sensor forms it,
    operation for operation: kind "range" u = r / sqrt((x·x + y·y) + z·z), each
    component divided; "z" u = (x / z, y / z, 1.0)."""
    r = np.asarray(sensor_rays, np.float64)
    if r.ndim != 3 or r.shape[2] != 3:
        raise ValueError(f"pixel_directions: rays must be [rows, cols, 3], got {r.shape}")
    r = r.reshape(-1, 3)
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    if not np.all(np.isfinite(r)):
        raise ValueError("pixel_directions: rays must be finite")
    if kind == "range":
        nrm = np.sqrt((x * x + y * y) + z * z)
        if not np.all(np.isfinite(nrm) & (nrm > 0.0)):
            raise ValueError("pixel_directions: a ray has no length")
        return np.stack([x / nrm, y / nrm, z / nrm], axis=1)
    if kind == "z":
        if not np.all(z > 0.0):
            raise ValueError("pixel_directions: kind 'z' needs rays with z > 0")
        return np.stack([x / z, y / z, np.ones_like(z)], axis=1)
    raise ValueError(f"pixel_directions: kind must be 'range' or 'z', got {kind!r}")


def depth_points(depth, sensor_rays, tform: Transform | None, near: float = 0.0, far: float = np.inf,
                 scale: float = 1.0, kind: str = "range"):
    """The cloud of a depth image -> (points [n, 3], pixels [n]): the numpy twin
    of fsdf_set_depth_* (csrc/depth.hip), the same bits. depth [rows, cols]
    (float64, float32 or uint16) over sensor_rays [rows, cols, 3]; tform the
    sensor in the world (None: identity). Per pixel, in this operation order
    (explicit column arithmetic — a BLAS product may fuse or reorder):
      s = scale · float64(depth); valid iff s finite, s > 0, near <= s <= far
      c = (s u_x, s u_y, s u_z), u = pixel_directions(sensor_rays, kind)
      p_j = ((R_j0 c_x + R_j1 c_y) + R_j2 c_z) + t_j
    The valid pixels in row-major order (src/depthsensors.jl:99-113
    raycast_points: misses dropped); pixels[i] = row · cols + col of point i."""
    d = np.asarray(depth)
    if d.dtype not in (np.dtype(np.float64), np.dtype(np.float32), np.dtype(np.uint16)):
        raise TypeError(f"depth_points: the image is float64, float32 or uint16, got {d.dtype}")
    u = pixel_directions(sensor_rays, kind)
    if d.size != len(u):
        raise ValueError(f"depth_points: an image of {d.size} pixels over {len(u)} rays")
    near, far, scale = np.float64(near), np.float64(far), np.float64(scale)
    if np.isnan(near) or np.isnan(far) or near > far:
        raise ValueError(f"depth_points: range [{near}, {far}] (near <= far, neither a NaN)")
    if not (np.isfinite(scale) and scale > 0.0):
        raise ValueError(f"depth_points: scale {scale} (finite and > 0)")
    R = np.eye(3) if tform is None else np.asarray(tform.R, np.float64)
    t = np.zeros(3) if tform is None else np.asarray(tform.t, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = scale * d.reshape(-1).astype(np.float64)
        valid = np.isfinite(s) & (s > 0.0) & (s >= near) & (s <= far)
    pixels = np.flatnonzero(valid).astype(np.int32)
    s = s[valid]
    cx, cy, cz = s * u[valid, 0], s * u[valid, 1], s * u[valid, 2]
    points = np.empty((len(s), 3), np.float64)
    for j in range(3):
        points[:, j] = ((R[j, 0] * cx + R[j, 1] * cy) + R[j, 2] * cz) + t[j]
    return points, pixels


@dataclass(frozen=True)
class FreeSpace:
    """The free-space samples of a depth frame (fsdf_set_free_space): `samples`
    = J points (1..16) per sending pixel, on every `stride`-th row and column.
    A valid pixel's free length is L = s − gap (gap: the margin kept in front
    of the return, a few noise sigmas); a miss's — no return: NaN, <= 0, beyond
    far, +inf, but not a too-near reading — is `miss_range` when that is > 0.
    A pixel sends its J samples at ranges L − (j − 1) · spacing, j = 1..J, iff
    the last one is > 0. Lengths are in the units of s = scale · depth (z units
    for kind "z")."""
    samples: int = 4
    stride: int = 1
    gap: float = 0.02
    spacing: float = 0.05
    miss_range: float = 0.0

    def __post_init__(self):
        if isinstance(self.samples, bool) or int(self.samples) != self.samples or not 1 <= self.samples <= 16:
            raise ValueError(f"FreeSpace: samples must be an integer in 1..16, got {self.samples!r}")
        if isinstance(self.stride, bool) or int(self.stride) != self.stride or self.stride < 1:
            raise ValueError(f"FreeSpace: stride must be an integer >= 1, got {self.stride!r}")
        for name in ("gap", "spacing", "miss_range"):
            v = float(getattr(self, name))
            if not (np.isfinite(v) and v >= 0.0):
                raise ValueError(f"FreeSpace: {name} must be finite and >= 0, got {v!r}")
        if self.samples > 1 and not float(self.spacing) > 0.0:
            raise ValueError(f"FreeSpace: spacing must be > 0 with more than one sample, got {self.spacing!r}")

    @property
    def lengths(self) -> np.ndarray:
        """{gap, spacing, miss_range} as fsdf_set_free_space takes them."""
        return np.array([self.gap, self.spacing, self.miss_range], np.float64)


def free_space_points(depth, sensor_rays, tform: Transform | None, near: float = 0.0, far: float = np.inf,
                      scale: float = 1.0, kind: str = "range", free_space: FreeSpace | None = None):
    """The cloud of a depth image with its free-space samples -> (points [n, 3],
    pixels [n]): the numpy twin of fsdf_set_depth_* under fsdf_set_free_space
    (csrc/depth.hip), the same bits. The first n_surface = (number of valid
    pixels) rows are depth_points'; then, with J = free_space.samples and m
    sending pixels, sample j of the r-th sending pixel (row-major) at row
    n_surface + (j − 1) · m + r. Per pixel on the stride grid, in this
    operation order (explicit column arithmetic, as depth_points):
      L = s − gap (valid) | miss_range (a miss: not valid and not
          (s > 0 and s < near), when miss_range > 0) | the pixel sends nothing
      sends iff L − float64(J − 1) · spacing > 0
      t = L − float64(j − 1) · spacing; c = (t u_x, t u_y, t u_z)
      p_k = ((R_k0 c_x + R_k1 c_y) + R_k2 c_z) + t_k
    free_space None: depth_points."""
    points, pixels = depth_points(depth, sensor_rays, tform, near, far, scale, kind)
    if free_space is None:
        return points, pixels
    fs = free_space
    d = np.asarray(depth)
    rays = np.asarray(sensor_rays, np.float64)
    rows, cols = rays.shape[:2]
    u = pixel_directions(sensor_rays, kind)
    near, far, scale = np.float64(near), np.float64(far), np.float64(scale)
    gap, spacing, miss = np.float64(fs.gap), np.float64(fs.spacing), np.float64(fs.miss_range)
    J = int(fs.samples)
    R = np.eye(3) if tform is None else np.asarray(tform.R, np.float64)
    t = np.zeros(3) if tform is None else np.asarray(tform.t, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = scale * d.reshape(-1).astype(np.float64)
        valid = np.isfinite(s) & (s > 0.0) & (s >= near) & (s <= far)
        too_near = (s > 0.0) & (s < near)
        is_miss = ~valid & ~too_near & (miss > 0.0)
        L = np.where(valid, s - gap, miss)
        i = np.arange(rows * cols)
        grid = ((i // cols) % fs.stride == 0) & ((i % cols) % fs.stride == 0)
        sends = grid & (valid | is_miss) & (L - np.float64(J - 1) * spacing > 0.0)
    send_pix = np.flatnonzero(sends).astype(np.int32)
    m = len(send_pix)
    L, us = L[sends], u[sends]
    out = np.empty((len(points) + J * m, 3), np.float64)
    out[:len(points)] = points
    for j in range(J):
        tt = L - np.float64(j) * spacing
        cx, cy, cz = tt * us[:, 0], tt * us[:, 1], tt * us[:, 2]
        blk = out[len(points) + j * m: len(points) + (j + 1) * m]
        for k in range(3):
            blk[:, k] = ((R[k, 0] * cx + R[k, 1] * cy) + R[k, 2] * cz) + t[k]
    return out, np.concatenate([pixels] + [send_pix] * J).astype(np.int32)


@dataclass
class DepthFrame:
    """One frame of a depth camera as it arrives: the image over a DepthSensor's
    fixed rays and the sensor's pose. estimate_state, Tracker.step, track and
    CostFunctor take it wherever they take a cloud; the device then
    back-projects and compacts it (Context.set_depth) and the host never forms
    the points unless something asks for them (points())."""
    depth: np.ndarray   # [rows, cols] float64, float32 or uint16
    sensor: DepthSensor
    tform: Transform | None = None  # the sensor in the world (None: identity)
    near: float = 0.0
    far: float = np.inf
    scale: float = 1.0
    kind: str = "range"
    free_space: FreeSpace | None = None  # free-space samples after the observed points (None: none)

    def points(self):
        """(points [n, 3], pixels [n]) by depth_points — with free_space set by
        free_space_points: the observed points followed by the samples —, the
        resident cloud's bits."""
        return free_space_points(self.depth, self.sensor.rays, self.tform, self.near, self.far, self.scale, self.kind,
                                 self.free_space)

    def voxel_points(self, grid):
        """(points [n, 3], pixels [n], weights [n]) of this frame under a
        depthdata.VoxelGrid, the resident cloud's bits (fsdf_set_depth_* with
        fsdf_set_voxel_grid): the observed points' voxel centroids
        (depthdata.voxel_downsample of depth_points) followed by the free-space
        samples unchanged; a voxel's pixel is its first point's; weights are the
        voxels' counts, then 1.0 per sample (what the library sets under
        "count"). points() itself stays the frame without a grid."""
        from .depthdata import voxel_downsample
        obs, pix = depth_points(self.depth, self.sensor.rays, self.tform, self.near, self.far, self.scale, self.kind)
        allp, allpix = self.points()
        xyz, count, _, first, _, _ = voxel_downsample(obs, grid)
        tail = len(allp) - len(obs)
        return (np.concatenate([xyz, allp[len(obs):]]), np.concatenate([pix[first], allpix[len(obs):]]).astype(np.int32),
                np.concatenate([count.astype(np.float64), np.ones(tail)]))

    def n_surface(self) -> int:
        """The number of observed points (valid pixels): the samples follow them."""
        return len(depth_points(self.depth, self.sensor.rays, self.tform, self.near, self.far, self.scale,
                                self.kind)[1])


def depth_noise_weights(points, origin, axis, sigma0: float = 0.0012, k: float = 0.0019, z0: float = 0.4):
    """Confidence weights (σ0 / σ(z))² in (0, 1] for the points of a depth cloud,
    σ(z) = σ0 + k (z − z0)² the axial noise of a structured-light camera at
    range z: the model of Nguyen, Izadi and Lovell, "Modeling Kinect sensor
    noise for improved 3D reconstruction and tracking" (3DIMPVT 2012), with
    their Kinect parameters as defaults (metres) — the caller's to set for
    another sensor. points [n, 3] in the world frame; origin [3] the sensor's
    position, axis [3] its optical axis (any length > 0); z = (p − origin) · axis
    / |axis| is the range along the axis. 1 at z = z0, decreasing beyond it.
    Evaluated as (σ0 / (σ0 + k (z − z0)²))², in that order. The weights are not
    normalised: the solvers divide the cost by the point count as before, so
    rescale to mean 1 where the cost per unit of weight matters."""
    p = np.asarray(points, np.float64)
    o, a = np.asarray(origin, np.float64), np.asarray(axis, np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError(f"depth_noise_weights: points must be [n, 3], got {p.shape}")
    if o.shape != (3,) or a.shape != (3,):
        raise ValueError(f"depth_noise_weights: origin and axis must be [3], got {o.shape} and {a.shape}")
    norm = float(np.sqrt(a @ a))
    if not (np.isfinite(norm) and norm > 0.0):
        raise ValueError("depth_noise_weights: the axis must be finite and not zero")
    if not (sigma0 > 0.0 and k >= 0.0 and np.isfinite(sigma0) and np.isfinite(k) and np.isfinite(z0)):
        raise ValueError("depth_noise_weights: sigma0 > 0, k >= 0 and z0 must be finite")
    z = (p - o) @ (a / norm)
    dz = z - z0
    r = sigma0 / (sigma0 + k * (dz * dz))
    return r * r
