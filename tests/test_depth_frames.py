"""Depth-frame ingest, host side: flash.depthsensors.depth_points — the numpy
twin of fsdf_set_depth_* (csrc/depth.hip) — against the reference's
raycast_points construction, its validity rule and formats; the ABI and the
Julia shim carry the new entry points."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, rng

DEPTH_SYMBOLS = ("fsdf_set_sensor", "fsdf_get_sensor", "fsdf_set_depth_f64", "fsdf_set_depth_f32",
                 "fsdf_set_depth_u16", "fsdf_set_depth_device", "fsdf_get_depth_pixels")


def _tform():
    from flash.geometry import Transform, angle_axis
    return Transform(angle_axis(0.7, [0.3, -0.5, 0.8]), np.array([0.4, -1.5, 0.9]))


def test_twin_matches_raycast_points_construction():
    """Kinect(7, 9) under a non-trivial Transform, a synthetic image with NaN
    misses: the pixels of ~isnan in row-major order, and the points of the body
    of raycast_points within 32 eps (max depth + max|t|): about 8 rounded
    operations per coordinate, row sums of |R| <= sqrt(3)."""
    from flash.depthsensors import Kinect, depth_points
    sensor, tf = Kinect(7, 9), _tform()
    r = rng(1)
    d = r.uniform(0.5, 3.0, size=(7, 9))
    d[r.uniform(size=d.shape) < 0.3] = np.nan
    d[0, 0], d[6, 8] = np.nan, 2.5
    pts, pix = depth_points(d, sensor.rays, tf)
    hit = ~np.isnan(d)
    assert pix.dtype == np.int32 and np.array_equal(pix, np.flatnonzero(hit.ravel()))
    nr = sensor.rays / np.linalg.norm(sensor.rays, axis=-1, keepdims=True)
    ref = tf.apply(d[hit][:, None] * nr[hit])
    bound = 32 * np.finfo(np.float64).eps * (np.nanmax(d) + np.abs(tf.t).max())
    assert pts.shape == ref.shape and np.abs(pts - ref).max() <= bound


def test_validity_rule():
    from flash.depthsensors import Kinect, depth_points
    sensor = Kinect(3, 5)
    near, far = 0.5, 2.0
    vals = [0.0, -1.0, np.nan, np.inf, -np.inf, near, far, np.nextafter(near, 0.0), np.nextafter(far, 3.0),
            1.0, -0.0, np.nextafter(near, 1.0), np.nextafter(far, 0.0), 5e-324, 1e300]
    keep = [False, False, False, False, False, True, True, False, False, True, False, True, True, False, False]
    d = np.array(vals).reshape(3, 5)
    _, pix = depth_points(d, sensor.rays, None, near=near, far=far)
    assert np.array_equal(pix, np.flatnonzero(keep))
    # the defaults {0, +inf, 1}: finite and > 0
    _, pix = depth_points(d, sensor.rays, None)
    assert np.array_equal(pix, np.flatnonzero([np.isfinite(v) and v > 0 for v in vals]))
    # the scale applies before the test
    _, pix = depth_points(d, sensor.rays, None, near=near, far=far, scale=2.0)
    assert np.array_equal(pix, np.flatnonzero([np.isfinite(v) and near <= 2.0 * v <= far for v in vals]))
    for bad in (dict(near=np.nan), dict(near=2.0, far=1.0), dict(scale=0.0), dict(scale=np.inf), dict(scale=-1.0)):
        with pytest.raises(ValueError):
            depth_points(d, sensor.rays, None, **bad)
    with pytest.raises(TypeError):
        depth_points(np.ones((3, 5), np.int32), sensor.rays, None)


def test_formats_give_the_f64_bits():
    """u16 with scale 0.001 = the f64 image 0.001 * float64(depth) with scale 1
    (exact widening, one multiply); f32 against the widened f64 image."""
    from flash.depthsensors import Kinect, depth_points
    sensor, tf = Kinect(6, 11), _tform()
    r = rng(2)
    u16 = r.integers(0, 6000, size=(6, 11)).astype(np.uint16)
    u16[1, 2], u16[5, 10] = 0, 65535
    a, pa = depth_points(u16, sensor.rays, tf, near=0.4, far=5.0, scale=0.001)
    b, pb = depth_points(0.001 * u16.astype(np.float64), sensor.rays, tf, near=0.4, far=5.0)
    assert len(pa) > 20 and np.array_equal(pa, pb) and np.array_equal(a, b)
    f32 = r.uniform(0.2, 4.0, size=(6, 11)).astype(np.float32)
    f32[0, 3], f32[2, 2] = np.nan, np.inf
    a, pa = depth_points(f32, sensor.rays, tf, near=0.4, far=3.5, scale=1.25)
    b, pb = depth_points(f32.astype(np.float64), sensor.rays, tf, near=0.4, far=3.5, scale=1.25)
    assert len(pa) > 20 and np.array_equal(pa, pb) and np.array_equal(a, b)


def test_kind_z_third_coordinate_is_the_depth():
    from flash.depthsensors import DepthFrame, Kinect
    sensor = Kinect(5, 8)
    r = rng(3)
    d = r.uniform(0.3, 4.0, size=(5, 8))
    d[2, 3] = np.nan
    frame = DepthFrame(d, sensor, None, scale=0.5, kind="z")
    pts, pix = frame.points()
    s = 0.5 * d.ravel()[pix]
    assert len(pix) == 39 and np.array_equal(pts[:, 2], s)
    # and x / z, y / z are the rays' slopes
    rays = sensor.rays.reshape(-1, 3)[pix]
    assert np.array_equal(pts[:, 0], s * (rays[:, 0] / rays[:, 2]))
    # the range model of the same image puts the points at distance s
    pr, _ = DepthFrame(d, sensor, None, scale=0.5).points()
    assert np.allclose(np.linalg.norm(pr, axis=1), s, rtol=1e-15)
    with pytest.raises(ValueError):
        DepthFrame(d, DepthFrameSensorBehind(sensor), None, kind="z").points()


class DepthFrameSensorBehind:
    """A sensor with one ray looking backwards (z <= 0): refused by kind 'z'."""

    def __init__(self, sensor):
        self.rays = sensor.rays.copy()
        self.rays[0, 0, 2] = -1.0


def test_abi_lists_the_depth_entry_points():
    from flash import _lib
    for name in DEPTH_SYMBOLS:
        assert name in _lib.SYMBOLS, name
    header = open(os.path.join(ROOT, "include", "flashsdf.h")).read()
    for name in DEPTH_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert "FSDF_DEPTH_RANGE = 0, FSDF_DEPTH_Z = 1" in header
    assert "FSDF_DEPTH_F64 = 0, FSDF_DEPTH_F32 = 1, FSDF_DEPTH_U16 = 2" in header


def test_shim_binds_the_f64_path():
    text = open(os.path.join(ROOT, "julia", "FlashSDF.jl")).read()
    bound = set(re.findall(r"ccall\(\(:(fsdf_\w+),\s*lib\)", text))
    for name in ("fsdf_set_sensor", "fsdf_set_depth_f64", "fsdf_get_depth_pixels"):
        assert name in bound, name
    # the other entry points take types the shim's table does not carry
    assert not bound & {"fsdf_set_depth_f32", "fsdf_set_depth_u16", "fsdf_set_depth_device", "fsdf_get_sensor"}
    for fn in ("function set_sensor!", "function set_depth!", "function depth_pixels"):
        assert fn in text, fn
