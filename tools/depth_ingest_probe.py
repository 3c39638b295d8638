#!/usr/bin/env python3
"""Per-frame ingest of a depth camera's frame (GPU box): the same valid points
made resident by fsdf_set_points from a page-locked host cloud (24 B per point
over the host link) and by fsdf_set_depth_* from the depth image in u16, f32
and f64 (2 / 4 / 8 B per pixel; csrc/depth.hip back-projects and compacts on
the device). Image sizes 480x640 and 1024x1024 (2^20 pixels), about 90 % of
the pixels valid. The arms alternate within every round; the table gives the
median, minimum and maximum over the rounds of the host clock around the
synchronous call (each ends in a stream synchronise).

    python tools/depth_ingest_probe.py [--rounds 15] [--json FILE]

The new kernels' own times come from a kernel trace in a run of its own
(tracing slows the host: no ingest table from that run):

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \\
        python3 tools/depth_ingest_probe.py --rounds 3 --size 1024x1024
    python tools/depth_ingest_probe.py --kernel-stats OUT/*/run_kernel_stats.csv
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "point-cloud-signed-distance_amd"))

ARMS = ("set_points", "depth_u16", "depth_f32", "depth_f64")


def kernel_stats(paths):
    rows = []
    for p in paths:
        with open(p) as f:
            for r in csv.DictReader(f):
                name = r.get("Name", "")
                if "depth_" in name and "_kernel" in name:
                    rows.append(dict(kernel=name.split("(")[0], calls=int(r["Calls"]),
                                     mean_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3,
                                     max_us=float(r["MaxNs"]) / 1e3))
    for r in rows:
        print(f"{r['kernel'][:90]:90s} calls {r['calls']:5d}  mean {r['mean_us']:8.2f} us  "
              f"[{r['min_us']:.2f} .. {r['max_us']:.2f}]")
    return rows


def frame(rows, cols, seed):
    """A u16 millimetre image with ~90 % of the pixels in range, and the f32 / f64
    images of the same depths in metres."""
    r = np.random.Generator(np.random.PCG64(seed))
    mm = r.integers(600, 3500, size=(rows, cols)).astype(np.uint16)
    mm[r.uniform(size=mm.shape) < 0.1] = 0
    m64 = 0.001 * mm.astype(np.float64)
    return mm, m64.astype(np.float32), m64


def probe(shape, rounds, device):
    import torch
    from flash import Models, _lib
    from flash.depthsensors import Kinect, depth_points
    from flash.geometry import Transform, angle_axis
    m = Models.irb140()
    ctx = _lib.Context(device=device, sort_points=True)
    ctx.set_model([(s.hull.vertices, s.hull.faces, s.hull.planes) for s in m.surfaces])
    rays = Kinect(*shape).rays
    tf = Transform(angle_axis(np.pi / 2, [1, 0, 0]), np.array([0.0, 1.5, 0.5]))
    u16, f32, f64 = frame(shape[0], shape[1], 3)
    pts, _ = depth_points(u16, rays, tf, 0.5, 4.0, 0.001)
    pinned = torch.from_numpy(pts).pin_memory()
    cloud = pinned.numpy()
    ctx.set_sensor(rays, "range")
    calls = {
        "set_points": lambda: ctx.set_points(cloud),
        "depth_u16": lambda: ctx.set_depth(u16, tf, 0.5, 4.0, 0.001),
        "depth_f32": lambda: ctx.set_depth(f32, tf, 0.5, 4.0, 1.0),
        "depth_f64": lambda: ctx.set_depth(f64, tf, 0.5, 4.0, 1.0),
    }
    for _ in range(3):  # warm every arm: code objects, buffer growth
        for arm in ARMS:
            calls[arm]()
    ms = {arm: [] for arm in ARMS}
    for _ in range(rounds):
        for arm in ARMS:
            ctx.synchronize()
            t0 = time.perf_counter()
            calls[arm]()
            ms[arm].append((time.perf_counter() - t0) * 1e3)
    n = ctx.n
    ctx.close()
    out = dict(shape=list(shape), pixels=shape[0] * shape[1], points=len(pts), rounds=rounds, arms={})
    px = shape[0] * shape[1]
    link = {"set_points": 24 * len(pts), "depth_u16": 2 * px, "depth_f32": 4 * px, "depth_f64": 8 * px}
    for arm in ARMS:
        v = np.sort(ms[arm])
        out["arms"][arm] = dict(median_ms=float(np.median(v)), min_ms=float(v[0]), max_ms=float(v[-1]),
                                host_link_bytes=link[arm])
        print(f"{shape[0]}x{shape[1]} ({len(pts)} points) {arm:11s} median {np.median(v):7.3f} ms  "
              f"[{v[0]:.3f} .. {v[-1]:.3f}]  host link {link[arm] / 1e6:6.2f} MB", flush=True)
    assert n == len(pts), (n, len(pts))  # (every arm makes the same points resident)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--size", action="append", help="ROWSxCOLS (repeatable; default 480x640 and 1024x1024)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json")
    ap.add_argument("--kernel-stats", nargs="+", metavar="CSV", help="print the depth kernels of rocprofv3 stats files")
    a = ap.parse_args()
    if a.kernel_stats:
        rows = kernel_stats(a.kernel_stats)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(rows, f, indent=1)
        return 0
    shapes = [tuple(int(v) for v in s.split("x")) for s in (a.size or ["480x640", "1024x1024"])]
    res = [probe(s, a.rounds, a.device) for s in shapes]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
