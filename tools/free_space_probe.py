#!/usr/bin/env python3
"""What free-space samples cost (GPU box; include/flashsdf.h "free space").

Ingest per frame: fsdf_set_depth_u16 with free space off against on, at J = 4
samples per sending pixel with stride 4 and with stride 1, for 480x640 and
1024x1024 images (tools/depth_ingest_probe.py's frames: about 90 % of the
pixels valid). The arms alternate within every round; the table gives the
median, minimum and maximum over the rounds of the host clock around the
synchronous call. With FLASHSDF_LIB naming a library from before the feature
only the off arm runs (--off-only): its figures against this library's off arm.

    python tools/free_space_probe.py [--rounds 15] [--json FILE] [--off-only]

The robust launch with and without a split at 2^20 points, from a kernel trace
in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \\
        python3 tools/free_space_probe.py --robust 1048576
    python tools/free_space_probe.py --kernel-stats OUT/*/run_kernel_stats.csv
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from depth_ingest_probe import frame  # noqa: E402

ARMS = ("off", "J4_stride4", "J4_stride1")


def kernel_stats(paths):
    rows = []
    for p in paths:
        with open(p) as f:
            for r in csv.DictReader(f):
                name = r.get("Name", "")
                if "robust_kernel" in name or ("depth_" in name and "_kernel" in name):
                    rows.append(dict(kernel=name, calls=int(r["Calls"]), mean_us=float(r["AverageNs"]) / 1e3,
                                     min_us=float(r["MinNs"]) / 1e3, max_us=float(r["MaxNs"]) / 1e3))
    for r in rows:
        print(f"{r['kernel'][:110]:110s} calls {r['calls']:5d}  mean {r['mean_us']:8.2f} us  "
              f"[{r['min_us']:.2f} .. {r['max_us']:.2f}]")
    return rows


def _context(device):
    from flash import Models, _lib
    m = Models.irb140()
    ctx = _lib.Context(device=device, sort_points=True)
    ctx.set_model([(s.hull.vertices, s.hull.faces, s.hull.planes) for s in m.surfaces])
    return m, ctx


def ingest(shape, rounds, device, off_only):
    from flash.depthsensors import FreeSpace, Kinect
    from flash.geometry import Transform, angle_axis
    _, ctx = _context(device)
    rays = Kinect(*shape).rays
    tf = Transform(angle_axis(np.pi / 2, [1, 0, 0]), np.array([0.0, 1.5, 0.5]))
    u16, _, _ = frame(shape[0], shape[1], 3)
    ctx.set_sensor(rays, "range")
    setting = {"off": None, "J4_stride4": FreeSpace(4, 4, 0.02, 0.1, 0.0), "J4_stride1": FreeSpace(4, 1, 0.02, 0.1, 0.0)}
    arms = ("off",) if off_only else ARMS
    points = {}

    def call(arm):
        if not off_only:
            ctx.set_free_space(setting[arm])
        points[arm] = ctx.set_depth(u16, tf, 0.5, 4.0, 0.001)

    for _ in range(3):  # warm every arm: code objects, buffer growth
        for arm in arms:
            call(arm)
    ms = {arm: [] for arm in arms}
    for _ in range(rounds):
        for arm in arms:
            ctx.synchronize()
            t0 = time.perf_counter()
            call(arm)
            ms[arm].append((time.perf_counter() - t0) * 1e3)
    ctx.close()
    out = dict(shape=list(shape), pixels=shape[0] * shape[1], rounds=rounds, library=os.environ.get("FLASHSDF_LIB", ""),
               arms={})
    for arm in arms:
        v = np.sort(ms[arm])
        out["arms"][arm] = dict(points=points[arm], median_ms=float(np.median(v)), min_ms=float(v[0]), max_ms=float(v[-1]))
        print(f"{shape[0]}x{shape[1]} {arm:11s} {points[arm]:8d} points  median {np.median(v):7.3f} ms  "
              f"[{v[0]:.3f} .. {v[-1]:.3f}]", flush=True)
    return out


def robust(n, device, repeats=20):
    """eval_robust over n points of both signs of d*, without and with a split at n / 2 (Huber, moments)."""
    import flash
    from flash import synthetic
    from flash.robust import Huber
    m, ctx = _context(device)
    q_true, q_eval = synthetic.perturbed_configuration(m, 21)
    poses = flash.hull_poses(m, q_eval)
    pts = synthetic.depth_cloud(m, q_true, n, seed=22)
    ctx.set_points(pts)
    _, _, (_, d, g) = ctx.eval(poses, per_point=True)
    ctx.set_points(pts - (d - np.where(np.arange(n) % 2 == 0, -0.01, 0.01))[:, None] * g)
    ctx.set_loss(Huber(0.02))
    costs = {}
    for split in (None, n // 2):
        ctx.set_free_split(split)
        for _ in range(repeats):
            costs[split] = ctx.eval_robust(poses)[0]
    ctx.close()
    print(f"robust launches at {n} points: {repeats} without a split (cost {costs[None]:.6f}), {repeats} with "
          f"n_surface = {n // 2} (cost {costs[n // 2]:.6f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--size", action="append", help="ROWSxCOLS (repeatable; default 480x640 and 1024x1024)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json")
    ap.add_argument("--off-only", action="store_true", help="the off arm alone (a library from before the feature)")
    ap.add_argument("--robust", type=int, metavar="N", help="run the robust launches at N points (under a kernel trace)")
    ap.add_argument("--kernel-stats", nargs="+", metavar="CSV", help="print the kernels of rocprofv3 stats files")
    a = ap.parse_args()
    if a.kernel_stats:
        rows = kernel_stats(a.kernel_stats)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(rows, f, indent=1)
        return 0
    if a.robust:
        robust(a.robust, a.device)
        return 0
    shapes = [tuple(int(v) for v in s.split("x")) for s in (a.size or ["480x640", "1024x1024"])]
    res = [ingest(s, a.rounds, a.device, a.off_only) for s in shapes]
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
