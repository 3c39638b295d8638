#!/usr/bin/env python3
"""What a voxel grid buys per frame (GPU box): a 480x640 u16 depth frame — the
IRB140 raycast on the device from 1 m, a wall at 2 m behind it, millimetres —
made resident by fsdf_set_depth_u16 with the grid off and at h = 5 mm and 10 mm
(csrc/voxel.hip between the scatter and the resident cloud), and a
30-evaluation Levenberg-Marquardt frame (fsdf_descend_lm, host loop, Huber
0.02) on each resident cloud. The arms alternate within every round; the table
gives the median, minimum and maximum over the rounds of the host clock around
each synchronous call.

    python tools/voxel_probe.py [--rounds 15] [--json FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "point-cloud-signed-distance_amd"))

ARMS = (("off", None), ("h=5mm", 0.005), ("h=10mm", 0.010))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--size", default="480x640")
    ap.add_argument("--json")
    a = ap.parse_args()
    import flash
    from flash import Models, VoxelGrid
    from flash.depthsensors import DepthFrame, Kinect, raycast_depths
    from flash.geometry import Transform, angle_axis
    from flash.gradientdescent import CostFunctor
    from flash.robust import Huber
    shape = tuple(int(v) for v in a.size.split("x"))
    m = Models.irb140()
    sensor = Kinect(*shape)
    tf = Transform(angle_axis(np.pi / 2, [1, 0, 0]), np.array([0.0, 1.0, 0.45]))
    state = flash.ManipulatorState(m)
    state.q[:] = [0.3, -0.2, 0.25, 0.1, -0.15, 0.2]
    d = raycast_depths(flash.skin(state), sensor, tf)
    # a wall 2 m in front of the camera behind the arm: range = 2 / (the ray's z component)
    u = sensor.rays / np.linalg.norm(sensor.rays, axis=-1, keepdims=True)
    d = np.where(np.isnan(d), 2.0 / u[..., 2], d)
    mm = np.round(1000.0 * d).astype(np.uint16)
    x0 = state.q + np.array([0.08, -0.06, 0.07, 0.05, -0.04, 0.06])
    frames = {name: (DepthFrame(mm, sensor, tf, 0.3, 4.0, 0.001), None if h is None else VoxelGrid(h))
              for name, h in ARMS}
    cost = CostFunctor(m, np.zeros((0, 3)), loss=Huber(0.02))
    ingest = {name: [] for name, _ in ARMS}
    solve = {name: [] for name, _ in ARMS}
    resident, divisor = {}, {}
    for r in range(a.rounds + 2):  # (two warm rounds: code objects, buffer growth)
        for name, _ in ARMS:
            frame, grid = frames[name]
            cost.set_sensed_points(frame, voxel=grid)  # (the functor's own ingest: sensor, settings, sizes)
            cost.ctx.set_voxel_grid(grid)
            cost.ctx.synchronize()
            t0 = time.perf_counter()
            cost.ctx.set_depth(mm, tf, 0.3, 4.0, 0.001)  # (the bare synchronous call: the same cloud again)
            t1 = time.perf_counter()
            cost.descend_lm(x0, 30, 1e-3, 0.5, 0.0, cost.n_divisor)
            t2 = time.perf_counter()
            cost.ctx.set_voxel_grid(None)
            if r >= 2:
                ingest[name].append((t1 - t0) * 1e3)
                solve[name].append((t2 - t1) * 1e3)
            resident[name], divisor[name] = cost.n_points, cost.n_divisor
    out = dict(shape=list(shape), rounds=a.rounds, arms={})
    for name, _ in ARMS:
        i, s = np.sort(ingest[name]), np.sort(solve[name])
        tot = np.sort(np.array(ingest[name]) + np.array(solve[name]))
        out["arms"][name] = dict(resident_points=int(resident[name]), divisor=int(divisor[name]),
                                 ingest_ms=[float(np.median(i)), float(i[0]), float(i[-1])],
                                 lm30_ms=[float(np.median(s)), float(s[0]), float(s[-1])],
                                 total_ms=[float(np.median(tot)), float(tot[0]), float(tot[-1])])
        print(f"{shape[0]}x{shape[1]} {name:7s} resident {resident[name]:7d} (N {divisor[name]:7d})  set_depth "
              f"{np.median(i):7.3f} ms [{i[0]:.3f} .. {i[-1]:.3f}]  LM x30 {np.median(s):8.3f} ms [{s[0]:.3f} .. "
              f"{s[-1]:.3f}]  total {np.median(tot):8.3f} ms [{tot[0]:.3f} .. {tot[-1]:.3f}]", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
