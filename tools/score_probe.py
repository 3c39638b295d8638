#!/usr/bin/env python3
"""What scoring B candidate states costs, batched against one by one (GPU box).

Per cell (scene, n points, B candidates; fp64, a resident Hilbert-sorted
synthetic depth cloud, candidates drawn around the cloud's configuration):

  batched  one fsdf_score_poses call over the B candidates (this tree's library)
  loop     B sequential fsdf_eval_robust calls, cost only (NULL outputs), on the
           library named by --loop-lib (the parent commit's build, through
           FLASHSDF_LIB; default: this tree's)

Each arm of a pair runs in a fresh child process (the library is chosen when
flash._lib is imported); the pairs alternate batched, loop, batched, loop, ...
A child warms every cell up, then takes the median host-clock time of --reps
synchronous calls (both arms end in a stream synchronise inside the library).
The driver reports, per cell, the median over the pairs and the spread
(max − min) of each arm, the ratio loop / batched, and whether the batched
median lies below the loop's by more than either spread.

    python3 tools/score_probe.py [--pairs 3] [--reps 5] [--loop-lib PATH] [--json OUT.jsonl]
                                 [--scenes irb140 m64] [--points 4096 16384 131072] [--batches 8 64 512]

The batched child also records the device time of one profiled call
(fsdf_score_time) and checks its costs against the loop's first candidate
(relative difference printed; both are sums of the same terms)."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "point-cloud-signed-distance_amd"))


def _scene(name, n, bmax):
    import flash
    from flash import Models, synthetic
    m = Models.irb140() if name == "irb140" else Models.arm_grid()
    qt, _ = synthetic.perturbed_configuration(m, 7)
    pts = synthetic.depth_cloud(m, qt, n, seed=8)
    r = np.random.default_rng(9)
    X = np.asarray(qt)[None, :] + r.normal(0.0, 0.1, (bmax, len(qt)))
    poses = np.ascontiguousarray(np.stack([flash.hull_poses(m, x) for x in X]))
    return m, pts, poses


def child(a):
    import torch  # noqa: F401  (the HIP runtime torch loads, before libflashsdf)
    from flash import _lib
    lib = _lib.load()
    bmax = max(a.batches)
    for name in a.scenes:
        ctx, poses_of = None, {}
        for n in a.points:
            m, pts, poses = _scene(name, n, bmax)
            if ctx is None:
                ctx = _lib.Context(device=0, precision=64, sort_points=True)
                ctx.set_model([(s.hull.vertices, s.hull.faces, s.hull.planes) for s in m.surfaces])
            ctx.set_points(pts)
            for B in a.batches:
                P = poses[:B]
                cost = ctypes.c_double(0.0)

                def loop():
                    for b in range(B):
                        st = lib.fsdf_eval_robust(ctx._ctx, _lib.ptr(P[b]), ctypes.byref(cost), None, None, None)
                        assert st == 0, st
                    return cost.value

                call = (lambda: ctx.score_poses(P)) if a.arm == "batched" else loop
                for _ in range(a.warmup):
                    last = call()
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    last = call()
                    ts.append((time.perf_counter() - t0) * 1e3)
                rec = dict(arm=a.arm, scene=name, points=n, B=B, ms=statistics.median(ts), ms_min=min(ts),
                           ms_max=max(ts), lib=os.environ.get("FLASHSDF_LIB", "in-tree"))
                if a.arm == "batched":
                    ctx.profile_pass(True)
                    ctx.score_poses(P)
                    rec["device_ms"] = ctx.score_time()[0]
                    ctx.profile_pass(False)
                    rec["cost_last"] = float(last[-1])
                else:
                    rec["cost_last"] = float(last)
                print("REC " + json.dumps(rec), flush=True)
        if ctx is not None:
            ctx.close()


def driver(a):
    cells = {}
    for pair in range(a.pairs):
        for arm in ("batched", "loop"):
            env = dict(os.environ)
            env.pop("FLASHSDF_LIB", None)
            if arm == "loop" and a.loop_lib:
                env["FLASHSDF_LIB"] = os.path.abspath(a.loop_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--reps", str(a.reps), "--warmup",
                   str(a.warmup), "--scenes", *a.scenes, "--points", *map(str, a.points), "--batches",
                   *map(str, a.batches)]
            out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=a.child_timeout)
            for line in out.stdout.splitlines():
                if line.startswith("REC "):
                    r = json.loads(line[4:])
                    cells.setdefault((r["scene"], r["points"], r["B"]), {}).setdefault(arm, []).append(r)
            print(f"pair {pair} {arm} done", flush=True)
    recs = []
    for (scene, n, B), arms in sorted(cells.items()):
        b = [r["ms"] for r in arms["batched"]]
        s = [r["ms"] for r in arms["loop"]]
        mb, ms_ = statistics.median(b), statistics.median(s)
        sb, ss = max(b) - min(b), max(s) - min(s)
        cb, cl = arms["batched"][0]["cost_last"], arms["loop"][0]["cost_last"]
        rec = dict(scene=scene, points=n, B=B, batched_ms=mb, batched_spread_ms=sb, loop_ms=ms_, loop_spread_ms=ss,
                   ratio=ms_ / mb, batched_faster_beyond_spread=bool(ms_ - mb > max(sb, ss)),
                   device_ms=statistics.median(r["device_ms"] for r in arms["batched"]),
                   cost_rel_diff=abs(cb - cl) / max(abs(cl), 1e-300), loop_lib=arms["loop"][0]["lib"], pairs=a.pairs,
                   reps=a.reps)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "a") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arm", choices=("batched", "loop"), default=None, help="(a child's: run one arm)")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-lib", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--scenes", nargs="+", default=["irb140", "m64"])
    ap.add_argument("--points", nargs="+", type=int, default=[4096, 16384, 131072])
    ap.add_argument("--batches", nargs="+", type=int, default=[8, 64, 512])
    args = ap.parse_args()
    child(args) if args.arm else driver(args)
