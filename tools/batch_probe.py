#!/usr/bin/env python3
"""What refining K starts costs, in lockstep against one after the other (GPU box).

Per cell (scene, n points, K starts; fp64, a resident Hilbert-sorted synthetic
depth cloud, Huber(0.02), starts drawn with sigma = 0.1 rad around the cloud's
configuration):

  batched     one fsdf_descend_lm_batch over the K starts, iteration limit 10
              (this tree's library)
  sequential  K fsdf_descend_lm calls from the same starts, the host loop, on the
              library named by --seq-lib (the parent commit's build, through
              FLASHSDF_LIB; default: this tree's)

and with --solver naive the same for fsdf_descend_batch against K fsdf_descend
host loops (NaiveSolver's rule: rate 0.1, max_step 0.5, 30 evaluations,
tolerance 0).

Each arm of a pair runs in a fresh child process (the library is chosen when
flash._lib is imported); the pairs alternate batched, sequential, ... A child
warms every cell up, then takes the median host-clock time of --reps calls (both
arms are synchronous). The driver reports, per cell, the median over the pairs
and the spread (max − min) of each arm, the ratio sequential / batched, and
whether the batched median lies below the sequential one by more than either
spread. The arms' evaluation counts and final objectives are recorded: the
sequential arm regroups its cloud after its first pass, so the two agree to
summation order, not to the bit.

    python3 tools/batch_probe.py [--solver lm|naive] [--pairs 3] [--reps 5] [--seq-lib PATH] [--json OUT.jsonl]
                                 [--scenes irb140 m64] [--points 4096 16384 131072] [--starts 3 8 32]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "point-cloud-signed-distance_amd"))

LM = dict(limit=10, damping=1e-3, max_step=0.5, tol=0.0)
NAIVE = dict(limit=30, rate=0.1, max_step=0.5, tol=0.0)


def _scene(name, n, kmax):
    from flash import Models, synthetic
    m = Models.irb140() if name == "irb140" else Models.arm_grid()
    qt, _ = synthetic.perturbed_configuration(m, 7)
    pts = synthetic.depth_cloud(m, qt, n, seed=8)
    r = np.random.default_rng(9)
    X = np.asarray(qt)[None, :] + r.normal(0.0, 0.1, (kmax, len(qt)))
    return m, pts, np.ascontiguousarray(X)


def child(a):
    import torch  # noqa: F401  (the HIP runtime torch loads, before libflashsdf)
    from flash.gradientdescent import CostFunctor
    from flash.robust import Huber
    kmax = max(a.starts)
    for name in a.scenes:
        for n in a.points:
            m, pts, X = _scene(name, n, kmax)
            cost = CostFunctor(m, pts, loss=Huber(0.02))
            cost.value_and_gradient(X[0])  # (resident, mechanism registered, loss set)
            ctx = cost.ctx
            ctx.set_solver(0)  # the sequential arm: fsdf_descend's host loop
            ctx.set_lm_solver(0)
            for K in a.starts:
                if a.solver == "lm":
                    def batched():
                        return ctx.descend_lm_batch(X[:K], LM["limit"], LM["damping"], LM["max_step"], LM["tol"], n)[1:3]

                    def sequential():
                        out = [ctx.descend_lm(X[k], LM["limit"], LM["damping"], LM["max_step"], LM["tol"], n)[1:3]
                               for k in range(K)]
                        return np.array([o[0] for o in out]), np.array([o[1] for o in out])
                else:
                    def batched():
                        return ctx.descend_batch(X[:K], NAIVE["limit"], NAIVE["rate"], NAIVE["max_step"], NAIVE["tol"],
                                                 None, n)[1:3]

                    def sequential():
                        out = [ctx.descend(X[k], NAIVE["limit"], NAIVE["rate"], NAIVE["max_step"], NAIVE["tol"], None,
                                           n)[1:3] for k in range(K)]
                        return np.array([o[0] for o in out]), np.array([o[1] for o in out])
                call = batched if a.arm == "batched" else sequential
                for _ in range(a.warmup):
                    f, its = call()
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    f, its = call()
                    ts.append((time.perf_counter() - t0) * 1e3)
                rec = dict(arm=a.arm, solver=a.solver, scene=name, points=n, K=K, ms=statistics.median(ts),
                           ms_min=min(ts), ms_max=max(ts), evaluations=int(np.sum(its)), f_mean=float(np.mean(f)),
                           lib=os.environ.get("FLASHSDF_LIB", "in-tree"))
                if a.arm == "batched":
                    ctx.profile_pass(True)
                    call()
                    rec["device_ms"], rec["device_calls"] = ctx.batch_time()
                    ctx.profile_pass(False)
                print("REC " + json.dumps(rec), flush=True)


def driver(a):
    cells = {}
    for pair in range(a.pairs):
        for arm in ("batched", "sequential"):
            env = dict(os.environ)
            env.pop("FLASHSDF_LIB", None)
            if arm == "sequential" and a.seq_lib:
                env["FLASHSDF_LIB"] = os.path.abspath(a.seq_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm, "--solver", a.solver, "--reps", str(a.reps),
                   "--warmup", str(a.warmup), "--scenes", *a.scenes, "--points", *map(str, a.points), "--starts",
                   *map(str, a.starts)]
            out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=a.child_timeout)
            for line in out.stdout.splitlines():
                if line.startswith("REC "):
                    r = json.loads(line[4:])
                    cells.setdefault((r["scene"], r["points"], r["K"]), {}).setdefault(arm, []).append(r)
            print(f"pair {pair} {arm} done", flush=True)
    recs = []
    for (scene, n, K), arms in sorted(cells.items()):
        b = [r["ms"] for r in arms["batched"]]
        s = [r["ms"] for r in arms["sequential"]]
        mb, ms_ = statistics.median(b), statistics.median(s)
        sb, ss = max(b) - min(b), max(s) - min(s)
        rec = dict(solver=a.solver, scene=scene, points=n, K=K, batched_ms=mb, batched_spread_ms=sb, sequential_ms=ms_,
                   sequential_spread_ms=ss, ratio=ms_ / mb, batched_faster_beyond_spread=bool(ms_ - mb > max(sb, ss)),
                   device_ms=statistics.median(r["device_ms"] for r in arms["batched"]),
                   rounds=arms["batched"][0]["device_calls"],
                   evaluations=(arms["batched"][0]["evaluations"], arms["sequential"][0]["evaluations"]),
                   f_mean=(arms["batched"][0]["f_mean"], arms["sequential"][0]["f_mean"]),
                   seq_lib=arms["sequential"][0]["lib"], pairs=a.pairs, reps=a.reps)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "a") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arm", choices=("batched", "sequential"), default=None, help="(a child's: run one arm)")
    ap.add_argument("--solver", choices=("lm", "naive"), default="lm")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seq-lib", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child-timeout", type=float, default=240.0)
    ap.add_argument("--scenes", nargs="+", default=["irb140", "m64"])
    ap.add_argument("--points", nargs="+", type=int, default=[4096, 16384, 131072])
    ap.add_argument("--starts", nargs="+", type=int, default=[3, 8, 32])
    args = ap.parse_args()
    child(args) if args.arm else driver(args)
