#!/usr/bin/env python3
"""The launches a robust objective adds on a scene with RBF skins, for a kernel
trace (GPU box): per configuration --reps evaluations of eval_robust_skins
(the pass, robust_kernel, the skins' block launch csrc/robust_skin.hip and the
factor variant of the skin moments) and --reps of eval_skin_moments (the pass
and the unweighted skin_moments_kernel), on tools/bench_configs.py's C3
(beanbag, 2^20 points, fp32 and fp64) and C5 (irb_and_squishable, 2^20) clouds
under Huber(0.02) with weights in (0.5, 1.5).

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \\
        python3 tools/robust_skins_launches.py [--only c3:32 | c3:64 | c5:64] [--reps R] [--points N]

(one configuration per trace keeps its kernels apart: the stats go by kernel name) and, from the trace's *_kernel_stats.csv files, the per-kernel table:

    python3 tools/robust_skins_launches.py --summarise OUT --json kernels.json
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "point-cloud-signed-distance_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("robust_skin_kernel", "skin_moments_factor_kernel", "skin_moments_kernel", "skin_moments_finish_kernel",
           "robust_kernel", "pass_kernel")


def run(a):
    import torch  # noqa: F401  (the HIP runtime torch loads, before libflashsdf)
    import flash
    from flash import Models, synthetic
    from flash.core import prepare_pass
    from flash.robust import Huber
    bb = Models.beanbag()
    r = np.random.Generator(np.random.PCG64(5))
    x = np.zeros(flash.num_states(bb))
    x[:7] = bb.mechanism.zero_configuration()
    x[4:7] = 2 * r.random(3) ** 3
    x[7:] = 0.5 * (r.random(18) - 0.5)
    sc, x0 = Models.irb_and_squishable()
    real = np.load(os.path.join(ROOT, "tests", "golden", "squishable_unsquished.npz"))["xyz"]
    configs = [("C3 beanbag", bb, x, lambda: synthetic.skin_cloud(bb, x, a.points, 6), (32, 64)),
               ("C5 irb_and_squishable", sc, np.asarray(x0, np.float64),
                lambda: synthetic.c5_cloud(sc, x0, a.points, real, seed=7), (64,))]
    for name, m, xx, cloud, precisions in configs:
        precisions = [p for p in precisions if a.only in (None, f"{name[:2].lower()}:{p}")]
        if not precisions:
            continue
        pts = cloud()
        w = np.random.default_rng(4).uniform(0.5, 1.5, len(pts))
        for prec in precisions:
            ctx = m.engine(device=0, precision=prec)
            ctx.set_points(pts)
            nq = m.mechanism.num_positions
            poses, _ = prepare_pass(ctx, m, m.mechanism.normalize(xx[:nq]), xx[nq:])
            ctx.set_robust_skins(True)
            ctx.set_loss(Huber(0.02))
            ctx.set_point_weights(w)
            for _ in range(a.reps):
                cost, acc, _, Ms, _ = ctx.eval_robust_skins(poses)
            for _ in range(a.reps):
                ctx.eval_skin_moments(poses)
            print(json.dumps(dict(config=name, precision=prec, points=len(pts), reps=a.reps, cost=cost,
                                  block_max=float(np.abs(acc[1 + 6 * len(m.surfaces):]).max()),
                                  moments_max=[float(np.abs(M).max()) for M in Ms])), flush=True)
            ctx.set_loss(None)
            ctx.set_robust_skins(False)


def summarise(a):
    rows = {}
    for path in glob.glob(os.path.join(a.summarise, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for rec in csv.DictReader(f):
                name = rec["Name"]
                if not any(k in name for k in KERNELS):
                    continue
                calls = int(rec["Calls"])
                total = float(rec["AverageNs"]) * calls
                e = rows.setdefault(name, dict(kernel=name, calls=0, total_ns=0.0, min_us=float("inf"), max_us=0.0))
                e["calls"] += calls
                e["total_ns"] += total
                e["min_us"] = min(e["min_us"], float(rec["MinNs"]) / 1e3)
                e["max_us"] = max(e["max_us"], float(rec["MaxNs"]) / 1e3)
    out = []
    for e in sorted(rows.values(), key=lambda e: e["kernel"]):
        out.append(dict(kernel=e["kernel"], calls=e["calls"], mean_us=e["total_ns"] / e["calls"] / 1e3,
                        min_us=e["min_us"], max_us=e["max_us"]))
        print(f"{out[-1]['mean_us']:10.2f} us [{e['min_us']:.2f} .. {e['max_us']:.2f}] x{e['calls']:4d}  {e['kernel'][:150]}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--only", default=None, help="one configuration: c3:32, c3:64 or c5:64")
    ap.add_argument("--summarise", default=None, help="a rocprofv3 output directory: print / write the kernel table")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    summarise(args) if args.summarise else run(args)
