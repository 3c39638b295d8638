#!/usr/bin/env python3
"""What the skins' second moments cost beside the pass (GPU box): per scene and
cloud size, the device time of the skin-moments launches (csrc/skin_moments.hip:
the kernel and its finish launch per skin, a pair of HIP events around them,
fsdf_skin_moments_time) beside the same evaluation's pass (pass kernel +
reduce, fsdf_pass_times), on a resident synthetic.skin_cloud at the scene's
zero configuration, after warm-up, median and spread over --reps evaluations.

    python3 tools/skin_moments_time.py [squishable:65536 squishable:1048576 two_link_arm:65536 ...] [--reps R]
                                       [--json OUT.jsonl]

FLASHSDF_LIB=path/to/libflashsdf_fma.so runs the same on an A/B build (a
library built with -DFSDF_SKIN_MOMENTS_FMA=1 forms JᵀJ with v_fma_f64 inner
products instead of the fp64 MFMA); the moments of the first evaluation are
hashed into the record, so two builds can be compared on what they computed."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "point-cloud-signed-distance_amd"))

DEFAULT = ("squishable:65536", "squishable:1048576", "two_link_arm:65536", "two_link_arm:1048576")


def run(a):
    import torch  # noqa: F401  (the HIP runtime torch loads, before libflashsdf)
    import flash
    from flash import Models, rbf, synthetic
    from flash.core import surface_poses
    out = []
    for cfg in a.configs:
        name, n = cfg.split(":")
        n = int(n)
        m = getattr(Models, name)()
        nq = m.mechanism.num_positions
        x = np.zeros(flash.num_states(m))
        x[:nq] = m.mechanism.zero_configuration()
        pts = synthetic.skin_cloud(m, x, n, seed=11)
        qn = m.mechanism.normalize(x[:nq])
        solves = rbf.solve(m, qn, x[nq:])
        poses = surface_poses(m, qn)
        ctx = m.engine()
        ctx.set_points(pts)
        ctx.set_rbf_params(rbf.rows(solves))
        first = None
        for _ in range(a.warmup):  # allocations, code objects, the block order
            _, _, Ms = ctx.eval_skin_moments(poses)
            first = first if first is not None else [M.copy() for M in Ms]
        ctx.profile_pass(True)
        skin, kern, whole = [], [], []
        for _ in range(a.reps):
            _, _, Ms = ctx.eval_skin_moments(poses)
            ms, launches = ctx.skin_moments_time()
            k, p, passes = ctx.pass_times()
            assert launches == 1 and passes == 1, (launches, passes)
            skin.append(ms * 1e3)
            kern.append(k * 1e3)
            whole.append(p * 1e3)
        ctx.profile_pass(False)
        same = all(np.array_equal(A, B) for A, B in zip(first, Ms))
        rec = dict(scene=name, points=n, m=[4 * r.n + 4 for r in solves], reps=a.reps,
                   lib=os.environ.get("FLASHSDF_LIB", "in-tree"),
                   skin_moments_us=dict(median=statistics.median(skin), min=min(skin), max=max(skin)),
                   pass_kernel_us=dict(median=statistics.median(kern), min=min(kern), max=max(kern)),
                   pass_us=dict(median=statistics.median(whole), min=min(whole), max=max(whole)),
                   bit_identical_runs=bool(same),
                   moments_sum=[float(M.sum()) for M in first], moments_max=[float(np.abs(M).max()) for M in first])
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if a.json:
        with open(a.json, "a") as f:
            for rec in out:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("configs", nargs="*", default=list(DEFAULT))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    run(ap.parse_args())
