#!/usr/bin/env python3
"""What the Gauss-Newton Hessian costs beside a gradient (GPU box): per call,
fsdf_value_gradient_hessian (pass + per-point k*, ∇d* + the moments launch and
its reduce + read-back + the host matrix) against fsdf_value_and_gradient on
the same resident cloud, alternating, in its steady layout (after the cloud's
first pass and auto regroup).

    python3 tools/lm_probe.py m64:1048576 m64:131072 irb140:1048576 [--reps R] [--json OUT.jsonl]

    python3 tools/lm_probe.py m64:1048576 --frames 5

times whole estimate_state frames instead (set_points + the solver from the
same perturbed start, as tools/descend_probe.py's): the default NaiveSolver
(30 iterations, rate 0.1, max_step 0.5, tolerance 1e-3) against
LevenbergMarquardt at several evaluation limits (--limits), with the f = c / n
each ends at and the evaluations it made. --device-loop runs the LM frames on
the device-resident loop (fsdf_set_lm_solver 2) instead of the host loop;
--prior W gives them the prior of fsdf_set_lm_prior at a uniform weight W, or
scaled per coordinate by the points of the joint's subtree (--prior-scale
subtree: W · N / points nearest a surface of the subtree; f is then the wrapped
objective's, the prior included). --loss huber:0.02 | tukey:0.05 gives every
frame (and, without --frames, every timed call) that robust point loss
(fsdf_set_loss: f is then Σρ/N, the LM frames run the host loop — with
--robust-loops the functor turns fsdf_set_robust_loops on, and --device-loop
then runs them, and the NaiveSolver frames, on the device-resident loops); the table
also carries the error over the three base joints of each arm. --weights
depth | random gives the resident cloud per-point confidence weights
(fsdf_set_point_weights; set again after every cloud swap): depth the axial
noise model of flash.depth_noise_weights for a sensor 1.5 m from the cloud's
centre looking along +x, random uniform in [0, 2] with one in ten exactly 0 —
the calls then run the weighted robust reduction, also without --loss.

And for the kernels' own times a kernel trace of the Hessian calls alone
(no counters in the same run):

    rocprofv3 --kernel-trace --output-format csv -d OUT -o run -- python3 tools/lm_probe.py m64:1048576 --hessian-only
    python3 tools/lm_probe.py --trace OUT/.../run_kernel_trace.csv

which prints per kernel the count, mean and median duration, and for
moments_kernel the span to the end of the tile reduce that follows it."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "point-cloud-signed-distance_amd"))


def point_weights(kind, pts):
    """The --weights array for a cloud (None: no weights)."""
    if kind is None:
        return None
    if kind == "depth":
        from flash import depth_noise_weights
        return depth_noise_weights(pts, pts.mean(0) - [1.5, 0.0, 0.0], [1.0, 0.0, 0.0])
    r = np.random.default_rng(99)
    w = r.uniform(0.0, 2.0, len(pts))
    w[r.random(len(pts)) < 0.1] = 0.0
    return w


def run(a):
    import torch  # noqa: F401  (the HIP runtime torch loads, before libflashsdf)
    from flash import Models, synthetic
    from flash.gradientdescent import CostFunctor
    for cfg in a.configs:
        model, n = cfg.split(":")
        n = int(n)
        m = Models.arm_grid() if model == "m64" else Models.irb140()
        q_true, q = synthetic.perturbed_configuration(m, 1234)
        q = np.asarray(q, np.float64)
        cf = CostFunctor(m, synthetic.depth_cloud(m, q_true, n, seed=1234 + 17), loss=a.loss)
        if a.weights:
            cf.set_point_weights(point_weights(a.weights, cf.sensed_points))
        for _ in range(5):  # the cloud's first pass, the regroup, the block order / plan, allocations
            cf.value_and_gradient(q)
            cf.value_gradient_hessian(q)
        vg, vgh = [], []
        for _ in range(a.reps):
            if not a.hessian_only:
                t0 = time.perf_counter()
                cf.value_and_gradient(q)
                vg.append((time.perf_counter() - t0) * 1e6)
            t0 = time.perf_counter()
            cf.value_gradient_hessian(q)
            vgh.append((time.perf_counter() - t0) * 1e6)
        out = {"model": model, "points": n, "reps": a.reps, "pass_kernel": cf.ctx.pass_kernel_name(),
               "loss": repr(a.loss) if a.loss is not None else None, "weights": a.weights,
               "value_gradient_hessian_us": statistics.median(vgh),
               "value_gradient_hessian_us_p10_p90": [float(np.percentile(vgh, 10)), float(np.percentile(vgh, 90))]}
        if vg:
            out["value_and_gradient_us"] = statistics.median(vg)
            out["value_and_gradient_us_p10_p90"] = [float(np.percentile(vg, 10)), float(np.percentile(vg, 90))]
            out["hessian_extra_us"] = out["value_gradient_hessian_us"] - out["value_and_gradient_us"]
        print(json.dumps(out), flush=True)
        if a.json:
            with open(a.json, "a") as f:
                f.write(json.dumps(out) + "\n")


def frames(a):
    import torch  # noqa: F401
    from flash import Models, synthetic
    from flash.gradientdescent import CostFunctor
    for cfg in a.configs:
        model, n = cfg.split(":")
        n = int(n)
        m = Models.arm_grid() if model == "m64" else Models.irb140()
        q_true, q = synthetic.perturbed_configuration(m, 1234)
        q = np.asarray(q, np.float64)
        pts = synthetic.depth_cloud(m, q_true, n, seed=1234 + 17)
        cf = CostFunctor(m, pts, loss=a.loss, **({"robust_loops": True} if a.robust_loops else {}))
        w = point_weights(a.weights, pts)
        f_true = cf.value_and_gradient(np.asarray(q_true, np.float64))[0] / n
        # the three base joints of each arm (IRB140: six revolute joints per arm, in arm order)
        base = np.array([j for j in range(len(q)) if j % 6 < 3])
        solvers = [("naive", None)] + [("lm", k) for k in a.limits]
        if a.device_loop:  # (the default is the host loop: an A/B library from before the switch runs it too)
            cf.ctx.set_lm_solver("require")
        prior = None
        if a.prior is not None:
            prior = np.full(len(q), a.prior)
            if a.prior_scale == "subtree":
                prior = prior * subtree_scale(m, cf, q_true, n)
        kw = {} if prior is None else {"prior_weight": prior}
        for rep in range(2):  # (alternating: each solver's frames twice, apart)
            for name, limit in solvers:
                ms = []
                for _ in range(a.frames + 1):
                    t0 = time.perf_counter()
                    cf.set_sensed_points(pts)
                    if w is not None:
                        cf.set_point_weights(w)
                    if name == "naive":
                        x, f, its = cf.descend(q, 30, 0.1, 0.5, 1e-3, None, float(n))
                    else:
                        x, f, its, _ = cf.descend_lm(q, limit, 1e-3, 0.5, 1e-6, float(n), **kw)
                    ms.append((time.perf_counter() - t0) * 1e3)
                out = {"model": model, "points": n, "solver": name, "limit": limit or 30, "rep": rep,
                       "frame_ms": statistics.median(ms[1:]), "evaluations": its, "f": f, "f_at_q_true": f_true,
                       "lm_loop": "device" if a.device_loop else "host", "prior": a.prior,
                       "prior_scale": a.prior_scale if a.prior is not None else None,
                       "max_abs_q_error": float(np.abs(x - q_true).max()),
                       "max_abs_base_joint_error": float(np.abs(x - q_true)[base].max()),
                       "loss": repr(a.loss) if a.loss is not None else None, "weights": a.weights,
                       "robust_loops": bool(a.robust_loops)}
                print(json.dumps(out), flush=True)
                if a.json:
                    with open(a.json, "a") as fh:
                        fh.write(json.dumps(out) + "\n")


def subtree_scale(m, cf, q, n):
    """Per coordinate N / (points whose nearest surface lies in the subtree of
    the coordinate's joint, at q): a joint that few points see gets the larger
    weight."""
    mech = m.mechanism
    k = next(v for v in cf.per_point(np.asarray(q, np.float64)) if np.issubdtype(np.asarray(v).dtype, np.integer))
    per_surface = np.bincount(k, minlength=len(m.surfaces))
    per_body = np.zeros(mech.num_bodies)
    for s_, c in zip(m.surfaces, per_surface):
        per_body[s_.body] += c
    for b in range(mech.num_bodies - 1, 0, -1):
        per_body[mech.edges[b].parent] += per_body[b]
    out = np.ones(mech.num_positions)
    for b in range(1, mech.num_bodies):
        r = mech.q_range(b)
        out[r.start:r.stop] = n / max(per_body[b], 1.0)
    return out


def trace(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    by = {}
    for r in rows:
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")[:70]
        by.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for name, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        print(f"{name:70s} {len(v):6d} x {statistics.mean(v):8.2f} us (median {statistics.median(v):.2f})")
    spans, red, gap = [], [], []
    for i, r in enumerate(rows[:-1]):
        nxt = rows[i + 1]
        if "moments_kernel" in r["Kernel_Name"] and "reduce_tiles_kernel" in nxt["Kernel_Name"]:
            spans.append((int(nxt["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            red.append((int(nxt["End_Timestamp"]) - int(nxt["Start_Timestamp"])) / 1e3)
            if i > 0:
                gap.append((int(r["Start_Timestamp"]) - int(rows[i - 1]["End_Timestamp"])) / 1e3)
    if spans:
        print(f"moments + reduce: span {statistics.median(spans):.2f} us (its reduce {statistics.median(red):.2f} us; "
              f"idle before the moments launch {statistics.median(gap):.2f} us), median over {len(spans)}")


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("configs", nargs="*", default=["m64:1048576"])
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--hessian-only", action="store_true")
    p.add_argument("--json", default=None)
    p.add_argument("--trace", default=None)
    p.add_argument("--frames", type=int, default=0)
    p.add_argument("--limits", type=lambda v: [int(t) for t in v.split(",")], default=[3, 4, 6, 10])
    p.add_argument("--device-loop", action="store_true")
    p.add_argument("--prior", type=float, default=None)
    p.add_argument("--prior-scale", choices=["uniform", "subtree"], default="uniform")
    p.add_argument("--loss", default=None, help="huber:SCALE or tukey:SCALE (flash.robust.parse)")
    p.add_argument("--weights", choices=["depth", "random"], default=None,
                   help="per-point confidence weights for the resident cloud (fsdf_set_point_weights)")
    p.add_argument("--robust-loops", action="store_true",
                   help="a robust objective may run on the device-resident loops (fsdf_set_robust_loops)")
    a = p.parse_args()
    if a.loss is not None:
        from flash import robust
        a.loss = robust.parse(a.loss)
    if a.trace:
        trace(a.trace)
    elif a.frames:
        frames(a)
    else:
        run(a)
