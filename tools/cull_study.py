#!/usr/bin/env python3
"""CPU study of the scene-level culling of a seeded pass (no GPU): how many
hulls a 64-point chunk looks at under today's Phase A / wave cull / Phase C and
under one wave-level cull taken after the seeds (scene_eval's seed-first path).

The bench cloud (synthetic.depth_cloud, seed 1251, M64) at two configurations
(q_eval and q_eval + 1e-3 on every joint); the oracle's d* and k*; Morton order
standing in for the device's Hilbert order, then a stable grouping by the other
configuration's k* (the regroup); the kernel's bounds restated in numpy: hull
sphere (vertex centroid, radius), body-frame box, chunk sphere (bbox centre,
half diagonal), the 1e-5 margins. After the seeds a lane's best is taken as its
d* where its prior is its k*, else as |p - c_prior| (0.1 % of points).

    python tools/cull_study.py [--points 1048576] [--seed 1251]

Needs numpy, the oracle (make -C oracle) and the host library.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "point-cloud-signed-distance_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def morton(pts):
    lo, hi = pts.min(0), pts.max(0)
    q = ((pts - lo) / (hi - lo).max() * 1023).astype(np.uint64)
    key = np.zeros(len(pts), np.uint64)
    for b in range(10):
        for a in range(3):
            key |= ((q[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + a)
    return np.argsort(key, kind="stable")


def bounds(manip, poses):
    """Per hull: world sphere (c, r) and oriented box (centre, axes [3,3] rows, half extents)."""
    out = []
    for s, p in zip(manip.convex_surfaces(), poses):
        R, t = p[:9].reshape(3, 3), p[9:]
        v = s.hull.vertices
        c = v.mean(0)
        lo, hi = v.min(0), v.max(0)
        out.append((R @ c + t, np.linalg.norm(v - c, axis=1).max(), R @ (0.5 * (lo + hi)) + t, R.T, 0.5 * (hi - lo)))
    return out


def box_lower(b, x):
    """Lower bound of the hull's distance at x [..., 3] from its oriented box."""
    u = np.abs((x - b[2]) @ b[3].T) - b[4]
    mx = u.max(-1)
    return np.where(mx <= 0, mx, np.sqrt((np.maximum(u, 0) ** 2).sum(-1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=1251)
    a = ap.parse_args()
    import flash
    import oracle
    from flash import Models, synthetic
    m = Models.arm_grid()
    qt, qe = synthetic.perturbed_configuration(m, 1234)
    pts = synthetic.depth_cloud(m, qt, a.points, seed=a.seed, order="shuffled")
    pa, pb = flash.hull_poses(m, qe), flash.hull_poses(m, qe + 1e-3)
    om = oracle.OracleModel.from_manipulator(m)
    da, ka, _ = om.skin(pa, pts)
    _, kb, _ = om.skin(pb, pts)
    order = morton(pts)
    order = order[np.argsort(kb[order], kind="stable")]
    n = len(pts) // 64 * 64
    P, d, k, prior = (x[order][:n] for x in (pts, da, ka, kb))
    P = P.reshape(-1, 64, 3)
    d, k, prior = d.reshape(-1, 64), k.reshape(-1, 64), prior.reshape(-1, 64)
    C, K = len(P), len(pa)
    B = bounds(m, pa)
    ck = np.stack([b[0] for b in B])
    rk = np.array([b[1] for b in B])
    smax = (np.abs(ck).sum(1) + 2 * rk).max()
    lo, hi = P.min(1), P.max(1)
    cw, rw = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo, axis=1)
    Dk = np.linalg.norm(cw[:, None] - ck[None], axis=2)  # [C, K]
    boxw = np.stack([box_lower(b, cw) for b in B], 1)     # [C, K]
    base = 1.0 + np.abs(cw).sum(1) + smax + 4 * rw

    def wave_cull(u):
        mrg = 1e-5 * (base + 2 * np.abs(u))
        t = (u + mrg)[:, None]
        return (Dk - rw[:, None] - rk[None] <= t) & (boxw <= t + rw[:, None])

    cand = wave_cull((Dk + rw[:, None]).min(1))  # today's cull: UB_w = min_k D_k + r_w
    dist = np.linalg.norm(P[:, :, None] - ck[None, None], axis=3)  # [C, 64, K]
    seed = np.zeros((C, K), bool)
    np.put_along_axis(seed, prior, True, 1)
    ubp = np.take_along_axis(dist, prior[:, :, None], 2)[:, :, 0]
    best = np.where(prior == k, d, ubp)  # after the seeds
    mrg = 1e-5 * (1.0 + np.abs(P).sum(2) + smax + 2 * ubp)
    tb = (np.minimum(ubp, best) + mrg)[:, :, None]
    need = dist - rk[None, None] <= tb
    for j, b in enumerate(B):
        need[:, :, j] &= box_lower(b, P) <= tb[:, :, 0]
    any_need = need.any(1)  # [C, K]
    post = wave_cull(np.minimum(ubp, best).max(1))
    non_seed = cand & ~seed
    out = {
        "points": int(n), "chunks": int(C), "hulls": int(K),
        "kstar_differs_frac": float((ka != kb).mean()),
        "candidates_after_wave_cull": {"mean": float(cand.sum(1).mean()), "median": float(np.median(cand.sum(1))),
                                       "p90": float(np.percentile(cand.sum(1), 90))},
        "distinct_seeds": float(seed.sum(1).mean()),
        "phase_c_need_tests_today": float(non_seed.sum(1).mean()),
        "non_seed_needed_by_some_lane": float((non_seed & any_need).sum(1).mean()),
        "evaluations_per_wave_estimate": float((seed | (non_seed & any_need)).sum(1).mean()),
        "non_seed_candidates_after_seed_first_cull": {
            "mean": float((post & ~seed).sum(1).mean()), "median": float(np.median((post & ~seed).sum(1))),
            "p90": float(np.percentile((post & ~seed).sum(1), 90))},
        "needed_hull_culled_by_seed_first_cull": int((any_need & ~seed & ~post).sum()),
    }
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
