"""GPU: many candidate states scored in one launch (fsdf_score_poses,
fsdf_score_states, csrc/score.hip) and the multi-start front end on top of it.

The expected cost of a candidate comes from the CPU oracle's d* at its poses
(the fp32 oracle for an fp32 context; the GPU's d* equals it bit for bit,
tests/test_gpu_parity.py, tests/test_gpu_fp32_exact.py), the terms a · ρ(d*)
from flash.robust (the numpy twins of csrc/robust_impl.h, the same bits), summed
with math.fsum. The terms are non-negative, so a floating-point sum of n of them
in ANY order is within (n − 1) · 2^-53 relative of the exact sum; fsum's own
rounding adds at most one ulp of the cost:

    |cost − fsum| <= (n − 1) · 2^-53 · fsum + ulp(fsum)

Against the library's own single-state sums (fsdf_eval_robust,
fsdf_value_and_gradient) both sides are any-order sums of the same terms:
2 (n − 1) · 2^-53 relative. Every other comparison here is bit for bit.

The oracle's d* of every scene is computed once, for 7 candidates over the
largest cloud, and shared (a point's d* does not depend on the other points)."""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import rng

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SIZES = (1, 63, 64, 65, 256, 257, 4097)
BATCHES = (1, 2, 7)
NMAX, BMAX = max(SIZES), max(BATCHES)
SLICE_ENV = "FSDF_SCORE_SLICE_BYTES"  # the byte budget of a slice of posed tables (csrc/score_api.hip)


# ---- scenes --------------------------------------------------------------------------------------

def _hulls_of(m):
    return [(s.hull.vertices, s.hull.faces, s.hull.planes) for s in m.surfaces]


def _random_rotation(r):
    q = r.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _boxes(K, seed):
    """K box hulls on a jittered grid, a free pose each: (hulls, poses [BMAX, K, 12], points)."""
    from flash.models import box_hull
    r = rng(seed)
    hulls = []
    for _ in range(K):
        h = box_hull(tuple(r.uniform(0.05, 0.15, 3)))
        hulls.append((h.vertices, h.faces, h.planes))
    side = int(math.ceil(K ** (1.0 / 3.0)))
    grid = np.array([[i, j, k] for i in range(side) for j in range(side) for k in range(side)], np.float64)[:K] * 0.4
    poses = np.empty((BMAX, K, 12))
    for b in range(BMAX):
        for k in range(K):
            poses[b, k, :9] = _random_rotation(r).ravel()
            poses[b, k, 9:] = grid[k] + r.normal(0.0, 0.05, 3)
    pts = r.uniform(-0.3, 0.4 * side + 0.1, (NMAX, 3))
    return hulls, poses, pts


def _mech_scene(shape):
    import flash
    from mech_ref import _manipulator, scene
    m, pts, x0 = scene(shape)
    r = rng(11 + len(shape))
    X = np.asarray(x0)[None, :] + r.normal(0.0, 0.1, (BMAX, len(x0)))
    X[0] = x0
    # (clouds of these scenes hold 2,048 points: tiled with a small jitter up to the largest size)
    reps = -(-NMAX // len(pts))
    big = np.concatenate([pts + r.normal(0.0, 0.01, pts.shape) for _ in range(reps)])[:NMAX]
    poses = np.stack([flash.hull_poses(m, x) for x in X])
    return m, _hulls_of(m), poses, np.ascontiguousarray(big), X


def _irb_scene():
    import flash
    from flash import Models, synthetic
    m = Models.irb140()
    qt, _ = synthetic.perturbed_configuration(m, 61)
    pts = synthetic.depth_cloud(m, qt, NMAX, seed=62, order="shuffled")
    r = rng(63)
    X = np.asarray(qt)[None, :] + r.normal(0.0, 0.15, (BMAX, 6))
    poses = np.stack([flash.hull_poses(m, x) for x in X])
    return m, _hulls_of(m), poses, np.ascontiguousarray(pts), X


SCENES = ("single", "chain_3", "irb140", "boxes64", "boxes65", "boxes129")
_CACHE = {}


def _scene(name):
    """dict(hulls, poses [7, K, 12], pts [4097, 3], m / X for the mechanism scenes, om the oracle)."""
    if name in _CACHE:
        return _CACHE[name]
    import oracle
    oracle.load()
    if name.startswith("boxes"):
        hulls, poses, pts = _boxes(int(name[5:]), 7 + int(name[5:]))
        sc = dict(hulls=hulls, poses=poses, pts=pts, m=None, X=None)
    else:
        m, hulls, poses, pts, X = _irb_scene() if name == "irb140" else _mech_scene(name)
        sc = dict(hulls=hulls, poses=poses, pts=pts, m=m, X=X)
    sc["om"] = oracle.OracleModel(sc["hulls"])
    sc["d"] = {}
    for a in ("poses", "pts"):
        sc[a].flags.writeable = False
    _CACHE[name] = sc
    return sc


def _dstar(sc, precision, pts=None):
    """The oracle's d* [7, n] of the scene's candidates over its cloud (cached) or over pts."""
    if pts is None:
        if precision not in sc["d"]:
            d = np.stack([sc["om"].skin(P, sc["pts"], precision=precision)[0] for P in sc["poses"]])
            d.flags.writeable = False
            sc["d"][precision] = d
        return sc["d"][precision]
    return np.stack([sc["om"].skin(P, pts, precision=precision)[0] for P in sc["poses"]])


def _expected(d, loss=None, weights=None, free=None):
    """(fsum of the terms a ρ(d*), the tolerance of an any-order fp64 sum against it)."""
    from flash.robust import _point_factors
    terms = _point_factors(np.asarray(d, np.float64), loss, weights, free, "test")[1]
    assert (terms >= 0).all()
    want = math.fsum(terms.tolist())
    return want, (len(d) - 1) * U * want + math.ulp(want)


def _ctx(hulls, precision=64, sort_points=False, cull=True):
    from flash import _lib
    c = _lib.Context(device=0, precision=precision, sort_points=sort_points, cull=cull)
    c.set_model(hulls)
    return c


def _check(cost, d, label, **kw):
    for b in range(len(cost)):
        want, tol = _expected(d[b], **kw)
        err = abs(cost[b] - want)
        print(f"{label} b={b}: cost {cost[b]:.17g} err/tol {err / tol if tol else 0.0:.3f}")
        assert err <= tol, (label, b, cost[b], want, err, tol)


# ---- against the oracle ----------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", SCENES)
def test_score_poses_vs_oracle(name, precision):
    sc = _scene(name)
    d = _dstar(sc, precision)
    c = _ctx(sc["hulls"], precision)
    for n in SIZES:
        c.set_points(sc["pts"][:n])
        for B in BATCHES:
            cost = c.score_poses(sc["poses"][:B])
            assert cost.shape == (B,)
            _check(cost, d[:B, :n], f"{name} f{precision} n={n} B={B}")
    c.close()


def _free_points(sc, n_free, seed):
    """Points inside the scene's hulls at candidate 0's poses (convex combinations of a hull's world vertices)."""
    r = rng(seed)
    out = np.empty((n_free, 3))
    for i in range(n_free):
        k = int(r.integers(len(sc["hulls"])))
        V = sc["hulls"][k][0]
        P = sc["poses"][0, k]
        w = r.dirichlet(np.ones(len(V)))
        out[i] = (w @ V) @ P[:9].reshape(3, 3).T + P[9:]
    return out


@pytest.mark.parametrize("sort_points", [False, True])
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", ["chain_3", "irb140"])
def test_score_losses_weights_free_split(name, precision, sort_points):
    """Huber, Tukey, weights in [0, 2] with exact zeros, a free split at n / 2 whose samples a body
    covers, and all three together; with and without the resident sort (the split and the weights
    then go through the permutation)."""
    from flash.robust import Huber, Tukey
    sc = _scene(name)
    n = 1001
    r = rng(5 + len(name))
    pts = np.concatenate([sc["pts"][:n // 2], _free_points(sc, n - n // 2, 17)])
    d = _dstar(sc, precision, pts)
    free = np.arange(n) >= n // 2
    assert (d[0][free] < 0).any() and (d[:, free] >= 0).any()
    w = r.uniform(0.0, 2.0, n)
    w[r.choice(n, n // 10, replace=False)] = 0.0
    c = _ctx(sc["hulls"], precision, sort_points=sort_points)
    c.set_points(pts)
    cases = [("huber", Huber(0.02), None, None), ("tukey", Tukey(0.05), None, None), ("weights", None, w, None),
             ("split", None, None, free), ("all-huber", Huber(0.02), w, free), ("all-tukey", Tukey(0.05), w, free)]
    for label, loss, weights, split in cases:
        c.set_loss(loss)
        c.set_point_weights(weights)
        c.set_free_split(n // 2 if split is not None else n)
        cost = c.score_poses(sc["poses"])
        _check(cost, d, f"{name} f{precision} sort={sort_points} {label}", loss=loss, weights=weights, free=split)
        # the library's own single-state sums of the same terms
        for b in range(BMAX):
            one = c.eval_robust(sc["poses"][b], moments=False)[0]
            assert abs(cost[b] - one) <= 2 * (n - 1) * U * max(cost[b], one), (label, b, cost[b], one)
    c.close()


# ---- against the single-state path ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["chain_3", "irb140"])
def test_score_states_vs_value_and_gradient(name):
    from flash.gradientdescent import CostFunctor
    from flash.robust import Huber
    sc = _scene(name)
    n = 1000
    for loss in (None, Huber(0.02)):
        cost = CostFunctor(sc["m"], sc["pts"][:n], loss=loss)
        got = cost.score(sc["X"])
        assert got.shape == (BMAX,)
        for b in range(BMAX):
            one = cost.value_and_gradient(sc["X"][b])[0]
            assert abs(got[b] - one) <= 2 * (n - 1) * U * max(got[b], one), (name, loss, b, got[b], one)
        # (a list of ManipulatorState is the same call)
        from flash.core import ManipulatorState
        states = []
        for x in sc["X"]:
            s = ManipulatorState(sc["m"])
            s.q[:] = x
            states.append(s)
        assert np.array_equal(cost.score(states), got)


# ---- invariance ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", ["irb140", "boxes129"])
def test_score_bits_do_not_depend_on_the_batch(name, precision, monkeypatch):
    sc = _scene(name)
    c = _ctx(sc["hulls"], precision, sort_points=True)
    c.set_points(sc["pts"][:2000])
    P = sc["poses"]
    whole = c.score_poses(P)
    assert np.array_equal(c.score_poses(P), whole)  # two runs of the same batch
    for b in range(BMAX):
        assert c.score_poses(P[b:b + 1])[0] == whole[b]  # alone
        first = np.concatenate([P[b:b + 1], P[:BMAX - 1]])
        last = np.concatenate([P[1:], P[b:b + 1]])
        assert c.score_poses(first)[0] == whole[b] and c.score_poses(last)[-1] == whole[b]
    monkeypatch.setenv(SLICE_ENV, "1")  # the smallest budget: one candidate per slice
    assert np.array_equal(c.score_poses(P), whole)
    # (a posed table is 46,592 / 17,920 B for IRB140 in f64 / f32 and about 122 / 55 KB for the 129 boxes:
    # two to six candidates per slice, so the 7 split unevenly)
    monkeypatch.setenv(SLICE_ENV, str(120000 if name == "irb140" else 300000))
    assert np.array_equal(c.score_poses(P), whole)
    monkeypatch.delenv(SLICE_ENV)
    assert np.array_equal(c.score_poses(P), whole)
    c.close()


# ---- read-only ----------------------------------------------------------------------------------------

def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_scoring_leaves_the_context_as_it_was(irb):
    """fsdf_eval and fsdf_eval_robust with per-point outputs, the permutation, the weights, the split
    and the loss before a scoring call and after it; then a second context that never scores: its
    seeded second pass — outputs and the seed counters of fsdf_kernel_stats — equals the first's.
    (The contexts run the one-chunk-per-wave pass, the one that reads the seeds at this size.)"""
    from flash.robust import Huber
    sc = _scene("irb140")
    n = 3000
    w = rng(3).uniform(0.0, 2.0, n)

    def context():
        c = _ctx(sc["hulls"], 64, sort_points=True)
        c.set_partition(0, 0)
        c.set_plan(False)
        c.set_points(sc["pts"][:n])
        c.set_loss(Huber(0.02))
        c.set_point_weights(w)
        c.set_free_split(n - 100)
        return c

    def state(c):
        return (c.permutation(), c.point_weights(), c.get_free_split(), c.loss_setting())

    def second_pass(c):
        c.kernel_stats(True)
        out = c.eval(sc["poses"][1], per_point=True)
        s = c.kernel_stats(False)
        return out, c.eval_robust(sc["poses"][1]), {k: s[k] for k in ("wave_iters", "seed_evals", "seed_first_waves")}

    a, b = context(), context()
    first = [(c.eval(sc["poses"][0], per_point=True), c.eval_robust(sc["poses"][0])) for c in (a, b)]
    assert _same(first[0], first[1])
    before = state(a)
    cost = a.score_poses(sc["poses"])
    assert np.isfinite(cost).all()
    assert _same(state(a), before)
    sa, sb = second_pass(a), second_pass(b)
    assert _same(sa[:2], sb[:2]) and sa[2] == sb[2], (sa[2], sb[2])
    assert sa[2]["seed_first_waves"] > 0  # (the second pass did read seeds)
    # and again after a scoring call between two passes of the same context
    again = (a.eval(sc["poses"][0], per_point=True), a.eval_robust(sc["poses"][0]))
    assert np.array_equal(a.score_poses(sc["poses"]), cost)
    assert _same((a.eval(sc["poses"][0], per_point=True), a.eval_robust(sc["poses"][0])), again)
    assert _same(again, first[0])
    a.close()
    b.close()


def test_scoring_leaves_the_chunk_costs(irb):
    """A planned pass's per-chunk durations (fsdf_chunk_costs) and the pass's outputs around a scoring call."""
    sc = _scene("irb140")
    c = _ctx(sc["hulls"], 64, sort_points=True)
    c.set_plan(True, max_points=1 << 20)
    c.set_points(sc["pts"][:3000])
    out = c.eval(sc["poses"][0], per_point=True)
    costs = c.chunk_costs()
    assert len(costs) == -(-3000 // 64)
    c.score_poses(sc["poses"])
    assert np.array_equal(c.chunk_costs(), costs)
    assert _same(c.eval(sc["poses"][0], per_point=True), out)
    c.close()


# ---- statuses -----------------------------------------------------------------------------------------

def test_score_statuses(irb):
    from flash import Models, _lib
    from flash.gradientdescent import CostFunctor
    sc = _scene("irb140")
    P = np.ascontiguousarray(sc["poses"])
    lib = _lib.load()
    c = _ctx(sc["hulls"])
    out = np.full(BMAX, -1.0)
    # no cloud yet
    assert lib.fsdf_score_poses(c._ctx, _lib.ptr(P), BMAX, _lib.ptr(out)) == 3
    c.set_points(sc["pts"][:500])
    # B = 0: OK, nothing written; B < 0 and NULL: FSDF_ERR_ARG
    assert lib.fsdf_score_poses(c._ctx, _lib.ptr(P), 0, _lib.ptr(out)) == 0 and (out == -1.0).all()
    assert lib.fsdf_score_states(c._ctx, _lib.ptr(P), 0, _lib.ptr(out)) == 0 and (out == -1.0).all()
    assert lib.fsdf_score_poses(c._ctx, _lib.ptr(P), -1, _lib.ptr(out)) == 1
    assert lib.fsdf_score_poses(c._ctx, None, BMAX, _lib.ptr(out)) == 1
    assert lib.fsdf_score_poses(c._ctx, _lib.ptr(P), BMAX, None) == 1
    assert lib.fsdf_score_poses(None, _lib.ptr(P), BMAX, _lib.ptr(out)) == 1
    assert lib.fsdf_score_states(c._ctx, None, BMAX, _lib.ptr(out)) == 1
    ms, cnt = ctypes.c_double(0.0), ctypes.c_int64(0)
    assert lib.fsdf_score_time(c._ctx, None, ctypes.byref(cnt)) == 1
    assert (out == -1.0).all()
    # no mechanism
    X = np.zeros((BMAX, 6))
    assert lib.fsdf_score_states(c._ctx, _lib.ptr(X), BMAX, _lib.ptr(out)) == 3
    # a NaN pose entry: that candidate NaN, the others' bits unchanged
    clean = c.score_poses(P)
    bad = P.copy()
    bad[3, 2, 5] = np.nan
    bad[5, 0, 11] = np.inf
    got = c.score_poses(bad)
    assert np.isnan(got[3]) and np.isnan(got[5])
    keep = [0, 1, 2, 4, 6]
    assert np.array_equal(got[keep], clean[keep])
    # an empty cloud: exact zeros
    c.set_points(np.zeros((0, 3)))
    assert np.array_equal(c.score_poses(P), np.zeros(BMAX))
    # a ranged cloud is refused, as weights refuse it
    c.set_points_range(sc["pts"][:500], 0, 250)
    with pytest.raises(_lib.FlashNativeError) as e:
        c.score_poses(P)
    assert e.value.status == 3
    # profiling: one pair of events per call
    c.set_points(sc["pts"][:500])
    c.profile_pass(True)
    c.score_poses(P)
    c.score_poses(P[:2])
    t, calls = c.score_time()
    assert calls == 2 and t > 0.0
    assert c.score_time() == (0.0, 0)
    c.profile_pass(False)
    c.close()
    # an RBF scene is refused
    sq = Models.squishable()
    from flash import num_states
    cost = CostFunctor(sq, sc["pts"][:300])
    x = np.concatenate([sq.mechanism.zero_configuration(), np.zeros(num_states(sq) - sq.mechanism.num_positions)])
    with pytest.raises(_lib.FlashNativeError) as e:
        cost.score(np.stack([x, x]))
    assert e.value.status == 3


# ---- multi-start end to end -----------------------------------------------------------------------------

OFFSET = 1.5  # rad on joint 1: the start of the plain run


def _multi_start_case():
    from flash import Models, synthetic
    m = Models.irb140()
    q_true = np.asarray(synthetic.perturbed_configuration(m, 41)[0], np.float64)
    pts = synthetic.depth_cloud(m, q_true, 3000, seed=43, sigma=0.0, frac_surface=1.0, frac_box=0.0)
    start = q_true.copy()
    start[0] += OFFSET
    # a grid over joints 1-3 around the start; its node (-3, 0, 0) lies OFFSET - 3 * 0.49 = 0.03 rad from q_true
    steps = np.arange(-3, 4) * 0.49
    cands = np.array([start + np.array([a, b, c, 0, 0, 0]) for a in steps for b in steps[2:5] for c in steps[2:5]])
    return m, pts, q_true, start, cands


def test_multi_start_end_to_end(oracle_mod):
    """IRB140, 3,000 noise-free synthetic surface points at q_true. The plain run starts OFFSET =
    1.5 rad off on joint 1: on the CPU, with the oracle-backed cost (tests/gn_helpers.py OracleCost)
    and estimate_state's default solver (NaiveSolver, rate 0.1, max_step 0.5, 30 iterations), it ends
    at c/N = 1.967e-2, 1.446 rad off on joint 1, where a run started 0.02 rad from q_true ends at
    c/N = 2.789e-4 — a factor of 70.5 (offsets 0.6 and 1.0 rad gave 11.1 and 34.2); asserted here on
    the device too. 63 candidates on a grid over joints 1-3 around the far start hold one state
    0.03 rad from q_true (its oracle c/N 2.853e-4; the next two 1.225e-3 and 1.228e-3; the least
    relative gap between two neighbouring oracle costs of the 63 is 3.2e-4)."""
    import flash
    from flash.gradientdescent import CostFunctor
    from flash.tracking import estimate_state, multi_start
    m, pts, q_true, start, cands = _multi_start_case()
    assert np.abs(cands - q_true).max(axis=1).min() <= 0.05
    n = len(pts)
    # the oracle's costs of the candidates, and their ranking
    om = oracle_mod.OracleModel.from_manipulator(m)
    want = np.array([math.fsum((om.skin(flash.hull_poses(m, x), pts)[0] ** 2).tolist()) for x in cands])
    order = np.argsort(want, kind="stable")
    gaps = np.diff(want[order]) / want[order][1:]
    assert gaps.min() > 1e-9, gaps.min()  # no two oracle costs within 1e-9 relative: the ranking is decided
    keep = 3
    x, info = multi_start(m, pts, cands, keep=keep)
    assert np.array_equal(np.argsort(info["scores"], kind="stable"), order)
    assert np.array_equal(info["kept"], order[:keep])
    assert info["refined_costs"].shape == (keep,) and info["chosen"] in info["kept"]
    # the refinement is estimate_state's own path: the same state, bit for bit, and the same objective
    measure = CostFunctor(m, pts)
    x_ref = estimate_state(m, pts, cands[info["chosen"]])
    c_ms, c_ref = measure(x), measure(x_ref)
    print(f"multi_start: chosen {info['chosen']} c/N {c_ms / n:.6g}; estimate_state from it {c_ref / n:.6g}")
    assert c_ms == c_ref
    # (multi_start's own figure of it: the same sum to rounding — its cloud may have been regrouped since)
    assert info["refined_costs"].min() == pytest.approx(c_ms, rel=1e-12)
    # the plain run from the far start, and one from 0.02 rad
    near = q_true.copy()
    near[0] += 0.02
    c_plain, c_near = measure(estimate_state(m, pts, start)), measure(estimate_state(m, pts, near))
    print(f"plain run c/N {c_plain / n:.6g}, near run c/N {c_near / n:.6g}, ratio {c_plain / c_near:.1f}")
    assert c_plain >= 10.0 * c_near
    assert c_ms < c_plain


def test_tracker_relocalize(irb):
    from flash.tracking import Tracker, candidates_around
    m, pts, q_true, start, cands = _multi_start_case()
    tr = Tracker(m)
    tr.state.q[:] = start
    x, info = tr.relocalize(pts, candidates=cands, keep=2)
    assert np.array_equal(tr.state.q, x) and len(info["scores"]) == len(cands)
    assert np.abs(x[:3] - q_true[:3]).max() < 0.1
    # drawn candidates: the tracker's state first
    tr.state.q[:] = q_true
    x2, info2 = tr.relocalize(pts, sigma=0.05, count=8, keep=1, seed=3)
    assert len(info2["scores"]) == 8
    assert np.array_equal(candidates_around(m, q_true, 0.05, 8, 3)[0], q_true)
