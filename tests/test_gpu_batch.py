"""GPU: gradients and Gauss-Newton moments of many candidate states in one batch
of launches (fsdf_batch_robust_poses, fsdf_batch_states, csrc/batch.hip), and the
two solver loops over a batch in lockstep (fsdf_descend_lm_batch,
fsdf_descend_batch, csrc/batch_api.hip).

1. The rows against an independent reference: flash.robust.weighted_sums on the
   CPU oracle's k*, d*, ∇d* at each candidate's poses (the fp32 oracle and the
   fp32-rounded points for an fp32 context). Its per-point terms — weighted_sums
   with every point a surface of its own, so that a "sum" is one term — are formed
   with the kernel's fp64 products, so only the summation order differs: per entry

       |got − fsum(terms)| <= (n_k − 1) · 2^-53 · Σ|term| + ulp(fsum)

   with n_k the points of that surface (for Σρ over all surfaces: n). The terms
   of a point do not depend on the other points, so they are formed once per
   (scene, precision, candidate) over the largest cloud and sliced.
2. The rows against fsdf_eval_robust on the same context: np.array_equal.
3. fsdf_batch_states against the single-state calls: np.array_equal.
4. Batch invariance, 5. read-only, 6. the loops against fsdf_lm_minimize /
   NaiveSolver.optimize over the batched evaluation of one state, and against the
   sequential host loops, 7. statuses, 8. multi_start(batched=True) end to end."""
import ctypes
import math

import numpy as np
import pytest

from conftest import rng

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
# 512 points is one workgroup's minimum run of the reduction (kRobustMinChunks = 8 chunks of 64):
# 511 / 513 straddle the first workgroup boundary, 64 ± 1 the chunk boundary
SIZES = (1, 63, 64, 65, 511, 513, 4097)
BATCHES = (1, 2, 7)
NMAX, BMAX = max(SIZES), max(BATCHES)
SLICE_ENV = "FSDF_BATCH_SLICE_BYTES"  # the byte budget of a slice of candidates (csrc/batch_api.hip)


# ---- scenes (the recipes of tests/test_gpu_score.py) ------------------------------------------------

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
    from mech_ref import scene
    m, pts, x0 = scene(shape)
    r = rng(11 + len(shape))
    X = np.asarray(x0)[None, :] + r.normal(0.0, 0.1, (BMAX, len(x0)))
    X[0] = x0
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


# SLOTS 1 / 2 / 4 of the evaluation (up to 64 / 128 / 256 surfaces) and robust_waves 4 / 2 / 1 (steps at
# 70 and 141 surfaces)
SCENES = ("single", "chain_3", "irb140", "boxes64", "boxes65", "boxes129", "boxes142")
_CACHE = {}


def _scene(name):
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
    sc["terms"] = {}
    for a in ("poses", "pts"):
        sc[a].flags.writeable = False
    _CACHE[name] = sc
    return sc


def _resident(pts, precision):
    """The points as the context holds them, widened: an fp32 context's are rounded to fp32."""
    return np.asarray(pts, np.float32).astype(np.float64) if precision == 32 else np.asarray(pts, np.float64)


def _terms(sc, precision, pts=None, loss=None, weights=None, free=None, cands=range(BMAX)):
    """Per candidate (k* [n], terms [n, 29]): the reference's per-point terms in a row's order — 21
    moments, 6 wrench, a ρ, a w — from flash.robust.weighted_sums with every point a surface of its own."""
    from flash.robust import weighted_sums
    P = sc["pts"] if pts is None else pts
    n = len(P)
    out = []
    for b in cands:
        d, k, g = sc["om"].skin(sc["poses"][b], P, precision=precision)
        cost, wrench, mom, W = weighted_sums(_resident(P, precision), np.arange(n), d, g, n, loss, weights, free)
        t = np.concatenate([mom, wrench, cost[:, None], W[:, None]], axis=1)
        t.flags.writeable = False
        out.append((np.asarray(k), t))
    return out


def _shared_terms(sc, precision):
    """The plain terms of the scene's 7 candidates over its whole cloud (cached)."""
    if precision not in sc["terms"]:
        sc["terms"][precision] = _terms(sc, precision)
    return sc["terms"][precision]


def _fsum(col):
    col = col.tolist()
    want = math.fsum(col)
    return want, max(len(col) - 1, 0) * U * math.fsum([abs(v) for v in col]) + math.ulp(want)


def _check_rows(label, k, terms, S, accum, mom, wts):
    """One candidate's outputs against fsum of the reference's terms, entry by entry."""
    worst = 0.0
    want, tol = _fsum(terms[:, 27])
    assert abs(accum[0] - want) <= tol, (label, "cost", accum[0], want, tol)
    for s in range(S):
        sel = terms[k == s]
        got = np.concatenate([mom[s], accum[1 + 6 * s:7 + 6 * s], [wts[s]]])
        for e, col in enumerate(list(range(27)) + [28]):
            want, tol = _fsum(sel[:, col])
            err = abs(got[e] - want)
            worst = max(worst, err / tol)
            assert err <= tol, (label, "surface", s, "entry", col, got[e], want, err, tol)
    return worst


def _ctx(hulls, precision=64, sort_points=False, cull=True):
    from flash import _lib
    c = _lib.Context(device=0, precision=precision, sort_points=sort_points, cull=cull)
    c.set_model(hulls)
    return c


# ---- 1 and 2: the rows against the reference and against fsdf_eval_robust ----------------------------

@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", SCENES)
def test_batch_rows_vs_reference_and_eval_robust(name, precision):
    sc = _scene(name)
    S = len(sc["hulls"])
    ref = _shared_terms(sc, precision)
    c = _ctx(sc["hulls"], precision)
    for n in SIZES:
        c.set_points(sc["pts"][:n])
        one = [c.eval_robust(sc["poses"][b]) for b in range(BMAX)]
        one8 = [c.eval_robust(sc["poses"][b], moments=False) for b in range(BMAX)]
        checked = set()
        for B in BATCHES:
            accum, mom, wts = c.batch_robust_poses(sc["poses"][:B])
            accum8, none, wts8 = c.batch_robust_poses(sc["poses"][:B], moments=False)
            assert accum.shape == (B, 1 + 6 * S) and mom.shape == (B, S, 21) and wts.shape == (B, S) and none is None
            for b in range(B):
                # (2) bit for bit what fsdf_eval_robust returns on this context, with and without moments
                assert accum[b, 0] == one[b][0]
                assert np.array_equal(accum[b], one[b][1]) and np.array_equal(mom[b], one[b][2])
                assert np.array_equal(wts[b], one[b][3])
                assert np.array_equal(accum8[b], one8[b][1]) and np.array_equal(wts8[b], one8[b][3])
                assert np.array_equal(accum8[b], accum[b]) and np.array_equal(wts8[b], wts[b])
                # (1) the independent reference (a candidate's bits are the same in every batch: once per b)
                if b not in checked:
                    k, t = ref[b]
                    worst = _check_rows(f"{name} f{precision} n={n} B={B} b={b}", k[:n], t[:n], S, accum[b], mom[b],
                                        wts[b])
                    print(f"{name} f{precision} n={n} b={b}: worst err/tol {worst:.3f}")
                    checked.add(b)
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


def _objective_cases(n, seed):
    from flash.robust import Huber, Tukey
    r = rng(seed)
    free = np.arange(n) >= n // 2
    w = r.uniform(0.0, 2.0, n)
    w[r.choice(n, n // 10, replace=False)] = 0.0
    return [("huber", Huber(0.02), None, None), ("tukey", Tukey(0.05), None, None), ("weights", None, w, None),
            ("split", None, None, free), ("all-huber", Huber(0.02), w, free), ("all-tukey", Tukey(0.05), w, free)]


@pytest.mark.parametrize("sort_points", [False, True])
@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", ["chain_3", "irb140"])
def test_batch_rows_losses_weights_free_split(name, precision, sort_points):
    """Huber, Tukey, weights in [0, 2] with exact zeros, a free split at n / 2 whose samples a body
    covers, and all three together; with and without the resident sort (the split and the weights
    then go through the permutation, and the rows are summed in the sorted order)."""
    sc = _scene(name)
    S = len(sc["hulls"])
    n = 1001
    pts = np.concatenate([sc["pts"][:n // 2], _free_points(sc, n - n // 2, 17)])
    c = _ctx(sc["hulls"], precision, sort_points=sort_points)
    c.set_points(pts)
    d0 = sc["om"].skin(sc["poses"][0], pts, precision=precision)[0]
    assert (d0[n // 2:] < 0).any()
    cands = (0, 3, 6)
    for label, loss, weights, free in _objective_cases(n, 5 + len(name)):
        c.set_loss(loss)
        c.set_point_weights(weights)
        c.set_free_split(n // 2 if free is not None else n)
        accum, mom, wts = c.batch_robust_poses(sc["poses"])
        for b in range(BMAX):
            one = c.eval_robust(sc["poses"][b])
            assert np.array_equal(accum[b], one[1]) and np.array_equal(mom[b], one[2]), (label, b)
            assert np.array_equal(wts[b], one[3]), (label, b)
        for b, (k, t) in zip(cands, _terms(sc, precision, pts, loss, weights, free, cands)):
            worst = _check_rows(f"{name} f{precision} sort={sort_points} {label} b={b}", k, t, S, accum[b], mom[b],
                                wts[b])
            print(f"{name} f{precision} sort={sort_points} {label} b={b}: worst err/tol {worst:.3f}")
    c.close()


# ---- 3: fsdf_batch_states against the single-state calls ----------------------------------------------

class _host_loops:
    """The functor's (shared) engine with the regroup off and fsdf_descend's host loop, for the
    single-state arm of a comparison; the defaults again on the way out."""

    def __init__(self, cost):
        self.ctx = cost.ctx

    def __enter__(self):
        self.ctx.set_regroup(False)
        self.ctx.set_solver(0)

    def __exit__(self, *exc):
        self.ctx.set_regroup(True)
        self.ctx.set_solver(1)


@pytest.mark.parametrize("name", ["single", "chain_3", "irb140"])
def test_batch_states_vs_single_state_calls(name):
    """(The functor's engine holds the cloud in the resident sort's order.)"""
    from flash.gradientdescent import CostFunctor
    sc = _scene(name)
    n = 1001
    pts = np.concatenate([sc["pts"][:n // 2], _free_points(sc, n - n // 2, 17)])
    for label, loss, weights, free in _objective_cases(n, 9)[0::2]:  # huber; weights; all-huber
        cost = CostFunctor(sc["m"], pts, loss=loss)
        if weights is not None:
            cost.set_point_weights(weights)
        if free is not None:
            cost.set_free_split(n // 2)
        c, g, H = cost.batch_value_gradient_hessian(sc["X"])
        c8, g8 = cost.batch_value_and_gradient(sc["X"])
        assert c.shape == (BMAX,) and g.shape == (BMAX, sc["X"].shape[1]) and H.shape == g.shape + g.shape[1:]
        assert np.array_equal(c8, c) and np.array_equal(g8, g)  # hess_out = NULL: the same (c, g)
        with _host_loops(cost):  # (the single-state calls would regroup the cloud after their first pass)
            for b in range(BMAX):
                c1, g1 = cost.value_and_gradient(sc["X"][b])
                c2, g2, H2 = cost.value_gradient_hessian(sc["X"][b])
                assert c[b] == c1 and np.array_equal(g[b], g1), (name, label, b)
                assert c[b] == c2 and np.array_equal(g[b], g2) and np.array_equal(H[b], H2), (name, label, b)
        assert np.isfinite(H).all() and np.abs(H).max() > 0


# ---- 4: batch invariance --------------------------------------------------------------------------------

def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is b
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("precision", [64, 32])
@pytest.mark.parametrize("name", ["irb140", "boxes129"])
def test_batch_bits_do_not_depend_on_the_batch(name, precision, monkeypatch):
    from flash.robust import Huber
    sc = _scene(name)
    c = _ctx(sc["hulls"], precision, sort_points=True)
    c.set_points(sc["pts"][:2000])
    c.set_loss(Huber(0.02))
    P = sc["poses"]
    whole = c.batch_robust_poses(P)
    assert _same(c.batch_robust_poses(P), whole)  # two runs of the same batch
    pick = lambda out, i: tuple(a[i] for a in out)  # noqa: E731
    for b in range(BMAX):
        assert _same(pick(c.batch_robust_poses(P[b:b + 1]), 0), pick(whole, b))  # alone
        first = np.concatenate([P[b:b + 1], P[:BMAX - 1]])
        last = np.concatenate([P[1:], P[b:b + 1]])
        assert _same(pick(c.batch_robust_poses(first), 0), pick(whole, b))
        assert _same(pick(c.batch_robust_poses(last), -1), pick(whole, b))
    # the slices a call ran, witnessed by fsdf_batch_time (a pair of events per slice)
    c.profile_pass(True)
    c.batch_time()

    def sliced():
        out = c.batch_robust_poses(P)
        return out, c.batch_time()[1]

    out, slices = sliced()
    assert _same(out, whole) and slices == 1
    monkeypatch.setenv(SLICE_ENV, "1")  # the smallest budget: one candidate per slice
    out, slices = sliced()
    assert _same(out, whole) and slices == BMAX
    # (a candidate costs its table, 36 B a point, its partials and rows — some 150 KB to 400 KB here:
    # two or three candidates per slice, so the 7 split unevenly)
    monkeypatch.setenv(SLICE_ENV, str(400000 if name == "irb140" else 900000))
    out, slices = sliced()
    print(f"{name} f{precision}: {slices} slices of 7 candidates")
    assert _same(out, whole) and 1 < slices < BMAX and BMAX % slices != 0
    monkeypatch.delenv(SLICE_ENV)
    out, slices = sliced()
    assert _same(out, whole) and slices == 1
    c.profile_pass(False)
    c.close()


# ---- 5: read-only ---------------------------------------------------------------------------------------

def test_batch_calls_leave_the_context_as_it_was(irb):
    """tests/test_gpu_score.py test_scoring_leaves_the_context_as_it_was, with a batch call in the
    scoring call's place: the permutation, the weights, the split and the loss before and after; a
    second context that never makes the call: its seeded second pass — outputs and the seed
    counters of fsdf_kernel_stats — equals the first's."""
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
    rows = a.batch_robust_poses(sc["poses"])
    assert np.isfinite(rows[0]).all()
    assert _same(state(a), before)
    sa, sb = second_pass(a), second_pass(b)
    assert _same(sa[:2], sb[:2]) and sa[2] == sb[2], (sa[2], sb[2])
    assert sa[2]["seed_first_waves"] > 0  # (the second pass did read seeds)
    again = (a.eval(sc["poses"][0], per_point=True), a.eval_robust(sc["poses"][0]))
    assert _same(a.batch_robust_poses(sc["poses"]), rows)
    assert _same((a.eval(sc["poses"][0], per_point=True), a.eval_robust(sc["poses"][0])), again)
    assert _same(again, first[0])
    a.close()
    b.close()


def test_batch_calls_leave_the_chunk_costs_and_the_prepared_states(irb):
    """A planned pass's per-chunk durations around a batch call; and the record of prepared states:
    fsdf_state_gradient accepts only the x of the last passes, and fsdf_value_and_gradient returns
    the same bits, with batched evaluations and loops of other states in between."""
    from flash.gradientdescent import CostFunctor
    from flash.robust import Huber
    sc = _scene("irb140")
    c = _ctx(sc["hulls"], 64, sort_points=True)
    c.set_plan(True, max_points=1 << 20)
    c.set_points(sc["pts"][:3000])
    out = c.eval(sc["poses"][0], per_point=True)
    costs = c.chunk_costs()
    assert len(costs) == -(-3000 // 64)
    c.batch_robust_poses(sc["poses"])
    assert np.array_equal(c.chunk_costs(), costs)
    assert _same(c.eval(sc["poses"][0], per_point=True), out)
    c.close()
    a = CostFunctor(sc["m"], sc["pts"][:3000], loss=Huber(0.02))
    X = sc["X"]
    with _host_loops(a):  # (no regroup: the layout is the same for both sequences)
        want = [a.value_and_gradient(x) for x in (X[0], X[1], X[0])]
        got = [a.value_and_gradient(X[0])]
        a.batch_value_gradient_hessian(X[2:])
        a.descend_lm_batch(X[3:5], 3, 1e-3, 0.5, 0.0, 3000)
        got.append(a.value_and_gradient(X[1]))
        a.descend_batch(X[5:], 2, 0.1, 0.5, 0.0, None, 3000)
        got.append(a.value_and_gradient(X[0]))
    assert _same(got, want)


# ---- 6: the loops -----------------------------------------------------------------------------------------

def _loop_case(name, n):
    from flash.gradientdescent import CostFunctor
    from flash.robust import Huber
    sc = _scene(name)
    return sc, CostFunctor(sc["m"], sc["pts"][:n], loss=Huber(0.02))


LOOP_CASES = [("irb140", 513), ("irb140", 3000), ("chain_3", 37)]


@pytest.mark.parametrize("name,n", LOOP_CASES)
def test_descend_lm_batch_vs_lm_minimize_and_the_host_loop(name, n):
    from flash import _lib
    from flash.tracking import state_prior
    sc, cost = _loop_case(name, n)
    X = sc["X"]
    nq = X.shape[1]
    mu = np.linspace(1e-3, 2e-3, nq)

    def reference(x0, limit, tol, prior):
        def vgh(x):
            c, g, H = cost.batch_value_gradient_hessian(x[None])
            return c[0] / n, g[0] / n, H[0] / n
        return _lib.lm_minimize(state_prior(vgh, x0, prior), x0, limit, 1e-3, 0.5, tol)

    # a tolerance between the candidates' gradient norms at their 3rd evaluation: some stop early
    probe = cost.descend_lm_batch(X[:5], 3, 1e-3, 0.5, 0.0, n)
    norms = np.array([np.linalg.norm(cost.batch_value_and_gradient(x[None])[1][0]) / n for x in probe[0]])
    tol_mid = float(np.sort(norms)[2] * 1.0000001)
    early_seen = False
    for B in (1, 5):
        for prior in (None, mu):
            for limit, tol in ((1, 0.0), (10, 0.0), (10, tol_mid)):
                xs, f, its, lam = cost.descend_lm_batch(X[:B], limit, 1e-3, 0.5, tol, n, prior_weight=prior)
                for b in range(B):
                    rx, rf, rits, rlam = reference(X[b], limit, tol, prior)
                    assert np.array_equal(xs[b], rx) and f[b] == rf and its[b] == rits and lam[b] == rlam, \
                        (name, n, B, prior is not None, limit, tol, b)
                    # the sequential host loop from the same start (Huber, regroup off): the same bits
                    with _host_loops(cost):
                        hx, hf, hits, hlam = cost.descend_lm(X[b], limit, 1e-3, 0.5, tol, n, prior_weight=prior,
                                                             device_loop=False)
                    assert np.array_equal(xs[b], hx) and f[b] == hf and its[b] == hits and lam[b] == hlam
                if B == 5 and tol > 0.0 and prior is None:
                    print(f"{name} n={n}: evaluations {its.tolist()} at tolerance {tol:.3g}")
                    early_seen = early_seen or len(set(its.tolist())) > 1
    assert early_seen  # candidates of one batch stopped after different numbers of evaluations


@pytest.mark.parametrize("name,n", LOOP_CASES)
def test_descend_batch_vs_naive_solver_and_the_host_loop(name, n):
    from flash.tracking import NaiveSolver
    sc, cost = _loop_case(name, n)
    X = sc["X"]
    nq = X.shape[1]
    div = np.linspace(1.0, 2.0, nq)

    def vg(x):
        c, g = cost.batch_value_and_gradient(x[None])
        return c[0] / n, g[0] / n

    probe = cost.descend_batch(X[:5], 4, 0.1, 0.5, 0.0, None, n)
    norms = np.array([np.linalg.norm(cost.batch_value_and_gradient(x[None])[1][0]) / n for x in probe[0]])
    tol_mid = float(np.sort(norms)[2] * 1.0000001)
    early_seen = False
    for B in (1, 5):
        for divisors in (None, div):
            for limit, tol in ((1, 0.0), (10, 0.0), (10, tol_mid)):
                xs, f, its = cost.descend_batch(X[:B], limit, 0.1, 0.5, tol, divisors, n)
                for b in range(B):
                    s = NaiveSolver(nq, rate=0.1, max_step=0.5, iteration_limit=limit,
                                    gradient_convergence_tolerance=tol, precondition_divisors=divisors)
                    rx, rf = s.optimize(vg, X[b])
                    assert np.array_equal(xs[b], rx) and f[b] == rf and its[b] == s.iterations, \
                        (name, n, B, divisors is not None, limit, tol, b)
                    with _host_loops(cost):  # the sequential host loop
                        hx, hf, hits = cost.descend(X[b], limit, 0.1, 0.5, tol, divisors, n)
                    assert np.array_equal(xs[b], hx) and f[b] == hf and its[b] == hits
                if B == 5 and tol > 0.0 and divisors is None:
                    print(f"{name} n={n}: evaluations {its.tolist()} at tolerance {tol:.3g}")
                    early_seen = early_seen or len(set(its.tolist())) > 1
    assert early_seen


# ---- 7: statuses ------------------------------------------------------------------------------------------

def test_batch_statuses(irb):
    from flash import Models, _lib, num_states
    from flash.gradientdescent import CostFunctor
    from flash.robust import Huber
    sc = _scene("irb140")
    P = np.ascontiguousarray(sc["poses"])
    S = len(sc["hulls"])
    lib = _lib.load()
    p = _lib.ptr
    c = _lib.Context(device=0, precision=64)
    acc = np.full((BMAX, 1 + 6 * S), -1.0)
    X = np.zeros((BMAX, 6))
    f, g, it = np.full(BMAX, -1.0), np.full((BMAX, 6), -1.0), np.full(BMAX, -1, np.int32)
    poses = lambda B=BMAX, P_=P, a=acc: lib.fsdf_batch_robust_poses(c._ctx, p(P_), B, p(a), None, None)  # noqa: E731
    states = lambda B=BMAX, x=X: lib.fsdf_batch_states(c._ctx, p(x), B, p(f), p(g), None)  # noqa: E731
    lm = lambda B=BMAX, x=X, limit=2, ms=0.5, npts=1.0: lib.fsdf_descend_lm_batch(  # noqa: E731
        c._ctx, p(x), B, limit, 1e-3, ms, 0.0, npts, p(f), p(it), None)
    gd = lambda B=BMAX, x=X, limit=2, ms=0.5, npts=1.0: lib.fsdf_descend_batch(  # noqa: E731
        c._ctx, p(x), B, limit, 0.1, ms, 0.0, None, npts, p(f), p(it))
    # no model (the three that need a mechanism cannot have one without a model: they refuse too)
    assert poses() == 3 and states() == 3 and lm() == 3 and gd() == 3
    c.set_model(sc["hulls"])
    # no cloud yet
    assert poses() == 3 and states() == 3 and lm() == 3 and gd() == 3
    c.set_points(sc["pts"][:500])
    # B = 0: OK, nothing written; B < 0, NULL and bad loop arguments: FSDF_ERR_ARG
    assert poses(0) == 0 and states(0) == 0 and lm(0) == 0 and gd(0) == 0
    assert (acc == -1.0).all() and (f == -1.0).all() and (g == -1.0).all() and (it == -1).all()
    assert poses(-1) == 1 and states(-1) == 1 and lm(-1) == 1 and gd(-1) == 1
    assert lib.fsdf_batch_robust_poses(c._ctx, None, BMAX, p(acc), None, None) == 1
    assert lib.fsdf_batch_robust_poses(c._ctx, p(P), BMAX, None, None, None) == 1
    assert lib.fsdf_batch_robust_poses(None, p(P), BMAX, p(acc), None, None) == 1
    assert lib.fsdf_batch_states(c._ctx, None, BMAX, p(f), p(g), None) == 1
    assert lib.fsdf_batch_states(c._ctx, p(X), BMAX, None, p(g), None) == 1
    assert lib.fsdf_batch_states(c._ctx, p(X), BMAX, p(f), None, None) == 1
    assert lib.fsdf_descend_lm_batch(c._ctx, None, BMAX, 2, 1e-3, 0.5, 0.0, 1.0, p(f), p(it), None) == 1
    assert lm(limit=-1) == 1 and lm(ms=-1.0) == 1 and lm(npts=0.0) == 1
    assert gd(limit=-1) == 1 and gd(ms=-1.0) == 1 and gd(npts=0.0) == 1
    cnt = ctypes.c_int64(0)
    assert lib.fsdf_batch_time(c._ctx, None, ctypes.byref(cnt)) == 1
    assert (acc == -1.0).all() and (f == -1.0).all()
    # no mechanism: the poses call serves, the others refuse
    assert poses() == 0 and states() == 3 and lm() == 3 and gd() == 3
    # a NaN pose entry: that candidate NaN, the others' bits unchanged
    clean = c.batch_robust_poses(P)
    bad = P.copy()
    bad[3, 2, 5] = np.nan
    bad[5, 0, 11] = np.inf
    got = c.batch_robust_poses(bad)
    keep = [0, 1, 2, 4, 6]
    for a, b in zip(got, clean):
        assert np.isnan(a[3]).all() and np.isnan(a[5]).all() and np.array_equal(a[keep], b[keep])
    # an empty cloud: exact zeros
    c.set_points(np.zeros((0, 3)))
    for a in c.batch_robust_poses(P):
        assert not a.any() and not np.signbit(a).any()
    # a ranged cloud is refused
    c.set_points_range(sc["pts"][:500], 0, 250)
    with pytest.raises(_lib.FlashNativeError) as e:
        c.batch_robust_poses(P)
    assert e.value.status == 3
    assert poses() == 3
    # a keyed cloud (an exchanged shard) is refused
    import torch
    sub = np.array(sc["pts"][:300])  # (a writable copy: torch refuses to wrap a read-only array quietly)
    d_pts = torch.from_numpy(sub).to("cuda:0")
    d_keys = torch.zeros(len(sub), dtype=torch.int32, device="cuda:0")
    d_idx = torch.arange(len(sub), dtype=torch.int64, device="cuda:0")
    c.curve_keys_device(d_pts.data_ptr(), len(sub), c.cloud_box_device(d_pts.data_ptr(), len(sub)), d_keys.data_ptr())
    c.set_points_keyed_device(d_pts.data_ptr(), d_keys.data_ptr(), d_idx.data_ptr(), len(sub))
    assert poses() == 3
    # a prefetched cloud that is not resident yet is refused; once it is, the call serves
    c.set_points(sc["pts"][:500])
    assert poses() == 0
    c.prefetch_points(sc["pts"][:400])
    assert poses() == 3
    c.set_points_prefetched()
    assert poses() == 0
    # profiling: one pair of events per slice, one slice per call here
    c.set_points(sc["pts"][:500])
    c.profile_pass(True)
    c.batch_robust_poses(P)
    c.batch_robust_poses(P[:2])
    t, calls = c.batch_time()
    assert calls == 2 and t > 0.0
    assert c.batch_time() == (0.0, 0)
    c.profile_pass(False)
    c.close()
    # an RBF scene is refused by every call
    sq = Models.squishable()
    cost = CostFunctor(sq, sc["pts"][:300])
    x = np.concatenate([sq.mechanism.zero_configuration(), np.zeros(num_states(sq) - sq.mechanism.num_positions)])
    for call in (lambda: cost.ctx.batch_states(x[None, :sq.mechanism.num_positions]),
                 lambda: cost.ctx.descend_lm_batch(x[None, :sq.mechanism.num_positions], 2, 1e-3, 0.5),
                 lambda: cost.ctx.descend_batch(x[None, :sq.mechanism.num_positions], 2, 0.1, 0.5)):
        with pytest.raises(_lib.FlashNativeError) as e:
            call()
        assert e.value.status == 3
    with pytest.raises(NotImplementedError):
        cost.batch_value_and_gradient(x[None])
    # under a mechanism (the functor's engine): the three that need one, on every state of the cloud
    arm = CostFunctor(sc["m"], sc["pts"][:500], loss=Huber(0.02))
    ctx = arm.ctx
    Xs = np.ascontiguousarray(sc["X"])
    arm.batch_value_and_gradient(Xs)  # (resident, the mechanism registered)
    three = (lambda: ctx.batch_states(Xs), lambda: ctx.descend_lm_batch(Xs, 2, 1e-3, 0.5),
             lambda: ctx.descend_batch(Xs, 2, 0.1, 0.5))

    def refused():
        for call in three:
            with pytest.raises(_lib.FlashNativeError) as err:
                call()
            assert err.value.status == 3
        with pytest.raises(_lib.FlashNativeError) as err:
            ctx.batch_robust_poses(P)
        assert err.value.status == 3

    def served():
        for call in three:
            call()
        ctx.batch_robust_poses(P)

    served()
    # a deformation alone (no RBF skin) is refused
    ctx.set_deformations(1, 10.0)
    refused()
    ctx.set_deformations(0, 10.0)
    served()
    # a pending prefetched cloud, a ranged cloud and a keyed cloud are refused
    ctx.prefetch_points(sc["pts"][:400])
    refused()
    ctx.set_points_prefetched()
    served()
    ctx.set_points_range(sc["pts"][:500], 0, 250)
    refused()
    ctx.set_points_keyed_device(d_pts.data_ptr(), d_keys.data_ptr(), d_idx.data_ptr(), len(sub))
    refused()
    # (the last refusal of csrc/batch_api.hip batch_ready, more surfaces than the robust table holds, cannot be
    # reached: the scene limit of 256 surfaces is checked before it and the table holds 282)
    # an empty cloud under a mechanism: exact zeros from fsdf_batch_states, NaN for a non-finite state
    arm.set_sensed_points(np.zeros((0, 3)))
    c0, g0, H0 = arm.batch_value_gradient_hessian(sc["X"])
    assert not c0.any() and not g0.any() and not H0.any()
    bad = sc["X"].copy()
    bad[2, 1] = np.nan
    c0, g0, H0 = arm.batch_value_gradient_hessian(bad)
    assert np.isnan(c0[2]) and np.isnan(g0[2]).all() and np.isnan(H0[2]).all()
    fin = [0, 1, 3, 4, 5, 6]
    assert not c0[fin].any() and not g0[fin].any() and not H0[fin].any()
    badP = P.copy()
    badP[4, 1, 3] = np.inf
    for a in ctx.batch_robust_poses(badP):
        assert np.isnan(a[4]).all() and not np.delete(a, 4, axis=0).any()


def test_a_nan_candidate_among_finite_ones_in_both_loops(irb):
    """A candidate whose state is NaN gets NaN (c, g, H); the loops treat it as fsdf_lm_minimize / the
    NaiveSolver rule treat a callback that returns those NaNs, and the others run as without it."""
    from flash import _lib
    from flash.tracking import NaiveSolver
    sc, cost = _loop_case("irb140", 513)
    n = 513
    X = sc["X"][:4].copy()
    X[2, 1] = np.nan
    c, g, H = cost.batch_value_gradient_hessian(X)
    assert np.isnan(c[2]) and np.isnan(g[2]).all() and np.isnan(H[2]).all()
    clean = cost.batch_value_gradient_hessian(sc["X"][:4])
    fin = [0, 1, 3]
    assert all(np.array_equal(a[fin], b[fin]) for a, b in zip((c, g, H), clean))

    def vgh(x):
        c_, g_, H_ = cost.batch_value_gradient_hessian(x[None])
        return c_[0] / n, g_[0] / n, H_[0] / n

    xs, f, its, lam = cost.descend_lm_batch(X, 6, 1e-3, 0.5, 0.0, n)
    ref = cost.descend_lm_batch(sc["X"][:4], 6, 1e-3, 0.5, 0.0, n)
    for b in range(4):
        rx, rf, rits, rlam = _lib.lm_minimize(vgh, X[b], 6, 1e-3, 0.5, 0.0)
        assert np.array_equal(xs[b], rx, equal_nan=True) and its[b] == rits and lam[b] == rlam
        assert f[b] == rf or (np.isnan(f[b]) and np.isnan(rf))
        if b != 2:
            assert np.array_equal(xs[b], ref[0][b]) and f[b] == ref[1][b] and its[b] == ref[2][b]
    assert np.isnan(f[2]) and its[2] == 1  # one evaluation, then the damping is raised past its limit

    xs, f, its = cost.descend_batch(X, 4, 0.1, 0.5, 0.0, None, n)
    ref = cost.descend_batch(sc["X"][:4], 4, 0.1, 0.5, 0.0, None, n)
    for b in range(4):
        s = NaiveSolver(6, rate=0.1, max_step=0.5, iteration_limit=4, gradient_convergence_tolerance=0.0)
        rx, rf = s.optimize(lambda x: tuple(v[0] / n for v in cost.batch_value_and_gradient(x[None])), X[b])
        assert np.array_equal(xs[b], rx, equal_nan=True) and its[b] == s.iterations
        assert f[b] == rf or (np.isnan(f[b]) and np.isnan(rf))
        if b != 2:
            assert np.array_equal(xs[b], ref[0][b]) and f[b] == ref[1][b] and its[b] == ref[2][b]
    assert np.isnan(f[2]) and its[2] == 4


# ---- 8: multi-start end to end --------------------------------------------------------------------------

OFFSET = 1.5  # rad on joint 1: the start of the plain run


def _multi_start_case():
    """The scene of tests/test_gpu_score.py test_multi_start_end_to_end."""
    from flash import Models, synthetic
    m = Models.irb140()
    q_true = np.asarray(synthetic.perturbed_configuration(m, 41)[0], np.float64)
    pts = synthetic.depth_cloud(m, q_true, 3000, seed=43, sigma=0.0, frac_surface=1.0, frac_box=0.0)
    start = q_true.copy()
    start[0] += OFFSET
    steps = np.arange(-3, 4) * 0.49
    cands = np.array([start + np.array([a, b, c, 0, 0, 0]) for a in steps for b in steps[2:5] for c in steps[2:5]])
    return m, pts, q_true, start, cands


def test_multi_start_batched_end_to_end(irb):
    from flash.gradientdescent import CostFunctor
    from flash.tracking import LevenbergMarquardt, Tracker, estimate_state, multi_start
    m, pts, q_true, start, cands = _multi_start_case()
    assert len(cands) == 63
    keep = 3
    x0, info0 = multi_start(m, pts, cands, keep=keep)
    x, info = multi_start(m, pts, cands, keep=keep, batched=True)
    assert set(info) == set(info0)
    assert np.array_equal(info["scores"], info0["scores"]) and np.array_equal(info["kept"], info0["kept"])
    assert info["refined_costs"].shape == (keep,) and info["refined"].shape == (keep, 6)
    assert info["chosen"] in info["kept"]
    assert np.abs(x[:3] - q_true[:3]).max() < 0.1
    measure = CostFunctor(m, pts)
    c_ms, c_plain = measure(x), measure(estimate_state(m, pts, start))
    print(f"batched multi_start: chosen {info['chosen']} c/N {c_ms / len(pts):.6g} (default path "
          f"{measure(x0) / len(pts):.6g}); plain run c/N {c_plain / len(pts):.6g}")
    assert c_ms <= c_plain
    # the second-order solver, and the tracker's front end
    x2, info2 = multi_start(m, pts, cands, keep=keep, batched=True,
                            solver=LevenbergMarquardt(6, iteration_limit=10, prior_weight=1e-3))
    assert np.array_equal(info2["kept"], info0["kept"]) and np.abs(x2[:3] - q_true[:3]).max() < 0.1
    tr = Tracker(m)
    tr.state.q[:] = start
    x3, info3 = tr.relocalize(pts, candidates=cands, keep=2, batched=True)
    assert np.array_equal(tr.state.q, x3) and np.abs(x3[:3] - q_true[:3]).max() < 0.1
