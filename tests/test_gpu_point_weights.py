"""GPU: per-point confidence weights (fsdf_set_point_weights,
csrc/point_weights.hip, the WEIGHTED instantiations of csrc/robust.hip) — the
per-surface rows against a longdouble reference, the exact identities of
uniform weights, the gather through sort and regroup, a zero weight against a
deleted point, the life cycle and the refusals, the iteration entry points and
the solver loops over the weighted objective, and estimate_state with weights.

The reference of a row is tests/test_gpu_robust.py's, restated with
aw = a · w: from the per-point k*, d*, ∇d* of fsdf_eval at the same poses, the
numpy twins of the loss and the caller's weights in numpy.longdouble,
v = (∇d*, p × ∇d*), R = Σ aw v vᵀ, the wrench Σ 2 aw d* v, Σ a ρ, Σ aw over the
n_k points of surface k. With u = 2^-53, s = (1, 1, 1, L, L, L), L = max |p|_2,
D = max |d*|, A = max a_i, A_i = Σ |2 aw d* v_i|:

    moments  |M − R|_ij  <= 2^-49 n_k (sqrt(R_ii R_jj) + A s_i s_j)
    wrench   |F − F_ref|_i <= 2^-49 n_k (A_i + 2 A D s_i)
    Σaρ      <= 2^-49 n_k (Σaρ + A max ρ)
    Σaw      <= 2^-49 n_k (Σaw + A)

These are that file's bounds with A carried into the absolute terms. Its
derivation holds with one more rounding: the weight a is the caller's fp64
number (exact), and aw = a · w adds one relative rounding u to w's absolute
error of 5u, so aw <= A carries at most (5 + 1) u A. A moment term aw v_i v_j
is then off by at most (6 + 5 + 2) u A s_i s_j = 13u A s_i s_j <= 16u A s_i s_j
(it was 12u), a wrench term 2 aw d v_i by at most (12 + 4 + 6) u A D s_i =
22u A D s_i <= 32u A D s_i = 16u · 2 A D s_i (it was 20u); a · ρ carries 9u
relative (it was 8u) and Σaw's terms 6u A each against the + A. The
fixed-order sums add n_k u Σ|term| as before: the sqrt(R_ii R_jj)
(Cauchy-Schwarz over sqrt(aw) v), A_i, Σaρ and Σaw terms."""
import ctypes

import numpy as np
import pytest

from conftest import rng
from gn_helpers import IU, surface_bodies
from test_gpu_moments import _context, _vgh_scene, scenes  # noqa: F401  (scenes: the fixture)
from test_gpu_robust import DIAG, EPS, RUN_POINTS, SIZES, _losses
from test_point_weights import ORACLE_WEIGHTS_ERR123, seed41_case

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 3


def _weights(r, n):
    """Uniform in [0, 2], about one in ten exactly 0."""
    a = r.uniform(0.0, 2.0, n)
    a[r.random(n) < 0.1] = 0.0
    return a


def _reference(pts, k, d, grad, S, loss, a):
    """longdouble (R [S, 21], wrench [S, 6], A_i [S, 6], Σaρ [S], max ρ [S], Σaw [S], n_k [S])."""
    P, G, dd, aa = (np.asarray(v, np.longdouble) for v in (pts, grad, d, a))
    w = np.ones_like(dd) if loss is None else loss.weight(dd)
    rho = dd * dd if loss is None else loss.rho(dd)
    assert w.dtype == np.longdouble and rho.dtype == np.longdouble
    aw, arho = aa * w, aa * rho
    v = np.concatenate([G, np.cross(P, G)], axis=1)
    term = v * (2 * aw * dd)[:, None]
    R, F, A = np.zeros((S, 21), np.longdouble), np.zeros((S, 6), np.longdouble), np.zeros((S, 6), np.longdouble)
    sr, mr, sw = np.zeros(S, np.longdouble), np.zeros(S, np.longdouble), np.zeros(S, np.longdouble)
    cnt = np.bincount(k, minlength=S)
    for s in np.nonzero(cnt)[0]:
        sel = k == s
        R[s] = np.einsum("ni,nj->ij", v[sel] * aw[sel, None], v[sel])[IU]
        F[s], A[s] = term[sel].sum(0), np.abs(term[sel]).sum(0)
        sr[s], mr[s], sw[s] = arho[sel].sum(), rho[sel].max(), aw[sel].sum()
    return R, F, A, sr, mr, sw, cnt


def _check_rows(ctx, poses, pts, S, loss, a, label):
    """eval_robust under `loss` with the weights `a` (caller order, as `pts`:
    the order of fsdf_eval's per-point outputs) against the reference; twice
    the same bits; moments=False the same bits of its entries. Sets the loss
    and the weights. Returns ((cost, accum, M, W), (b_m, b_f, b_c, b_w)): the
    outputs and their bounds."""
    ctx.set_loss(loss)
    ctx.set_point_weights(a)
    cost, accum, M, W = ctx.eval_robust(poses)
    again = ctx.eval_robust(poses)
    assert again[0] == cost and all(np.array_equal(u, v) for u, v in zip(again[1:], (accum, M, W))), label
    lean = ctx.eval_robust(poses, moments=False)
    assert lean[0] == cost and np.array_equal(lean[1], accum) and lean[2] is None and np.array_equal(lean[3], W), label
    assert M.shape == (S, 21) and accum.shape == (1 + 6 * S,) and W.shape == (S,)
    n = len(pts)
    if n == 0:
        assert cost == 0.0 and not accum.any() and not M.any() and not W.any(), label
        return (cost, accum, M, W), None
    _, _, (k, d, g) = ctx.eval(poses, per_point=True)  # (least squares whatever the weights: per-point outputs)
    assert k.min() >= 0 and k.max() < S
    if ctx.precision == 32:
        pts = pts.astype(np.float32)
    R, F, A, sr, mr, sw, cnt = _reference(pts, k, d, g, S, loss, a)
    L = np.sqrt((np.asarray(pts, np.float64) ** 2).sum(1)).max()
    D, amax = float(np.abs(d).max()), float(np.max(a))
    s = np.array([1.0, 1.0, 1.0, L, L, L])
    f64 = lambda v: np.asarray(v, np.float64)  # noqa: E731
    b_m = EPS * cnt[:, None] * (np.sqrt(f64(R[:, DIAG])[:, IU[0]] * f64(R[:, DIAG])[:, IU[1]]) +
                                amax * s[IU[0]] * s[IU[1]])
    b_f = EPS * cnt[:, None] * (f64(A) + 2.0 * amax * D * s[None, :])
    b_r = EPS * cnt * (f64(sr) + amax * f64(mr))
    b_w = EPS * cnt * (f64(sw) + amax)
    wrench = accum[1:].reshape(S, 6)
    e_m = f64(np.abs(np.asarray(M, np.longdouble) - R))
    e_f = f64(np.abs(np.asarray(wrench, np.longdouble) - F))
    e_w = f64(np.abs(np.asarray(W, np.longdouble) - sw))
    e_c = float(abs(np.longdouble(cost) - sr.sum()))
    b_c = float(b_r.sum()) + S * 2.0 ** -52 * float(sr.sum())  # (+ the S − 1 additions of the surfaces' sums)

    def worst(e, b):
        return float((e / np.where(b > 0, b, 1.0)).max())

    print(f"{label}: n {n}, hit {int((cnt > 0).sum())}/{S}, zero weights {int((np.asarray(a) == 0).sum())}, worst / bound: "
          f"moments {worst(e_m, b_m):.3f} wrench {worst(e_f, b_f):.3f} weight {worst(e_w, b_w):.3f} "
          f"cost {e_c / b_c if b_c else 0.0:.3f}")
    assert (e_m <= b_m).all(), (label, "moments", worst(e_m, b_m))
    assert (e_f <= b_f).all(), (label, "wrench", worst(e_f, b_f))
    assert (e_w <= b_w).all(), (label, "weight", worst(e_w, b_w))
    assert e_c <= b_c, (label, "cost", e_c, b_c)
    assert accum[0] == cost
    hit = cnt > 0
    assert not M[~hit].any() and not wrench[~hit].any() and not W[~hit].any(), label  # exactly zero
    return (cost, accum, M, W), (b_m, b_f, b_c, b_w)


# ---- 1. rows against the longdouble reference ------------------------------------------------

@pytest.mark.parametrize("sort_points", [False, True])
@pytest.mark.parametrize("scene,precision", [("box", 64), ("irb140", 64), ("irb140", 32), ("m64", 64),
                                             ("many200", 64)])
def test_weighted_rows_match_per_point_outputs(scenes, scene, precision, sort_points):  # noqa: F811
    """One box (S = 1), IRB140 (7), M64 (64: four waves per workgroup) and 200
    random hulls (one wave); Huber 0.02, Tukey 0.05 and no loss at every size of
    SIZES on one context, sorted and unsorted, the weights drawn anew for every
    cloud."""
    surfaces, poses, pool = scenes[scene]
    ctx = _context(surfaces, precision, sort_points)
    r = rng(901)
    try:
        for step, n in enumerate(SIZES):
            pts = pool[53 * step:53 * step + n]
            ctx.set_points(pts)
            a = _weights(r, n)
            for loss in _losses():
                _check_rows(ctx, poses, pts, len(surfaces), loss, a,
                            f"{scene} f{precision} sorted={sort_points} n={n} {loss!r}")
    finally:
        ctx.close()


# ---- 2. exact identities -----------------------------------------------------------------

@pytest.mark.parametrize("sort_points", [False, True])
@pytest.mark.parametrize("scene", ["irb140", "m64"])
def test_uniform_weights_scale_eval_robust_exactly(scenes, scene, sort_points):  # noqa: F811
    """Weights all 1.0: the bits of the same context without weights (1 · w and
    1 · ρ are exact). All 0.25: every output exactly 0.25 × the unweighted bits
    (a power of two scales every term and every partial sum exactly). All 0:
    exact zeros."""
    surfaces, poses, pool = scenes[scene]
    ctx = _context(surfaces, 64, sort_points)
    try:
        for n in (1, 257, 2 * RUN_POINTS + 101):
            pts = pool[11:11 + n]
            ctx.set_points(pts)
            for loss in _losses():
                ctx.set_loss(loss)
                for moments in (True, False):
                    ctx.set_point_weights(None)
                    plain = ctx.eval_robust(poses, moments=moments)
                    assert plain[0] > 0
                    for value in (1.0, 0.25, 0.0):
                        ctx.set_point_weights(np.full(n, value))
                        got = ctx.eval_robust(poses, moments=moments)
                        assert got[0] == value * plain[0], (n, loss, value)
                        for u, v in zip(got[1:], plain[1:]):
                            assert (u is None and v is None) or np.array_equal(u, value * v), (n, loss, value)
    finally:
        ctx.close()


@pytest.mark.parametrize("sort_points", [False, True])
@pytest.mark.parametrize("spec", ["huber:0.02", "tukey:0.05", "square"])
def test_unit_weights_return_the_unweighted_bits_of_the_iteration_calls(spec, sort_points):
    """value_and_gradient and value_gradient_hessian with weights all 1.0
    return the bits of the same context without weights, at the same cloud
    layout (the auto regroup switched off), under Huber and Tukey: both run the
    robust reduction. Without a loss the unweighted calls are the least-squares
    pass's own sums — another kernel and summation order — so there the two
    agree to rounding only. Weights all 0.25 scale c, g and H exactly: the
    chain rule and the Gauss-Newton matrix are linear in the sums, and a power
    of two commutes with every rounding."""
    from flash import _lib, robust
    from flash.gradientdescent import register_native
    m, pts, x = _vgh_scene("irb140")
    loss = robust.parse(spec)
    ctx = _lib.Context(device=0, precision=64, sort_points=sort_points)
    try:
        ctx.set_surfaces([("hull", (s.hull.vertices, s.hull.faces, s.hull.planes)) for s in m.surfaces])
        register_native(m, ctx, 10)
        ctx.set_regroup(False)
        ctx.set_points(pts)
        ctx.set_loss(loss)
        ctx.set_point_weights(np.ones(len(pts)))
        c1, g1 = ctx.value_and_gradient(x)
        c2, g2, H2 = ctx.value_gradient_hessian(x)
        assert c1 == c2 and np.array_equal(g1, g2)
        ctx.set_point_weights(np.full(len(pts), 0.25))
        cq, gq, Hq = ctx.value_gradient_hessian(x)
        ctx.set_point_weights(None)
        assert ctx.point_weights() is None
        if loss is not None:
            c0, g0 = ctx.value_and_gradient(x)
            c3, g3, H3 = ctx.value_gradient_hessian(x)
            assert c0 == c1 and np.array_equal(g0, g1)
            assert c3 == c2 and np.array_equal(g3, g2) and np.array_equal(H3, H2)
        else:
            # no loss, no weights: the least-squares pass's own sums, another kernel — to rounding
            c0, g0 = ctx.value_and_gradient(x)
            assert abs(c0 - c1) <= 1e-12 * c0 and np.abs(g0 - g1).max() <= 1e-12 * np.abs(g0).max()
        assert cq == 0.25 * c2 and np.array_equal(gq, 0.25 * g2) and np.array_equal(Hq, 0.25 * H2)
    finally:
        ctx.close()


# ---- 3. the gather -------------------------------------------------------------------------

def test_resident_weights_follow_the_permutation(scenes):  # noqa: F811
    surfaces, poses, pool = scenes["irb140"]
    r = rng(902)
    n = 2 * RUN_POINTS + 101
    pts, a = pool[:n], _weights(r, n)
    for sort_points in (False, True):
        ctx = _context(surfaces, 64, sort_points)
        try:
            ctx.set_points(pts)
            assert ctx.point_weights() is None
            ctx.set_point_weights(a)
            perm = ctx.permutation()
            assert np.array_equal(perm, np.arange(n)) == (not sort_points)
            assert np.array_equal(ctx.point_weights(), a[perm])
            if not sort_points:
                continue
            ctx.eval_robust(poses)  # (a pass: the regroup's groups)
            ctx.regroup_points()
            perm2 = ctx.permutation()
            assert not np.array_equal(perm2, perm) and np.array_equal(np.sort(perm2), np.arange(n))
            assert np.array_equal(ctx.point_weights(), a[perm2])
            _check_rows(ctx, poses, pts, len(surfaces), None, a, "regrouped")
            # the next frame through the prefetch: unset until set again
            pts_b, b = pool[n:n + 1000], _weights(r, 1000)
            ctx.prefetch_points(pts_b)
            ctx.eval_robust(poses)
            ctx.set_points_prefetched()
            assert ctx.point_weights() is None
            ctx.set_loss(None)
            unweighted = ctx.eval_robust(poses)
            ctx.set_point_weights(b)
            assert np.array_equal(ctx.point_weights(), b[ctx.permutation()])
            _check_rows(ctx, poses, pts_b, len(surfaces), None, b, "prefetched")
            ctx.set_point_weights(None)
            again = ctx.eval_robust(poses)
            assert again[0] == unweighted[0] and all(np.array_equal(u, v) for u, v in zip(again[1:], unweighted[1:]))
        finally:
            ctx.close()


def test_resident_weights_follow_the_auto_regroup():
    """The first value_and_gradient on a new sorted cloud queues the auto
    regroup after its robust launch: that call reads the Hilbert layout's
    weights, the next one the regrouped layout's."""
    from flash import Models, synthetic
    from flash.gradientdescent import CostFunctor
    m = Models.irb140()
    q_true, q = synthetic.perturbed_configuration(m, 41)
    pts = synthetic.depth_cloud(m, q_true, 4000, seed=43)
    a = _weights(rng(903), len(pts))
    cf = CostFunctor(m, np.zeros((0, 3)))
    ctx = cf.ctx
    ctx.set_plan(False)
    ctx.set_partition(0, 0)  # every pass one wave per chunk: the auto rule regroups
    res = []
    for auto in (False, True):
        ctx.set_regroup(auto)
        cf.set_sensed_points(pts)
        assert cf.point_weights is None and ctx.point_weights() is None
        cf.set_point_weights(a)
        perm = ctx.permutation()
        assert np.array_equal(ctx.point_weights(), a[perm])
        res.append(cf.value_and_gradient(q))
        perm2 = ctx.permutation()
        assert np.array_equal(perm2, perm) == (not auto)  # (auto: regrouped by the call above)
        assert np.array_equal(ctx.point_weights(), a[perm2])
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1])  # (the layout the pass ran on)
    again = cf.value_and_gradient(q)  # the regrouped layout: other summation order, the same sums to rounding
    assert abs(again[0] - res[0][0]) <= 1e-9 * abs(res[0][0])
    assert np.linalg.norm(again[1] - res[0][1]) <= 1e-9 * np.linalg.norm(again[1])


# ---- 4. zero weight against deletion --------------------------------------------------------

@pytest.mark.parametrize("sort_points", [False, True])
def test_zero_weights_against_the_cloud_without_those_points(scenes, sort_points):  # noqa: F811
    from flash.robust import Huber
    surfaces, poses, pool = scenes["irb140"]
    r = rng(904)
    n = 2 * RUN_POINTS + 101
    pts, a = pool[:n], _weights(r, n)
    keep = a > 0
    assert 0 < (~keep).sum() < n
    ctx = _context(surfaces, 64, sort_points)
    try:
        for loss in (Huber(0.02), None):
            ctx.set_points(pts)
            full, bf = _check_rows(ctx, poses, pts, len(surfaces), loss, a, f"zero weights {loss!r}")
            ctx.set_points(pts[keep])
            cut, bc = _check_rows(ctx, poses, pts[keep], len(surfaces), loss, a[keep], f"deleted {loss!r}")
            S = len(surfaces)
            assert (np.abs(full[2] - cut[2]) <= bf[0] + bc[0]).all()
            assert (np.abs(full[1][1:] - cut[1][1:]).reshape(S, 6) <= bf[1] + bc[1]).all()
            assert abs(full[0] - cut[0]) <= bf[2] + bc[2]
            assert (np.abs(full[3] - cut[3]) <= bf[3] + bc[3]).all()
    finally:
        ctx.close()


# ---- 5. life cycle and refusals ------------------------------------------------------------

def test_life_cycle_and_bad_arguments(scenes):  # noqa: F811
    from flash import _lib
    from flash.robust import Huber
    surfaces, poses, pool = scenes["irb140"]
    r = rng(905)
    n = 1000
    pts, a = pool[:n], _weights(r, n)
    ctx = _context(surfaces, 64, sort_points=True)
    lib, raw = ctx._lib, ctx._ctx
    try:
        ctx.set_loss(Huber(0.02))
        ctx.set_points(pts)
        unweighted = ctx.eval_robust(poses)
        ctx.set_point_weights(a)
        weighted = ctx.eval_robust(poses)
        assert weighted[0] != unweighted[0]
        # a wrong count
        ones = np.ones(n + 1)
        for m in (n - 1, n + 1, 0):
            assert lib.fsdf_set_point_weights(raw, _lib.ptr(ones), m) == ERR_ARG
        # a negative, NaN or infinite entry: refused, the earlier weights kept
        for bad in (-1e-300, float("nan"), float("inf"), -float("inf")):
            b = np.ones(n)
            b[n // 2] = bad
            with pytest.raises(_lib.FlashNativeError) as e:
                ctx.set_point_weights(b)
            assert e.value.status == ERR_ARG
            assert np.array_equal(ctx.point_weights(), a[ctx.permutation()])
        kept = ctx.eval_robust(poses)
        assert kept[0] == weighted[0] and all(np.array_equal(u, v) for u, v in zip(kept[1:], weighted[1:]))
        # ignored by the least-squares queries
        ctx.set_point_weights(None)
        plain = ctx.eval(poses)
        mom = ctx.eval_moments(poses)
        ctx.set_point_weights(a)
        got, gmom = ctx.eval(poses), ctx.eval_moments(poses)
        assert got[0] == plain[0] and np.array_equal(got[1], plain[1])
        assert gmom[0] == mom[0] and np.array_equal(gmom[2], mom[2])
        # cleared by set_points: unset, and the unweighted bits come back
        ctx.set_points(pts)
        flag = ctypes.c_int32(7)
        assert lib.fsdf_get_point_weights(raw, None, ctypes.byref(flag)) == 0 and flag.value == 0
        assert ctx.point_weights() is None
        back = ctx.eval_robust(poses)
        assert back[0] == unweighted[0] and all(np.array_equal(u, v) for u, v in zip(back[1:], unweighted[1:]))
        # a ranged cloud
        ctx.set_points_range(pool[:3000], 7, 7 + n)
        assert lib.fsdf_set_point_weights(raw, _lib.ptr(a), n) == ERR_STATE
        assert ctx.point_weights() is None
    finally:
        ctx.close()


def test_refusals_on_skins_and_in_the_required_device_loops():
    from flash import Models, _lib
    from flash.gradientdescent import CostFunctor, flatten
    m = Models.irb_and_squishable()[0]
    cf = CostFunctor(m, np.zeros((10, 3)) + 0.3)
    x = flatten(cf.state)
    with pytest.raises(NotImplementedError):
        cf.set_point_weights(np.ones(10))
    assert cf.point_weights is None
    cf.ctx.set_point_weights(np.ones(10))  # (behind the functor's back: the library refuses the calls itself)
    try:
        for call in (lambda: cf.ctx.value_and_gradient(x), lambda: cf.ctx.value_gradient_hessian(x),
                     lambda: cf.ctx.descend(x, 2, 0.1, 0.5), lambda: cf.ctx.descend_lm(x, 2, 1e-3, 0.5)):
            with pytest.raises(_lib.FlashNativeError) as e:
                call()
            assert e.value.status == ERR_STATE
    finally:
        cf.ctx.set_point_weights(None)
    assert np.isfinite(cf.value_and_gradient(x)[0])
    # a rigid scene: the required device loops are refused, modes 1 run the host loop (the same bits)
    m, pts, q0 = _vgh_scene("irb140")
    n = len(pts)
    cf = CostFunctor(m, pts)
    cf.set_point_weights(_weights(rng(906), n))
    cf.value_and_gradient(q0)  # (the cloud's first pass: the same layout for every loop)
    with pytest.raises(_lib.FlashNativeError) as e:
        cf.descend_lm(q0, 6, 1e-3, 0.5, 0.0, n, device_loop="require")
    assert e.value.status == ERR_STATE and "weights" in str(e.value)
    host = cf.descend_lm(q0, 6, 1e-3, 0.5, 0.0, n, device_loop=False)
    mode1 = cf.descend_lm(q0, 6, 1e-3, 0.5, 0.0, n, device_loop=True)
    assert np.array_equal(host[0], mode1[0]) and host[1:] == mode1[1:]
    try:
        cf.ctx.set_solver("require")
        with pytest.raises(_lib.FlashNativeError) as e:
            cf.descend(q0, 5, 0.1, 0.5, 0.0, None, n)
        assert e.value.status == ERR_STATE and "weights" in str(e.value)
        cf.ctx.set_solver(False)
        host = cf.descend(q0, 5, 0.1, 0.5, 0.0, None, n)
        cf.ctx.set_solver(True)
        mode1 = cf.descend(q0, 5, 0.1, 0.5, 0.0, None, n)
        assert np.array_equal(host[0], mode1[0]) and host[1:] == mode1[1:]
    finally:
        cf.ctx.set_solver(True)


# ---- 6. value_gradient_hessian with weights -------------------------------------------------

@pytest.mark.parametrize("spec", ["huber:0.02", "square"])
@pytest.mark.parametrize("name", ["irb140", "floating"])
def test_value_gradient_hessian_with_weights(name, spec):
    """tests/test_gpu_robust.py::test_value_gradient_hessian_with_a_loss with
    weights, its steps and tolerances: (c, g) the same bits from
    value_and_gradient and value_gradient_hessian; H within 1e-12 |T|_F of T =
    twice the numpy Gauss-Newton twin on eval_robust's weighted moments,
    exactly symmetric, H q̂ = 0 for quaternion blocks; g against central
    differences of the weighted cost cf(x) within 2^-49 n c / h + 1e-7 |g|_∞
    (h = 1e-6 on IRB140, 1e-7 on the floating scene: see there)."""
    import flash
    from flash import robust
    from flash.gradientdescent import CostFunctor
    m, pts, x = _vgh_scene(name)
    loss = robust.parse(spec)
    a = _weights(rng(907), len(pts))
    cf = CostFunctor(m, pts, loss=loss)
    cf.set_point_weights(a)
    assert np.array_equal(cf.ctx.point_weights(), a[cf.ctx.permutation()])
    cf.value_and_gradient(x)  # warm-up
    c0, g0 = cf.value_and_gradient(x)
    c, g, H = cf.value_gradient_hessian(x)
    assert c == c0 and np.array_equal(g, g0)
    c1, g1 = cf.value_and_gradient(x)
    assert c1 == c0 and np.array_equal(g1, g0) and cf(x) == c0
    again = cf.value_gradient_hessian(x)
    assert again[0] == c and np.array_equal(again[1], g) and np.array_equal(again[2], H)
    mech = m.mechanism
    cr, _, mom, W = cf.ctx.eval_robust(flash.hull_poses(m, mech.normalize(x)))
    assert abs(cr - c) <= 1e-12 * c and 0 < W.sum() < 2 * len(pts)
    T = 2.0 * mech.gauss_newton_matrix_numpy(x, surface_bodies(m), mom)
    assert np.linalg.norm(T) > 0
    assert np.linalg.norm(H - T) <= 1e-12 * np.linalg.norm(T), np.linalg.norm(H - T) / np.linalg.norm(T)
    assert np.array_equal(H, H.T)
    h, eye = (1e-7 if name == "floating" else 1e-6), np.eye(len(x))
    g_fd = np.array([(cf(x + h * e) - cf(x - h * e)) / (2 * h) for e in eye])
    err, tol = float(np.abs(g - g_fd).max()), EPS * len(pts) * c / h + 1e-7 * float(np.abs(g).max())
    print(f"{name} {spec} weighted: c {c:.6f} |g|_inf {np.abs(g).max():.4f} |g - g_fd|_inf {err:.2e} "
          f"(tolerance {tol:.2e})")
    assert err <= tol, (err, tol)
    if name == "floating":
        quats = [e.q_offset for e in mech.edges[1:] if e.joint.kind == "quaternion_floating"]
        assert len(quats) == 2
        for o in quats:
            v = np.zeros(len(x))
            v[o:o + 4] = x[o:o + 4] / np.linalg.norm(x[o:o + 4])
            assert np.linalg.norm(H @ v) <= 1e-12 * np.linalg.norm(H), np.linalg.norm(H @ v) / np.linalg.norm(H)
    # the weights leave with the cloud
    cf.set_sensed_points(pts)
    assert cf.point_weights is None and cf.ctx.point_weights() is None


# ---- 7. the loops --------------------------------------------------------------------------

@pytest.mark.parametrize("spec", ["huber:0.02", "square"])
def test_loops_with_weights_match_the_python_loops(spec):
    """tests/test_gpu_robust.py::test_loops_with_a_loss_match_the_python_loops
    with weights: fsdf_descend and fsdf_descend_lm are NaiveSolver.optimize and
    LevenbergMarquardt.optimize over the functor, the same bits, with and
    without a prior."""
    from flash import robust
    from flash.gradientdescent import CostFunctor
    from flash.tracking import LevenbergMarquardt, NaiveSolver, state_prior
    m, pts, q0 = _vgh_scene("irb140")
    n = len(pts)
    cf = CostFunctor(m, pts, loss=robust.parse(spec))
    cf.set_point_weights(_weights(rng(908), n))
    cf.value_and_gradient(q0)  # (the cloud's first pass: the same layout for every loop)

    def vg(x):
        c, g = cf.value_and_gradient(x)
        return c / n, g / n

    def vgh(x):
        c, g, H = cf.value_gradient_hessian(x)
        return c / n, g / n, H / n

    naive = NaiveSolver(len(q0), rate=0.1, max_step=0.5, iteration_limit=5, gradient_convergence_tolerance=0.0)
    x_py, f_py = naive.optimize(vg, q0)
    x, f, its = cf.descend(q0, 5, 0.1, 0.5, 0.0, None, n)
    assert its == naive.iterations == 5 and np.array_equal(x, x_py) and f == f_py
    for mu in (None, 1e-3):
        for limit, tol in ((6, 0.0), (30, 1e-4)):
            solver = LevenbergMarquardt(len(q0), iteration_limit=limit, gradient_convergence_tolerance=tol)
            x_py, f_py = solver.optimize(state_prior(vgh, q0, mu), q0)
            x, f, its, lam = cf.descend_lm(q0, limit, solver.damping, solver.max_step, tol, n, prior_weight=mu)
            assert its == solver.iterations and lam == solver.final_damping, (mu, limit)
            assert np.array_equal(x, x_py) and f == f_py, (mu, limit)
    assert not np.array_equal(x, q0)


# ---- 8. end to end -------------------------------------------------------------------------

def test_estimate_state_with_oracle_weights_reproduces_the_cpu_run():
    """tests/test_point_weights.py's seed-41 run on the device: weight 0 on the
    cloud's synthetic outliers and interior points, 10 LM evaluations, damping
    1e-3, max_step 0.5, tolerance 0, prior μ = 1e-3 — its err123 to four
    digits; a Tracker with a callable gives the same state."""
    from flash.tracking import LevenbergMarquardt, Tracker, estimate_state
    m, pts, q_true, q0, off = seed41_case()
    a = np.where(off, 0.0, 1.0)

    def solver():
        return LevenbergMarquardt(len(q0), damping=1e-3, max_step=0.5, iteration_limit=10,
                                  gradient_convergence_tolerance=0.0, prior_weight=1e-3)

    s = solver()
    x = estimate_state(m, pts, q0, solver=s, weights=a)
    assert s.iterations == 10
    err = float(np.abs(x - q_true)[:3].max())
    print(f"seed 41: err123 with oracle weights {err:.4f} (CPU {ORACLE_WEIGHTS_ERR123:.4f})")
    assert abs(err - ORACLE_WEIGHTS_ERR123) <= 5e-5, err
    seen = []
    x_cb = estimate_state(m, pts, q0, callback=lambda x, c: seen.append(c), solver=solver(), weights=lambda p: a)
    assert len(seen) == 10 and np.array_equal(x_cb, x)
    tr = Tracker(m, solver=solver(), weights=lambda p: a)
    tr.state.q[:] = q0
    assert np.array_equal(tr.step(pts), x)
