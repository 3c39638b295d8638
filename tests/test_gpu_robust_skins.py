"""GPU: robust objectives on RBF skins and deformations behind
fsdf_set_robust_skins — the skins' robust blocks Σ 2 (aw d*) j
(csrc/robust_skin.hip) and weighted second moments Σ aw j jᵀ
(csrc/skin_moments.hip's factor variant) against their numpy twins
(flash/robust.py weighted_skin_blocks, weighted_skin_moments), known answers
through value_and_gradient, the one-sided gate, the solver loops against the
Python loops bit for bit, estimate_state end to end, and the context's buffers.

Tolerance of the blocks and the moments: max(1e-9, 100 ε) relative to the
largest entry, ε the twin's own disagreement with np.longdouble on the same
inputs (at most 1,000 points) in the arithmetic the device uses — float64, and
for the blocks of an fp32 context float32, since rbf_adjoint's arithmetic is
the context's (the moments are fp64 in either) — tests/test_gpu_skin_moments.py's
rule. Printed by each test."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_skin_moments import _box_cloud, _ctx, _posed
from test_gpu_solver_rbf import _build, _scene

pytestmark = pytest.mark.gpu

# 1, around one 64-point chunk, 1,125 = two workgroups of the skin moments, 4,097 = 65 chunks: more than one
# workgroup of the block launch (a run of 32 chunks at most up to 2^20 points: 8 here)
COUNTS = (1, 63, 64, 65, 1125, 4097)
ERR_STATE = 3


def _skin_rows(solves, rows):
    """[(surface, rows [n + 1, 4])] of the scene's skins from the flat rows."""
    out, row0 = [], 0
    for r in solves:
        out.append((r.surface, rows[row0:row0 + r.n + 1]))
        row0 += r.n + 1
    return out


def _objectives(n):
    """(name, loss, weights, split): SQUARE + weights, Huber, Tukey, a split at 0, mid-cloud and n − 1."""
    from flash.robust import Huber, Tukey
    w = np.random.default_rng(8).uniform(0.0, 2.0, n)
    w[::5] = 0.0
    return [("square+weights", None, w, None), ("huber", Huber(0.05), None, None), ("tukey", Tukey(0.15), None, None),
            ("huber+weights+split 0", Huber(0.05), w, 0), ("split mid", None, None, n // 2),
            ("tukey+split n-1", Tukey(0.15), None, n - 1)]


def _set_objective(c, loss, w, split):
    c.set_loss(loss)
    c.set_point_weights(w)
    c.set_free_split(split)


def _eps(f, dtype):
    """The twin's relative disagreement with np.longdouble on its own inputs."""
    a, b = f(dtype), f(np.longdouble)
    return max((float(np.abs(x.astype(np.longdouble) - y).max() / max(np.abs(y).max(), np.finfo(float).tiny))
                for x, y in zip(a, b)), default=0.0)


@pytest.mark.parametrize("name,precision", [("beanbag", 64), ("beanbag", 32), ("two_link_arm", 64),
                                            ("two_link_arm+beanbag", 64), ("irb_and_squishable", 64)])
def test_blocks_and_moments_match_the_twins(name, precision):
    from flash import robust, synthetic
    m, x = _build(name)
    poses, solves, rows = _posed(m, x)
    S = len(m.surfaces)
    c = _ctx(m, precision)
    c.set_robust_skins(True)
    assert c.get_robust_skins()
    c.set_rbf_params(rows)
    block_dtype = np.float64
    if precision == 32:  # (the context works on its fp32 points and rows; the blocks in fp32 arithmetic)
        rows = rows.astype(np.float32).astype(np.float64)
        block_dtype = np.float32
    skins = _skin_rows(solves, rows)
    big = synthetic.skin_cloud(m, x, max(COUNTS), seed=11) if name == "irb_and_squishable" else \
        _box_cloud(solves, max(COUNTS), 11)
    for n in COUNTS:
        pts = big[:n]
        c.set_points(pts)
        _set_objective(c, None, None, None)
        _, acc_e, (k, d, _) = c.eval(poses, per_point=True)
        if precision == 32:
            pts = pts.astype(np.float32).astype(np.float64)
        if name == "irb_and_squishable" and n >= 64:  # hull and skin lanes in one wave
            on = (k == solves[0].surface)[:n - n % 64].reshape(-1, 64)
            assert (on.any(1) & ~on.all(1)).any()
        sub = slice(0, 1000)
        for what, loss, w, split in _objectives(n):
            _set_objective(c, loss, w, split)
            cost, acc, mom, Ms, wts = c.eval_robust_skins(poses)
            cost2, acc2, mom2, Ms2, wts2 = c.eval_robust_skins(poses)
            assert cost == cost2 and np.array_equal(acc, acc2) and np.array_equal(mom, mom2)  # the same bits twice
            assert np.array_equal(wts, wts2) and all(np.array_equal(a, b) for a, b in zip(Ms, Ms2))
            acc8 = c.eval_robust_skins(poses, moments=False)[1]  # (without the moments: the same accumulator)
            assert np.array_equal(acc, acc8)
            assert acc.shape == acc_e.shape
            free = None if split is None else np.arange(n) >= split
            off = 1 + 6 * S
            for (surface, _), M in zip(skins, Ms):  # a skin's wrench and moments row stay zero
                assert not acc[1 + 6 * surface: 7 + 6 * surface].any() and not mom[surface].any()
                assert np.array_equal(M, M.T)
            want = robust.weighted_skin_blocks(pts, k, d, skins, loss, w, free)
            wantM = robust.weighted_skin_moments(pts, k, d, skins, loss, w, free)
            ws, fs = (None if w is None else w[sub]), (None if free is None else free[sub])
            eps_b = _eps(lambda t: robust.weighted_skin_blocks(pts[sub], k[sub], d[sub], skins, loss, ws, fs, dtype=t),
                         block_dtype)
            eps_m = _eps(lambda t: robust.weighted_skin_moments(pts[sub], k[sub], d[sub], skins, loss, ws, fs, dtype=t),
                         np.float64)
            for (surface, sr), wb, wm, M in zip(skins, want, wantM, Ms):
                mlen = len(wb)
                got = acc[off: off + mlen]
                off += mlen
                if not (k == surface).any():
                    assert not got.any() and not M.any()
                    continue
                tol_b, tol_m = max(1e-9, 100.0 * eps_b), max(1e-9, 100.0 * eps_m)
                sb, sm = max(np.abs(wb).max(), 1e-300), max(np.abs(wm).max(), 1e-300)
                err_b, err_m = np.abs(got - wb).max() / sb, np.abs(M - wm).max() / sm
                print(f"{name} f{precision} n={n} {what} surface {surface}: block err {err_b:.3e} (eps {eps_b:.3e}, "
                      f"tol {tol_b:.3e}), moments err {err_m:.3e} (eps {eps_m:.3e}, tol {tol_m:.3e})")
                if np.abs(wb).max() > 0:
                    assert err_b <= tol_b, (n, what, err_b, tol_b)
                else:
                    assert not got.any()
                if np.abs(wm).max() > 0:
                    assert err_m <= tol_m, (n, what, err_m, tol_m)
                else:
                    assert not M.any()
            assert off == len(acc)
    c.close()


def test_unit_factor_matches_the_plain_kernels():
    """aw ≡ 1 (weights ≡ 1 under SQUARE): the blocks are the pass's own to rounding (the same
    summands, another order), the weighted moments eval_skin_moments' within the twins' rule."""
    from flash import rbf
    for name in ("beanbag", "irb_and_squishable"):
        m, x = _build(name)
        poses, solves, rows = _posed(m, x)
        c = _ctx(m)
        c.set_robust_skins(True)
        c.set_rbf_params(rows)
        from flash import synthetic
        pts = synthetic.skin_cloud(m, x, 1125, seed=11)
        c.set_points(pts)
        cost_e, acc_e, (k, d, _) = c.eval(poses, per_point=True)
        _, _, Ms_plain = c.eval_skin_moments(poses)
        c.set_point_weights(np.ones(len(pts)))
        cost, acc, _, Ms, _ = c.eval_robust_skins(poses)
        off = 1 + 6 * len(m.surfaces)
        scale = np.abs(acc_e[off:]).max()
        assert np.allclose(acc[off:], acc_e[off:], rtol=1e-9, atol=1e-9 * scale), np.abs(acc - acc_e)[off:].max() / scale
        assert cost == pytest.approx(cost_e, rel=1e-12)
        for r, M, P in zip(solves, Ms, Ms_plain):
            J = rbf.skin_jacobian(r.centres, r.u, pts[k == r.surface][:1000])
            Jl = rbf.skin_jacobian(r.centres, r.u, pts[k == r.surface][:1000], dtype=np.longdouble)
            eps = float(np.abs(J.T @ J - Jl.T @ Jl).max() / np.abs(Jl.T @ Jl).max())
            err = np.abs(M - P).max() / np.abs(P).max()
            print(f"{name}: weighted moments with aw = 1 against eval_skin_moments: err {err:.3e}, eps {eps:.3e}")
            assert err <= max(1e-9, 100.0 * eps)
        c.close()


def test_switch_off_or_never_used_changes_nothing():
    """A context with the switch on and no robust objective returns eval's and
    value_and_gradient's bits of one with it off; off, the skins are refused as before."""
    from flash import Models, _lib
    from flash.gradientdescent import CostFunctor
    from flash.robust import Huber
    for name in ("c3_beanbag", "c5_scene"):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        res = []
        for on in (False, True):
            m = Models.beanbag() if name == "c3_beanbag" else Models.irb_and_squishable()[0]
            cf = CostFunctor(m, z["points"], robust_skins=on)
            assert cf.ctx.get_robust_skins() is on
            c, g = cf.value_and_gradient(z["x"])
            cost, acc, _ = cf.ctx.eval(z["poses"])
            res.append((c, g, cost, acc))
            if not on:  # today's refusals, by the functor and by the library
                with pytest.raises(NotImplementedError):
                    cf.set_loss(Huber(0.05))
                cf.ctx.set_loss(Huber(0.05))
                for call in (lambda: cf.ctx.value_and_gradient(z["x"]), lambda: cf.ctx.eval_robust(z["poses"]),
                             lambda: cf.ctx.eval_robust_skins(z["poses"])):
                    with pytest.raises(_lib.FlashNativeError) as e:
                        call()
                    assert e.value.status == ERR_STATE
                cf.ctx.set_loss(None)
            else:  # eval_robust itself keeps refusing skins
                with pytest.raises(_lib.FlashNativeError) as e:
                    cf.ctx.eval_robust(z["poses"])
                assert e.value.status == ERR_STATE
        (c0, g0, cost0, acc0), (c1, g1, cost1, acc1) = res
        assert c0 == c1 and cost0 == cost1 and np.array_equal(g0, g1) and np.array_equal(acc0, acc1)
    # (enable is 0 or 1: anything else is refused and the setting stays)
    assert cf.ctx._lib.fsdf_set_robust_skins(cf.ctx._ctx, 2) != 0 and cf.ctx.get_robust_skins()


def _known(name):
    from flash import Models
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    m = Models.beanbag() if name == "c3_beanbag" else Models.irb_and_squishable()[0]
    return z, m


def _acc_grad(cf, z):
    """(the robust accumulator, the chained gradient) of the functor at the golden state."""
    c, g = cf.value_and_gradient(z["x"])
    return cf.ctx.eval_robust_skins(z["poses"], moments=False)[1], g


def _close(acc, g, acc_want, g_want):
    assert np.allclose(acc, acc_want, rtol=1e-9, atol=1e-9 * np.abs(acc_want).max()), np.abs(acc - acc_want).max()
    assert np.allclose(g, g_want, rtol=1e-7, atol=1e-7 * np.abs(g_want).max()), np.abs(g - g_want).max()


@pytest.mark.parametrize("name", ["c3_beanbag", "c5_scene"])
def test_known_answers_through_value_and_gradient(name):
    """tests/test_gpu_rbf.py's tolerances: the accumulator at 1e-9, the chained gradient at 1e-7."""
    from flash.gradientdescent import CostFunctor
    from flash.robust import Huber
    z, m = _known(name)
    pts, n = z["points"], len(z["points"])
    cf = CostFunctor(m, pts, robust_skins=True)
    # weights ≡ 1 under SQUARE, and a Huber that never bends: least squares (the golden vectors)
    cf.set_point_weights(np.ones(n))
    _close(*_acc_grad(cf, z), z["accum"], z["dcdx"])
    cf.set_point_weights(None)
    cf.set_loss(Huber(1e30))
    _close(*_acc_grad(cf, z), z["accum"], z["dcdx"])
    cf.set_loss(None)
    # a 0/1 mask is the subcloud; weight 2 is each point sent twice
    mask = (np.arange(n) % 3 != 0).astype(np.float64)
    cf.set_point_weights(mask)
    acc_m, g_m = _acc_grad(cf, z)
    cf.set_point_weights(np.full(n, 2.0))
    acc_2, g_2 = _acc_grad(cf, z)
    cf.set_point_weights(None)
    for cloud, acc, g in ((pts[mask > 0], acc_m, g_m), (np.concatenate([pts, pts]), acc_2, g_2)):
        ref = CostFunctor(_known(name)[1], cloud)  # (a model, and so an engine, of its own)
        c_ref, g_ref = ref.value_and_gradient(z["x"])
        _close(acc, g, ref.ctx.eval(z["poses"])[1], g_ref)


@pytest.mark.parametrize("name", ["beanbag", "irb_and_squishable"])
def test_one_sided_is_the_weighted_kernel_with_gated_weights(name):
    """Blocks and moments under a split equal, bit for bit, the weighted ones given a · [d* < 0] on the samples."""
    from flash import synthetic
    from flash.robust import Huber
    m, x = _build(name)
    poses, solves, rows = _posed(m, x)
    c = _ctx(m)
    c.set_robust_skins(True)
    c.set_rbf_params(rows)
    n = 1125
    pts = synthetic.skin_cloud(m, x, n, seed=11)
    pts = pts + np.random.default_rng(2).normal(0.0, 0.01, pts.shape)  # (both signs of d*)
    c.set_points(pts)
    d = c.eval(poses, per_point=True)[2][1]
    a = np.random.default_rng(3).uniform(0.5, 1.5, n)
    for split in (0, n // 2, n - 1):
        free = np.arange(n) >= split
        assert split == n - 1 or ((d[free] < 0).any() and (d[free] >= 0).any())
        for loss in (None, Huber(0.005)):
            _set_objective(c, loss, a, split)
            one = c.eval_robust_skins(poses)
            _set_objective(c, loss, np.where(free & ~(d < 0), 0.0, a), None)
            two = c.eval_robust_skins(poses)
            assert one[0] == two[0] and np.array_equal(one[1], two[1]) and np.array_equal(one[2], two[2])
            assert all(np.array_equal(p, q) for p, q in zip(one[3], two[3])) and np.array_equal(one[4], two[4])
    c.close()


def test_no_point_on_the_skin_and_no_point_at_all():
    from flash import synthetic
    from flash.robust import Huber
    m, x = _build("irb_and_squishable")
    poses, solves, rows = _posed(m, x)
    c = _ctx(m)
    c.set_robust_skins(True)
    c.set_loss(Huber(0.05))
    c.set_rbf_params(rows)
    verts = np.concatenate([v for v, _ in synthetic.world_hulls(m, x[:m.mechanism.num_positions])[:3]])
    c.set_points(verts)
    _, _, (k, _, _) = c.eval(poses, per_point=True)
    assert (k != solves[0].surface).all()
    cost, acc, mom, Ms, wts = c.eval_robust_skins(poses)
    off = 1 + 6 * len(m.surfaces)
    assert len(acc) == off + 56 and not acc[off:].any() and not Ms[0].any() and wts[:3].any()
    c.set_points(np.zeros((0, 3)))
    cost, acc, mom, Ms, wts = c.eval_robust_skins(poses)
    assert cost == 0.0 and not acc.any() and not mom.any() and not Ms[0].any() and not wts.any()
    c.close()


def test_descend_with_huber_equals_the_python_loop():
    from flash._lib import FlashNativeError
    from flash.gradientdescent import CostFunctor
    from flash.robust import Huber
    from flash.tracking import NaiveSolver
    m, pts, x0 = _scene("beanbag")
    n = float(len(pts))
    cf = CostFunctor(m, pts, loss=Huber(0.02), robust_skins=True)
    try:
        cf.value_and_gradient(x0)

        def vg(x):
            c, g = cf.value_and_gradient(x)
            return c / n, g / n

        naive = NaiveSolver(len(x0), rate=0.1, max_step=0.5, iteration_limit=6, gradient_convergence_tolerance=0.0)
        x_py, f_py = naive.optimize(vg, x0)
        cf.ctx.set_solver(False)
        x, f, its = cf.descend(x0, 6, 0.1, 0.5, 0.0, None, n)
        assert its == naive.iterations == 6 and np.array_equal(x, x_py) and f == f_py
        assert not np.array_equal(x, x0)
        for mode in (True, "all"):  # the host loop serves it: the same bits
            cf.ctx.set_solver(mode)
            x2, f2, its2 = cf.descend(x0, 6, 0.1, 0.5, 0.0, None, n)
            assert its2 == its and f2 == f and np.array_equal(x2, x)
        for mode in ("require", "require-all"):
            cf.ctx.set_solver(mode)
            with pytest.raises(FlashNativeError) as e:
                cf.descend(x0, 6, 0.1, 0.5, 0.0, None, n)
            assert e.value.status == ERR_STATE
        c_huber = cf.value_and_gradient(x0)[0]  # (the Huber objective is not least squares here)
        cf.set_loss(None)
        assert cf.value_and_gradient(x0)[0] > c_huber
    finally:
        cf.ctx.set_solver(True)
        cf.ctx.set_loss(None)
        cf.ctx.set_robust_skins(False)


@pytest.mark.parametrize("name", ["squishable", "irb_and_squishable"])
@pytest.mark.parametrize("prior", [None, 1e-3])
def test_descend_lm_equals_the_python_loop(name, prior):
    """tests/test_gpu_skin_moments.py::test_descend_lm_equals_the_python_loop under a Huber loss and weights."""
    from flash._lib import FlashNativeError
    from flash.gradientdescent import CostFunctor
    from flash.robust import Huber
    from flash.tracking import LevenbergMarquardt, state_prior
    m, pts, x0 = _scene(name)
    n = float(len(pts))
    cf = CostFunctor(m, pts, skin_hessian=True, loss=Huber(0.02), robust_skins=True)
    try:
        cf.set_point_weights(np.random.default_rng(4).uniform(0.5, 1.5, len(pts)))
        limit = 8
        c, g, H = cf.value_gradient_hessian(x0)
        c2, g2 = cf.value_and_gradient(x0)
        assert c == c2 and np.array_equal(g, g2) and np.array_equal(H, H.T)
        got = cf.descend_lm(x0, limit, 1e-3, 0.5, 1e-6, n, prior_weight=prior)

        def wrapped(x):
            c, g, H = cf.ctx.value_gradient_hessian(x)
            return c / n, g / n, H / n

        solver = LevenbergMarquardt(len(x0), iteration_limit=limit, skins=True)
        x, f = solver.optimize(state_prior(wrapped, x0, prior), x0)
        assert got[2] == solver.iterations and got[3] == solver.final_damping
        assert got[1] == f and np.array_equal(got[0], x)
        assert got[2] > 1 and f < wrapped(x0)[0]
        same = cf.descend_lm(x0, limit, 1e-3, 0.5, 1e-6, n, prior_weight=prior, device_loop=True)
        assert same[1:] == got[1:] and np.array_equal(same[0], got[0])
        with pytest.raises(FlashNativeError) as e:
            cf.descend_lm(x0, limit, 1e-3, 0.5, 1e-6, n, prior_weight=prior, device_loop="require")
        assert e.value.status == ERR_STATE
        # without lm_skins the Hessian of such a scene is refused, the gradient served
        cf.ctx.set_lm_skins(False)
        with pytest.raises(FlashNativeError) as e:
            cf.ctx.value_gradient_hessian(x0)
        assert e.value.status == ERR_STATE
        assert cf.ctx.value_and_gradient(x0)[0] == c
    finally:
        cf.set_skin_hessian(False)  # (the scene's engine is shared with other tests: as it was)
        cf.ctx.set_loss(None)
        cf.ctx.set_robust_skins(False)


def test_hessian_matches_the_twin():
    """value_gradient_hessian under Huber + weights on squishable against the twin Gauss-Newton
    Hessian from the device's per-point outputs (tests/test_gpu_skin_moments.py's rule)."""
    from flash import rbf, robust
    from flash.gradientdescent import CostFunctor
    m, pts, x0 = _scene("squishable")
    loss = robust.Huber(0.02)
    w = np.random.default_rng(4).uniform(0.0, 1.5, len(pts))
    cf = CostFunctor(m, pts, skin_hessian=True, loss=loss, robust_skins=True)
    try:
        cf.set_point_weights(w)
        c, g, H = cf.value_gradient_hessian(x0)
        k, d, _ = cf.per_point(x0)
        _, solves, _ = _posed(m, x0)
        Ms = robust.weighted_skin_moments(pts, k, d, solves, loss, w)
        sub = slice(0, 1000)
        eps = _eps(lambda t: robust.weighted_skin_moments(pts[sub], k[sub], d[sub], solves, loss, w[sub], dtype=t),
                   np.float64)
        want = rbf.gauss_newton(m, x0, solves, Ms, None, cf.weight)
        err = np.abs(H - want).max() / np.abs(want).max()
        tol = max(1e-9, 100.0 * eps)
        print(f"squishable huber + weights: H err {err:.3e}, eps {eps:.3e}, tol {tol:.3e}")
        assert err <= tol, (err, tol)
    finally:
        cf.set_skin_hessian(False)
        cf.ctx.set_loss(None)
        cf.ctx.set_robust_skins(False)


@pytest.mark.parametrize("seed", [12, 7, 19])
def test_huber_halves_the_error_end_to_end(seed, oracle_mod):
    """tests/test_robust_skins.py's cluttered squishable through estimate_state on the device:
    Huber(0.0075)'s translation error and max |δ| each below half of least squares'. On the CPU
    twin (the same seeds): least squares 0.0081 / 0.0070, 0.0068 / 0.0070, 0.0073 / 0.0065 against
    Huber 0.0017 / 0.0013, 0.0016 / 0.0013, 0.0015 / 0.0015."""
    from flash.robust import Huber
    from flash.tracking import LevenbergMarquardt, estimate_state
    from test_robust_skins import _payoff_scene, payoff_cloud, payoff_errors
    m, x_true, pts, lo, hi = _payoff_scene()
    cloud, _ = payoff_cloud(pts, lo, hi, seed)
    x0 = x_true + np.random.default_rng(seed).normal(0.0, 0.03, len(x_true))
    try:
        x_ls = estimate_state(m, cloud, x0, solver=LevenbergMarquardt(len(x0), skins=True))
        x_h = estimate_state(m, cloud, x0, solver=LevenbergMarquardt(len(x0), skins=True), loss=Huber(0.0075),
                             robust_skins=True)
    finally:
        m.engine().set_loss(None)
        m.engine().set_robust_skins(False)
        m.engine().set_lm_skins(False)
    (t_ls, d_ls), (t_h, d_h) = payoff_errors(m, x_true, x_ls), payoff_errors(m, x_true, x_h)
    print(f"seed {seed} (GPU): least squares {t_ls:.4f} / {d_ls:.4f}, Huber(0.0075) {t_h:.4f} / {d_h:.4f}")
    assert t_h < 0.5 * t_ls, (t_h, t_ls)
    assert d_h < 0.5 * d_ls, (d_h, d_ls)


def test_depth_frame_with_free_space_on_a_skin():
    """A DepthFrame with FreeSpace on a scene with a skin makes resident the bits of
    set_points(free_space_points twin) + set_free_split, checked on value_and_gradient."""
    from flash import Models
    from flash._lib import FlashNativeError
    from flash.depthsensors import DepthFrame, FreeSpace, Kinect
    from flash.geometry import Transform
    from flash.gradientdescent import CostFunctor
    m, x = _build("squishable")
    _, solves, _ = _posed(m, x)
    centre = solves[0].centres.mean(0)
    sensor = Kinect(17, 31)
    tform = Transform(np.eye(3), centre - np.array([0.0, 0.0, 1.0]))
    depth = np.random.default_rng(6).uniform(0.9, 1.1, (17, 31))
    depth[::4, ::3] = np.nan
    fs = FreeSpace(samples=3, stride=2, gap=0.02, spacing=0.05)
    frame = DepthFrame(depth, sensor, tform, free_space=fs)
    x0 = x + np.random.default_rng(12).normal(0.0, 0.03, len(x))
    cf = CostFunctor(m, frame, robust_skins=True)
    try:
        ns, n = cf.n_surface, cf.n_points
        assert ns == frame.n_surface() and n > ns and cf.ctx.get_free_split() == ns
        c, g = cf.value_and_gradient(x0)
        d = cf.per_point(x0)[1]
        assert (d[ns:] < 0).any() and (d[ns:] > 0).any()
        twin = CostFunctor(Models.squishable(), frame.points()[0], robust_skins=True)
        twin.set_free_split(ns)
        c2, g2 = twin.value_and_gradient(x0)
        assert c == c2 and np.array_equal(g, g2)
        plain = CostFunctor(Models.squishable(), frame.points()[0])
        assert plain.value_and_gradient(x0)[0] > c  # (the samples outside the model do not count)
        # without the switch the frame's objective is refused by the library, as before
        off = CostFunctor(Models.squishable(), frame)
        with pytest.raises(FlashNativeError) as e:
            off.value_and_gradient(x0)
        assert e.value.status == ERR_STATE
    finally:
        cf.ctx.set_free_space(None)
        cf.ctx.set_robust_skins(False)


def test_buffers_follow_cloud_sizes_and_a_model_swap():
    """One context walked 1,000 -> 65,573 -> 64 points and a model swap (beanbag ->
    irb_and_squishable), every step against a fresh context, bit for bit
    (tests/test_gpu_lm_device.py::test_buffers_follow_cloud_sizes_and_a_model_swap)."""
    from flash import _lib, synthetic
    from flash.core import ConvexGeometry
    from flash.robust import Huber

    def surfaces(m):
        return [("hull", (s.hull.vertices, s.hull.faces, s.hull.planes)) if isinstance(s, ConvexGeometry)
                else ("rbf", len(s.surface_points) + len(s.skeleton_points)) for s in m.surfaces]

    def load(c, m, rows, pts, w):
        c.set_surfaces(surfaces(m))
        c.set_robust_skins(True)
        c.set_loss(Huber(0.05))
        c.set_rbf_params(rows)
        c.set_points(pts)
        c.set_point_weights(w)
        c.set_free_split(len(pts) // 2)

    walked = _lib.Context(device=0)
    try:
        for name, n in (("beanbag", 1000), ("beanbag", 65573), ("beanbag", 64), ("irb_and_squishable", 1000),
                        ("irb_and_squishable", 65573), ("beanbag", 64)):
            m, x = _build(name)
            poses, solves, rows = _posed(m, x)
            pts = synthetic.skin_cloud(m, x, n, seed=n)
            w = np.random.default_rng(n).uniform(0.0, 2.0, n)
            load(walked, m, rows, pts, w)
            fresh = _lib.Context(device=0)
            load(fresh, m, rows, pts, w)
            a, b = walked.eval_robust_skins(poses), fresh.eval_robust_skins(poses)
            fresh.close()
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (name, n)
            assert all(np.array_equal(p, q) for p, q in zip(a[3], b[3])) and np.array_equal(a[4], b[4]), (name, n)
            assert a[1][1 + 6 * len(m.surfaces):].any()
    finally:
        walked.close()
