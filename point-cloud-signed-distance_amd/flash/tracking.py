"""module Flash.Tracking (src/tracking.jl) — `track!`.

estimate_state(manipulator, sensed_points, x_estimated; callback, solver)
(src/tracking.jl:8-27): wraps the cost as c/N with a callback(x, c) on every
evaluation (:16-21), hands it to a gradient-descent solver warm-started at
x_estimated (:23-26), and returns the solution.

The frame loop around it is the notebooks' (examples/irb_and_squishable.ipynb
cells 11-12): for every KINECT_POINTS_REDUCED message, sensed_points =
msg.points[1:200:end] and gradient_descent!(state, model, sensed_points) runs
estimate_state from the current state with NaiveSolver(num_states; rate=0.5,
max_step=0.1, iteration_limit=1) and writes the solution back into the state
(unflatten!) — the warm start carried from frame to frame. `track` restates
that loop; `Tracker` is its resident form (one device context and CostFunctor
for the whole sequence, the cloud swapped per frame).

The solver lives in the un-vendored SimpleGradientDescent.jl @0fcc1f95
(REQUIRE.dev:24). `NaiveSolver` below restates its interface (num_vars, rate,
max_step, iteration_limit, gradient_convergence_tolerance,
precondition_divisors — the kwargs examples/irb140.ipynb cell 9 and
examples/squishable.ipynb cell 9 pass). Its update rule is pinned by the
reference notebook's own per-trial traces (examples/manipulator.ipynb cells
9/10/14, fixture tests/golden/manipulator_traces.json,
tests/test_manipulator_traces.py): the step is −rate·∇f (κ = rate measured
within 2 % from single trajectories at two rates), clipped component-wise at
max_step (the far set's largest |Δerr| per step is max_step·√2), one
objective evaluation per iteration, and a positive default convergence
tolerance (trials stop early; 1e-3 estimated from where they stop). Trajectory
parity on the RBF scene itself is not reached: the landscape diverges
(DESIGN.md §2).
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field

import numpy as np

from .core import Manipulator, ManipulatorState, num_states
from .depthsensors import DepthFrame
from .gradientdescent import CostFunctor, flatten, unflatten


@dataclass
class NaiveSolver:
    """NaiveSolver(num_vars; rate, max_step, iteration_limit,
    gradient_convergence_tolerance, precondition_divisors): per iteration
    g ← ∇f(x) ./ precondition_divisors; stop when ‖g‖ < tolerance; else
    x ← x + clamp(−rate·g, ±max_step) (component-wise). Rule and default
    tolerance per the notebook traces (module docstring)."""
    num_vars: int
    rate: float = 0.1
    max_step: float = 0.5
    iteration_limit: int = 30
    gradient_convergence_tolerance: float = 1e-3
    precondition_divisors: np.ndarray | None = None
    iterations: int = field(default=0, init=False)  # of the last optimize

    def optimize(self, value_and_gradient, x0):
        x = np.array(x0, np.float64, copy=True)
        div = np.ones(self.num_vars) if self.precondition_divisors is None else np.broadcast_to(
            np.asarray(self.precondition_divisors, np.float64), x.shape)
        f = None
        self.iterations = 0
        for _ in range(self.iteration_limit):
            f, g = value_and_gradient(x)
            self.iterations += 1
            g = g / div
            if np.linalg.norm(g) < self.gradient_convergence_tolerance:
                break
            x = x + np.clip(-self.rate * g, -self.max_step, self.max_step)
        return x, f


def state_prior(value_gradient_hessian, x_ref, weight):
    """Wrap an objective x -> (f, g, H) in a prior on the frame's start state:
    F(x) = f(x) + Σ_i μ_i (x_i − x̄_i)², x̄ = x_ref, μ = weight (a scalar or one
    value per coordinate, each >= 0). Gauss-Newton moves the coordinates a noisy
    cloud does not determine (IRB140's wrist: H_ii/N of 6e-5 .. 3e-9 against
    1e-2 .. 7e-2 for joints 1-3) by 1-1.5 rad for a last 1e-6 of cost; μ = 1e-3
    keeps them within ~0.1 rad of x̄ (tests/test_lm_prior.py). The arithmetic is
    fsdf_set_lm_prior's, operation for operation (the same bits as
    fsdf_descend_lm with that prior): e = x − x̄; r = 0.0, r += μ_i (e_i e_i) in
    index order; f + r; g_i + (2 μ_i) e_i; H_ii + 2 μ_i. Quaternion coordinates
    are penalised raw: a weight there also fixes the quaternion's scale.
    weight None: the objective itself, untouched."""
    if weight is None:
        return value_gradient_hessian
    x_ref = np.array(x_ref, np.float64, copy=True).reshape(-1)
    mu = np.broadcast_to(np.asarray(weight, np.float64), x_ref.shape).copy()
    if not (np.all(np.isfinite(mu)) and np.all(mu >= 0.0)):
        raise ValueError("state_prior: weights must be finite and >= 0")
    two_mu = 2.0 * mu

    def wrapped(x):
        f, g, H = value_gradient_hessian(x)
        e = np.asarray(x, np.float64).reshape(-1) - x_ref
        r = 0.0
        for m, v in zip(mu, e):  # (summed in index order: the native loop's bits)
            r += float(m) * (float(v) * float(v))
        H = np.array(H, np.float64, copy=True)
        i = np.arange(x_ref.size)
        H[i, i] = H[i, i] + two_mu
        return float(f) + r, np.asarray(g, np.float64) + two_mu * e, H

    return wrapped


@dataclass
class LevenbergMarquardt:
    """Damped Gauss-Newton on the sum-of-squares cost (rigid scenes): the
    second-order solver for frames where NaiveSolver's 30 gradient steps are
    too slow, as the reference's notebooks swap in Ipopt
    (examples/squishable.ipynb). `optimize` takes a function x -> (f, g, H)
    with H the Gauss-Newton Hessian 2 JᵀJ (Mechanism.gauss_newton_matrix from
    the per-surface second moments of the residual) and loops over
    _lib.lm_step (fsdf_lm_step): a trial step that does not lower f (a NaN one
    included) is rejected and the damping raised tenfold, up to 1e12; an
    accepted one lowers it tenfold, down to 1e-12. It stops when |g| is below
    the tolerance or after iteration_limit evaluations; `iterations` counts
    evaluations, as NaiveSolver's. On the CPU oracle (IRB140, 6,000 noise-free
    surface points, start off by σ = 0.2 rad) it is at the cloud's floor
    f(q_true) = 2.83e-4 after 4 evaluations, where NaiveSolver(rate 0.1,
    max_step 0.5) is at 6.12e-4 after 30 (tests/test_gauss_newton.py).
    estimate_state, Tracker and track take it for native rigid scenes: the
    second moments are reduced on the device (fsdf_value_gradient_hessian), and
    without a callback the whole loop runs natively (fsdf_descend_lm, the same
    bits). Scenes with RBF skins or deformations have no Gauss-Newton matrix
    here: NotImplementedError.
    prior_weight (a scalar or one value per coordinate; None: no prior): in
    estimate_state / Tracker / track the objective gains state_prior's Σ μ_i
    (x_i − x̄_i)² about the frame's warm start x̄ — through the context on the
    native path (fsdf_set_lm_prior), through state_prior with a callback;
    `optimize` itself takes the objective as given (wrap it in state_prior).
    device_loop (False, True or "require"): the native path's loop
    (fsdf_set_lm_solver): False the host loop, True the device-resident loop
    where the scene fits, "require" an error otherwise; the same bits.
    skins (False): True admits native scenes with RBF skins and deformations in
    estimate_state / Tracker / track — the cost's skin_hessian is turned on
    (fsdf_set_lm_skins: the skins' second moments reduced on the device, H over
    the whole state [q; δ]; the host loop). The default refuses them as before.
    With a robust point loss (estimate_state / Tracker / track `loss=`,
    flash.robust) f is Σρ(d*)/N and H the IRLS Gauss-Newton Hessian; the loop
    is the host loop whatever device_loop says ("require" is refused)."""
    num_vars: int
    damping: float = 1e-3
    max_step: float = 0.5
    iteration_limit: int = 30
    gradient_convergence_tolerance: float = 1e-6
    prior_weight: float | np.ndarray | None = None
    device_loop: bool | str = False
    skins: bool = False
    iterations: int = field(default=0, init=False)  # evaluations of the last optimize
    final_damping: float = field(default=0.0, init=False)

    def optimize(self, value_gradient_hessian, x0):
        from ._lib import lm_step
        x = np.array(x0, np.float64, copy=True)
        lam = float(self.damping)
        self.iterations = 0
        self.final_damping = lam
        f = None
        if self.iteration_limit > 0:
            f, g, H = value_gradient_hessian(x)
            self.iterations = 1
        while self.iterations < self.iteration_limit:
            nrm2 = 0.0
            for v in g:  # (summed in index order: the same bits wherever the loop is restated)
                nrm2 += float(v) * float(v)
            if np.sqrt(nrm2) < self.gradient_convergence_tolerance:
                break
            st, step = lm_step(H, g, lam, self.max_step)
            if st != 0:  # degenerate: more damping
                lam *= 10.0
                if lam > 1e12:
                    break
                continue
            xt = x + step
            ft, gt, Ht = value_gradient_hessian(xt)
            self.iterations += 1
            if ft < f:
                x, f, g, H = xt, ft, gt, Ht
                lam = max(lam / 10.0, 1e-12)
            else:
                lam *= 10.0
                if lam > 1e12:
                    break
        self.final_damping = lam
        return x, f


def _default_solver(manipulator):
    # src/tracking.jl:10-13
    return NaiveSolver(num_states(manipulator), rate=0.1, max_step=0.5, iteration_limit=30)


def _frame_weights(weights, points):
    """weights as estimate_state / Tracker / track take them: None, one array
    per call, or a callable points -> weights applied to the frame's cloud
    (points may itself be a callable -> points: a DepthFrame's host cloud is
    formed only when a weights callable asks for it)."""
    if weights is None:
        return None
    if callable(weights):
        weights = weights(points() if callable(points) else points)
    return np.asarray(weights, np.float64).reshape(-1)


def _loops_kw(robust_loops):
    # (handed to the functor only when asked for: a functor without the switch is built as before)
    return {"robust_loops": True} if robust_loops else {}


def _optimize(cost: CostFunctor, n_points: int, x_estimated, callback, solver, loss=None, weights=None,
              robust_skins: bool = False):
    """wrapped_cost (src/tracking.jl:16-21) over a CostFunctor, then optimize!.
    Without a callback, a NaiveSolver runs natively (fsdf_descend: the same
    arithmetic, no Python round trip per iteration), and so does a
    LevenbergMarquardt on a native rigid scene (fsdf_descend_lm, with the
    solver's prior_weight and device_loop); with a callback its Python loop
    runs over the objective wrapped in state_prior. A native scene with RBF
    skins or deformations is admitted only by LevenbergMarquardt(skins=True),
    which turns the cost's skin_hessian on.
    loss (flash.robust.Huber / Tukey; None: the functor as it is): handed to
    the functor (CostFunctor.set_loss) before anything runs, so every path
    above — the native loops, the Python loops, the callback's cost — is over
    the robust objective Σρ(d*)/N. The device-resident loops serve a loss
    only in a functor with robust_loops on (CostFunctor.set_robust_loops);
    otherwise device_loop=True runs the host loop and "require" is refused.
    weights (one confidence weight per point of the functor's cloud; None: the
    functor as it is): handed to the functor (CostFunctor.set_point_weights)
    before anything runs, under the loss's rules. n_points stays the divisor:
    pass weights of mean 1 for c / Σa.
    robust_skins (False: the functor as it is): turned on in the functor
    (CostFunctor.set_robust_skins) before the loss and the weights are handed
    over, so a native scene with RBF skins or deformations accepts them; a
    LevenbergMarquardt on such a scene needs skins=True as well."""
    n = max(n_points, 1)
    if robust_skins:
        cost.set_robust_skins(True)
    if loss is not None:
        cost.set_loss(loss)
    if weights is not None:
        cost.set_point_weights(weights)
    if callback is None and type(solver) is NaiveSolver and cost._native:
        x0 = np.asarray(x_estimated, np.float64)
        div = solver.precondition_divisors
        if div is not None:  # NaiveSolver broadcasts the divisors; fsdf_descend takes one per entry
            div = np.broadcast_to(np.asarray(div, np.float64), x0.shape).copy()
        x, _, its = cost.descend(x0, solver.iteration_limit, solver.rate, solver.max_step,
                                 solver.gradient_convergence_tolerance, div, n)
        solver.iterations = its
        return x
    if isinstance(solver, LevenbergMarquardt):
        # its objective returns (f, g, H): native rigid scenes have the Hessian
        # (the second moments of the residual, reduced on the device)
        skins = bool(getattr(solver, "skins", False)) and cost._native and hasattr(cost, "set_skin_hessian")
        if not (cost._native and (getattr(cost, "rigid", True) or skins) and hasattr(cost, "value_gradient_hessian")):
            raise NotImplementedError("estimate_state: LevenbergMarquardt needs an objective with a Gauss-Newton "
                                      "Hessian: a native rigid scene (no RBF skin, no deformation); or call its "
                                      "optimize() with one")
        if skins and not getattr(cost, "rigid", True) and not cost.skin_hessian:
            cost.set_skin_hessian(True)
        x0 = np.asarray(x_estimated, np.float64)
        if callback is None and type(solver) is LevenbergMarquardt and hasattr(cost, "descend_lm"):
            x, _, its, lam = cost.descend_lm(x0, solver.iteration_limit, solver.damping, solver.max_step,
                                             solver.gradient_convergence_tolerance, n,
                                             prior_weight=solver.prior_weight, device_loop=solver.device_loop)
            solver.iterations, solver.final_damping = its, lam
            return x

        def wrapped_h(x):
            c, g, H = cost.value_gradient_hessian(x)
            if callback is not None:
                callback(x, c)
            return c / n, g / n, H / n

        x, _ = solver.optimize(state_prior(wrapped_h, x0, solver.prior_weight), x0)
        return x

    def wrapped(x):
        c, g = cost.value_and_gradient(x)
        if callback is not None:
            callback(x, c)
        return c / n, g / n

    x, _ = solver.optimize(wrapped, np.asarray(x_estimated, np.float64))
    return x


def estimate_state(manipulator: Manipulator, sensed_points, x_estimated, callback=None, solver=None,
                   device: int = 0, precision: int = 64, loss=None, weights=None, robust_skins: bool = False,
                   voxel=None, robust_loops: bool = False):
    """Tracking.estimate_state (src/tracking.jl:8-27). Returns the solution x.

    The default callback accepts (x, c): the reference's default `x -> ()` is
    called with two arguments (src/tracking.jl:9 vs :19) and would throw.
    loss: a robust point loss (flash.robust.Huber / Tukey) in place of the
    squared distance — native rigid scenes; the callback then sees Σρ(d*).
    weights: one confidence weight >= 0 per sensed point (an array, or a
    callable points -> weights, e.g. depthsensors.depth_noise_weights bound to
    a sensor pose): the objective is Σ a ρ(d*) / N — native rigid scenes; set
    after the cloud is resident.
    robust_skins: loss, weights and a frame's free space also serve native
    scenes with RBF skins and deformations (fsdf_set_robust_skins).
    robust_loops: a loss, weights, a frame's free space and a grid's counts may
    run on the device-resident solver loops (fsdf_set_robust_loops; native rigid
    scenes, the same bits as the host loop). Where the loop runs is still the
    solver's say (LevenbergMarquardt(device_loop=…), Context.set_solver); off,
    such an objective takes the host loop and device_loop="require" is refused.
    sensed_points may be a depthsensors.DepthFrame (the depth image, the
    sensor and its pose): the device forms the cloud (fsdf_set_depth_*), N is
    the number of valid pixels, and the host forms the points only for a
    weights callable. A frame with free_space set (depthsensors.FreeSpace)
    needs no further argument: its samples follow the observed points, the
    objective penalises a sample only where the model covers it, and N in c / N
    is the resident point count, samples included (weights: one per resident
    point, samples included — CostFunctor.depth_pixels names every point's
    pixel).
    voxel (a depthdata.VoxelGrid; None: none): the cloud — of a DepthFrame its
    observed points — is thinned on the device to one centroid per occupied
    cell (include/flashsdf.h "voxel grid"); under weights "count" the cells'
    populations are point weights (native rigid scenes, others with
    robust_skins), under "unit" every centroid counts 1. A weights callable
    receives the resident points in caller order, centroids then samples, and
    under "count" its result is multiplied by the counts. N in c / N is then
    Σ count plus the sample count — the input cloud's size, not the number of
    centroids —, so a rate and tolerance tuned on full clouds keep their
    meaning; under "unit" it is the resident count."""
    solver = solver or _default_solver(manipulator)
    if isinstance(sensed_points, DepthFrame) or voxel is not None:
        if not isinstance(sensed_points, DepthFrame):
            sensed_points = np.asarray(sensed_points, np.float64).reshape(-1, 3)
        kw = {} if voxel is None else {"voxel": voxel}
        kw.update(_loops_kw(robust_loops))
        cost = CostFunctor(manipulator, sensed_points, device=device, precision=precision,
                           robust_skins=robust_skins, **kw)
        pts = lambda: cost.sensed_points  # noqa: E731 (formed when asked for)
    else:
        pts = np.asarray(sensed_points, np.float64).reshape(-1, 3)
        cost = CostFunctor(manipulator, pts, device=device, precision=precision, robust_skins=robust_skins,
                           **_loops_kw(robust_loops))
    return _optimize(cost, getattr(cost, "n_divisor", cost.n_points), x_estimated, callback, solver, loss=loss,
                     weights=_frame_weights(weights, pts), robust_skins=robust_skins)


def candidates_around(manipulator: Manipulator, x, sigma, count: int, seed=0) -> np.ndarray:
    """`count` candidate states around x for multi_start: x itself first, then
    count − 1 Gaussian perturbations x + σ ∘ z, z ~ N(0, I) drawn row by row
    from numpy.random.default_rng(seed) — the same rows for the same seed.
    sigma is a scalar or one value per coordinate of the state (>= 0, finite);
    every quaternion block of every row, x's included, is renormalised
    (Mechanism.normalize). Returns [count, n_states]."""
    n = num_states(manipulator)
    x = np.array(x, np.float64, copy=True).reshape(-1)
    if x.size != n:
        raise ValueError(f"candidates_around: x must have {n} entries, got {x.size}")
    count = int(count)
    if count < 1:
        raise ValueError(f"candidates_around: count must be >= 1, got {count}")
    sig = np.asarray(sigma, np.float64)
    if sig.ndim > 1 or (sig.ndim == 1 and sig.size != n):
        raise ValueError(f"candidates_around: sigma must be a scalar or have {n} entries")
    if not (np.all(np.isfinite(sig)) and np.all(sig >= 0.0)):
        raise ValueError("candidates_around: sigma must be finite and >= 0")
    rng = np.random.default_rng(seed)
    X = np.empty((count, n))
    X[0] = x
    if count > 1:
        X[1:] = x + np.broadcast_to(sig, (n,)) * rng.standard_normal((count - 1, n))
    nq = manipulator.mechanism.num_positions
    for row in X:
        row[:nq] = manipulator.mechanism.normalize(row[:nq])
    return X


def select_candidates(scores, keep: int) -> np.ndarray:
    """multi_start's selection rule: the indices of the `keep` lowest scores,
    best first. A NaN score ranks after every number (NaN last), equal scores
    rank by lower index; keep above the number of scores keeps them all."""
    s = np.asarray(scores, np.float64).reshape(-1)
    keep = int(keep)
    if keep < 1:
        raise ValueError(f"multi_start: keep must be >= 1, got {keep}")
    order = sorted(range(s.size), key=lambda i: (bool(np.isnan(s[i])), 0.0 if np.isnan(s[i]) else float(s[i]), i))
    return np.array(order[:keep], np.int64)


def _refine_batched(cost, n_points: int, X, solver):
    """The kept candidates X [keep, n_states] refined by one lockstep loop
    (CostFunctor.descend_batch / descend_lm_batch, by the solver's type) with
    _optimize's arguments; the refined objectives come from one score call.
    Returns (refined states, their objectives, the final dampings or None). The
    lockstep loops are host loops: a LevenbergMarquardt's device_loop does not
    apply (None, False and True are ignored; "require" is refused by
    _check_batched)."""
    n = max(n_points, 1)
    lam = None
    if type(solver) is NaiveSolver:
        div = solver.precondition_divisors
        if div is not None:  # NaiveSolver broadcasts the divisors; fsdf_descend_batch takes one per entry
            div = np.broadcast_to(np.asarray(div, np.float64), (X.shape[1],)).copy()
        R, _, its = cost.descend_batch(X, solver.iteration_limit, solver.rate, solver.max_step,
                                       solver.gradient_convergence_tolerance, div, n)
    else:
        R, _, its, lam = cost.descend_lm_batch(X, solver.iteration_limit, solver.damping, solver.max_step,
                                             solver.gradient_convergence_tolerance, n,
                                             prior_weight=solver.prior_weight)
    solver.iterations = int(np.max(its)) if len(its) else 0
    R = np.asarray(R, np.float64)
    return [R[i] for i in range(R.shape[0])], np.asarray(cost.score(R), np.float64).reshape(-1), lam


def _check_batched(cost, solver, callback):
    """multi_start(batched=True)'s conditions: the lockstep loops are the two
    native solver loops without a per-evaluation callback (cost None: the scene
    is checked later, once the functor exists)."""
    if callback is not None:
        raise ValueError("multi_start: batched=True takes no callback (the candidates advance in lockstep)")
    if type(solver) is not NaiveSolver and type(solver) is not LevenbergMarquardt:
        raise ValueError(f"multi_start: batched=True refines with NaiveSolver or LevenbergMarquardt, not "
                         f"{type(solver).__name__}")
    if getattr(solver, "device_loop", None) == "require":
        raise ValueError('multi_start: batched=True runs host loops around a batched device evaluation; a '
                         'LevenbergMarquardt(device_loop="require") cannot be honoured')
    if cost is not None and not (getattr(cost, "_native", False) and getattr(cost, "rigid", True)):
        raise ValueError("multi_start: batched=True needs a native rigid scene (no RBF skin, no deformation)")


def _multi_start_on(cost, n_points: int, candidates, keep, solver, callback, batched: bool = False):
    """multi_start over a functor whose cloud is resident and whose loss and
    weights are set: score, select, refine each kept candidate with _optimize
    (batched: all of them by one lockstep loop, _refine_batched), return the
    refined state of least final objective (ties: the better-scored candidate;
    a NaN objective last)."""
    if batched:
        _check_batched(cost, solver, callback)
    X = np.ascontiguousarray(candidates, np.float64)
    if X.ndim != 2 or X.shape[0] < 1:
        raise ValueError(f"multi_start: candidates must be [B >= 1, n_states], got shape {X.shape}")
    scores = np.asarray(cost.score(X), np.float64).reshape(-1)
    if scores.size != X.shape[0]:
        raise ValueError(f"multi_start: {scores.size} scores for {X.shape[0]} candidates")
    kept = select_candidates(scores, keep)
    refined, refined_costs, dampings = [], [], None
    if batched:
        refined, refined_costs, dampings = _refine_batched(cost, n_points, np.ascontiguousarray(X[kept]), solver)
    else:
        for b in kept:
            x = _optimize(cost, n_points, X[b], callback, solver)
            refined.append(np.asarray(x, np.float64))
            refined_costs.append(float(cost(x)))
    refined_costs = np.array(refined_costs, np.float64)
    j = int(select_candidates(refined_costs, 1)[0])
    if dampings is not None:  # (batched LevenbergMarquardt: the chosen candidate's, as one optimize leaves it)
        solver.final_damping = float(dampings[j])
    info = {"scores": scores, "kept": kept, "refined_costs": refined_costs, "chosen": int(kept[j]),
            "refined": np.array(refined)}
    return refined[j], info


def multi_start(manipulator: Manipulator, sensed_points, candidates, keep: int = 1, solver=None, loss=None,
                weights=None, voxel=None, device: int = 0, precision: int = 64, callback=None,
                robust_loops: bool = False, batched: bool = False):
    """A start in the right basin, found rather than given: score every
    candidate state against the cloud in one batch of launches
    (CostFunctor.score, fsdf_score_states), keep the `keep` lowest, refine each
    with estimate_state's own path (_optimize on the same CostFunctor: one
    upload for everything) and return (x, info): the refined state of least
    final objective and
      info["scores"]        [B] the candidates' objectives (Σ, not Σ/N)
      info["kept"]          indices of the candidates refined, best score first
      info["refined_costs"] [keep] the objective at each refined state
      info["chosen"]        the index of the candidate whose refinement won
      info["refined"]       [keep, n_states] the refined states
    Selection rule (select_candidates): NaN ranks last, equal values by lower
    index — for the scores and for the refined costs (in `kept` order) alike.
    sensed_points, loss, weights, voxel, device, precision, callback and solver
    and robust_loops are estimate_state's (a DepthFrame and a VoxelGrid included); candidates is
    [B, n_states] (candidates_around draws them). Native rigid scenes.
    batched (False: the path above, untouched): the kept candidates are refined
    together by one lockstep loop (CostFunctor.descend_batch for a NaiveSolver,
    descend_lm_batch for a LevenbergMarquardt: one batched evaluation and one
    synchronisation per iteration for all of them) and their refined objectives
    come from one score call; info keeps its keys and the selection rule is the
    same. A callback, any other solver, a LevenbergMarquardt with
    device_loop="require" (the lockstep loops are host loops; any other
    device_loop is ignored) or a non-native scene raises ValueError. Afterwards
    solver.iterations is the largest evaluation count among the kept candidates
    and a LevenbergMarquardt's final_damping the chosen candidate's.
    On least squares the refined objectives differ from the default path's in
    their last bits (the batched evaluation reduces in the robust path's order)."""
    solver = solver or _default_solver(manipulator)
    if batched:  # (before anything is uploaded; the scene is checked once the functor exists)
        _check_batched(None, solver, callback)
    X = np.ascontiguousarray(candidates, np.float64)
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] != num_states(manipulator):
        raise ValueError(f"multi_start: candidates must be [B >= 1, {num_states(manipulator)}], got shape {X.shape}")
    if int(keep) < 1:
        raise ValueError(f"multi_start: keep must be >= 1, got {keep}")
    if isinstance(sensed_points, DepthFrame) or voxel is not None:
        if not isinstance(sensed_points, DepthFrame):
            sensed_points = np.asarray(sensed_points, np.float64).reshape(-1, 3)
        kw = {} if voxel is None else {"voxel": voxel}
        kw.update(_loops_kw(robust_loops))
        cost = CostFunctor(manipulator, sensed_points, device=device, precision=precision, **kw)
        pts = lambda: cost.sensed_points  # noqa: E731 (formed when asked for)
    else:
        pts = np.asarray(sensed_points, np.float64).reshape(-1, 3)
        cost = CostFunctor(manipulator, pts, device=device, precision=precision, **_loops_kw(robust_loops))
    # (the objective the candidates are scored under is the one they are refined under)
    if loss is not None:
        cost.set_loss(loss)
    w = _frame_weights(weights, pts)
    if w is not None:
        cost.set_point_weights(w)
    return _multi_start_on(cost, getattr(cost, "n_divisor", cost.n_points), X, keep, solver, callback, batched)


def notebook_frame_solver(manipulator):
    """gradient_descent!'s solver (examples/irb_and_squishable.ipynb cell 11)."""
    return NaiveSolver(num_states(manipulator), rate=0.5, max_step=0.1, iteration_limit=1)


class Tracker:
    """The frame loop with everything resident: one CostFunctor (device model,
    context, ManipulatorState) for the whole sequence; per frame the cloud is
    swapped (one upload + device sort) and estimate_state runs warm-started
    from the previous frame's solution. Timings per frame and per solver
    iteration are recorded (host FK + pass + chain rule, end to end)."""

    def __init__(self, manipulator: Manipulator, state: ManipulatorState | None = None, solver=None,
                 device: int = 0, precision: int = 64, loss=None, weights=None, robust_skins: bool = False,
                 voxel=None, robust_loops: bool = False):
        self.manipulator = manipulator
        self.state = state if state is not None else ManipulatorState(manipulator)
        self.solver = solver or notebook_frame_solver(manipulator)
        self.cost = CostFunctor(manipulator, np.zeros((0, 3)), device=device, precision=precision,
                                robust_skins=robust_skins, **_loops_kw(robust_loops))
        # a robust objective may run on the device-resident loops (step and relocalize alike: the
        # functor carries the switch)
        self.robust_loops = bool(robust_loops)
        self.robust_skins = bool(robust_skins)  # loss / weights / free space also on skins and deformations
        self.loss = loss  # a robust point loss for every frame (flash.robust; None: least squares)
        # per-point confidence weights: a callable points -> weights applied to every frame (an
        # array fits one frame only: give it to step); None: every point counts 1
        self.weights = weights
        self.voxel = voxel  # a depthdata.VoxelGrid every frame is thinned through (None: none)
        self.frame_ms: list[float] = []
        self.set_points_ms: list[float] = []
        self.iterations: list[int] = []

    def step(self, sensed_points, callback=None, next_points=None, weights=None, voxel="tracker") -> np.ndarray:
        """gradient_descent!(state, model, sensed_points): one frame.
        next_points (optional): the next frame's cloud, whose upload then runs
        under this frame's solver iterations (CostFunctor.prefetch_sensed_points).
        weights (optional): this frame's confidence weights, an array or a
        callable points -> weights; None: the Tracker's own. They are set after
        the frame's cloud is resident, prefetched or not.
        sensed_points may be a depthsensors.DepthFrame: its image is made
        resident by the device ingest (never prefetched), and the host forms
        its points only for a weights callable. With the frame's free_space set
        the cloud holds its free-space samples after the observed points; N in
        c / N is the resident point count, samples included.
        voxel (optional): this frame's depthdata.VoxelGrid, or None for none;
        by default the Tracker's own. A frame thinned through a grid is as
        estimate_state's `voxel=`; with a grid the next cloud is not prefetched
        (next_points is ignored)."""
        grid = self.voxel if isinstance(voxel, str) and voxel == "tracker" else voxel
        if isinstance(sensed_points, DepthFrame) or grid is not None:
            pts = lambda: self.cost.sensed_points  # noqa: E731 (formed when asked for)
        else:
            pts = np.asarray(sensed_points, np.float64).reshape(-1, 3)
        t0 = time.perf_counter()
        # (the object itself: a prefetched frame is matched by identity)
        if grid is None and getattr(self.cost, "voxel", None) is None:
            self.cost.set_sensed_points(sensed_points)
        else:
            self.cost.set_sensed_points(sensed_points, voxel=grid)
        if next_points is not None and not isinstance(next_points, DepthFrame) and grid is None:
            self.cost.prefetch_sensed_points(next_points)
        t1 = time.perf_counter()
        w = _frame_weights(self.weights if weights is None else weights, pts)
        x = _optimize(self.cost, getattr(self.cost, "n_divisor", self.cost.n_points), flatten(self.state), callback, self.solver, loss=self.loss,
                      weights=w, robust_skins=self.robust_skins)
        unflatten(self.state, x)
        t2 = time.perf_counter()
        self.set_points_ms.append((t1 - t0) * 1e3)
        self.frame_ms.append((t2 - t0) * 1e3)
        self.iterations.append(getattr(self.solver, "iterations", 0))
        return x

    def relocalize(self, sensed_points, candidates=None, sigma=0.3, count: int = 64, keep: int = 2, seed=0,
                   solver=None, callback=None, weights=None, voxel="tracker", batched: bool = False):
        """Find the state again (a first frame, or after an occlusion or a
        dropped frame): make the frame's cloud resident as step does, run
        multi_start's search on the Tracker's own CostFunctor around its current
        state — candidates, or candidates_around(state, sigma, count, seed) —
        and adopt the result. Returns (x, info) as multi_start. solver: the
        refinement's solver (default: estimate_state's, 30 iterations; the
        Tracker's own frame solver takes single steps). batched: multi_start's
        (the kept candidates refined by one lockstep loop). step itself never
        calls this: recovery is the caller's decision."""
        if batched:  # (before the cloud is swapped)
            _check_batched(self.cost, solver or _default_solver(self.manipulator), callback)
        grid = self.voxel if isinstance(voxel, str) and voxel == "tracker" else voxel
        if isinstance(sensed_points, DepthFrame) or grid is not None:
            pts = lambda: self.cost.sensed_points  # noqa: E731 (formed when asked for)
        else:
            pts = np.asarray(sensed_points, np.float64).reshape(-1, 3)
        if grid is None and getattr(self.cost, "voxel", None) is None:
            self.cost.set_sensed_points(sensed_points)
        else:
            self.cost.set_sensed_points(sensed_points, voxel=grid)
        if candidates is None:
            candidates = candidates_around(self.manipulator, flatten(self.state), sigma, count, seed)
        if self.robust_skins:
            self.cost.set_robust_skins(True)
        if self.loss is not None:
            self.cost.set_loss(self.loss)
        w = _frame_weights(self.weights if weights is None else weights, pts)
        if w is not None:
            self.cost.set_point_weights(w)
        x, info = _multi_start_on(self.cost, getattr(self.cost, "n_divisor", self.cost.n_points), candidates, keep,
                                  solver or _default_solver(self.manipulator), callback, batched)
        unflatten(self.state, x)
        return x, info

    def iteration_ms(self) -> float:
        """Mean end-to-end milliseconds per solver iteration (excluding the cloud swap)."""
        its = sum(self.iterations)
        return (sum(self.frame_ms) - sum(self.set_points_ms)) / its if its else float("nan")


def track(manipulator: Manipulator, frames, state: ManipulatorState | None = None, solver=None, callback=None,
          device: int = 0, precision: int = 64, loss=None, weights=None, robust_skins: bool = False, voxel=None,
          robust_loops: bool = False):
    """for event in log: gradient_descent!(state, model, sensed_points)
    (examples/irb_and_squishable.ipynb cells 11-12). `frames` yields sensed
    clouds ([n,3]) or depthsensors.DepthFrames (made resident by the device
    ingest, not prefetched; a frame's free_space adds its free-space samples, and
    N in c / N is then the resident point count, samples included); returns (the
    per-frame solutions [F, n_states], the Tracker).
    loss: a robust point loss for every frame (flash.robust).
    weights: a callable points -> weights applied to every frame (or one array,
    where every frame has as many points).
    robust_skins, robust_loops: as estimate_state's.
    voxel: a depthdata.VoxelGrid every frame is thinned through (as
    estimate_state's). With it set the next cloud is NOT prefetched — the grid
    stage has no prefetched form —, so a frame's upload does not overlap the
    previous frame's iterations."""
    tr = Tracker(manipulator, state, solver, device, precision, loss=loss, weights=weights,
                 robust_skins=robust_skins, voxel=voxel, robust_loops=robust_loops)
    xs = []
    it = iter(frames)
    cur = next(it, None)
    while cur is not None:
        nxt = next(it, None)  # (its upload overlaps this frame's iterations)
        xs.append(tr.step(cur, callback, next_points=nxt))
        cur = nxt
    return np.array(xs), tr
