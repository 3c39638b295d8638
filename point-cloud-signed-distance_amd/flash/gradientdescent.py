"""module Flash.GradientDescent (src/gradientdescent.jl).

  default_deformation_cost_weight = 10          :7
  flatten(state) / unflatten!(state, x)         :9-17
  normalize!(mechanism_state)                   :19-26
  cost(state, sensed_points, weight)            :28-39
  CostFunctor(manipulator, sensed_points)(x)    :41-57
In the reference the gradient of CostFunctor comes from ForwardDiff (Dual{9}
chunk passes, ⌈n/9⌉ full point passes per gradient, examples/irb_and_squishable
.ipynb:482). Here ONE GPU residual pass returns the cost and the per-hull
wrenches, and `value_and_gradient` chains them analytically to ∂c/∂x.
"""
from __future__ import annotations

import numpy as np

from .core import ConvexGeometry, InterpolatingGeometry, Manipulator, ManipulatorState, num_states, prepare_pass
from .depthsensors import DepthFrame

default_deformation_cost_weight = 10


def flatten(state: ManipulatorState) -> np.ndarray:
    """vcat(q, deformation_data) (src/gradientdescent.jl:9-11)."""
    return np.concatenate([state.q, state.deformation_data])


def unflatten(state: ManipulatorState, x) -> None:
    """unflatten!(state, x) (src/gradientdescent.jl:13-17)."""
    x = np.asarray(x, np.float64)
    nq = state.manipulator.mechanism.num_positions
    state.q[:] = x[:nq]
    state.deformation_data[:] = x[nq:]


def normalize(state: ManipulatorState) -> None:
    """normalize!(state.mechanism_state) in place (src/gradientdescent.jl:19-26)."""
    state.q[:] = state.manipulator.mechanism.normalize(state.q)


def _regularizer(state: ManipulatorState, weight) -> float:
    return float(weight) * float(np.dot(state.deformation_data, state.deformation_data))


def cost(state: ManipulatorState, sensed_points, deformation_cost_weight=default_deformation_cost_weight,
         device: int = 0, precision: int = 64) -> float:
    """Σ_p skin(p)^2 + w·Σ‖δ‖² (src/gradientdescent.jl:28-39); normalizes q in place first."""
    normalize(state)
    m = state.manipulator
    ctx = m.engine(device, precision)
    pts = np.asarray(sensed_points, np.float64).reshape(-1, 3)
    d = np.zeros(0)
    if len(pts):
        poses, _ = prepare_pass(ctx, m, state.q, state.deformation_data)
        d, _, _ = ctx.skin(poses, pts)
    return float(np.dot(d, d)) + _regularizer(state, deformation_cost_weight)


def gradient_from_accum(manip: Manipulator, x: np.ndarray, accum: np.ndarray, solves, weight) -> np.ndarray:
    """∂c/∂x from one pass's accumulator: hull wrenches (slot = surface index)
    plus the RBF adjoint block, contracted with the joint motion subspaces;
    ∂c/∂δ from the RBF block plus the regularizer 2wδ."""
    mech = manip.mechanism
    nq = mech.num_positions
    S = len(manip.surfaces)
    sb = getattr(manip, "_surface_body", None)
    if sb is None or len(sb) != S:
        sb = np.array([s.body if isinstance(s, ConvexGeometry) else -1 for s in manip.surfaces], np.int32)
        manip._surface_body = sb
    gd = 2.0 * weight * np.asarray(x[nq:], np.float64)
    body_w = None
    if solves:
        from . import rbf
        w_rbf, g_rbf = rbf.chain(manip, mech.normalize(x[:nq]), solves, accum[1 + 6 * S:], manip.num_deformations())
        body_w = w_rbf
        gd = gd + g_rbf
    # the gradient is taken at the caller's (un-normalized) x: the chain rule
    # includes the normalization projection (src/gradientdescent.jl:30)
    gq = mech.config_gradient(np.asarray(x[:nq], np.float64), body_w, sb, np.asarray(accum[1:1 + 6 * S]))
    return np.concatenate([gq, gd])


def native_capable(manipulator: Manipulator) -> bool:
    """Scenes fsdf_value_and_gradient handles: convex hulls and RBF skins."""
    return all(isinstance(s, (ConvexGeometry, InterpolatingGeometry)) for s in manipulator.surfaces)


def register_native(manipulator: Manipulator, ctx, weight) -> None:
    """Declare the mechanism, surface bodies/frames, RBF centres and
    deformations to the context (fsdf_set_mechanism, fsdf_set_rbf_centres,
    fsdf_set_deformations) for its native iterations."""
    m = manipulator
    surf = m.surfaces
    hull = [isinstance(s, ConvexGeometry) for s in surf]
    eye, zero = np.eye(3), np.zeros(3)
    ctx.set_mechanism(m.mechanism, [s.body if h else -1 for s, h in zip(surf, hull)],
                      [s.frame.R if h else eye for s, h in zip(surf, hull)],
                      [s.frame.t if h else zero for s, h in zip(surf, hull)])
    row0 = 0  # deformation rows in surface order (flash/rbf.py solve)
    for k, s in enumerate(surf):
        nd = s.num_deformations()
        if isinstance(s, InterpolatingGeometry):
            rows = np.arange(row0, row0 + nd, dtype=np.int32) if nd else None
            ctx.set_rbf_centres(k, s.surface_points, s.skeleton_points, rows)
        row0 += nd
    ctx.set_deformations(m.num_deformations(), weight)
    ctx._mechanism_of = (m, weight)


class CostFunctor:
    """CostFunctor(manipulator, sensed_points) (src/gradientdescent.jl:41-57).

    The sensed cloud is uploaded once (the reference keeps it by reference for
    every evaluation); each call ships only the hull poses. sensed_points may
    be a depthsensors.DepthFrame: the depth image is uploaded and the device
    forms the cloud (Context.set_depth); `sensed_points` then forms the host
    copy (frame.points()) only when it is read, `n_points` is the cloud's size
    either way and `depth_pixels()` names each point's pixel. A frame with
    `free_space` set sends free-space samples after the observed points
    (fsdf_set_free_space): `n_surface` is the number of observed points,
    `n_points` counts the samples too, and the objective penalises a sample
    only where the model covers it (include/flashsdf.h "free space").
    voxel (a depthdata.VoxelGrid; None: none): the cloud — of a DepthFrame its
    observed points — is thinned on the device to one centroid per occupied
    cell before it becomes resident (fsdf_set_points_voxel / fsdf_set_voxel_grid;
    include/flashsdf.h "voxel grid"). `sensed_points` is then the resident
    cloud in caller order (centroids, then a frame's samples), `n_points` its
    size, and under weights "count" the cells' populations are the point
    weights (`voxel_weights`: the counts, then 1.0 per sample) and `n_divisor`
    — what the solvers divide the cost by — is their sum, the input cloud's
    size; under "unit" it is `n_points`."""

    # (the switch's default lives on the class: a functor assembled without __init__ — the stand-ins
    # of tests/test_robust_skins.py — has it off, and _assert_loss reads it plainly)
    robust_loops = False

    def __init__(self, manipulator: Manipulator, sensed_points, device: int = 0, precision: int = 64,
                 deformation_cost_weight=default_deformation_cost_weight, skin_hessian: bool = False, loss=None,
                 robust_skins: bool = False, voxel=None, robust_loops: bool = False):
        self.manipulator = manipulator
        self.voxel = voxel
        self.weight = deformation_cost_weight
        self.state = ManipulatorState(manipulator)
        self.ctx = manipulator.engine(device, precision)
        # a private context would be needed to keep two functors resident at once
        self._take(sensed_points)
        self._upload()
        self._resident = id(self)
        manipulator._resident_cloud = self._resident
        # the whole iteration (FK, RBF weight solve, pass, chain rule,
        # regularizer) in one native call (fsdf_value_and_gradient)
        self._native = native_capable(manipulator)
        # rigid: hulls only, nothing deformable — the scenes with a Gauss-Newton
        # Hessian (value_gradient_hessian, descend_lm)
        self.rigid = all(isinstance(s, ConvexGeometry) for s in manipulator.surfaces) and \
            manipulator.num_deformations() == 0
        if self._native and getattr(self.ctx, "_mechanism_of", None) != (manipulator, self.weight):
            self._register_native()
        # skin_hessian: value_gradient_hessian / descend_lm also serve RBF skins
        # and deformations (fsdf_set_lm_skins; the skins' second moments are
        # reduced on the device, csrc/skin_moments.hip)
        self.skin_hessian = False
        if skin_hessian:
            self.set_skin_hessian(True)
        # robust_skins: a loss, point weights and a free split also serve native
        # scenes with RBF skins and deformations (fsdf_set_robust_skins; the
        # skins' robust blocks are reduced on the device, csrc/robust_skin.hip)
        self.robust_skins = False
        if robust_skins:
            self.set_robust_skins(True)
        # robust_loops: a loss, point weights and a free split may run on the
        # device-resident solver loops of descend / descend_lm (fsdf_set_robust_loops;
        # rigid scenes — where the loop runs stays set_solver's / device_loop's say)
        self.robust_loops = False
        if robust_loops:
            self.set_robust_loops(True)
        # loss: a robust point loss (flash.robust.Huber / Tukey; None: least
        # squares) for __call__, value_and_gradient, value_gradient_hessian,
        # descend and descend_lm (fsdf_set_loss; native rigid scenes, others
        # with robust_skins)
        self.loss = None
        self.set_loss(loss)
        # point_weights: one confidence weight per sensed point (set_point_weights;
        # None: every point counts 1), dropped whenever the sensed points change
        self.point_weights = None

    @property
    def sensed_points(self):
        """The sensed cloud [n, 3] on the host; of a DepthFrame, formed on the
        first read (frame.points(): the resident cloud's bits and order)."""
        if self.voxel is not None:  # (the resident cloud: centroids, then a frame's samples)
            if self._voxel_points is None:
                from .depthdata import voxel_downsample
                self._voxel_points = voxel_downsample(self._points, self.voxel)[0] if self._frame is None \
                    else self._frame.voxel_points(self.voxel)[0]
            return self._voxel_points
        if self._points is None:
            self._points = self._frame.points()[0]
        return self._points

    @sensed_points.setter
    def sensed_points(self, points):
        self._frame, self._points, self._voxel_points = None, points, None

    def _take(self, sensed_points):
        # a DepthFrame as it is, anything else as the [n, 3] f64 array
        if isinstance(sensed_points, DepthFrame):
            self._frame, self._points, self._voxel_points = sensed_points, None, None
        else:
            self.sensed_points = np.ascontiguousarray(sensed_points, np.float64).reshape(-1, 3)

    def _upload(self):
        """Make this functor's cloud resident: set_points of the array, or — a
        DepthFrame — set_depth of its image, after set_sensor when the
        context's sensor is not the frame's already (by identity, like
        _mechanism_of)."""
        f = self._frame
        if f is None and self.voxel is None:
            self.ctx.set_points(self._points)
        else:
            if f is not None:
                have = getattr(self.ctx, "_sensor_of", None)
                if have is None or have[0] is not f.sensor or have[1] != f.kind:
                    self.ctx._sensor_of = None
                    self.ctx.set_sensor(f.sensor.rays, f.kind)
                    self.ctx._sensor_of = (f.sensor, f.kind)
                self.ctx.set_free_space(getattr(f, "free_space", None))  # (a context setting: this frame's)
            # the grid is a context setting too, and the engine is shared: set for this upload alone,
            # so that whoever next hands the context a depth image gets the frame it asked for
            self.ctx.set_voxel_grid(self.voxel)
            try:
                if f is None:
                    self.ctx.set_points_voxel(self._points)
                else:
                    self.ctx.set_depth(f.depth, f.tform, f.near, f.far, f.scale)
            finally:
                if self.voxel is not None:
                    self.ctx.set_voxel_grid(None)
        self.n_points = self.ctx.n
        # n_surface: the first n_surface sensed points are surface observations, the rest free-space
        # samples (a frame with free_space: the library set the split itself; a plain cloud: none
        # until set_free_split)
        split = self.ctx.get_free_split()
        self.n_surface = self.n_points if split is None else split
        # a voxel cloud: the counts (then 1.0 per sample) and the cost's divisor — under "count" the
        # input cloud's size (Σ count + samples), so a rate and tolerance tuned on full clouds keep
        # their meaning; else the resident count
        self.voxel_weights, self.n_divisor = None, self.n_points
        if self.voxel is not None:
            m, n_in, dropped = self.ctx.voxel_sizes()
            if self.voxel.weights == "count":
                self.voxel_weights = np.concatenate([self.ctx.get_voxels()[1].astype(np.float64),
                                                     np.ones(self.n_points - m)])
                self.n_divisor = (n_in - dropped) + (self.n_points - m)

    def depth_pixels(self):
        """Of a DepthFrame: pixel (row · cols + col) of every sensed point, in
        the points' order (fsdf_get_depth_pixels) — per-pixel confidences
        w_img.ravel()[cost.depth_pixels()] are point weights."""
        if self._frame is None:
            raise ValueError("depth_pixels: the sensed points did not come from a DepthFrame")
        self._ensure_resident()
        return self.ctx.depth_pixels()

    def set_point_weights(self, weights):
        """Per-point confidence weights a_i >= 0 of this functor's objective,
        one per sensed point in the order of `sensed_points` (None: none):
        Σ a ρ(d*) in place of Σ ρ(d*), its gradient and the Gauss-Newton Hessian
        (fsdf_set_point_weights; the robust reduction, also without a loss).
        Native rigid scenes, others with robust_skins. They belong to the sensed cloud:
        set_sensed_points drops them. per_point and the least-squares queries
        of the context are not affected."""
        if weights is not None:
            if not self._robust_capable():
                raise NotImplementedError(
                    "point weights: they serve native rigid scenes (no RBF skin, no deformation)")
            weights = np.array(weights, np.float64, copy=True).reshape(-1)
            if len(weights) != self.n_points:
                raise ValueError(f"point weights: {len(weights)} weights for {self.n_points} sensed points")
            if getattr(self, "voxel_weights", None) is not None:  # (a voxel cloud under "count": times the counts)
                weights = weights * self.voxel_weights
        self._ensure_resident()
        if weights is None and getattr(self, "voxel_weights", None) is not None:  # (back to the counts alone)
            self.ctx.set_point_weights(self.voxel_weights)
        else:
            self.ctx.set_point_weights(weights)  # (refused: the earlier weights stay, here too)
        self.point_weights = weights

    def set_free_split(self, n_surface):
        """Of a plain cloud whose tail the caller filled with free-space
        samples of their own: sensed points [n_surface, n) are positions known
        to be empty and count only where the model covers them (d* < 0) —
        Σ_surface ρ(d*) + Σ_free [d* < 0] ρ(d*), its gradient and Gauss-Newton
        Hessian (fsdf_set_free_split; the robust reduction, also without a
        loss). None or n clears it. Native rigid scenes, others with robust_skins. It belongs to
        the sensed cloud: set_sensed_points drops it (a DepthFrame with
        free_space sets its own)."""
        n = self.n_points if n_surface is None else int(n_surface)
        if n != self.n_points:
            if not self._robust_capable():
                raise NotImplementedError("free split: it serves native rigid scenes (no RBF skin, no deformation)")
            if not 0 <= n <= self.n_points:
                raise ValueError(f"free split: n_surface {n} of {self.n_points} sensed points")
        self._ensure_resident()
        self.ctx.set_free_split(n)
        self.n_surface = n

    def set_loss(self, loss):
        """The robust point loss of this functor's objective (flash.robust;
        None: least squares, the default): Σρ(d*) in place of Σd*², its
        gradient, and the IRLS Gauss-Newton Hessian (fsdf_set_loss; reduced on
        the device, csrc/robust.hip). Native rigid scenes, others with
        robust_skins (csrc/robust_skin.hip). per_point and
        the least-squares queries of the context are not affected."""
        if loss is not None and not self._robust_capable():
            raise NotImplementedError("loss: robust losses serve native rigid scenes (no RBF skin, no deformation)")
        self.loss = loss
        self._assert_loss()

    def _robust_capable(self):
        # a robust objective: native rigid scenes, and with robust_skins any native scene
        return self._native and (self.rigid or self.robust_skins)

    def set_robust_skins(self, enable: bool = True):
        """Let the robust objective (set_loss, set_point_weights,
        set_free_split, a DepthFrame's free_space) serve scenes with RBF skins
        and deformations (fsdf_set_robust_skins); native scenes only.
        value_gradient_hessian / descend_lm on such a scene need skin_hessian
        as well."""
        if enable and not self._native:
            raise NotImplementedError("robust_skins: scene is not native-capable")
        self.robust_skins = bool(enable)
        if self._native:
            self.ctx.set_robust_skins(self.robust_skins)

    def set_robust_loops(self, enable: bool = True):
        """Let the robust objective (set_loss, set_point_weights,
        set_free_split, a DepthFrame's free_space, a VoxelGrid's counts) run on
        the device-resident loops of descend and descend_lm
        (fsdf_set_robust_loops): rigid native scenes, bit-identical to the host
        loop. Off (the default), such an objective takes the host loop and
        device_loop="require" / set_solver("require") are refused. Where the
        loop runs is still LevenbergMarquardt(device_loop=…)'s and
        Context.set_solver's say; scenes with RBF skins or deformations keep
        the host loop."""
        if enable and not self._native:
            raise NotImplementedError("robust_loops: scene is not native-capable")
        self.robust_loops = bool(enable)
        if self._native:
            self.ctx.set_robust_loops(self.robust_loops)

    def _assert_loss(self):
        # (the engine is shared: another functor of it may have set its own)
        if self.ctx.loss != self.loss:
            self.ctx.set_loss(self.loss)
        if self._native and getattr(self.ctx, "robust_skins", False) != self.robust_skins:
            self.ctx.set_robust_skins(self.robust_skins)
        if self._native and getattr(self.ctx, "robust_loops", False) != self.robust_loops:
            self.ctx.set_robust_loops(self.robust_loops)

    def set_skin_hessian(self, enable: bool = True):
        """Turn the Gauss-Newton Hessian of non-rigid scenes on or off
        (fsdf_set_lm_skins); native scenes only."""
        if enable and not self._native:
            raise NotImplementedError("skin_hessian: scene is not native-capable")
        self.skin_hessian = bool(enable)
        if self._native:
            self.ctx.set_lm_skins(self.skin_hessian)

    def _register_native(self):
        register_native(self.manipulator, self.ctx, self.weight)

    def set_sensed_points(self, sensed_points, voxel="keep"):
        """Swap the resident cloud (a new frame): one upload + device sort; the
        functor, its state and the device model are kept. The array given to
        prefetch_sensed_points last is made resident from its device copy. A
        depthsensors.DepthFrame is made resident from its image (set_depth).
        voxel: a depthdata.VoxelGrid for this and later clouds, None for none
        ("keep": the functor's as it is). A voxel cloud is never made resident
        from a prefetched copy."""
        pre, src = getattr(self, "_prefetched", None), getattr(self, "_prefetched_src", None)
        self._prefetched = self._prefetched_src = None
        self.point_weights = None  # (another cloud: the library drops its copy with the old one)
        if not (isinstance(voxel, str) and voxel == "keep"):
            self.voxel = voxel
        if pre is not None and sensed_points is src and self.voxel is None:  # (the object prefetched: its device copy)
            self.sensed_points = pre
            self.ctx.set_points_prefetched()
            self.n_points = self.n_surface = self.n_divisor = self.ctx.n
            self.voxel_weights = None
        else:
            self._take(sensed_points)
            self._upload()
        self.manipulator._resident_cloud = self._resident

    def prefetch_sensed_points(self, sensed_points):
        """Start the NEXT frame's upload now (fsdf_prefetch_points: a copy on a
        stream of the context's own, running under the current frame's passes —
        fully when the array is page-locked); set_sensed_points(that array)
        then skips the host-to-device copy. The array must not change until then."""
        self._prefetched = np.ascontiguousarray(sensed_points, np.float64).reshape(-1, 3)
        self._prefetched_src = sensed_points
        self.ctx.prefetch_points(self._prefetched)

    def regroup(self):
        """Once per frame, after its first evaluation: regroup the resident
        cloud by each point's nearest surface in that pass (fsdf_regroup_points;
        hull-only scenes). Later evaluations give the same per-point results and
        sums to rounding, faster on large clouds."""
        self._ensure_resident()
        self.ctx.regroup_points()

    def _ensure_resident(self):
        if getattr(self.manipulator, "_resident_cloud", None) != self._resident:
            split = getattr(self, "n_surface", None) if self._frame is None else None
            self._upload()
            if split is not None and split != self.n_points:  # (a plain cloud's split left with the cloud)
                self.ctx.set_free_split(split)
                self.n_surface = split
            self.manipulator._resident_cloud = self._resident
            if getattr(self, "point_weights", None) is not None:  # (they left with the cloud)
                self.ctx.set_point_weights(self.point_weights)

    def _pass(self, x, per_point=False):
        unflatten(self.state, x)
        normalize(self.state)
        self._ensure_resident()
        poses, self._solves = prepare_pass(self.ctx, self.manipulator, self.state.q, self.state.deformation_data)
        c, accum, extras = self.ctx.eval(poses, per_point)
        return c + _regularizer(self.state, self.weight), accum, extras

    def __call__(self, x) -> float:
        if self.loss is not None or self.point_weights is not None or self.n_surface != self.n_points or \
                getattr(self, "voxel_weights", None) is not None:
            # (the robust / weighted / split objective: the native iteration's cost)
            return self.value_and_gradient(x)[0]
        return self._pass(x)[0]

    def value_and_gradient(self, x):
        """(c(x), ∂c/∂x) from one residual pass (with a loss: of the robust
        objective Σρ(d*))."""
        x = np.asarray(x, np.float64)
        if self._native:
            self._ensure_resident()
            if getattr(self.ctx, "_mechanism_of", None) != (self.manipulator, self.weight):
                self._register_native()  # another functor of this engine registered its own
            self._assert_loss()
            return self.ctx.value_and_gradient(x)
        c, accum, _ = self._pass(x)
        return c, gradient_from_accum(self.manipulator, x, accum, self._solves, self.weight)

    def score(self, X) -> np.ndarray:
        """The objective at many candidate states in one batch of launches
        (fsdf_score_states, csrc/score.hip): X is [B, n_states], or a list of
        ManipulatorState; returns the costs [B] — value_and_gradient's cost at
        each row (the functor's loss, weights and split; Σ, not Σ/N), to
        summation order, with no gradient. Native rigid scenes; the others are
        refused with the library's error. Read-only on the resident cloud: a
        later evaluation returns the bits it returns without the call."""
        if not self._native:
            raise NotImplementedError("score: scene is not native-capable")
        if isinstance(X, (list, tuple)) and len(X) and isinstance(X[0], ManipulatorState):
            X = [flatten(s) for s in X]
        X = np.ascontiguousarray(X, np.float64)
        if X.ndim == 1:
            X = X.reshape(1, -1) if X.size else X.reshape(0, num_states(self.manipulator))
        if X.ndim != 2 or X.shape[1] != num_states(self.manipulator):
            raise ValueError(f"score: X must be [B, {num_states(self.manipulator)}], got shape {X.shape}")
        self._ensure_resident()
        if getattr(self.ctx, "_mechanism_of", None) != (self.manipulator, self.weight):
            self._register_native()
        self._assert_loss()
        return self.ctx.score_states(X)

    def descend(self, x, iteration_limit, rate, max_step, tolerance=0.0, divisors=None, n_points=1.0):
        """The NaiveSolver loop over value_and_gradient in one native call
        (fsdf_descend); native-capable scenes only. Returns (x, f, iterations)."""
        if not self._native:
            raise NotImplementedError("descend: scene is not native-capable")
        self._ensure_resident()
        if getattr(self.ctx, "_mechanism_of", None) != (self.manipulator, self.weight):
            self._register_native()
        self._assert_loss()
        return self.ctx.descend(x, iteration_limit, rate, max_step, tolerance, divisors, n_points)

    def _native_rigid(self, who):
        if not (self._native and (self.rigid or self.skin_hessian)):
            raise NotImplementedError(f"{who}: rigid native scenes only (no RBF skin, no deformation)")
        self._ensure_resident()
        if getattr(self.ctx, "_mechanism_of", None) != (self.manipulator, self.weight):
            self._register_native()
        if getattr(self.ctx, "lm_skins", False) != self.skin_hessian:  # (another functor of this engine set its own)
            self.ctx.set_lm_skins(self.skin_hessian)
        self._assert_loss()

    def value_gradient_hessian(self, x):
        """(c(x), ∂c/∂x, the Gauss-Newton Hessian 2 JᵀJ) from one residual pass
        and the device reduction of its second moments
        (fsdf_value_gradient_hessian); rigid scenes, and with skin_hessian
        scenes with RBF skins and deformations (H over the whole state)."""
        self._native_rigid("value_gradient_hessian")
        return self.ctx.value_gradient_hessian(np.asarray(x, np.float64))

    def descend_lm(self, x, iteration_limit, damping, max_step, tolerance=0.0, n_points=1.0, prior_weight=None,
                   device_loop=None):
        """The LevenbergMarquardt loop over value_gradient_hessian in one native
        call (fsdf_descend_lm); rigid scenes, and with skin_hessian scenes with
        RBF skins and deformations (the host loop). Returns (x, f, evaluations, final
        damping). Both options hold for this call alone; the context is as it
        was on return. prior_weight (a scalar or one value per coordinate): the
        prior Σ μ_i (x_i − x_i at entry)² on the wrapped objective
        (fsdf_set_lm_prior; set after the mechanism is registered, cleared
        again). device_loop (False / True / "require"): the LM loop
        (fsdf_set_lm_solver); None: the context's own mode
        (Context.set_lm_solver)."""
        self._native_rigid("descend_lm")
        ctx = self.ctx
        mode = getattr(ctx, "lm_solver_mode", 0)
        try:
            if device_loop is not None:
                ctx.set_lm_solver(device_loop)
            if prior_weight is not None:
                ctx.set_lm_prior(prior_weight)
            return ctx.descend_lm(x, iteration_limit, damping, max_step, tolerance, n_points)
        finally:
            if prior_weight is not None:
                ctx.set_lm_prior(None)
            if device_loop is not None:
                ctx.set_lm_solver(mode)

    def _batch_states(self, X, who):
        """X as [B, n_states] for the batched calls, the functor ready for them
        (native rigid scenes: resident cloud, mechanism, loss)."""
        if not (self._native and self.rigid):
            raise NotImplementedError(f"{who}: rigid native scenes only (no RBF skin, no deformation)")
        if isinstance(X, (list, tuple)) and len(X) and isinstance(X[0], ManipulatorState):
            X = [flatten(s) for s in X]
        X = np.ascontiguousarray(X, np.float64)
        n = num_states(self.manipulator)
        if X.ndim == 1:
            X = X.reshape(1, -1) if X.size else X.reshape(0, n)
        if X.ndim != 2 or X.shape[1] != n:
            raise ValueError(f"{who}: X must be [B, {n}], got shape {X.shape}")
        self._ensure_resident()
        if getattr(self.ctx, "_mechanism_of", None) != (self.manipulator, self.weight):
            self._register_native()
        self._assert_loss()
        return X

    def batch_value_and_gradient(self, X):
        """(c [B], ∂c/∂x [B, n]) at every row of X in one batch of launches and
        one synchronisation (fsdf_batch_states, csrc/batch.hip): the robust
        path's value_and_gradient at each row — the functor's loss, weights and
        split; least squares as FSDF_LOSS_SQUARE — bit for bit on the same cloud
        layout. Native rigid scenes; read-only on the resident cloud."""
        X = self._batch_states(X, "batch_value_and_gradient")
        c, g, _ = self.ctx.batch_states(X, hessian=False)
        return c, g

    def batch_value_gradient_hessian(self, X):
        """(c [B], ∂c/∂x [B, n], the Gauss-Newton Hessians [B, n, n]) at every
        row of X, as batch_value_and_gradient; the same (c, g) bits."""
        X = self._batch_states(X, "batch_value_gradient_hessian")
        return self.ctx.batch_states(X, hessian=True)

    def descend_batch(self, X, iteration_limit, rate, max_step, tolerance=0.0, divisors=None, n_points=1.0):
        """descend's host loop (the NaiveSolver rule) from every row of X in
        lockstep, one batched evaluation and one synchronisation per iteration
        for all of them (fsdf_descend_batch). Returns (X, f [B], iterations
        [B])."""
        X = self._batch_states(X, "descend_batch")
        return self.ctx.descend_batch(X, iteration_limit, rate, max_step, tolerance, divisors, n_points)

    def descend_lm_batch(self, X, iteration_limit, damping, max_step, tolerance=0.0, n_points=1.0,
                         prior_weight=None):
        """descend_lm's host loop from every row of X in lockstep
        (fsdf_descend_lm_batch): one batched (c, g, H) per round over the rows
        still running. prior_weight as descend_lm's, about each row's own start;
        it holds for this call alone. Returns (X, f [B], evaluations [B], final
        dampings [B])."""
        X = self._batch_states(X, "descend_lm_batch")
        ctx = self.ctx
        try:
            if prior_weight is not None:
                ctx.set_lm_prior(prior_weight)
            return ctx.descend_lm_batch(X, iteration_limit, damping, max_step, tolerance, n_points)
        finally:
            if prior_weight is not None:
                ctx.set_lm_prior(None)

    def per_point(self, x):
        """(d*, k*, ∇d*) for every sensed point at configuration x."""
        return self._pass(x, per_point=True)[2]
