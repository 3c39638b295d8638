/*
 * flashsdf.h — C-ABI of the MI355X-native signed-distance residual pass.
 *
 * This is the drop-in boundary for the hot path of Flash.jl
 * (JuliaTagBot/point-cloud-signed-distance). In the reference the path is pure
 * Julia; no FFI exists. The entry points below are exactly what a Julia
 * `ccall` shim under src/tracking.jl would bind:
 *
 *   reference                                     replaced by
 *   ---------------------------------------------------------------------------
 *   Flash.skin(state)          src/Flash.jl:265-268   fsdf_eval / fsdf_skin
 *     (min over surfaces, one closure per point)      (all points in one launch)
 *   skin(state, ::ConvexGeometry) src/Flash.jl:245-250 fsdf_set_model + poses
 *     + ConvexSurface functor  src/Flash.jl:233-243    (exact polytope SDF)
 *   GradientDescent.cost       src/gradientdescent.jl:28-39
 *     c = Σ_p skin(p)^2                               accum[0]
 *     ∂c/∂x via ForwardDiff (Dual{9} chunk passes)    accum[1..6K] wrenches,
 *                                                     chained to ∂c/∂q on host
 *   CostFunctor(manip, pts)    src/gradientdescent.jl:41-57
 *     sensed_points held by reference             fsdf_set_points (once/frame)
 *   EnhancedGJK.NeighborMesh / conv(vertices)   src/models.jl:152
 *                                                     fsdf_convex_hull
 *   transform_to_root(state, frame) src/Flash.jl:248  fsdf_tree_transforms
 *     (RigidBodyDynamics forward kinematics)          (host, per pass; on the
 *                                                     device inside fsdf_descend)
 *
 * Conventions
 *   - All host buffers are caller-owned. Nothing is retained past a call
 *     except what set_model / set_points copy to the device.
 *   - Points are AoS xyz float64, exactly Julia's Vector{SVector{3,Float64}}.
 *   - A pose is 12 float64: R (3x3, row-major) then t (3); x_world = R x_local + t.
 *   - Every function returns 0 (FSDF_OK) or a nonzero status; the message of the
 *     last failure on a context is fsdf_last_error(ctx).
 *   - Accumulator layout (length 1 + 6K + Σ_rbf (4 n_r + 4), K = surfaces):
 *       accum[0]            = Σ_p d*(p)^2                     (cost, no regularizer)
 *       accum[1+6k+0..2]    = Σ_{p: k*(p)=k} 2 d*(p) ∇d*(p)   (force-like, world)
 *       accum[1+6k+3..5]    = Σ_{p: k*(p)=k} 2 d*(p) p × ∇d*(p) (moment about origin)
 *     so that for a world twist (ω, v) of hull k:  δc = -(ω·M_k + v·F_k)
 *     (zero for RBF surfaces); then per RBF surface r with n_r centres, over
 *     the points with k* = r:
 *       λ_w[n_r], λ_a, λ_b[3]  = Σ 2 s ∂s/∂(w, a, b)
 *       E[n_r][3]              = Σ 2 s ∂s/∂c_i (coefficients held fixed)
 *     from which the host forms dc/dc_i = E_i − μᵀ(∂M/∂c_i)u, μ = M⁻ᵀλ.
 *   - Nearest-primitive index k*(p) is the FIRST k attaining the minimum,
 *     matching Julia's left-fold `minimum` (src/Flash.jl:267).
 *   - The library never falls back to a CPU path: without a usable gfx950
 *     device every compute call fails with FSDF_ERR_HIP.
 */
#ifndef FLASHSDF_H
#define FLASHSDF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSDF_OK 0
#define FSDF_ERR_ARG 1        /* bad argument (null pointer, size, index)      */
#define FSDF_ERR_HIP 2        /* HIP runtime failure / no device                */
#define FSDF_ERR_STATE 3      /* call order violated (no model / no points)     */
#define FSDF_ERR_NOMEM 4      /* allocation failure                             */
#define FSDF_ERR_DEGENERATE 5 /* geometry degenerate (coplanar hull input, ...) */

#define FSDF_PRECISION_F64 64
#define FSDF_PRECISION_F32 32

typedef struct fsdf_ctx fsdf_ctx;

typedef struct fsdf_opts {
  int32_t device;      /* HIP device ordinal (process-local)                      */
  int32_t precision;   /* FSDF_PRECISION_F64 (default) or FSDF_PRECISION_F32       */
  int32_t sort_points; /* 1: reorder the resident cloud spatially at set_points
                          (outputs are still returned in caller order)            */
  int32_t cull;        /* 1 (default): exact-safe bounding-sphere culling;
                          0: brute force over every hull (reference loop order)    */
} fsdf_opts;

/* One convex primitive in its body (local) frame.
 * Replaces ConvexGeometry(NeighborMesh(mesh), frame) (src/models.jl:152,159). */
typedef struct fsdf_hull {
  int32_t n_vertices;
  int32_t n_faces;
  const double* vertices; /* [n_vertices][3]                                     */
  const int32_t* faces;   /* [n_faces][3], counter-clockwise seen from outside    */
  const double* planes;   /* [n_faces][4] = (n, d), |n| = 1, n·x <= d inside      */
} fsdf_hull;

/* A scene surface, in the reference's surface order (Manipulator.surfaces,
 * src/Flash.jl:62-65): k* indexes this list.
 *   FSDF_SURFACE_HULL: a convex primitive (`hull`), posed by poses[k].
 *   FSDF_SURFACE_RBF:  an interpolating skin (src/Flash.jl:207-213) over
 *                      `n_centers` centres; its world centres and RBF
 *                      coefficients are supplied per pass (fsdf_set_rbf_params),
 *                      its pose is ignored. Value: s = f/|∇f| with
 *                      f(x) = Σ w_i |x-c_i|^3 + a + b·x (XCubed + affine).
 *                      Matches the reference KAT (test/runtests.jl:17) but NOT
 *                      the costs printed by examples/manipulator.ipynb:5512,
 *                      :14179 (ours 4.44x / 2.0x; no candidate formulation fits
 *                      all three): a documented divergence, DESIGN.md §2. */
#define FSDF_SURFACE_HULL 0
#define FSDF_SURFACE_RBF 1
typedef struct fsdf_surface {
  int32_t kind;      /* FSDF_SURFACE_HULL or FSDF_SURFACE_RBF */
  int32_t n_centers; /* RBF only */
  fsdf_hull hull;    /* HULL only */
} fsdf_surface;

/* ---- geometry ingest (host only, no device needed) --------------------------
 * Convex hull of a point set (the shape GJK's support function sees,
 * EnhancedGJK.NeighborMesh over the mesh vertices, src/models.jl:152).
 * Capacities: vertices_out >= 3n doubles, faces_out >= 3(2n-4) ints,
 * planes_out >= 4(2n-4) doubles. Output faces are triangles, outward, CCW. */
int fsdf_convex_hull(const double* points, int32_t n, int32_t* n_vertices_out,
                     double* vertices_out, int32_t* n_faces_out, int32_t* faces_out,
                     double* planes_out);

/* Forward kinematics of a mechanism tree (host only, no device): the body
 * poses transform_to_root(state, body) that the per-pass surface poses are
 * built from (src/Flash.jl:248; RigidBodyDynamics in the reference). Bodies in
 * topological order (parent[b] < b, body 0 = root). Per body b >= 1:
 * kind 0 fixed, 1 revolute about unit axis[b] by q[qoff[b]], 2 quaternion
 * floating q[qoff[b] .. +7] = (w, x, y, z, tx, ty, tz) (normalized here);
 * joint_to_parent (AR[b] row-major 3x3, At[b]) and body_to_joint (BR[b], Bt[b]).
 * Out: R[b], t[b] = transform_to_root(body b); Rb[b], tb[b] = the parent's
 * transform composed with joint_to_parent (the joint frame before its motion,
 * where the chain rule's motion subspaces live). All arrays [nb][9] / [nb][3]. */
int fsdf_tree_transforms(int32_t nb, const int32_t* parent, const int32_t* kind, const int32_t* qoff,
                         const double* axis, const double* AR, const double* At, const double* BR,
                         const double* Bt, const double* q, double* R, double* t, double* Rb, double* tb);

/* Host chain rule (no device): ∂c/∂q of the mechanism from the accumulator's
 * per-surface wrenches (surface_wrench[k] = accum[1+6k .. 7+6k]: F, M about the
 * world origin) on surface_body[k] (-1: none), plus optional per-body wrenches
 * body_wrench [nb][6] (the RBF chain's); tree arrays as fsdf_tree_transforms,
 * Rb/tb = its joint frames before the motion; work = nb*6 doubles of scratch;
 * gq [num_positions]. Replaces ForwardDiff's ⌈n/9⌉ Dual passes through
 * RigidBodyDynamics (src/gradientdescent.jl:28-39, src/tracking.jl:16-21) for
 * fixed, revolute and quaternion-floating joints (with normalize!'s projection,
 * src/gradientdescent.jl:30); flash/mechanism.py config_gradient is the numpy
 * twin the tests compare it with. */
int fsdf_config_gradient(int32_t nb, const int32_t* parent, const int32_t* kind, const int32_t* qoff,
                         const double* axis, const double* Rb, const double* tb, const double* q, int32_t nsurf,
                         const int32_t* surface_body, const double* surface_wrench, const double* body_wrench,
                         double* work, double* gq);

/* RBF weight solve and its adjoint (host only, no device; the host side of
 * the interpolating skins, src/Flash.jl:143-213, around fsdf_set_rbf_params and
 * the pass). fsdf_rbf_solve: centres [n][3] (world), values [n] (0 surface
 * points, -1 skeleton points) -> u [n+4] = (w, a, b) of
 * [A P; Pᵀ 0] u = [v; 0], A_ij = |c_i - c_j|^3, P_i = (1, c_iᵀ); lu
 * [(n+4)^2] and piv [n+4] receive the factorization for the adjoint.
 * fsdf_rbf_adjoint: this surface's accumulator block [4n+4] (λ [n+4], then E
 * [n][3]) -> G [n][3] = ∂cost/∂c_j (world); work [n+4]. flash/rbf.py solve /
 * chain are the numpy twins. FSDF_ERR_DEGENERATE: singular system. */
int fsdf_rbf_solve(int32_t n, const double* centres, const double* values, double* u, double* lu, int32_t* piv);
int fsdf_rbf_adjoint(int32_t n, const double* centres, const double* u, const double* lu, const int32_t* piv,
                     const double* block, double* G, double* work);

/* The whole CostFunctor iteration of a rigid (hull-only) scene in one call:
 * fsdf_set_mechanism registers the mechanism tree (the arrays of
 * fsdf_tree_transforms, nq = num_positions) and, per surface of
 * fsdf_set_surfaces, its body (-1: none) and body-to-geometry frame (R
 * row-major [S][9], t [S][3]); fsdf_value_and_gradient(x) then runs host FK,
 * the surface poses, one residual pass over the resident cloud, and the chain
 * rule: cost_out = Σ_p d*(p)^2 and grad_out [nq] = ∂cost/∂x at the caller's x
 * (quaternion blocks normalized for the evaluation, the projection in the
 * gradient) — CostFunctor(x) with its ForwardDiff gradient
 * (src/gradientdescent.jl:28-57). Scenes with RBF skins also declare their
 * centres (fsdf_set_rbf_centres, below; FSDF_ERR_STATE until every RBF
 * surface has them). */
int fsdf_set_mechanism(fsdf_ctx* ctx, int32_t nb, const int32_t* parent, const int32_t* kind, const int32_t* qoff,
                       const double* axis, const double* AR, const double* At, const double* BR, const double* Bt,
                       int32_t nq, const int32_t* surface_body, const double* frame_R, const double* frame_t);
int fsdf_value_and_gradient(fsdf_ctx* ctx, const double* x, double* cost_out, double* grad_out);
/* RBF scenes in fsdf_value_and_gradient: after fsdf_set_mechanism (which
 * clears earlier declarations) every RBF surface's centres are declared once —
 * n_sp surface points (body, body-frame xyz, deformation row or -1; value 0)
 * then n_sk skeleton points (value -1), n_sp + n_sk = its n_centers
 * (src/Flash.jl:143-213) — and fsdf_set_deformations gives the deformation
 * count (x = [q; δ], 3 per deformable point, src/gradientdescent.jl:9-17) and
 * the regularizer weight (default_deformation_cost_weight = 10, :7). value_and_gradient then also
 * places the centres (c = R_b (p + δ) + t_b), solves the weights, uploads the
 * rows, and chains the pass's RBF block through the solve: cost_out = Σ d*^2 +
 * weight Σ|δ|^2, grad_out [nq + 3 n_deform] (CostFunctor(x) with its gradient,
 * src/gradientdescent.jl:28-57). */
int fsdf_set_rbf_centres(fsdf_ctx* ctx, int32_t surface, int32_t n_sp, const int32_t* body_sp,
                         const double* local_sp, const int32_t* deform_row_sp, int32_t n_sk, const int32_t* body_sk,
                         const double* local_sk);
int fsdf_set_deformations(fsdf_ctx* ctx, int32_t n_deform, double weight);
/* The same iteration split around a multi-GPU all-reduce (one context per
 * rank, each over its shard): fsdf_eval_state_device(x) runs FK, the RBF solve,
 * the poses and the pass into the DEVICE accumulator d_accum (asynchronous on
 * the context's stream); after the caller's all-reduce (RCCL) and read-back,
 * fsdf_state_gradient(x, accum) returns cost and gradient as
 * fsdf_value_and_gradient does, on the FK / weight solve of that pass. x may
 * be the x of either of this context's last two fsdf_eval_state_device passes
 * (pipelined passes: the next pass is enqueued before the previous all-reduce
 * completes): the host FK and weight solve are then redone for x — the same
 * arithmetic, the same bits. Any other x (not the configuration of an
 * accumulator this context produced) is refused with FSDF_ERR_STATE. */
int fsdf_eval_state_device(fsdf_ctx* ctx, const double* x, double* d_accum);
int fsdf_state_gradient(fsdf_ctx* ctx, const double* x, const double* accum, double* cost_out, double* grad_out);

/* estimate_state's solver loop (src/tracking.jl:16-26: wrapped_cost c/N, warm
 * start x) around fsdf_value_and_gradient, with no host-language round trip per
 * iteration. Up to iteration_limit times: f = cost/n_points, g = (grad/n_points)
 * ./ divisors (NULL = ones); stop when |g|_2 < tolerance; else x += clamp(-rate g,
 * ±max_step) component-wise (NaiveSolver's rule as restated in
 * flash/tracking.py — the solver itself is the un-vendored
 * SimpleGradientDescent.jl; the rule is pinned by examples/manipulator.ipynb's
 * own per-trial traces, tests/test_manipulator_traces.py). n_points = 1
 * reproduces the notebook's session, whose objective was the undivided c.
 * x [nq + 3 n_deform] is updated in place;
 * value_out = f of the last evaluation, iterations_out = evaluations made. */
int fsdf_descend(fsdf_ctx* ctx, double* x, int32_t iteration_limit, double rate, double max_step, double tolerance,
                 const double* divisors, double n_points, double* value_out, int32_t* iterations_out);
/* Where fsdf_descend iterates. device_loop = 1 (default): rigid scenes (no RBF
 * skin, no deformation) iterate on the device where the mechanism fits the
 * solver step's 64 KB of LDS, others on the host; 0: always the host loop
 * around fsdf_value_and_gradient, one synchronization per iteration; 2: the
 * device loop is required (FSDF_ERR_STATE otherwise; scenes with RBF skins or
 * deformations are refused); 3: as 1, and scenes with RBF skins or deformations
 * iterate on the device too — the step then also runs the adjoint of the
 * skins' weight solve, the deformation gradient and regularizer, and after its
 * FK the new centres, the (n+4)x(n+4) LU and the weight solve, and writes the
 * next pass's RBF rows (csrc/rbf_impl.h, the host's arithmetic) — where every
 * skin's system fits the step's LDS with the rest (n + 4 <= 128 and all LU
 * factors in the 64 KB), others on the host; 4: as 2 with those scenes
 * admitted (3 and 4 decide by the same condition: what 4 refuses is what 3
 * runs on the host). A singular RBF system fails the frame with FSDF_ERR_DEGENERATE, as
 * on the host. After a device frame of such a scene the RBF rows on the device
 * are those of the last posed x. The device loop enqueues
 * the frame's passes and solver steps up front and reads x, value and count
 * back once (csrc/solver.hip: FK, chain rule, the clipped NaiveSolver step and
 * the next pass's pose after each pass, the host loop's arithmetic in the same
 * order — x, value and iterations bit-identical to it; after convergence the
 * remaining launches return at once). Measured: on
 * resident clouds 7-8 % faster per iteration than the host loop (C2, C4, M64),
 * per fresh 2^20 frame 1.5 % (M64) or level (IRB140). */
int fsdf_set_solver(fsdf_ctx* ctx, int32_t device_loop);

/* ---- second-order solver: host side (no device) -------------------------------
 * The cost is a sum of squares, c = Σ_p d*(p)^2, so a Gauss-Newton step with
 * Levenberg-Marquardt damping fits it (the reference's notebooks swap in a
 * second-order solver, Ipopt in examples/squishable.ipynb, where the naive one
 * is too slow). For a point p with nearest surface k and world gradient
 * n = ∇d*(p), let w_p = (n, p × n) ∈ R^6 — the accumulator's wrench order: force
 * slots, then the moment about the world origin — and per surface the second
 * moments
 *     moments[k][21] = Σ_{p: k*(p)=k} w_p w_pᵀ     (upper triangle, row-major:
 *                                                    00 01 .. 05 11 .. 55)
 * The two functions below are the host half of that solver: the matrix JᵀJ
 * from the moments, and one damped step. The moments are reduced on the device
 * (fsdf_eval_moments, fsdf_value_gradient_hessian below), and fsdf_descend_lm is
 * the solver loop over them.
 *
 * fsdf_gauss_newton_matrix, the sibling of fsdf_config_gradient: the
 * Gauss-Newton matrix A [nq][nq] = Σ_k S_b(k) M_k S_b(k)ᵀ of the mechanism from
 * the per-surface moments [nsurf][21], where S_b (nq x 6) is the linear map
 * fsdf_config_gradient applies to a wrench on body b = surface_body[k] (-1:
 * skipped): ∂d*(p)/∂x_i = (S_b)_i · w_p; 2A is the Gauss-Newton Hessian of the
 * cost. Its rows are the joints' motion rows of the chain rule, the quaternion
 * rows with their (I − q̂q̂ᵀ)/|q| projection at the caller's un-normalised q.
 * Composite form: moments summed per body, then over subtrees, then each
 * coordinate against those on its path to the root — O(n_dof · depth · 36).
 * Tree arrays, Rb / tb and q as fsdf_config_gradient; work = 36 nb + 6 nq
 * doubles. A is symmetric (exactly) and positive semi-definite when the
 * moments are. flash/mechanism.py gauss_newton_matrix_numpy is the numpy twin. */
int fsdf_gauss_newton_matrix(int32_t nb, const int32_t* parent, const int32_t* kind, const int32_t* qoff,
                             const double* axis, const double* Rb, const double* tb, const double* q, int32_t nsurf,
                             const int32_t* surface_body, const double* moments, int32_t nq, double* work,
                             double* A_out);
/* One damped step: D_ii = max(H_ii, 1e-12 max_j H_jj); Cholesky of
 * H + lambda diag(D) (H symmetric [n][n], its lower triangle is read);
 * dx_out = clamp(−(H + lambda D)^-1 g, ±max_step) component-wise; work =
 * n^2 + n doubles. FSDF_ERR_DEGENERATE when the factorisation meets a
 * non-positive or non-finite pivot (or the solve is not finite).
 * flash.tracking.LevenbergMarquardt loops over it: a trial that does not lower
 * the cost is rejected and lambda raised tenfold, an accepted one lowers it
 * tenfold. */
int fsdf_lm_step(int32_t n, const double* H, const double* g, double lambda, double max_step, double* work,
                 double* dx_out);
/* The Levenberg-Marquardt loop (host only, no device): replaces
 * flash.tracking.LevenbergMarquardt.optimize, operation for operation — x, f,
 * the evaluation count and the final damping are bit-identical to it. fn
 * evaluates the objective at x: *f, g [n], H [n][n] (the Gauss-Newton Hessian);
 * a nonzero return ends the loop with that status (x the last accepted point).
 * One evaluation at the start x; then until iteration_limit evaluations: stop
 * when |g|_2 (summed in index order) < tolerance; a step by fsdf_lm_step at
 * the current damping — a degenerate one raises the damping tenfold without an
 * evaluation; the trial x + step is accepted only when its f is lower (a NaN is
 * not), the damping then divided by 10 (down to 1e-12), else multiplied by 10;
 * a damping beyond 1e12 ends the loop. x [n] is updated in place; work =
 * 3 n^2 + 5 n doubles; value_out = f at x (NaN when iteration_limit is 0),
 * iterations_out = evaluations made, damping_out = the final damping (outputs
 * may be NULL). */
typedef int (*fsdf_vgh_fn)(void* user, const double* x, double* f, double* g, double* H);
int fsdf_lm_minimize(fsdf_vgh_fn fn, void* user, int32_t n, double* x, int32_t iteration_limit, double damping,
                     double max_step, double tolerance, double* work, double* value_out, int32_t* iterations_out,
                     double* damping_out);

/* ---- Gauss-Newton for RBF skins: host side (no device) --------------------------
 * A point p whose nearest surface is an RBF skin of n centres has the residual
 * s(p) = f/|∇f| (fsdf_set_rbf_params), and in the skin's m = 4n + 4 parameters
 * the row j(p) ∈ R^m, laid out as the skin's accumulator block:
 *     ∂s/∂w [n], ∂s/∂a, ∂s/∂b [3], ∂s/∂c [n][3]   (coefficients fixed for ∂s/∂c)
 * With dsdf = 1/|∇f|, c = f/|∇f|^3, u = −c ∇f and per centre d = p − c_i,
 * ρ = |d|, e = d·u:  ∂s/∂w_i = dsdf ρ^3 + 3 ρ e;  ∂s/∂c_i = −w_i (k1 d + 3ρ u),
 * k1 = 3ρ dsdf + (ρ > 0 ? 3e/ρ : 0);  ∂s/∂a = dsdf;  ∂s/∂b = dsdf p + u — the
 * summands of the accumulator block without their factor 2s (the block is
 * Σ 2 s j). The skin's second moment is
 *     M [m][m] = Σ_{p: k*(p) = the skin} j(p) j(p)ᵀ   (row-major, full, symmetric)
 * (reduced on the device: fsdf_eval_skin_moments below), and ∂s/∂x = L j with L
 * (nx x m, nx = nq + 3 n_deform) the linear map fsdf_value_and_gradient applies
 * to the block: fsdf_rbf_adjoint, the centre forces to body wrenches and ∂/∂δ,
 * fsdf_config_gradient. So JᵀJ gains L M Lᵀ per skin, and the Gauss-Newton
 * Hessian of cost = Σ d*^2 + weight Σ|δ|^2 is
 *     H = 2 (A_hulls + Σ_r L_r M_r L_rᵀ) + 2 weight I on the deformations,
 * A_hulls = fsdf_gauss_newton_matrix over the hull surfaces, in the nq block.
 * Replaces what the reference reaches for Ipopt for on its deformable scene
 * (examples/squishable.ipynb). No cross terms between surfaces exist: every
 * point has one nearest surface.
 *
 * fsdf_rbf_state_map: one skin's L [nx][m], row-major, built by sending the m
 * unit blocks through that same code, so it is the gradient's map by
 * construction, signs and quaternion projection included. Tree arrays, Rb / tb
 * and q (the caller's, un-normalised) as fsdf_config_gradient; R [nb][9] the
 * bodies' rotations (fsdf_tree_transforms); centres, u, lu, piv as
 * fsdf_rbf_solve left them; body [n] each centre's body (-1: world), drow [n]
 * its deformation row (-1: none; NULL: none has one), rows < n_deform.
 * work = 8n + 8 + 12 nb + nx doubles. flash/rbf.py state_map is the numpy twin.
 *
 * fsdf_gauss_newton_add: A [nx][nx] += L M Lᵀ, symmetrised exactly: the upper
 * triangle of A is read and added to, the lower overwritten with its mirror
 * image. work = nx m doubles. Both: FSDF_ERR_ARG for bad arguments; limits
 * are the caller's memory alone. */
int fsdf_rbf_state_map(int32_t nb, const int32_t* parent, const int32_t* kind, const int32_t* qoff, const double* axis,
                       const double* R, const double* Rb, const double* tb, const double* q, int32_t nq, int32_t n,
                       const double* centres, const double* u, const double* lu, const int32_t* piv,
                       const int32_t* body, const int32_t* drow, int32_t n_deform, double* work, double* L_out);
int fsdf_gauss_newton_add(int32_t nx, int32_t m, const double* L, const double* M, double* work, double* A);

/* ---- second-order solver: device side ------------------------------------------
 * The moments above, reduced on the device (csrc/moments.hip): a launch of its
 * own after the pass — the pass kernels are the headline path's, unchanged —
 * over the pass's per-point k* and ∇d* in resident order, one wave per 64-point
 * chunk, per distinct k* of the wave a masked wave sum of the 21 products into
 * the wave's [S][21] table in LDS; every workgroup a fixed run of chunks, its
 * waves' tables summed in wave order, the workgroups' partials in workgroup
 * order. No floating-point atomics: for a given cloud layout the moments are
 * bit-identical from run to run, with the planned pass on or off. All
 * arithmetic is fp64 (fp32 contexts: their fp32 points, widened). Rigid scenes
 * only: a scene with RBF skins or deformations is refused with FSDF_ERR_STATE,
 * as is one whose table does not fit 64 KB of LDS (more than 390 surfaces).
 *
 * fsdf_eval_moments: fsdf_eval's pass over the resident cloud plus the moments,
 * moments_out [S][21] host (required; cost_out, accum_out may be NULL).
 * Synchronous. Replaces forming the moments on the host from fsdf_eval's
 * per-point outputs. A cloud of no points gives zero moments.
 *
 * fsdf_value_gradient_hessian: fsdf_value_and_gradient plus hess_out [nq][nq] =
 * 2 JᵀJ, the Gauss-Newton Hessian of the cost, by fsdf_gauss_newton_matrix on
 * that pass's FK and moments. cost_out and grad_out are bit-identical to
 * fsdf_value_and_gradient's at the same x and cloud layout. The auto regroup of
 * the iteration entry points applies (fsdf_set_regroup), queued after the
 * moments launch. Replaces the (c, g, H) objective a caller of
 * LevenbergMarquardt.optimize assembled from per-point outputs.
 *
 * fsdf_descend_lm: fsdf_lm_minimize over fsdf_value_gradient_hessian with
 * estimate_state's wrapped cost (src/tracking.jl:16-21): f = cost / n_points,
 * g = grad / n_points, H / n_points — fsdf_descend's sibling for the
 * second-order solver. By default a host loop, one synchronization per
 * evaluation (fsdf_set_lm_solver: the device loop). x [nq] is updated in
 * place; outputs as fsdf_lm_minimize's.
 *
 * fsdf_set_lm_prior: a prior on the frame's start state for fsdf_descend_lm.
 * Gauss-Newton moves coordinates the cloud does not determine (a wrist joint
 * under a noisy cloud: H_ii / N of 1e-5 .. 1e-9 against 1e-2 for the shoulder)
 * by radians for a last 1e-6 of cost; with weights mu [nq], each >= 0, the
 * objective of fsdf_descend_lm becomes
 *     F(x) = c(x) / N + Σ_i mu_i (x_i − x̄_i)^2,
 * x̄ the x handed to that call (the frame's warm start). One operation order,
 * shared with flash.tracking.state_prior (the same bits): e_i = x_i − x̄_i;
 * r = 0.0, r += mu_i * (e_i * e_i) in index order; f = c / N + r;
 * g_i = g_i / N + (2.0 mu_i) e_i; H_ii = H_ii / N + 2.0 mu_i. weight NULL or
 * n = 0 clears the prior (the default: fsdf_descend_lm is then exactly what it
 * was, no zeros added); a negative or non-finite weight is FSDF_ERR_ARG; n
 * other than nq is FSDF_ERR_STATE at the next fsdf_descend_lm;
 * fsdf_set_mechanism clears it. Quaternion coordinates are penalised raw
 * (un-normalised): a weight on a quaternion's four entries also fixes the
 * quaternion's scale, which the cost itself leaves free. fsdf_lm_minimize and
 * fsdf_lm_step know nothing of it: the prior is part of the objective.
 *
 * fsdf_set_lm_solver: where fsdf_descend_lm's loop runs. 0 (the default): the
 * host loop above. 1: the device loop where the scene fits, the host loop
 * otherwise. 2: the device loop is required — FSDF_ERR_STATE for a scene
 * without resident points or whose solver kernels' work arrays do not fit
 * their 64 KB of LDS (at most 64 joint coordinates; M64's 65 bodies, 48
 * coordinates and 64 surfaces take 60 KB), FSDF_ERR_ARG for a damping that is
 * not > 0 (mode 1 then takes the host loop: the device step's raises of a
 * degenerate factorisation are bounded only from a positive damping). The
 * device loop (csrc/lm_solver.hip) enqueues the whole frame up front, as
 * fsdf_descend's: FK of x and the first posed model, then per evaluation the
 * pass with k* and ∇d* in resident order, its reduce, the moments and their
 * reduce, one single-workgroup LM step — chain rule, the prior, accept or
 * reject, on acceptance the Gauss-Newton matrix, the end conditions, the
 * Cholesky step, the next trial — and the FK and pose of that trial; after the
 * end the remaining launches return at once; x, value, count and damping are
 * read back once. The arithmetic is the host loop's in its order
 * (csrc/gn_impl.h, csrc/kin_impl.h): x, value, the evaluation count and the
 * final damping are bit-identical to mode 0. A configuration whose poses are
 * not finite fails the frame with FSDF_ERR_ARG (the host loop goes on with a
 * NaN cost). */
int fsdf_set_lm_prior(fsdf_ctx* ctx, const double* weight, int32_t n);
int fsdf_set_lm_solver(fsdf_ctx* ctx, int32_t device_loop);
int fsdf_eval_moments(fsdf_ctx* ctx, const double* poses, double* cost_out, double* accum_out, double* moments_out);
int fsdf_value_gradient_hessian(fsdf_ctx* ctx, const double* x, double* cost_out, double* grad_out,
                                double* hess_out);
int fsdf_descend_lm(fsdf_ctx* ctx, double* x, int32_t iteration_limit, double damping, double max_step,
                    double tolerance, double n_points, double* value_out, int32_t* iterations_out,
                    double* damping_out);

/* ---- robust point losses -------------------------------------------------------
 * The cost Σ d*(p)² gives a far point — a depth outlier, a point of another
 * object — a pull that grows with its distance. A loss (kind, scale c > 0)
 * bounds it. It is given by its weight w(d) = ρ′(d) / (2d), with ρ(d) = d² near
 * zero (one definition and operation order: csrc/robust_impl.h, restated in
 * numpy by flash/robust.py):
 *   FSDF_LOSS_SQUARE  w = 1, ρ = d² (the default: no loss).
 *   FSDF_LOSS_HUBER   |d| <= c: w = 1, ρ = d²; else w = c / |d|, ρ = 2c|d| − c².
 *   FSDF_LOSS_TUKEY   u = d / c; |d| < c: w = (1 − u²)², ρ = (c²/3)(1 − (1 − u²)³);
 *                     else w = 0 exactly, ρ = c²/3.
 * With v = (∇d*, p × ∇d*), per surface k over the points with k*(p) = k the
 * robust objective and its Gauss-Newton (IRLS) model are: cost Σ ρ(d*); wrench
 * (F_k, M_k) = Σ 2 w d* v, in the accumulator's slots and sign; moments
 * Σ w v vᵀ (21 entries, the order of fsdf_gauss_newton_matrix); W_k = Σ w, the
 * surface's effective inlier count. H = 2 Σ_k JᵀM_kJ stays positive
 * semi-definite: the second-order term of ρ is dropped. They are reduced on the
 * device by a launch of its own after the pass (csrc/robust.hip: the design of
 * the moments' reduction above, no floating-point atomics, bit-identical from
 * run to run for a given cloud layout), from the pass's k*, d* and ∇d* in
 * resident order; all arithmetic fp64, an fp32 context's pass outputs as
 * stored. Hull-only scenes of at most 282 surfaces (the workgroup's tables in
 * 64 KB of LDS; fsdf_set_surfaces itself holds a scene to 256); beyond,
 * FSDF_ERR_STATE.
 *
 * fsdf_set_loss: a context setting, kept over model and cloud swaps; only
 * FSDF_LOSS_SQUARE clears it (its scale is ignored). An unknown kind, or a
 * Huber / Tukey scale that is not finite and > 0, is FSDF_ERR_ARG.
 * fsdf_get_loss reads it back (either output may be NULL).
 *
 * fsdf_eval_robust: fsdf_eval's pass over the resident cloud, then the sums
 * above under the context's loss. accum_out [1 + 6S] in fsdf_eval's layout:
 * [0] = cost = Σρ, the surfaces' sums added in surface order; then every
 * surface's wrench. moments_out [S][21] and weight_out [S] (W_k); every output
 * may be NULL. Synchronous; needs no mechanism; a scene with an RBF skin is
 * FSDF_ERR_STATE; a cloud of no points gives exact zeros. With
 * FSDF_LOSS_SQUARE set it returns the least-squares sums as this reduction
 * forms them: fsdf_eval_moments' cost, wrench and moments to rounding.
 *
 * With a loss other than FSDF_LOSS_SQUARE set, on a rigid scene (no RBF skin,
 * no deformation; others: FSDF_ERR_STATE from the four calls below):
 * fsdf_value_and_gradient and fsdf_value_gradient_hessian evaluate the robust
 * objective — the same FK, chain rule and fsdf_gauss_newton_matrix, on the
 * robust accumulator and moments; cost_out and grad_out of the two are
 * bit-identical at the same x and cloud layout; the auto regroup is queued
 * after the robust launch. fsdf_descend and fsdf_descend_lm inherit it through
 * their host loops, and fsdf_set_lm_prior applies unchanged. The device loops
 * do not serve a loss: fsdf_set_solver 1 / 3 and fsdf_set_lm_solver 1 take the
 * host loop, the required modes (fsdf_set_solver 2 / 4, fsdf_set_lm_solver 2)
 * return FSDF_ERR_STATE. fsdf_eval, fsdf_eval_device, fsdf_eval_moments,
 * fsdf_eval_skin_moments, fsdf_skin, fsdf_raycast, fsdf_eval_state_device and
 * fsdf_state_gradient are least squares always, whatever the loss. With
 * FSDF_LOSS_SQUARE every call returns the bits it returned before there was a
 * loss. */
enum { FSDF_LOSS_SQUARE = 0, FSDF_LOSS_HUBER = 1, FSDF_LOSS_TUKEY = 2 };
int fsdf_set_loss(fsdf_ctx* ctx, int32_t kind, double scale);
/* fsdf_set_loss with the scale read through a pointer, for bindings that pass
 * every floating-point argument by reference (julia/FlashSDF.jl); NULL reads
 * as 0.0 (FSDF_LOSS_SQUARE ignores it). */
int fsdf_set_loss_ref(fsdf_ctx* ctx, int32_t kind, const double* scale);
int fsdf_get_loss(const fsdf_ctx* ctx, int32_t* kind_out, double* scale_out);
int fsdf_eval_robust(fsdf_ctx* ctx, const double* poses, double* cost_out, double* accum_out /* [1+6S] */,
                     double* moments_out /* [S][21] or NULL */, double* weight_out /* [S] or NULL */);

/* ---- per-point confidence weights ----------------------------------------------
 * A loss bounds what a point does after its residual is known; a weight says
 * what the caller knows before the pass: a depth sensor's noise at the point's
 * range, the probability that the point belongs to the scene, the number of
 * points a subsampled one stands for. A weight a_i >= 0 (finite) per resident
 * point enters every sum of the robust objective above, with w = w(d*) and ρ of
 * the context's loss: cost Σ a ρ(d*); wrench Σ 2 a w d* v; moments Σ a w v vᵀ;
 * W_k = Σ a w. With FSDF_LOSS_SQUARE this is weighted least squares (w = 1,
 * ρ = d²). H = 2 Σ_k JᵀM_kJ stays positive semi-definite because a >= 0. The
 * reduction (csrc/robust.hip, its WEIGHTED instantiations) forms one product
 * aw = a · w per point and uses it wherever w stands, and a · ρ for the cost. A
 * point of weight 0 stays in the sums as zero terms: the summation order is a
 * function of the cloud layout alone, as without weights, and the results are
 * bit-identical from run to run. Weights all 1 give the bits of the same calls
 * without weights; weights all 2^-k scale every sum exactly. The solver loops'
 * n_points divisor is the caller's as before (the cost is c / N): a caller who
 * wants c / Σa passes weights of mean 1.
 *
 * fsdf_set_point_weights: a host array of n doubles in the CALLER'S order of
 * the resident cloud — the order of the array the cloud was set from, whatever
 * the sort or a regroup did to the resident order. n must equal the resident
 * cloud's size (else FSDF_ERR_ARG); a weight that is negative or not finite is
 * FSDF_ERR_ARG, and the weights held before stay in force. weights == NULL
 * clears: every point counts 1 again, on the code path of a context that never
 * had weights (n is ignored). Synchronous: the array may be reused on return.
 * fsdf_set_point_weights_device: the same from device memory, stream-ordered
 * on the context stream, with NO validation: the caller vouches for finite,
 * non-negative values.
 * fsdf_get_point_weights: *set_out = 1 when weights are set, and out [n] (may
 * be NULL) the weights in RESIDENT order — the order fsdf_permutation names
 * and resident-order per-point outputs come in: out[i] is the caller's weight
 * fsdf_permutation()[i] (no permutation: the caller's order). Synchronous.
 *
 * Weights belong to the resident cloud. Every call that makes another cloud
 * resident clears them (fsdf_set_points, _device, _prefetched, _range*,
 * _keyed_device): set them after the cloud. They survive fsdf_regroup_points
 * and the auto regroup: the resident-order copy (csrc/point_weights.hip, a
 * gather through the permutation) is rebuilt before the next robust launch,
 * once per layout change. On a ranged or keyed cloud the two set calls return
 * FSDF_ERR_STATE.
 *
 * With weights set, on a hull-only rigid scene: fsdf_eval_robust,
 * fsdf_value_and_gradient and fsdf_value_gradient_hessian evaluate the weighted
 * objective through the robust path, also when the loss is FSDF_LOSS_SQUARE;
 * fsdf_descend and fsdf_descend_lm inherit it through their host loops, and
 * fsdf_set_lm_prior applies unchanged. The refusals are the loss's: a scene
 * with an RBF skin or a deformation is FSDF_ERR_STATE from those calls; the
 * device loops do not serve weights (fsdf_set_solver 1 / 3 and
 * fsdf_set_lm_solver 1 take the host loop, the required modes return
 * FSDF_ERR_STATE). fsdf_eval, fsdf_eval_device, fsdf_eval_moments, fsdf_skin,
 * fsdf_raycast, fsdf_eval_state_device and fsdf_state_gradient ignore weights,
 * as they ignore the loss. Without weights every call returns the bits it
 * returned before there were any. */
int fsdf_set_point_weights(fsdf_ctx* ctx, const double* weights /* [n], caller order, or NULL */, int64_t n);
int fsdf_set_point_weights_device(fsdf_ctx* ctx, const double* d_weights /* [n], caller order */, int64_t n);
int fsdf_get_point_weights(fsdf_ctx* ctx, double* out /* [n], resident order, or NULL */, int32_t* set_out);

/* ---- depth frames ----------------------------------------------------------------
 * What a depth camera delivers is an image: 2 to 8 bytes per pixel over rays
 * that never change (the reference's DepthSensor holds rays[rows, cols], a
 * frame is the distances along them, and raycast_points turns those into the
 * cloud, row-major with the misses dropped: src/depthsensors.jl:99-113). Here
 * the rays stay resident, a frame is the depth image plus the sensor's pose,
 * and the device back-projects and compacts the valid pixels
 * (csrc/depth.hip: a count, a scan and a scatter on the context stream — no
 * atomics, no workgroup waiting on another: the output order is a function of
 * the image alone, bit-identical from run to run) and hands the fp64 cloud to
 * the path of fsdf_set_points_device. The host link carries the image instead
 * of 24 bytes per point, and every resident point knows its pixel
 * (fsdf_get_depth_pixels), which is what per-pixel confidences need
 * (fsdf_set_point_weights takes the caller's order, the order of that list).
 *
 * fsdf_set_sensor: rays [rows*cols][3] in the camera frame, row-major (pixel
 * row*cols + col) — a context setting like the loss: it survives cloud and
 * model swaps. One direction u per pixel is computed on the host, once, and
 * kept on the device as fp64:
 *   FSDF_DEPTH_RANGE  the depth is the distance along the ray (the reference's
 *                     model): u = r / sqrt((x·x + y·y) + z·z), each component
 *                     divided;
 *   FSDF_DEPTH_Z      the depth is the camera-frame z (what real cameras
 *                     report): u = (x / z, y / z, 1.0).
 * A ray that is not finite or has no length, FSDF_DEPTH_Z with z <= 0, rows or
 * cols < 1, rows·cols >= 2^31 or an unknown kind is FSDF_ERR_ARG and the earlier
 * sensor stays. rays == NULL clears the sensor (rows, cols, kind ignored).
 * fsdf_get_sensor: the sensor's shape and kind (rows 0: none); any output may
 * be NULL.
 *
 * fsdf_set_depth_f64 / _f32 / _u16: a host image [rows*cols] of the sensor's
 * shape becomes the resident cloud. pose: the project's 12 doubles (R
 * row-major, then t) of the sensor in the world, NULL = identity. range:
 * {near, far, scale}, NULL = {0, +inf, 1}. Per pixel i, in this operation
 * order and uncontracted:
 *   s = scale · (double)depth_i     (the widening is exact for all three formats)
 *   valid iff s is finite, s > 0, s >= near and s <= far
 *   c = (s·u_x, s·u_y, s·u_z)
 *   p_j = ((R_j0·c_x + R_j1·c_y) + R_j2·c_z) + t_j
 * The resident cloud is the valid pixels' points in row-major pixel order: the
 * order of raycast_points, and the CALLER ORDER of this cloud (per-point
 * outputs, fsdf_get_permutation, fsdf_set_point_weights).
 * flash/depthsensors.py depth_points restates the arithmetic operation for
 * operation: the same bits. From there the frame is exactly
 * fsdf_set_points_device of that fp64 array — the Hilbert sort and
 * permutation with sort_points, the fp32 conversion of fp32 contexts, the chunk
 * spheres, the seeds carried from the previous cloud, cleared point weights, a
 * pending auto regroup — by calling that path. Synchronous like
 * fsdf_set_points: the image may be reused on return. No sensor:
 * FSDF_ERR_STATE. A pose entry that is not finite, a NaN near or far,
 * near > far, or a scale that is not finite and > 0: FSDF_ERR_ARG; in all of
 * these the resident cloud stays. A frame with no valid pixel makes a cloud of
 * 0 points resident: not an error (a pass over it costs 0).
 * fsdf_set_depth_device: the same from an image in device memory (format
 * FSDF_DEPTH_F64 / _F32 / _U16): only the upload is skipped.
 *
 * fsdf_get_depth_pixels: pixels_out[i] = row·cols + col of caller point i, *n_out
 * the cloud's size; pixels_out may be NULL to read n alone. FSDF_ERR_STATE when
 * the resident cloud did not come from a depth frame (every fsdf_set_points*
 * ends a depth frame's list). Synchronous.
 *
 * Not done: a prefetched depth frame (fsdf_prefetch_points has no depth form: a
 * live sensor has no next frame); ranged and keyed (sharded) depth frames;
 * weights computed on the device other than a voxel grid's multiplicities
 * ("voxel grid" below; the caller forms any others from the pixel list).
 * The free-space term for what the rays passed through and for the pixels that
 * saw nothing: "free space" below. */
enum { FSDF_DEPTH_RANGE = 0, FSDF_DEPTH_Z = 1 };
int fsdf_set_sensor(fsdf_ctx* ctx, const double* rays /* [rows*cols][3], camera frame, row-major, or NULL */,
                    int32_t rows, int32_t cols, int32_t depth_kind);
int fsdf_get_sensor(const fsdf_ctx* ctx, int32_t* rows_out, int32_t* cols_out, int32_t* kind_out);
int fsdf_set_depth_f64(fsdf_ctx* ctx, const double* depth, const double* pose /* [12] or NULL */,
                       const double* range /* [3] or NULL */);
int fsdf_set_depth_f32(fsdf_ctx* ctx, const float* depth, const double* pose, const double* range);
int fsdf_set_depth_u16(fsdf_ctx* ctx, const uint16_t* depth, const double* pose, const double* range);
enum { FSDF_DEPTH_F64 = 0, FSDF_DEPTH_F32 = 1, FSDF_DEPTH_U16 = 2 };
int fsdf_set_depth_device(fsdf_ctx* ctx, const void* d_depth, int32_t format, const double* pose, const double* range);
int fsdf_get_depth_pixels(fsdf_ctx* ctx, int32_t* pixels_out /* [n], caller order, or NULL */, int64_t* n_out);

/* ---- free space ------------------------------------------------------------------
 * A resident point is a surface observation: Σ ρ(d*) pulls the nearest model
 * surface onto it. A depth pixel also says that the ray up to its return is
 * empty, and nothing above sees that: a body in front of what the camera saw,
 * nearest to no observed point, has zero gradient. A FREE-SPACE SAMPLE is a
 * position known to be empty, penalised only where the model covers it.
 *
 * The objective. The resident cloud may be split in the CALLER'S order: points
 * [0, n_surface) are surface observations as above, points [n_surface, n) are
 * free-space samples. With the gate g = (d* < 0) a sample's terms are
 * ρ -> g ? ρ(d*) : 0 and w -> g ? w(d*) : 0 under the context's loss, times the
 * point's weight a when weights are set; from there the sums are those of the
 * two sections above (a ρ, aw, 2 (aw d*) v, Σ aw v vᵀ, Σ aw). Under
 * FSDF_LOSS_SQUARE the samples' cost is Σ min(d*, 0)², which is C¹; its
 * Gauss-Newton moments are those of the active set. A gated-out sample stays in
 * the sums as zero terms, exactly as a weight-0 point does: the summation order
 * remains a function of the cloud layout alone, and the results are the bits of
 * the weighted reduction given weights a · g. The reduction (csrc/robust.hip,
 * its ONE_SIDED instantiations; the gate: csrc/robust_impl.h) reads the
 * cloud's resident-to-caller permutation: resident point i is a sample iff
 * permutation[i] >= n_surface (no permutation: i). Nothing is gathered and
 * nothing goes stale across fsdf_regroup_points. The pass kernels are not
 * involved.
 *
 * fsdf_set_free_split: 0 <= n_surface <= n of the resident cloud (beyond:
 * FSDF_ERR_ARG, the earlier split stays). n_surface == n or a negative value
 * clears it. The split belongs to the resident cloud like the weights: every
 * call that makes another cloud resident clears it (fsdf_set_points, _device,
 * _prefetched, _range*, _keyed_device, and a depth frame, which sets its own,
 * below). On a ranged or keyed cloud it is FSDF_ERR_STATE. fsdf_get_free_split:
 * *n_surface_out (n when none is set) and *set_out; either may be NULL.
 *
 * With a split set, on a hull-only rigid scene: fsdf_eval_robust,
 * fsdf_value_and_gradient and fsdf_value_gradient_hessian evaluate the split
 * objective through the robust path, also under FSDF_LOSS_SQUARE and without
 * weights; fsdf_descend and fsdf_descend_lm inherit it through their host
 * loops. The refusals are the loss's and name the split: a scene with an RBF
 * skin or a deformation is FSDF_ERR_STATE; the device loops do not serve it
 * (fsdf_set_solver 1 / 3 and fsdf_set_lm_solver 1 take the host loop, the
 * required modes return FSDF_ERR_STATE). The least-squares calls listed above
 * ignore it. With no split every call returns the bits it returned before.
 *
 * Samples from a depth frame. fsdf_set_free_space: a context setting like the
 * sensor and the loss, kept over frames. samples = J in 0..16 per sending pixel
 * (0: off; stride and lengths are then ignored), stride >= 1, lengths = {gap,
 * spacing, miss_range}, each finite and >= 0, spacing > 0 when J > 1; anything
 * else is FSDF_ERR_ARG and the earlier setting stays. fsdf_get_free_space reads
 * it back (any output may be NULL). With J > 0 every fsdf_set_depth_* makes
 * resident the observed points FOLLOWED BY the samples, and sets the split
 * itself to n_surface = the number of valid pixels. Per pixel i = row·cols +
 * col with row % stride == 0 and col % stride == 0, in this operation order and
 * uncontracted (s and valid as in "depth frames"):
 *   L = s − gap                for a valid pixel;
 *   L = miss_range             for a miss when miss_range > 0 — a pixel that is
 *                              not valid and not too near, !(s > 0 && s < near):
 *                              NaN, <= 0, beyond far, +inf;
 *   otherwise the pixel sends nothing.
 *   The pixel sends all J samples iff L − (double)(J − 1)·spacing > 0, else none.
 *   Sample j = 1..J: t = L − (double)(j − 1)·spacing along the pixel's direction u,
 *   c = (t·u_x, t·u_y, t·u_z), p_k = ((R_k0·c_x + R_k1·c_y) + R_k2·c_z) + t_k.
 * For FSDF_DEPTH_Z sensors t, gap, spacing and miss_range are in z units; the
 * point is on the ray either way. The caller order of the samples is j-major,
 * then pixel row-major: with m sending pixels, sample j of the r-th sending
 * pixel is caller point n_surface + (j − 1)·m + r. fsdf_get_depth_pixels
 * returns the pixel of every one of the n points, samples included, so
 * per-pixel confidences work through fsdf_set_point_weights with one weight per
 * resident point. flash/depthsensors.py free_space_points restates the
 * arithmetic: the same bits. The ingest is the depth frame's (csrc/depth.hip):
 * the count, the scan and the scatter with a second predicate and a second
 * total, both totals read back in the frame's one sizing synchronisation, and
 * the combined cloud goes through the path of fsdf_set_points_device as before.
 * More than 2^31 − 1 points in all is FSDF_ERR_ARG before anything resident is
 * replaced. With J = 0 a depth frame runs the launches it ran before.
 *
 * The solver loops' n_points divisor is the caller's as before: for a frame it
 * is the resident point count, samples included.
 *
 * Not done: the device solver loops with a split; RBF or deformable scenes;
 * ranged, keyed or sharded free-space frames; a prefetched depth frame; samples
 * whose count varies per pixel; a visibility (model-to-image) term, which would
 * need the raycaster inside the loop. */
int fsdf_set_free_split(fsdf_ctx* ctx, int64_t n_surface);
int fsdf_get_free_split(const fsdf_ctx* ctx, int64_t* n_surface_out, int32_t* set_out);
int fsdf_set_free_space(fsdf_ctx* ctx, int32_t samples /* J, 0..16; 0 = off */, int32_t stride /* >= 1 */,
                        const double* lengths /* [3]: gap >= 0, spacing > 0, miss_range >= 0 */);
int fsdf_get_free_space(const fsdf_ctx* ctx, int32_t* samples_out, int32_t* stride_out, double* lengths_out /* [3] */);

/* ---- voxel grid ------------------------------------------------------------------
 * A depth frame is hundreds of thousands of points, 2-4 mm apart at 1-2 m
 * range: far denser than the scale the model's geometry varies on, and a
 * frame's cost is its point count times the solver's iterations. A voxel grid
 * thins the cloud before the solver sees it: one centroid per occupied cell,
 * and the cell's population as that point's weight, so that Σ a ρ(d*) over the
 * centroids approximates the full frame's objective at an even spatial density.
 * The stage runs on the device (csrc/voxel.hip) ahead of the path of
 * fsdf_set_points_device; the pass and the solver kernels are not involved.
 *
 * The definition (flash/depthdata.py voxel_downsample restates it operation for
 * operation: the same bits). The grid has a cell size h (finite, > 0) and an
 * origin o (3 finite doubles); it is anchored in the world, so cells do not
 * move from frame to frame. All arithmetic is fp64 in every context precision
 * and uncontracted. Per point and axis:
 *   q = floor((x − o) / h)          (the division correctly rounded)
 *   c = q clamped to [−2^20, 2^20 − 1], as int32
 *   key = (c_z + 2^20) << 42 | (c_y + 2^20) << 21 | (c_x + 2^20)      (63 bits)
 * A point with a non-finite coordinate belongs to no voxel: it is dropped and
 * counted (its key is all ones). Voxels are ordered by ascending key — the
 * CALLER ORDER of the downsampled cloud — and within a voxel the points stay in
 * ascending input index (a stable sort). A voxel's centroid is, per coordinate,
 * the left fold in that order, acc = p_first; acc = acc + p_next; ..., then
 * acc / (double)count: no floating-point atomics and no tree whose shape
 * depends on the launch geometry, so the result is a function of the input
 * array alone, the same from run to run. The fold runs on one lane per voxel
 * and is linear in the largest cell's population (a few to a few dozen points
 * on camera data).
 *
 * fsdf_set_voxel_grid: a context setting like the sensor and the free-space
 * setting, kept over frames and model swaps. size 0 turns it off (origin and
 * weights are then ignored); origin NULL is (0, 0, 0); weights FSDF_VOXEL_COUNT
 * or FSDF_VOXEL_UNIT. A size that is negative or not finite, an origin entry
 * that is not finite or an unknown mode is FSDF_ERR_ARG and the earlier setting
 * stays. fsdf_set_voxel_grid_ref is the same with the size read through a
 * pointer (NULL reads as 0), for bindings that pass every floating-point
 * argument by reference (julia/FlashSDF.jl). fsdf_get_voxel_grid reads the
 * setting back; any output may be NULL.
 *
 * fsdf_set_points_voxel / _device: xyz [n][3] fp64 (host / device) is
 * downsampled, and the centroids [m][3] then take exactly the path of
 * fsdf_set_points_device. Under FSDF_VOXEL_COUNT the point weights are then set
 * to (double)count through the path of fsdf_set_point_weights_device (so the
 * robust reduction serves the objective, also under FSDF_LOSS_SQUARE); under
 * FSDF_VOXEL_UNIT no weights are set. With no grid set: FSDF_ERR_STATE.
 * n >= 2^31: FSDF_ERR_ARG. n == 0, or every point dropped, makes a cloud of 0
 * points resident: not an error. Synchronous like fsdf_set_points. It costs one
 * sizing synchronisation, for m and the number dropped. fsdf_set_points,
 * _device, _prefetched, _range* and _keyed_device ignore the grid, and each
 * ends a voxel cloud's lists as it ends a depth frame's pixel list.
 *
 * Depth frames. With a grid set, every fsdf_set_depth_* downsamples its
 * observed points (the valid pixels' points, in pixel order) between the
 * scatter and the path of fsdf_set_points_device: one more sizing
 * synchronisation per frame. With free-space samples configured the samples
 * follow the centroids unchanged, the split is set to m, and under
 * FSDF_VOXEL_COUNT the weights are the counts followed by 1.0 per sample.
 * fsdf_get_depth_pixels returns, for a voxel, the pixel of its first point (the
 * lowest pixel index in the cell) and the samples' pixels as before. With
 * size 0 a frame runs the launches it ran before and returns the bits it
 * returned before.
 *
 * fsdf_get_voxels: of the resident voxel cloud, xyz_out [m][3] the centroids,
 * count_out [m], cell_out [m][3] the cells (c_x, c_y, c_z), all in caller
 * order; *m_out, *n_in_out the number of input points (a depth frame: of valid
 * pixels), *dropped_out of dropped ones. Any pointer may be NULL (read m first).
 * fsdf_get_voxel_of_point: out[i] = the caller index of input point i's voxel,
 * −1 for a dropped point; out may be NULL to read n_in alone. Both return
 * FSDF_ERR_STATE when the resident cloud did not come through the grid.
 * Synchronous.
 *
 * A later fsdf_set_point_weights replaces the counts, as with any weights; the
 * caller who wants both multiplies by count_out. The solver loops' n_points
 * divisor is the caller's as before.
 *
 * Not done: prefetched, ranged, keyed and sharded voxel clouds; centroids
 * weighted by caller weights (weights are set after the cloud); voxelised
 * free-space samples (their stride thins them); a parallel fold for a cell
 * with very many points (the one-lane fold's worst case is the whole cloud in
 * one cell). */
enum { FSDF_VOXEL_UNIT = 0, FSDF_VOXEL_COUNT = 1 };
int fsdf_set_voxel_grid(fsdf_ctx* ctx, double size /* 0 = off */, const double* origin /* [3] or NULL */,
                        int32_t weights);
int fsdf_set_voxel_grid_ref(fsdf_ctx* ctx, const double* size, const double* origin /* [3] or NULL */,
                            int32_t weights);
int fsdf_get_voxel_grid(const fsdf_ctx* ctx, double* size_out, double* origin_out /* [3] */, int32_t* weights_out);
int fsdf_set_points_voxel(fsdf_ctx* ctx, const double* xyz, int64_t n);
int fsdf_set_points_voxel_device(fsdf_ctx* ctx, const double* d_xyz, int64_t n);
int fsdf_get_voxels(fsdf_ctx* ctx, double* xyz_out /* [m][3] */, int32_t* count_out /* [m] */,
                    int32_t* cell_out /* [m][3] */, int64_t* m_out, int64_t* n_in_out, int64_t* dropped_out);
int fsdf_get_voxel_of_point(fsdf_ctx* ctx, int32_t* out /* [n_in] or NULL */, int64_t* n_in_out);

/* ---- Gauss-Newton for RBF skins: device side -----------------------------------
 * The skins' second moments M_r above, reduced on the device
 * (csrc/skin_moments.hip): a launch of its own after the pass — the pass
 * kernels are unchanged — over the resident points, the pass's k* in resident
 * order and the current RBF rows. Every workgroup owns one 64x64 block pair
 * (bi <= bj) of one skin's matrix and a fixed run of 64-point chunks; it
 * recomputes the field, forms the chunk's rows in LDS (zero for points nearest
 * to another surface) and adds JᵀJ on the fp64 matrix unit; the finish launch
 * sums the workgroups' partial blocks in workgroup order and mirrors the upper
 * block pairs. No floating-point atomics: for a given cloud layout the moments
 * are bit-identical from run to run, and exactly symmetric. All arithmetic is
 * fp64 (fp32 contexts: their fp32 points and rows, widened). Skins of up to 124
 * centres (n + 4 <= 128, fsdf_set_solver's own limit) are served; a larger one
 * is FSDF_ERR_STATE. The grid and the partials' memory are functions of the
 * point count and the skins' centre counts alone: 32 KB per workgroup, at most
 * 1,024 workgroups' worth — 32 MB per context (beyond, a workgroup's run
 * grows instead).
 *
 * fsdf_eval_skin_moments: fsdf_eval's pass over the resident cloud plus the
 * skins' moments at the rows of the last fsdf_set_rbf_params; moments_out holds
 * Σ_r m_r^2 doubles, the skins' [m_r][m_r] matrices one after the other in
 * surface order (required; cost_out, accum_out may be NULL). Synchronous; needs
 * no mechanism. Replaces forming Σ j jᵀ on the host from per-point outputs. A
 * cloud of no points, or with no point on a skin, gives that skin exact zeros;
 * a scene without a skin is FSDF_ERR_STATE.
 *
 * fsdf_set_lm_skins: enable = 0 (the default) leaves every refusal above as it
 * is. With enable = 1 the second-order solver serves scenes with RBF skins and
 * deformations: fsdf_value_gradient_hessian returns hess_out [nx][nx], nx =
 * nq + 3 n_deform, the H above (the hulls' moments, the skins' moments, one
 * fsdf_rbf_state_map and fsdf_gauss_newton_add per skin, the regulariser's
 * 2 weight on the deformations' diagonal), cost_out and grad_out [nx]
 * bit-identical to fsdf_value_and_gradient's; fsdf_descend_lm runs its host
 * loop over the nx coordinates and fsdf_set_lm_prior expects n = nx;
 * fsdf_set_lm_solver 1 takes the host loop for such scenes and 2 refuses them
 * (FSDF_ERR_STATE: the device loop serves rigid scenes). Skins not all declared
 * or a deformation row out of range fail as in fsdf_value_and_gradient. Rigid
 * scenes are served as before, whatever the switch. */
int fsdf_set_lm_skins(fsdf_ctx* ctx, int32_t enable);
int fsdf_eval_skin_moments(fsdf_ctx* ctx, const double* poses, double* cost_out, double* accum_out,
                           double* moments_out);

/* ---- robust objectives on skins --------------------------------------------------
 * Robust losses, per-point weights and the free-space split above serve
 * hull-only rigid scenes. fsdf_set_robust_skins (a context setting like
 * fsdf_set_lm_skins; enable = 0, the default, leaves every refusal above as it
 * is — the same status, message and bits) opens them to scenes with RBF skins
 * and deformations: with enable = 1 the robust objective Σ a ρ(d*) (a loss
 * other than SQUARE, weights, or a split) is served by
 * fsdf_value_and_gradient and the host loop of fsdf_descend, and — with
 * fsdf_set_lm_skins(1) as well — by fsdf_value_gradient_hessian and the host
 * loop of fsdf_descend_lm. The required device loops (fsdf_set_solver 2 / 4,
 * fsdf_set_lm_solver 2), ranged and keyed clouds, and skins of more than 124
 * centres for the Hessian are refused as before; fsdf_set_solver 1 / 3 and
 * fsdf_set_lm_solver 1 run the host loop.
 *
 * A skin's block of the accumulator is Σ 2 s j(p), j the point's row of
 * ∂s/∂(w, a, b, c); the robust objective needs Σ 2 (aw d*) j and, for the
 * Gauss-Newton term, Σ aw j jᵀ, with aw = a · w(d*), w = ρ′/2d, a through the
 * one-sided gate when a split is set. Both are launches of their own after
 * the pass (csrc/robust_skin.hip; csrc/skin_moments.hip's factor variant),
 * from the pass's k* and d* in resident order and the current RBF rows; the
 * point's factor is formed in fp64 exactly as the hulls' reduction forms it,
 * and stands in the pass's own arithmetic (the context's precision) where 2s
 * does — with a ≡ 1 under SQUARE a point's summands are the pass's, only the
 * order of summation differs. No floating-point atomics: for a given cloud
 * layout the results are bit-identical from run to run. The regulariser's
 * 2 · weight on the deformations is not robustified.
 *
 * fsdf_eval_robust_skins (needs the switch; fsdf_eval_robust itself keeps
 * refusing skins): one pass at the rows of the last fsdf_set_rbf_params.
 * accum_out: fsdf_eval's full layout [1 + 6S + Σ(4n+4)] — the cost Σρ summed
 * in surface order from 0.0, a hull's robust wrench, a skin surface's six
 * wrench entries 0.0 (as the pass leaves them), then the skins' robust
 * blocks. moments_out: NULL or [S][21], a skin surface's row zero.
 * skin_moments_out: NULL, or the skins' m×m matrices Σ aw j jᵀ in
 * fsdf_eval_skin_moments' layout. weight_out: NULL or [S], Σ aw. A cloud of
 * no points gives zeros and launches nothing. */
int fsdf_set_robust_skins(fsdf_ctx* ctx, int32_t enable);
int fsdf_get_robust_skins(const fsdf_ctx* ctx, int32_t* enable_out);
int fsdf_eval_robust_skins(fsdf_ctx* ctx, const double* poses, double* cost_out, double* accum_out,
                           double* moments_out, double* skin_moments_out, double* weight_out);

/* ---- robust objectives on the device solver loops ----------------------------------
 * With a robust objective (a loss other than SQUARE, point weights, or a free
 * split) the solver loops above run on the host: fsdf_set_solver 1 and
 * fsdf_set_lm_solver 1 take the host loop, the required modes are refused.
 * fsdf_set_robust_loops (a context setting like fsdf_set_robust_skins;
 * enable = 0, the default, leaves every such answer as it is — the same
 * status, message and bits; other values than 0 / 1 are FSDF_ERR_ARG) admits
 * the robust objective to the device-resident loops of fsdf_descend and
 * fsdf_descend_lm on hull-only rigid scenes of at most 282 surfaces. What
 * fsdf_set_solver and fsdf_set_lm_solver say is unchanged — where the loop
 * runs; this switch says whether a robust objective may run there. With
 * enable = 1: modes 1 take the device loop where it fits (resident points, the
 * solver kernels' LDS, for LM a damping > 0) and the host loop otherwise; the
 * required modes (fsdf_set_solver 2, fsdf_set_lm_solver 2) succeed where it
 * fits and answer FSDF_ERR_STATE with the reason where it does not. Scenes
 * with RBF skins or deformations (fsdf_set_robust_skins, fsdf_set_solver
 * 3 / 4) keep the host loop under a robust objective and their required modes
 * stay refused: the robust device loops do not serve them.
 *
 * Per evaluation the pass writes k*, d* and ∇d* in resident order, the robust
 * launch (csrc/robust.hip) reduces them per surface, an assembly launch forms
 * the accumulator [1 + 6S] (Σρ summed over the surfaces in ascending order
 * from 0.0) and the moments [S][21] from the rows on the device — the
 * arithmetic the host does after its read-back — and the unchanged step
 * kernels read those. All three return at once on the evaluations a finished
 * frame still has queued. After the first evaluation's regroup the loop reads
 * the regrouped layout's permutation and weights, as the host loop's second
 * evaluation does. x, the value, the evaluation count and the final damping
 * are bit-identical to the host loop's on the same context state.
 *
 * fsdf_eval_robust_device: the asynchronous twin of fsdf_eval_robust, as
 * fsdf_eval_device is of fsdf_eval, and needs no switch. The pass, the robust
 * launch and the assembly are enqueued on the context stream and the call
 * returns: d_accum [1 + 6S] and d_moments [S][21] (NULL: the rows of 8, no
 * moments) are device memory, fsdf_eval_robust's accum_out and moments_out bit
 * for bit once the stream reaches them. Hull-only scenes (an RBF skin or a
 * deformation: FSDF_ERR_STATE); a cloud of no points gives zeros. It never
 * regroups. */
int fsdf_set_robust_loops(fsdf_ctx* ctx, int32_t enable);
int fsdf_get_robust_loops(const fsdf_ctx* ctx, int32_t* enable_out);
int fsdf_eval_robust_device(fsdf_ctx* ctx, const double* poses, double* d_accum /* [1 + 6S], device */,
                            double* d_moments /* [S][21], device, or NULL */);

/* ---- scoring candidate states ------------------------------------------------------
 * Every call that estimates a state needs a start in the right basin. To find
 * one — a tracker's first state, or its state again after an occlusion — a
 * caller compares many candidates, and B calls of fsdf_eval_robust cost B times
 * the fixed price of a pass (pose, pass, robust launch, reduce, read-back) on a
 * cloud small enough that the price is nearly all there is. These calls score
 * B candidates against the resident cloud at once: one pose launch over
 * (item x candidate), one score launch over (chunk group x candidate), one
 * small launch that sums each candidate's partial sums (csrc/score.hip); a
 * large batch runs in slices of a fixed byte budget of posed models.
 *
 * cost_out[b] is the objective fsdf_eval_robust puts into accum_out[0] at
 * candidate b's poses — Σ_i a_i ρ(d*(p_i)) under the context's loss
 * (FSDF_LOSS_SQUARE: d*²), per-point weights (1.0 without) and free-space split
 * (a sample counts only where d* < 0) — as a sum, not a mean, with neither the
 * prior of fsdf_set_lm_prior nor a regulariser in it. d* is the pass's, bit for
 * bit; the terms are formed and summed in fp64 (an fp32 context's d* widened as
 * stored) in an order that depends on the cloud's size and layout alone: no
 * floating-point atomics, and candidate b's bits depend neither on B, nor on
 * its place in the batch, nor on the slicing. Against fsdf_eval_robust the
 * cost differs by summation order only (both sum the same terms).
 *
 * fsdf_score_poses: poses [B][S][12], each as fsdf_eval's. fsdf_score_states:
 * x [B][nq] after fsdf_set_mechanism — the host forward kinematics and surface
 * poses of fsdf_value_and_gradient at each x (quaternion blocks normalised),
 * then the same path; a configuration the kinematics refuses fails the call.
 * Both are synchronous. B = 0 is FSDF_OK and writes nothing; a cloud of no
 * points gives exact zeros; a candidate with a non-finite pose entry gets a NaN
 * cost and the others theirs. NULL arguments and B < 0 are FSDF_ERR_ARG.
 * FSDF_ERR_STATE: no model, no cloud, no mechanism (fsdf_score_states), a
 * scene with an RBF skin or a deformation, a ranged or keyed cloud, a
 * prefetched cloud not yet made resident.
 *
 * The calls are read-only on the context: seeds, plan, block orders, regroup
 * state, loss, weights and split are as before, and any later call returns the
 * bits it returns without the scoring call.
 *
 * fsdf_score_time: with fsdf_profile_pass enabled a pair of events is recorded
 * around each scoring call's launches (up to 256 pairs between queries); this
 * synchronizes, returns their summed time and the number of calls recorded and
 * resets the record, as fsdf_skin_moments_time. */
int fsdf_score_poses(fsdf_ctx* ctx, const double* poses /* [B][S][12] */, int32_t B, double* cost_out /* [B] */);
int fsdf_score_states(fsdf_ctx* ctx, const double* x /* [B][nq] */, int32_t B, double* cost_out /* [B] */);
int fsdf_score_time(fsdf_ctx* ctx, double* total_ms_out, int64_t* launches_out);

/* ---- gradients of candidate states ------------------------------------------------
 * The scoring calls above rank B candidates; refining the kept ones is one
 * solver loop after the other, every evaluation of every candidate a pose
 * launch, a pass, a robust launch, a reduce, a read-back and a synchronisation
 * — on the thinned clouds multi-start runs on, nearly all fixed cost. These
 * calls give (f, g, H) at B states of the resident cloud at once, and run the
 * two solver loops over a batch in lockstep with one synchronisation per round
 * for the whole batch (csrc/batch.hip, csrc/batch_api.hip).
 *
 * Per candidate b the device forms the rows fsdf_eval_robust reduces at b's
 * poses — per surface the 21 moments, the wrench, Σρ and Σw (or the last 8
 * alone when no moments are asked for) — under the context's loss
 * (FSDF_LOSS_SQUARE too), per-point weights and free-space split, over the
 * resident cloud in resident order: one pose launch over (item x candidate)
 * into the scoring calls' posed tables, one evaluation launch over (chunk group
 * x candidate) that writes k*, d* and ∇d* per (candidate, point) — 36 bytes —
 * into a slice buffer, then fsdf_eval_robust's own reduction, statement for
 * statement, with the candidate on the grid's second dimension. A large batch
 * runs in slices of a fixed byte budget (tables, per-point blocks, partials,
 * rows; the environment variable FSDF_BATCH_SLICE_BYTES overrides it; at least
 * one candidate a slice). Candidate b's rows are bit-identical to the rows
 * fsdf_eval_robust returns at the same poses on the same cloud layout, and
 * depend neither on B, nor on b's place in the batch, nor on the slicing. No
 * floating-point atomics.
 *
 * fsdf_batch_robust_poses: poses [B][S][12] -> accum_out [B][1 + 6S], the
 * accumulator of fsdf_eval_robust per candidate ([0] Σρ summed over the
 * surfaces in ascending order from 0.0, then the wrenches); moments_out
 * [B][S][21] and weight_out [B][S] (Σw per surface) may be NULL.
 *
 * fsdf_batch_states: x [B][nq] after fsdf_set_mechanism -> cost_out [B],
 * grad_out [B][nq], hess_out [B][nq][nq] (may be NULL). Per candidate the host
 * forward kinematics of fsdf_score_states, then on its accumulator and moments
 * the chain rule and the Gauss-Newton matrix (factor 2) of
 * fsdf_value_and_gradient / fsdf_value_gradient_hessian under a robust
 * objective — the same (c, g, H) bits as those calls at x on the same layout
 * (they may regroup the cloud: compare with FSDF_REGROUP_OFF). hess_out NULL
 * reduces the rows of 8 and gives the same (c, g) bits.
 *
 * fsdf_descend_lm_batch: fsdf_lm_minimize's loop for B candidates in lockstep
 * over fsdf_descend_lm's objective — cost / n_points and the prior of
 * fsdf_set_lm_prior about each candidate's own start x[b] —, one
 * fsdf_batch_states per round over the candidates still running, in ascending
 * index order. x [B][nq] is updated in place; value_out [B], iterations_out [B]
 * (evaluations made) and damping_out [B] as fsdf_lm_minimize's, per candidate,
 * and bit-identical to it over fsdf_batch_states of a single state.
 * fsdf_descend_batch: the same for the NaiveSolver rule of fsdf_descend's host
 * loop (divisors [nq] or NULL, shared by the candidates). fsdf_set_solver,
 * fsdf_set_lm_solver and fsdf_set_robust_loops do not apply: both are host
 * loops around a batched device evaluation.
 *
 * All are synchronous and read-only on the context, as the scoring calls:
 * seeds, plan, block orders, regroup state, loss, weights, split and the
 * record of prepared states stay as they are. B = 0 is FSDF_OK and writes
 * nothing; a cloud of no points gives exact zeros; a candidate with a
 * non-finite pose entry gets NaN outputs — on a cloud of no points too — and
 * the others theirs (in the loops
 * it runs on as under a callback that returns those NaNs). NULL arguments and
 * B < 0 are FSDF_ERR_ARG. FSDF_ERR_STATE: no model, no cloud, no mechanism
 * (all but fsdf_batch_robust_poses), a scene with an RBF skin or a
 * deformation, a ranged or keyed cloud, a prefetched cloud not yet made
 * resident, more surfaces than the robust table holds. A configuration the
 * kinematics refuses fails the call.
 *
 * fsdf_descend_lm_batch_ref / fsdf_descend_batch_ref: the two loops with every
 * floating-point scalar read through a pointer, for bindings that pass them by
 * reference (julia/FlashSDF.jl), as fsdf_set_loss_ref: params [4] = (damping,
 * max_step, tolerance, n_points), respectively (rate, max_step, tolerance,
 * n_points); NULL params is FSDF_ERR_ARG; everything else as the call it names.
 *
 * fsdf_batch_time: as fsdf_score_time, for the device work of these calls, with
 * a pair of events around every slice's launches: launches_out counts the
 * slices run (one per call unless the byte budget split its batch). */
int fsdf_batch_robust_poses(fsdf_ctx* ctx, const double* poses /* [B][S][12] */, int32_t B,
                            double* accum_out /* [B][1+6S] */, double* moments_out /* [B][S][21] or NULL */,
                            double* weight_out /* [B][S] or NULL */);
int fsdf_batch_states(fsdf_ctx* ctx, const double* x /* [B][nq] */, int32_t B, double* cost_out /* [B] */,
                      double* grad_out /* [B][nq] */, double* hess_out /* [B][nq][nq] or NULL */);
int fsdf_descend_lm_batch(fsdf_ctx* ctx, double* x /* [B][nq] */, int32_t B, int32_t iteration_limit, double damping,
                          double max_step, double tolerance, double n_points, double* value_out,
                          int32_t* iterations_out, double* damping_out);
int fsdf_descend_batch(fsdf_ctx* ctx, double* x /* [B][nq] */, int32_t B, int32_t iteration_limit, double rate,
                       double max_step, double tolerance, const double* divisors, double n_points, double* value_out,
                       int32_t* iterations_out);
int fsdf_descend_lm_batch_ref(fsdf_ctx* ctx, double* x /* [B][nq] */, int32_t B, int32_t iteration_limit,
                              const double* params /* [4] */, double* value_out, int32_t* iterations_out,
                              double* damping_out);
int fsdf_descend_batch_ref(fsdf_ctx* ctx, double* x /* [B][nq] */, int32_t B, int32_t iteration_limit,
                           const double* params /* [4] */, const double* divisors, double* value_out,
                           int32_t* iterations_out);
int fsdf_batch_time(fsdf_ctx* ctx, double* total_ms_out, int64_t* launches_out);

/* ---- context ---------------------------------------------------------------- */
int fsdf_create(fsdf_ctx** out, const fsdf_opts* opts);
int fsdf_destroy(fsdf_ctx* ctx);
const char* fsdf_last_error(const fsdf_ctx* ctx);
/* Launch on a caller-owned hipStream_t (NULL = the context's own stream;
 * FSDF_HIP_NULL_STREAM = HIP's null/default stream, the handle 0 that e.g.
 * torch's default stream reports). */
#define FSDF_HIP_NULL_STREAM ((void*)(intptr_t)-1)
int fsdf_set_stream(fsdf_ctx* ctx, void* hip_stream);
int fsdf_num_hulls(const fsdf_ctx* ctx, int32_t* k_out);
int fsdf_accum_len(const fsdf_ctx* ctx, int32_t* len_out); /* 1 + 6K + Σ(4n+4) */

/* Upload the model once (per model). Replaces the per-evaluation
 * CollisionCache construction of src/Flash.jl:246. fsdf_set_model is the
 * hull-only form of fsdf_set_surfaces. */
int fsdf_set_model(fsdf_ctx* ctx, const fsdf_hull* hulls, int32_t n_hulls);
int fsdf_set_surfaces(fsdf_ctx* ctx, const fsdf_surface* surfaces, int32_t n_surfaces);

/* Per-pass RBF parameters (before fsdf_eval / fsdf_skin when the scene has RBF
 * surfaces): for every RBF surface in surface order, n_centers rows
 * (c_x, c_y, c_z, w) in the world frame, then one row (a, b_x, b_y, b_z).
 * n_doubles must equal 4·Σ(n_centers + 1). The host solves the (n+4)² system
 * [A P; Pᵀ 0][w; a; b] = [v; 0] (surface points v = 0, skeleton v = -1). */
int fsdf_set_rbf_params(fsdf_ctx* ctx, const double* params, int64_t n_doubles);

/* Upload the sensed cloud once per frame (src/gradientdescent.jl:43 holds it
 * by reference across every cost evaluation). A sorting hull-only context
 * seeds the new cloud's first pass from the previous cloud's last nearest
 * surfaces (a voxel grid over the first cloud's box, grown by half its extent;
 * seeds order the search only — results do not depend on them). */
int fsdf_set_points(fsdf_ctx* ctx, const double* xyz, int64_t n);
/* Same, from a device-resident AoS buffer (copied device-to-device). */
int fsdf_set_points_device(fsdf_ctx* ctx, const double* d_xyz, int64_t n);
/* The next frame's cloud ahead of time (a frame loop over recorded or queued
 * clouds, src/gradientdescent.jl:43 once per frame): fsdf_prefetch_points
 * queues its host-to-device copy on a stream of the context's own and returns
 * at once; the copy is issued right after the context's next pass is launched
 * (or by fsdf_set_points_prefetched when no pass comes between), so it runs
 * during the current frame's passes (overlapped from page-locked memory; the
 * caller keeps xyz unchanged until the next call below returns; a second
 * prefetch replaces a pending one);
 * fsdf_set_points_prefetched then makes it resident as fsdf_set_points would
 * (FSDF_ERR_STATE when nothing is pending). A sorting context also Hilbert-
 * sorts the prefetched cloud on that stream, into a second resident buffer set,
 * so fsdf_set_points_prefetched only swaps buffers. fsdf_set_points meanwhile
 * leaves a pending prefetch pending. */
int fsdf_prefetch_points(fsdf_ctx* ctx, const double* xyz, int64_t n);
int fsdf_set_points_prefetched(fsdf_ctx* ctx);
/* One rank's shard of a cloud split over several devices (the
 * cost is a plain sum over points, src/gradientdescent.jl:32): the whole
 * n-point cloud is uploaded and ordered (the Hilbert order with sort_points,
 * else the caller's), and positions [begin, end) of that order stay resident —
 * a contiguous region of space, so the shard keeps the whole cloud's point
 * density per 64-point chunk (a slice of an arbitrary order would scatter each
 * rank's points over the whole scene). Every rank of a job passes the same
 * cloud and its own range; the ranges partition [0, n). Per-point outputs of a
 * ranged cloud are always in its resident order, and fsdf_get_permutation names
 * each resident point's index in the whole cloud. fsdf_chunk_costs then reports
 * the range's chunks — the chunks of the whole cloud's order when begin is a
 * multiple of 64 — which is what flash.distributed balances the ranges by; once
 * the range has been regrouped (fsdf_regroup_points) its chunks are no longer
 * the whole cloud's and fsdf_chunk_costs refuses (FSDF_ERR_STATE) until the
 * next set_points. */
int fsdf_set_points_range(fsdf_ctx* ctx, const double* xyz, int64_t n, int64_t begin, int64_t end);
int fsdf_set_points_range_device(fsdf_ctx* ctx, const double* d_xyz, int64_t n, int64_t begin, int64_t end);
int fsdf_num_points(const fsdf_ctx* ctx, int64_t* n_out);
/* Spatial shards with O(N/W) ingest per rank (flash.distributed.exchange_points):
 * each rank uploads only its 1/W slice of the sensed cloud; the ranks agree on
 * the whole cloud's bounding box (fsdf_cloud_box_device of each slice, then a
 * 6-double all-reduce), compute each point's 30-bit Hilbert key in it
 * (fsdf_curve_keys_device: the keys fsdf_set_points orders by), split the key
 * range into W contiguous ranges from an all-reduced key histogram, move every
 * point to the rank owning its key over one all-to-all, and each rank makes its
 * received points resident (fsdf_set_points_keyed_device): ordered by (key,
 * whole-cloud index) — exactly the whole cloud's sorted order restricted to its
 * key range — with the whole-cloud indices as the permutation (FSDF_ORDER_RESIDENT
 * outputs, like fsdf_set_points_range; indices < 2^31). Per-point results are
 * those of a single context over the whole cloud, bit for bit. box: host
 * [6] = (lo xyz, hi xyz); all calls synchronous. */
int fsdf_cloud_box_device(fsdf_ctx* ctx, const double* d_xyz, int64_t n, double* box_out);
int fsdf_curve_keys_device(fsdf_ctx* ctx, const double* d_xyz, int64_t n, const double* box, uint32_t* d_keys);
int fsdf_set_points_keyed_device(fsdf_ctx* ctx, const double* d_xyz, const uint32_t* d_keys, const int64_t* d_index,
                                 int64_t n);
/* Regroup the resident cloud by each point's nearest surface in the last pass
 * over it, keeping the current (Hilbert) order within each surface's group: a
 * stable device sort, once per frame after its first pass. The reference has no
 * counterpart — its track! loop (src/tracking.jl:8-27) evaluates the cost of
 * one frame's cloud over and over (src/gradientdescent.jl:43), which is what
 * this exploits: the passes seed each point from its last nearest surface, and
 * a 64-point chunk whose points share one evaluates fewer hulls. Per-point
 * results are unchanged; the cost and wrench sums change in rounding only (the
 * chunks group other points). It pays where the pass is bound by its summed
 * work — the one-wave grid of clouds above the planned window — and costs where
 * the planned pass is bound by its heaviest chunk, which grouping makes heavier
 * (DESIGN.md §7 round 5). The resident order changes: re-read
 * fsdf_get_permutation for FSDF_ORDER_RESIDENT outputs. Requires a sorted
 * (sort_points) or ranged cloud and a pass over that very cloud (hull-only
 * scenes of <= 64 surfaces): FSDF_ERR_STATE, with the resident order unchanged,
 * before the first pass since the cloud was set — also when that cloud's first
 * pass will be seeded from the previous cloud (the carried seeds are hints, not
 * this cloud's nearest surfaces). Asynchronous on the context stream. */
int fsdf_regroup_points(fsdf_ctx* ctx);
/* The regroup where it pays, decided by the library: only after a pass that
 * ran one wave per chunk (the grid above the planned window, bound by its
 * summed work), on a sorted or ranged cloud not yet regrouped since its
 * set_points. *applied_out = 1 when it regrouped (NULL allowed).
 * fsdf_set_regroup: FSDF_REGROUP_AUTO (default) — the iteration entry points
 * that return no per-point outputs (fsdf_value_and_gradient,
 * fsdf_eval_state_device, fsdf_descend) apply this rule after a new cloud's
 * first pass, so track! frames regroup by themselves; FSDF_REGROUP_OFF — only
 * explicit calls regroup. fsdf_eval / fsdf_eval_device never regroup on their
 * own (their resident-order outputs index the permutation of the pass). */
#define FSDF_REGROUP_OFF 0
#define FSDF_REGROUP_AUTO 1
int fsdf_regroup_auto(fsdf_ctx* ctx, int32_t* applied_out);
int fsdf_set_regroup(fsdf_ctx* ctx, int32_t mode);

/* One residual pass over the resident cloud (synchronous, host buffers).
 * poses: [K][12] host. Outputs may be NULL when not wanted:
 *   cost_out   1 double         accum_out  1+6K doubles
 *   kstar_out  n int32          d_out      n doubles      grad_out [n][3] doubles */
int fsdf_eval(fsdf_ctx* ctx, const double* poses, double* cost_out, double* accum_out,
              int32_t* kstar_out, double* d_out, double* grad_out);

/* Same pass, asynchronous on the context stream, outputs in DEVICE memory
 * (used by the multi-GPU path: the caller all-reduces d_accum over RCCL).
 * d_accum: 1+6K doubles (required); per-point outputs may be NULL. */
int fsdf_eval_device(fsdf_ctx* ctx, const double* poses, double* d_accum,
                     int32_t* d_kstar, double* d_d, double* d_grad);

/* Scene signed distance at arbitrary query points (the closure returned by
 * Flash.skin(state), src/Flash.jl:265-268), not touching the resident cloud.
 * xyz: [n][3] host; outputs host, any may be NULL. Synchronous. */
int fsdf_skin(fsdf_ctx* ctx, const double* poses, const double* xyz, int64_t n,
              double* d_out, int32_t* kstar_out, double* grad_out);

/* Depth-sensor raycast on the scene SDF (src/depthsensors.jl:56-97, doRaycast;
 * the field is Flash.skin(state), src/depthsensors.jl:116): per ray a secant
 * march from `origin` — step = -SDF/est_grad (est_grad starts at -1, then the
 * secant slope), |step| <= 0.4, stop at |SDF| <= 1e-5 or after 60 steps;
 * depth = NaN when the final |SDF| > 1e-2. origin: 3 doubles (world);
 * rays: [n][3] unit directions (world); depth_out: n doubles. Synchronous.
 * Uses the current RBF parameters when the scene has skins. */
int fsdf_raycast(fsdf_ctx* ctx, const double* poses, const double* origin, const double* rays, int64_t n,
                 double* depth_out);

/* Order of the per-point outputs of fsdf_eval / fsdf_eval_device:
 *   FSDF_ORDER_CALLER (default): output i belongs to input point i;
 *   FSDF_ORDER_RESIDENT: output i belongs to resident point i — the device
 *     order after fsdf_opts.sort_points (Hilbert order), written with
 *     coalesced stores instead of a scatter through the permutation. Caller
 *     point perm[i] (fsdf_get_permutation) is resident point i. Without
 *     sort_points the two orders coincide. fsdf_skin always uses caller order. */
#define FSDF_ORDER_CALLER 0
#define FSDF_ORDER_RESIDENT 1
int fsdf_set_output_order(fsdf_ctx* ctx, int32_t order);
/* perm[i] = caller index of resident point i (n = fsdf_num_points int64s;
 * identity without sort_points). Host / device destination. */
int fsdf_get_permutation(fsdf_ctx* ctx, int64_t* perm_out);
int fsdf_get_permutation_device(fsdf_ctx* ctx, int64_t* d_perm_out);

/* Block until all work queued on the context stream has finished. */
int fsdf_synchronize(fsdf_ctx* ctx);

/* ---- measurement ------------------------------------------------------------
 * With profiling enabled, every residual pass stamps HIP events at the start
 * and end of the pass kernel (the dominant launch) and at the end of the
 * reduction that follows it, through the kernel dispatches themselves
 * (hipExtLaunchKernel: no event packets between the kernels, so profiling
 * leaves the step's timing alone). fsdf_pass_times synchronizes, returns the
 * summed pass-kernel time, the summed pass + reduction time of the passes
 * recorded since the last query and their count, and resets the record;
 * fsdf_pass_time returns the pass + reduction sum only. */
int fsdf_profile_pass(fsdf_ctx* ctx, int32_t enable);
int fsdf_pass_times(fsdf_ctx* ctx, double* kernel_ms_out, double* pass_ms_out, int64_t* launches_out);
int fsdf_pass_time(fsdf_ctx* ctx, double* total_ms_out, int64_t* launches_out);
/* The same for the skin moments (fsdf_eval_skin_moments, fsdf_value_gradient_hessian
 * with fsdf_set_lm_skins): with profiling enabled on a scene with RBF skins, a
 * pair of events is recorded around the skins' launches (the kernels and their
 * finish launches; up to 256 pairs between queries). fsdf_skin_moments_time
 * synchronizes, returns their summed time and count and resets the record
 * (tools/skin_moments_time.py). */
int fsdf_skin_moments_time(fsdf_ctx* ctx, double* total_ms_out, int64_t* launches_out);

/* The pass-kernel variant the context's last residual pass dispatched, as
 * rocprofv3 names it without the namespace, e.g.
 * "pass_kernel<double, 1, true, false, true, false, 256, 4>"; "" before any
 * pass. (bench.py attaches PMC counters to its roofline only when the
 * profiled kernel is this one.) */
const char* fsdf_pass_kernel_name(const fsdf_ctx* ctx);

/* ---- hull-partitioned pass tiers ---------------------------------------------
 * Small clouds leave wave slots idle while a chunk's serial hull evaluations
 * set the pass time; up to a tier's point count the pass instead runs 4 (or
 * 2) waves per 64-point chunk, each evaluating every 4th (2nd) hull, merged by
 * the first-index (d, k) minimum — bit-identical per point. The tiers apply to
 * f64 hull-only scenes of <= 64 surfaces. Defaults depend on the model (hull
 * count); fsdf_set_partition overrides them for this context:
 * -1 = the model's default, 0 = tier off, else the largest cloud (points per
 * device) the tier runs. fsdf_get_partition reports the limits in effect and
 * the waves per chunk (4, 2, 0 = one) a pass over n points would run.
 * Replaces the reference's nothing: a scheduling knob of this build. */
int fsdf_set_partition(fsdf_ctx* ctx, int64_t four_way_max_points, int64_t two_way_max_points);
int fsdf_get_partition(fsdf_ctx* ctx, int64_t n, int64_t* four_way_max_out, int64_t* two_way_max_out,
                       int32_t* parts_out);

/* ---- planned pass --------------------------------------------------------------
 * Resident-cloud passes of f64 hull-only scenes with <= 64 surfaces (the
 * metric's M64, IRB140) run a planned grid: every 64-point chunk writes its
 * own partial row (so the accumulator sums chunks in index order, bit-identical
 * whatever the plan), records its duration, and from the cloud's first pass on
 * (rebuilt every 16 passes) the heaviest chunks — `four_way_share` of them —
 * are split over 4 waves (hull-partitioned), the next `two_way_share` over 2,
 * the rest run one wave each grouped by similar cost, heaviest workgroups
 * first. enable = 0 runs the unplanned one-block-per-4-chunks grid instead
 * (A/B). Shares < 0 select the default: the heaviest 96 chunks over 4 waves
 * and the next 192 over 2; at least as many chunks go 4 ways as the device has
 * idle wave slots for (a strong-scaling shard smaller than the machine splits
 * its heaviest third). A new cloud's first pass runs the tier shape of
 * fsdf_set_partition. max_points: the largest cloud (points per device) the
 * planned pass runs, -1 = the model's default window: more than 98,304 and
 * at most 524,288 points for models of >= 32 hulls, 393,216 for smaller ones
 * (outside it the unplanned grid measured faster); a value >= 0
 * runs it for every cloud of 1 .. max_points points. Memory: the per-chunk
 * rows take (25 + 6 S) doubles per 64-point chunk per context (1.6 KB at
 * S = 64: 13 MB for the default window's 524,288 points, 105 MB at the
 * 4,194,304-point limit); a second context in flight holds its own. */
int fsdf_set_plan(fsdf_ctx* ctx, int32_t enable, double four_way_share, double two_way_share, int64_t max_points);

/* Diagnostics: the serial-equivalent durations (100 MHz ticks) the last
 * planned pass measured per 64-point chunk of the resident cloud (resident
 * order), as the plan is built from them. *count_out = the chunk count (0
 * before a planned pass); costs_out may be NULL to query it. FSDF_ERR_STATE
 * for a ranged cloud that has been regrouped (see fsdf_set_points_range). */
int fsdf_chunk_costs(fsdf_ctx* ctx, uint32_t* costs_out, int64_t* count_out);

/* Kernel work counters (diagnostics). enable=1 zeroes and starts counting in
 * every following pass; enable=0 stops and writes the counters:
 *   [0] wave-iterations (64 points each)  [1] hull evaluations (per wave)
 *   [2] slow-path entries (per wave)      [3] lane-needs summed over evaluations
 *   [4] lanes on the slow path            [5] best-first seed evaluations
 *   [6] waves reaching the exhaustive scan [7] lanes in the exhaustive scan
 *   [8] candidate hulls after wave culling [9] faces of the evaluated hulls
 *   [10..18] reserved (0; the per-phase clocks live in the -DFSDF_WAVE_TIMES=1
 *   timeline build, tools/wave_times.py)
 *   [19] screened plane maxima that fell back to the full fp64 scan (per
 *   wave) [20] evaluations rejected early by the screen [21] descent-walk
 *   steps (per wave) [22] waves on the seed-first path (their candidates
 *   in [8] are those left by the cull after the seeds) [23] reserved (0).
 *   24 counters. */
int fsdf_kernel_stats(fsdf_ctx* ctx, int32_t enable, uint64_t* counters_out);

#ifdef __cplusplus
}
#endif

#endif /* FLASHSDF_H */
