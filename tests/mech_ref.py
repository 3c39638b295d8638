"""An independent reference for everything after the residual pass, and the
family of scenes the solver-loop tests run on.

The reference is written from the conventions of include/flashsdf.h and the
header comment of csrc/kin_impl.h alone:
    T_b  = T_parent · A · J(q) · B      (A = joint_to_parent, B = body_to_joint)
    Tb_b = T_parent · A                 (the joint frame before its motion)
    J    = I (fixed) | rotation by q about the unit axis (revolute) |
           R(q̂), t = q[4:7] with q̂ = q[:4] / |q[:4]| (quaternion-floating,
           q = (w, x, y, z, tx, ty, tz))
    a revolute angle with |q| >= 8.23549136e5 means fmod(q, fl(2π)) (the fold
    kin::sincos documents)
It reads the tree's data (parents, joint kinds, axes, the two fixed frames)
from flash.mechanism's containers and calls none of its kinematics, nothing of
flash.core's poses, of oracle/kinematics.py or of the library. Derivatives come
from the complex step through that forward kinematics, so the quaternion
projection is differentiated, not restated. Per-point d*, k*, ∇d* come from the
CPU oracle (bit for bit the pass's, tests/test_gpu_parity.py) at this file's
own surface poses; sums are its own (math.fsum for the cost).
"""
import math

import numpy as np

FOLD = 8.23549136e5  # kin::sincos folds beyond 2^19 pi/2 ...
TWO_PI_FL = 6.28318530717958623200  # ... by fmod(x, this)
STEP_H = 1e-30  # the complex step


# ---- forward kinematics --------------------------------------------------------
def _tree(mech):
    """The tree's data as plain lists (no kinematics of flash.mechanism)."""
    out = [None]
    for e in mech.edges[1:]:
        j = e.joint
        a = np.asarray(j.axis, np.float64)
        out.append((e.parent, j.kind, e.q_offset, a / np.sqrt(a @ a), np.asarray(e.joint_to_parent.R, np.float64),
                    np.asarray(e.joint_to_parent.t, np.float64), np.asarray(e.body_to_joint.R, np.float64),
                    np.asarray(e.body_to_joint.t, np.float64)))
    return out


def _cross_matrix(a, dt):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dt)


def _folded(ang):
    """The documented meaning of an angle beyond the fold (its imaginary part,
    the complex step's, rides along)."""
    re = np.real(ang)
    big = ~(np.abs(re) < FOLD)
    if not np.any(big):
        return ang
    red = np.where(big, np.fmod(re, np.asarray(TWO_PI_FL, re.dtype)), re)
    return red + 1j * np.imag(ang) if np.iscomplexobj(ang) else red


def fold_configuration(mechanism, x):
    """x with every revolute angle beyond the fold replaced by its documented
    meaning, for code that takes a true sine of what it is given."""
    x = np.array(x, np.float64)
    for e in mechanism.edges[1:]:
        if e.joint.kind == "revolute":
            x[e.q_offset] = _folded(x[e.q_offset:e.q_offset + 1])[0]
    return x


def fk_ref(mechanism, x):
    """(R [.., nb, 3, 3], t [.., nb, 3], Rb, tb) of every body and joint frame
    at x [.., nx] — float64, complex128, np.longdouble or np.clongdouble,
    batched over leading axes. numpy's own sin and cos."""
    x = np.asarray(x)
    dt = x.dtype if x.dtype in (np.complex128, np.longdouble, np.clongdouble) else np.float64
    x = x.astype(dt)
    tree = _tree(mechanism)
    nb, lead = len(tree), x.shape[:-1]
    eye = np.eye(3).astype(dt)
    R = np.zeros(lead + (nb, 3, 3), dt)
    t = np.zeros(lead + (nb, 3), dt)
    Rb, tb = R.copy(), t.copy()
    R[..., 0, :, :] = eye
    Rb[..., 0, :, :] = eye
    for b in range(1, nb):
        p, kind, o, axis, AR, At, BR, Bt = tree[b]
        AR, At, BR, Bt = AR.astype(dt), At.astype(dt), BR.astype(dt), Bt.astype(dt)
        Rp, tp = R[..., p, :, :], t[..., p, :]
        Rb[..., b, :, :] = Rp @ AR
        tb[..., b, :] = Rp @ At + tp
        if kind == "fixed":
            JR, Jt = np.broadcast_to(eye, lead + (3, 3)), np.zeros(lead + (3,), dt)
        elif kind == "revolute":
            ang = _folded(x[..., o])
            c, s = np.cos(ang)[..., None, None], np.sin(ang)[..., None, None]
            a = axis.astype(dt)
            JR = c * eye + s * _cross_matrix(a, dt) + (1 - c) * np.outer(a, a)
            Jt = np.zeros(lead + (3,), dt)
        elif kind == "quaternion_floating":
            q = x[..., o:o + 4]
            q = q / np.sqrt(np.sum(q * q, axis=-1))[..., None]  # (no conjugate: analytic in the complex step)
            w, v = q[..., 0], q[..., 1:4]
            vx = np.zeros(lead + (3, 3), dt)
            vx[..., 0, 1], vx[..., 0, 2] = -v[..., 2], v[..., 1]
            vx[..., 1, 0], vx[..., 1, 2] = v[..., 2], -v[..., 0]
            vx[..., 2, 0], vx[..., 2, 1] = -v[..., 1], v[..., 0]
            vv = np.sum(v * v, axis=-1)
            JR = ((w * w - vv)[..., None, None] * eye + 2 * v[..., :, None] * v[..., None, :]
                  + 2 * w[..., None, None] * vx)
            Jt = x[..., o + 4:o + 7]
        else:
            raise ValueError(kind)
        RJ = Rb[..., b, :, :] @ JR
        R[..., b, :, :] = RJ @ BR
        t[..., b, :] = RJ @ Bt + (Rb[..., b, :, :] @ Jt[..., None])[..., 0] + tb[..., b, :]
    return R, t, Rb, tb


def surface_poses_ref(m, x):
    """[S, 12] float64: T_body · T_body_geometry per surface, from fk_ref."""
    R, t, _, _ = fk_ref(m.mechanism, np.asarray(x, np.float64))
    out = np.empty((len(m.surfaces), 12))
    for k, s in enumerate(m.surfaces):
        out[k, :9] = (R[s.body] @ np.asarray(s.frame.R, np.float64)).ravel()
        out[k, 9:] = R[s.body] @ np.asarray(s.frame.t, np.float64) + t[s.body]
    return out


def twists_ref(mechanism, x):
    """(omega [nx, nb, 3], v [nx, nb, 3]): per coordinate i and body b the
    world twist ∂/∂x_i — [ω]× = ∂R Rᵀ, v = ∂t − ω × t (the velocity of the
    body's point at the world origin) — by the complex step through fk_ref."""
    x = np.asarray(x, np.float64)
    nx = x.size
    xc = np.broadcast_to(x.astype(np.complex128), (nx, nx)).copy()
    xc[np.arange(nx), np.arange(nx)] += 1j * STEP_H
    R, t, _, _ = fk_ref(mechanism, xc)
    dR, dt_ = R.imag / STEP_H, t.imag / STEP_H
    R, t = R.real, t.real
    W = dR @ np.swapaxes(R, -1, -2)
    om = 0.5 * np.stack([W[..., 2, 1] - W[..., 1, 2], W[..., 0, 2] - W[..., 2, 0], W[..., 1, 0] - W[..., 0, 1]], axis=-1)
    return om, dt_ - np.cross(om, t)


def config_gradient_ref(mechanism, x, body_wrench):
    """∂c/∂x_i = −Σ_b (ω_ib · M_b + v_ib · F_b) for wrenches (F, M about the
    world origin) [nb, 6], in np.longdouble sums."""
    om, v = twists_ref(mechanism, x)
    w = np.asarray(body_wrench, np.longdouble).reshape(-1, 6)
    g = -(np.sum(om.astype(np.longdouble) * w[None, :, 3:], axis=(1, 2))
          + np.sum(v.astype(np.longdouble) * w[None, :, :3], axis=(1, 2)))
    return g.astype(np.float64)


# ---- the objective of a rigid scene -------------------------------------------
class ObjectiveRef:
    """x -> (c, g, J, H) of Σ d*² over a cloud: d*, k*, ∇d* from the CPU oracle
    at surface_poses_ref(x); J[p, i] = −n_p · (v + ω × p) for the body of
    k*(p); g = 2 Jᵀd; H = 2 JᵀJ; c by math.fsum. No wrench accumulator."""

    def __init__(self, m, pts):
        import oracle
        self.m = m
        self.om = oracle.OracleModel.from_manipulator(m)
        self.pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        self.body = np.array([s.body for s in m.surfaces], np.int64)

    def per_point(self, x):
        return self.om.skin(surface_poses_ref(self.m, x), self.pts)

    def value(self, x):
        d, _, _ = self.per_point(x)
        return math.fsum(float(v) * float(v) for v in d)

    def __call__(self, x):
        x = np.asarray(x, np.float64)
        d, k, n = self.per_point(x)
        om, v = twists_ref(self.m.mechanism, x)
        b = self.body[k]
        vel = v[:, b, :] + np.cross(om[:, b, :], self.pts[None, :, :])  # [nx, N, 3]
        J = -np.einsum("inc,nc->ni", vel, n)
        Jl, dl = J.astype(np.longdouble), d.astype(np.longdouble)
        g = (2 * (Jl.T @ dl)).astype(np.float64)
        H = (2 * (Jl.T @ Jl)).astype(np.float64)
        return math.fsum(float(u) * float(u) for u in d), g, J, H


def objective_ref(m, pts, x):
    return ObjectiveRef(m, pts)(x)


# ---- solver steps ---------------------------------------------------------------
def naive_step_ref(g, rate, max_step, divisors=None):
    """NaiveSolver's rule (flash/tracking.py) on the wrapped gradient g (already
    divided by N): (clipped step, unclipped step)."""
    g = np.asarray(g, np.float64)
    if divisors is not None:
        g = g / np.asarray(divisors, np.float64)
    raw = -rate * g
    return np.clip(raw, -max_step, max_step), raw


def lm_trial_ref(H, g, lam, max_step):
    """One damped step as include/flashsdf.h defines it: D_ii = max(H_ii, 1e-12
    max_j H_jj), dx = clamp(−(H + λ D)⁻¹ g, ±max_step); solved in np.longdouble
    by elimination with partial pivoting (not the library's Cholesky)."""
    H = np.asarray(H, np.longdouble)
    n = H.shape[0]
    d = np.diag(H)
    D = np.maximum(d, np.longdouble(1e-12) * d.max())
    A = H + np.longdouble(lam) * np.diag(D)
    rhs = -np.asarray(g, np.longdouble)
    M = np.concatenate([A, rhs[:, None]], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if p != c:
            M[[c, p]] = M[[p, c]]
        M[c + 1:] -= (M[c + 1:, c] / M[c, c])[:, None] * M[c]
    z = np.zeros(n, np.longdouble)
    for c in range(n - 1, -1, -1):
        z[c] = (M[c, n] - M[c, c + 1:n] @ z[c + 1:]) / M[c, c]
    z = z.astype(np.float64)
    return np.clip(z, -max_step, max_step), z


# ---- the shape family -----------------------------------------------------------
CHAIN_LENGTHS = (1, 2, 3, 4, 5, 8, 9)


def angle_values():
    """The edge angles of kin::sincos the `angles` shape starts from."""
    h = np.pi / 2
    out = [0.0, 2.0 ** -28, -2.0 ** -28, np.pi / 4, np.nextafter(np.pi / 4, 0.0), np.nextafter(np.pi / 4, 4.0)]
    for k in range(1, 5):
        c = k * h
        out += [c, np.nextafter(c, 0.0), np.nextafter(c, 8.0), c - 1e-9, c + 1e-9, c - 1e-5, c + 1e-5]
    out += [3.0, 100.0, 823549.0, 823550.0, 1.0e6]
    return np.array(out, np.float64)


ANGLE_TRIPLES = len(angle_values()) // 3  # 39 angles: 13 triples

SHAPES = (["single"] + [f"chain_{k}" for k in CHAIN_LENGTHS]
          + ["wide10", "wide11", "float9_r0", "float9_r1", "float9_r2", "float10", "star66"])
MIXED_SEEDS = (0, 1, 2)


def all_cases():
    """(shape, seed) of every scene but star_too_large."""
    return ([(s, 0) for s in SHAPES] + [("mixed", s) for s in MIXED_SEEDS]
            + [("angles", s) for s in range(ANGLE_TRIPLES)])


def case_id(case):
    return f"{case[0]}-{case[1]}" if case[0] in ("mixed", "angles") else case[0]


def _at(x, y, z):
    from flash.geometry import Transform
    return Transform(np.eye(3), np.array([x, y, z], np.float64))


def _random_rotation(r):
    q = r.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


class _Builder:
    def __init__(self):
        from flash.mechanism import Mechanism
        self.mech, self.surfaces = Mechanism("world"), []

    def link(self, parent, joint, where, label, half=None, centre=(0, 0, 0), body_to_joint=None, frame=None):
        from flash import Models
        from flash.core import ConvexGeometry
        b = self.mech.attach(parent, joint, where, label, body_to_joint)
        if half is not None:
            self.surfaces.append(ConvexGeometry(Models.box_hull(half), b, frame or _at(*centre), label))
        return b

    def box(self, b, half, frame, label):
        from flash import Models
        from flash.core import ConvexGeometry
        self.surfaces.append(ConvexGeometry(Models.box_hull(half), b, frame, label))

    def done(self):
        from flash.core import Manipulator
        return Manipulator(self.mech, self.surfaces)


AXES = ([0, 0, 1], [1, 0, 0], [0, 1, 0])


def _chain(k):
    """A serial chain of k links. Every box sits skew in its link (a frame
    rotated by 0.37 + 0.23 i rad about an oblique axis) and has its own size:
    at joint angles that are multiples of pi/2 no two boxes then share a face
    plane, so the cloud has no points that are exactly tied between two hulls."""
    from flash.geometry import Transform, angle_axis
    from flash.mechanism import Fixed, Revolute
    B, p = _Builder(), 0
    for i in range(k):
        fixed = k == 5 and i == 2  # chain_5: a Fixed joint in the middle ...
        bare = k == 5 and i == 3  # ... and a body without a surface
        joint = Fixed(f"joint{i}") if fixed else Revolute(AXES[i % 3], f"joint{i}")
        skew = np.array([1.0 + i % 2, 2.0, 3.0 - i % 3])
        frame = Transform(angle_axis(0.37 + 0.23 * i, skew / np.linalg.norm(skew)), np.array([0.02, 0.005 * i, 0.1]))
        p = B.link(p, joint, _at(0, 0, 0.0 if i == 0 else 0.2), f"link{i}",
                   None if bare else (0.05 + 0.004 * i, 0.03 + 0.003 * i, 0.08 - 0.003 * i), frame=frame)
    return B.done()


def _comb(teeth):
    """gn_helpers.branching_scene("comb")'s form with `teeth` teeth."""
    from flash.mechanism import Revolute
    B = _Builder()
    half = 0.1 * teeth + 0.1
    spine = B.link(0, Revolute([0, 0, 1], "spine_joint"), None, "spine", (half, 0.04, 0.04))
    for i in range(teeth):
        tooth = B.link(spine, Revolute([1, 0, 0], f"tooth{i}_joint"), _at(0.2 * i - 0.1 * (teeth - 1), 0, 0.06),
                       f"tooth{i}", (0.05, 0.03, 0.08), (0, 0, 0.1))
        for side, y in enumerate((-0.07, 0.07)):
            B.link(tooth, Revolute([0, 1, 0], f"leaf{i}_{side}_joint"), _at(0, y, 0.2), f"leaf{i}_{side}",
                   (0.04, 0.025, 0.05), (0, 0, 0.07))
    return B.done()


def _floating(boxes, links):
    from flash.mechanism import QuaternionFloating, Revolute
    B, first = _Builder(), 0
    for i in range(boxes):
        b = B.link(0, QuaternionFloating(f"float{i}"), None, f"box{i}", (0.12, 0.08, 0.05))
        first = first or b
    p = first
    for i in range(links):
        p = B.link(p, Revolute(AXES[(i + 1) % 3], f"arm{i}_joint"), _at(0, 0, 0.05 if i == 0 else 0.2), f"arm{i}",
                   (0.03, 0.03, 0.08), (0, 0, 0.1))
    return B.done()


def _star(arms):
    from flash.mechanism import Revolute
    B, cols = _Builder(), 12
    for i in range(arms):
        ax = AXES[i % 3] if i % 2 else [1.0, 0.5 * (i % 5), 0.25 * (i % 3)]
        B.link(0, Revolute(ax, f"arm{i}_joint"), _at(0.3 * (i % cols), 0.3 * (i // cols), 0.0), f"arm{i}",
               (0.04, 0.05, 0.1), (0.01, 0, 0.1))
    return B.done()


def _mixed(seed):
    """A random tree of 12 bodies: parents uniform among earlier bodies, about
    30 % quaternion-floating, 15 % fixed, the rest revolute about random axes;
    random joint_to_parent / body_to_joint rotations with 0.3 m offsets; a
    quaternion joint below a revolute parent; one body with two surfaces, one
    with none."""
    from flash.geometry import Transform
    from flash.mechanism import Fixed, QuaternionFloating, Revolute
    r = np.random.default_rng(1000 + seed)
    B, n = _Builder(), 12
    kinds = r.choice(["quaternion_floating", "fixed", "revolute"], size=n, p=[0.3, 0.15, 0.55])
    kinds[0] = "revolute"
    parents = [0] + [int(r.integers(0, b + 1)) for b in range(1, n)]  # (body indices: 0 the world)
    parents[1], kinds[1] = 1, "quaternion_floating"  # a quaternion joint below the revolute body 1
    bare, double = 5, 7
    for i in range(n):
        def frame():
            return Transform(_random_rotation(r), r.uniform(-0.3, 0.3, 3))
        joint = {"quaternion_floating": lambda: QuaternionFloating(f"joint{i}"), "fixed": lambda: Fixed(f"joint{i}"),
                 "revolute": lambda: Revolute(r.normal(size=3), f"joint{i}")}[kinds[i]]()
        b = B.link(parents[i], joint, frame(), f"body{i}", None, body_to_joint=frame())
        if i != bare:
            B.box(b, r.uniform(0.04, 0.12, 3), Transform(_random_rotation(r), r.uniform(-0.05, 0.05, 3)), f"box{i}")
        if i == double:
            B.box(b, r.uniform(0.04, 0.1, 3), Transform(_random_rotation(r), r.uniform(0.1, 0.25, 3)), f"box{i}b")
    return B.done()


def _manipulator(shape, seed):
    if shape == "single":
        from flash.mechanism import Revolute
        B = _Builder()
        B.link(0, Revolute([0, 0, 1], "joint"), None, "body", (0.2, 0.1, 0.05), (0.15, 0, 0))
        return B.done()
    if shape.startswith("chain_"):
        return _chain(int(shape[6:]))
    if shape == "angles":
        return _chain(3)
    if shape.startswith("wide"):
        return _comb(int(shape[4:]))
    if shape.startswith("float"):
        boxes, _, links = shape[5:].partition("_r")
        return _floating(int(boxes), int(links or 0))
    if shape.startswith("star"):
        return _star(120 if shape == "star_too_large" else int(shape[4:]))
    if shape == "mixed":
        return _mixed(seed)
    raise ValueError(shape)


def _start(m, shape, seed):
    """x0: small angles, the floating boxes on a grid with quaternions of norm
    0.9 .. 1.1; `angles`: the seed-th triple of angle_values()."""
    mech = m.mechanism
    r = np.random.default_rng(77 + 13 * seed + len(shape))
    x0 = r.uniform(-0.3, 0.3, mech.num_positions)
    if shape == "angles":
        return angle_values()[3 * seed:3 * seed + 3].copy()
    nfloat = 0
    for b in range(1, mech.num_bodies):
        e = mech.edges[b]
        if e.joint.kind != "quaternion_floating":
            continue
        q = r.normal(size=4)
        o = e.q_offset
        x0[o:o + 4] = q / np.linalg.norm(q) * r.uniform(0.9, 1.1)
        if shape == "mixed":
            x0[o + 4:o + 7] = r.uniform(-0.3, 0.3, 3)
        else:
            x0[o + 4:o + 7] = (0.5 * (nfloat % 4), 0.5 * (nfloat // 4), 0.3)
        nfloat += 1
    return x0


def untied(m, pts, x, gap=1e-12):
    """Mask of the points whose two smallest per-hull distances differ by at
    least `gap` at x (k* is then the same at poses an ulp apart)."""
    import oracle
    pts = np.ascontiguousarray(pts, np.float64)
    poses = surface_poses_ref(m, x)
    if len(m.surfaces) < 2:
        return np.ones(len(pts), bool)
    best = np.full(len(pts), np.inf)
    second = np.full(len(pts), np.inf)
    for k, s in enumerate(m.surfaces):
        one = oracle.OracleModel([(s.hull.vertices, s.hull.faces, s.hull.planes)])
        d, _, _ = one.skin(poses[k:k + 1], pts)
        second = np.minimum(second, np.maximum(best, d))
        best = np.minimum(best, d)
    return second - best >= gap


_SCENES = {}


def scene(shape, seed=0, n=None, noisy=False):
    """(manipulator, cloud, x0) — cached; the returned arrays are read-only.
    The cloud: synthetic.depth_cloud at a configuration 0.03 from x0 in every
    coordinate's scale, 2,048 points (3,072 for the wide and floating shapes,
    4,096 for the stars), minus the points tied between two hulls at x0 (at
    most 0.1 % of them, asserted). noisy: sigma 2 cm and 20 % box outliers in
    place of depth_cloud's defaults, for the LM loop's rejected trials."""
    key = (shape, seed, n, noisy)
    if key in _SCENES:
        return _SCENES[key]
    from flash import synthetic
    m = _manipulator(shape, seed)
    x0 = _start(m, shape, seed)
    r = np.random.default_rng(4242 + seed)
    x_true = x0 + r.normal(0.0, 0.03, x0.size)
    if n is None:
        n = 4096 if shape.startswith("star") else 3072 if shape[:4] in ("wide", "floa") else 2048
    kw = dict(sigma=0.02, frac_surface=0.75, frac_box=0.2) if noisy else {}
    pts = synthetic.depth_cloud(m, x_true, n, seed=900 + seed, **kw)
    keep = untied(m, pts, x0)
    assert (~keep).sum() <= 1e-3 * len(pts), (shape, seed, int((~keep).sum()))
    pts = np.ascontiguousarray(pts[keep])
    pts.flags.writeable = False
    x0.flags.writeable = False
    _SCENES[key] = (m, pts, x0)
    return _SCENES[key]


# The NaiveSolver rate per shape for the one-step checks (max_step 0.05): the
# largest of 64, 32, 16, ... at which the reference's own descent (fk_ref,
# the oracle's per-point values, naive_step_ref) leaves at least half of the
# coordinates unclipped in each of its first four iterations — found by
# reference_rate() on the CPU, asserted again by tests/test_mech_ref.py.
MAX_STEP = 0.05
OVER_64 = ("float9_r2", "float10", "star66", "star_too_large")  # more than 64 coordinates: no LM device loop
RATES = {"chain_8": 8.0, "chain_9": 8.0, "mixed-0": 16.0, "mixed-1": 8.0, "mixed-2": 2.0, "angles-2": 32.0,
         "angles-3": 32.0}
DEFAULT_RATE = 64.0  # (every other shape)


def rate_of(case):
    return RATES.get(case_id(tuple(case)), DEFAULT_RATE)


def divisors_of(nx):
    """The preconditioning divisors of tests/test_gpu_solver.py."""
    return np.linspace(1.0, 1.5, nx)


def reference_descent(m, pts, x0, rate, iterations=4, divisors=None):
    """The reference's own descent: [(x, f, g / N, clipped step, unclipped)]."""
    ref, x, n, out = ObjectiveRef(m, pts), np.array(x0, np.float64), float(len(pts)), []
    for _ in range(iterations):
        c, g, _, _ = ref(x)
        step, raw = naive_step_ref(g / n, rate, MAX_STEP, divisors)
        out.append((x.copy(), c / n, g / n, step, raw))
        x = x + step
    return out


def reference_rate(m, pts, x0, iterations=4):
    rate = 64.0
    while rate > 1e-6:
        tr = reference_descent(m, pts, x0, rate, iterations)
        if all(2 * np.count_nonzero(np.abs(raw) < MAX_STEP * (1 - 1e-9)) >= raw.size for *_, raw in tr):
            return rate
        rate *= 0.5
    raise AssertionError("no rate leaves half of the coordinates unclipped")
