"""An independent reference for scenes with RBF skins and deformations, and the
family of skin scenes the device solver step's RBF half is tested on.

Written from include/flashsdf.h and the header comment of oracle/rbf.py alone:
    centres   c_j = R_b (p_j + δ_j) + t_b from mech_ref.fk_ref (p_j + δ_j for a
              centre on the world: body 0, or -1 as the C-ABI writes it); the
              surface points (value 0) first, then the skeleton points (-1)
    fit       [A P; Pᵀ 0] u = [v; 0], A_ik = |c_i - c_k|³ with an exactly zero
              diagonal, P_i = (1, c_iᵀ), u = (w, a, b) — by a Gaussian
              elimination with partial pivoting on the real part written here
              (numpy.linalg has no extended-precision solve), generic in
              complex128 / clongdouble, batched over the leading axis
    field     f(p) = Σ w_i |p - c_i|³ + a + b·p, s = f / √(∇f·∇f) (no conjugate:
              analytic in the complex step)
    objective c(x) = Σ_p d*(p)² + weight · |δ|², k* frozen at the value the CPU
              oracle gives at the reference's own poses and rows; a skin's
              points take the reference's own s, a hull's the oracle's d*
              (mech_ref.ObjectiveRef's formula)
    gradient  over the whole state (joint coordinates, un-normalised
              quaternions, δ): the skins' part by the complex step (h = 1e-30)
              through FK, centres, fit and field — the weight solve and the
              quaternion projection are differentiated, no adjoint restated;
              the hulls' part ObjectiveRef's -n·(v + ω × p) sums; 2 weight δ.
It calls nothing of flash.rbf, of flash.gradientdescent.gradient_from_accum, of
oracle/rbf.py or of the library; the tree and the skins are read from the
containers as mech_ref._tree does.
"""
import math

import numpy as np

import mech_ref

STEP_H = mech_ref.STEP_H
MAX_STEP = mech_ref.MAX_STEP
HULL_GAP = 1e-12  # mech_ref.untied's rule, hull against hull
SKIN_GAP = 1e-9   # hull against skin, skin against skin


# ---- centres, fit, field ---------------------------------------------------------
def skins_of(m):
    """Per RBF surface in surface order: (surface index, body [n] (<= 0: the
    world), local [n, 3], deformation row [n] (-1: none), values [n]). The
    deformation rows count through all surfaces in surface order."""
    out, row0 = [], 0
    for k, s in enumerate(m.surfaces):
        nd = s.num_deformations()
        if hasattr(s, "skeleton_points"):
            sp, sk = s.surface_points, s.skeleton_points
            body = np.array([b for b, _ in sp] + [b for b, _ in sk], np.int64)
            local = np.array([p for _, p in sp] + [p for _, p in sk], np.float64).reshape(-1, 3)
            drow = np.full(len(body), -1, np.int64)
            if nd:
                drow[:len(sp)] = row0 + np.arange(len(sp))
            out.append((k, body, local, drow, np.concatenate([np.zeros(len(sp)), -np.ones(len(sk))])))
        row0 += nd
    return out


def _dtype(x):
    return x.dtype if x.dtype in (np.complex128, np.clongdouble, np.longdouble) else np.dtype(np.float64)


def centres_ref(m, x, skins=None):
    """[.., n, 3] world centres of every skin at x [.., nx] (any dtype of
    fk_ref), batched over the leading axes."""
    x = np.asarray(x)
    dt = _dtype(x)
    x = x.astype(dt)
    nq = m.mechanism.num_positions
    R, t, _, _ = mech_ref.fk_ref(m.mechanism, x[..., :nq])  # (R[0] = I, t[0] = 0: the world)
    out = []
    for _, body, local, drow, _ in (skins_of(m) if skins is None else skins):
        P = np.broadcast_to(local.astype(dt), x.shape[:-1] + local.shape).copy()
        has = drow >= 0
        if has.any():
            P[..., has, :] += x[..., nq + 3 * drow[has][:, None] + np.arange(3)]
        b = np.maximum(body, 0)
        out.append(np.sum(R[..., b, :, :] * P[..., None, :], axis=-1) + t[..., b, :])
    return out


def system_ref(C):
    """[.., m, m] of the fit over centres C [.., n, 3]."""
    n = C.shape[-2]
    d = C[..., :, None, :] - C[..., None, :, :]
    r = np.sqrt(np.sum(d * d, axis=-1))
    A = r * r * r
    i = np.arange(n)
    A[..., i, i] = 0
    M = np.zeros(C.shape[:-2] + (n + 4, n + 4), C.dtype)
    M[..., :n, :n] = A
    M[..., :n, n] = 1
    M[..., :n, n + 1:] = C
    M[..., n, :n] = 1
    M[..., n + 1:, :n] = np.swapaxes(C, -1, -2)
    return M


def solve_ref(M, b):
    """M z = b [.., m] by Gaussian elimination with partial pivoting on the real
    part, in M's own dtype (complex128 / clongdouble / real), every system of
    the batch with its own pivots. LinAlgError on an exactly zero pivot."""
    m = M.shape[-1]
    lead = M.shape[:-2]
    W = np.concatenate([M, np.broadcast_to(b, lead + (m,))[..., None].astype(M.dtype)], axis=-1).reshape(-1, m, m + 1)
    rows = np.arange(len(W))
    for c in range(m):
        p = c + np.argmax(np.abs(W[:, c:, c].real), axis=1)
        top = W[rows, p].copy()
        W[rows, p] = W[rows, c]
        W[rows, c] = top
        if np.any(top[:, c].real == 0) or not np.all(np.isfinite(top[:, c].real)):
            raise np.linalg.LinAlgError(f"singular system at column {c}")
        l = W[:, c + 1:, c] / top[:, None, c]
        W[:, c + 1:, c:] -= l[:, :, None] * top[:, None, c:]
    z = np.zeros((len(W), m), M.dtype)
    for c in range(m - 1, -1, -1):
        z[:, c] = (W[:, c, m] - np.sum(W[:, c, c + 1:m] * z[:, c + 1:], axis=1)) / W[:, c, c]
    return z.reshape(lead + (m,))


def fit_ref(C, values):
    """u = (w, a, b) [.., n + 4] of the skin over centres C [.., n, 3]."""
    rhs = np.concatenate([np.asarray(values), np.zeros(4)]).astype(C.dtype)
    return solve_ref(system_ref(C), rhs)


def field_ref(C, u, pts):
    """s = f / √(∇f·∇f) [B, N] at pts [N, 3] for C [B, n, 3], u [B, n + 4]."""
    pts = np.asarray(pts, np.float64).astype(C.dtype)
    B, n = C.shape[0], C.shape[1]
    out = np.empty((B, len(pts)), C.dtype)
    per = max(1, int(2.5e6 // max(1, len(pts) * n * 3)))
    for s0 in range(0, B, per):
        c, v = C[s0:s0 + per], u[s0:s0 + per]
        d = pts[None, :, None, :] - c[:, None, :, :]
        r = np.sqrt(np.sum(d * d, axis=-1))
        w = v[:, None, :n]
        f = np.sum(w * (r * r * r), axis=-1) + v[:, n, None] + np.sum(pts[None] * v[:, None, n + 1:], axis=-1)
        g = np.sum((3 * w * r)[..., None] * d, axis=2) + v[:, None, n + 1:]
        out[s0:s0 + per] = f / np.sqrt(np.sum(g * g, axis=-1))
    return out


# ---- the objective ----------------------------------------------------------------
class SkinObjective:
    """x -> (c, g) of Σ d*² + weight |δ|² over a cloud, as the module's header
    defines it."""

    def __init__(self, m, pts, weight=10.0):
        import oracle
        self.m, self.weight = m, float(weight)
        self.pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
        self.om = oracle.OracleModel.from_manipulator(m)
        self.skins = skins_of(m)
        self.nq = m.mechanism.num_positions
        self.hulls = [k for k, s in enumerate(m.surfaces) if not hasattr(s, "skeleton_points")]
        self.body = np.array([getattr(s, "body", -1) if k in self.hulls else -1 for k, s in enumerate(m.surfaces)])
        self._one = {}

    def poses(self, x):
        """[S, 12] float64: T_body · T_body_geometry of a hull, the identity of a skin."""
        R, t, _, _ = mech_ref.fk_ref(self.m.mechanism, np.asarray(x, np.float64)[:self.nq])
        out = np.tile(np.concatenate([np.eye(3).ravel(), np.zeros(3)]), (len(self.m.surfaces), 1))
        for k in self.hulls:
            s = self.m.surfaces[k]
            out[k, :9] = (R[s.body] @ np.asarray(s.frame.R, np.float64)).ravel()
            out[k, 9:] = R[s.body] @ np.asarray(s.frame.t, np.float64) + t[s.body]
        return out

    def fits(self, x, dtype=np.complex128):
        """[(C [n, 3], u [n + 4])] per skin at one x, in dtype."""
        xc = np.asarray(x, np.float64).astype(dtype)[None]
        return [(C[0], fit_ref(C, sk[4])[0]) for C, sk in zip(centres_ref(self.m, xc, self.skins), self.skins)]

    def rows(self, x):
        """The rows a pass takes (per skin n rows (c, w), then (a, b)) from the reference's own fit."""
        parts = []
        for C, u in self.fits(x):
            n = len(C)
            parts += [np.hstack([C.real, u.real[:n, None]]), u.real[n:][None]]
        return np.ascontiguousarray(np.concatenate(parts)) if parts else None

    def assign(self, x):
        """(d*, k*, ∇d*) of the CPU oracle at the reference's own poses and rows."""
        return self.om.skin(self.poses(x), self.pts, rbf_rows=self.rows(x))

    def per_surface(self, x):
        """[S, N] float64: every surface's own value at every point."""
        import oracle
        x = np.asarray(x, np.float64)
        poses = self.poses(x)
        D = np.empty((len(self.m.surfaces), len(self.pts)))
        for k in self.hulls:
            if k not in self._one:
                h = self.m.surfaces[k].hull
                self._one[k] = oracle.OracleModel([(h.vertices, h.faces, h.planes)])
            D[k] = self._one[k].skin(poses[k:k + 1], self.pts)[0]
        for (k, *_), (C, u) in zip(self.skins, self.fits(x)):
            D[k] = field_ref(C[None], u[None], self.pts)[0].real
        return D

    def value(self, x, k=None):
        """c(x) with the assignment k (default: the oracle's at x) held."""
        x = np.asarray(x, np.float64)
        if k is None:
            k = self.assign(x)[1]
        D = self.per_surface(x)
        d = D[k, np.arange(len(self.pts))]
        delta = x[self.nq:]
        return math.fsum(float(v) * float(v) for v in d) + self.weight * math.fsum(float(v) * float(v) for v in delta)

    def __call__(self, x, dtype=np.complex128):
        x = np.asarray(x, np.float64)
        nx, nq = x.size, self.nq
        d, k, nrm = self.assign(x)
        terms = []
        g = np.zeros(nx, np.longdouble)
        if self.skins:
            xc = np.broadcast_to(x.astype(dtype), (nx + 1, nx)).copy()
            xc[np.arange(1, nx + 1), np.arange(nx)] += dtype(1j) * dtype(STEP_H)
            for (ks, *_, values), C in zip(self.skins, centres_ref(self.m, xc, self.skins)):
                sel = np.nonzero(k == ks)[0]
                if not len(sel):
                    continue
                s = field_ref(C, fit_ref(C, values), self.pts[sel])
                terms += [float(v) * float(v) for v in s[0].real]
                g += np.sum(s * s, axis=1)[1:].imag.astype(np.longdouble) / np.longdouble(STEP_H)
        hull = np.isin(k, self.hulls)
        if hull.any():
            om, v = mech_ref.twists_ref(self.m.mechanism, x[:nq])
            b = self.body[k[hull]]
            p = self.pts[hull]
            vel = v[:, b, :] + np.cross(om[:, b, :], p[None, :, :])
            J = -np.einsum("inc,nc->ni", vel, nrm[hull])
            g[:nq] += 2 * (J.astype(np.longdouble).T @ d[hull].astype(np.longdouble))
            terms += [float(v) * float(v) for v in d[hull]]
        delta = x[nq:]
        g[nq:] += 2 * np.longdouble(self.weight) * delta.astype(np.longdouble)
        c = math.fsum(terms) + self.weight * math.fsum(float(v) * float(v) for v in delta)
        return c, g.astype(np.float64)


def untied(obj, x):
    """Mask of the points whose k* is the same at poses an ulp apart: the two
    smallest surface values differ by HULL_GAP where both are hulls
    (mech_ref.untied's rule), by SKIN_GAP where a skin is one of them."""
    D = obj.per_surface(x)
    if len(D) < 2:
        return np.ones(D.shape[1], bool)
    order = np.argsort(D, axis=0, kind="stable")[:2]
    cols = np.arange(D.shape[1])
    both_hulls = np.isin(order[0], obj.hulls) & np.isin(order[1], obj.hulls)
    return D[order[1], cols] - D[order[0], cols] >= np.where(both_hulls, HULL_GAP, SKIN_GAP)


# ---- the skin shape family ------------------------------------------------------
# name -> what its system sizes m = n + 4 are (asserted by tests/test_skin_ref.py)
SHAPES = {
    "m8": (8,), "m16": (16,), "m17": (17,), "m63": (63,), "m64": (64,), "m65": (65,), "m66": (66,),
    "lattice13": (13,), "lattice69": (69,), "skins17": (9,) * 17, "big_small": (66, 9), "anchored": (11, 11),
    "deform2": (10, 20), "chain_deform": (12,), "with_hulls": (17,),
}
# the largest single skin "require-all" accepts, n centres stepped down from 100
# (tests/test_gpu_solver_rbf_shapes.py test_mmax_boundary finds and asserts it)
MMAX_N = 77
POINTS = 2048
FP32_SHAPES = ("big_small", "with_hulls")


def sphere_points(n, radius, centre):
    """n distinct points on a sphere (the Fibonacci spiral of
    tests/test_gpu_solver_rbf.py's _sphere_skin)."""
    k = np.arange(n) + 0.5
    phi, th = np.arccos(1.0 - 2.0 * k / n), np.pi * (1.0 + 5.0 ** 0.5) * k
    return radius * np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1) + centre


class _Builder(mech_ref._Builder):
    """mech_ref's builder with skins, and the placement of every floating body."""

    def __init__(self):
        super().__init__()
        self.place = {}

    def floating(self, where, label):
        from flash.mechanism import QuaternionFloating
        b = self.link(0, QuaternionFloating(f"{label}_joint"), None, label)
        self.place[b] = np.asarray(where, np.float64)
        return b

    def skin(self, surface, skeleton, deformable=False):
        from flash.core import DeformableInterpolatingSkin, RigidInterpolatingSkin
        kind = DeformableInterpolatingSkin if deformable else RigidInterpolatingSkin
        self.surfaces.append(kind([(b, np.asarray(p, np.float64)) for b, p in surface],
                                  [(b, np.asarray(p, np.float64)) for b, p in skeleton]))

    def base(self):
        """The zero configuration with the floating bodies at their placements."""
        mech = self.mech
        x = mech.zero_configuration()
        for b, where in self.place.items():
            o = mech.edges[b].q_offset
            x[o + 4:o + 7] = where
        return x


def _sphere_scene(n):
    """A rigid skin of n centres (n − 1 on a sphere, one skeleton point at its
    middle) on one revolute body: the _sphere_skin form, m = n + 4."""
    from flash.mechanism import Revolute
    B = _Builder()
    big = n >= 40
    mid = np.array([0.6, 0.0, 0.0] if big else [0.4, 0.0, 0.05])
    body = B.link(0, Revolute([0, 0, 1], "joint1"), None, "body1")
    B.skin([(body, p) for p in sphere_points(n - 1, 0.5 if big else 0.25, mid)], [(body, mid)])
    return B


def _lattice_scene(side, deformable=False):
    """side³ surface points on a cubic lattice and a skeleton point at its middle on one revolute
    body; every coordinate a multiple of 1/8, so at angle 0 (R = I exactly) the distances tie exactly."""
    from flash.mechanism import Revolute
    B = _Builder()
    body = B.link(0, Revolute([0, 0, 1], "joint1"), None, "body1")
    ticks = np.array([-0.25, 0.25]) if side == 2 else np.array([-0.375, -0.125, 0.125, 0.375])
    mid = np.array([0.5, 0.0, 0.0])
    B.skin([(body, mid + np.array([a, b, c])) for a in ticks for b in ticks for c in ticks], [(body, mid)], deformable)
    return B


def _build(shape):
    from flash.mechanism import Revolute
    if shape == "m8":  # three surface points and a skeleton point off their plane: w = 0, s the plane's distance
        B = _Builder()
        body = B.link(0, Revolute([0, 0, 1], "joint1"), None, "body1")
        B.skin([(body, [0.5, 0.0, 0.0]), (body, [0.3, 0.3, 0.1]), (body, [0.3, -0.2, 0.3])], [(body, [0.2, 0.0, -0.2])])
        return B
    if shape[0] == "m" and shape[1:].isdigit():
        return _sphere_scene(int(shape[1:]) - 4)
    if shape.startswith("sphere"):
        return _sphere_scene(int(shape[6:]))
    if shape == "lattice13_soft":  # (lattice13 with deformable corners: δ can put one corner on another)
        return _lattice_scene(2, deformable=True)
    if shape.startswith("lattice"):
        return _lattice_scene({13: 2, 69: 4}[int(shape[7:])])
    B = _Builder()
    if shape == "skins17":
        tetra = 0.2 * np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]) / np.sqrt(3.0)
        mid = np.array([0.15, 0.0, 0.05])
        for i in range(17):
            b = B.link(0, Revolute(mech_ref.AXES[i % 3], f"joint{i}"), mech_ref._at(1.0 * (i % 5), 1.0 * (i // 5), 0.0),
                       f"body{i}")
            B.skin([(b, mid + (1.0 + 0.02 * i) * p) for p in tetra], [(b, mid)])
    elif shape == "big_small":
        b1 = B.link(0, Revolute([0, 0, 1], "joint1"), None, "body1")
        mid = np.array([0.6, 0.0, 0.0])
        B.skin([(b1, p) for p in sphere_points(61, 0.5, mid)], [(b1, mid)])
        b2 = B.link(0, Revolute([1, 0, 0], "joint2"), mech_ref._at(2.5, 0.0, 0.0), "body2")
        mid = np.array([0.0, 0.2, 0.05])
        B.skin([(b2, p) for p in sphere_points(4, 0.2, mid)], [(b2, mid)])
    elif shape == "anchored":
        octa = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1.0]])
        # a rigid skin on a floating body whose skeleton point is the world's (-1, as the C-ABI writes the world)
        fl = B.floating([0.0, 0.0, 0.5], "floating")
        B.skin([(fl, 0.3 * p) for p in octa], [(-1, [0.02, -0.01, 0.5])])
        # a deformable skin with four of its six surface points on the world, two and the skeleton point
        # on a revolute body
        b2 = B.link(0, Revolute([0, 0, 1], "joint2"), mech_ref._at(2.0, 0.0, 0.0), "body2")
        mid = np.array([0.3, 0.0, 0.0])
        B.skin([(-1 if i in (1, 2, 3, 5) else b2, (mid + 0.25 * p) + ([2.0, 0.0, 0.0] if i in (1, 2, 3, 5) else 0.0))
                for i, p in enumerate(octa)], [(b2, mid)], deformable=True)
    elif shape == "deform2":
        f1 = B.floating([0.0, 0.0, 0.3], "float1")
        B.skin([(f1, p) for p in sphere_points(5, 0.3, np.zeros(3))], [(f1, [0.0, 0.0, 0.0])], deformable=True)
        B.link(0, Revolute([0, 0, 1], "joint2"), mech_ref._at(1.5, 0.0, 0.0), "body2", (0.2, 0.1, 0.05), (0.15, 0, 0))
        f3 = B.floating([3.0, 0.0, 0.3], "float3")
        B.skin([(f3, p) for p in sphere_points(15, 0.3, np.zeros(3))], [(f3, [0.0, 0.0, 0.0])], deformable=True)
    elif shape == "chain_deform":
        p = 0
        links = []
        for i in range(3):
            p = B.link(p, Revolute(mech_ref.AXES[i % 3], f"joint{i}"), mech_ref._at(0, 0, 0.0 if i == 0 else 0.3),
                       f"link{i}")
            links.append(p)
        mid = np.array([0.0, 0.0, 0.1])
        sp = sphere_points(7, 0.2, mid)
        low = np.argsort(sp[:, 2])[:3]  # the three lowest on the second link, in its frame
        B.skin([(links[1], q + [0.0, 0.0, 0.3]) if j in low else (links[2], q) for j, q in enumerate(sp)],
               [(links[2], mid)], deformable=True)
    else:
        raise ValueError(shape)
    return B


def _manipulator(shape):
    """(manipulator, the base state: zero angles, identity quaternions at the placements, δ = 0)."""
    import flash
    if shape == "with_hulls":
        from flash import Models
        m, x = Models.irb_and_squishable()
        return m, np.asarray(x, np.float64)
    B = _build(shape)
    m = B.done()
    x = np.zeros(flash.num_states(m))
    x[:m.mechanism.num_positions] = B.base()
    return m, x


def _start(m, base, shape):
    """x0: angles U(−0.3, 0.3) (the lattices: 0 exactly), quaternions turned by
    N(0, 0.2) per entry and scaled to norm 0.9 .. 1.1, the placements kept,
    δ ~ N(0, 0.01)."""
    mech = m.mechanism
    nq = mech.num_positions
    r = np.random.default_rng(177 + sum(map(ord, shape)))
    x0 = base.copy()
    for b in range(1, mech.num_bodies):
        e = mech.edges[b]
        o = e.q_offset
        if e.joint.kind == "revolute":
            x0[o] = 0.0 if shape.startswith("lattice") else r.uniform(-0.3, 0.3)
        elif e.joint.kind == "quaternion_floating":
            q = x0[o:o + 4] + r.normal(0.0, 0.2, 4)
            x0[o:o + 4] = q / np.linalg.norm(q) * r.uniform(0.9, 1.1)
    x0[nq:] = r.normal(0.0, 0.01, x0.size - nq)
    return x0


def cloud(m, x, n, seed, near=0.85, sigma=0.005, pad=0.3):
    """flash.synthetic.skin_cloud's recipe on the CPU: uniform samples of every
    surface's box (a skin's centres, a hull's vertices) padded by `pad`, in
    equal shares; the first `near` fraction is moved onto the scene's zero set
    by five Newton steps p <- p − d*(p) ∇d*(p) through the CPU oracle at the
    reference's rows (a step at most 0.2 long) and jittered by N(0, sigma)."""
    obj = SkinObjective(m, np.zeros((1, 3)))
    r = np.random.Generator(np.random.PCG64(seed))
    poses, rows = obj.poses(x), obj.rows(x)
    boxes = {k: C.real for (k, *_), (C, _) in zip(obj.skins, obj.fits(x))}
    for k in obj.hulls:
        boxes[k] = m.surfaces[k].hull.vertices @ poses[k, :9].reshape(3, 3).T + poses[k, 9:]
    S = len(m.surfaces)
    parts = []
    for k in range(S):
        lo, hi = boxes[k].min(0) - pad, boxes[k].max(0) + pad
        parts.append(lo + r.random((n // S + (k < n % S), 3)) * (hi - lo))
    pts = np.concatenate(parts)[r.permutation(n)]
    k = int(near * n)
    for _ in range(5):
        d, _, g = obj.om.skin(poses, pts[:k], rbf_rows=rows)
        step = -d[:, None] * g
        nrm = np.linalg.norm(step, axis=1, keepdims=True)
        pts[:k] += step * np.minimum(1.0, 0.2 / np.maximum(nrm, 1e-300))
    pts[:k] += r.normal(scale=sigma, size=(k, 3))
    return np.ascontiguousarray(pts)


_SCENES = {}


def scene(shape, n=POINTS):
    """(manipulator, cloud, x0) — cached, the arrays read-only. The cloud:
    cloud() at a state N(0, 0.03) from x0 in every entry, minus the points that
    untied() drops at x0 (at most 0.1 % of them, asserted)."""
    key = (shape, n)
    if key not in _SCENES:
        m, base = _manipulator(shape)
        x0 = _start(m, base, shape)
        r = np.random.default_rng(4242 + len(shape))
        x_true = x0 + r.normal(0.0, 0.03, x0.size)
        pts = cloud(m, x_true, n, seed=900 + len(shape))
        keep = untied(SkinObjective(m, pts), x0)
        assert (~keep).sum() <= 1e-3 * len(pts), (shape, int((~keep).sum()))
        pts = np.ascontiguousarray(pts[keep])
        pts.flags.writeable = False
        x0.flags.writeable = False
        _SCENES[key] = (m, pts, x0)
    return _SCENES[key]


_OBJECTIVES, _GAPS = {}, {}


def objective(shape):
    """The scene's SkinObjective (weight: CostFunctor's default), cached."""
    if shape not in _OBJECTIVES:
        from flash.gradientdescent import default_deformation_cost_weight
        m, pts, _ = scene(shape)
        _OBJECTIVES[shape] = SkinObjective(m, pts, default_deformation_cost_weight)
    return _OBJECTIVES[shape]


def precision_gap(shape):
    """The reference's own noise floor: max |g128 − g80| / max |g80| of its
    gradient at x0 in complex128 and in clongdouble (the fit's condition number
    enters here). Computed once per shape."""
    if shape not in _GAPS:
        obj, x0 = objective(shape), scene(shape)[2]
        g128, g80 = obj(x0)[1], obj(x0, np.clongdouble)[1]
        _GAPS[shape] = float(np.abs(g128 - g80).max() / np.abs(g80).max())
    return _GAPS[shape]


def condition_numbers(shape):
    """cond₂ of every skin's system at x0 (numpy's SVD on the float64 system:
    a figure to print, not part of the reference)."""
    obj, x0 = objective(shape), scene(shape)[2]
    return [float(np.linalg.cond(system_ref(C.real[None])[0])) for C, _ in obj.fits(x0)]


def bound_of(shape):
    """The relative bound of every check against this reference."""
    return max(1e-9, 100.0 * precision_gap(shape))


# The NaiveSolver rate per shape (max_step 0.05): the largest of 64, 32, 16, ...
# at which the reference's own descent leaves at least half of the coordinates
# unclipped in each of its first four iterations, with and without
# mech_ref.divisors_of, and the fourth step is still at least 1 % of the first
# (still_descending) — found by reference_rate() on the CPU, asserted again by
# tests/test_skin_ref.py.
RATES = {"m8": 4.0, "m16": 16.0, "m17": 16.0, "m63": 2.0, "m64": 2.0, "m65": 2.0, "m66": 2.0, "lattice13": 4.0,
         "lattice69": 2.0, "skins17": 64.0, "big_small": 64.0, "anchored": 16.0, "deform2": 16.0, "chain_deform": 2.0,
         "with_hulls": 4.0, f"sphere{MMAX_N}": 8.0}


def rate_of(shape):
    return RATES[shape]


def reference_descent(shape, rate, iterations=4, divisors=None):
    """The reference's own descent: [(x, f, g / N, clipped step, unclipped)]."""
    obj, x = objective(shape), np.array(scene(shape)[2])
    n, out = float(len(obj.pts)), []
    for _ in range(iterations):
        c, g = obj(x)
        step, raw = mech_ref.naive_step_ref(g / n, rate, MAX_STEP, divisors)
        out.append((x.copy(), c / n, g / n, step, raw))
        x = x + step
    return out


def half_unclipped(trace):
    return all(2 * np.count_nonzero(np.abs(raw) < MAX_STEP * (1 - 1e-9)) >= raw.size for *_, raw in trace)


def still_descending(trace):
    """The last iteration's largest unclipped step is at least 1 % of the
    first's. Most shapes have one coordinate, and a rate near 1 / c'' converges
    quadratically: the fourth step would be 1e-10 of the first, below the
    rounding of the sums it is made of (relative to Σ|2 d ∂d|, not to their
    cancelled sum), and a check relative to the step would measure that
    rounding, not the step."""
    return np.abs(trace[-1][4]).max() >= 1e-2 * np.abs(trace[0][4]).max()


def rate_holds(shape, rate, iterations=4):
    from mech_ref import divisors_of
    for div in (None, divisors_of(scene(shape)[2].size)):
        tr = reference_descent(shape, rate, iterations, div)
        if not (half_unclipped(tr) and still_descending(tr)):
            return False
    return True


def reference_rate(shape, iterations=4):
    rate = 64.0
    while rate > 1e-6:
        if rate_holds(shape, rate, iterations):
            return rate
        rate *= 0.5
    raise AssertionError("no rate leaves half of the coordinates unclipped")
