"""RBF interpolating skins: the host work around the GPU pass.

Flash.skin for an InterpolatingGeometry (src/Flash.jl:207-213) builds
SpatialFields.InterpolatingSurface(points, values, XCubed(), true) from the
world-frame surface points (value 0, each displaced by its deformation δ_i in
its body frame, src/Flash.jl:158-168) and skeleton points (value -1). Per pass
the host
  1. places the centres (forward kinematics + δ) and solves the (n+4)² system
     [A P; Pᵀ 0][w; a; b] = [v; 0], A_ik = |c_i - c_k|^3, P_i = [1, c_iᵀ];
  2. ships rows (c_i, w_i) and (a, b) to the device (fsdf_set_rbf_params);
and after the pass turns the RBF adjoint block of the accumulator
(λ = Σ 2s ∂s/∂(w,a,b), E_i = Σ 2s ∂s/∂c_i) into ∂c/∂c_j through the solve
(μ = M⁻ᵀλ), then into body wrenches (∂c/∂q) and ∂c/∂δ. The field value on the
device is s = f/|∇f| (matches the KAT test/runtests.jl:17; diverges from the
examples/manipulator.ipynb costs by 4.44x / 2.0x — DESIGN.md §2).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .core import InterpolatingGeometry, Manipulator


@dataclass
class RbfSolve:
    surface: int                  # index in Manipulator.surfaces
    centres: np.ndarray           # [n,3] world
    bodies: np.ndarray            # [n] body of each centre
    deform_rows: np.ndarray       # [n] row of deformation_data/3, -1 if none
    M: np.ndarray                 # [(n+4),(n+4)]
    u: np.ndarray                 # [n+4] = w, a, b

    @property
    def n(self) -> int:
        return len(self.centres)


def rbf_surfaces(manip: Manipulator):
    return [i for i, s in enumerate(manip.surfaces) if isinstance(s, InterpolatingGeometry)]


def solve(manip: Manipulator, q: np.ndarray, deformation_data: np.ndarray) -> list[RbfSolve]:
    """Centres and coefficients of every RBF surface at (q, δ); q normalized by the caller."""
    T = manip.mechanism.body_transforms(q)
    out = []
    row0 = 0
    for i, s in enumerate(manip.surfaces):
        nd = s.num_deformations()
        if not isinstance(s, InterpolatingGeometry):
            row0 += nd
            continue
        cs, bodies, drows = [], [], []
        for j, (b, p) in enumerate(s.surface_points):
            loc = p + deformation_data[3 * (row0 + j): 3 * (row0 + j) + 3] if nd else p
            cs.append(T[b].R @ loc + T[b].t)
            bodies.append(b)
            drows.append(row0 + j if nd else -1)
        for b, p in s.skeleton_points:
            cs.append(T[b].R @ p + T[b].t)
            bodies.append(b)
            drows.append(-1)
        C = np.array(cs)
        n = len(C)
        v = np.concatenate([np.zeros(len(s.surface_points)), -np.ones(len(s.skeleton_points))])
        D = np.linalg.norm(C[:, None] - C[None], axis=-1)
        P = np.hstack([np.ones((n, 1)), C])
        M = np.block([[D ** 3, P], [P.T, np.zeros((4, 4))]])
        u = np.linalg.solve(M, np.concatenate([v, np.zeros(4)]))
        out.append(RbfSolve(i, C, np.array(bodies), np.array(drows), M, u))
        row0 += nd
    return out


def rows(solves: list[RbfSolve]) -> np.ndarray:
    """Device rows: per surface n rows (c, w) then (a, b)."""
    parts = []
    for r in solves:
        n = r.n
        parts.append(np.hstack([r.centres, r.u[:n, None]]))
        parts.append(r.u[n:][None])
    return np.ascontiguousarray(np.concatenate(parts))


def _solve_refined(A: np.ndarray, b: np.ndarray) -> np.ndarray:
    """A x = b (float64 data) to np.longdouble accuracy: a float64 solve and
    two steps of iterative refinement with the residual and the sum in
    np.longdouble."""
    ld = np.longdouble
    Al, bl = A.astype(ld), np.asarray(b, np.float64).astype(ld)
    x = np.linalg.solve(A, b).astype(ld)
    for _ in range(2):
        x = x + np.linalg.solve(A, (bl - Al @ x).astype(np.float64)).astype(ld)
    return x


def chain(manip: Manipulator, q: np.ndarray, solves: list[RbfSolve], block: np.ndarray, n_deform: int):
    """RBF accumulator block -> (body wrenches [nb,6] in the δc = -(ω·M + v·F)
    convention, ∂c/∂δ [3·n_deform]); q normalized as for `solve`.

    From the adjoint solve to the wrench sums the arithmetic is np.longdouble,
    rounded to float64 once at the end: the centre forces G cancel heavily in
    the wrenches (two_link_arm's 46-centre skin: |G| = 7.8e4 against a wrench of
    15, on a system of cond 7.7e4), so in float64 the result carries ~2e-11 of
    rounding noise — harmless for a gradient, but visible once the chain is
    used as a linear map (state_map: the unit blocks' gradients must add up to
    the gradient of their sum)."""
    ld = np.longdouble
    T = manip.mechanism.body_transforms(q)
    nb = manip.mechanism.num_bodies
    wrench = np.zeros((nb, 6), ld)
    gdef = np.zeros(3 * n_deform)
    off = 0
    for r in solves:
        n = r.n
        acc = np.asarray(block[off: off + 4 * n + 4], np.float64)
        off += 4 * n + 4
        lam, E = acc[: n + 4], acc[n + 4:].reshape(n, 3).astype(ld)
        mu = _solve_refined(r.M.T, lam)
        C, u = r.centres.astype(ld), r.u.astype(ld)
        w, b = u[:n], u[n + 1:]
        mw, mb = mu[:n], mu[n + 1:]
        d = C[:, None, :] - C[None]                            # c_j - c_i
        gphi = 3 * np.sqrt((d * d).sum(-1))[..., None] * d     # ∇φ(c_j - c_i)
        term = (w[:, None] * np.einsum("i,jid->jd", mw, gphi) + mw[:, None] * np.einsum("i,jid->jd", w, gphi)
                + mw[:, None] * b[None] + w[:, None] * mb[None])
        G = E - term                                           # ∂c/∂c_j (world)
        np.add.at(wrench[:, :3], r.bodies, -G)
        np.add.at(wrench[:, 3:], r.bodies, -np.cross(C, G))
        for j in range(n):
            if r.deform_rows[j] >= 0:                          # c_j = R_B (p_j + δ_j) + t_B
                row = r.deform_rows[j]
                gdef[3 * row: 3 * row + 3] = (T[r.bodies[j]].R.T.astype(ld) @ G[j]).astype(np.float64)
    return wrench.astype(np.float64), gdef


# ---- Gauss-Newton for skins (include/flashsdf.h "Gauss-Newton for RBF skins") ----
def skin_jacobian(centres, u, pts, dtype=np.float64):
    """Rows j(p) [N, 4n+4] of the skin's residual s = f/|∇f| in the skin's
    parameters, laid out as its accumulator block: ∂s/∂w [n], ∂s/∂a, ∂s/∂b [3],
    ∂s/∂c [n][3] with the coefficients held fixed — rbf_adjoint's summands
    (csrc/rbf_sdf.h) without the factor 2s, so the block is Σ 2 s(p) j(p) and
    the skin's second moment Σ j jᵀ (csrc/skin_moments.hip). dtype: the
    arithmetic's (np.longdouble measures float64's own rounding)."""
    C = np.asarray(centres, dtype)
    u = np.asarray(u, dtype)
    x = np.asarray(pts, dtype).reshape(-1, 3)
    n = len(C)
    w, a, b = u[:n], u[n], u[n + 1:]
    d = x[:, None, :] - C[None]                                   # [N,n,3]
    rho = np.sqrt((d * d).sum(-1))
    f = (w[None] * rho ** 3).sum(1) + a + (x * b[None]).sum(1)
    g = (3 * (w[None] * rho)[..., None] * d).sum(1) + b[None]
    G = np.sqrt((g * g).sum(1))
    dsdf = 1 / G
    uu = -(f / G ** 3)[:, None] * g                                # ∂s/∂∇f
    e = (d * uu[:, None, :]).sum(-1)                               # [N,n]
    Jw = dsdf[:, None] * rho ** 3 + 3 * rho * e
    with np.errstate(invalid="ignore", divide="ignore"):
        k1 = 3 * rho * dsdf[:, None] + np.where(rho > 0, 3 * e / np.where(rho > 0, rho, 1), 0)
    Jc = -w[None, :, None] * (k1[..., None] * d + 3 * rho[..., None] * uu[:, None, :])
    Jb = dsdf[:, None] * x + uu
    return np.concatenate([Jw, dsdf[:, None], Jb, Jc.reshape(len(x), 3 * n)], axis=1)


def state_map(manip: Manipulator, x: np.ndarray, solve_r: RbfSolve, n_deform: int | None = None) -> np.ndarray:
    """L [nx, 4n+4] of one skin at the caller's (un-normalised) x = [q; δ]:
    ∂s/∂x = L j. Column k is the gradient `chain` + Mechanism.config_gradient
    give for the unit block e_k — the map the gradient applies to the skin's
    accumulator block, signs and quaternion projection included
    (fsdf_rbf_state_map is the native form)."""
    mech = manip.mechanism
    nq = mech.num_positions
    nd = manip.num_deformations() if n_deform is None else n_deform
    x = np.asarray(x, np.float64)
    qn = mech.normalize(x[:nq])
    m = 4 * solve_r.n + 4
    L = np.empty((nq + 3 * nd, m))
    for k in range(m):
        block = np.zeros(m)
        block[k] = 1.0
        wrench, gdef = chain(manip, qn, [solve_r], block, nd)
        L[:nq, k] = mech.config_gradient(x[:nq], wrench)
        L[nq:, k] = gdef
    return L


def gauss_newton(manip: Manipulator, x: np.ndarray, solves: list[RbfSolve], skin_moments, hull_moments=None,
                 weight: float = 0.0) -> np.ndarray:
    """The Gauss-Newton Hessian [nx, nx] of c = Σ d*² + weight Σ|δ|²:
    2 (A_hulls + Σ_r L_r M_r L_rᵀ) + 2·weight·I on the deformation
    coordinates. skin_moments: one [m_r, m_r] per skin, in surface order;
    hull_moments [S, 21] (None: no hull term) through
    Mechanism.gauss_newton_matrix, RBF surfaces without a body."""
    from .core import ConvexGeometry
    mech = manip.mechanism
    nq = mech.num_positions
    nd = manip.num_deformations()
    x = np.asarray(x, np.float64)
    A = np.zeros((nq + 3 * nd, nq + 3 * nd))
    if hull_moments is not None:
        sb = np.array([s.body if isinstance(s, ConvexGeometry) else -1 for s in manip.surfaces], np.int32)
        A[:nq, :nq] = mech.gauss_newton_matrix(x[:nq], sb, hull_moments)
    for r, M in zip(solves, skin_moments):
        L = state_map(manip, x, r, nd)
        A += L @ np.asarray(M, np.float64) @ L.T
    H = 2.0 * A
    i = np.arange(nq, nq + 3 * nd)
    H[i, i] += 2.0 * weight
    return H
