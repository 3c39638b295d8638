"""Shared by the Gauss-Newton / Levenberg-Marquardt tests: scenes, the point
vectors w = (∇d*, p × ∇d*), plain-numpy moments, and the cost / gradient /
Gauss-Newton Hessian of a scene evaluated through the CPU oracle."""
import numpy as np

IU = np.triu_indices(6)  # the 21 upper-triangle slots, row-major


def floating_irb_table():
    """IRB140 on a QuaternionFloating base plus the floating table box
    (examples/irb_and_squishable.ipynb cells 3-4 without the RBF skin): a
    rigid scene with two quaternion joints, 20 states."""
    from flash import Models
    from flash.mechanism import QuaternionFloating
    m = Models.irb140()
    m.mechanism.change_joint_type(1, QuaternionFloating("base_link_floating"))
    Models.merge(m, Models.table())
    x0 = np.array(m.mechanism.zero_configuration(), np.float64)
    for name, t in (("base_link", (0.0, 0.0, 0.75)), ("table_body", (0.4, 0.0, 0.6))):
        r = m.mechanism.q_range(m.mechanism.body_index(name))
        x0[r.start + 4: r.start + 7] = t
    return m, x0


def floating_scene(n, seed=5):
    """(manipulator, cloud, start) of the floating scene; the start's table
    quaternion is off identity and not normalised."""
    from flash import synthetic
    m, x_true = floating_irb_table()
    r = np.random.default_rng(seed)
    x_true[7:13] = r.uniform(-0.4, 0.4, 6)
    pts = synthetic.depth_cloud(m, x_true, n, seed=seed + 1, frac_box=0.1, frac_surface=0.9, sigma=0.002)
    x0 = x_true.copy()
    x0[7:13] += 0.04
    x0[4:7] += 0.01
    x0[13:17] = [0.999, 0.02, -0.01, 0.03]
    return m, pts, x0


def convergence_case():
    """The issue's case: IRB140, 6,000 noise-free surface points, the start
    perturbed by σ = 0.2 rad."""
    from flash import Models, synthetic
    m = Models.irb140()
    q_true, _ = synthetic.perturbed_configuration(m, 41)
    pts = synthetic.depth_cloud(m, q_true, 6000, seed=42, sigma=0.0, frac_surface=1.0, frac_box=0.0)
    _, q0 = synthetic.perturbed_configuration(m, 41, sigma=0.2)
    return m, pts, np.asarray(q_true, np.float64), np.asarray(q0, np.float64)


def surface_bodies(m):
    return np.array([s.body for s in m.surfaces], np.int32)


def point_vectors(pts, grad):
    """w [n, 6] = (n, p × n) in float64."""
    pts = np.asarray(pts, np.float64)
    grad = np.asarray(grad, np.float64)
    return np.concatenate([grad, np.cross(pts, grad)], axis=1)


def moments_numpy(pts, grad, kstar, S):
    """[S, 21] by plain float64 sums (a reference to ~1e-13, not the exact one)."""
    w = point_vectors(pts, grad)
    out = np.zeros((S, 21))
    for k in range(S):
        wk = w[kstar == k]
        out[k] = (wk.T @ wk)[IU]
    return out


def random_psd_moments(S, seed):
    r = np.random.default_rng(seed)
    out = np.empty((S, 21))
    for k in range(S):
        B = r.normal(size=(6, 6))
        out[k] = (B @ B.T)[IU]
    return out


class OracleCost:
    """x -> (c, ∂c/∂x, 2A) of a rigid scene through the CPU oracle's per-point
    d*, k*, ∇d*, the numpy chain rule and the numpy Gauss-Newton twin."""

    def __init__(self, m, pts):
        import oracle
        self.m = m
        self.om = oracle.OracleModel.from_manipulator(m)
        self.pts = np.ascontiguousarray(pts, np.float64)
        self.sb = surface_bodies(m)

    def per_point(self, x):
        import flash
        mech = self.m.mechanism
        return self.om.skin(flash.hull_poses(self.m, mech.normalize(x)), self.pts)

    def value_and_gradient(self, x):
        x = np.asarray(x, np.float64)
        d, k, g = self.per_point(x)
        mech = self.m.mechanism
        w = point_vectors(self.pts, g) * (2.0 * d)[:, None]
        bw = np.zeros((mech.num_bodies, 6))
        np.add.at(bw, self.sb[k], w)
        return float(d @ d), mech.config_gradient_numpy(x, bw), (d, k, g)

    def __call__(self, x):
        c, gq, (d, k, g) = self.value_and_gradient(x)
        A = self.m.mechanism.gauss_newton_matrix_numpy(x, self.sb, moments_numpy(self.pts, g, k, len(self.sb)))
        return c, gq, 2.0 * A


def branching_scene(name, n=4096):
    """(manipulator, cloud, start) of a tree that branches below the root, one
    box per body — the scenes whose subtree sums run level by level:
      hand  a revolute base link carries a revolute palm, the palm three fingers
            of two links each (8 bodies; the middle finger's first joint is
            Fixed, so a body without coordinates lies inside the ancestor
            walks): three parents at the widest height, the one-wave form
      comb  a revolute spine carries 11 revolute teeth of two revolute leaves
            each (34 bodies, 34 coordinates): 11 parents at one height, more
            than one wave's ten, so a barrier per level
    The boxes are apart at the cloud's configuration (angles within 0.2 rad);
    the start is that configuration perturbed by sigma = 0.05 rad."""
    from flash import Models, synthetic
    from flash.core import ConvexGeometry, Manipulator
    from flash.geometry import Transform
    from flash.mechanism import Fixed, Mechanism, Revolute

    def at(x, y, z):
        return Transform(np.eye(3), np.array([x, y, z], np.float64))

    mech, surfaces = Mechanism("world"), []

    def link(parent, joint, where, label, half, centre):
        b = mech.attach(parent, joint, where, label)
        surfaces.append(ConvexGeometry(Models.box_hull(half), b, at(*centre), label))
        return b

    if name == "hand":
        base = link(0, Revolute([0, 0, 1], "base_joint"), None, "base", (0.15, 0.15, 0.05), (0, 0, 0.05))
        palm = link(base, Revolute([0, 1, 0], "palm_joint"), at(0, 0, 0.15), "palm", (0.2, 0.05, 0.1), (0, 0, 0.15))
        first = []
        for i, x in enumerate((-0.15, 0.0, 0.15)):
            joint = Fixed(f"finger{i}_joint1") if i == 1 else Revolute([1, 0, 0], f"finger{i}_joint1")
            first.append(link(palm, joint, at(x, 0, 0.28), f"finger{i}_link1", (0.03, 0.03, 0.08), (0, 0, 0.1)))
        for i, b in enumerate(first):
            link(b, Revolute([1, 0, 0], f"finger{i}_joint2"), at(0, 0, 0.2), f"finger{i}_link2", (0.03, 0.03, 0.08),
                 (0, 0, 0.1))
        seed = 51
    elif name == "comb":
        spine = link(0, Revolute([0, 0, 1], "spine_joint"), None, "spine", (1.2, 0.04, 0.04), (0, 0, 0))
        teeth = [link(spine, Revolute([1, 0, 0], f"tooth{i}_joint"), at(-1.0 + 0.2 * i, 0, 0.06), f"tooth{i}",
                      (0.05, 0.03, 0.08), (0, 0, 0.1)) for i in range(11)]
        for i, b in enumerate(teeth):
            for side, y in enumerate((-0.07, 0.07)):
                link(b, Revolute([0, 1, 0], f"leaf{i}_{side}_joint"), at(0, y, 0.2), f"leaf{i}_{side}",
                     (0.04, 0.025, 0.05), (0, 0, 0.07))
        seed = 61
    else:
        raise ValueError(name)
    m = Manipulator(mech, surfaces)
    nq = mech.num_positions
    q_true = np.random.default_rng(seed).uniform(-0.2, 0.2, nq)
    pts = synthetic.depth_cloud(m, q_true, n, seed=seed + 1)
    x0 = q_true + np.random.default_rng(seed + 2).normal(0.0, 0.05, nq)
    return m, pts, x0
