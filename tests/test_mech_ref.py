"""CPU: the host kinematics, chain rule and Gauss-Newton matrix (the code the
device solver loops share through csrc/kin_impl.h and csrc/gn_impl.h) against
tests/mech_ref.py — a forward kinematics written from the header's conventions
alone, differentiated by the complex step — on the shape family of
mech_ref.scene, and kin::sincos against mpmath's sine and cosine
(tests/golden/sincos_edges.npz, made by tests/golden/make_sincos_golden.py)."""
import os

import numpy as np
import pytest

import mech_ref
from conftest import GOLDEN
from gn_helpers import moments_numpy

CASES = mech_ref.all_cases() + [("star_too_large", 0)]
IDS = [mech_ref.case_id(c) for c in CASES]


def _revolute_fan(angles):
    """R[1][0] and R[0][0] of fsdf_tree_transforms for one revolute joint about
    z with identity frames per angle: s exactly (every other term of that
    entry is a product with an exact zero) and 1 − (1 − c)."""
    from flash.mechanism import Mechanism, Revolute
    mech = Mechanism("world")
    for i in range(len(angles)):
        mech.attach(0, Revolute([0, 0, 1], f"j{i}"), None, f"b{i}")
    R, t, _, _ = mech.body_transform_arrays(np.asarray(angles, np.float64))
    assert np.all(t == 0.0) and np.all(R[1:, 2, 2] == 1.0)
    assert np.array_equal(R[1:, 0, 1], -R[1:, 1, 0]) and np.array_equal(R[1:, 0, 0], R[1:, 1, 1])
    return R[1:, 1, 0].copy(), R[1:, 0, 0].copy()


def test_sincos_against_mpmath_golden():
    """Sine below 1 ulp (the bound fdlibm documents for these kernels; odd
    quadrants return ±cos_poly as the sine, so both polynomials are covered),
    R[0][0] = 1 − (1 − c) within 2^-52 of the cosine. Measured on the host:
    0.79 ulp and 1.1e-16."""
    z = np.load(os.path.join(GOLDEN, "sincos_edges.npz"))
    x = z["x"]
    assert 0 < len(x) <= 2000 and np.all(np.abs(x) < mech_ref.FOLD)
    s, c1 = _revolute_fan(x)
    L = np.longdouble
    err = np.abs((s.astype(L) - z["sin_hi"].astype(L)) - z["sin_lo"].astype(L))
    ulp = np.spacing(np.abs(z["sin_hi"]))
    ulps = np.where(err == 0, 0.0, (err / ulp.astype(L)).astype(np.float64))
    cerr = np.abs((c1.astype(L) - z["cos_hi"].astype(L)) - z["cos_lo"].astype(L)).astype(np.float64)
    i, j = int(np.argmax(ulps)), int(np.argmax(cerr))
    print(f"sincos: {len(x)} angles, sine worst {ulps[i]:.3f} ulp at {x[i]!r}, 1-(1-c) worst {cerr[j]:.3e} at {x[j]!r}")
    assert ulps[i] < 1.0
    assert cerr[j] <= 2.0 ** -52
    assert s[x == 0.0][0] == 0.0 and c1[x == 0.0][0] == 1.0


def test_sincos_beyond_the_fold():
    """|x| >= 8.23549136e5: the values of fmod(x, fl(2π)), bit for bit, and
    s² + c² − 1 within 2^-51."""
    x = np.array([823550.0, 1.0e6, 1.0e9, 1.0e15, -823550.0, -1.0e15])
    s, c1 = _revolute_fan(x)
    sf, cf = _revolute_fan(np.fmod(x, mech_ref.TWO_PI_FL))
    assert np.array_equal(s, sf) and np.array_equal(c1, cf)
    L = np.longdouble
    unit = np.abs(s.astype(L) ** 2 + c1.astype(L) ** 2 - 1).astype(np.float64)
    print(f"beyond the fold: |s^2 + c^2 - 1| worst {unit.max():.3e}")
    assert unit.max() <= 2.0 ** -51
    # against the true sine the fold is off by x · 3.9e-17 rad by design
    assert abs(s[1] - np.sin(L(1.0e6))) < 1.0e6 * 4e-17 + 1e-16


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_kinematics_against_fk_ref(case):
    """fsdf_tree_transforms and its numpy twin against fk_ref in np.longdouble
    at the scene's start and at a start with angles from N(0, 1): 1e-14
    absolute (tests/test_kinematics.py's cap). The twin takes numpy's sine of
    what it is given, so beyond the fold (`angles`) it is given the folded
    angle, the fold's documented meaning; the native code folds by itself."""
    m, _, x0 = mech_ref.scene(*case)
    mech = m.mechanism
    xs = [np.array(x0)]
    if case[0] != "angles":
        xs.append(x0 + np.random.default_rng(5).normal(0.0, 1.0, x0.size))
    worst = 0.0
    for x in xs:
        ref = mech_ref.fk_ref(mech, x.astype(np.longdouble))
        twin = mech.body_transform_arrays_numpy(mech_ref.fold_configuration(mech, x))
        for got in (mech.body_transform_arrays(x), twin):
            for a, b in zip(got, ref):
                worst = max(worst, float(np.abs(a.astype(np.longdouble) - b).max()))
    print(f"{mech_ref.case_id(case)}: FK worst |native or twin - fk_ref| {worst:.2e}")
    assert worst <= 1e-14


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_chain_rule_against_twists_ref(case):
    """fsdf_config_gradient and config_gradient_numpy on random body wrenches
    against the complex-step twists: rtol = atol = 1e-12, the absolute term
    scaled by max |g|."""
    m, _, x0 = mech_ref.scene(*case)
    mech = m.mechanism
    bw = np.random.default_rng(11).normal(0.0, 1.0, (mech.num_bodies, 6))
    bw[0] = 0.0
    x = np.array(x0)
    ref = mech_ref.config_gradient_ref(mech, x, bw)
    scale = np.abs(ref).max()
    worst = 0.0
    for g in (mech.config_gradient(x, bw), mech.config_gradient_numpy(x, bw)):
        excess = np.abs(g - ref) / (1e-12 * np.abs(ref) + 1e-12 * scale)
        worst = max(worst, float(excess.max()))
    print(f"{mech_ref.case_id(case)}: chain rule worst |g - ref| / (1e-12 |ref| + 1e-12 max|g|) = {worst:.3e}")
    assert worst <= 1.0


def test_shapes_over_64_coordinates():
    for case in CASES:
        assert (mech_ref.scene(*case)[2].size > 64) == (case[0] in mech_ref.OVER_64), case


@pytest.mark.parametrize("case", [c for c in CASES if c[0] not in mech_ref.OVER_64],
                         ids=[mech_ref.case_id(c) for c in CASES if c[0] not in mech_ref.OVER_64])
def test_gauss_newton_matrix_against_jacobian(case):
    """2 · fsdf_gauss_newton_matrix (from plain-numpy moments of the oracle's
    per-point values) against 2 JᵀJ of the reference's per-point Jacobian:
    1e-12 of the largest entry."""
    m, pts, x0 = mech_ref.scene(*case)
    x = np.array(x0)
    ref = mech_ref.ObjectiveRef(m, pts)
    _, _, _, H = ref(x)
    d, k, g = ref.per_point(x)
    sb = np.array([s.body for s in m.surfaces], np.int32)
    A = m.mechanism.gauss_newton_matrix(x, sb, moments_numpy(pts, g, k, len(sb)))
    err = float(np.abs(2.0 * A - H).max() / np.abs(H).max())
    print(f"{mech_ref.case_id(case)}: Gauss-Newton matrix worst |2A - 2JtJ| / max|H| = {err:.2e}")
    assert err <= 1e-12


@pytest.mark.parametrize("case", [c for c in CASES if c[0] != "star_too_large"],
                         ids=[i for i in IDS if i != "star_too_large"])
def test_rates_leave_half_of_the_coordinates_unclipped(case):
    """The reference's own descent at mech_ref.RATES: in each of its first four
    iterations at least half of the coordinates move by less than max_step,
    and the clouds lost at most 0.1 % of their points to ties (scene())."""
    m, pts, x0 = mech_ref.scene(*case)
    for div in (None, mech_ref.divisors_of(x0.size)):
        tr = mech_ref.reference_descent(m, pts, x0, mech_ref.rate_of(case), divisors=div)
        _check_unclipped(tr)


def _check_unclipped(tr):
    for _, _, _, _, raw in tr:
        assert 2 * np.count_nonzero(np.abs(raw) < mech_ref.MAX_STEP * (1 - 1e-9)) >= raw.size
    assert any(np.abs(raw).max() > 0.0 for *_, raw in tr)


@pytest.mark.parametrize("case", [c for c in CASES if c[0].startswith("chain_") or c[0] == "mixed"],
                         ids=[i for i in IDS if i.startswith("chain_") or i.startswith("mixed")])
def test_reference_accepts_the_first_lm_trial(case):
    """At damping 1 the reference's own trial lowers the reference's own cost
    from the scene's start: the device test then compares an accepted step."""
    m, pts, x0 = mech_ref.scene(*case)
    ref = mech_ref.ObjectiveRef(m, pts)
    c, g, _, H = ref(np.array(x0))
    step, _ = mech_ref.lm_trial_ref(H, g, 1.0, 0.5)
    assert ref.value(x0 + step) < c
