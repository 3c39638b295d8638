"""GPU: the pass kernel's prologue, staging and epilogue change no bit.

The hull table now comes posed (the pose kernel writes every HullRow and the
culling-margin scale; the pass copies the table into LDS), and a k* group's six
wrench sums — in the one-chunk-per-wave kernels the chunk's Σ d² too — come from
ONE packed wave reduction with wave_sum's addition tree. Every case of
tools/record_pass_accum.py (M64, IRB140 and a tetrahedron next to a 112-face
hull; n in 1, 63, 64, 65, 4133; f64 on the one-wave grid and the planned pass,
f32 on the grid; a sorted context's first pass and its seeded pass after
fsdf_regroup_points, and an unsorted context on the shuffled cloud) is compared
bit for bit (uint64 views):

  k*, d*, ∇d*        with the C oracle, as the parity tests do;
  cost, accumulator  with tests/golden/pass_accum_parent.npz, what the parent
                     commit's library computed on the GPU for the same cases.
"""
import importlib.util
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("record_pass_accum", os.path.join(ROOT, "tools", "record_pass_accum.py"))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)


@pytest.fixture(scope="module")
def golden():
    z = np.load(cases.GOLDEN_FILE)
    want = [cases.case_id(s, p, sh, o, n, j) for s, p, sh, o in cases.groups() for n in cases.SIZES
            for j in ((0, 1) if o == "sorted" else (1,))]
    assert list(z["cases"]) == want  # the file was recorded for exactly these cases
    return z


@pytest.fixture(scope="module")
def scenes():
    """Scene data and oracle models, built once (read-only)."""
    return {}


@pytest.fixture(scope="module")
def oracle_ref():
    """(scene, precision, n, pass) -> the oracle's (d*, k*, ∇d*), computed once."""
    return {}


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(_bits(got).reshape(-1) != _bits(want).reshape(-1))[0]
    assert bad.size == 0, (what, bad[:8].tolist(), got.reshape(-1)[bad[:8]].tolist(), want.reshape(-1)[bad[:8]].tolist())


@pytest.mark.parametrize("order", cases.ORDERS)
@pytest.mark.parametrize("precision,shape", cases.CONFIGS)
@pytest.mark.parametrize("scene", cases.SCENES)
def test_pass_bits(scene, precision, shape, order, golden, scenes, oracle_ref, oracle_mod):
    if scene not in scenes:
        data = cases.scene(scene)
        scenes[scene] = (data, oracle_mod.OracleModel(data[0]))
    data, om = scenes[scene]
    for n, j, cloud, poses, (cost, acc, (k, d, g)), kernel in cases.run_group(data, precision, shape, order):
        cid = cases.case_id(scene, precision, shape, order, n, j)
        # the kernels under test: the one-chunk-per-wave pass with the hull's
        # stage image (f64), the planned pass, the grid-stride pass (f32)
        if precision == 64:
            want_kernel = ("pass_kernel<double, 1, true, false, true, false, 256, 4>" if shape == "grid"
                           else "planned_pass_kernel<double, true>")
        else:
            want_kernel = "pass_kernel<float, 1, true, false, false, false, 256, 4>"
        assert kernel == want_kernel, (cid, kernel)
        key = (scene, precision, n, j)
        if key not in oracle_ref:
            oracle_ref[key] = om.skin(poses, cloud, precision=precision)
        od, ok, og = oracle_ref[key]
        assert np.array_equal(k, ok), (cid, np.nonzero(k != ok)[0][:8].tolist())
        _same_bits(d, od, cid + " d*")
        _same_bits(g, og, cid + " grad")
        _same_bits(np.float64(cost), golden["cost:" + cid], cid + " cost")
        _same_bits(acc, golden["acc:" + cid], cid + " accumulator")
