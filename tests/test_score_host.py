"""CPU: the host side of candidate scoring and multi-start (flash/tracking.py
candidates_around, select_candidates, multi_start's selection over a stub
scorer), argument validation, and the three new entry points' declarations in
the header, the ctypes table and the Julia shim."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("fsdf_score_poses", "fsdf_score_states", "fsdf_score_time")


def _table_and_arm():
    from flash import Models
    return Models.table(), Models.irb140()


def test_candidates_around_is_deterministic_and_keeps_x_first():
    from flash.tracking import candidates_around
    table, arm = _table_and_arm()
    x = np.array([0.3, -1.0, 0.5, 0.0, 1.2, -0.4])
    A = candidates_around(arm, x, 0.2, 16, seed=5)
    assert A.shape == (16, 6) and np.array_equal(A[0], x)
    assert np.array_equal(A, candidates_around(arm, x, 0.2, 16, seed=5))
    assert not np.array_equal(A[1:], candidates_around(arm, x, 0.2, 16, seed=6)[1:])
    # the rows are numpy.random.default_rng(seed)'s standard normals, row by row
    z = np.random.default_rng(5).standard_normal((15, 6))
    assert np.array_equal(A[1:], x + 0.2 * z)
    # a prefix of a larger draw: the same rows
    assert np.array_equal(candidates_around(arm, x, 0.2, 4, seed=5), A[:4])
    assert np.array_equal(candidates_around(arm, x, 0.2, 1, seed=5), x[None, :])


def test_candidates_around_per_coordinate_sigma_and_unit_quaternions():
    from flash.tracking import candidates_around
    table, arm = _table_and_arm()
    x = np.array([0.3, -1.0, 0.5, 0.0, 1.2, -0.4])
    sig = np.array([0.5, 0.0, 0.1, 0.0, 0.0, 0.0])
    A = candidates_around(arm, x, sig, 32, seed=1)
    assert np.array_equal(A[:, [1, 3, 4, 5]], np.broadcast_to(x[[1, 3, 4, 5]], (32, 4)))
    assert A[1:, 0].std() > 3 * A[1:, 2].std() > 0
    # a quaternion-floating state (w, x, y, z, t): every row's block is a unit quaternion, x's too
    xq = np.array([2.0, 0.0, 0.0, 0.0, 0.1, 0.2, 0.3])
    Q = candidates_around(table, xq, 0.3, 20, seed=2)
    assert np.allclose(np.linalg.norm(Q[:, :4], axis=1), 1.0, rtol=0, atol=1e-15)
    assert np.array_equal(Q[0], [1.0, 0.0, 0.0, 0.0, 0.1, 0.2, 0.3])
    assert Q[1:, 4:].std() > 0


def test_candidates_around_validates():
    from flash.tracking import candidates_around
    table, arm = _table_and_arm()
    x = np.zeros(6)
    for bad in (dict(x=np.zeros(5)), dict(count=0), dict(sigma=-0.1), dict(sigma=np.ones(5)), dict(sigma=np.nan),
                dict(sigma=np.ones((2, 6)))):
        kw = dict(x=x, sigma=0.1, count=4)
        kw.update(bad)
        with pytest.raises(ValueError):
            candidates_around(arm, kw["x"], kw["sigma"], kw["count"], 0)


def test_selection_rule_ties_nan_and_keep_beyond_the_batch():
    from flash.tracking import select_candidates
    nan = float("nan")
    s = [3.0, 1.0, nan, 1.0, 0.5, nan, 3.0]
    assert select_candidates(s, 1).tolist() == [4]
    assert select_candidates(s, 3).tolist() == [4, 1, 3]           # equal costs: the lower index first
    assert select_candidates(s, 5).tolist() == [4, 1, 3, 0, 6]
    assert select_candidates(s, 7).tolist() == [4, 1, 3, 0, 6, 2, 5]  # NaN last, by index
    assert select_candidates(s, 100).tolist() == [4, 1, 3, 0, 6, 2, 5]  # keep > B: all of them
    assert select_candidates([nan, nan], 1).tolist() == [0]
    assert select_candidates([-0.0, 0.0], 2).tolist() == [0, 1]
    assert select_candidates([np.inf, nan, 2.0], 3).tolist() == [2, 0, 1]
    with pytest.raises(ValueError):
        select_candidates(s, 0)


class _StubCost:
    """A functor over f(x) = |x − target|² with prescribed scores: what multi_start needs of a
    CostFunctor on its Python-loop path."""
    _native = False

    def __init__(self, target, scores):
        self.target = np.asarray(target, np.float64)
        self.scores = np.asarray(scores, np.float64)
        self.scored = []
        self.starts = []

    def score(self, X):
        self.scored.append(np.array(X))
        return self.scores.copy()

    def value_and_gradient(self, x):
        e = np.asarray(x, np.float64) - self.target
        return float(e @ e), 2.0 * e

    def __call__(self, x):
        return self.value_and_gradient(x)[0]


def test_multi_start_selects_refines_and_reports():
    from flash.tracking import NaiveSolver, _multi_start_on
    nan = float("nan")
    target = np.array([1.0, -2.0])
    X = np.array([[5.0, 5.0], [1.5, -2.0], [0.0, 0.0], [1.0, -2.5], [9.0, 9.0]])
    scores = [50.0, 0.25, nan, 0.25, 200.0]
    cost = _StubCost(target, scores)
    seen = []
    solver = NaiveSolver(2, rate=0.25, max_step=10.0, iteration_limit=3, gradient_convergence_tolerance=0.0)
    x, info = _multi_start_on(cost, 1, X, 3, solver, lambda x_, c_: seen.append(c_))
    assert len(cost.scored) == 1 and np.array_equal(cost.scored[0], X)  # all candidates in ONE scoring call
    assert np.array_equal(info["scores"][[0, 1, 3, 4]], [50.0, 0.25, 0.25, 200.0]) and np.isnan(info["scores"][2])
    assert info["kept"].tolist() == [1, 3, 0]
    assert info["refined_costs"].shape == (3,) and info["refined"].shape == (3, 2)
    # each step halves the error (rate 0.25 on 2 e): three evaluations -> e / 8; equal refined costs
    # of candidates 1 and 3: the better-scored (first kept) one wins
    assert np.allclose(info["refined_costs"], [0.25 / 64, 0.25 / 64, 41.0 + 24.0] / np.array([1, 1, 64.0]))
    assert info["chosen"] == 1 and np.array_equal(x, info["refined"][0])
    assert len(seen) == 9  # the callback saw every refinement evaluation
    # keep beyond the batch: everything is refined, the NaN-scored candidate last
    x, info = _multi_start_on(_StubCost(target, scores), 1, X, 10, solver, None)
    assert info["kept"].tolist() == [1, 3, 0, 4, 2] and info["chosen"] == 1
    # a NaN refined objective never wins
    class _NanFirst(_StubCost):
        def __call__(self, x):
            v = super().__call__(x)
            return nan if v < 0.01 else v
    x, info = _multi_start_on(_NanFirst(target, scores), 1, X, 3, solver, None)
    assert np.isnan(info["refined_costs"][:2]).all() and info["chosen"] == 0


def test_multi_start_validates_before_it_touches_a_device():
    from flash.tracking import _multi_start_on, multi_start
    table, arm = _table_and_arm()
    pts = np.zeros((4, 3))
    for cands in (np.zeros(6), np.zeros((0, 6)), np.zeros((3, 5)), np.zeros((2, 3, 6))):
        with pytest.raises(ValueError):
            multi_start(arm, pts, cands)
    with pytest.raises(ValueError):
        multi_start(arm, pts, np.zeros((3, 6)), keep=0)
    with pytest.raises(ValueError):
        _multi_start_on(_StubCost(np.zeros(2), [1.0]), 1, np.zeros((2, 2)), 1, None, None)  # 1 score, 2 candidates


def test_reexports():
    import flash
    from flash import tracking
    assert flash.multi_start is tracking.multi_start and flash.candidates_around is tracking.candidates_around
    assert hasattr(tracking.Tracker, "relocalize")
    from flash.gradientdescent import CostFunctor
    assert callable(CostFunctor.score)


def _header_protos():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flashsdf.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"^int\s+(fsdf_\w+)\s*\(([^)]*)\)\s*;", text, re.M):
        args = [a.strip() for a in m.group(2).replace("\n", " ").split(",") if a.strip()]
        out[m.group(1)] = [re.sub(r"\s*\w+$", "", a).replace(" *", "*").strip() for a in args]
    return out


def test_new_symbols_agree_in_header_ctypes_and_julia():
    import ctypes
    from flash import _lib
    protos = _header_protos()
    want = {"fsdf_score_poses": ["fsdf_ctx*", "const double*", "int32_t", "double*"],
            "fsdf_score_states": ["fsdf_ctx*", "const double*", "int32_t", "double*"],
            "fsdf_score_time": ["fsdf_ctx*", "double*", "int64_t*"]}
    shim = open(os.path.join(ROOT, "julia", "FlashSDF.jl")).read()
    ok = {"fsdf_ctx*": {ctypes.c_void_p}, "const double*": {ctypes.c_void_p}, "int32_t": {ctypes.c_int32},
          "double*": {ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)}, "int64_t*": {ctypes.POINTER(ctypes.c_int64)}}
    for name in NEW:
        assert protos[name] == want[name], (name, protos[name])
        res, args = _lib._PROTOS[name]
        assert res is ctypes.c_int32 and len(args) == len(want[name])
        for a, c in zip(args, want[name]):
            assert a in ok[c], (name, a, c)
        assert name in _lib.SYMBOLS
        assert re.search(r"ccall\(\(:%s,\s*lib\), Cint," % name, shim), name
    # the header's block documents what the cost is and is not
    text = open(os.path.join(ROOT, "include", "flashsdf.h")).read()
    block = text[text.index("---- scoring candidate states"):text.index("int fsdf_score_time")]
    for phrase in ("a sum, not a mean", "regulariser", "read-only", "FSDF_ERR_STATE", "NaN"):
        assert phrase in block, phrase
