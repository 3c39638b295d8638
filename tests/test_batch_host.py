"""CPU: the host side of the batched gradients and lockstep loops — the new entry
points' declarations in the header, the ctypes table and the Julia shim, and
multi_start(batched=True)'s argument validation and selection over a stub
functor (flash/tracking.py _refine_batched).

The Julia shim's static check (tests/test_julia_shim.py) has no type for a double
by value, so the shim binds the two loops through their _ref forms, which read
the scalars through a pointer (as fsdf_set_loss_ref). The lockstep loops' compaction lives in
csrc/batch_api.hip around a device evaluation and is not reachable without a
device: tests/test_gpu_batch.py holds it to fsdf_lm_minimize and
NaiveSolver.optimize."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("fsdf_batch_robust_poses", "fsdf_batch_states", "fsdf_descend_lm_batch", "fsdf_descend_batch",
       "fsdf_batch_time", "fsdf_descend_lm_batch_ref", "fsdf_descend_batch_ref")
# the five calls in the shim: the two loops through their by-reference forms
IN_SHIM = ("fsdf_batch_robust_poses", "fsdf_batch_states", "fsdf_batch_time", "fsdf_descend_lm_batch_ref",
           "fsdf_descend_batch_ref")


def _header_protos():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flashsdf.h")).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"^int\s+(fsdf_\w+)\s*\(([^)]*)\)\s*;", text, re.M):
        args = [a.strip() for a in m.group(2).replace("\n", " ").split(",") if a.strip()]
        out[m.group(1)] = [re.sub(r"\s*\w+$", "", a).replace(" *", "*").strip() for a in args]
    return out


def test_new_symbols_agree_in_header_ctypes_and_julia():
    from flash import _lib
    protos = _header_protos()
    ctx, cd, d, i32 = "fsdf_ctx*", "const double*", "double*", "int32_t"
    want = {"fsdf_batch_robust_poses": [ctx, cd, i32, d, d, d],
            "fsdf_batch_states": [ctx, cd, i32, d, d, d],
            "fsdf_descend_lm_batch": [ctx, d, i32, i32, "double", "double", "double", "double", d, "int32_t*", d],
            "fsdf_descend_batch": [ctx, d, i32, i32, "double", "double", "double", cd, "double", d, "int32_t*"],
            "fsdf_batch_time": [ctx, d, "int64_t*"],
            "fsdf_descend_lm_batch_ref": [ctx, d, i32, i32, cd, d, "int32_t*", d],
            "fsdf_descend_batch_ref": [ctx, d, i32, i32, cd, cd, d, "int32_t*"]}
    ok = {ctx: {ctypes.c_void_p}, cd: {ctypes.c_void_p}, i32: {ctypes.c_int32}, "double": {ctypes.c_double},
          d: {ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)}, "int32_t*": {ctypes.c_void_p},
          "int64_t*": {ctypes.POINTER(ctypes.c_int64)}}
    shim = open(os.path.join(ROOT, "julia", "FlashSDF.jl")).read()
    for name in NEW:
        assert protos[name] == want[name], (name, protos[name])
        res, args = _lib._PROTOS[name]
        assert res is ctypes.c_int32 and len(args) == len(want[name])
        for a, c in zip(args, want[name]):
            assert a in ok[c], (name, a, c)
        assert name in _lib.SYMBOLS
    for name in IN_SHIM:
        assert re.search(r"ccall\(\(:%s,\s*lib\), Cint," % name, shim), name
    # (every ccall of the shim, these among them, is held to the header by tests/test_julia_shim.py)
    for fn in ("batch_robust_poses", "batch_states", "descend_lm_batch!", "descend_batch!", "batch_time"):
        assert re.search(r"^function %s\(" % re.escape(fn), shim, re.M), fn
    # the header's block documents the contract
    text = open(os.path.join(ROOT, "include", "flashsdf.h")).read()
    block = text[text.index("---- gradients of candidate states"):text.index("int fsdf_batch_time")]
    for phrase in ("bit-identical", "read-only", "FSDF_ERR_STATE", "NaN", "FSDF_BATCH_SLICE_BYTES", "lockstep",
                   "exact zeros", "nor on the slicing", "counts the", "params [4]"):
        assert phrase in block, phrase


def test_state_rows_shapes():
    """Context._state_rows: a single state is a batch of one; a wrong width is a ValueError with the
    mechanism's width in it; without a mechanism any shape goes through to the library's own refusal."""
    from flash import _lib
    c = _lib.Context.__new__(_lib.Context)
    c.nq = 6
    assert c._state_rows(np.zeros(6), "t").shape == (1, 6) and c._state_rows(np.zeros(12), "t").shape == (2, 6)
    assert c._state_rows(np.zeros((3, 6)), "t").shape == (3, 6) and c._state_rows(np.zeros((0, 6)), "t").shape == (0, 6)
    for bad in (np.zeros(5), np.zeros((2, 5)), np.zeros((2, 3, 6))):
        with pytest.raises(ValueError, match=r"\[B, 6\]"):
            c._state_rows(bad, "t")
    del c.nq
    assert c._state_rows(np.zeros(5), "t").shape == (1, 5) and c._state_rows(np.zeros((2, 5)), "t").shape == (2, 5)
    assert c._state_rows(np.zeros(0), "t").shape[0] == 0


def test_library_exports_the_new_symbols():
    from flash import _lib
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name


def test_python_front_ends_exist():
    from flash import _lib
    from flash.gradientdescent import CostFunctor
    from flash.tracking import Tracker, multi_start
    import inspect
    for name in ("batch_robust_poses", "batch_states", "descend_lm_batch", "descend_batch", "batch_time"):
        assert callable(getattr(_lib.Context, name)), name
    for name in ("batch_value_and_gradient", "batch_value_gradient_hessian", "descend_batch", "descend_lm_batch"):
        assert callable(getattr(CostFunctor, name)), name
    assert "prior_weight" in inspect.signature(CostFunctor.descend_lm_batch).parameters
    for fn in (multi_start, Tracker.relocalize):
        p = inspect.signature(fn).parameters["batched"]
        assert p.default is False  # the default path is the one it was


class _StubCost:
    """A functor over f(x) = |x − target|² with prescribed scores and the two lockstep loops
    restated in numpy over it: what multi_start(batched=True) needs of a CostFunctor."""
    _native = True
    rigid = True

    def __init__(self, target, scores):
        self.target = np.asarray(target, np.float64)
        self.scores = np.asarray(scores, np.float64)
        self.scored, self.calls = [], []

    def score(self, X):
        X = np.array(X)
        self.scored.append(X)
        if len(self.scored) == 1:
            return self.scores.copy()
        return ((X - self.target) ** 2).sum(axis=1)  # the refined objectives: one call for all of them

    def __call__(self, x):
        raise AssertionError("the batched path scores the refined states in one call")

    def descend_batch(self, X, iteration_limit, rate, max_step, tolerance=0.0, divisors=None, n_points=1.0):
        self.calls.append(("descend_batch", np.array(X), divisors, n_points))
        X = np.array(X, np.float64)
        for _ in range(iteration_limit):
            g = 2.0 * (X - self.target) / n_points
            X = X + np.clip(-rate * g, -max_step, max_step)
        return X, ((X - self.target) ** 2).sum(axis=1) / n_points, np.full(len(X), iteration_limit, np.int32)

    def descend_lm_batch(self, X, iteration_limit, damping, max_step, tolerance=0.0, n_points=1.0, prior_weight=None):
        self.calls.append(("descend_lm_batch", np.array(X), prior_weight, n_points))
        X = np.broadcast_to(self.target, np.shape(X)).copy()  # (a quadratic: one Newton step)
        return X, np.zeros(len(X)), np.full(len(X), 2, np.int32), np.full(len(X), damping / 10)


def test_multi_start_batched_selects_refines_and_reports():
    from flash.tracking import LevenbergMarquardt, NaiveSolver, _multi_start_on
    nan = float("nan")
    target = np.array([1.0, -2.0])
    X = np.array([[5.0, 5.0], [1.5, -2.0], [0.0, 0.0], [1.0, -2.5], [9.0, 9.0]])
    scores = [50.0, 0.25, nan, 0.25, 200.0]
    cost = _StubCost(target, scores)
    solver = NaiveSolver(2, rate=0.25, max_step=10.0, iteration_limit=3, gradient_convergence_tolerance=0.0,
                         precondition_divisors=2.0)
    x, info = _multi_start_on(cost, 1, X, 3, solver, None, batched=True)
    assert len(cost.scored) == 2 and np.array_equal(cost.scored[0], X)  # candidates, then the refined states
    assert info["kept"].tolist() == [1, 3, 0]  # the selection rule of the default path
    name, started, div, n = cost.calls[0]
    assert len(cost.calls) == 1 and name == "descend_batch"  # ONE lockstep loop for the kept candidates
    assert np.array_equal(started, X[[1, 3, 0]]) and n == 1 and np.array_equal(div, [2.0, 2.0])
    assert set(info) == {"scores", "kept", "refined_costs", "chosen", "refined"}
    assert info["refined"].shape == (3, 2) and np.array_equal(cost.scored[1], info["refined"])
    # each step halves the error: e / 8 after three; equal refined costs: the better-scored one wins
    assert np.allclose(info["refined_costs"], np.array([0.25, 0.25, 65.0]) / 64)
    assert info["chosen"] == 1 and np.array_equal(x, info["refined"][0])
    assert solver.iterations == 3
    # the second-order solver takes the other loop, with its prior
    cost = _StubCost(target, scores)
    lm = LevenbergMarquardt(2, iteration_limit=5, prior_weight=1e-3)
    x, info = _multi_start_on(cost, 7, X, 2, lm, None, batched=True)
    name, started, prior, n = cost.calls[0]
    assert name == "descend_lm_batch" and np.array_equal(started, X[[1, 3]]) and prior == 1e-3 and n == 7
    assert np.array_equal(x, target) and info["chosen"] == 1 and not info["refined_costs"].any()
    assert lm.iterations == 2 and lm.final_damping == lm.damping / 10  # the chosen candidate's
    # device_loop: ignored unless it demands the device loop, which a host loop cannot honour
    _multi_start_on(_StubCost(target, scores), 1, X, 2, LevenbergMarquardt(2, device_loop=True), None, batched=True)
    cost = _StubCost(target, scores)
    with pytest.raises(ValueError, match="require"):
        _multi_start_on(cost, 1, X, 2, LevenbergMarquardt(2, device_loop="require"), None, batched=True)
    assert not cost.scored


def test_multi_start_batched_validates():
    from flash import Models
    from flash.tracking import NaiveSolver, _multi_start_on, multi_start

    class _MySolver(NaiveSolver):
        pass

    X = np.zeros((2, 2))
    good = NaiveSolver(2)
    stub = lambda: _StubCost(np.zeros(2), [1.0, 2.0])  # noqa: E731
    with pytest.raises(ValueError, match="callback"):
        _multi_start_on(stub(), 1, X, 1, good, lambda x, c: None, batched=True)
    with pytest.raises(ValueError, match="NaiveSolver or LevenbergMarquardt"):
        _multi_start_on(stub(), 1, X, 1, _MySolver(2), None, batched=True)
    with pytest.raises(ValueError, match="NaiveSolver or LevenbergMarquardt"):
        _multi_start_on(stub(), 1, X, 1, object(), None, batched=True)
    for attr in ("_native", "rigid"):
        cost = stub()
        setattr(cost, attr, False)
        with pytest.raises(ValueError, match="native rigid"):
            _multi_start_on(cost, 1, X, 1, good, None, batched=True)
        assert not cost.scored  # refused before anything is scored
    # the same solvers and a callback pass the default path's checks (batched=False touches none of this)
    class _Plain(_StubCost):
        _native = False

        def value_and_gradient(self, x):
            return float(x @ x), 2.0 * x

        def __call__(self, x):
            return float(x @ x)

    _multi_start_on(_Plain(np.zeros(2), [1.0, 2.0]), 1, X, 1, _MySolver(2, iteration_limit=1), lambda x, c: None)
    # multi_start itself refuses before it touches a device
    arm = Models.irb140()
    with pytest.raises(ValueError, match="callback"):
        multi_start(arm, np.zeros((4, 3)), np.zeros((3, 6)), batched=True, callback=lambda x, c: None)
    with pytest.raises(ValueError, match="NaiveSolver or LevenbergMarquardt"):
        multi_start(arm, np.zeros((4, 3)), np.zeros((3, 6)), batched=True, solver=_MySolver(6))
