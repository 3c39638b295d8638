"""Without a GPU: the argument checks of fsdf_set_robust_loops,
fsdf_get_robust_loops and fsdf_eval_robust_device on a null context, the
prototypes flash/_lib.py binds them with, and the plumbing of `robust_loops`
through CostFunctor and estimate_state / Tracker / track / multi_start (the
device side: tests/test_gpu_robust_loops.py)."""
import ctypes
import types

import numpy as np

NEW = ("fsdf_set_robust_loops", "fsdf_get_robust_loops", "fsdf_eval_robust_device")


def test_new_calls_reject_a_null_context():
    from flash import _lib
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    v = ctypes.c_int32(7)
    assert lib.fsdf_set_robust_loops(None, 1) == 1  # FSDF_ERR_ARG
    assert lib.fsdf_set_robust_loops(None, 2) == 1
    assert lib.fsdf_get_robust_loops(None, ctypes.byref(v)) == 1 and v.value == 7
    assert lib.fsdf_get_robust_loops(None, None) == 1
    assert lib.fsdf_eval_robust_device(None, None, None, None) == 1
    assert lib.fsdf_last_error(None) == b"null context"


def test_context_wrappers_call_the_library():
    """Context.set_robust_loops / get_robust_loops / eval_robust_device hand their arguments to the
    three calls (a stand-in library: no device)."""
    from flash import _lib
    seen = []

    def ok(name):
        def call(*a):
            seen.append((name,) + tuple(getattr(x, "value", x) for x in a[1:]))
            if name == "fsdf_get_robust_loops":
                a[1]._obj.value = 1
            return 0
        return call

    c = _lib.Context.__new__(_lib.Context)
    c._ctx, c.K = ctypes.c_void_p(1), 2
    c._lib = types.SimpleNamespace(**{n: ok(n) for n in NEW})
    c.set_robust_loops(True)
    assert c.robust_loops is True and seen[-1] == ("fsdf_set_robust_loops", 1)
    c.set_robust_loops(0)
    assert c.robust_loops is False and seen[-1] == ("fsdf_set_robust_loops", 0)
    assert c.get_robust_loops() is True
    c.eval_robust_device(np.zeros((2, 12)), 4096)
    assert seen[-1][0] == "fsdf_eval_robust_device" and seen[-1][2:] == (4096, None)
    c.eval_robust_device(np.zeros((2, 12)), 4096, 8192)
    assert seen[-1][2:] == (4096, 8192)
    c._ctx = ctypes.c_void_p()  # (nothing to destroy)


def test_functor_applies_the_switch_and_reapplies_it_to_a_shared_engine():
    from flash.gradientdescent import CostFunctor
    seen = []
    ctx = types.SimpleNamespace(loss=None, robust_skins=False, robust_loops=False)

    def set_robust_loops(on):
        ctx.robust_loops = on
        seen.append(("set_robust_loops", on))

    ctx.set_robust_loops = set_robust_loops
    cf = CostFunctor.__new__(CostFunctor)
    cf._native, cf.rigid, cf.robust_skins, cf.robust_loops, cf.loss, cf.ctx = True, True, False, False, None, ctx
    cf._assert_loss()
    assert seen == []
    cf.set_robust_loops(True)
    assert cf.robust_loops is True and seen == [("set_robust_loops", True)]
    ctx.robust_loops = False  # (another functor of the same engine turned it off)
    cf._assert_loss()
    assert seen[-1] == ("set_robust_loops", True) and len(seen) == 2
    cf.set_robust_loops(False)
    assert cf.robust_loops is False and seen[-1] == ("set_robust_loops", False)
    cf2 = CostFunctor.__new__(CostFunctor)
    cf2._native = False
    try:
        cf2.set_robust_loops(True)
        raise AssertionError("a scene that is not native-capable has no device loop")
    except NotImplementedError:
        pass


def test_front_end_hands_robust_loops_to_the_functor(monkeypatch):
    """estimate_state / Tracker (step and relocalize) / track / multi_start build their functor with
    robust_loops=True when asked, and as before when not."""
    from flash import tracking
    from flash.robust import Huber
    made = []

    class FakeCost:
        _native, rigid, n_points = True, True, 4

        def __init__(self, manipulator, pts, device=0, precision=64, robust_skins=False, **kw):
            self.kw, self.calls = kw, []
            made.append(self)

        def set_loss(self, loss):
            self.calls.append(("set_loss", loss))

        def set_sensed_points(self, pts):
            pass

        def descend(self, x, *a):
            self.calls.append(("descend",))
            return x, 0.0, 1

        def score(self, X):
            return np.arange(len(X), dtype=np.float64)

        def __call__(self, x):
            return 0.0

    monkeypatch.setattr(tracking, "CostFunctor", FakeCost)
    monkeypatch.setattr(tracking, "num_states", lambda m: 3)
    solver = tracking.NaiveSolver(3, iteration_limit=1)
    loss = Huber(0.01)
    pts = np.zeros((4, 3))
    tracking.estimate_state(None, pts, np.zeros(3), solver=solver, loss=loss, robust_loops=True)
    assert made[-1].kw == {"robust_loops": True} and made[-1].calls == [("set_loss", loss), ("descend",)]
    tracking.estimate_state(None, pts, np.zeros(3), solver=solver, loss=loss)
    assert made[-1].kw == {}
    x, info = tracking.multi_start(None, pts, np.zeros((2, 3)), solver=solver, loss=loss, robust_loops=True)
    assert made[-1].kw == {"robust_loops": True} and info["chosen"] == 0
    tracking.multi_start(None, pts, np.zeros((2, 3)), solver=solver, loss=loss)
    assert made[-1].kw == {}
    state = types.SimpleNamespace()
    monkeypatch.setattr(tracking, "flatten", lambda s: np.zeros(3))
    monkeypatch.setattr(tracking, "unflatten", lambda s, x: None)
    tr = tracking.Tracker(None, state, solver, loss=loss, robust_loops=True)
    assert made[-1].kw == {"robust_loops": True} and tr.robust_loops is True
    count = len(made)
    tr.step(pts)
    tr.relocalize(pts, candidates=np.zeros((2, 3)), solver=solver)
    assert len(made) == count  # (step and relocalize run on the Tracker's own functor, which carries the switch)
    assert tracking.Tracker(None, state, solver).robust_loops is False and made[-1].kw == {}
    xs, tr = tracking.track(None, [pts], state, solver, loss=loss, robust_loops=True)
    assert made[-1].kw == {"robust_loops": True} and len(xs) == 1
    xs, tr = tracking.track(None, [pts], state, solver, loss=loss)
    assert made[-1].kw == {}
