"""bench.py --dump-outputs: the files written for a build-to-build comparison
(host side only: the arrays are made here, no GPU)."""
import os

import numpy as np

from conftest import rng

import bench


def _arrays(n, seed, resident=True):
    g = rng(seed)
    arrs = {"accum": g.standard_normal(1 + 6 * 7),
            "kstar": g.integers(0, 7, n).astype(np.int32),
            "d": g.standard_normal(n),
            "grad": g.standard_normal((n, 3))}
    if resident:
        arrs["perm"] = g.permutation(n).astype(np.int64)
    return arrs


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_in_caller_order(tmp_path):
    n = 1000
    a = _arrays(n, 1)
    bench.write_outputs(str(tmp_path), a, seed=5)
    out = _load(str(tmp_path))
    assert sorted(out) == ["accum", "d", "grad", "kstar"]
    assert out["accum"].dtype == np.float64 and out["d"].dtype == np.float64
    assert out["grad"].dtype == np.float64 and out["kstar"].dtype == np.float32
    assert np.array_equal(out["accum"], a["accum"])
    # resident row i is caller point perm[i]
    assert np.array_equal(out["d"][a["perm"]], a["d"])
    assert np.array_equal(out["grad"][a["perm"]], a["grad"])
    assert np.array_equal(out["kstar"][a["perm"]], a["kstar"].astype(np.float32))


def test_dump_caller_order_written_as_is(tmp_path):
    a = _arrays(257, 2, resident=False)
    bench.write_outputs(str(tmp_path), a, seed=5)
    out = _load(str(tmp_path))
    assert np.array_equal(out["d"], a["d"]) and np.array_equal(out["grad"], a["grad"])


def test_dump_without_per_point_outputs(tmp_path):
    bench.write_outputs(str(tmp_path), {"accum": np.arange(43.0)}, seed=5)
    assert os.listdir(str(tmp_path)) == ["accum.npy"]


def test_large_dump_is_a_fixed_sample_within_the_cap(tmp_path, monkeypatch):
    n = 5000
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 * 1000)
    a = _arrays(n, 3)
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    bench.write_outputs(d1, a, seed=5)
    bench.write_outputs(d2, a, seed=5)
    assert sum(os.path.getsize(os.path.join(d1, f)) for f in os.listdir(d1)) <= 64 * 1000
    o1, o2 = _load(d1), _load(d2)
    assert sorted(o1) == ["accum", "d", "grad", "index", "kstar"]
    for k in o1:
        assert np.array_equal(o1[k], o2[k])
    idx = o1["index"].astype(np.int64)
    assert 1000 < len(idx) < n and np.all(np.diff(idx) > 0)
    inv = np.empty(n, np.int64)
    inv[a["perm"]] = np.arange(n)  # caller index -> resident row
    assert np.array_equal(o1["d"], a["d"][inv[idx]])
    assert np.array_equal(o1["grad"], a["grad"][inv[idx]])
