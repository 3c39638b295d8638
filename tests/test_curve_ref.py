"""The numpy Hilbert twin (curve_ref.py) checked by what makes a curve a
Hilbert curve, not against the kernel's code: every key names one cell, keys
h and h+1 name face-adjacent cells, encode inverts decode, the curve runs
from the origin to the far end of the x axis, and an aligned coarse cell's
points share their keys' leading bits (the curve nests)."""
import numpy as np
import pytest

from conftest import rng
from curve_ref import box_of, cells_of, hilbert_decode, hilbert_encode, keys_of


def _adjacent(a, b):
    return np.abs(a - b).sum(-1) == 1


@pytest.mark.parametrize("bits", [1, 2, 3, 4])
def test_exhaustive_small_orders(bits):
    n = 8 ** bits
    h = np.arange(n)
    cells = hilbert_decode(h, bits)
    assert cells.shape == (n, 3) and cells.min() == 0 and cells.max() == (1 << bits) - 1
    flat = (cells[:, 0] << (2 * bits)) | (cells[:, 1] << bits) | cells[:, 2]
    assert np.array_equal(np.sort(flat), h)  # a bijection onto the lattice
    assert np.all(_adjacent(cells[1:], cells[:-1]))  # L1 distance exactly 1
    assert np.array_equal(hilbert_encode(cells, bits), h)
    assert np.array_equal(cells[0], [0, 0, 0]) and np.array_equal(cells[-1], [(1 << bits) - 1, 0, 0])


def test_order_10_adjacency_and_inversion():
    top = 1 << 30
    ranges = [np.arange(70000), np.arange(top - 4096, top), np.sort(rng(31).integers(0, top - 1, 200000))]
    for h in ranges:
        cells = hilbert_decode(h)
        assert cells.min() >= 0 and cells.max() <= 1023
        assert np.array_equal(hilbert_encode(cells), h)
        nxt = np.minimum(h + 1, top - 1)
        step = _adjacent(hilbert_decode(nxt), cells)
        assert np.all(step[h + 1 < top])
    # ... and cell -> key -> cell on random cells
    c = rng(32).integers(0, 1024, size=(200000, 3))
    assert np.array_equal(hilbert_decode(hilbert_encode(c)), c)


def test_order_10_end_points():
    assert np.array_equal(hilbert_decode(np.array([0, (1 << 30) - 1])), [[0, 0, 0], [1023, 0, 0]])
    assert hilbert_encode(np.array([[0, 0, 0]]))[0] == 0
    assert hilbert_encode(np.array([[1023, 0, 0]]))[0] == (1 << 30) - 1


def test_order_10_nests_in_aligned_coarse_cells():
    """The centres of the 32^3 aligned coarse cells (32 fine cells a side): their
    keys' leading 15 bits are a bijection onto [0, 32768) whose successors are
    face-adjacent coarse cells — the order-10 curve visits each coarse cell in
    one run, along an order-5 Hilbert curve."""
    g = np.arange(32)
    coarse = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    k = hilbert_encode(coarse * 32 + 16) >> 15
    assert np.array_equal(np.sort(k), np.arange(32 ** 3))
    along = coarse[np.argsort(k)]
    assert np.all(_adjacent(along[1:], along[:-1]))
    # every fine cell of a coarse cell shares those leading bits
    r = rng(33)
    fine = coarse[:4096] * 32 + r.integers(0, 32, size=(4096, 3))
    assert np.array_equal(hilbert_encode(fine) >> 15, k[:4096])


def test_quantisation():
    """cells_of: truncation towards zero, clamped to [0, 1023]; hi itself and
    everything beyond clamp to 1023, everything below lo to 0; a degenerate
    axis (ext <= 0) is cell 0; box_of is the per-axis minimum and maximum."""
    box = np.array([0.0, 0.0, 0.0, 1024.0, 1024.0, 1024.0])
    p = np.array([[0.0, 0.5, 0.999], [1.0, 1023.0, 1023.999], [1024.0, 1025.0, 3000.0], [-0.5, -1.0, -2048.0]])
    assert np.array_equal(cells_of(p, box), [[0, 0, 0], [1, 1023, 1023], [1023, 1023, 1023], [0, 0, 0]])
    flat = np.array([1.0, 2.0, 3.0, 1.0, 4.0, 3.0])  # x and z degenerate
    assert np.array_equal(cells_of([[1.0, 3.0, 3.0], [5.0, 4.0, -7.0]], flat), [[0, 512, 0], [0, 1023, 0]])
    assert np.array_equal(keys_of(p, box), hilbert_encode(cells_of(p, box)))
    pts = rng(34).normal(size=(100, 3))
    assert np.array_equal(box_of(pts), np.concatenate([pts.min(0), pts.max(0)]))
    assert np.array_equal(box_of(np.zeros((0, 3))), [np.inf] * 3 + [-np.inf] * 3)
