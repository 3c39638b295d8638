"""Numpy twin of the resident order's keys (csrc/sort.hip): the 3-D Hilbert
curve in Skilling's transpose form (J. Skilling, "Programming the Hilbert
curve", AIP Conf. Proc. 707, 2004), the kernel's quantisation of a point to a
cell of its box, and the bounding box. Shared by test_curve_ref.py (which
validates the curve by its properties: bijection, face adjacency, inversion,
end points, nesting) and test_gpu_resident_order.py (which holds the device
keys, sort and regroup to it, integer for integer).

A key holds `bits` bits per axis, interleaved with x most significant:
bit 3*b+2 of the key is bit b of the transposed x, 3*b+1 of y, 3*b of z."""
import numpy as np


def _deinterleave(h, bits):
    X = np.zeros((3,) + h.shape, np.int64)
    for b in range(bits):
        for a in range(3):
            X[a] |= ((h >> (3 * b + 2 - a)) & 1) << b
    return X


def _interleave(X, bits):
    h = np.zeros(X.shape[1:], np.int64)
    for b in range(bits):
        for a in range(3):
            h |= ((X[a] >> b) & 1) << (3 * b + 2 - a)
    return h


def hilbert_decode(h, bits=10):
    """Keys [...] in [0, 8**bits) -> cells [..., 3] in [0, 2**bits)
    (Skilling's TransposeToAxes)."""
    h = np.asarray(h, np.int64)
    X = _deinterleave(h, bits)
    # Gray decode
    t = X[2] >> 1
    X[2] ^= X[1]
    X[1] ^= X[0]
    X[0] ^= t
    # undo the excess work, coarse to fine
    Q = 2
    while Q != (1 << bits):
        P = Q - 1
        for a in (2, 1, 0):
            hit = (X[a] & Q) != 0
            t = np.where(hit, 0, (X[0] ^ X[a]) & P)
            X[0] ^= np.where(hit, P, t)
            X[a] ^= t
        Q <<= 1
    return np.stack([X[0], X[1], X[2]], axis=-1)


def hilbert_encode(cells, bits=10):
    """Cells [..., 3] in [0, 2**bits) -> keys [...] (Skilling's AxesToTranspose)."""
    c = np.asarray(cells, np.int64)
    X = np.stack([c[..., 0], c[..., 1], c[..., 2]]).copy()
    Q = 1 << (bits - 1)
    while Q > 1:
        P = Q - 1
        for a in range(3):
            hit = (X[a] & Q) != 0
            t = np.where(hit, 0, (X[0] ^ X[a]) & P)
            X[0] ^= np.where(hit, P, t)
            X[a] ^= t
        Q >>= 1
    # Gray encode
    X[1] ^= X[0]
    X[2] ^= X[1]
    t = np.zeros_like(X[0])
    Q = 1 << (bits - 1)
    while Q > 1:
        t ^= np.where((X[2] & Q) != 0, Q - 1, 0)
        Q >>= 1
    X ^= t
    return _interleave(X, bits)


def cells_of(points, box):
    """The kernel's quantisation, in IEEE fp64 and in its operation order:
    u = (p - lo) / ext (0 where ext <= 0), c = trunc(u * 1024) clamped to
    [0, 1023] (clamped before the integer cast). box = (lo xyz, hi xyz)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    box = np.asarray(box, np.float64).reshape(6)
    lo = box[:3]
    ext = box[3:] - lo
    pos = ext > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(pos, (p - lo) / np.where(pos, ext, 1.0), 0.0)
    c = np.clip(np.trunc(u * 1024.0), 0.0, 1023.0)
    return c.astype(np.int64)


def keys_of(points, box):
    return hilbert_encode(cells_of(points, box))


def box_of(points):
    """(lo xyz, hi xyz): per-axis minimum and maximum; (+inf, -inf) of no points."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if len(p) == 0:
        return np.array([np.inf] * 3 + [-np.inf] * 3)
    return np.concatenate([p.min(0), p.max(0)])
