"""Generator of tests/golden/sincos_edges.npz: angles at which kin::sincos
(csrc/kin_impl.h) changes branch, with sin and cos from mpmath at 200 bits as
double-double pairs (hi = the nearest double, lo = the nearest double to the
rest), so tests/test_mech_ref.py needs no mpmath at run time.

    python tests/golden/make_sincos_golden.py

At most 2,000 angles, all with |x| < 8.23549136e5 (the fold's threshold):
  * 0, ±2^-28, the thresholds 2^-27, 0.3, 0.78125 and pi/4 with their neighbours
  * k pi/2 + delta for k = 1..40, delta in {0, ±1 ulp, ±1e-9, ±1e-5}, both signs
    of every fourth (the second and third Cody-Waite rounds run next to a
    multiple of pi/2)
  * 3.0, 100.0, 823549.0 and the last double below the threshold
  * fl(k pi/2) for 500 random k up to 5e5, a quarter of them negated
  * uniform draws: 350 in (-pi/4, pi/4), 350 in (-10, 10), 350 below the threshold
"""
import os

import mpmath
import numpy as np

FOLD = 8.23549136e5


def angles():
    h = np.pi / 2
    out = [0.0, 2.0 ** -28, -2.0 ** -28]
    for c in (2.0 ** -27, 0.3, 0.78125, np.pi / 4):
        out += [c, np.nextafter(c, 0.0), np.nextafter(c, 4.0), -c]
    for k in range(1, 41):
        c = k * h
        edge = [c, np.nextafter(c, 0.0), np.nextafter(c, np.inf), c - 1e-9, c + 1e-9, c - 1e-5, c + 1e-5]
        out += edge
        if k % 4 == 0:
            out += [-v for v in edge]
    out += [3.0, 100.0, 823549.0, -823549.0, np.nextafter(FOLD, 0.0)]
    r = np.random.default_rng(20261021)
    k = r.integers(41, 500001, 500).astype(np.float64)
    out += list(k * h * np.where(r.random(500) < 0.25, -1.0, 1.0))
    out += list(r.uniform(-np.pi / 4, np.pi / 4, 350))
    out += list(r.uniform(-10.0, 10.0, 350))
    out += list(r.uniform(-FOLD, FOLD, 350))
    x = np.array(out, np.float64)
    assert len(x) <= 2000 and np.all(np.abs(x) < FOLD)
    return x


def double_double(v):
    hi = float(v)
    return hi, float(v - mpmath.mpf(hi))


def main():
    mpmath.mp.prec = 200
    x = angles()
    s = np.array([double_double(mpmath.sin(mpmath.mpf(float(v)))) for v in x])
    c = np.array([double_double(mpmath.cos(mpmath.mpf(float(v)))) for v in x])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sincos_edges.npz")
    np.savez_compressed(path, x=x, sin_hi=s[:, 0], sin_lo=s[:, 1], cos_hi=c[:, 0], cos_lo=c[:, 1])
    print(f"{len(x)} angles -> {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
