"""Generator of tests/golden/k3_voigt.npz: Re w(x + i y) of the Faddeeva function at 40 digits.

    python tests/golden/make_k3_voigt_golden.py          (needs mpmath; a few seconds)

w(z) = exp(-z^2) erfc(-i z) is evaluated with mpmath at 40 digits on the grid below and its real
part rounded to float64.  The grid sits where the Voigt paths of rajepy_amd/csrc/rrl_voigt.h switch
or are at their least accurate:
    y   half-decades from 1e-10 to 1e3, and +-0.5 % around the y thresholds of the paths: 0.03
        (centred lattice), 1.0 (far-field rule), 1.3 (lite pole term), pi/0.675 and pi/0.6 (where the
        pole term of either lattice ends) and 8 (|z|^2 = 64 at x = 0);
    x   on and beside the nodes n h of both lattices (h = 0.6 and 0.675; n h, n h +- h/4 and
        n h +- 1e-6, up to |x| ~ 8), +-2 % around the far-field switches at 8, 14 and 16, and
        40, 1e3, 1e4 in the wings.
The file holds x [nx], y [ny] and rew [ny, nx]: nx * ny <= 6000 triples.
tests/test_k3_voigt_reference_cpu.py holds scipy.special.wofz to it and regenerates a sample.
"""
import os

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "k3_voigt.npz")
DPS = 40
Y_THRESHOLDS = (0.03, 1.0, 1.3, np.pi / 0.675, np.pi / 0.6, 8.0)


def grid():
    y = list(np.geomspace(1e-10, 1e3, 27))
    for t in Y_THRESHOLDS:
        y += [t * (1.0 - 5e-3), t * (1.0 + 5e-3)]
    x = []
    for h, nmax in ((0.6, 13), (0.675, 11)):
        for n in range(nmax + 1):
            x += [n * h, n * h - 0.25 * h, n * h + 0.25 * h, n * h - 1e-6, n * h + 1e-6]
    for c in (8.0, 14.0, 16.0):
        x += [c * f for f in (0.98, 0.995, 1.0, 1.005, 1.02)]
    x += [40.0, 1e3, 1e4]
    x = np.unique(np.array([v for v in x if v >= 0.0]))
    y = np.unique(np.array(y))
    assert x.size * y.size <= 6000
    return x, y


def rew_mp(x, y):
    """Re[exp(-z^2) erfc(-i z)], z = x + i y, at DPS digits from the float64 x and y."""
    import mpmath
    with mpmath.workdps(DPS):
        z = mpmath.mpc(mpmath.mpf(float(x)), mpmath.mpf(float(y)))
        return float(mpmath.re(mpmath.exp(-z * z) * mpmath.erfc(-1j * z)))


def main():
    x, y = grid()
    rew = np.array([[rew_mp(xv, yv) for xv in x] for yv in y])
    np.savez_compressed(OUT, x=x, y=y, rew=rew)
    print("%s: %d x %d points, %d bytes" % (OUT, y.size, x.size, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
