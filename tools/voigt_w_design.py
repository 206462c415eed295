#!/usr/bin/env python3
"""The accuracy census of rajepy_amd/csrc/voigt_w.h (K24's complex Faddeeva function): the float64
restatement of the device algorithm (tests/voigtfit_ref.py: w_dev) against mpmath at 50 digits,
exp(-z^2) erfc(-i z), the error taken against the modulus, |w_dev - w| / |w|.

    python tools/voigt_w_design.py [--dps 50] [--out FILE.json]

The grid (`grid()`, which tests/test_voigtfit_reference_cpu.py runs too): every a of A_VALUES --
with the path boundary a = 6 and pi / h, each -+ 1e-9 -- and for each more than 2000 u in [0, 1e8],
negatives mirrored: 1200 log-spaced and 600 linear ones over the lattice's range, every node and
half-node of both lattices (multiples of 1/4), the lattice switch points (odd multiples of 1/8), the
path boundary u = sqrt(49 - a^2) and the far-field boundary 1e100, each -+ 1 ulp.  Prints the worst
error per path and per a, and kVoigtWEps = twice the worst, rounded up to two digits.

The restatement itself lives in tests/voigtfit_ref.py, not here, and this tool imports it from
there: the reference that follows the device's trace, the kernel's float64 emulation and this census
must use ONE restatement of voigt_w.h, and the tests may not depend on a file they cannot see change.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import voigtfit_ref as R  # noqa: E402

H = 0.5
A_VALUES = (0.0, 1e-300, 1e-12, 1e-6, 1e-3, 0.03, 0.5, 1.0, 6.0 - 1e-9, 6.0, 6.0 + 1e-9,
            np.pi / H - 1e-9, np.pi / H + 1e-9, 10.0, 1e3, 1e6)


def _ulps(v):
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)])


def grid(a, thin=1):
    """The u of the census for one a (>= 0 only; `census` mirrors them); `thin` keeps every thin-th
    of the log-spaced and linear points (the special points all stay)."""
    special = [np.arange(0, 61) * 0.125]
    if a < 7.0:
        special.append([np.sqrt(49.0 - a * a)])
    special.append([1e100, 1e8])
    u = np.concatenate([np.logspace(-12, 8, 1200)[::thin], np.linspace(0.0, 9.0, 600)[::thin]] +
                       [_ulps(s) for s in special])
    return np.unique(np.abs(u))


def census(dps=50, a_values=A_VALUES, thin=1):
    """-> (worst per path name, worst per a, number of points)"""
    per_path = {p: 0.0 for p in R.PATHS}
    per_a = {}
    n = 0
    for a in a_values:
        u = grid(a, thin)
        u = np.concatenate([u, -u[u > 0][::7]])
        err, path = R.w_error(u, a, dps)
        n += u.size
        per_a[repr(float(a))] = float(err.max())
        for i, p in enumerate(R.PATHS):
            if (path == i).any():
                per_path[p] = max(per_path[p], float(err[path == i].max()))
    return per_path, per_a, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dps", type=int, default=50)
    ap.add_argument("--out")
    args = ap.parse_args()
    per_path, per_a, n = census(args.dps)
    print("%d points" % n)
    for p, e in per_path.items():
        print("path %-12s worst |w_dev - w| / |w| = %.3e" % (p, e))
    for a, e in per_a.items():
        print("a = %-22s worst %.3e" % (a, e))
    worst = max(per_path.values())
    print("worst %.3e -> kVoigtWEps = 2 x worst = %.2e (stated: %.2e)" % (worst, 2 * worst, R.EPS_W))
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"per_path": per_path, "per_a": per_a, "points": n, "worst": worst,
                       "stated_eps_w": R.EPS_W}, f, indent=1)


if __name__ == "__main__":
    main()
