#!/usr/bin/env python3
"""CPU simulation of what a wave of the bucketed single-epoch scan fetches beyond its lanes' own
runs (ff_scan_sorted_kernel / ff_scan_hybrid_kernel, ff_scan_tab.hip).  A group is 64 lanes x
`--ny` cells with i.i.d. uniform launch times over K = 32 bins, as rjp_synth_fields makes them;
a scan reads the bins [b0, b1) of a jet cell by cell: per lane one run of rows, the wave streams
the rows from the smallest start to the largest end of the runs.  Printed per case: rows fetched /
rows needed when
  every lane loads every row of the window           (64 x 16 B per row, whoever needs it),
  a lane loads the rows of its own run only, memory serving whole 128-byte lines (8 lanes),
  the same with 64-byte sectors (4 lanes).
The first three cases are the bins read (not contracted) at cfg4 with the example bursts: red 0-5
and blue 0-3 at 1.0 yr, red 0-1 at 0.3 yr (tests/test_srt_truncation_cpu.coefficient_counts); the
last shows runs that do not start at row 0."""
import argparse

import numpy as np

CASES = (("1.0 yr red", 0, 6), ("1.0 yr blue", 0, 4), ("0.3 yr red", 0, 2), ("ragged starts", 4, 10))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ny", type=int, default=4096)
    ap.add_argument("--groups", type=int, default=400)
    ap.add_argument("--K", type=int, default=32)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    print("%-14s %10s %10s %10s" % ("bins", "every lane", "128-B line", "64-B sector"))
    for name, b0, b1 in CASES:
        need = allrows = lines = sectors = 0
        for _ in range(args.groups):
            bins = rng.integers(0, args.K, (64, args.ny))
            rs = (bins < b0).sum(axis=1)
            re = (bins < b1).sum(axis=1)
            lo, hi = rs.min(), re.max()
            need += int((re - rs).sum())
            allrows += 64 * int(hi - lo)
            for width, tot in ((8, "lines"), (4, "sectors")):
                s = rs.reshape(-1, width).min(axis=1)
                e = re.reshape(-1, width).max(axis=1)
                n = width * int((e - s).sum())
                if tot == "lines":
                    lines += n
                else:
                    sectors += n
        print("%-14s %10.3f %10.3f %10.3f" % ("%s %d-%d" % (name, b0, b1 - 1), allrows / need,
                                              lines / need, sectors / need))


if __name__ == "__main__":
    main()
