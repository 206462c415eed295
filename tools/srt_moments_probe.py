"""The bucketed layout's Chebyshev moments at cfg4 (512 x 4096 x 512, the bench's map): build time
and bytes per order N, the single-epoch scan at 0.3 / 1.0 / 2.6 yr with contracted bins, with
every bin of the support read (RTEngine.use_srt_moments = False) and in grid order, and the
(contracted, read) bin counters.  Writes JSON to the path given with --out.

    python tools/srt_moments_probe.py --out srt_moments.json [--orders 16 20 24]
    python tools/srt_moments_probe.py --scan-only --reps 20     # a lean run for rocprofv3 --pmc
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from oracle import rt_oracle as orc  # noqa: E402
from tests import gpu_util as U  # noqa: E402

SHAPE = (512, 4096, 512)
SEED = 20240507


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--orders", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scan-only", action="store_true",
                    help="build with the default order, then only `reps` hybrid scans at 1.0 yr")
    args = ap.parse_args()
    from rajepy_amd import engine as E
    eng = E.RTEngine(0)
    mode = E.RJP_GFF_SCALAR
    # the reference example's four bursts (as tests/test_gpu_sorted_layout.py)
    bp = U.example_bursts_params()
    red, blue = [], []
    for t0, hl, chi, which in zip(bp["t_0"], bp["hl"], bp["chi"], bp["which"]):
        sig = hl * orc.YEAR * 2. / (2. * np.sqrt(2. * np.log(2.)))
        for j, lst in (("R", red), ("B", blue)):
            if j in str(which):
                lst.append((t0 * orc.YEAR, chi - 1., sig))
    bursts = E.make_bursts(red, blue)
    fields = eng.synth_fields(SHAPE, SEED, 0, E.RJP_F64, csize_au=0.5, tau_mode=mode,
                              wide=False, with_em0=False)
    if args.scan_only:
        for _ in range(args.reps):
            eng.ff_scan(fields, bursts, [1.0 * orc.YEAR], mode, want_em=False, want_tavg=False)
        eng.synchronize()
        print("layout", eng.last_scan_layout(), "bins (contracted, read)", eng.last_srt_bins())
        return

    def scan_ms(years, sorted_, moments):
        eng.use_sorted, eng.use_srt_moments = sorted_, moments
        try:
            ms = eng.time_ff_scan(fields, bursts, [years * orc.YEAR], mode, reps=args.reps,
                                  want_em=False, want_tavg=False)
            return ms, eng.last_scan_layout(), eng.last_srt_bins()
        finally:
            eng.use_sorted = eng.use_srt_moments = True

    res = {"shape": SHAPE, "reps": args.reps, "orders": {}}
    for N in args.orders:
        eng.srt_N = N
        srt = eng.build_sorted(fields)
        row = {"K": srt["K"], "N": srt["N"], "layout_bytes": srt["bytes"],
               "layout_build_ms": srt["build_ms"], "mom_bytes": srt["mom_bytes"],
               "mom_build_ms": srt["mom_build_ms"], "epochs": {}}
        for years in (1.0, 0.3, 2.6):
            e = {}
            for tag, so, mo in (("hybrid", True, True), ("sorted", True, False),
                                ("grid", False, True)):
                ms, lay, bins = scan_ms(years, so, mo)
                e[tag] = {"ms": ms, "layout": lay, "bins_contracted_read": bins}
            row["epochs"]["%.1f_yr" % years] = e
        res["orders"][str(N)] = row
        print(json.dumps({str(N): row}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
