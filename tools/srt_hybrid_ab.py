#!/usr/bin/env python3
"""Same-buffer A/B of the hybrid single-epoch scan between builds of librjprt: every library scans
the SAME fields, bucketed layout and moments (cfg4, 512 x 4096 x 512, the example bursts) in ONE
process, alternating, at 1.0, 0.3 and 2.6 yr (the last takes the grid order in every build).  Per
build: the time of one rjp_ff_scan (chi table + coefficients + scan, HIP events, `--reps` launches
per round), the (contracted, read) counters with the residual bins and fallback cells where the build has
them, and the worst relative difference of its map from the first named build's.

    python tools/srt_hybrid_ab.py --out ab.json parent=rajepy_amd/librjprt_parent.so \\
        trunc=rajepy_amd/librjprt_trunc.so pair=rajepy_amd/librjprt_pair.so

(the default build takes part as "new"; the variants are builds with -DRJP_SRT_PAIR=0 /
-DRJP_SRT_TRUNC=0 / -DRJP_SRT_DIAG=0 / -DRJP_SRT_OWNROWS=0 / -DRJP_SRT_CODES=0, see
ff_scan_tab.hip -- three libraries on one allocation: parent=..., codes0=... and "new"; a build without
the counters, RJP_SRT_DIAG=0, reports whatever its slots held; --no-moments times the moment-free
ff_scan_sorted_kernel of every build instead)
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from oracle import rt_oracle as orc  # noqa: E402
from rajepy_amd import _lib, engine as E  # noqa: E402
from tests import gpu_util as U  # noqa: E402

SHAPE = (512, 4096, 512)
SEED = 20240507


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="name=path of further builds; the first is the yardstick")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-moments", action="store_true",
                    help="scan without the layout's moments: every build runs ff_scan_sorted_kernel")
    args = ap.parse_args()
    eng = E.RTEngine(0)
    mode = E.RJP_GFF_SCALAR
    builds = []
    for spec in args.libs:
        name, path = spec.split("=", 1)
        lib = C.CDLL(os.path.abspath(path))
        for fn_name, (res, argt) in _lib.SIGNATURES.items():
            if not hasattr(lib, fn_name):       # (an older build: an entry point added since)
                continue
            fn = getattr(lib, fn_name)
            fn.restype, fn.argtypes = res, argt
        assert lib.rjp_version() == _lib.RJP_VERSION
        ctx = C.c_void_p()
        assert lib.rjp_ctx_create(0, C.byref(ctx)) == 0
        builds.append((name, lib, ctx))
    builds.append(("new", eng.lib, eng.ctx))
    bursts = E.make_bursts(*U.example_burst_lists())
    fields = eng.synth_fields(SHAPE, SEED, 0, E.RJP_F64, csize_au=0.5, tau_mode=mode, wide=False,
                              with_em0=False)
    assert fields.srt is not None and fields.srt["mom"] is not None
    nx, ny, nz = SHAPE
    P = fields.npix
    work = eng._workspace(eng.lib.rjp_ff_scan_workspace(nx, ny, nz, 1))
    eng.use_srt_moments = not args.no_moments
    fs = eng._scan_struct(fields, bursts, 1)
    res = {"shape": SHAPE, "K": fields.srt["K"], "N": int(fs.srt_N), "reps": args.reps,
           "rounds": args.rounds, "epochs": {}}
    packed = fields.srt.get("packed") or {}
    res["build_ms"] = {"layout": fields.srt["build_ms"], "moments": fields.srt["mom_build_ms"],
                       "packed": packed.get("build_ms"), "codes": packed.get("pc_build_ms")}
    res["codes_attached"] = bool(fs.d_srt_pc)
    for years in (1.0, 0.3, 2.6):
        ep = _lib.dbl_array([years * orc.YEAR])
        maps = {name: eng._f64(1, P) for name, _, _ in builds}

        def run(name, lib, ctx, reps):
            ms = C.c_double()
            st = lib.rjp_time_ff_scan(ctx, C.byref(fs), C.byref(bursts), ep, 1, mode,
                                      maps[name].data_ptr(), None, None, work.data_ptr(),
                                      work.numel(), eng._stream(), reps, C.byref(ms))
            assert st == 0, (name, lib.rjp_last_error(ctx))
            return ms.value
        row = {}
        for name, lib, ctx in builds:
            run(name, lib, ctx, 2)
            c, r = C.c_int64(), C.c_int64()
            assert lib.rjp_last_srt_bins(ctx, C.byref(c), C.byref(r)) == 0
            row[name] = {"ms": [], "layout": int(lib.rjp_last_scan_layout(ctx)),
                         "bins_contracted_read": [int(c.value), int(r.value)]}
            if hasattr(lib, "rjp_last_srt_resid"):
                row[name]["bins_residual"] = int(lib.rjp_last_srt_resid(ctx))
            if hasattr(lib, "rjp_last_srt_fallbacks"):
                row[name]["cells_fallback"] = int(lib.rjp_last_srt_fallbacks(ctx))
        for _ in range(args.rounds):
            for name, lib, ctx in builds:
                row[name]["ms"].append(run(name, lib, ctx, args.reps))
        eng.synchronize()
        ref = maps[builds[0][0]]
        for name, _, _ in builds:
            ms = np.array(row[name]["ms"])
            row[name].update(ms_mean=float(ms.mean()), ms_min=float(ms.min()), ms_max=float(ms.max()),
                             rel_vs_first=float(((maps[name] - ref).abs() / ref).max().item()))
        res["epochs"]["%.1f_yr" % years] = row
        print(json.dumps({"%.1f_yr" % years: row}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
