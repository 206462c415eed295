#!/usr/bin/env python3
"""Same-buffer A/B of the single-epoch STEP (rjp_ff_step: chi table + bin coefficients + scan + map
stage) between builds of librjprt, in the scheme of tools/srt_hybrid_ab.py: every library runs the
SAME fields, bucketed layout, moments and output buffers (cfg4, 512 x 4096 x 512, 256 channels, the
example bursts) in ONE process, alternating.

    python tools/step_ab.py --out profiles/r19_cfg4_step_ab.json parent=<librjprt of the parent> \\
        ahead0=<-DRJP_TABLES_AHEAD=0> early0=<-DRJP_SRT_EARLYIDX=0> half0=<-DRJP_SRT_HALFBATCH=0>

The first named build is the yardstick; the default build takes part as "new".  Per build:

  back_to_back  `--rounds` rounds of `--reps` rjp_ff_step calls enqueued without a synchronisation,
                HIP events around the `--reps`: ms per step of each round (1.0 yr)
  synchronised  single steps, each followed by a stream synchronisation: host wall time per step
  bits          sum_a, tau, flux and ftot against the first build's, bit for bit, at 0.3, 1.0 and
                2.6 yr (the last takes the grid-order table kernel)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from oracle import rt_oracle as orc  # noqa: E402
from rajepy_amd import _lib, engine as E  # noqa: E402
from rajepy_amd.maths import physics as ph  # noqa: E402
from tests import gpu_util as U  # noqa: E402

SHAPE = (512, 4096, 512)
NCHAN = 256
SEED = 20240504


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="name=path of further builds; the first is the yardstick")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shape", type=int, nargs=3, default=SHAPE)
    ap.add_argument("--nchan", type=int, default=NCHAN)
    args = ap.parse_args()
    shape = tuple(args.shape)
    eng = E.RTEngine(0)
    eng.cache_moments = False
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
    fields = eng.synth_fields(shape, SEED, 0, E.RJP_F64, csize_au=0.5, tau_mode=mode, wide=False,
                              with_em0=False)
    assert fields.srt is not None and fields.srt["mom"] is not None
    nx, ny, nz = shape
    P, F = fields.npix, args.nchan
    freqs = np.geomspace(1e9, 5e10, F)
    ctau, cflux = E.ff_channel_coeffs(freqs, 0.5, 120., mode, [ph.gff(nu, 1e4) for nu in freqs])
    ctau, cflux = _lib.dbl_array(ctau), _lib.dbl_array(cflux)
    tavg = eng.tavg(fields)
    work = eng._workspace(eng.lib.rjp_ff_scan_workspace(nx, ny, nz, 1))
    wm = eng._workspace_maps(eng.lib.rjp_ff_maps_workspace(P, 1, F))
    fs = eng._scan_struct(fields, bursts, 1)
    # one set of outputs for every build, and the yardstick's kept beside it
    out = [eng._f64(1, P), eng._f64(1, F, P), eng._f64(1, F, P), eng._f64(1, F)]
    kept = [torch.empty_like(t) for t in out]
    names = ("sum_a", "tau", "flux", "ftot")

    def step(lib, ctx, ep):
        st = lib.rjp_ff_step(ctx, C.byref(fs), C.byref(bursts), ep, 1, mode, tavg.data_ptr(), ctau,
                             cflux, F, out[0].data_ptr(), None, out[1].data_ptr(),
                             out[2].data_ptr(), out[3].data_ptr(), work.data_ptr(), work.numel(),
                             wm.data_ptr(), wm.numel(), eng._stream())
        assert st == 0, lib.rjp_last_error(ctx)

    res = {"shape": shape, "nchan": F, "K": fields.srt["K"], "N": int(fs.srt_N), "reps": args.reps,
           "rounds": args.rounds, "builds": [b[0] for b in builds], "bits": {}}
    # ---- bits against the first build, at three epochs ---------------------------------------
    for years in (0.3, 1.0, 2.6):
        ep = _lib.dbl_array([years * orc.YEAR])
        row = {}
        for i, (name, lib, ctx) in enumerate(builds):
            for t in out:
                t.fill_(float("nan"))
            step(lib, ctx, ep)
            step(lib, ctx, ep)                       # (twice: the second call's tables run ahead)
            eng.synchronize()
            layout = int(lib.rjp_last_scan_layout(ctx))
            if i == 0:
                for k, t in zip(kept, out):
                    k.copy_(t)
                eng.synchronize()
            row[name] = {"layout": "sorted" if layout else "grid"}
            for nm, k, t in zip(names, kept, out):
                row[name][nm + "_bit_equal"] = bool(torch.equal(k.view(torch.int64),
                                                                t.view(torch.int64)))
                ok = torch.isfinite(k) & (k != 0)
                row[name][nm + "_max_rel"] = float(((t - k).abs()[ok] / k.abs()[ok]).max().item())
        res["bits"]["%.1f_yr" % years] = row
        print(json.dumps({"%.1f_yr" % years: row}), flush=True)
    # ---- timing at 1.0 yr, the builds alternating -----------------------------------------------
    ep = _lib.dbl_array([1.0 * orc.YEAR])
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b2b = {name: [] for name, _, _ in builds}
    syn = {name: [] for name, _, _ in builds}
    for name, lib, ctx in builds:                     # warm-up of every build
        for _ in range(3):
            step(lib, ctx, ep)
    eng.synchronize()
    for _ in range(args.rounds):
        for name, lib, ctx in builds:
            ev0.record()
            for _ in range(args.reps):
                step(lib, ctx, ep)
            ev1.record()
            eng.synchronize()
            b2b[name].append(ev0.elapsed_time(ev1) / args.reps)
        for name, lib, ctx in builds:
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                step(lib, ctx, ep)
                eng.synchronize()
            syn[name].append((time.perf_counter() - t0) / args.reps * 1e3)

    def stats(v):
        v = np.array(v)
        return {"ms": [float(x) for x in v], "ms_mean": float(v.mean()), "ms_min": float(v.min()),
                "ms_max": float(v.max())}
    res["back_to_back"] = {n: stats(v) for n, v in b2b.items()}
    res["synchronised"] = {n: stats(v) for n, v in syn.items()}
    res["all_bit_equal"] = all(v for row in res["bits"].values() for b in row.values()
                               for k, v in b.items() if k.endswith("_bit_equal"))
    print(json.dumps({k: res[k] for k in ("back_to_back", "synchronised", "all_bit_equal")}),
          flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    for name, lib, ctx in builds[:-1]:
        lib.rjp_ctx_destroy(ctx)
    eng.close()
    return 0 if res["all_bit_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
