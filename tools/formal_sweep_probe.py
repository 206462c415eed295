#!/usr/bin/env python3
"""Times K8 (rjp_ff_formal_sweep: the formal-solution light curves of E epochs from one walk of the
grid) against the route it replaces, E calls of K5 (rjp_ff_formal) each followed by a nansum of its
maps, in ONE process on the same buffers:

    python tools/formal_sweep_probe.py [--point small1|small4|large2|all] [--reps N] [--out FILE.json]

Dense synthetic fields with a temperature spread (temp_mode 1, power-law Gaunt factor, tau layout)
and the example bursts.  small1 / small4 = 256 x 1024 x 256 cells, 32 epochs x 1 / 4 channels;
large2 = 512 x 4096 x 512 cells, 32 epochs x 2 channels.  Every shape is warmed up once, then both
paths are timed with HIP events.  One JSON record per point: both times, their ratio, the update
rate of the new path (cell-epoch-channels / s) and whether the two light curves agree (the sweep's
totals against the nansums of K5's maps, 1e-12).  Under `rocprofv3 --pmc` run it with --reps 1."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rajepy_amd import engine as E  # noqa: E402

YEAR = 31536000.0
POINTS = {"small1": ((256, 1024, 256), 32, 1), "small4": ((256, 1024, 256), 32, 4),
          "large2": ((512, 4096, 512), 32, 2)}
# the example model's bursts (files/example-model-params.py:51-54): t_0 [yr], half-life [yr],
# peak / steady mass-loss rate, jets
BURSTS = [(0.5, 0.15, 5., "R"), (0.75, 0.15, 5., "B"), (1., 0.45, 2.5, "B"), (2., 0.5, 10., "RB")]


def bursts():
    red, blue = [], []
    for t0, hl, chi, which in BURSTS:
        sig = hl * YEAR * 2. / (2. * np.sqrt(2. * np.log(2.)))
        for jet, lst in (("R", red), ("B", blue)):
            if jet in which:
                lst.append((t0 * YEAR, chi - 1., sig))
    return E.make_bursts(red, blue)


def timed(fn, reps):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1) / reps, out


def probe(eng, fields, name, reps):
    shape, n_ep, nchan = POINTS[name]
    mode = E.RJP_GFF_POWERLAW
    freqs = np.geomspace(5e9, 4e10, nchan)
    ctau, cflux = E.ff_channel_coeffs(freqs, 0.5, 120., mode)
    b = bursts()
    epochs = [float(t) for t in np.linspace(0., 4., n_ep) * YEAR]
    maps = eng._f64(nchan, fields.npix)
    lc_old = eng._f64(n_ep, nchan)

    def new_path():
        return eng.ff_formal_sweep(fields, b, epochs, mode, ctau, cflux, want_maps=False)[1]

    def old_path():
        for e, t in enumerate(epochs):
            eng.ff_formal(fields, b, t, mode, ctau, cflux, out=maps)
            torch.nansum(maps, dim=1, out=lc_old[e])
        return lc_old

    new_path(), old_path()                                   # warm-up of both shapes
    eng.synchronize()
    ms_new, lc_new = timed(new_path, reps)
    ms_old, _ = timed(old_path, reps)
    rel = float(((lc_new - lc_old).abs() / lc_old.abs()).max().item())
    updates = float(np.prod(shape)) * n_ep * nchan
    return {"point": name, "shape": list(shape), "epochs": n_ep, "channels": nchan, "reps": reps,
            "ms_sweep": ms_new, "ms_per_epoch_calls": ms_old, "speedup": ms_old / ms_new,
            "updates": updates, "updates_per_s": updates / (ms_new * 1e-3),
            "light_curves_max_rel_diff": rel, "agree_1e-12": rel <= 1e-12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=tuple(POINTS) + ("all",), default="all")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = E.RTEngine(0)
    recs, fields, have = [], None, None
    for name in (tuple(POINTS) if args.point == "all" else (args.point,)):
        shape = POINTS[name][0]
        if have != shape:
            fields = None
            torch.cuda.empty_cache()
            fields = eng.synth_fields(shape, 20240504, 1, E.RJP_F64, csize_au=0.5, wide=False,
                                      tau_mode=E.RJP_GFF_POWERLAW)
            have = shape
        recs.append(probe(eng, fields, name, args.reps))
        print(json.dumps(recs[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "records": recs}, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
