#!/usr/bin/env python3
"""Times the light-curve Jacobian of K7 (rjp_ff_grad, totals only) against the only other routes
to the same numbers, in one process on the same buffers:

    python tools/ff_grad_probe.py [--point small|large|both] [--reps N] [--out FILE.json]

small = 256 x 1024 x 256 cells, 8 epochs, 32 channels; large = 512 x 4096 x 512, 32 epochs,
64 channels; dense synthetic fields on the tau layout, the example model's five registered bursts
(n_par = 15), uniformly spaced epochs.  Per point, with HIP events after a warm-up call of every
shape timed:
  grad      one rjp_ff_grad call (F and dF/dtheta, no maps)
  fd_tiles  the 2 n_par rjp_ff_step sweeps of a central difference, forced onto the epoch tiles
            (no launch-time range attached), each with its own perturbed burst set
  fd_mom    the same sweeps with the launch-time moments allowed and the moment cache live (filled
            by an untimed sweep); recorded with the path the library took -- sweeps of fewer than
            12 epochs never take it
Writes one JSON record per point (default profiles/r10_ff_grad_probe.json)."""
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
POINTS = {"small": ((256, 1024, 256), 8, 32), "large": ((512, 4096, 512), 32, 64)}
# the example model's bursts (files/example-model-params.py:51-54): t_0 [yr], half-life [yr],
# peak / steady mass-loss rate, jets
BURSTS = [(0.5, 0.15, 5., "R"), (0.75, 0.15, 5., "B"), (1., 0.45, 2.5, "B"), (2., 0.5, 10., "RB")]


def burst_lists():
    red, blue = [], []
    for t0, hl, chi, which in BURSTS:
        sig = hl * YEAR * 2. / (2. * np.sqrt(2. * np.log(2.)))
        for jet, lst in (("R", red), ("B", blue)):
            if jet in which:
                lst.append([t0 * YEAR, chi - 1., sig])
    return red, blue


def fd_sets(rel=1e-4):
    """The 2 n_par perturbed burst sets of a central difference (t0 by rel sigma, the others by
    rel of themselves)."""
    sets = []
    base = burst_lists()
    for j in range(2):
        for i in range(len(base[j])):
            for c in range(3):
                for sign in (+1., -1.):
                    lists = [[list(b) for b in base[0]], [list(b) for b in base[1]]]
                    b = lists[j][i]
                    b[c] += sign * rel * (b[2] if c == 0 else b[c])
                    sets.append(E.make_bursts(*lists))
    return sets


def timed(fn, reps):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1) / reps


def probe(eng, name, reps):
    shape, n_ep, n_ch = POINTS[name]
    mode = E.RJP_GFF_SCALAR
    eng.use_sorted = False                       # (single-epoch layout: not part of any sweep here)
    fields = eng.synth_fields(shape, 20261018, 0, E.RJP_F64, csize_au=0.5, wide=False,
                              tau_mode=mode, with_em0=False)
    tavg = eng.tavg(fields)
    eng.synchronize()
    fields.temp = None                           # (no sweep below reads the temperature)
    freqs = np.geomspace(1e9, 5e10, n_ch)
    ctau, cflux = E.ff_channel_coeffs(freqs, 0.5, 120., mode, np.full(n_ch, 5.0))
    epochs = [float(t) * YEAR for t in np.linspace(0.2, 3.0, n_ep)]
    base = E.make_bursts(*burst_lists())
    n_par = 3 * (int(base.n[0]) + int(base.n[1]))
    sets = fd_sets()
    assert len(sets) == 2 * n_par
    rec = {"point": name, "shape": list(shape), "epochs": n_ep, "channels": n_ch, "n_par": n_par,
           "reps": reps}

    grad = lambda: eng.ff_grad(fields, base, epochs, mode, tavg, ctau, cflux)
    out = grad()                                 # warm-up
    eng.synchronize()
    rec["grad_ms"] = timed(grad, reps)
    rec["grad_finite"] = bool(torch.isfinite(out[2]).all().item() and
                              torch.isfinite(out[3]).all().item())

    sumA, ftot = eng._f64(n_ep, fields.npix), eng._f64(n_ep, n_ch)
    step_out = (sumA, None, None, None, ftot)

    def sweeps():
        for b in sets:
            eng.ff_step(fields, b, epochs, mode, tavg, ctau, cflux, step_out)

    eng.use_moments, eng.cache_moments = False, False
    eng.ff_step(fields, base, epochs, mode, tavg, ctau, cflux, step_out)      # warm-up
    eng.synchronize()
    rec["fd_tiles_path"] = eng.last_scan_path()[0]
    rec["fd_tiles_ms"] = timed(sweeps, max(1, reps // 2))

    eng.use_moments, eng.cache_moments = True, True
    eng.ff_step(fields, base, epochs, mode, tavg, ctau, cflux, step_out)      # fills the cache
    eng.ff_step(fields, sets[0], epochs, mode, tavg, ctau, cflux, step_out)   # warm-up
    eng.synchronize()
    rec["fd_mom_path"] = eng.last_scan_path()[0]
    rec["fd_mom_ms"] = timed(sweeps, max(1, reps // 2))
    rec["fd_mom_last_path"] = eng.last_scan_path()[0]
    rec["speedup_vs_fd_tiles"] = rec["fd_tiles_ms"] / rec["grad_ms"]
    rec["speedup_vs_fd_mom"] = rec["fd_mom_ms"] / rec["grad_ms"]
    rec["grad_cell_epochs_per_s"] = float(np.prod(shape)) * n_ep / (rec["grad_ms"] * 1e-3)
    del fields
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=("small", "large", "both"), default="both")
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_ff_grad_probe.json"))
    args = ap.parse_args()
    eng = E.RTEngine(0)
    recs = []
    for name in (("small", "large") if args.point == "both" else (args.point,)):
        recs.append(probe(eng, name, args.reps))
        print(json.dumps(recs[-1]), flush=True)
    props = torch.cuda.get_device_properties(0)
    meta = {"device": torch.cuda.get_device_name(0), "cus": props.multi_processor_count,
            "clock_mhz": getattr(props, "clock_rate", 0) / 1e3, "records": recs}
    with open(args.out, "w") as f:
        json.dump(meta, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
