#!/usr/bin/env python3
"""Times K5 (rjp_ff_formal, the formal solution along the line of sight) alone on dense synthetic
fields with a temperature spread (temp_mode 1, power-law Gaunt factor, tau layout):

    python tools/formal_probe.py [--config cfg4|cfg2|both] [--reps N] [--out FILE.json]

cfg4 = 512 x 4096 x 512 cells x 256 channels, cfg2 = 256 x 1024 x 256 x 32 channels, one epoch
with the example bursts.  Prints (and with --out writes) one JSON record per configuration: the
average device time of one call (HIP events, after a warm-up call) and the update rate
(cells x channels / s).  Under `rocprofv3 --kernel-trace --stats` or a `--pmc` pass run it with
--reps 1."""
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
CONFIGS = {"cfg4": ((512, 4096, 512), 256), "cfg2": ((256, 1024, 256), 32)}
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


def probe(eng, cfg, reps):
    shape, nchan = CONFIGS[cfg]
    mode = E.RJP_GFF_POWERLAW
    fields = eng.synth_fields(shape, 20240504, 1, E.RJP_F64, csize_au=0.5, wide=False,
                              tau_mode=mode)
    freqs = np.geomspace(1e9, 5e10, nchan)
    ctau, cflux = E.ff_channel_coeffs(freqs, 0.5, 120., mode)
    b = bursts()
    out = eng._f64(nchan, fields.npix)
    eng.ff_formal(fields, b, YEAR, mode, ctau, cflux, out=out)          # warm-up
    eng.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        eng.ff_formal(fields, b, YEAR, mode, ctau, cflux, out=out)
    ev1.record()
    ev1.synchronize()
    ms = ev0.elapsed_time(ev1) / reps
    updates = float(np.prod(shape)) * nchan
    finite = bool(torch.isfinite(out).all().item())
    return {"config": cfg, "shape": list(shape), "channels": nchan, "reps": reps,
            "ms_per_call": ms, "updates": updates, "updates_per_s": updates / (ms * 1e-3),
            "all_finite": finite}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("cfg4", "cfg2", "both"), default="both")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = E.RTEngine(0)
    recs = []
    for cfg in (("cfg2", "cfg4") if args.config == "both" else (args.config,)):
        recs.append(probe(eng, cfg, args.reps))
        print(json.dumps(recs[-1]), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "records": recs}, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
