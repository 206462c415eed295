#!/usr/bin/env python3
"""Times K6 (rjp_rrl_formal, the RRL formal solution along the line of sight) against the two
kernels it is built from, in one process on one device with the same dense synthetic fields
(temperature spread: temp_mode 1, power-law Gaunt factor) and the same 256 H66a channels:

    python tools/rrl_formal_probe.py [--config cfg3|cfg2] [--reps N] [--only NAME] [--out FILE.json]

cfg3 = 512 x 2048 x 512 cells x 256 channels, cfg2 = 256 x 1024 x 256 x 256 channels, one epoch
with the example bursts.  Launches: rrl_scan (K3), ff_formal (K5) on the wide fields K6 reads and on the tau layout, rrl_formal
(K6); each is the average device time of one call (HIP events, after a warm-up call).  K6 does one Voigt
evaluation and the continuum's and the line's 1 - e^-x per update where K3 and K5 do one and one:
the acceptance bound is t(rrl_formal) <= t(rrl_scan) + 2 t(ff_formal), with the faster of K5's two
layouts.  Prints (and with --out
writes) one JSON record.  Under a `rocprofv3 --pmc` pass run it with --reps 1 --only rrl_formal."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rajepy_amd import _lib, engine as E  # noqa: E402
from rajepy_amd.maths import rrls  # noqa: E402
from tools.formal_probe import YEAR, bursts  # noqa: E402

CONFIGS = {"cfg3": (512, 2048, 512), "cfg2": (256, 1024, 256)}
NCHAN = 256
NAMES = ("rrl_scan", "ff_formal_wide", "ff_formal_tau", "rrl_formal")


def timed(eng, call, reps):
    call()                                                             # warm-up
    eng.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    for _ in range(reps):
        call()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1) / reps


def probe(eng, cfg, reps, only=None):
    shape = CONFIGS[cfg]
    mode = E.RJP_GFF_POWERLAW
    full = eng.synth_fields(shape, 20240504, 1, E.RJP_F64, csize_au=0.5, with_vy=True,
                            tau_mode=mode)
    # K3 and K6 read the wide fields only; K5 is timed on them too, and on the tau layout it
    # prefers when a model carries one: the bound takes the faster of the two
    fields = E.DeviceFields(shape, E.RJP_F64, 0.5, full.nd, full.xi, full.temp, full.pf, full.ts,
                            full.vy)
    lc = rrls.line_constants("H66a")
    line = _lib.Line(**lc)
    freqs = lc["nu_rest"] - NCHAN * 1e5 / 2. + 1e5 / 2. + np.arange(NCHAN) * 1e5
    ctau, cflux = E.ff_channel_coeffs(freqs, 0.5, 120., mode)
    csrc, hnu_k = E.rrl_channel_coeffs(freqs, 0.5, 120.)
    b = bursts()
    out = eng._f64(NCHAN, fields.npix)
    calls = {
        "rrl_scan": lambda: eng.rrl_scan(fields, b, YEAR, line, freqs),
        "ff_formal_wide": lambda: eng.ff_formal(fields, b, YEAR, mode, ctau, cflux, out=out),
        "ff_formal_tau": lambda: eng.ff_formal(full, b, YEAR, mode, ctau, cflux, out=out),
        "rrl_formal": lambda: eng.rrl_formal(fields, b, YEAR, mode, line, freqs, ctau, csrc, hnu_k,
                                             out=out),
    }
    rec = {"config": cfg, "shape": list(shape), "channels": NCHAN, "reps": reps,
           "updates": float(np.prod(shape)) * NCHAN, "ms_per_call": {}}
    for name in NAMES:
        if only in (None, name):
            rec["ms_per_call"][name] = timed(eng, calls[name], reps)
    ms = rec["ms_per_call"]
    if len(ms) == len(NAMES):
        rec["ff_formal_ms"] = min(ms["ff_formal_wide"], ms["ff_formal_tau"])
        rec["bound_ms"] = ms["rrl_scan"] + 2.0 * rec["ff_formal_ms"]
        rec["within_bound"] = bool(ms["rrl_formal"] <= rec["bound_ms"])
    if "rrl_formal" in ms:
        rec["all_finite"] = bool(torch.isfinite(out).all().item())
        rec["negative_share"] = float((out < 0).double().mean().item())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=tuple(CONFIGS), default="cfg3")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=NAMES, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = E.RTEngine(0)
    rec = probe(eng, args.config, args.reps, args.only)
    print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "records": [rec]}, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
