#!/usr/bin/env python3
"""Times K24 (rjp_voigtfit: one Levenberg-Marquardt fit of Voigt profiles plus a baseline per
sightline, the whole fit of a pixel in one launch) against K21's Gaussian fit (rjp_specfit) on the
SAME cube at the SAME trial count, in ONE process on one allocation:

    python tools/voigtfit_probe.py [--point small|cfg3|all] [--rounds N] [--wing SHARE] [--out FILE.json]

A Voigt trial does strictly more arithmetic than a Gaussian one -- w(u + i a) per channel and
component, one more parameter per component in N and g -- so nothing is asserted on the ratio: the
number says what w(z) costs per channel.  small = 128 x 128 pixels x 64 channels; cfg3 = 512 x 512
pixels x 256 channels (0.54 GB), K21's shapes, each with one component and with two, the baseline
free.  The data are K21's probe's noisy (2 % of the amplitude) lines with a share `--wing` of each
line's peak in Lorentzian wings, so that the Voigt fit has wings to find and the lanes of a wave take
both paths of voigt_w.h (lattice in the core, continued fraction further out); `ITER` trials with
xtol tiny, so that neither kernel stops early: every pixel of BOTH fits must end with status 0 after
`ITER` trials, and the record carries the share that does (`share_status0_*`).  Every shape is warmed
up once; then the two are timed with device events in alternating rounds; minimum, median and
maximum of each are reported with the ratio of the medians."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rajepy_amd import engine as E  # noqa: E402

POINTS = {"small": (128 * 128, 64), "cfg3": (512 * 512, 256)}
ITER, LAM0, XTOL = 12, 1e-3, 1e-300
NOISE = 0.02


def timed(fn):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1), out


def stats(t):
    return [float(min(t)), float(np.median(t)), float(max(t))]


def probe(eng, name, nc, rounds, wing):
    n, Cn = POINTS[name]
    dev = eng.device
    g = torch.Generator(device=dev)
    g.manual_seed(20240524 + nc)
    rnd = lambda lo, hi: lo + (hi - lo) * torch.rand(n, 1, dtype=torch.float64, device=dev, generator=g)
    xh = np.linspace(-60.0, 60.0, Cn)
    x_ref = float(xh[Cn // 2])
    x = torch.from_numpy(xh).to(dev)[None, :]
    b0, b1 = rnd(0.1, 0.3), rnd(0.001, 0.004)
    Y = b0 + b1 * (x - x_ref)
    gauss, voigt = [], []
    for c in range(nc):
        if c == 0:
            A, x0, s = rnd(0.5, 2.0), rnd(-12.0, 12.0), rnd(6.0, 12.0)
        else:
            A, x0, s = rnd(0.3, 0.8), x0 + rnd(28.0, 36.0), rnd(4.0, 8.0)
        gam = rnd(0.5, 1.0) * s
        d = x - x0
        Y = Y + A * ((1.0 - wing) * torch.exp(-0.5 * (d / s) ** 2) + wing * gam * gam / (d * d + gam * gam))
        gauss += [1.2 * A, x0 + 2.0, 1.25 * s]
        voigt += [1.2 * A * ((1.0 - wing) * s * 2.5066282746310002 + wing * np.pi * gam), x0 + 2.0, 1.25 * s,
                  0.5 * gam]
    Y = Y + NOISE * torch.randn(n, Cn, dtype=torch.float64, device=dev, generator=g)
    cube = Y.t().contiguous()                                                 # [C, n]: the cube
    del Y
    thg = torch.cat(gauss + [b0, b1], dim=1).t().contiguous()                 # parameter planes
    thv = torch.cat(voigt + [b0, b1], dim=1).t().contiguous()
    k21 = lambda: eng.specfit(cube, xh, thg, x_ref, n_comp=nc, n_iter=ITER, lambda0=LAM0, xtol=XTOL)
    k24 = lambda: eng.voigtfit(cube, xh, thv, x_ref, n_comp=nc, n_iter=ITER, lambda0=LAM0, xtol=XTOL)
    got21, got24 = k21(), k24()                                               # warm-up of every shape
    eng.synchronize()
    t21, t24 = [], []
    for _ in range(rounds):                                                   # alternating rounds
        t21.append(timed(k21)[0])
        t24.append(timed(k24)[0])
    med = lambda t: float(np.median(t))
    a = (got24["theta"][3] / (got24["theta"][2] * np.sqrt(2.0)))
    return {"point": name, "pixels": n, "channels": Cn, "components": nc, "trials": ITER, "rounds": rounds,
            "cube_bytes": int(cube.numel() * 8), "workgroups": eng.last_specfit_workgroups,
            "wing": wing,
            "share_status0_k21": float((got21["status"] == 0).double().mean().item()),
            "share_status0_k24": float((got24["status"] == 0).double().mean().item()),
            "status_k21": sorted(set(got21["status"].cpu().tolist())),
            "status_k24": sorted(set(got24["status"].cpu().tolist())),
            "niter_k24": sorted(set(got24["niter"].cpu().tolist())),
            "ms_k21": stats(t21), "ms_k24": stats(t24),
            "ns_per_pixel_channel_trial_k21": 1e6 * med(t21) / ITER / (n * Cn),
            "ns_per_pixel_channel_trial_k24": 1e6 * med(t24) / ITER / (n * Cn),
            "ns_per_w_evaluation_upper_bound": 1e6 * (med(t24) - med(t21)) / ITER / (n * Cn * nc),
            "cube_GBps_k24": cube.numel() * 8 * ITER / (med(t24) * 1e-3) / 1e9,
            "k24_over_k21_median": med(t24) / med(t21), "k24_over_k21_worst_case": max(t24) / min(t21),
            "median_chi2_k21": float(got21["chi2"].median().item()),
            "median_chi2_k24": float(got24["chi2"].median().item()),
            "median_fitted_a": float(a.median().item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=tuple(POINTS) + ("all",), default="all")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--wing", type=float, default=0.15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = E.RTEngine(0)
    recs = []
    for name in (tuple(POINTS) if args.point == "all" else (args.point,)):
        for nc in (1, 2):
            torch.cuda.empty_cache()
            recs.append(probe(eng, name, nc, args.rounds, args.wing))
            print(json.dumps(recs[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "records": recs}, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
