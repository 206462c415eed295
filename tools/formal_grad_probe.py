#!/usr/bin/env python3
"""Times K9 (rjp_ff_formal_grad: the formal-solution light curves AND their Jacobian with respect
to the burst parameters from one walk of the grid, totals only) against the cheapest route to the
same Jacobian without it: n_par + 1 calls of K8 (rjp_ff_formal_sweep), the one-sided differences of
`flux_vs_time(formal=True)`.  ONE process, the same buffers:

    python tools/formal_grad_probe.py [--point A|B|all] [--rounds N] [--out FILE.json]

Dense synthetic fields with a temperature spread (temp_mode 1, power-law Gaunt factor, tau layout)
and the example's five bursts (n_par = 15).  A = 256 x 1024 x 256 cells, 32 epochs x 1 channel;
B = 512 x 4096 x 512 cells, 32 epochs x 2 channels.  Every shape is warmed up once; then the two
routes are timed with HIP events in alternating rounds, and the minimum and maximum of each are
reported with the ratio of the medians and the worst case for the new kernel (its slowest round
against the sweeps' fastest).  The perturbed burst sets of the differenced route are real (each
parameter moved by 1e-6 of its scale), so its launches do the work a user's would.  The record also
says whether K9's light curves are K8's bit for bit."""
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
POINTS = {"A": ((256, 1024, 256), 32, 1), "B": ((512, 4096, 512), 32, 2)}
# the example model's bursts (files/example-model-params.py:51-54): t_0 [yr], half-life [yr],
# peak / steady mass-loss rate, jets
BURSTS = [(0.5, 0.15, 5., "R"), (0.75, 0.15, 5., "B"), (1., 0.45, 2.5, "B"), (2., 0.5, 10., "RB")]


def burst_lists():
    red, blue = [], []
    for t0, hl, chi, which in BURSTS:
        sig = hl * YEAR * 2. / (2. * np.sqrt(2. * np.log(2.)))
        for jet, lst in (("R", red), ("B", blue)):
            if jet in which:
                lst.append((t0 * YEAR, chi - 1., sig))
    return red, blue


def perturbed_sets():
    """The n_par burst sets of a one-sided difference: one of (t0, amp_rel, sigma) moved by 1e-6."""
    red, blue = burst_lists()
    sets = []
    for j, lst in enumerate((red, blue)):
        for i in range(len(lst)):
            for c in range(3):
                new = [list(red), list(blue)]
                b = list(new[j][i])
                b[c] += 1e-6 * (b[2] if c == 0 else b[c])
                new[j][i] = tuple(b)
                sets.append(E.make_bursts(new[0], new[1]))
    return sets


def timed(fn):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1), out


def probe(eng, fields, name, rounds):
    shape, n_ep, nchan = POINTS[name]
    mode = E.RJP_GFF_POWERLAW
    freqs = np.geomspace(5e9, 4e10, nchan)
    ctau, cflux = E.ff_channel_coeffs(freqs, 0.5, 120., mode)
    base = E.make_bursts(*burst_lists())
    moved = perturbed_sets()
    n_par = len(moved)
    epochs = [float(t) for t in np.linspace(0., 4., n_ep) * YEAR]

    def grad():
        return eng.ff_formal_grad(fields, base, epochs, mode, ctau, cflux)

    def sweeps():
        out = [eng.ff_formal_sweep(fields, base, epochs, mode, ctau, cflux, want_maps=False)[1]]
        for b in moved:
            out.append(eng.ff_formal_sweep(fields, b, epochs, mode, ctau, cflux, want_maps=False)[1])
        return out

    g, s = grad(), sweeps()                                    # warm-up of every shape
    eng.synchronize()
    same = bool(torch.equal(g[0], s[0]))
    finite = bool(torch.isfinite(g[1]).all().item()) and bool((g[1] != 0).any().item())
    t_grad, t_sweeps = [], []
    for _ in range(rounds):                                    # alternating rounds
        t_grad.append(timed(grad)[0])
        t_sweeps.append(timed(sweeps)[0])
    updates = float(np.prod(shape)) * n_ep * nchan
    med = lambda v: float(np.median(v))
    return {"point": name, "shape": list(shape), "epochs": n_ep, "channels": nchan, "n_par": n_par,
            "rounds": rounds, "ms_grad_min": min(t_grad), "ms_grad_max": max(t_grad),
            "ms_sweeps_min": min(t_sweeps), "ms_sweeps_max": max(t_sweeps),
            "sweeps": n_par + 1, "ms_one_sweep": med(t_sweeps) / (n_par + 1),
            "speedup_median": med(t_sweeps) / med(t_grad),
            "speedup_worst_case": min(t_sweeps) / max(t_grad),
            "grad_over_one_sweep": med(t_grad) / (med(t_sweeps) / (n_par + 1)),
            "updates_per_s": updates / (med(t_grad) * 1e-3),
            "light_curves_bit_identical_to_k8": same, "jacobian_finite_and_nonzero": finite}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=tuple(POINTS) + ("all",), default="all")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = E.RTEngine(0)
    recs, fields = [], None
    for name in (tuple(POINTS) if args.point == "all" else (args.point,)):
        fields = None
        torch.cuda.empty_cache()
        fields = eng.synth_fields(POINTS[name][0], 20240504, 1, E.RJP_F64, csize_au=0.5, wide=False,
                                  tau_mode=E.RJP_GFF_POWERLAW)
        recs.append(probe(eng, fields, name, args.rounds))
        print(json.dumps(recs[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "records": recs}, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
