#!/usr/bin/env python3
"""Times K23 (rjp_normal_eq: chi^2, gradient and Gauss-Newton matrix from data, model and
derivative stacks; two launches, no atomics) against the torch route that stays on the device, on
the same buffers, in ONE process:

    python tools/normal_eq_probe.py [--samples N] [--rounds N] [--out FILE.json]

The torch route is complex128 on the device: with J [P, n] the selected planes gathered from the
[n_rows, n_par, n_vis] stack (a copy torch needs and K23 does not), r = data - model and w the
weights, N = Re(conj(J) @ (w J)^T), g = Re(conj(J) @ (w r)) and chi^2 = sum w |r|^2; every sample
counts (finite data, positive weights), so both routes do the same arithmetic.  Shapes: n_rows =
16, n_vis = samples / 16, n_par = P + 2 with the selection permuted, P = 9 (three ejections) and 48
(the cap), complex and -- at P = 9 -- real samples.  Every shape is warmed up once; then the routes
are timed with device events in alternating rounds; minimum, median and maximum of each are
reported with the algorithmic bytes 8 n_part (P + 2) + 8 per sample, the rate they imply at K23's
median, the ratio of the medians and the worst case for K23 (its slowest round against torch's
fastest)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rajepy_amd import engine as E  # noqa: E402


def timed(fn):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1), out


def stats(t):
    return {"min": float(np.min(t)), "median": float(np.median(t)), "max": float(np.max(t))}


def torch_route(data, model, dmodel, sel, w):
    R, n_par, V = dmodel.shape
    J = dmodel[:, sel].permute(1, 0, 2).reshape(len(sel), R * V)
    r = (data - model).reshape(-1)
    ww = w.reshape(-1).to(J.dtype)
    wJ = J * ww
    N = (J.conj() @ wJ.T).real
    g = (J.conj() @ (ww * r)).real
    chi2 = (w.reshape(-1) * (r.real * r.real + (r.imag * r.imag if r.is_complex() else 0.0))).sum()
    return chi2, g, N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = E.RTEngine(0)
    gen = torch.Generator(device=eng.device).manual_seed(23)
    R, V = 16, a.samples // 16
    rows = []
    for P, cplx in ((9, True), (48, True), (9, False)):
        dt = torch.complex128 if cplx else torch.float64
        n_par = P + 2
        rnd = lambda *s: torch.randn(*s, dtype=dt, device=eng.device, generator=gen)
        model, dmodel = rnd(R, V), rnd(R, n_par, V)
        data = model + 0.1 * rnd(R, V)
        w = torch.rand(R, V, dtype=torch.float64, device=eng.device, generator=gen) + 0.5
        sel = np.random.default_rng(P).permutation(n_par)[:P].astype(np.int32)
        tsel = torch.from_numpy(sel.astype(np.int64)).to(eng.device)
        k23 = lambda: eng.normal_eq(data, model, dmodel, sel, w)
        ref = lambda: torch_route(data, model, dmodel, tsel, w)
        (c1, g1, N1, n1), (c2, g2, N2) = k23(), ref()
        torch.cuda.synchronize()
        iu = np.triu_indices(P)
        dN = float((N1.cpu() - N2.cpu()[iu]).abs().max() / N2.abs().max())
        assert int(n1) == R * V and dN < 1e-10 and abs(float(c1) / float(c2) - 1) < 1e-10, (int(n1), dN)
        t_k, t_t = [], []
        for _ in range(a.rounds):
            t_k.append(timed(k23)[0])
            t_t.append(timed(ref)[0])
        n_part = 2 if cplx else 1
        nbytes = (8 * n_part * (P + 2) + 8) * R * V
        row = dict(P=P, n_part=n_part, samples=R * V, workgroups=eng.last_normal_eq_workgroups,
                   algorithmic_bytes=nbytes, k23_ms=stats(t_k), torch_ms=stats(t_t),
                   k23_tb_per_s=nbytes / (np.median(t_k) * 1e-3) / 1e12,
                   ratio_of_medians=float(np.median(t_t) / np.median(t_k)),
                   worst_case=float(np.min(t_t) / np.max(t_k)), max_rel_diff_N=dN)
        rows.append(row)
        print(json.dumps(row))
        del model, dmodel, data, w
    out = dict(device=torch.cuda.get_device_name(0), rounds=a.rounds, points=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
