#!/usr/bin/env python3
"""Times K22 (rjp_gaincal: StefCal for every (map, solution interval) at once -- one pass over the
data, then one wave per solution with the whole iteration in one launch, then the residual;
rjp_gain_apply) against torch routes that stay on the device, on the same buffers, in ONE process:

    python tools/gaincal_probe.py [--point vla|small] [--rounds N] [--out FILE.json]

The torch solve does the same work by the same rule: A = sum_t w D conj(M) and B = sum_t w |M|^2
per (map, interval, pair) with `index_add_` over the integrations, the dense Hermitian A and
symmetric B [M S, n, n] filled from the triangle, `ITER` steps of num = A g, den = B |g|^2 as
batched matrix-vector products (`torch.bmm`), h = num / den, g' = h or (h + g) / 2, the reference
rotation, and chi^2 at the start and at the solution from the data.  tol is tiny so that neither
route stops early.  The torch apply is g[sol][:, :, p] conj(g[sol][:, :, q]) V with gathers.
vla = 27 antennas, 2048 intervals of 8 integrations, 8 maps with a shared model (0.74 GB of data);
small = 27 antennas, 64 intervals of 8, 2 maps.  Noise-free data of seeded gains.  Every shape is
warmed up once; then the routes are timed with device events in alternating rounds; minimum, median
and maximum of each are reported with the ratio of the medians and the worst case for K22 (its
slowest round against torch's fastest)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rajepy_amd import engine as E  # noqa: E402

POINTS = {"vla": (27, 2048, 8, 8), "small": (27, 64, 8, 2)}       # antennas, intervals, integrations each, maps
ITER, TOL = 20, 1e-300


def timed(fn):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1), out


def stats(t):
    return {"min": float(np.min(t)), "median": float(np.median(t)), "max": float(np.max(t))}


def torch_stefcal(D, Mod, sol, S, n_ant, p, q, n_iter):
    """D [M, T, nb], Mod [1, T, nb] complex, sol [T] int64 -> (gains [M, S, n], chi2 [M, S, 2])."""
    M, T, nb = D.shape
    ok = torch.isfinite(D.real) & torch.isfinite(D.imag) & torch.isfinite(Mod.real) & \
        torch.isfinite(Mod.imag) & (Mod.abs() > 0)
    zero = torch.zeros((), dtype=D.dtype, device=D.device)
    a = torch.where(ok, D * Mod.conj(), zero)
    b = torch.where(ok, (Mod.real * Mod.real + Mod.imag * Mod.imag).expand(M, T, nb), zero.real)
    A = torch.zeros(M, S, nb, dtype=D.dtype, device=D.device).index_add_(1, sol, a)
    B = torch.zeros(M, S, nb, dtype=torch.float64, device=D.device).index_add_(1, sol, b)
    Af = torch.zeros(M * S, n_ant, n_ant, dtype=D.dtype, device=D.device)
    Bf = torch.zeros(M * S, n_ant, n_ant, dtype=torch.float64, device=D.device)
    Af[:, p, q], Af[:, q, p] = A.reshape(M * S, nb), A.reshape(M * S, nb).conj()
    Bf[:, p, q] = Bf[:, q, p] = B.reshape(M * S, nb)
    g = torch.ones(M * S, n_ant, dtype=D.dtype, device=D.device)

    def chi2(g):
        gt = g.reshape(M, S, n_ant)[:, sol]                                  # [M, T, n]
        r = torch.where(ok, D - gt[:, :, p] * gt[:, :, q].conj() * Mod, zero)
        return torch.zeros(M, S, dtype=torch.float64, device=D.device).index_add_(
            1, sol, (r.real * r.real + r.imag * r.imag).sum(dim=2))

    c0 = chi2(g)
    for k in range(1, n_iter + 1):
        num = torch.bmm(Af, g[:, :, None])[:, :, 0]
        den = torch.bmm(Bf, (g.real * g.real + g.imag * g.imag)[:, :, None])[:, :, 0]
        h = num / den
        g = h if k % 2 else 0.5 * (h + g)
    g = g * (g[:, :1].conj() / g[:, :1].abs())
    return g.reshape(M, S, n_ant), torch.stack([c0, chi2(g)], dim=2)


def probe(eng, name, rounds):
    n_ant, S, L, M = POINTS[name]
    dev = eng.device
    T, nb = S * L, n_ant * (n_ant - 1) // 2
    gen = torch.Generator(device=dev).manual_seed(20260101)
    rnd = lambda *shape: torch.rand(*shape, dtype=torch.float64, device=dev, generator=gen)
    pn, qn = np.triu_indices(n_ant, 1)
    p, q = torch.from_numpy(pn).to(dev), torch.from_numpy(qn).to(dev)
    h_sol = np.repeat(np.arange(S, dtype=np.int32), L)
    sol = torch.from_numpy(h_sol.astype(np.int64)).to(dev)
    Mod = torch.polar(0.5 + 1.5 * rnd(1, T, nb), 2 * np.pi * rnd(1, T, nb))
    G = torch.polar(0.8 + 0.4 * rnd(M, S, n_ant), np.radians(60.) * (2 * rnd(M, S, n_ant) - 1))
    Gt = G[:, sol]
    D = (Gt[:, :, p] * Gt[:, :, q].conj() * Mod).contiguous()
    del Gt
    Dk, Mk = D.reshape(M, T * nb), Mod.reshape(1, T * nb)

    k22 = lambda: eng.gaincal(Dk, Mk, h_sol, n_ant, mode="ap", refant=0, min_bl=4, tol=TOL, n_iter=ITER)
    route = lambda: torch_stefcal(D, Mod, sol, S, n_ant, p, q, ITER)
    app = lambda: eng.gain_apply(Dk, G, h_sol, n_ant, mode="correct")

    def app_route():
        gt = G[:, sol]
        c = gt[:, :, p] * gt[:, :, q].conj()
        return D * c.conj() / (c.real * c.real + c.imag * c.imag)

    got, ref = k22(), route()                                                 # warm-up of every shape
    ga, ra = app(), app_route()
    eng.synchronize()
    gain_diff = float((got["gains"] - ref[0]).abs().max().item())
    chi_diff = float(((got["chi2"][..., 0] - ref[1][..., 0]).abs() / ref[1][..., 0]).max().item())   # at the start
    app_diff = float((ga.reshape(M, T, nb) - ra).abs().max().item())
    del ga, ra
    t_k, t_r, t_a, t_ar = [], [], [], []
    for _ in range(rounds):                                                   # alternating rounds
        t_k.append(timed(k22)[0])
        t_r.append(timed(route)[0])
        t_a.append(timed(app)[0])
        t_ar.append(timed(app_route)[0])
    med = lambda t: float(np.median(t))
    vis_bytes = int(D.numel() * 16)
    return {"point": name, "antennas": n_ant, "intervals": S, "integrations": T, "maps": M, "steps": ITER,
            "rounds": rounds, "vis_bytes": vis_bytes, "workgroups": eng.last_gaincal_workgroups,
            "status": sorted(set(got["status"].cpu().reshape(-1).tolist())),
            "ms_k22": stats(t_k), "ms_torch": stats(t_r),
            "torch_over_k22_median": med(t_r) / med(t_k), "torch_over_k22_worst_case": min(t_r) / max(t_k),
            "ms_apply_k22": stats(t_a), "ms_apply_torch": stats(t_ar),
            "apply_GBps_k22": 2 * vis_bytes / (med(t_a) * 1e-3) / 1e9,
            "apply_torch_over_k22_median": med(t_ar) / med(t_a),
            "apply_torch_over_k22_worst_case": min(t_ar) / max(t_a),
            "gains_max_abs_diff": gain_diff, "chi2_max_rel_diff": chi_diff, "apply_max_abs_diff": app_diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=tuple(POINTS) + ("all",), default="vla")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = E.RTEngine(0)
    recs = []
    for name in (tuple(POINTS) if args.point == "all" else (args.point,)):
        torch.cuda.empty_cache()
        recs.append(probe(eng, name, args.rounds))
        print(json.dumps(recs[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "records": recs}, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
