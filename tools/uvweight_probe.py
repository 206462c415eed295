#!/usr/bin/env python3
"""Times K15 (rjp_uv_weights: Briggs imaging weights from the fixed-point (u, v) density, one memset
and five launches) against a torch route to the same weights that stays on the device, on the same
buffers, in ONE process:

    python tools/uvweight_probe.py [--point track|cube|all] [--rounds N] [--out FILE.json]

The torch route: `torch.round` (ties to even) of the two products, the range and flag tests, a flat
cell index per (map, visibility), the density by `index_add_` (variant "index_add") or by
`torch.bincount` with weights (variant "bincount") -- float64 atomics, so neither the order-free sum
nor the bitwise invariances of K15 --, the fold `S + S.flip`, `sum W^2`, and a `gather` for
w / (1 + f2 W).  No parent kernel exists, so the FASTER of the two variants is the yardstick.
track = 1 map x 1 263 600 visibilities (351 baselines x 3600 integrations) on 501 x 501;
cube = 64 maps x 65 536 visibilities on 256 x 256, a scale per map.  Baselines peaked at short
spacings (radius ~ uniform^2, up to 0.5 cycles per cell), log-normal weights, 1 % flagged.  Every
shape is warmed up once; then the routes are timed with device events in alternating rounds;
minimum, median and maximum of each are reported with the ratio of the medians, the worst case for
K15 (its slowest round against torch's fastest) and the largest relative difference of a weight."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rajepy_amd import engine as E  # noqa: E402

POINTS = {"track": (501, 501, 1, 351 * 3600), "cube": (256, 256, 64, 65536)}
ROBUST = 0.5


def timed(fn):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1), out


def torch_route(u, v, w, su, sv, nx, nz, variant):
    M = su.numel()
    hx, hz = nx // 2, nz // 2
    nzc, nc = 2 * hz + 1, (2 * hx + 1) * (2 * hz + 1)
    gu = torch.round((su[:, None] * u[None, :]) * nx)
    gv = torch.round((sv[:, None] * v[None, :]) * nz)
    ok = (torch.isfinite(u) & torch.isfinite(v) & torch.isfinite(w) & (w >= 0))[None, :] & \
        (gu.abs() <= hx) & (gv.abs() <= hz)
    idx = torch.where(ok, (gu + hx) * nzc + (gv + hz), torch.zeros_like(gu)).to(torch.int64)
    wk = torch.where(ok, w[None, :].expand_as(gu), torch.zeros_like(gu))
    flat = (idx + nc * torch.arange(M, device=u.device)[:, None]).reshape(-1)
    if variant == "index_add":
        S = torch.zeros(M * nc, dtype=torch.float64, device=u.device).index_add_(0, flat, wk.reshape(-1))
    else:
        S = torch.bincount(flat, weights=wk.reshape(-1), minlength=M * nc)
    S = S.reshape(M, nc)
    W = S + S.flip(1)
    f2 = (5.0 * 10.0 ** -ROBUST) ** 2 * 2.0 * wk.sum(dim=1) / (W * W).sum(dim=1)
    return wk / (1.0 + f2[:, None] * W.gather(1, idx))


def probe(eng, name, rounds):
    nx, nz, M, K = POINTS[name]
    g = torch.Generator(device=eng.device)
    g.manual_seed(20240517)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, device=eng.device, generator=g)
    uni = lambda *s: torch.rand(*s, dtype=torch.float64, device=eng.device, generator=g)
    r, th = 0.5 * uni(K) ** 2, 2.0 * np.pi * uni(K)
    u, v = r * torch.cos(th), r * torch.sin(th)
    w = torch.exp(0.5 * rnd(K))
    w[uni(K) < 0.01] = float("nan")
    su_h = -1.0 / (1.0 + 0.01 * np.arange(M))               # a scale per map, |a| <= 0.5
    sv_h = -su_h
    su, sv = torch.from_numpy(su_h).to(eng.device), torch.from_numpy(sv_h).to(eng.device)

    k15 = lambda: eng.uv_weights(u, v, su_h, sv_h, nx, nz, w=w, mode="briggs", robust=ROBUST)
    routes = {n: (lambda n=n: torch_route(u, v, w, su, sv, nx, nz, n)) for n in ("index_add", "bincount")}
    a = k15()                                                 # warm-up of every shape
    tiles = eng.last_uv_weight_tiles
    stats = eng.last_uv_weight_stats.cpu().numpy()
    diff = {}
    for n, fn in routes.items():
        b = fn()
        live = a > 0
        assert bool(((b > 0) == live).all())
        diff[n] = float(((a - b).abs()[live] / a[live]).max().item())
        del b
    eng.synchronize()
    t = {n: [] for n in ("k15",) + tuple(routes)}
    for _ in range(rounds):                                   # alternating rounds
        t["k15"].append(timed(k15)[0])
        for n, fn in routes.items():
            t[n].append(timed(fn)[0])
    med = lambda x: float(np.median(x))
    best = min(routes, key=lambda n: med(t[n]))
    rec = {"point": name, "nx": nx, "nz": nz, "maps": M, "visibilities": K, "rounds": rounds,
           "scatter_workgroups": tiles, "counted": float(stats[:, 3].sum()),
           "out_of_range": float(stats[:, 4].sum()), "shift": float(stats[0, 5]),
           "ms_k15": [min(t["k15"]), med(t["k15"]), max(t["k15"])],
           "faster_torch_variant": best,
           "torch_over_k15_median": med(t[best]) / med(t["k15"]),
           "torch_over_k15_worst_case": min(t[best]) / max(t["k15"]),
           "k15_points_per_s": float(M) * K / (med(t["k15"]) * 1e-3),
           "max_relative_difference": diff}
    for n in routes:
        rec["ms_torch_" + n] = [min(t[n]), med(t[n]), max(t[n])]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=tuple(POINTS) + ("all",), default="all")
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
