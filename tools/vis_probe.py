#!/usr/bin/env python3
"""Times K10 (rjp_vis: model visibilities of a map stack by the direct Fourier sum, phasors never
in memory) against the torch route to the same numbers on the same buffers, in ONE process:

    python tools/vis_probe.py [--point big|small|all] [--rounds N] [--out FILE.json]

The torch route builds the phasor matrices Ez[M, K, nz] and Ex[M, K, nx] with torch (complex128,
torch.polar), forms W = Ez @ I^T with a batched complex128 matmul and V = sum_x Ex W: the same
factorisation, with every phasor in HBM (2 GB each at the big point).  Its time is reported whole
(what a user without K10 pays per call: the baselines scale with frequency, so the phasors belong to
the call) and for the matmul + reduction alone on prebuilt phasors.
big = 512 x 512 maps x 64 channels x 4096 visibilities (6.9e10 multiply-adds); small = 256 x 256 x
8 x 512.  Random log-normal maps with 20 % NaN pixels, a scale per channel, |a|, |b| <= 0.5 cycles
per cell.  Every shape is warmed up once; then the routes are timed with device events in
alternating rounds; minimum, median and maximum of each are reported with the ratio of the medians
and the worst case for K10 (its slowest round against torch's fastest), and the largest difference
between the two results relative to sum |I|."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rajepy_amd import engine as E  # noqa: E402

POINTS = {"big": (512, 512, 64, 4096), "small": (256, 256, 8, 512)}


def timed(fn):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1), out


def phasors(scale, pts, n):
    """e^{-2 pi i scale[m] pts[k] (index - (n-1)/2)} -> complex128 [M, K, n]."""
    j = torch.arange(n, dtype=torch.float64, device=pts.device) - (n - 1) / 2.0
    ph = (scale[:, None] * pts[None, :])[:, :, None] * j
    return torch.polar(torch.ones_like(ph), -2.0 * np.pi * ph)


def torch_matmul(maps, ex, ez):
    I = torch.nan_to_num(maps, nan=0.0).to(torch.complex128)
    W = torch.matmul(ez, I.transpose(1, 2))                 # [M, K, nz] @ [M, nz, nx]
    return (W * ex).sum(dim=-1)


def torch_route(maps, su, sv, u, v):
    nx, nz = maps.shape[1], maps.shape[2]
    return torch_matmul(maps, phasors(su, u, nx), phasors(sv, v, nz))


def probe(eng, name, rounds):
    nx, nz, M, K = POINTS[name]
    g = torch.Generator(device=eng.device)
    g.manual_seed(20240510)
    maps = torch.exp(2.0 * torch.randn(M, nx, nz, dtype=torch.float64, device=eng.device, generator=g))
    maps[torch.rand(M, nx, nz, device=eng.device, generator=g) < 0.2] = float("nan")
    u = torch.rand(K, dtype=torch.float64, device=eng.device, generator=g) - 0.5
    v = torch.rand(K, dtype=torch.float64, device=eng.device, generator=g) - 0.5
    u[0] = v[0] = 0.0
    su_h = -1.0 / (1.0 + 0.01 * np.arange(M))               # a scale per channel, |a| <= 0.5
    sv_h = -su_h
    su, sv = torch.from_numpy(su_h).to(eng.device), torch.from_numpy(sv_h).to(eng.device)
    flat = maps.reshape(M, -1)

    k10 = lambda: eng.vis(flat, nx, nz, su_h, sv_h, u, v)
    route = lambda: torch_route(maps, su, sv, u, v)
    a, b = k10(), route()                                       # warm-up of every shape
    ex, ez = phasors(su, u, nx), phasors(sv, v, nz)
    mm = lambda: torch_matmul(maps, ex, ez)
    mm()
    eng.synchronize()
    S = torch.nan_to_num(maps, nan=0.0).abs().sum(dim=(1, 2))
    diff = float(((a - b).abs() / S[:, None]).max().item())
    t_k10, t_route, t_mm = [], [], []
    for _ in range(rounds):                                     # alternating rounds
        t_k10.append(timed(k10)[0])
        t_route.append(timed(route)[0])
        t_mm.append(timed(mm)[0])
    med = lambda t: float(np.median(t))
    macs = float(M) * K * nx * nz
    return {"point": name, "nx": nx, "nz": nz, "channels": M, "visibilities": K, "rounds": rounds,
            "multiply_adds": macs,
            "ms_k10": [min(t_k10), med(t_k10), max(t_k10)],
            "ms_torch": [min(t_route), med(t_route), max(t_route)],
            "ms_torch_matmul_only": [min(t_mm), med(t_mm), max(t_mm)],
            "torch_over_k10_median": med(t_route) / med(t_k10),
            "torch_over_k10_worst_case": min(t_route) / max(t_k10),
            "torch_matmul_only_over_k10_median": med(t_mm) / med(t_k10),
            "k10_fma_lanes_per_s": 2.0 * macs / (med(t_k10) * 1e-3),
            "phasor_bytes_torch": 16.0 * M * K * (nx + nz),
            "max_diff_over_sum_abs": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=tuple(POINTS) + ("all",), default="all")
    ap.add_argument("--rounds", type=int, default=7)
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
