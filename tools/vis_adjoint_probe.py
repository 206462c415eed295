#!/usr/bin/env python3
"""Times K11 (rjp_vis_adjoint: dirty images from visibilities by the transposed direct Fourier sum,
phasors never in memory) against the torch route to the same numbers on the same buffers, in ONE
process:

    python tools/vis_adjoint_probe.py [--point big|small|all] [--rounds N] [--out FILE.json]

The torch route builds the phasor matrices Ex[M, nx, K] and Ez[M, K, nz] with torch (complex128,
torch.polar), scales Ex by w V and forms D = Re(Ex @ Ez) with a batched complex128 matmul: the same
factorisation, with every phasor in HBM (2 GB each at the big point).  Its time is reported whole
(what a user without K11 pays per call: the baselines scale with frequency, so the phasors belong to
the call) and for the matmul alone on prebuilt phasors.
big = 512 x 512 images x 64 channels x 4096 visibilities (6.9e10 multiply-adds); small = 256 x 256 x
8 x 512.  Random log-normal visibilities with random phases and weights, 20 % flagged (NaN), a scale
per channel, |a|, |b| <= 0.5 cycles per cell.  Every shape is warmed up once; then the routes are
timed with device events in alternating rounds; minimum, median and maximum of each are reported
with the ratio of the medians and the worst case for K11 (its slowest round against torch's
fastest), and the largest difference between the two results relative to sum |w V|."""
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
    """e^{+2 pi i scale[m] pts[k] (index - (n-1)/2)} -> complex128 [M, K, n]."""
    j = torch.arange(n, dtype=torch.float64, device=pts.device) - (n - 1) / 2.0
    ph = (scale[:, None] * pts[None, :])[:, :, None] * j
    return torch.polar(torch.ones_like(ph), 2.0 * np.pi * ph)


def torch_matmul(wv, ex, ez):
    """Re(sum_k (w V)[m, k] Ex[m, k, ix] Ez[m, k, iz]) -> [M, nx, nz]."""
    return torch.matmul((ex * wv[:, :, None]).transpose(1, 2), ez).real


def torch_route(vis, w, su, sv, u, v, nx, nz):
    wv = torch.nan_to_num(vis * w[None, :], nan=0.0)
    return torch_matmul(wv, phasors(su, u, nx), phasors(sv, v, nz))


def probe(eng, name, rounds):
    nx, nz, M, K = POINTS[name]
    g = torch.Generator(device=eng.device)
    g.manual_seed(20240511)
    rnd = lambda *s: torch.randn(*s, dtype=torch.float64, device=eng.device, generator=g)
    uni = lambda *s: torch.rand(*s, dtype=torch.float64, device=eng.device, generator=g)
    vis = torch.polar(torch.exp(2.0 * rnd(M, K)), 2.0 * np.pi * uni(M, K))
    vis[uni(M, K) < 0.2] = complex(float("nan"), 0.0)
    w = torch.exp(0.5 * rnd(K))
    u, v = uni(K) - 0.5, uni(K) - 0.5
    u[0] = v[0] = 0.0
    su_h = -1.0 / (1.0 + 0.01 * np.arange(M))               # a scale per channel, |a| <= 0.5
    sv_h = -su_h
    su, sv = torch.from_numpy(su_h).to(eng.device), torch.from_numpy(sv_h).to(eng.device)

    k11 = lambda: eng.vis_adjoint(vis, nx, nz, su_h, sv_h, u, v, w)
    route = lambda: torch_route(vis, w, su, sv, u, v, nx, nz)
    a, b = k11(), route()                                       # warm-up of every shape
    tiles = eng.last_vis_adjoint_tiles
    ex, ez = phasors(su, u, nx), phasors(sv, v, nz)
    wv = torch.nan_to_num(vis * w[None, :], nan=0.0)
    mm = lambda: torch_matmul(wv, ex, ez)
    mm()
    eng.synchronize()
    S = wv.abs().sum(dim=1)
    diff = float(((a.reshape(M, nx, nz) - b).abs().amax(dim=(1, 2)) / S).max().item())
    del a, b
    t_k11, t_route, t_mm = [], [], []
    for _ in range(rounds):                                     # alternating rounds
        t_k11.append(timed(k11)[0])
        t_route.append(timed(route)[0])
        t_mm.append(timed(mm)[0])
    med = lambda t: float(np.median(t))
    macs = float(M) * K * nx * nz
    return {"point": name, "nx": nx, "nz": nz, "channels": M, "visibilities": K, "rounds": rounds,
            "multiply_adds": macs, "tiles": tiles,
            "ms_k11": [min(t_k11), med(t_k11), max(t_k11)],
            "ms_torch": [min(t_route), med(t_route), max(t_route)],
            "ms_torch_matmul_only": [min(t_mm), med(t_mm), max(t_mm)],
            "torch_over_k11_median": med(t_route) / med(t_k11),
            "torch_over_k11_worst_case": min(t_route) / max(t_k11),
            "torch_matmul_only_over_k11_median": med(t_mm) / med(t_k11),
            "k11_fma_lanes_per_s": 2.0 * macs / (med(t_k11) * 1e-3),
            "phasor_bytes_torch": 16.0 * M * K * (nx + nz),
            "max_diff_over_sum_abs": diff}


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
