#!/usr/bin/env python3
"""Times K18 (rjp_vis_components: the visibilities of a list of clean components, n_comp x n_vis
phasors) against the two other routes to the same numbers on the same buffers, and one CLEAN major
cycle against its parts, in ONE process:

    python tools/major_cycle_probe.py [--point big|small|all] [--rounds N] [--out FILE.json]

  * K10 on the dense model image: `RTEngine.components_image` of the list, then `RTEngine.vis` --
    nx nz x n_vis multiply-adds whatever the list's length (the image is made once, outside the
    timing: the route is charged K10 alone);
  * a torch complex matmul on the list: the phasor matrix e^{-2 pi i (a jx + b jz)} [M, K, n] built
    with torch.polar (every phasor in HBM) times the fluxes;
  * one major cycle = V - K18(list) followed by K11 on the image grid (`RTEngine.vis_adjoint`); its
    parts are timed alone and together.
big = 512 x 512 images x 16 channels x 4096 visibilities x 2000 components; small = 256 x 256 x 4 x
512 x 500.  Random pixels (30 % repeating an earlier one), fluxes of both signs, a scale per
channel, |a|, |b| <= 0.5 cycles per cell.  Every shape is warmed up once; then the routes are timed
with device events in alternating rounds; minimum, median and maximum of each are reported with the
ratios of the medians, and the largest difference between the results relative to sum |f|."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rajepy_amd import engine as E  # noqa: E402

POINTS = {"big": (512, 512, 16, 4096, 2000), "small": (256, 256, 4, 512, 500)}


def timed(fn):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1), out


def torch_route(cpix, cflux, nx, nz, su, sv, u, v):
    jx = torch.div(cpix, nz, rounding_mode="floor").to(torch.float64) - (nx - 1) / 2.0
    jz = (cpix % nz).to(torch.float64) - (nz - 1) / 2.0
    ph = (su[:, None] * u[None, :])[:, :, None] * jx[:, None, :] + \
        (sv[:, None] * v[None, :])[:, :, None] * jz[:, None, :]
    return torch.matmul(torch.polar(torch.ones_like(ph), -2.0 * np.pi * ph),
                        cflux.to(torch.complex128)[:, :, None]).squeeze(-1)


def probe(eng, name, rounds):
    nx, nz, M, K, n = POINTS[name]
    g = torch.Generator(device=eng.device)
    g.manual_seed(20240518)
    cpix = torch.randint(0, nx * nz, (M, n), device=eng.device, generator=g)
    dup = torch.rand(M, n, device=eng.device, generator=g) < 0.3
    cpix = torch.where(dup, cpix.roll(1, dims=1), cpix).to(torch.int32).contiguous()
    cflux = torch.exp(1.5 * torch.randn(M, n, dtype=torch.float64, device=eng.device, generator=g))
    cflux = (cflux * torch.where(torch.rand(M, n, device=eng.device, generator=g) < 0.5, -1.0, 1.0)).contiguous()
    ncomp = torch.full((M,), n, dtype=torch.int32, device=eng.device)
    u = torch.rand(K, dtype=torch.float64, device=eng.device, generator=g) - 0.5
    v = torch.rand(K, dtype=torch.float64, device=eng.device, generator=g) - 0.5
    u[0] = v[0] = 0.0
    su_h = -1.0 / (1.0 + 0.01 * np.arange(M))               # a scale per channel, |a| <= 0.5
    sv_h = -su_h
    su, sv = torch.from_numpy(su_h).to(eng.device), torch.from_numpy(sv_h).to(eng.device)
    V = torch.randn(M, K, dtype=torch.complex128, device=eng.device, generator=g)

    k18 = lambda: eng.vis_components(cpix, cflux, ncomp, nx, nz, su_h, sv_h, u, v)
    image = eng.components_image(cpix, cflux, ncomp, nx, nz).reshape(M, nx * nz).contiguous()
    k10 = lambda: eng.vis(image, nx, nz, su_h, sv_h, u, v)
    route = lambda: torch_route(cpix.to(torch.int64), cflux, nx, nz, su, sv, u, v)
    make_image = lambda: eng.components_image(cpix, cflux, ncomp, nx, nz)
    forward = lambda: eng.vis_components(cpix, cflux, ncomp, nx, nz, su_h, sv_h, u, v, vis_in=V, sign=-1)
    vres = forward()
    adjoint = lambda: eng.vis_adjoint(vres, nx, nz, su_h, sv_h, u, v)
    cycle = lambda: eng.vis_adjoint(forward(), nx, nz, su_h, sv_h, u, v)
    a, b, c = k18(), k10(), route()                             # warm-up of every shape
    make_image(), adjoint(), cycle()
    eng.synchronize()
    S = cflux.abs().sum(dim=1)[:, None]
    diff10 = float(((a - b).abs() / S).max().item())
    diff_t = float(((a - c).abs() / S).max().item())
    names = ("k18", "k10_dense", "torch_list", "components_image", "forward", "adjoint", "cycle")
    fns = (k18, k10, route, make_image, forward, adjoint, cycle)
    t = {k: [] for k in names}
    for _ in range(rounds):                                     # alternating rounds
        for k, fn in zip(names, fns):
            t[k].append(timed(fn)[0])
    med = lambda x: float(np.median(x))
    rec = {"point": name, "nx": nx, "nz": nz, "channels": M, "visibilities": K, "components": n,
           "rounds": rounds, "phasor_pairs": float(M) * K * n}
    for k in names:
        rec["ms_" + k] = [min(t[k]), med(t[k]), max(t[k])]
    rec.update(k10_over_k18_median=med(t["k10_dense"]) / med(t["k18"]),
               k10_over_k18_worst_case=min(t["k10_dense"]) / max(t["k18"]),
               torch_over_k18_median=med(t["torch_list"]) / med(t["k18"]),
               torch_over_k18_worst_case=min(t["torch_list"]) / max(t["k18"]),
               cycle_over_parts_median=med(t["cycle"]) / (med(t["forward"]) + med(t["adjoint"])),
               forward_share_of_cycle=med(t["forward"]) / med(t["cycle"]),
               k18_ns_per_phasor_pair=med(t["k18"]) * 1e6 / (float(M) * K * n),
               phasor_bytes_torch=16.0 * M * K * n,
               max_diff_k10_over_sum_abs=diff10, max_diff_torch_over_sum_abs=diff_t)
    return rec


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
