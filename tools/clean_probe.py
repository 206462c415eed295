#!/usr/bin/env python3
"""Times K12 (rjp_clean: Hogbom CLEAN, one fused launch per iteration for a whole stack of images)
against torch routes to the same components on the same buffers, and K13 (rjp_restore) against a
dense torch evaluation of the same sum, in ONE process:

    python tools/clean_probe.py [--point image|cube|all] [--rounds N] [--out FILE.json]

The torch route needs no host round trip per iteration: batched abs().argmax(), gathers for the peak
value, and advanced indexing for the shifted beam (B[m, ix - ix* + cx, iz - iz* + cz], always inside
the full 2 n - 1 beam), some eight launches per iteration over the whole stack.  A second variant
with one .item() per iteration (the arg-max goes to the host, the beam window is a slice) is timed
at the single-map point for information only.
image = 501 x 501 x 1 map x 500 iterations (the reference's imaging case); cube = 256 x 256 x 64
maps x 200 iterations, every map with its own beam.  The images are a few point sources convolved
with the dirty beam of 32 random baselines plus noise at 1e-3 of the peak; gain 0.1, threshold 0,
no mask.  Every shape is warmed up once; then the routes are timed with device events in alternating
rounds on fresh copies of the same dirty images (the copy is outside the events); minimum, median
and maximum of each are reported with the ratio of the medians and the worst case for K12 (its
slowest round against torch's fastest).  The launch-bound floor of an iteration is K12 itself on a
1 x 1 image: the same number of dependent launches with nothing to do."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rajepy_amd import engine as E  # noqa: E402

POINTS = {"image": (501, 501, 1, 500), "cube": (256, 256, 64, 200)}
GAIN = 0.1


def timed(fn):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1), out


def make_beams(M, px, pz, dev, g, n_vis=32):
    """[M, px, pz]: the dirty beams of 32 random baselines each, 1 at the centre."""
    jx = torch.arange(px, dtype=torch.float64, device=dev) - (px - 1) / 2.0
    jz = torch.arange(pz, dtype=torch.float64, device=dev) - (pz - 1) / 2.0
    out = torch.empty(M, px, pz, dtype=torch.float64, device=dev)
    for m in range(M):
        a = (torch.rand(n_vis, dtype=torch.float64, device=dev, generator=g) - 0.5) * 0.5
        b = (torch.rand(n_vis, dtype=torch.float64, device=dev, generator=g) - 0.5) * 0.5
        ph = 2.0 * np.pi * (a[:, None, None] * jx[None, :, None] + b[:, None, None] * jz[None, None, :])
        out[m] = torch.cos(ph).mean(dim=0)
        out[m, (px - 1) // 2, (pz - 1) // 2] = 1.0
    return out


def shifted(B, ix, iz, nx, nz):
    """B[m, qx - ix[m] + cx, qz - iz[m] + cz] -> [M, nx, nz] (the full beam: always inside)."""
    M = B.shape[0]
    cx, cz = (B.shape[1] - 1) // 2, (B.shape[2] - 1) // 2
    qx = torch.arange(nx, device=B.device)
    qz = torch.arange(nz, device=B.device)
    bx = qx[None, :] - ix[:, None] + cx
    bz = qz[None, :] - iz[:, None] + cz
    return B[torch.arange(M, device=B.device)[:, None, None], bx[:, :, None], bz[:, None, :]]


def torch_clean(R, B, nx, nz, n_iter, thresh=0.0):
    """The device-only torch route; R [M, nx nz] in place -> (cpix, cflux)."""
    M = R.shape[0]
    cpix = torch.empty(M, n_iter, dtype=torch.int64, device=R.device)
    cflux = torch.empty(M, n_iter, dtype=torch.float64, device=R.device)
    R3 = R.view(M, nx, nz)
    for t in range(n_iter):
        idx = R.abs().argmax(dim=1)
        v = R.gather(1, idx[:, None])[:, 0]
        f = torch.where(v.abs() > thresh, GAIN * v, torch.zeros_like(v))
        R3 -= f[:, None, None] * shifted(B, idx // nz, idx % nz, nx, nz)
        cpix[:, t] = idx
        cflux[:, t] = f
    return cpix, cflux


def torch_clean_item(R, B, nx, nz, n_iter):
    """One .item() per iteration, the beam window a slice (single map)."""
    R2, B2 = R.view(nx, nz), B[0]
    comps = []
    for t in range(n_iter):
        p = int(R.abs().argmax().item())
        ix, iz = p // nz, p % nz
        f = GAIN * R2[ix, iz]
        R2 -= f * B2[nx - 1 - ix:2 * nx - 1 - ix, nz - 1 - iz:2 * nz - 1 - iz]
        comps.append((p, f))
    return comps


def torch_restore(cpix, cflux, abc, nx, nz, add, chunk=16):
    """The dense sum [M, nx nz], components in chunks of 16."""
    M, S = cpix.shape
    A, B, C = abc
    qx = torch.arange(nx, dtype=torch.float64, device=add.device)[None, None, :, None]
    qz = torch.arange(nz, dtype=torch.float64, device=add.device)[None, None, None, :]
    out = add.view(M, nx, nz).clone()
    for c0 in range(0, S, chunk):
        p = cpix[:, c0:c0 + chunk]
        dx = qx - (p // nz).to(torch.float64)[:, :, None, None]
        dz = qz - (p % nz).to(torch.float64)[:, :, None, None]
        g = torch.exp(-(A * dx * dx + 2.0 * B * dx * dz + C * dz * dz))
        out += (cflux[:, c0:c0 + chunk, None, None] * g).sum(dim=1)
    return out.view(M, -1)


def stats(t):
    return [float(min(t)), float(np.median(t)), float(max(t))]


def probe(eng, name, rounds):
    nx, nz, M, n_iter = POINTS[name]
    dev = eng.device
    g = torch.Generator(device=dev)
    g.manual_seed(20240512)
    px, pz = 2 * nx - 1, 2 * nz - 1
    B = make_beams(M, px, pz, dev, g)
    D = torch.zeros(M, nx, nz, dtype=torch.float64, device=dev)
    for _ in range(5):
        ix = torch.randint(0, nx, (M,), device=dev, generator=g)
        iz = torch.randint(0, nz, (M,), device=dev, generator=g)
        s = 0.3 + 0.7 * torch.rand(M, dtype=torch.float64, device=dev, generator=g)
        D += s[:, None, None] * shifted(B, ix, iz, nx, nz)
    D += 1e-3 * D.abs().amax() * torch.randn(M, nx, nz, dtype=torch.float64, device=dev, generator=g)
    D = D.reshape(M, -1).contiguous()

    def k12():
        return eng.clean(work_a, nx, nz, B, px, pz, n_iter, GAIN, 0.0)

    def route():
        return torch_clean(work_b, B, nx, nz, n_iter)

    work_a, work_b = D.clone(), D.clone()
    got, ref = k12(), route()                                    # warm-up of every shape
    eng.synchronize()
    same = float((got[0].to(torch.int64) == ref[0]).to(torch.float64).mean().item())
    res_diff = float((work_a - work_b).abs().max().item() / D.abs().max().item())
    tiles = eng.last_clean_tiles
    one = torch.full((1, 1), 1.0, dtype=torch.float64, device=dev)
    floor_fn = lambda: eng.clean(one.clone(), 1, 1, one, 1, 1, n_iter, GAIN, 0.0)
    floor_fn()
    abc = (0.05, 0.01, 0.04)
    k13 = lambda: eng.restore(got[0], got[1], got[2], abc, nx, nz, add=work_a)
    t13 = lambda: torch_restore(ref[0], ref[1], abc, nx, nz, work_b)
    r_diff = float((k13() - t13()).abs().max().item() / D.abs().max().item())
    t_k12, t_route, t_item, t_floor, t_k13, t_t13 = [], [], [], [], [], []
    for _ in range(rounds):                                      # alternating rounds
        work_a.copy_(D)
        t_k12.append(timed(k12)[0])
        work_b.copy_(D)
        t_route.append(timed(route)[0])
        if M == 1:
            work_b.copy_(D)
            t_item.append(timed(lambda: torch_clean_item(work_b, B, nx, nz, n_iter))[0])
        t_floor.append(timed(floor_fn)[0])
        t_k13.append(timed(k13)[0])
        t_t13.append(timed(t13)[0])
    med = lambda t: float(np.median(t))
    rec = {"point": name, "nx": nx, "nz": nz, "maps": M, "iterations": n_iter, "rounds": rounds,
           "workgroups_per_iteration": tiles,
           "ms_k12": stats(t_k12), "ms_torch": stats(t_route),
           "ms_k12_on_1x1_same_iterations": stats(t_floor),
           "us_per_iteration_k12": 1e3 * med(t_k12) / n_iter,
           "us_per_iteration_floor": 1e3 * med(t_floor) / n_iter,
           "us_per_iteration_torch": 1e3 * med(t_route) / n_iter,
           "torch_over_k12_median": med(t_route) / med(t_k12),
           "torch_over_k12_worst_case": min(t_route) / max(t_k12),
           "share_of_components_equal_to_torch": same,
           "residual_max_diff_over_peak": res_diff,
           "ms_k13": stats(t_k13), "ms_torch_restore": stats(t_t13),
           "torch_over_k13_median": med(t_t13) / med(t_k13),
           "restore_max_diff_over_peak": r_diff}
    if t_item:
        rec["ms_torch_item_per_iteration"] = stats(t_item)
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
