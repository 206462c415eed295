#!/usr/bin/env python3
"""Times K19 (rjp_mtmfs: multi-term MFS CLEAN, one fused launch per iteration for a whole stack of
maps of n_t Taylor planes) against a torch route on the same buffers, in ONE process:

    python tools/mtmfs_probe.py [--point image|cube|all] [--nterms N] [--rounds N] [--out FILE.json]

The torch route needs no host round trip per iteration either: the principal solution's term 0 over
the whole stack (n_t multiply-adds), its abs().argmax() per map, a gather of the n_t plane values
at the peak, a small matrix product with Hinv for the coefficients, and advanced indexing for the
shifted spectral beams of every plane and term, a dozen launches per iteration.
image = 256 x 256 x 1 map, cube = 128 x 128 x 16 maps; n_t = 2 by default (--nterms 1 .. 4), the
spectral beams on a 63 x 63 window, gain 0.1, threshold 0, no mask, 200 iterations.  The beams are
those of 32 random baselines seen at 8 channels over a band of 40 % (the baselines in wavelengths
scale with the frequency), B_q = mean_f w_f^q beam_f; the planes are those of six point sources
with spectral slopes between -1 and 1 seen through them, plus noise.  Every shape is warmed up
once; then the routes are timed with device events in alternating rounds on fresh copies of the
same planes (the copy is outside the events); minimum, median and maximum of each are reported with
the ratio of the medians and the worst case (the kernel's slowest round against torch's fastest)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rajepy_amd import engine as E  # noqa: E402
from tools.clean_probe import stats, timed  # noqa: E402

POINTS = {"image": (256, 256, 1, 200), "cube": (128, 128, 16, 200)}
WINDOW = 63
GAIN = 0.1
BAND = np.linspace(4e9, 6e9, 8)


def spectral_beams(M, n_t, p, dev, g, n_vis=32):
    """[M, 2 n_t - 1, p, p]: B_q = mean_f w_f^q beam_f of 32 random baselines per map, B_0(centre) = 1."""
    tw = torch.from_numpy(E.taylor_weights(BAND, 5e9, 2 * n_t - 1)).to(dev)
    s = torch.from_numpy(BAND / 5e9).to(dev)
    j = torch.arange(p, dtype=torch.float64, device=dev) - (p - 1) / 2.0
    out = torch.empty(M, 2 * n_t - 1, p, p, dtype=torch.float64, device=dev)
    for m in range(M):
        a = (torch.rand(n_vis, dtype=torch.float64, device=dev, generator=g) - 0.5) * 0.4
        b = (torch.rand(n_vis, dtype=torch.float64, device=dev, generator=g) - 0.5) * 0.4
        ph = 2.0 * np.pi * s[:, None, None, None] * (a[None, :, None, None] * j[None, None, :, None] +
                                                     b[None, :, None, None] * j[None, None, None, :])
        beams = torch.cos(ph).mean(dim=1)                           # [F, p, p], 1 at the centre
        out[m] = torch.einsum("qf,fxz->qxz", tw, beams) / len(BAND)
        out[m, 0, (p - 1) // 2, (p - 1) // 2] = 1.0
    return out


def shifted(B, ix, iz, nx, nz):
    """B[m, :, qx - ix[m] + c, qz - iz[m] + c] -> ([M, nb, nx, nz], inside [M, 1, nx, nz])."""
    M, p = B.shape[0], B.shape[-1]
    c = (p - 1) // 2
    bx = torch.arange(nx, device=B.device)[None, :] - ix[:, None] + c
    bz = torch.arange(nz, device=B.device)[None, :] - iz[:, None] + c
    ok = ((bx >= 0) & (bx < p))[:, None, :, None] & ((bz >= 0) & (bz < p))[:, None, None, :]
    rows = torch.arange(M, device=B.device)[:, None, None, None]
    q = torch.arange(B.shape[1], device=B.device)[None, :, None, None]
    planes = B[rows, q, bx.clamp(0, p - 1)[:, None, :, None], bz.clamp(0, p - 1)[:, None, None, :]]
    return torch.where(ok, planes, torch.zeros_like(planes))


def torch_mtmfs(R, B, Hinv, nx, nz, n_iter):
    """The device-only torch route; R [M, n_t, nx nz] in place, B [M, 2 n_t - 1, p, p], Hinv
    [M, n_t, n_t] -> (cpix, ccoef)."""
    M, n_t, npix = R.shape
    dev = R.device
    cpix = torch.empty(M, n_iter, dtype=torch.int64, device=dev)
    ccoef = torch.empty(M, n_iter, n_t, dtype=torch.float64, device=dev)
    R4 = R.view(M, n_t, nx, nz)
    idx = torch.arange(n_t, device=dev)
    tq = idx[:, None] + idx[None, :]                                # [t, q] -> t + q
    for it in range(n_iter):
        a0 = (Hinv[:, 0, :, None] * R).sum(dim=1)
        pix = a0.abs().argmax(dim=1)
        v = R.gather(2, pix[:, None, None].expand(M, n_t, 1))[:, :, 0]
        c = GAIN * torch.einsum("mqt,mt->mq", Hinv, v)
        S = shifted(B, pix // nz, pix % nz, nx, nz)                 # [M, nb, nx, nz]
        R4 -= torch.einsum("mq,mtqxz->mtxz", c, S[:, tq])
        cpix[:, it], ccoef[:, it] = pix, c
    return cpix, ccoef


def probe(eng, name, n_t, rounds):
    nx, nz, M, n_iter = POINTS[name]
    dev = eng.device
    g = torch.Generator(device=dev)
    g.manual_seed(20240519)
    B = spectral_beams(M, n_t, WINDOW, dev, g)
    c = (WINDOW - 1) // 2
    hs = [E.taylor_hessian_inverse(x)[1] for x in B[:, :, c, c].cpu().numpy()]
    Hh = np.stack(hs)
    Hinv = torch.from_numpy(Hh).to(dev)
    idx = torch.arange(n_t, device=dev)
    tq = idx[:, None] + idx[None, :]
    R0 = torch.zeros(M, n_t, nx, nz, dtype=torch.float64, device=dev)
    for _ in range(6):
        ix = torch.randint(c, nx - c, (M,), device=dev, generator=g)
        iz = torch.randint(c, nz - c, (M,), device=dev, generator=g)
        i0 = 0.3 + 0.7 * torch.rand(M, dtype=torch.float64, device=dev, generator=g)
        coef = torch.stack([i0] + [i0 * (2 * torch.rand(M, dtype=torch.float64, device=dev, generator=g) - 1)
                                   for _ in range(n_t - 1)], dim=1)
        R0 += torch.einsum("mq,mtqxz->mtxz", coef, shifted(B, ix, iz, nx, nz)[:, tq])
    R0 += 1e-3 * R0[:, 0].abs().amax() * torch.randn(M, n_t, nx, nz, dtype=torch.float64, device=dev, generator=g)
    R0 = R0.reshape(M, n_t, nx * nz).contiguous()
    Bf = B.reshape(M, 2 * n_t - 1, WINDOW * WINDOW).contiguous()

    work_a, work_b = R0.clone(), R0.clone()
    k19 = lambda: eng.mtmfs(work_a, n_t, nx, nz, Bf, WINDOW, WINDOW, Hh, n_iter, GAIN, 0.0)
    route = lambda: torch_mtmfs(work_b, B, Hinv, nx, nz, n_iter)
    got, ref = k19(), route()                                    # warm-up of every shape
    eng.synchronize()
    same = float((got[0].to(torch.int64) == ref[0]).to(torch.float64).mean().item())
    res_diff = float((work_a - work_b).abs().max().item() / R0.abs().max().item())
    wgs = eng.last_mtmfs_workgroups
    t = {"k19": [], "torch": []}
    for _ in range(rounds):                                      # alternating rounds
        work_a.copy_(R0)
        t["k19"].append(timed(k19)[0])
        work_b.copy_(R0)
        t["torch"].append(timed(route)[0])
    med = lambda x: float(np.median(x))
    return {"point": name, "nx": nx, "nz": nz, "maps": M, "nterms": n_t, "iterations": n_iter,
            "rounds": rounds, "workgroups_per_iteration": wgs,
            "ms_k19": stats(t["k19"]), "ms_torch": stats(t["torch"]),
            "us_per_iteration_k19": 1e3 * med(t["k19"]) / n_iter,
            "us_per_iteration_torch": 1e3 * med(t["torch"]) / n_iter,
            "torch_over_k19_median": med(t["torch"]) / med(t["k19"]),
            "torch_over_k19_worst_case": min(t["torch"]) / max(t["k19"]),
            "share_of_components_equal_to_torch": same, "planes_max_diff_over_peak": res_diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=tuple(POINTS) + ("all",), default="all")
    ap.add_argument("--nterms", type=int, default=2, choices=(1, 2, 3, 4))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = E.RTEngine(0)
    recs = []
    for name in (tuple(POINTS) if args.point == "all" else (args.point,)):
        torch.cuda.empty_cache()
        recs.append(probe(eng, name, args.nterms, args.rounds))
        print(json.dumps(recs[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "records": recs}, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
