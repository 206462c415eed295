#!/usr/bin/env python3
"""Times K17 (rjp_msclean: multi-scale CLEAN, one fused launch per iteration for a whole stack of
maps of n_s planes) and rjp_convolve2d against torch routes on the same buffers, in ONE process:

    python tools/msclean_probe.py [--point image|cube|all] [--rounds N] [--out FILE.json]

The torch route of the CLEAN needs no host round trip per iteration: the weighted planes'
abs().argmax() over (plane, pixel), gathers for the peak value and the cross beam's centre, and
advanced indexing for the shifted cross beams of every plane, a dozen launches per iteration over
the whole stack.  The torch route of the convolution is torch.nn.functional.conv2d on the flipped
kernel with zero padding (float64), whose order of summation is the library's own.
image = 256 x 256 x 1 map, cube = 128 x 128 x 16 maps; scales 0 / 4 / 10 pixels (kernels of 1, 7
and 19 pixels), cross beams on a 63 x 63 window, gain 0.1, threshold 0, a mask 9 pixels inside the
border, 200 iterations.  The planes are those of a few sources of mixed scales seen through the
dirty beam of 32 random baselines plus noise.  Every shape is warmed up once; then the routes are
timed with device events in alternating rounds on fresh copies of the same planes (the copy is
outside the events); minimum, median and maximum of each are reported with the ratio of the medians
and the worst case (the kernel's slowest round against torch's fastest)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rajepy_amd import engine as E  # noqa: E402
from tools.clean_probe import make_beams, stats, timed  # noqa: E402

POINTS = {"image": (256, 256, 1, 200), "cube": (128, 128, 16, 200)}
SCALES = (0.0, 4.0, 10.0)
WINDOW = 63
GAIN = 0.1


def tri(k, l, n_s):
    a, b = min(k, l), max(k, l)
    return a * n_s - a * (a - 1) // 2 + (b - a)


def torch_conv(x, nx, nz, ker):
    """[M, nx nz] * ker [kx, kz] by conv2d on the flipped kernel -> [M, nx nz]."""
    kx, kz = ker.shape
    w = torch.flip(ker, (0, 1))[None, None]
    y = torch.nn.functional.conv2d(x.view(-1, 1, nx, nz), w, padding=((kx - 1) // 2, (kz - 1) // 2))
    return y.reshape(x.shape[0], -1)


def torch_msclean(R, X, W, mask, nx, nz, n_iter):
    """The device-only torch route; R [M, n_s, nx nz] in place, X [M, tri, p, p], W [M, n_s] ->
    (cpix, cscale, cflux)."""
    M, n_s, npix = R.shape
    p = X.shape[-1]
    c = (p - 1) // 2
    dev = R.device
    cpix = torch.empty(M, n_iter, dtype=torch.int64, device=dev)
    cscale = torch.empty(M, n_iter, dtype=torch.int64, device=dev)
    cflux = torch.empty(M, n_iter, dtype=torch.float64, device=dev)
    tab = torch.tensor([[tri(k, l, n_s) for l in range(n_s)] for k in range(n_s)], device=dev)
    rows = torch.arange(M, device=dev)
    qx = torch.arange(nx, device=dev)
    qz = torch.arange(nz, device=dev)
    R4 = R.view(M, n_s, nx, nz)
    neg = torch.full((), -1.0, dtype=torch.float64, device=dev)
    for t in range(n_iter):
        score = torch.where(mask[None, None, :], W[:, :, None] * R.abs(), neg)
        idx = score.view(M, -1).argmax(dim=1)
        k, pix = idx // npix, idx % npix
        v = R.view(M, -1).gather(1, idx[:, None])[:, 0]
        f = GAIN * v / X[rows, tab[k, k], c, c]
        bx = qx[None, :] - (pix // nz)[:, None] + c
        bz = qz[None, :] - (pix % nz)[:, None] + c
        ok = ((bx >= 0) & (bx < p))[:, None, :, None] & ((bz >= 0) & (bz < p))[:, None, None, :]
        planes = X[rows[:, None, None, None], tab[k][:, :, None, None],
                   bx.clamp(0, p - 1)[:, None, :, None], bz.clamp(0, p - 1)[:, None, None, :]]
        R4 -= f[:, None, None, None] * torch.where(ok, planes, torch.zeros_like(planes))
        cpix[:, t], cscale[:, t], cflux[:, t] = pix, k, f
    return cpix, cscale, cflux


def probe(eng, name, rounds):
    nx, nz, M, n_iter = POINTS[name]
    dev = eng.device
    g = torch.Generator(device=dev)
    g.manual_seed(20240517)
    kers = [torch.from_numpy(E.scale_kernel(s)).to(dev) for s in SCALES]
    n_s, hmax = len(SCALES), kers[-1].shape[0] // 2
    big = WINDOW + 4 * hmax
    B = make_beams(M, big, big, dev, g).reshape(M, -1)
    conv = lambda x, n, k: x if kers[k].numel() == 1 else eng.convolve2d(
        x, n, n, kers[k].reshape(-1), kers[k].shape[0], kers[k].shape[1])
    single = [conv(B, big, k) for k in range(n_s)]
    o = 2 * hmax
    X = torch.stack([conv(single[k], big, l).view(M, big, big)[:, o:o + WINDOW, o:o + WINDOW]
                     for k in range(n_s) for l in range(k, n_s)], dim=1).contiguous()
    # a few sources of mixed scales through the beam window, plus noise
    sky = torch.zeros(M, nx * nz, dtype=torch.float64, device=dev)
    for j in range(6):
        src = torch.zeros(M, nx, nz, dtype=torch.float64, device=dev)
        ix = torch.randint(2 * hmax, nx - 2 * hmax, (M,), device=dev, generator=g)
        iz = torch.randint(2 * hmax, nz - 2 * hmax, (M,), device=dev, generator=g)
        src[torch.arange(M, device=dev), ix, iz] = 0.3 + 0.7 * torch.rand(M, dtype=torch.float64, device=dev,
                                                                          generator=g)
        k = j % n_s
        s = src.view(M, -1)
        sky += s if kers[k].numel() == 1 else eng.convolve2d(s, nx, nz, kers[k].reshape(-1), *kers[k].shape)
    beam_k = X[:, 0].contiguous().view(M, -1)
    D = torch.stack([eng.convolve2d(sky[m:m + 1], nx, nz, beam_k[m], WINDOW, WINDOW)[0] for m in range(M)])
    D += 1e-3 * D.abs().amax() * torch.randn(M, nx * nz, dtype=torch.float64, device=dev, generator=g)
    R0 = torch.stack([D if kers[l].numel() == 1 else eng.convolve2d(D, nx, nz, kers[l].reshape(-1),
                                                                    *kers[l].shape) for l in range(n_s)],
                     dim=1).contiguous()
    c = (WINDOW - 1) // 2
    bias = torch.from_numpy(E.scale_biases(SCALES)).to(dev)
    W = (bias[None, :] / torch.stack([X[:, tri(k, k, n_s), c, c] for k in range(n_s)], dim=1)).contiguous()
    Wh = W.cpu().numpy()
    mask = torch.zeros(nx, nz, dtype=torch.bool, device=dev)
    mask[hmax:nx - hmax, hmax:nz - hmax] = True
    mask = mask.reshape(-1)

    work_a, work_b = R0.clone(), R0.clone()
    k17 = lambda: eng.msclean(work_a, n_s, nx, nz, X, WINDOW, WINDOW, Wh, n_iter, GAIN, 0.0, mask=mask)
    route = lambda: torch_msclean(work_b, X, W, mask, nx, nz, n_iter)
    got, ref = k17(), route()                                    # warm-up of every shape
    eng.synchronize()
    same = float(((got[0].to(torch.int64) == ref[0]) & (got[1].to(torch.int64) == ref[1]))
                 .to(torch.float64).mean().item())
    res_diff = float((work_a - work_b).abs().max().item() / R0.abs().max().item())
    wgs = eng.last_msclean_workgroups
    big_k = kers[-1]
    cv = lambda: eng.convolve2d(D, nx, nz, big_k.reshape(-1), *big_k.shape)
    tcv = lambda: torch_conv(D, nx, nz, big_k)
    c_diff = float((cv() - tcv()).abs().max().item() / D.abs().max().item())
    cw = lambda: eng.convolve2d(D, nx, nz, beam_k[0], WINDOW, WINDOW)
    tcw = lambda: torch_conv(D, nx, nz, X[0, 0])
    cw(), tcw()
    t = {k: [] for k in ("k17", "torch", "conv19", "torch19", "conv63", "torch63")}
    for _ in range(rounds):                                      # alternating rounds
        work_a.copy_(R0)
        t["k17"].append(timed(k17)[0])
        work_b.copy_(R0)
        t["torch"].append(timed(route)[0])
        t["conv19"].append(timed(cv)[0])
        t["torch19"].append(timed(tcv)[0])
        t["conv63"].append(timed(cw)[0])
        t["torch63"].append(timed(tcw)[0])
    med = lambda x: float(np.median(x))
    return {"point": name, "nx": nx, "nz": nz, "maps": M, "planes": n_s, "iterations": n_iter,
            "rounds": rounds, "workgroups_per_iteration": wgs,
            "ms_k17": stats(t["k17"]), "ms_torch": stats(t["torch"]),
            "us_per_iteration_k17": 1e3 * med(t["k17"]) / n_iter,
            "us_per_iteration_torch": 1e3 * med(t["torch"]) / n_iter,
            "torch_over_k17_median": med(t["torch"]) / med(t["k17"]),
            "torch_over_k17_worst_case": min(t["torch"]) / max(t["k17"]),
            "share_of_components_equal_to_torch": same, "planes_max_diff_over_peak": res_diff,
            "ms_convolve2d_19x19": stats(t["conv19"]), "ms_torch_conv2d_19x19": stats(t["torch19"]),
            "torch_over_convolve2d_19x19_median": med(t["torch19"]) / med(t["conv19"]),
            "ms_convolve2d_63x63": stats(t["conv63"]), "ms_torch_conv2d_63x63": stats(t["torch63"]),
            "torch_over_convolve2d_63x63_median": med(t["torch63"]) / med(t["conv63"]),
            "convolve2d_max_diff_over_peak": c_diff}


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
