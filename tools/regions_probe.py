#!/usr/bin/env python3
"""Times K25 (rjp_image_stats, rjp_label_regions, rjp_mask_grow) against the obvious routes on the
same buffers, in ONE process:

    python tools/regions_probe.py [--maps M] [--size N] [--rounds N] [--out FILE.json]

Statistics: `RTEngine.image_stats` against torch on the device -- `nanmedian` of the stack, then
`nanmedian` of |x - median| (torch's median is the lower one too), plus min, max, sum and the sum of
squares.  Labels and growth: torch has neither, so the route is `scipy.ndimage.label` /
`binary_dilation(iterations=75, mask=...)` on the HOST, the copies of the stack down and of the
result up included -- what a caller without K25 does every major cycle.  Shapes: M maps (default 16)
of N x N pixels (default 512), noise plus a few sources; the masks are the pixels above 3 and 1.5
robust sigma.  Every route is warmed up once; then the routes are timed in alternating rounds
(device events for the device routes, the wall clock around a synchronisation for the host ones);
minimum, median and maximum of each are reported with the ratio of the medians and the worst case
for K25 (its slowest round against the other route's fastest)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from scipy import ndimage  # noqa: E402

from rajepy_amd import engine as E  # noqa: E402


def timed(fn):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1), out


def walled(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(t):
    return {"min": float(np.min(t)), "median": float(np.median(t)), "max": float(np.max(t))}


def torch_stats(img):
    med = torch.nanmedian(img, dim=1).values
    mad = torch.nanmedian((img - med[:, None]).abs(), dim=1).values
    return med, mad, img.amin(dim=1), img.amax(dim=1), img.sum(dim=1), (img * img).sum(dim=1)


def host_labels(mask, n, conn):
    st = ndimage.generate_binary_structure(2, conn)
    out = np.stack([ndimage.label(m.reshape(n, n), structure=st)[0] for m in mask.cpu().numpy()])
    return torch.from_numpy(out).to(mask.device)


def host_grow(seed, con, n, conn, n_iter):
    st = ndimage.generate_binary_structure(2, conn)
    s, c = seed.cpu().numpy() != 0, con.cpu().numpy() != 0
    out = np.stack([ndimage.binary_dilation(a.reshape(n, n), structure=st, iterations=n_iter,
                                            mask=b.reshape(n, n)) for a, b in zip(s, c)])
    return torch.from_numpy(out).to(seed.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    eng = E.RTEngine(0)
    M, n = a.maps, a.size
    g = torch.Generator(device=eng.device).manual_seed(25)
    img = torch.randn(M, n * n, dtype=torch.float64, device=eng.device, generator=g)
    x = torch.arange(n, dtype=torch.float64, device=eng.device)
    for k in range(5):
        cx, cz = n * (k + 1) / 6.0, n * ((3 * k) % 5 + 1) / 6.0
        img += (8.0 * torch.exp(-((x[:, None] - cx) ** 2 + (x[None, :] - cz) ** 2) / (2.0 * 6.0 ** 2))).reshape(-1)
    st = eng.image_stats(img, n, n)
    med, sig = st[:, 4:5], 1.4826 * st[:, 5:6]
    seed = (img > med + 3.0 * sig).to(torch.uint8)
    con = (img > med + 1.5 * sig).to(torch.uint8)
    ref = torch_stats(img)
    assert torch.equal(ref[0], st[:, 4]) and torch.equal(ref[1], st[:, 5]), "the routes disagree"
    routes = {
        "image_stats": (lambda: timed(lambda: eng.image_stats(img, n, n)),
                        lambda: timed(lambda: torch_stats(img))),
        "label_regions": (lambda: walled(lambda: eng.label_regions(seed, n, n, 1)),
                          lambda: walled(lambda: host_labels(seed, n, 1))),
        "mask_grow 75": (lambda: walled(lambda: eng.mask_grow(seed, con, n, n, 75, 1)),
                         lambda: walled(lambda: host_grow(seed, con, n, 1, 75))),
        "mask_grow stable": (lambda: walled(lambda: eng.mask_grow(seed, con, n, n, -1, 1)),
                             lambda: walled(lambda: host_grow(seed, con, n, 1, 0))),
    }
    report = {"maps": M, "size": n, "rounds": a.rounds, "routes": {}}
    for name, (ours, other) in routes.items():
        ours(), other()
        t_k, t_o = [], []
        for _ in range(a.rounds):
            t_k.append(ours()[0])
            t_o.append(other()[0])
        r = {"k25_ms": stats(t_k), "other_ms": stats(t_o),
             "ratio_of_medians": float(np.median(t_o) / np.median(t_k)),
             "worst_case": float(np.min(t_o) / np.max(t_k))}
        report["routes"][name] = r
        print("%-18s K25 %.3f ms (%.3f-%.3f), other %.3f ms (%.3f-%.3f), x%.2f, worst x%.2f"
              % (name, r["k25_ms"]["median"], r["k25_ms"]["min"], r["k25_ms"]["max"],
                 r["other_ms"]["median"], r["other_ms"]["min"], r["other_ms"]["max"],
                 r["ratio_of_medians"], r["worst_case"]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
