#!/usr/bin/env python3
"""Times K21 (rjp_specfit: one Levenberg-Marquardt fit of Gaussians plus a baseline per sightline of
a line cube, the whole fit of a pixel in one launch, one lane per pixel; rjp_cube_moments: the
moment maps) against torch routes that stay on the device, on the same cube, in ONE process:

    python tools/specfit_probe.py [--point small|cfg3|all] [--rounds N] [--out FILE.json]

The torch fit is a batched Levenberg-Marquardt over all pixels with the same rule: the explicit
Jacobian [n_pix, P, C], J^T W J and J^T W r by batched matrix products, the damped system by
torch.linalg.cholesky_ex / cholesky_solve (both on at most 32768 pixels per call), and K20's decision written with torch.where (accept iff
every width is finite and > 0, chi^2 finite and better; lambda / 10 or 10 lambda), so the route
sends nothing to the host.  The torch moments are sums over where(counted, y, 0) along the channel
axis (what nansum does) with max / argmax for the peak.
small = 128 x 128 pixels x 64 channels; cfg3 = 512 x 512 pixels x 256 channels (0.54 GB).  Each with
one component and with two, the baseline free.  Noisy analytic data (2 % of the amplitude), `ITER`
trials with xtol tiny so that neither route stops early and both do the same work.  Every shape is
warmed up once; then the routes are timed with device events in alternating rounds; minimum, median
and maximum of each are reported with the ratio of the medians and the worst case for K21 (its
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

POINTS = {"small": (128 * 128, 64), "cfg3": (512 * 512, 256)}
ITER, LAM0, XTOL = 12, 1e-3, 1e-300
NOISE = 0.02
# torch's batched matmul / Cholesky routines take at most this many matrices per call here: on
# 262144 at once the route ended far above the noise level on three quarters of the pixels
BATCH = 32768


def chunked(fn, *tensors):
    n = tensors[0].shape[0]
    if n <= BATCH:
        return fn(*tensors)
    return torch.cat([fn(*(t[i:i + BATCH] for t in tensors)) for i in range(0, n, BATCH)])


def timed(fn):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1), out


def model_sums(Y, x, xr, th):
    """chi^2 [n], N [n, P, P], g [n, P] of theta [n, P] against the spectra Y [n, C]."""
    P = th.shape[1]
    rows, m = [], torch.zeros_like(Y)
    for c in range((P - 2) // 3):
        A, x0, s = (th[:, 3 * c + k:3 * c + k + 1] for k in range(3))
        z = (x[None, :] - x0) / s
        Ee = torch.exp(-0.5 * z * z)
        ae = A * Ee
        jx = ae * z / s
        rows += [Ee, jx, jx * z]
        m = m + ae
    m = m + th[:, P - 2:P - 1] + th[:, P - 1:P] * xr[None, :]
    rows += [torch.ones_like(Y), xr[None, :].expand_as(Y)]
    J = torch.stack(rows, dim=1)                                              # [n, P, C]
    r = Y - m
    return ((r * r).sum(dim=1), chunked(lambda a: a @ a.transpose(1, 2), J),
            chunked(lambda a, b: (a @ b[:, :, None])[:, :, 0], J, r))


def torch_lm(Y, x, xr, th0, n_iter):
    n, P = th0.shape
    dev = th0.device
    cur = th0.clone()
    chi_cur = torch.full((n,), float("inf"), dtype=torch.float64, device=dev)
    lam = torch.full((n,), LAM0, dtype=torch.float64, device=dev)
    N = torch.eye(P, dtype=torch.float64, device=dev).repeat(n, 1, 1)
    g = torch.zeros(n, P, dtype=torch.float64, device=dev)
    trial = th0.clone()
    for t in range(n_iter):
        chi_t, N_t, g_t = model_sums(Y, x, xr, trial)
        s = trial[:, 2:P - 2:3]
        acc = (torch.isfinite(s) & (s > 0)).all(dim=1) & torch.isfinite(chi_t) & (chi_t < chi_cur)
        cur = torch.where(acc[:, None], trial, cur)
        chi_cur = torch.where(acc, chi_t, chi_cur)
        N = torch.where(acc[:, None, None], N_t, N)
        g = torch.where(acc[:, None], g_t, g)
        down = lam if t == 0 else torch.clamp(lam / 10.0, min=1e-12)
        lam = torch.where(acc, down, lam * 10.0)
        d = torch.diagonal(N, dim1=1, dim2=2)
        step = chunked(lambda m, b: torch.cholesky_solve(b[:, :, None], torch.linalg.cholesky_ex(m)[0])[:, :, 0],
                       N + torch.diag_embed(lam[:, None] * d), g)
        trial = cur + step
    return cur, chi_cur


def torch_moments(cube, x, dx, x_ref, clip):
    ok = torch.isfinite(cube) & (cube.abs() >= clip)
    y = torch.where(ok, cube, torch.zeros_like(cube))
    yd = y * dx[:, None]
    m0 = yd.sum(dim=0)
    m1 = x_ref + (yd * (x[:, None] - x_ref)).sum(dim=0) / m0
    m2 = torch.sqrt((yd * (x[:, None] - m1[None, :]) ** 2).sum(dim=0) / m0)
    peak, ipeak = torch.where(ok, cube, torch.full_like(cube, float("-inf"))).max(dim=0)
    return m0, m1, m2, peak, ipeak, ok.sum(dim=0)


def stats(t):
    return [float(min(t)), float(np.median(t)), float(max(t))]


def probe(eng, name, nc, rounds):
    n, Cn = POINTS[name]
    dev = eng.device
    g = torch.Generator(device=dev)
    g.manual_seed(20240521 + nc)
    rnd = lambda lo, hi: lo + (hi - lo) * torch.rand(n, dtype=torch.float64, device=dev, generator=g)
    xh = np.linspace(-60.0, 60.0, Cn)
    x_ref = float(xh[Cn // 2])
    x = torch.from_numpy(xh).to(dev)
    xr = x - x_ref
    cols = [rnd(0.5, 2.0), rnd(-12.0, 12.0), rnd(6.0, 12.0)]
    if nc == 2:
        cols += [rnd(0.3, 0.8), cols[1] + rnd(28.0, 36.0), rnd(4.0, 8.0)]
    cols += [rnd(0.1, 0.3), rnd(0.001, 0.004)]
    truth = torch.stack(cols, dim=1)                                          # [n, P]
    P = truth.shape[1]
    zero = torch.zeros(n, Cn, dtype=torch.float64, device=dev)
    Yt = zero + truth[:, P - 2:P - 1] + truth[:, P - 1:P] * xr[None, :]
    for c in range(nc):
        A, x0, s = (truth[:, 3 * c + k:3 * c + k + 1] for k in range(3))
        Yt = Yt + A * torch.exp(-0.5 * ((x[None, :] - x0) / s) ** 2)
    Yt = Yt + NOISE * torch.randn(n, Cn, dtype=torch.float64, device=dev, generator=g)
    cube = Yt.t().contiguous()                                                # [C, n]: the cube
    del Yt, zero
    Y = cube.t()                                                              # the same buffer, [n, C]
    th0 = truth.clone()
    th0[:, 0:P - 2:3] *= 1.2
    th0[:, 1:P - 2:3] += 2.0
    th0[:, 2:P - 2:3] *= 1.25
    th0p = th0.t().contiguous()                                               # parameter planes
    dxh = E.channel_widths(xh)
    dx = torch.from_numpy(dxh).to(dev)

    k21 = lambda: eng.specfit(cube, xh, th0p, x_ref, n_comp=nc, n_iter=ITER, lambda0=LAM0, xtol=XTOL)
    route = lambda: torch_lm(Y, x, xr, th0, ITER)
    mom = lambda: eng.cube_moments(cube, xh, dxh, x_ref, 0.05)
    mroute = lambda: torch_moments(cube, x, dx, x_ref, 0.05)
    got, ref = k21(), route()                                                 # warm-up of every shape
    gm, rm = mom(), mroute()
    eng.synchronize()
    sc = ref[0].abs().clamp(min=1e-300)
    sc[:, 1:P - 2:3] = sc[:, 2:P - 2:3]
    per_pixel = ((got["theta"].t() - ref[0]).abs() / sc).max(dim=1)[0]
    theta_diff = float(per_pixel.max().item())
    # (noisy data, no stop: the routes may end apart on single pixels -- the torch route has no
    # answer to a failed pivot, and a near-tie of chi^2 may fall either way; the share of pixels on
    # which they end together and the medians say how rare that is)
    theta_med = float(per_pixel.median().item())
    share = float((per_pixel <= 1e-6).double().mean().item())
    chi_diff = float(((got["chi2"] - ref[1]).abs() / ref[1]).max().item())
    chi_med = float(((got["chi2"] - ref[1]).abs() / ref[1]).median().item())
    # each route against the data's own noise: chi^2 of a fitted pixel is about (C - P) sigma^2
    level = 1.5 * Cn * NOISE ** 2
    at_noise = [float((c <= level).double().mean().item()) for c in (got["chi2"], ref[1])]
    m_diff = float(max(((gm[0][i] - rm[i]).abs() / rm[i].abs().clamp(min=1e-300)).max().item() for i in range(3)))
    t_k, t_r, t_m, t_mr = [], [], [], []
    for _ in range(rounds):                                                   # alternating rounds
        t_k.append(timed(k21)[0])
        t_r.append(timed(route)[0])
        t_m.append(timed(mom)[0])
        t_mr.append(timed(mroute)[0])
    med = lambda t: float(np.median(t))
    return {"point": name, "pixels": n, "channels": Cn, "components": nc, "trials": ITER, "rounds": rounds,
            "cube_bytes": int(cube.numel() * 8), "workgroups": eng.last_specfit_workgroups,
            "status": sorted(set(got["status"].cpu().tolist())),
            "niter": sorted(set(got["niter"].cpu().tolist())),
            "ms_k21": stats(t_k), "ms_torch": stats(t_r),
            "ms_k21_per_trial": med(t_k) / ITER, "ms_torch_per_trial": med(t_r) / ITER,
            "ns_per_pixel_channel_trial_k21": 1e6 * med(t_k) / ITER / (n * Cn),
            "cube_GBps_k21": cube.numel() * 8 * ITER / (med(t_k) * 1e-3) / 1e9,
            "torch_over_k21_median": med(t_r) / med(t_k), "torch_over_k21_worst_case": min(t_r) / max(t_k),
            "ms_moments_k21": stats(t_m), "ms_moments_torch": stats(t_mr),
            "moments_cube_GBps_k21": 2 * cube.numel() * 8 / (med(t_m) * 1e-3) / 1e9,
            "moments_torch_over_k21_median": med(t_mr) / med(t_m),
            "moments_torch_over_k21_worst_case": min(t_mr) / max(t_m),
            "theta_max_diff_over_scale": theta_diff, "theta_median_diff_over_scale": theta_med,
            "share_of_pixels_within_1e-6": share, "chi2_max_rel_diff": chi_diff,
            "chi2_median_rel_diff": chi_med,
            "share_of_pixels_at_the_noise_level_k21": at_noise[0],
            "share_of_pixels_at_the_noise_level_torch": at_noise[1], "torch_batch": BATCH,
            "moments_max_rel_diff": m_diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--point", choices=tuple(POINTS) + ("all",), default="all")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    eng = E.RTEngine(0)
    recs = []
    for name in (tuple(POINTS) if args.point == "all" else (args.point,)):
        for nc in (1, 2):
            torch.cuda.empty_cache()
            recs.append(probe(eng, name, nc, args.rounds))
            print(json.dumps(recs[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "records": recs}, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
