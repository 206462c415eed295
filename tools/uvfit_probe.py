#!/usr/bin/env python3
"""Times K20 (rjp_uvfit: Levenberg-Marquardt fits of point / Gaussian components to visibilities,
one fused launch per iteration for a whole stack of visibility sets) against a torch
Levenberg-Marquardt that stays on the device, on the same buffers, in ONE process:

    python tools/uvfit_probe.py [--point tracks|dense|all] [--rounds N] [--out FILE.json]

The torch route is the same algorithm: the explicit complex Jacobian of the model as stacked real
and imaginary rows, Re(J^H W J) and Re(J^H W r) by batched matrix products (and, as a second route,
by broadcast products summed over the visibilities; the ratios are quoted against the faster of the
two), the damped system by torch.linalg.cholesky_ex / cholesky_solve, and K20's decision rule
written with torch.where (accept iff positive semi-definite, finite and better; lambda / 10 or
10 lambda), so the route itself sends nothing to the host.
tracks = the 7020 visibilities of the 27-antenna fixture over 20 integrations x 8 maps x 1
component; dense = 2^18 visibilities x 1 map x 2 components.  Noisy analytic data (1 % of the
flux), `ITER` = 20 iterations with xtol tiny so that neither route stops early and both do the same
work.  Every shape is warmed up once; then the routes are timed with device events in alternating
rounds; minimum, median and maximum of each are reported with the ratio of the medians and the worst
case for K20 (its slowest round against torch's fastest).  The launch-bound floor of an iteration is
K20 itself on six visibilities: the same number of dependent launches with next to nothing to do."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rajepy_amd import engine as E  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "antenna_configs", "vla.a.cfg")
# maps, components (the visibilities: see `points`)
POINTS = {"tracks": (8, 1), "dense": (1, 2)}
ITER, LAM0, XTOL = 20, 1e-3, 1e-300
TWO_PI2 = 2.0 * np.pi ** 2


def timed(fn):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1), out


def model_sums(Vr, Vi, a, b, w, th, matmul=True):
    """chi^2 [M], N [M, P, P], g [M, P] of theta [M, P] at the points (a, b) [M, K] against the data
    (Vr, Vi) [M, K] with the weights w [M, K]."""
    M, P = th.shape
    rows_r, rows_i = [], []
    mr, mi = torch.zeros_like(a), torch.zeros_like(a)
    for c in range(P // 6):
        F, x, z, sxx, sxz, szz = (th[:, 6 * c + k:6 * c + k + 1] for k in range(6))
        ph = 2.0 * np.pi * (a * x + b * z)
        cs, sn = torch.cos(ph), torch.sin(ph)
        Ee = torch.exp(-TWO_PI2 * (sxx * a * a + 2.0 * sxz * a * b + szz * b * b))
        cr, ci = F * Ee * cs, -F * Ee * sn
        ka, kb = 2.0 * np.pi * a, 2.0 * np.pi * b
        rows_r += [Ee * cs, ci * ka, ci * kb, -TWO_PI2 * a * a * cr, -2.0 * TWO_PI2 * a * b * cr,
                   -TWO_PI2 * b * b * cr]
        rows_i += [-Ee * sn, -cr * ka, -cr * kb, -TWO_PI2 * a * a * ci, -2.0 * TWO_PI2 * a * b * ci,
                   -TWO_PI2 * b * b * ci]
        mr, mi = mr + cr, mi + ci
    J = torch.cat([torch.stack(rows_r, dim=1), torch.stack(rows_i, dim=1)], dim=2)      # [M, P, 2 K]
    r = torch.cat([Vr - mr, Vi - mi], dim=1)
    w2 = torch.cat([w, w], dim=1)
    wJ = J * w2[:, None, :]
    chi = (w2 * r * r).sum(dim=1)
    if matmul:
        return chi, wJ @ J.transpose(1, 2), (wJ @ r[:, :, None])[:, :, 0]
    return chi, (wJ[:, :, None, :] * J[:, None, :, :]).sum(dim=3), (wJ * r[:, None, :]).sum(dim=2)


def psd(th):
    ok = torch.ones(th.shape[0], dtype=torch.bool, device=th.device)
    for c in range(th.shape[1] // 6):
        sxx, sxz, szz = th[:, 6 * c + 3], th[:, 6 * c + 4], th[:, 6 * c + 5]
        ok &= (sxx >= 0) & (szz >= 0) & (sxx * szz >= sxz * sxz)
    return ok


def torch_lm(Vr, Vi, a, b, w, th0, n_iter, matmul=True):
    """The device-only route -> (theta, chi2, accepted steps)."""
    M, P = th0.shape
    dev = th0.device
    cur = th0.clone()
    chi_cur = torch.full((M,), float("inf"), dtype=torch.float64, device=dev)
    lam = torch.full((M,), LAM0, dtype=torch.float64, device=dev)
    N = torch.eye(P, dtype=torch.float64, device=dev).repeat(M, 1, 1)
    g = torch.zeros(M, P, dtype=torch.float64, device=dev)
    trial = th0.clone()
    n_acc = torch.zeros(M, dtype=torch.int64, device=dev)
    for t in range(n_iter):
        chi_t, N_t, g_t = model_sums(Vr, Vi, a, b, w, trial, matmul)
        acc = psd(trial) & torch.isfinite(chi_t) & (chi_t < chi_cur)
        cur = torch.where(acc[:, None], trial, cur)
        chi_cur = torch.where(acc, chi_t, chi_cur)
        N = torch.where(acc[:, None, None], N_t, N)
        g = torch.where(acc[:, None], g_t, g)
        down = lam if t == 0 else torch.clamp(lam / 10.0, min=1e-12)
        lam = torch.where(acc, down, lam * 10.0)
        n_acc += acc
        d = torch.diagonal(N, dim1=1, dim2=2)
        L, _ = torch.linalg.cholesky_ex(N + torch.diag_embed(lam[:, None] * d))
        trial = cur + torch.cholesky_solve(g[:, :, None], L)[:, :, 0]
    return cur, chi_cur, n_acc


def stats(t):
    return [float(min(t)), float(np.median(t)), float(max(t))]


def points(eng, name, g):
    """(u, v) in cycles per cell of the first map, at most 0.25, as device tensors [K]."""
    if name == "dense":
        uv = 0.5 * torch.rand(2, 1 << 18, dtype=torch.float64, device=eng.device, generator=g) - 0.25
        return uv[0].contiguous(), uv[1].contiguous()
    cfg = E.read_antenna_config(FIXTURE)
    geo = E.geodetic(cfg.xyz)
    ha = (np.arange(20) - 9.5) * 60.0 / E.SIDEREAL_DAY_S
    u, v, _ = eng.uv_tracks(cfg.xyz, ha - geo.lon0_deg / 360.0, np.radians(30.0))
    u, v = u.reshape(-1), v.reshape(-1)
    s = 0.25 / float(torch.maximum(u.abs().max(), v.abs().max()).item())
    return (u * s).contiguous(), (v * s).contiguous()


def probe(eng, name, rounds):
    M, nc = POINTS[name]
    dev = eng.device
    g = torch.Generator(device=dev)
    g.manual_seed(20240520)
    u, v = points(eng, name, g)
    K = int(u.numel())
    su = np.linspace(1.0, 0.6, M)
    sv = -su if name == "tracks" else su.copy()
    one = np.array([1.3, 2.3, -1.8, 6.0, 1.5, 3.0, 0.4, -5.1, 4.2, 2.0, -0.5, 1.0])[:6 * nc]
    truth = torch.from_numpy(np.tile(one, (M, 1))).to(dev)
    truth[:, 0::6] *= 0.5 + torch.rand(M, nc, dtype=torch.float64, device=dev, generator=g)
    col = lambda s: torch.from_numpy(s).to(dev)[:, None]
    a, b = (col(su) * u[None, :]).contiguous(), (col(sv) * v[None, :]).contiguous()
    w = torch.exp(0.5 * torch.randn(M, K, dtype=torch.float64, device=dev, generator=g))
    zero = torch.zeros(M, K, dtype=torch.float64, device=dev)
    Vr, Vi = zero.clone(), zero.clone()
    for c in range(nc):                                          # the data: the model at the truth
        F, x, z, sxx, sxz, szz = (truth[:, 6 * c + k:6 * c + k + 1] for k in range(6))
        ph = 2.0 * np.pi * (a * x + b * z)
        Ee = F * torch.exp(-TWO_PI2 * (sxx * a * a + 2.0 * sxz * a * b + szz * b * b))
        Vr, Vi = Vr + Ee * torch.cos(ph), Vi - Ee * torch.sin(ph)
    amp = truth[:, 0::6].abs().sum(dim=1, keepdim=True)
    Vr = Vr + 0.01 * amp * torch.randn(M, K, dtype=torch.float64, device=dev, generator=g)
    Vi = Vi + 0.01 * amp * torch.randn(M, K, dtype=torch.float64, device=dev, generator=g)
    V = torch.complex(Vr, Vi).contiguous()
    th0 = truth.clone()
    th0[:, 0::6] *= 1.3
    th0[:, 1::6] += 0.5
    th0[:, 2::6] -= 0.4
    th0[:, 3::6] *= 1.4
    th0[:, 5::6] *= 0.7

    k20 = lambda: eng.uvfit(V, su, sv, u, v, th0, weights=w, n_iter=ITER, lambda0=LAM0, xtol=XTOL)
    route = lambda: torch_lm(Vr, Vi, a, b, w, th0, ITER)
    route_el = lambda: torch_lm(Vr, Vi, a, b, w, th0, ITER, matmul=False)
    got, ref = k20(), route()                                    # warm-up of every shape
    ref_el = route_el()
    eng.synchronize()
    tiles = eng.last_uvfit_tiles
    sc = torch.ones_like(ref[0])
    sc[:, 0::6] = ref[0][:, 0::6].abs()
    for c in range(nc):
        sc[:, 6 * c + 3:6 * c + 6] = torch.clamp(ref[0][:, 6 * c + 3] + ref[0][:, 6 * c + 5], min=1.0)[:, None]
    theta_diff = float(((got["theta"] - ref[0]).abs() / sc).max().item())
    chi_diff = float(((got["chi2"] - ref[1]).abs() / ref[1]).max().item())
    small_v = torch.complex(torch.rand(1, 6, dtype=torch.float64, device=dev, generator=g),
                            torch.rand(1, 6, dtype=torch.float64, device=dev, generator=g))
    small_uv = 0.2 * torch.rand(2, 6, dtype=torch.float64, device=dev, generator=g)
    floor_fn = lambda: eng.uvfit(small_v, [1.0], [1.0], small_uv[0].contiguous(), small_uv[1].contiguous(),
                                 one, n_iter=ITER, lambda0=LAM0, xtol=XTOL)
    floor_fn()
    t_k20, t_route, t_route_el, t_floor = [], [], [], []
    for _ in range(rounds):                                      # alternating rounds
        t_k20.append(timed(k20)[0])
        t_route.append(timed(route)[0])
        t_floor.append(timed(floor_fn)[0])
        t_route_el.append(timed(route_el)[0])
    med = lambda t: float(np.median(t))
    return {"point": name, "visibilities": K, "maps": M, "components": nc, "iterations": ITER,
            "rounds": rounds, "workgroups_per_iteration": tiles,
            "status": sorted(set(got["status"].cpu().tolist())),
            "accepted_steps_torch": [int(ref[2].min().item()), int(ref[2].max().item())],
            "ms_k20": stats(t_k20), "ms_torch": stats(t_route),
            "ms_torch_broadcast_products": stats(t_route_el),
            "ms_k20_on_6_visibilities_same_iterations": stats(t_floor),
            "us_per_iteration_k20": 1e3 * med(t_k20) / (ITER + 1),
            "us_per_iteration_floor": 1e3 * med(t_floor) / (ITER + 1),
            "us_per_iteration_torch": 1e3 * min(med(t_route), med(t_route_el)) / ITER,
            "torch_over_k20_median": min(med(t_route), med(t_route_el)) / med(t_k20),
            "torch_over_k20_worst_case": min(t_route + t_route_el) / max(t_k20),
            "theta_max_diff_between_torch_routes": float((ref_el[0] - ref[0]).abs().max().item()),
            "theta_max_diff_over_scale": theta_diff, "chi2_max_rel_diff": chi_diff}


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
