#!/usr/bin/env python3
"""Times K14 (rjp_gaussfit: Levenberg-Marquardt fits of one elliptical Gaussian per map, one fused
launch per iteration for a whole stack of images) against a torch Levenberg-Marquardt that stays on
the device, on the same buffers, in ONE process:

    python tools/gaussfit_probe.py [--point image|cube|all] [--rounds N] [--out FILE.json]

The torch route is the same algorithm: the explicit Jacobian of the model over the box, J^T J and
J^T r by batched matrix products, the damped system by torch.linalg.cholesky_ex / cholesky_solve,
and K14's decision rule written with torch.where (accept iff positive definite, finite and better;
lambda / 10 or 10 lambda), so the route itself sends nothing to the host; whether the library calls
under torch.linalg do is not this tool's to say, so the two halves of an iteration are also timed
alone, `ITER` times each on the same operands: the sums (model_sums) and the factorisation with its
solve.  The products J J^T and J r are taken by batched matmul and, as a second route, by broadcast
products summed over the pixels; the ratios are quoted against the faster of the two.  A further variant that reads chi^2 back with one .item() per iteration and decides in Python
is timed at the single-map point for information only.
image = 501 x 501 x 1 map with a 201 x 201 box; cube = 256 x 256 x 64 maps, the whole image as the
box.  Noisy Gaussians (1 % of the peak), `ITER` = 20 iterations with xtol tiny so that neither route
stops early and both do the same work (by then the fits have converged and lambda has climbed
back, still below the 1e12 that would end K14 as stalled).  Every shape is warmed up once; then the
routes are timed with device events in alternating rounds; minimum, median and maximum of each are
reported with the ratio of the medians and the worst case for K14 (its slowest round against
torch's fastest).  The launch-bound floor of an iteration is K14 itself on a 3 x 3 image: the same
number of dependent launches with next to nothing to do."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from rajepy_amd import engine as E  # noqa: E402

# nx, nz, maps, box
POINTS = {"image": (501, 501, 1, (150, 350, 150, 350)), "cube": (256, 256, 64, (0, 255, 0, 255))}
ITER, LAM0, XTOL = 20, 1e-3, 1e-300


def timed(fn):
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev0.record()
    out = fn()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1), out


def model_sums(I, X, Z, th, matmul=True):
    """chi^2 [M], N [M, 6, 6], g [M, 6] of theta [M, 6] over the box pixels I [M, P] at (X, Z) [P];
    the products J J^T and J r by batched matmul, or (`matmul` False) by broadcast products and
    sums over the pixels."""
    S, x0, z0, A, B, C = (th[:, k:k + 1] for k in range(6))
    dx, dz = X[None, :] - x0, Z[None, :] - z0
    ex = torch.exp(-(A * dx * dx + 2.0 * B * dx * dz + C * dz * dz))
    G = S * ex
    r = I - G
    J = torch.stack([ex, G * (2.0 * A * dx + 2.0 * B * dz), G * (2.0 * B * dx + 2.0 * C * dz),
                     -G * dx * dx, -2.0 * G * dx * dz, -G * dz * dz], dim=1)          # [M, 6, P]
    if matmul:
        return (r * r).sum(dim=1), J @ J.transpose(1, 2), (J @ r[:, :, None])[:, :, 0]
    return ((r * r).sum(dim=1), (J[:, :, None, :] * J[:, None, :, :]).sum(dim=3),
            (J * r[:, None, :]).sum(dim=2))


def posdef(th):
    return (th[:, 3] > 0) & (th[:, 5] > 0) & (th[:, 3] * th[:, 5] > th[:, 4] * th[:, 4])


def torch_lm(I, X, Z, th0, n_iter, matmul=True):
    """The device-only route -> (theta, chi2, accepted steps)."""
    M = I.shape[0]
    cur = th0.clone()
    chi_cur = torch.full((M,), float("inf"), dtype=torch.float64, device=I.device)
    lam = torch.full((M,), LAM0, dtype=torch.float64, device=I.device)
    N = torch.eye(6, dtype=torch.float64, device=I.device).repeat(M, 1, 1)
    g = torch.zeros(M, 6, dtype=torch.float64, device=I.device)
    trial = th0.clone()
    n_acc = torch.zeros(M, dtype=torch.int64, device=I.device)
    for t in range(n_iter):
        chi_t, N_t, g_t = model_sums(I, X, Z, trial, matmul)
        acc = posdef(trial) & torch.isfinite(chi_t) & (chi_t < chi_cur)
        cur = torch.where(acc[:, None], trial, cur)
        chi_cur = torch.where(acc, chi_t, chi_cur)
        N = torch.where(acc[:, None, None], N_t, N)
        g = torch.where(acc[:, None], g_t, g)
        down = lam if t == 0 else torch.clamp(lam / 10.0, min=1e-12)
        lam = torch.where(acc, down, lam * 10.0)
        n_acc += acc
        d = torch.diagonal(N, dim1=1, dim2=2)
        L, _ = torch.linalg.cholesky_ex(N + torch.diag_embed(lam[:, None] * d))
        delta = torch.cholesky_solve(g[:, :, None], L)[:, :, 0]
        trial = cur + delta
    return cur, chi_cur, n_acc


def torch_lm_item(I, X, Z, th0, n_iter):
    """One .item() per iteration: chi^2 goes to the host, the decision is Python (single map)."""
    cur, chi_cur, lam = th0.clone(), float("inf"), LAM0
    trial, N, g = th0.clone(), None, None
    for t in range(n_iter):
        chi_t, N_t, g_t = model_sums(I, X, Z, trial)
        c = float(chi_t.item())
        if np.isfinite(c) and c < chi_cur:
            cur, chi_cur, N, g = trial, c, N_t, g_t
            lam = lam if t == 0 else max(lam / 10.0, 1e-12)
        else:
            lam *= 10.0
        d = torch.diagonal(N, dim1=1, dim2=2)
        L, _ = torch.linalg.cholesky_ex(N + torch.diag_embed(lam * d))
        trial = cur + torch.cholesky_solve(g[:, :, None], L)[:, :, 0]
    return cur, chi_cur


def stats(t):
    return [float(min(t)), float(np.median(t)), float(max(t))]


def probe(eng, name, rounds):
    nx, nz, M, box = POINTS[name]
    dev = eng.device
    g = torch.Generator(device=dev)
    g.manual_seed(20240514)
    i0, i1, j0, j1 = box
    qx = torch.arange(nx, dtype=torch.float64, device=dev)
    qz = torch.arange(nz, dtype=torch.float64, device=dev)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(M, 1, 1, dtype=torch.float64, device=dev, generator=g)
    S = u(0.5, 2.0) * torch.where(u(0, 1) < 0.25, -1.0, 1.0)
    x0, z0 = u(0.45 * (i0 + i1), 0.55 * (i0 + i1)), u(0.45 * (j0 + j1), 0.55 * (j0 + j1))
    w = 0.12 * min(i1 - i0, j1 - j0)
    a = 4.0 * np.log(2.0) / w ** 2
    A, C, B = u(0.6 * a, 1.8 * a), u(0.6 * a, 1.8 * a), u(-0.3 * a, 0.3 * a)
    dx, dz = qx[None, :, None] - x0, qz[None, None, :] - z0
    D = S * torch.exp(-(A * dx * dx + 2.0 * B * dx * dz + C * dz * dz))
    D += 0.01 * S.abs() * torch.randn(M, nx, nz, dtype=torch.float64, device=dev, generator=g)
    D = D.reshape(M, -1).contiguous()
    th0 = E.gauss_start(D, nx, nz, (a, 0.0, a), box=box)
    # the box of the torch routes: gathered once, outside the events
    X = qx[i0:i1 + 1, None].expand(-1, j1 - j0 + 1).reshape(-1).contiguous()
    Z = qz[None, j0:j1 + 1].expand(i1 - i0 + 1, -1).reshape(-1).contiguous()
    I = D.view(M, nx, nz)[:, i0:i1 + 1, j0:j1 + 1].reshape(M, -1).contiguous()

    k14 = lambda: eng.gaussfit(D, nx, nz, th0, box=box, n_iter=ITER, lambda0=LAM0, xtol=XTOL)
    route = lambda: torch_lm(I, X, Z, th0, ITER)
    route_el = lambda: torch_lm(I, X, Z, th0, ITER, matmul=False)
    got, ref = k14(), route()                                    # warm-up of every shape
    ref_el = route_el()
    eng.synchronize()
    tiles = eng.last_gaussfit_tiles
    sc = torch.stack([ref[0][:, 0].abs(), torch.ones_like(ref[0][:, 0]), torch.ones_like(ref[0][:, 0])]
                     + [ref[0][:, 3] + ref[0][:, 5]] * 3, dim=1)
    theta_diff = float(((got["theta"] - ref[0]).abs() / sc).max().item())
    chi_diff = float(((got["chi2"] - ref[1]).abs() / ref[1]).max().item())
    small = torch.rand(1, 9, dtype=torch.float64, device=dev, generator=g)
    floor_fn = lambda: eng.gaussfit(small, 3, 3, [1.0, 1.0, 1.0, 0.5, 0.0, 0.5], n_iter=ITER,
                                    lambda0=LAM0, xtol=XTOL)
    floor_fn()
    if M == 1:
        torch_lm_item(I, X, Z, th0, ITER)
    # the two halves of a torch iteration alone, on the operands of the route's last iteration
    _, N_end, g_end = model_sums(I, X, Z, ref[0])
    M_end = N_end + torch.diag_embed(LAM0 * torch.diagonal(N_end, dim1=1, dim2=2))

    def sums_alone():
        for _ in range(ITER):
            out = model_sums(I, X, Z, ref[0])
        return out

    def sums_el_alone():
        for _ in range(ITER):
            out = model_sums(I, X, Z, ref[0], matmul=False)
        return out

    def factor_alone():
        for _ in range(ITER):
            L, _ = torch.linalg.cholesky_ex(M_end)
            out = torch.cholesky_solve(g_end[:, :, None], L)
        return out

    def solve_alone():
        for _ in range(ITER):
            out = torch.linalg.solve(M_end, g_end[:, :, None])
        return out
    sums_alone(), sums_el_alone(), factor_alone(), solve_alone()
    t_sums, t_factor, t_solve, t_sums_el, t_route_el = [], [], [], [], []
    t_k14, t_route, t_item, t_floor = [], [], [], []
    for _ in range(rounds):                                      # alternating rounds
        t_k14.append(timed(k14)[0])
        t_route.append(timed(route)[0])
        if M == 1:
            t_item.append(timed(lambda: torch_lm_item(I, X, Z, th0, ITER))[0])
        t_floor.append(timed(floor_fn)[0])
        t_route_el.append(timed(route_el)[0])
        t_sums.append(timed(sums_alone)[0])
        t_sums_el.append(timed(sums_el_alone)[0])
        t_factor.append(timed(factor_alone)[0])
        t_solve.append(timed(solve_alone)[0])
    med = lambda t: float(np.median(t))
    rec = {"point": name, "nx": nx, "nz": nz, "maps": M, "box": list(box), "iterations": ITER,
           "rounds": rounds, "workgroups_per_iteration": tiles,
           "status": sorted(set(got["status"].cpu().tolist())),
           "accepted_steps_torch": [int(ref[2].min().item()), int(ref[2].max().item())],
           "ms_k14": stats(t_k14), "ms_torch": stats(t_route),
           "ms_k14_on_3x3_same_iterations": stats(t_floor),
           "us_per_iteration_k14": 1e3 * med(t_k14) / (ITER + 1),
           "us_per_iteration_floor": 1e3 * med(t_floor) / (ITER + 1),
           "us_per_iteration_torch": 1e3 * med(t_route) / ITER,
           "ms_torch_broadcast_products": stats(t_route_el),
           "torch_over_k14_median": min(med(t_route), med(t_route_el)) / med(t_k14),
           "torch_over_k14_worst_case": min(t_route + t_route_el) / max(t_k14),
           "theta_max_diff_between_torch_routes": float((ref_el[0] - ref[0]).abs().max().item()),
           "ms_torch_sums_alone": stats(t_sums),
           "ms_torch_sums_alone_broadcast_products": stats(t_sums_el),
           "ms_torch_cholesky_ex_and_cholesky_solve_alone": stats(t_factor),
           "ms_torch_linalg_solve_alone": stats(t_solve),
           "theta_max_diff_over_scale": theta_diff, "chi2_max_rel_diff": chi_diff}
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
