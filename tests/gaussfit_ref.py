"""A long-double NumPy reference for rjp_gaussfit (K14, imfit.hip) that FOLLOWS the device's trace,
as tests/clean_ref.py follows the component list: two correct Levenberg-Marquardt codes may part
ways on a near-tie of chi^2, so the reference never runs a fit of its own.  It takes the images as
the device read them and the trace rows (chi^2_t, lambda used, accepted, theta_t[6]) and checks,
for every iteration t (u = 2^-53):

(a) chi^2_t against its own long-double sum over the counting pixels.  Per pixel, with
    Q = A dx^2 + 2 |B dx dz| + C dz^2:
      * the exponent is formed from dx, dz (one rounding each), three products of two and three
        factors and two additions: every term within 6 u of itself, taken as 8 u Q absolute;
      * exp_any: 1e-14 relative (rjp_device.h); G = S exp(): one rounding.  So
        eG = |G| (1e-14 + 8 u Q + 2 u)  (+ 1e-300 |S| for an exponent that straddles -700);
      * r = I - G: er = eG + u |r|;  r^2: 2 |r| er + er^2 + u r^2;
      * the accumulation: a fixed tree of depth D = 4 (a thread's pixels) + 32 + 8 (the block sum)
        + ceil(tiles / 256) + 32 + 8 (the tiles' partials): D u sum r^2.
    bound = 1.01 (sum of the per-pixel terms + D u sum r^2), the 1.01 for the second-order terms.
(b) the accept flag: a trial that is not positive definite, or whose chi^2 is not finite, is
    rejected; a trial identical in all six parameters to theta_cur is rejected (the same sum in the
    same order gives the same bits, and the rule is a strict <); else the flag must agree with the
    reference's two chi^2 wherever they differ by more than the sum of their bounds (a).
(c) the proposed step delta = theta_{t+1} - theta_cur by its componentwise backward error against
    the reference's N = J^T J and g = J^T r at theta_cur, M = N + lambda diag N:
      |M delta - g|_i <= c u (sum_j |M_ij| |delta_j| + |g_i|)                 (Cholesky)
                         + u sum_j |M_ij| |theta_{t+1, j}|                    (recovering delta)
                         + sum_j bN_ij (1 + lambda [i = j]) |delta_j| + bg_i    (summation of N, g)
    c = 3 n + 1 + 3 = 22 for n = 6: gamma_{3n+1} of a Cholesky solve (Higham, Accuracy and
    Stability, Thm 10.4) plus forming M_ii = fma(lambda, N_ii, N_ii) and the rounding of g.  The
    theorem's own majorant is |R^T| |R|, whose entries sqrt(M_ii M_jj) bounds and |M_ij| need not;
    the form with |M_ij| is the one asked for and the one held here.  The second term is the
    rounding of theta_cur + delta, from which the trace's delta is recovered.  No condition number.
    bN, bg are the bounds of N and g built like (a): the Jacobian's entries are G (or exp())
    times a polynomial P in dx, dz, A, B, C, each within (1e-14 + 8 u Q + 6 u) |G| P(|.|).
(d) lambda: row 0 uses lambda0; an accepted trial gives max(lambda / 10, 1e-12) (the start leaves
    lambda0), a rejected one 10 lambda, in float64 as the device computes them; the next row's
    lambda must be that times 10^j, j the Cholesky breakdowns, and j = 0 wherever the reference's
    own factorisation has every pivot above 1e-6 of its diagonal entry.  The stop: chi^2_cur = 0,
    lambda > 1e12, the step test max |delta_i| / s_i <= xtol with the margin |M^-1| (bound of (c))
    on the reference's delta, n_iter.
(e) at the end d_theta and d_chi2 are the bits of the last accepted trace row, d_chi2 and d_cov
    are within their bounds of the reference at d_theta, d_npix is the count, d_niter the rows
    written, and the trace beyond d_niter holds the caller's poison.
`follow` returns the worst error / bound it saw; anything else fails an assertion."""
import numpy as np

from tests.lm_ref import (LAM_MAX, LAM_MIN, LD, U53, cholesky_solve, damped, pack, pivots_clear,
                          tri_list, unpack)

TILE, REDUCE_PASS, NSUM, NSTATE = 1024, 256, 29, 48
EXP_RTOL = 1e-14
C_CHOL = 22.0
# the library's refusals, in the order check_gaussfit makes them; the workspace comes last
MSG = {"nulls": "rjp_gaussfit: NULL images, box, parameters or outputs",
       "sizes": "rjp_gaussfit: n_maps, nx and nz must be positive",
       "npix": "rjp_gaussfit: nx * nz exceeds 2^31 - 1",
       "box": "rjp_gaussfit: the box (i0, i1, j0, j1) must lie inside the image, i0 <= i1 and j0 <= j1",
       "tol": "rjp_gaussfit: lambda0 and xtol must be finite and positive",
       "iter": "rjp_gaussfit: n_iter < 1",
       "wgs": "rjp_gaussfit: more than 2^31 - 1 workgroups",
       "short": "rjp_gaussfit: workspace smaller than rjp_gaussfit_workspace()"}
PARTS = {}                   # the worst error / bound of checks (a), (c) and d_cov seen by `follow`


def tri(i, j):
    """Index of (i, j), i <= j, in the packed upper triangle, row by row."""
    return tri_list(6).index((i, j))


TRI = tri_list(6)


def box_pixels(box):
    return (box[1] - box[0] + 1) * (box[3] - box[2] + 1)


def tiling(n_maps, npix_box):
    tiles = (npix_box + TILE - 1) // TILE
    return {"tiles": tiles, "workgroups": tiles * n_maps}


def workspace_bytes(n_maps, npix_box):
    return (tiling(n_maps, npix_box)["workgroups"] * NSUM + n_maps * NSTATE) * 2 * 8


def depth(npix_box):
    tiles = tiling(1, npix_box)["tiles"]
    return 4 + 32 + 8 + (tiles + REDUCE_PASS - 1) // REDUCE_PASS + 32 + 8


def posdef(th):
    return bool(th[3] > 0 and th[5] > 0 and th[3] * th[5] > th[4] * th[4])


def counting(img, box, mask):
    """(ix, iz, I) of the pixels that count: inside the box, unmasked, finite."""
    i0, i1, j0, j1 = box
    ok = np.zeros(img.shape, dtype=bool)
    ok[i0:i1 + 1, j0:j1 + 1] = True
    if mask is not None:
        ok &= np.asarray(mask) != 0
    ok &= np.isfinite(img)
    ix, iz = np.nonzero(ok)
    return ix, iz, img[ix, iz]


def model(theta, ix, iz, dtype=LD, centre=0.0, with_jac=True, b_factor=2.0):
    """G and the Jacobian [6, n] at the pixels (ix, iz), in `dtype`; an exact 0 below an exponent of
    -700.  (`centre`, `b_factor`: the planted mistakes of tests/test_gaussfit_reference_cpu.py.)"""
    S, x0, z0, A, B, C = (dtype(t) for t in theta)
    dx = ix.astype(dtype) - x0 + dtype(centre)
    dz = iz.astype(dtype) - z0 + dtype(centre)
    e = -(A * dx * dx + 2 * B * dx * dz + C * dz * dz)
    with np.errstate(all="ignore"):
        ex = np.where(e < -700, dtype(0), np.exp(np.maximum(e, dtype(-745))))
        ex = np.where(np.isnan(e), dtype(np.nan), ex)
        G = S * ex
        if not with_jac:
            return G, None
        J = np.stack([ex, G * (2 * A * dx + 2 * B * dz), G * (2 * B * dx + 2 * C * dz),
                      -G * dx * dx, -dtype(b_factor) * G * dx * dz, -G * dz * dz])
    return G, J


class Sums:
    """chi^2, N [21], g [6] of `theta` over the counting pixels in long double, with the bounds of
    the module docstring (bchi, bN [21], bg [6]) for a box of `npix_box` pixels."""

    def __init__(self, theta, pix, npix_box, want_jac=True):
        ix, iz, I = pix
        th = [LD(t) for t in theta]
        S, x0, z0, A, B, C = th
        G, J = model(th, ix, iz, LD, with_jac=want_jac)
        dx, dz = ix.astype(LD) - x0, iz.astype(LD) - z0
        r = I.astype(LD) - G
        Q = A * dx * dx + 2 * np.abs(B * dx * dz) + C * dz * dz
        D = depth(npix_box) * LD(U53)
        u = LD(U53)
        relG = LD(EXP_RTOL) + 8 * u * Q + 2 * u
        eG = np.abs(G) * relG + LD(1e-300) * abs(S)
        er = eG + u * np.abs(r)
        self.n = int(I.size)
        self.chi2 = LD(np.sum(r * r))
        self.bchi = LD(1.01) * (np.sum(2 * np.abs(r) * er + er * er + u * r * r) + D * self.chi2)
        if not want_jac:
            return
        # (a pixel whose exponential is an exact 0 adds nothing to N, g or their bounds)
        live = J[0] != 0
        if not live.all():
            J, G, r, er, relG, dx, dz = (a[..., live] for a in (J, G, r, er, relG, dx, dz))
        aG = np.abs(G)
        ex = np.abs(J[0])
        Jabs = np.stack([ex, aG * (np.abs(2 * A * dx) + np.abs(2 * B * dz)),
                         aG * (np.abs(2 * B * dx) + np.abs(2 * C * dz)), aG * dx * dx,
                         2 * aG * np.abs(dx * dz), aG * dz * dz])
        eJ = Jabs * (relG + 6 * u) + LD(1e-300)
        ar = np.abs(r)
        self.N = pack(J @ J.T)
        cross = Jabs @ eJ.T
        self.bN = LD(1.01) * pack(cross + cross.T + eJ @ eJ.T + (u + D) * (Jabs @ Jabs.T))
        self.g = J @ r
        self.bg = LD(1.01) * (Jabs @ er + eJ @ ar + eJ @ er + (u + D) * (Jabs @ ar))


def scales(th):
    sh = abs(th[3] + th[5])
    return np.array([max(abs(th[0]), 1e-300), 1.0, 1.0, sh, sh, sh], dtype=LD)


def step_bound(s, lam, delta, theta_next):
    """The bound of (c) on |M delta - g|, per component (long double)."""
    M = damped(unpack(s.N, 6), LD(lam))
    ad = np.abs(np.asarray(delta, dtype=LD))
    bM = unpack(s.bN, 6)
    for i in range(6):
        bM[i, i] *= 1 + LD(lam)
    u = LD(U53)
    return (LD(C_CHOL) * u * (np.abs(M) @ ad + np.abs(s.g))
            + u * np.abs(M) @ np.abs(np.asarray(theta_next, dtype=LD)) + bM @ ad + s.bg)


def emulate(img, box, mask, theta0, lambda0, xtol, n_iter, poison=None, mistake=None):
    """The device's arithmetic in float64 NumPy (np.exp, np.sum: other roundings, inside the
    bounds) -> dict like the device's outputs (theta, chi2, cov, npix, niter, status, trace), or
    status 3 with theta None.  `mistake`: one of "centre" (a centre off by half a pixel), "b_factor"
    (no factor 2 on the B derivative), "lam_identity" (lambda I for lambda diag N), "accept_le"
    (accept on <=)."""
    f = np.float64
    pix = counting(img, box, mask)
    ix, iz, I = pix
    trace = np.full((n_iter, 9), np.nan if poison is None else poison)
    th_t = np.array(theta0, dtype=f)
    out = dict(theta=None, chi2=None, cov=None, npix=None, niter=None, status=3, trace=trace)
    if not (np.all(np.isfinite(th_t)) and posdef(th_t)):
        return out
    cur, chi_cur, lam, lam_used, N, g = th_t.copy(), np.inf, f(lambda0), f(lambda0), None, None
    status, it = None, 0
    while status is None:
        it += 1
        G, J = model(th_t, ix, iz, f, centre=0.5 if mistake == "centre" else 0.0,
                     b_factor=1.0 if mistake == "b_factor" else 2.0)
        r = I - G
        with np.errstate(all="ignore"):
            chi_t = f(np.sum(r * r))
        if it == 1 and (I.size < 6 or not np.isfinite(chi_t)):
            return out
        better = chi_t <= chi_cur if mistake == "accept_le" else chi_t < chi_cur
        acc = bool(posdef(th_t) and np.isfinite(chi_t) and better)
        trace[it - 1] = [chi_t, lam_used, float(acc)] + list(th_t)
        if acc:
            cur, chi_cur = th_t.copy(), chi_t
            with np.errstate(all="ignore"):
                N = np.array([np.sum(J[a] * J[b]) for a, b in TRI])
                g = np.array([np.sum(J[a] * r) for a in range(6)])
            if it > 1:
                lam = max(lam / f(10.0), f(LAM_MIN))
        else:
            lam = lam * f(10.0)
        if chi_cur == 0.0:
            status = 1
            break
        while True:
            if lam > LAM_MAX:
                status = 2
                break
            delta, ok = cholesky_solve(damped(unpack(N, 6), lam, identity=mistake == "lam_identity"), g)
            if ok:
                break
            lam = lam * f(10.0)
        if status is not None:
            break
        with np.errstate(all="ignore"):
            worst = np.max(np.abs(delta) / scales(cur).astype(f))
        if not np.any(np.isnan(delta)) and worst <= xtol:
            status = 1
        elif it == n_iter:
            status = 0
        else:
            th_t, lam_used = cur + delta, lam
    out.update(theta=cur, chi2=chi_cur, cov=N, npix=int(I.size), niter=it, status=status)
    return out


def follow(img, box, mask, theta0, lambda0, xtol, n_iter, out, poison):
    """Checks (a)-(e) of the module docstring on one map: `img` [nx, nz] as the device read it,
    `out` the device's (theta, chi2, cov, npix, niter, status, trace [n_iter, 9]) of a map whose
    status is not 3 -> the worst error / bound.  `poison`: what the trace held before the call."""
    pix = counting(img, box, mask)
    nb = box_pixels(box)
    trace, niter, status = np.asarray(out["trace"]), int(out["niter"]), int(out["status"])
    assert pix[2].size >= 6 and int(out["npix"]) == pix[2].size, "d_npix"
    assert 1 <= niter <= n_iter and status in (0, 1, 2), (niter, status)
    assert np.all(trace[niter:] == poison), "a trace row beyond d_niter was written"
    assert np.array_equal(trace[0, 3:], np.asarray(theta0, dtype=np.float64)), "row 0 is the start"
    worst = 0.0
    lam = np.float64(lambda0)
    cur = s_cur = None
    chi_cur_dev = np.inf
    for t in range(niter):
        chi_t, lam_used, acc = trace[t, 0], trace[t, 1], trace[t, 2]
        th_t = trace[t, 3:]
        assert acc in (0.0, 1.0)
        # (d) the lambda of this row
        if t == 0:
            assert lam_used == lam, "row 0 uses lambda0"
        good = posdef(th_t) and np.all(np.isfinite(th_t))
        s_t = Sums(th_t, pix, nb) if good else None
        # (a)
        if s_t is not None and np.isfinite(float(s_t.chi2)):
            err, bnd = abs(LD(chi_t) - s_t.chi2), s_t.bchi
            ratio = float(err / bnd) if bnd > 0 else (0.0 if err == 0 else np.inf)
            assert ratio <= 1.0, ("chi^2 of trial %d" % t, float(err), float(bnd))
            worst = max(worst, ratio)
            PARTS["chi2"] = max(PARTS.get("chi2", 0.0), ratio)
        # (b)
        if not good or not np.isfinite(chi_t):
            assert acc == 0.0, "a trial that is not positive definite / finite was accepted"
        elif cur is not None and np.array_equal(th_t, cur):
            assert acc == 0.0, "a trial identical to theta_cur was accepted"
        elif cur is None:
            assert acc == 1.0, "the start was not accepted"
        else:
            margin = s_t.bchi + s_cur.bchi
            if s_t.chi2 < s_cur.chi2 - margin:
                assert acc == 1.0, ("trial %d is better beyond the bounds, but was rejected" % t)
            elif s_t.chi2 > s_cur.chi2 + margin:
                assert acc == 0.0, ("trial %d is worse beyond the bounds, but was accepted" % t)
            assert bool(acc) == bool(chi_t < chi_cur_dev), "the flag against the device's own chi^2"
        if acc:
            cur, s_cur, chi_cur_dev = th_t.copy(), s_t, chi_t
            if t > 0:
                lam = max(lam / np.float64(10.0), np.float64(LAM_MIN))
        else:
            lam = lam * np.float64(10.0)
        last = t == niter - 1
        if chi_cur_dev == 0.0:
            assert last and status == 1, "chi^2 = 0 ends the fit with status 1"
            break
        # the reference's own factorisation: breakdowns, the step and its margin
        if last:
            # (the device's own breakdowns are not on record: a lambda whose pivots are all clear
            # cannot have broken down)
            while lam <= LAM_MAX and status == 2 and not pivots_clear(damped(unpack(s_cur.N, 6), LD(lam))):
                lam = lam * np.float64(10.0)
            assert (status == 2) == bool(lam > LAM_MAX), ("status 2 iff lambda > 1e12", status, lam)
            if status == 2:
                break
        else:
            j = 0
            while lam != trace[t + 1, 1]:
                assert j < 25 and lam < trace[t + 1, 1] and \
                    not pivots_clear(damped(unpack(s_cur.N, 6), LD(lam))), \
                    ("lambda of row %d" % (t + 1), trace[t + 1, 1], lam)
                lam, j = lam * np.float64(10.0), j + 1
            assert lam <= LAM_MAX
        M = damped(unpack(s_cur.N, 6), LD(lam))
        d_ref, ok = cholesky_solve(M, s_cur.g)
        if last and not ok:
            break                                     # (a breakdown in the last launch: no step to judge)
        assert ok, "the reference's factorisation broke down where the device's went through"
        sc = scales(cur)
        with np.errstate(all="ignore"):
            w_ref = float(np.max(np.abs(d_ref) / sc))
            slack = float(np.max((np.abs(np.linalg.inv(M.astype(np.float64))).astype(LD)
                                  @ step_bound(s_cur, lam, d_ref, cur + d_ref)) / sc))
        if last:
            if status == 1:
                assert w_ref <= xtol + slack, ("stopped converged with a step of", w_ref, slack)
            else:
                assert status == 0 and niter == n_iter, (status, niter)
                assert w_ref >= xtol - slack, ("exhausted, but the step converged", w_ref, slack)
            break
        assert w_ref >= xtol - slack, ("went on after a converged step", t, w_ref, slack)
        # (d) the next row's lambda, (c) the step
        assert trace[t + 1, 1] == lam, ("lambda of row %d" % (t + 1), trace[t + 1, 1], lam)
        th_n = trace[t + 1, 3:]
        delta = th_n.astype(LD) - cur.astype(LD)
        resid = np.abs(M @ delta - s_cur.g)
        bnd = step_bound(s_cur, lam, delta, th_n)
        ratio = float(np.max(resid / bnd))
        assert ratio <= 1.0, ("step %d" % t, ratio)
        worst = max(worst, ratio)
        PARTS["step"] = max(PARTS.get("step", 0.0), ratio)
    # (e)
    assert cur is not None
    assert np.array_equal(np.asarray(out["theta"]), cur), "d_theta is the last accepted trial"
    assert out["chi2"] == chi_cur_dev, "d_chi2 is the last accepted chi^2"
    cov = np.asarray(out["cov"]).astype(LD)
    ratio = float(np.max(np.abs(cov - s_cur.N) / s_cur.bN))
    assert ratio <= 1.0, ("d_cov", ratio)
    PARTS["cov"] = max(PARTS.get("cov", 0.0), ratio)
    return max(worst, ratio)
