"""A long-double NumPy reference for K21 (specfit.hip): rjp_cube_moments per pixel, and rjp_specfit
by FOLLOWING the device's trace, as tests/uvfit_ref.py follows K20's -- two correct
Levenberg-Marquardt codes may part ways on a near-tie of chi^2, so the reference never runs a fit
of its own.  The sums are vectorised over (pixel, trial) rows (`Sums`); the decisions are judged
pixel by pixel (`follow`).  u = 2^-53, n = the counted channels of the pixel (the length of every
chain), P = 3 n_comp + 2.  Every bound below is derived from the arithmetic the header comment of
rjp_cube_moments / rjp_specfit (include/rjprt.h) states; none is measured.

MOMENTS (`check_moments`).  Over the counted channels (y finite, |y| >= clip; exact):
  m0 = chain of fma(y, dx, .): the product is exact inside the fma, n roundings of partial sums:
       |m0 - M0| <= b0 = 1.01 n u sum |y| dx;
  s1 = chain of fma(y * dx, x - x_ref, .): y * dx and x - x_ref round once each (2 u relative on
       the term), n roundings of partial sums: b1 = 1.01 (n + 2) u sum |y dx (x - x_ref)|;
  m1 = x_ref + s1 / m0: the quotient is within (b1 + |q| b0) / (|m0| - b0) of q = S1 / M0, rounds
       once (u |q|), and the sum rounds once (u |m1|):  bm1 = the three terms, times 1.01;
  s2 = chain of fma(y * dx, d * d, .), d = x - m1: d rounds once and carries the error of m1,
       |d - D| <= bm1 + u |D| =: ed, so d * d is within 2 |D| ed + ed^2 + u D^2 of D^2; with the
       rounding of y * dx and the chain:
       b2 = 1.01 sum |y| dx (2 |D| ed + ed^2 + 2 u D^2) + 1.01 n u sum |y| dx D^2;
  m2 = sqrt(s2 / m0): q2 within e2 = (b2 + |q2| b0) / (|m0| - b0) + u |q2| of Q2, and the root
       rounds once: sqrt(max(Q2 - e2, 0)) (1 - u) <= m2 <= sqrt(Q2 + e2) (1 + u); NaN is right
       where Q2 + e2 < 0 and admissible where Q2 - e2 < 0.
  The peak, ipeak and the count are exact; so is the pattern (+0.0, NaN, NaN, NaN, -1) of a pixel
  without counted channels.  Where |M0| <= b0 the device's own m0 may or may not be an exact 0:
  either the pattern or an m0 within b0 is right, m1 and m2 are not judged.

FIT, per (pixel, trial) and counted channel (y finite, w > 0) and component, as the header forms
them:
  d = x - x0 rounds once, z = d / s once more: z within 2 u |z|; z * z rounds once (the factor
  -0.5 is exact): e within 5 u |e|, 1.01 for the second order; exp_any: 1e-14 relative
  (rjp_device.h): E within r_E = 1e-14 + 5.05 u |e| relative (+ 1e-300 absolute for an exponent
  that straddles -700); A * E rounds once: the component within |A| E (r_E + u);
  the model: n_comp - 1 roundings of the component sum, the baseline fma(b1, x - x_ref, b0) with
  its rounded x - x_ref (u |b1 (x - x_ref)|) and its own rounding (u |base|), one more for the
  sum with the baseline (u |model|), and r = y - model rounds once:
    e_r = sum_c |A| E (r_E + u) + (n_comp - 1) u sum_c |A| E + u |b1 (x - x_ref)| + u |base|
          + u |model| + u |r|;
(a) chi^2 = chain of fma(w * r, r, .): w * r rounds once, n roundings of partial sums:
    bchi = 1.01 (sum w (2 |r| e_r + e_r^2 + u r^2) + n u chi^2).
  The Jacobian: dA = E within E r_E; dx0 = ((A E) z) r with r = 1 / s rounded (component r_E + u,
  z 2 u, two products and the reciprocal u each): within |dx0| (r_E + 6 u); ds = dx0 z (z 2 u, one
  product): within |ds| (r_E + 9 u); db0 = 1 exact; db1 = x - x_ref within u |x - x_ref|.
  N_ij = chain of fma(w * J_i, J_j, .), g_i = chain of fma(w * J_i, r, .), w * J_i rounded once:
    bN_ij = 1.01 sum w (|J_i| eJ_j + eJ_i |J_j| + eJ_i eJ_j + (2 + n) u |J_i J_j|)
    bg_i  = 1.01 sum w (|J_i| e_r + eJ_i |r| + eJ_i e_r + (2 + n) u |J_i r|).
  Underflow: a product w * r or w * J_i, or an fma, that falls below the normal range errs by at
  most 2^-1075 absolutely; per channel that is 2^-1075 (1 + |r|) on chi^2 and g_i and 2^-1075 (1 +
  |J_j|) on N_ij: n 2^-1074 (1 + max |r|), n 2^-1074 (1 + max |J_j|) are added to the bounds (they
  matter only where a fitted amplitude has gone to 1e-150 and below: a flat spectrum).
(b) the accept flag: a trial with an s_c that is not finite and > 0, or whose chi^2 is not finite,
    is rejected; a trial identical to theta_cur is rejected (same sums, strict <); else the flag
    must agree with the reference's two chi^2 wherever they differ by more than the sum of their
    bounds, and always with the device's own two chi^2.
(c) the proposed step delta = theta_{t+1} - theta_cur: a FIXED parameter's is exactly 0; the free
    ones by their componentwise backward error against the reference's N, g at theta_cur
    (identity rows for fixed parameters), M = N + lambda diag N:
      |M delta - g|_i <= c u (sum_j (|L| |L^T|)_ij |delta_j| + |g_i|)      (Cholesky; L the
                                                                          reference's factor of M)
                         + u sum_j |M_ij| |theta_{t+1, j}|                (recovering delta)
                         + sum_j bN_ij (1 + lambda [i = j]) |delta_j| + bg_i
    c = 3 P + 4: gamma_{3P+1} of a Cholesky solve (Higham, Accuracy and Stability, Thm 10.4) plus
    forming M_ii = fma(lambda, N_ii, N_ii) and the rounding of g.
(d) lambda, the stop and the status: K20's rules (tests/uvfit_ref.py (d)) with the step scale
    (max(|A|, 1e-300), max(s, 1e-300), max(s, 1e-300)) per component, max(|b0|, 1e-300),
    max(|b1|, 1e-300).
(e) at the end d_theta and d_chi2 are the bits of the last accepted trace row, d_cov is within bN
    of the reference at d_theta (the identity's entries exactly), d_nchan is the count, d_niter
    the rows written, and the trace beyond d_niter holds the caller's poison.
`follow` returns the worst error / bound it saw; anything else fails an assertion."""
import numpy as np

from tests.lm_ref import (LAM_MAX, LAM_MIN, LD, U53, cholesky_solve, damped, pack, pivots_clear,
                          tri_list, unpack)

EXP_RTOL = 1e-14
MAX_COMP, MAX_CHAN, LANES = 2, 4096, 64
MSG_M = {"nulls": "rjp_cube_moments: NULL cube, axis, widths or output",
         "sizes": "rjp_cube_moments: n_pix and n_chan must be positive",
         "chan": "rjp_cube_moments: n_chan exceeds RJP_SPECFIT_MAX_CHAN (4096)",
         "x": "rjp_cube_moments: non-finite h_x",
         "dx": "rjp_cube_moments: negative or non-finite h_dx",
         "xref": "rjp_cube_moments: non-finite x_ref",
         "clip": "rjp_cube_moments: clip must be finite and >= 0",
         "wgs": "rjp_cube_moments: more than 2^31 - 1 workgroups"}
MSG_F = {"nulls": "rjp_specfit: NULL cube, axis, parameters or outputs",
         "sizes": "rjp_specfit: n_pix and n_chan must be positive",
         "chan": "rjp_specfit: n_chan exceeds RJP_SPECFIT_MAX_CHAN (4096)",
         "comp": "rjp_specfit: n_comp must lie in 1 .. RJP_SPECFIT_MAX_COMP (2)",
         "x": "rjp_specfit: non-finite h_x",
         "xref": "rjp_specfit: non-finite x_ref",
         "w": "rjp_specfit: negative or non-finite h_w",
         "free": "rjp_specfit: no free parameter",
         "tol": "rjp_specfit: lambda0 and xtol must be finite and positive",
         "iter": "rjp_specfit: n_iter < 1",
         "wgs": "rjp_specfit: more than 2^31 - 1 workgroups"}
PARTS = {}                   # the worst error / bound per check seen by `follow` / `check_moments`


def _part(k, r):
    PARTS[k] = max(PARTS.get(k, 0.0), float(r))


def workgroups(n_pix):
    return (n_pix + LANES - 1) // LANES


# ---- moments -----------------------------------------------------------------------------------
def moments(y, x, dx, x_ref, clip=0.0, live=True, dtype=LD, mistake=None):
    """The moments of ONE spectrum `y` [C] in `dtype` -> dict(m0, m1, m2, peak, ipeak, count) as
    the header defines them (dtype float64: the emulation, np.sum for the chains).  `mistake`:
    "no_dx_m1" (dx ignored in m1), "var_xref" (the variance about x_ref instead of m1),
    "peak_abs" (the peak by |y|)."""
    y = np.asarray(y, dtype=np.float64)
    nan = dtype(np.nan)
    ok = np.isfinite(y) & (np.abs(y) >= clip) if live else np.zeros(y.size, dtype=bool)
    n = int(ok.sum())
    out = dict(m0=dtype(0), m1=nan, m2=nan, peak=nan, ipeak=-1, count=n)
    if n == 0:
        return out
    idx = np.nonzero(ok)[0]
    yy, xx, dd = y[ok].astype(dtype), np.asarray(x)[ok].astype(dtype), np.asarray(dx)[ok].astype(dtype)
    m0 = np.sum(yy * dd)
    if m0 == 0:
        return out
    with np.errstate(all="ignore"):
        s1 = np.sum((yy if mistake == "no_dx_m1" else yy * dd) * (xx - dtype(x_ref)))
        m1 = dtype(x_ref) + s1 / (np.sum(yy) if mistake == "no_dx_m1" else m0)
        about = dtype(x_ref) if mistake == "var_xref" else m1
        q2 = np.sum(yy * dd * (xx - about) ** 2) / m0
        m2 = nan if q2 < 0 else np.sqrt(q2)
    k = int(np.argmax(np.abs(yy) if mistake == "peak_abs" else yy))     # (the first on a tie)
    out.update(m0=m0, m1=m1, m2=m2, peak=yy[k], ipeak=int(idx[k]), count=n)
    return out


def check_moments(y, x, dx, x_ref, clip, live, got):
    """One pixel of rjp_cube_moments, `got` = dict(m0, m1, m2, peak, ipeak, count) of the device,
    against the long-double reference at the module docstring's bounds -> the worst error / bound."""
    u = LD(U53)
    ref = moments(y, x, dx, x_ref, clip, live, LD)
    assert int(got["count"]) == ref["count"], ("count", got["count"], ref["count"])
    special = (got["m0"] == 0.0 and not np.signbit(got["m0"]) and np.isnan(got["m1"]) and
               np.isnan(got["m2"]) and np.isnan(got["peak"]) and int(got["ipeak"]) == -1)
    if ref["count"] == 0:
        assert special, "a pixel without counted channels"
        return 0.0
    yf = np.asarray(y, dtype=np.float64)
    ok = np.isfinite(yf) & (np.abs(yf) >= clip)
    yy, xx, dd = yf[ok].astype(LD), np.asarray(x)[ok].astype(LD), np.asarray(dx)[ok].astype(LD)
    n = LD(ref["count"])
    M0 = np.sum(yy * dd)
    ayd = np.abs(yy) * dd
    b0 = LD(1.01) * n * u * np.sum(ayd)
    if abs(M0) <= b0:
        if special:
            return 0.0
        assert abs(LD(got["m0"]) - M0) <= b0, "m0 of a cancelling spectrum"
        return 0.0
    assert not special, "the empty pattern on a pixel whose m0 is clear of 0"
    assert got["peak"] == float(ref["peak"]) and int(got["ipeak"]) == ref["ipeak"], "the peak"
    worst = float(abs(LD(got["m0"]) - M0) / b0) if b0 > 0 else float(LD(got["m0"]) != M0)
    _part("m0", worst)
    xr = xx - LD(x_ref)
    b1 = LD(1.01) * (n + 2) * u * np.sum(ayd * np.abs(xr))
    q = np.sum(yy * dd * xr) / M0
    den = abs(M0) - b0
    bm1 = LD(1.01) * ((b1 + abs(q) * b0) / den + u * abs(q) + u * abs(ref["m1"]))
    r1 = float(abs(LD(got["m1"]) - ref["m1"]) / bm1) if bm1 > 0 else float(LD(got["m1"]) != ref["m1"])
    _part("m1", r1)
    D = xx - ref["m1"]
    ed = bm1 + u * np.abs(D)
    b2 = LD(1.01) * (np.sum(ayd * (2 * np.abs(D) * ed + ed * ed + 2 * u * D * D)) +
                     n * u * np.sum(ayd * D * D))
    Q2 = np.sum(yy * dd * D * D) / M0
    e2 = (b2 + abs(Q2) * b0) / den + u * abs(Q2)
    if np.isnan(got["m2"]):
        assert Q2 - e2 < 0, ("m2 is NaN where s2 / m0 is clear of 0", float(Q2), float(e2))
        r2 = 0.0
    else:
        assert Q2 + e2 >= 0, "m2 is a number where s2 / m0 < 0"
        lo, hi = np.sqrt(max(Q2 - e2, LD(0))) * (1 - u), np.sqrt(Q2 + e2) * (1 + u)
        mid, half = (hi + lo) / 2, (hi - lo) / 2
        r2 = float(abs(LD(got["m2"]) - mid) / half) if half > 0 else float(LD(got["m2"]) != mid)
    _part("m2", r2)
    worst = max(worst, r1, r2)
    assert worst <= 1.0, ("moments", worst, dict(m0=PARTS["m0"], m1=r1, m2=r2))
    return worst


# ---- the fit -----------------------------------------------------------------------------------
def feasible(th):
    th = np.asarray(th, dtype=np.float64)
    s = th[..., 2:-2:3]
    return np.all(np.isfinite(s) & (s > 0), axis=-1)


def scales(th):
    th = np.asarray(th)
    out = []
    for c in range((th.size - 2) // 3):
        s = max(th[3 * c + 2], 1e-300)
        out += [max(abs(th[3 * c]), 1e-300), s, s]
    out += [max(abs(th[-2]), 1e-300), max(abs(th[-1]), 1e-300)]
    return np.array(out, dtype=LD)


def model(TH, x, x_ref, dtype=LD, two_s2=True):
    """(m [R, C], J [R, P, C], E [R, nc, C], e [R, nc, C]) of the rows `TH` [R, P] at the channels
    `x` [C] in `dtype`; an exact 0 of E below an exponent of -700.  `two_s2` False: the planted
    mistake exp(-(x - x0)^2 / s^2)."""
    TH = np.atleast_2d(np.asarray(TH)).astype(dtype)
    R, P = TH.shape
    nc = (P - 2) // 3
    xx = np.asarray(x).astype(dtype)[None, :]
    xr = xx - dtype(x_ref)
    half = dtype(0.5) if two_s2 else dtype(1.0)
    m = np.zeros((R, xx.shape[1]), dtype=dtype)
    J = np.zeros((R, P, xx.shape[1]), dtype=dtype)
    Es, es = np.zeros((R, nc, xx.shape[1]), dtype=dtype), np.zeros((R, nc, xx.shape[1]), dtype=dtype)
    with np.errstate(all="ignore"):
        for c in range(nc):
            A, x0, s = TH[:, 3 * c, None], TH[:, 3 * c + 1, None], TH[:, 3 * c + 2, None]
            z = (xx - x0) / s
            e = -half * z * z
            E = np.where(e < -700, dtype(0), np.exp(np.clip(e, dtype(-745), dtype(0))))
            E = np.where(np.isnan(e), dtype(np.nan), E)
            Es[:, c], es[:, c] = E, e
            m += A * E
            J[:, 3 * c] = E
            J[:, 3 * c + 1] = A * E * z / s * (2 * half)
            J[:, 3 * c + 2] = A * E * z * z / s * (2 * half)
        m += TH[:, P - 2, None] + TH[:, P - 1, None] * xr
    J[:, P - 2] = 1
    J[:, P - 1] = xr
    return m, J, Es, es


class Sums:
    """chi^2 [R], N [R, P, P], g [R, P] and the bounds (bchi, bN, bg) of the module docstring, in
    long double, of the trial rows `TH` [R, P] on the spectra `Y` [R, C] (row r's own spectrum),
    the axis `x`, weights `w` (None: ones), `free` [P] bool (identity rows, zero bounds)."""

    def __init__(self, TH, Y, x, w, x_ref, free=None):
        TH = np.atleast_2d(np.asarray(TH, dtype=np.float64))
        Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
        R, P = TH.shape
        nc = (P - 2) // 3
        fr = np.ones(P, dtype=bool) if free is None else np.asarray(free, dtype=bool)
        wv = np.ones(Y.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
        ok = np.isfinite(Y) & (wv > 0)[None, :]
        W = np.where(ok, wv[None, :], 0.0).astype(LD)
        Yl = np.where(ok, Y, 0.0).astype(LD)
        u = LD(U53)
        n = ok.sum(axis=1).astype(LD)
        self.count = ok.sum(axis=1)
        m, J, Es, es = model(TH, x, x_ref, LD)
        THl = TH.astype(LD)
        xr = np.asarray(x).astype(LD)[None, :] - LD(x_ref)
        with np.errstate(all="ignore"):
            r = Yl - m
            AE = np.abs(THl[:, 0:3 * nc:3, None]) * Es                  # [R, nc, C]
            rE = LD(EXP_RTOL) + LD(5.05) * u * np.abs(es)
            base = THl[:, P - 2, None] + THl[:, P - 1, None] * xr
            er = (np.sum(AE * (rE + u) + LD(1e-300) * np.abs(THl[:, 0:3 * nc:3, None]), axis=1)
                  + (nc - 1) * u * AE.sum(axis=1) + u * np.abs(THl[:, P - 1, None] * xr)
                  + u * np.abs(base) + u * np.abs(m) + u * np.abs(r))
            self.chi2 = np.sum(W * r * r, axis=1)
            tiny = LD(2.0) ** -1074
            rmax = np.max(np.where(ok, np.abs(r), 0), axis=1)
            self.bchi = LD(1.01) * (np.sum(W * (2 * np.abs(r) * er + er * er + u * r * r), axis=1)
                                    + n * u * self.chi2) + n * tiny * (1 + rmax)
            Ja = np.abs(J)
            eJ = np.zeros_like(J)
            for c in range(nc):
                eJ[:, 3 * c] = Es[:, c] * rE[:, c] + LD(1e-300)
                eJ[:, 3 * c + 1] = Ja[:, 3 * c + 1] * (rE[:, c] + 6 * u) + LD(1e-300)
                eJ[:, 3 * c + 2] = Ja[:, 3 * c + 2] * (rE[:, c] + 9 * u) + LD(1e-300)
            eJ[:, P - 1] = u * np.abs(xr)
            wJ, wJa, weJ = J * W[:, None, :], Ja * W[:, None, :], eJ * W[:, None, :]
            N = np.einsum("ric,rjc->rij", wJ, J)
            g = np.einsum("ric,rc->ri", wJ, r)
            k = (2 + n)[:, None, None] * u
            cross = np.einsum("ric,rjc->rij", wJa, eJ)
            bN = LD(1.01) * (cross + cross.transpose(0, 2, 1) + np.einsum("ric,rjc->rij", weJ, eJ)
                             + k * np.einsum("ric,rjc->rij", wJa, Ja))
            ar = np.abs(r)
            Jmax = np.max(np.where(ok[:, None, :], Ja, 0), axis=2)                 # [R, P]
            bN = bN + (n * tiny)[:, None, None] * (1 + Jmax[:, None, :])
            bg = LD(1.01) * (np.einsum("ric,rc->ri", wJa, er) + np.einsum("ric,rc->ri", weJ, ar)
                             + np.einsum("ric,rc->ri", weJ, er)
                             + k[:, 0] * np.einsum("ric,rc->ri", wJa, ar)) \
                + (n * tiny * (1 + rmax))[:, None]
        for i in range(P):
            if not fr[i]:
                N[:, i, :] = N[:, :, i] = 0
                bN[:, i, :] = bN[:, :, i] = 0
                N[:, i, i] = 1
                g[:, i] = bg[:, i] = 0
        self.N, self.bN, self.g, self.bg = N, bN, g, bg

    def row(self, r):
        s = object.__new__(Sums)
        s.chi2, s.bchi, s.N, s.bN, s.g, s.bg = (self.chi2[r], self.bchi[r], self.N[r], self.bN[r],
                                                self.g[r], self.bg[r])
        return s


def step_bound(s, lam, delta, theta_next):
    """The bound of (c) on |M delta - g|, per component (long double)."""
    P = len(delta)
    M = damped(s.N, LD(lam))
    ad = np.abs(np.asarray(delta, dtype=LD))
    bM = np.array(s.bN, copy=True)
    for i in range(P):
        bM[i, i] *= 1 + LD(lam)
    u = LD(U53)
    L = cholesky_solve(M, s.g, want_L=True)[2]
    LL = np.abs(L) @ np.abs(L).T                       # >= |M| entry by entry
    return (LD(3 * P + 4) * u * (LL @ ad + np.abs(s.g))
            + u * np.abs(M) @ np.abs(np.asarray(theta_next, dtype=LD)) + bM @ ad + s.bg)


def emulate(Y, x, w, x_ref, theta0, free, lambda0, xtol, n_iter, live=None, poison=np.nan,
            mistake=None):
    """The device's arithmetic in float64 NumPy (np.exp, np.sum: other roundings, inside the
    bounds), vectorised over the pixels: `Y` [n, C], `theta0` [n, P] -> dict like the device's
    outputs (theta [n, P], chi2, cov [n, T], nchan, niter, status, trace [n, n_iter, 3 + P]); a
    status-3 pixel keeps theta0 and `poison` / -1 elsewhere.  `paths` counts the pixel-iterations
    that took each path of the rule.  `mistake`: "s2" (2 s^2 written as s^2), "no_weight" (the
    weights dropped), "uncounted" (a channel of weight 0 enters N and g with weight 1)."""
    f = np.float64
    Y = np.atleast_2d(np.asarray(Y, dtype=f))
    n, Cn = Y.shape
    th0 = np.broadcast_to(np.asarray(theta0, dtype=f), (n, np.shape(theta0)[-1])).copy()
    P = th0.shape[1]
    T = P * (P + 1) // 2
    fr = np.ones(P, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    wv = np.ones(Cn) if w is None else np.asarray(w, dtype=f)
    ok = np.isfinite(Y) & (wv > 0)[None, :]
    W = np.where(ok, (np.ones(Cn) if mistake == "no_weight" else wv)[None, :], 0.0)
    WN = np.where(np.isfinite(Y), np.where(wv > 0, wv, 1.0)[None, :], 0.0) if mistake == "uncounted" else W
    Y0 = np.where(np.isfinite(Y), Y, 0.0)
    cnt = ok.sum(axis=1)
    lv = np.ones(n, dtype=bool) if live is None else np.asarray(live).reshape(-1) != 0
    status = np.full(n, -1)
    status[~(lv & np.all(np.isfinite(th0), axis=1) & feasible(th0))] = 3
    cur, th_t = th0.copy(), th0.copy()
    chi_cur = np.full(n, np.inf)
    lam, lam_used = np.full(n, f(lambda0)), np.full(n, f(lambda0))
    N, g = np.zeros((n, P, P)), np.zeros((n, P))
    niter = np.zeros(n, dtype=int)
    trace = np.full((n, n_iter, 3 + P), poison, dtype=f)
    paths = dict(accept=0, reject=0, pivot=0, stalled=0, converged=0, exhausted=0, degenerate=0)
    TRI = tri_list(P)
    for it in range(1, n_iter + 1):
        a = np.nonzero(status == -1)[0]
        if a.size == 0:
            break
        m, J, _, _ = model(th_t[a], x, x_ref, f, two_s2=mistake != "s2")
        with np.errstate(all="ignore"):
            r = Y0[a] - m
            chi_t = np.sum(W[a] * r * r, axis=1)
            wJ = J * WN[a][:, None, :]
            Nt = np.einsum("ric,rjc->rij", wJ, J)
            gt = np.einsum("ric,rc->ri", wJ, r)
        if it == 1:
            deg = (cnt[a] < fr.sum()) | ~np.isfinite(chi_t)
            status[a[deg]] = 3
            keep = ~deg
            a, chi_t, Nt, gt = a[keep], chi_t[keep], Nt[keep], gt[keep]
        niter[a] = it
        acc = feasible(th_t[a]) & np.isfinite(chi_t) & (chi_t < chi_cur[a])
        trace[a, it - 1, 0], trace[a, it - 1, 1], trace[a, it - 1, 2] = chi_t, lam_used[a], acc
        trace[a, it - 1, 3:] = th_t[a]
        paths["accept"] += int(acc.sum())
        paths["reject"] += int((~acc).sum())
        for i in range(P):
            if not fr[i]:
                Nt[:, i, :] = Nt[:, :, i] = 0
                Nt[:, i, i] = 1
                gt[:, i] = 0
        ia = a[acc]
        cur[ia], chi_cur[ia], N[ia], g[ia] = th_t[ia], chi_t[acc], Nt[acc], gt[acc]
        if it > 1:
            lam[ia] = np.maximum(lam[ia] / f(10.0), f(LAM_MIN))
        lam[a[~acc]] = lam[a[~acc]] * f(10.0)
        zero = chi_cur[a] == 0.0
        status[a[zero]] = 1
        paths["converged"] += int(zero.sum())
        need = a[~zero]
        delta = np.zeros((n, P))
        while need.size:
            st = lam[need] > LAM_MAX
            status[need[st]] = 2
            paths["stalled"] += int(st.sum())
            need = need[~st]
            if not need.size:
                break
            d, good = cholesky_solve(damped(N[need], lam[need]), g[need])
            delta[need[good]] = d[good]
            paths["pivot"] += int((~good).sum())
            lam[need[~good]] = lam[need[~good]] * f(10.0)
            need = need[~good]
        b = a[status[a] == -1]
        if not b.size:
            continue
        with np.errstate(all="ignore"):
            sc = np.stack([scales(t).astype(f) for t in cur[b]])
            worst = np.max(np.abs(delta[b]) / sc, axis=1)
        conv = ~np.any(np.isnan(delta[b]), axis=1) & (worst <= xtol)
        status[b[conv]] = 1
        paths["converged"] += int(conv.sum())
        rest = b[~conv]
        if it == n_iter:
            status[rest] = 0
            paths["exhausted"] += int(rest.size)
        else:
            th_t[rest] = cur[rest] + delta[rest]
            lam_used[rest] = lam[rest]
    d3 = status == 3
    paths["degenerate"] = int(d3.sum())
    cov = np.stack([[N[p][i, j] for i, j in TRI] for p in range(n)]) if n else np.zeros((0, T))
    cur[d3], cov[d3] = th0[d3], poison
    chi_cur = np.where(d3, poison, chi_cur)
    trace[d3] = poison
    return dict(theta=cur, chi2=chi_cur, cov=cov, nchan=np.where(d3, -1, cnt),
                niter=np.where(d3, -1, niter), status=status, trace=trace, paths=paths)


def follow(y, x, w, x_ref, theta0, free, lambda0, xtol, n_iter, out, poison, sums=None):
    """Checks (a)-(e) of the module docstring on ONE pixel whose status is not 3: `y` [C] its
    spectrum as the device read it, `out` the device's (theta [P], chi2, cov [T], nchan, niter,
    status, trace [n_iter, 3 + P]) -> the worst error / bound.  `sums`: the `Sums` of this pixel's
    trace rows 0 .. niter - 1 (made here when None; `follow_all` makes them for all pixels at
    once)."""
    theta0 = np.asarray(theta0, dtype=np.float64)
    P = theta0.size
    fr = np.ones(P, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    trace, niter, status = np.asarray(out["trace"]), int(out["niter"]), int(out["status"])
    wv = np.ones(len(y)) if w is None else np.asarray(w, dtype=np.float64)
    count = int(np.sum(np.isfinite(y) & (wv > 0)))
    assert count >= fr.sum() and int(out["nchan"]) == count, ("d_nchan", out["nchan"], count)
    assert 1 <= niter <= n_iter and status in (0, 1, 2), (niter, status)
    assert np.all(trace[niter:] == poison), "a trace row beyond d_niter was written"
    assert np.array_equal(trace[0, 3:], theta0), "row 0 is the start"
    if sums is None:
        sums = Sums(trace[:niter, 3:], np.broadcast_to(y, (niter, len(y))), x, w, x_ref, fr)
    worst = 0.0
    lam = np.float64(lambda0)
    cur = s_cur = None
    chi_cur_dev = np.inf
    for t in range(niter):
        chi_t, lam_used, acc = trace[t, 0], trace[t, 1], trace[t, 2]
        th_t = trace[t, 3:]
        assert acc in (0.0, 1.0)
        assert np.array_equal(th_t[~fr], theta0[~fr]), "a fixed parameter moved"
        if t == 0:
            assert lam_used == lam, "row 0 uses lambda0"
        finite = bool(np.all(np.isfinite(th_t)))
        good = finite and bool(feasible(th_t))
        s_t = sums.row(t) if finite else None
        # (a)
        if s_t is not None and np.isfinite(float(s_t.chi2)) and np.isfinite(float(s_t.bchi)):
            err, bnd = abs(LD(chi_t) - s_t.chi2), s_t.bchi
            ratio = float(err / bnd) if bnd > 0 else (0.0 if err == 0 else np.inf)
            assert ratio <= 1.0, ("chi^2 of trial %d" % t, float(err), float(bnd))
            worst = max(worst, ratio)
            _part("chi2", ratio)
        # (b)
        if not good or not np.isfinite(chi_t):
            assert acc == 0.0, "an infeasible / non-finite trial was accepted"
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
        if last:
            # (the device's own breakdowns are not on record: a lambda whose pivots are all clear
            # cannot have broken down)
            while lam <= LAM_MAX and status == 2 and not pivots_clear(damped(s_cur.N, LD(lam))):
                lam = lam * np.float64(10.0)
            assert (status == 2) == bool(lam > LAM_MAX), ("status 2 iff lambda > 1e12", status, lam)
            if status == 2:
                break
        else:
            j = 0
            while lam != trace[t + 1, 1]:
                assert j < 25 and lam < trace[t + 1, 1] and \
                    not pivots_clear(damped(s_cur.N, LD(lam))), \
                    ("lambda of row %d" % (t + 1), trace[t + 1, 1], lam)
                lam, j = lam * np.float64(10.0), j + 1
            assert lam <= LAM_MAX
        M = damped(s_cur.N, LD(lam))
        d_ref, ok = cholesky_solve(M, s_cur.g)
        if last and not ok:
            break                                     # (a breakdown in the last trial: no step to judge)
        assert ok, "the reference's factorisation broke down where the device's went through"
        sc = scales(cur)
        with np.errstate(all="ignore"):
            w_ref = float(np.max(np.abs(d_ref) / sc))
            slack = float(np.max((np.abs(np.linalg.inv(M.astype(np.float64))).astype(LD)
                                  @ step_bound(s_cur, lam, d_ref, cur + d_ref)) / sc))
        if not np.isfinite(slack):
            slack = np.inf        # (M has no float64 inverse: the stop of this trial is not judged)
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
        assert np.array_equal(th_n[~fr], cur[~fr]), "a fixed parameter moved"
        delta = th_n.astype(LD) - cur.astype(LD)
        resid = np.abs(M @ delta - s_cur.g)[fr]
        bnd = step_bound(s_cur, lam, delta, th_n)[fr]
        ratio = float(np.max(resid / bnd))
        assert ratio <= 1.0, ("step %d" % t, ratio)
        worst = max(worst, ratio)
        _part("step", ratio)
    # (e)
    assert cur is not None
    assert np.array_equal(np.asarray(out["theta"]), cur), "d_theta is the last accepted trial"
    assert out["chi2"] == chi_cur_dev, "d_chi2 is the last accepted chi^2"
    cov = unpack(np.asarray(out["cov"]).astype(LD), P)
    err = np.abs(cov - s_cur.N)
    exact = s_cur.bN == 0
    assert np.all(err[exact] == 0), "d_cov: the identity's entries of a fixed parameter"
    ratio = float(np.max(err[~exact] / s_cur.bN[~exact])) if np.any(~exact) else 0.0
    assert ratio <= 1.0, ("d_cov", ratio)
    _part("cov", ratio)
    return max(worst, ratio)


def follow_all(Y, x, w, x_ref, theta0, free, lambda0, xtol, n_iter, out, poison, p_float, p_int,
               live=None):
    """`follow` on every pixel of a stack (`Y` [n, C], `theta0` [n, P], `out` the device's arrays
    with the pixel axis first), the sums of all trace rows made in one vectorised pass; a status-3
    pixel must have nothing but its status written (`p_float`, `p_int`, `poison`: what the float
    outputs, the int outputs and the trace held before the call) and must BE degenerate -> the
    worst error / bound."""
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    n = Y.shape[0]
    th0 = np.broadcast_to(np.asarray(theta0, dtype=np.float64), (n, np.shape(theta0)[-1]))
    P = th0.shape[1]
    fr = np.ones(P, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    wv = np.ones(Y.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
    lv = np.ones(n, dtype=bool) if live is None else np.asarray(live).reshape(-1) != 0
    st = np.asarray(out["status"])
    run = np.nonzero(st != 3)[0]
    nit = np.asarray(out["niter"])
    rows = [(p, t) for p in run for t in range(int(nit[p]))]
    worst = 0.0
    if rows:
        pi, ti = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
        TH = np.asarray(out["trace"])[pi, ti, 3:]
        TH = np.where(np.isfinite(TH), TH, 1.0)        # (rows that are not finite are not judged)
        S = Sums(TH, Y[pi], x, w, x_ref, fr)
        first = {}
        for k, (p, t) in enumerate(rows):
            first.setdefault(p, k)
    for p in range(n):
        if st[p] == 3:
            cnt = int(np.sum(np.isfinite(Y[p]) & (wv > 0)))
            deg = (not lv[p]) or not np.all(np.isfinite(th0[p])) or not feasible(th0[p]) or cnt < fr.sum()
            if not deg:
                chi0 = Sums(th0[p], Y[p], x, w, x_ref, fr).chi2[0]
                deg = not np.isfinite(float(chi0)) or float(chi0) > 1e300
            assert deg, ("pixel %d ended degenerate without a reason" % p)
            assert np.array_equal(out["theta"][p], th0[p], equal_nan=True), "status 3 wrote theta"
            assert out["chi2"][p] == p_float and np.all(out["cov"][p] == p_float), "status 3 wrote"
            assert out["nchan"][p] == p_int and out["niter"][p] == p_int, "status 3 wrote"
            assert np.all(out["trace"][p] == poison), "status 3 wrote the trace"
            continue
        k0 = first[p]
        sub = object.__new__(Sums)
        sl = slice(k0, k0 + int(nit[p]))
        sub.chi2, sub.bchi, sub.N, sub.bN, sub.g, sub.bg = (S.chi2[sl], S.bchi[sl], S.N[sl],
                                                            S.bN[sl], S.g[sl], S.bg[sl])
        one = {k: out[k][p] for k in ("theta", "chi2", "cov", "nchan", "niter", "status", "trace")}
        worst = max(worst, follow(Y[p], x, w, x_ref, th0[p], fr, lambda0, xtol, n_iter, one, poison, sub))
    return worst
