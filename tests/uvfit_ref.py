"""A long-double NumPy reference for rjp_uvfit (K20, uvfit.hip) that FOLLOWS the device's trace, as
tests/gaussfit_ref.py follows K14's: two correct Levenberg-Marquardt codes may part ways on a
near-tie of chi^2, so the reference never runs a fit of its own.  It takes the data as the device
read them -- V [K] complex, a = su u and b = sv v as the float64 products the device forms, the
weights -- and the trace rows (chi^2_t, lambda used, accepted, theta_t[P]) and checks, for every
iteration t (u = 2^-53, P = 6 n_comp):

(a) chi^2_t against its own long-double sum over the counting visibilities.  Per visibility and
    component, as the header comment of uvfit.hip forms them:
      * the phase ph = fma(a, x, b z): the product b z and the fma round once each, so ph is within
        u (|b z| + |ph|) <= 2 u (|a x| + |b z|) =: e_ph turns of a x + b z;
      * sincos_2pi: truncation < 2e-14 / 1e-15 (rjp_device.h) and the roundings of its reduction
        and Horner forms (< 8 u), taken as 2.1e-14 absolute on both; with the phase error, sine and
        cosine are within e_sc = 2.1e-14 + 2 pi e_ph;
      * the exponent q = fma(sxx, a a, fma(2 sxz, a b, szz (b b))): at most four roundings on any
        term, taken as 5 u Qabs, Qabs = |sxx| a^2 + 2 |sxz a b| + |szz| b^2; e = q c with c the
        float64 of -2 pi^2 (u) and one rounding: e within e_e = 7 u 2 pi^2 Qabs;
      * exp_any: 1e-14 relative (rjp_device.h): E within r_E = 1e-14 + e_e relative;
      * A = F E and A cs / A sn: one rounding each.  So each part of the component is within
        e_c = |F| E (r_E + 2 u + e_sc)   (+ 1e-300 |F| for an exponent that straddles -700);
      * the components are added in order (n_comp roundings of at most sum |F| E each), and
        r = V - M rounds once: each part of r is within e_r = sum e_c + n_comp u sum |F| E + u |r|;
      * a part adds fma(w r, r, .): w (2 |r| e_r + e_r^2 + 2 u r^2);
      * the accumulation: a fixed tree of depth D = 8 (a thread's four visibilities, two fmas
        each) + 32 + 8 (the block sum) + ceil(tiles / 256) + 32 + 8 (the tiles' partials):
        D u chi^2.
    bound = 1.01 (sum of the per-part terms + D u chi^2), the 1.01 for the second-order terms.
(b) the accept flag: a trial that is not positive semi-definite in every component, or whose chi^2
    is not finite, is rejected; a trial identical in all parameters to theta_cur is rejected (the
    same sum in the same order gives the same bits, and the rule is a strict <); else the flag must
    agree with the reference's two chi^2 wherever they differ by more than the sum of their bounds.
(c) the proposed step delta = theta_{t+1} - theta_cur: a FIXED parameter's is exactly 0; the free
    ones are judged by their componentwise backward error against the reference's N = Re(J^H W J)
    and g = Re(J^H W r) at theta_cur (identity rows for fixed parameters), M = N + lambda diag N:
      |M delta - g|_i <= c u (sum_j |M_ij| |delta_j| + |g_i|)                 (Cholesky)
                         + u sum_j |M_ij| |theta_{t+1, j}|                    (recovering delta)
                         + sum_j bN_ij (1 + lambda [i = j]) |delta_j| + bg_i    (summation of N, g)
    c = 3 P + 1 + 3 (22, 40): gamma_{3n+1} of a Cholesky solve (Higham, Accuracy and Stability,
    Thm 10.4) plus forming M_ii = fma(lambda, N_ii, N_ii) and the rounding of g.  bN, bg are built
    like (a): a Jacobian column is a part of the component (dF: of E (cos, -sin), within
    E (r_E + u + e_sc)) times a real factor of at most three roundings and a rounded constant
    (2 pi a; -2 pi^2 a^2, -4 pi^2 a b, -2 pi^2 b^2), one more for the product: within
    e_J = |f| (e_c + 5 u |F| E) of itself, |J| <= |f| |F| E =: Jabs.  A sum adds two fmas per
    visibility (real and imaginary parts) with the weighted factor rounded first:
      bN_ij = 1.01 sum 2 w (Jabs_i e_Jj + e_Ji Jabs_j + e_Ji e_Jj + (2 + D) u Jabs_i Jabs_j)
      bg_i  = 1.01 sum 2 w (Jabs_i e_r + e_Ji |r| + e_Ji e_r + (2 + D) u Jabs_i |r|),  |r| the modulus.
(d) lambda, the stop and the status: K14's rules (tests/gaussfit_ref.py (d)) with the step scale
    s = (max(|F|, 1e-300), 1, 1, t, t, t), t = max(sxx + szz, 1) per component.
(e) at the end d_theta and d_chi2 are the bits of the last accepted trace row, d_cov is within its
    bound of the reference at d_theta (the identity's entries exactly), d_nvis is the count,
    d_niter the rows written, and the trace beyond d_niter holds the caller's poison.
`follow` returns the worst error / bound it saw; anything else fails an assertion."""
import numpy as np

from tests.lm_ref import (LAM_MAX, LAM_MIN, LD, U53, cholesky_solve, damped, pack, pivots_clear,
                          tri_list, unpack)

TILE, REDUCE_PASS = 1024, 256
EXP_RTOL, SINCOS_ATOL = 1e-14, 2.1e-14
MAX_COMP = 2
PI_LD = LD("3.14159265358979323846264338327950288")
TWO_PI2 = 2 * PI_LD * PI_LD
# the library's refusals, in the order check_uvfit makes them; the workspace comes last
MSG = {"nulls": "rjp_uvfit: NULL visibilities, scales, baselines, parameters or outputs",
       "sizes": "rjp_uvfit: n_maps and n_vis must be positive",
       "comp": "rjp_uvfit: n_comp must lie in 1 .. RJP_UVFIT_MAX_COMP (2)",
       "wmaps": "rjp_uvfit: w_maps must be 1 or n_maps",
       "scale": "rjp_uvfit: non-finite h_su / h_sv",
       "free": "rjp_uvfit: no free parameter",
       "tol": "rjp_uvfit: lambda0 and xtol must be finite and positive",
       "iter": "rjp_uvfit: n_iter < 1",
       "wgs": "rjp_uvfit: more than 2^31 - 1 workgroups",
       "short": "rjp_uvfit: workspace smaller than rjp_uvfit_workspace()"}
PARTS = {}                   # the worst error / bound of checks (a), (c) and d_cov seen by `follow`


def sizes(n_comp):
    """(P, T, Q, S): parameters, packed entries of N, sums per tile, doubles of state per map."""
    P = 6 * n_comp
    T = P * (P + 1) // 2
    return P, T, 1 + T + P + 1, (3 * P + 6 + T + 7) // 8 * 8


def tiling(n_maps, n_vis):
    tiles = (n_vis + TILE - 1) // TILE
    return {"tiles": tiles, "workgroups": tiles * n_maps}


def workspace_bytes(n_maps, n_vis, n_comp):
    _, _, Q, S = sizes(n_comp)
    return (tiling(n_maps, n_vis)["workgroups"] * Q + n_maps * S) * 2 * 8


def depth(n_vis):
    tiles = tiling(1, n_vis)["tiles"]
    return 8 + 32 + 8 + (tiles + REDUCE_PASS - 1) // REDUCE_PASS + 32 + 8


def psd(th):
    th = np.asarray(th)
    return all(bool(th[6 * c + 3] >= 0 and th[6 * c + 5] >= 0 and
                    th[6 * c + 3] * th[6 * c + 5] >= th[6 * c + 4] * th[6 * c + 4])
               for c in range(th.size // 6))


def counting(V, a, b, w, u=None, v=None):
    """(V, a, b, w) of the visibilities that count: Re V, Im V, u, v and w finite, w > 0.  `a`,
    `b`: the float64 products su u, sv v; `u`, `v`: the raw baselines (None: judged by a, b, which
    are finite with them for finite scales short of overflow)."""
    V = np.asarray(V, dtype=np.complex128)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    w = np.ones(V.size) if w is None else np.asarray(w, dtype=np.float64)
    ok = np.isfinite(V.real) & np.isfinite(V.imag) & np.isfinite(w) & (w > 0)
    ok &= np.isfinite(a if u is None else np.asarray(u)) & np.isfinite(b if v is None else np.asarray(v))
    return V[ok], a[ok], b[ok], w[ok]


def _pi(dtype):
    return PI_LD if dtype is LD else dtype(np.pi)


def model(theta, a, b, dtype=LD, with_jac=True, phase_sign=-1, env=2, xz_factor=2):
    """(M [2, n], J [P, 2, n], E [nc, n]) at the points (a, b), parts (re, im), in `dtype`; an
    exact 0 of the envelope below an exponent of -700.  (`phase_sign`, `env`, `xz_factor`: the
    planted mistakes of tests/test_uvfit_reference_cpu.py -- the sign of the phase, the constant
    env pi^2 of the envelope, the factor on the sxz derivative.)"""
    th = np.asarray(theta)
    nc = th.size // 6
    a, b = np.asarray(a).astype(dtype), np.asarray(b).astype(dtype)
    pi = _pi(dtype)
    M = np.zeros((2, a.size), dtype=dtype)
    J = np.zeros((6 * nc, 2, a.size), dtype=dtype) if with_jac else None
    Es = np.zeros((nc, a.size), dtype=dtype)
    with np.errstate(all="ignore"):
        for c in range(nc):
            F, x, z, sxx, sxz, szz = (dtype(t) for t in th[6 * c:6 * c + 6])
            ph = a * x + b * z
            ph = ph - np.rint(ph)                    # (sine and cosine of 2 pi ph: period 1)
            cs, sn = np.cos(2 * pi * ph), np.sin(2 * pi * ph)
            e = -(dtype(env) * pi * pi) * (sxx * a * a + 2 * sxz * a * b + szz * b * b)
            E = np.where(e < -700, dtype(0), np.exp(np.clip(e, dtype(-745), dtype(709))))
            E = np.where(np.isnan(e), dtype(np.nan), E)
            E = np.where(e > 709, dtype(np.inf), E)
            Es[c] = E
            s = dtype(-phase_sign)                   # (the model's phasor is cos - i sin)
            cr, ci = F * E * cs, -s * F * E * sn
            M[0] += cr
            M[1] += ci
            if not with_jac:
                continue
            ka, kb = 2 * pi * a, 2 * pi * b
            J[6 * c] = [E * cs, -s * E * sn]
            J[6 * c + 1] = [s * ci * ka, -s * cr * ka]
            J[6 * c + 2] = [s * ci * kb, -s * cr * kb]
            for k, f in ((3, -2 * pi * pi * a * a), (4, -dtype(xz_factor) * 2 * pi * pi * a * b),
                         (5, -2 * pi * pi * b * b)):
                J[6 * c + k] = [cr * f, ci * f]
    return M, J, Es


class Sums:
    """chi^2, N [T], g [P] of `theta` over the counting visibilities in long double, with the
    bounds of the module docstring (bchi, bN [T], bg [P]) for a set of `n_vis` visibilities.
    `free` [P] bool: the identity's rows and zeros for the fixed parameters, with bounds 0."""

    def __init__(self, theta, data, n_vis, free=None, want_jac=True):
        V, a, b, w = data
        th = np.array([LD(t) for t in theta], dtype=LD)
        P = th.size
        nc = P // 6
        fr = np.ones(P, dtype=bool) if free is None else np.asarray(free, dtype=bool)
        M, J, Es = model(th, a, b, LD, with_jac=want_jac)
        al, bl, wl = a.astype(LD), b.astype(LD), w.astype(LD)
        u = LD(U53)
        D = depth(n_vis) * u
        r = np.stack([V.real.astype(LD) - M[0], V.imag.astype(LD) - M[1]])
        FE = np.zeros((nc, a.size), dtype=LD)          # |F| E, the modulus of a component
        ec = np.zeros((nc, a.size), dtype=LD)          # the bound of each of its parts
        eb = np.zeros((nc, a.size), dtype=LD)          # the bound of a part of E (cos, -sin)
        for c in range(nc):
            F, x, z, sxx, sxz, szz = th[6 * c:6 * c + 6]
            e_ph = 2 * u * (np.abs(al * x) + np.abs(bl * z))
            e_sc = LD(SINCOS_ATOL) + 2 * PI_LD * e_ph
            Qabs = np.abs(sxx) * al * al + 2 * np.abs(sxz * al * bl) + np.abs(szz) * bl * bl
            r_E = LD(EXP_RTOL) + 7 * u * TWO_PI2 * Qabs
            FE[c] = np.abs(F) * Es[c]
            ec[c] = FE[c] * (r_E + 2 * u + e_sc) + LD(1e-300) * np.abs(F)
            eb[c] = Es[c] * (r_E + u + e_sc) + LD(1e-300)
        er = ec.sum(axis=0)[None, :] + nc * u * FE.sum(axis=0)[None, :] + u * np.abs(r)
        self.n = int(V.size)
        self.chi2 = LD(np.sum(wl * (r[0] * r[0] + r[1] * r[1])))
        self.bchi = LD(1.01) * (np.sum(wl[None, :] * (2 * np.abs(r) * er + er * er + 2 * u * r * r))
                                + D * self.chi2)
        if not want_jac:
            return
        pi = PI_LD
        Jabs = np.zeros((P, a.size), dtype=LD)
        eJ = np.zeros((P, a.size), dtype=LD)
        for c in range(nc):
            f = [None, 2 * pi * np.abs(al), 2 * pi * np.abs(bl), TWO_PI2 * al * al,
                 2 * TWO_PI2 * np.abs(al * bl), TWO_PI2 * bl * bl]
            Jabs[6 * c], eJ[6 * c] = Es[c], eb[c]
            for k in range(1, 6):
                Jabs[6 * c + k] = f[k] * FE[c]
                eJ[6 * c + k] = f[k] * (ec[c] + 5 * u * FE[c]) + LD(1e-300)
        rabs = np.sqrt(r[0] * r[0] + r[1] * r[1])
        ermax = np.max(er, axis=0)
        wJ = J * wl[None, None, :]
        N = np.einsum("ipk,jpk->ij", wJ, J)
        g = np.einsum("ipk,pk->i", wJ, r)
        wJa, weJ = Jabs * wl[None, :], eJ * wl[None, :]
        cross = wJa @ eJ.T
        bN = LD(1.01) * 2 * (cross + cross.T + weJ @ eJ.T + (2 * u + D) * (wJa @ Jabs.T))
        bg = LD(1.01) * 2 * (wJa @ ermax + weJ @ rabs + weJ @ ermax + (2 * u + D) * (wJa @ rabs))
        for i in range(P):
            if not fr[i]:
                N[i, :] = N[:, i] = 0
                bN[i, :] = bN[:, i] = 0
                N[i, i] = 1
                g[i] = bg[i] = 0
        self.N, self.bN, self.g, self.bg = pack(N), pack(bN), g, bg


def scales(th):
    out = []
    for c in range(len(th) // 6):
        t = max(th[6 * c + 3] + th[6 * c + 5], 1.0)
        out += [max(abs(th[6 * c]), 1e-300), 1.0, 1.0, t, t, t]
    return np.array(out, dtype=LD)


def step_bound(s, lam, delta, theta_next):
    """The bound of (c) on |M delta - g|, per component (long double)."""
    P = len(delta)
    M = damped(unpack(s.N, P), LD(lam))
    ad = np.abs(np.asarray(delta, dtype=LD))
    bM = unpack(s.bN, P)
    for i in range(P):
        bM[i, i] *= 1 + LD(lam)
    u = LD(U53)
    return (LD(3 * P + 4) * u * (np.abs(M) @ ad + np.abs(s.g))
            + u * np.abs(M) @ np.abs(np.asarray(theta_next, dtype=LD)) + bM @ ad + s.bg)


def emulate(data, n_vis, theta0, free, lambda0, xtol, n_iter, poison=None, mistake=None):
    """The device's arithmetic in float64 NumPy (np.exp, np.sum: other roundings, inside the
    bounds) on the counting visibilities `data` = (V, a, b, w) -> dict like the device's outputs
    (theta, chi2, cov, nvis, niter, status, trace), or status 3 with theta None.  `mistake`: one of
    "phase_sign", "env_4pi2", "xz_factor" (no factor 2 on the sxz derivative), "no_weight" (the
    weights dropped), "lam_identity" (lambda I for lambda diag N), "accept_le" (accept on <=),
    "fixed_moves" (a fixed parameter keeps its row of N and g)."""
    f = np.float64
    V, a, b, w = data
    th_t = np.array(theta0, dtype=f)
    P = th_t.size
    fr = np.ones(P, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    TRI = tri_list(P)
    trace = np.full((n_iter, 3 + P), np.nan if poison is None else poison)
    out = dict(theta=None, chi2=None, cov=None, nvis=None, niter=None, status=3, trace=trace)
    if not (np.all(np.isfinite(th_t)) and psd(th_t)):
        return out
    ww = np.ones_like(w) if mistake == "no_weight" else w
    kw = dict(phase_sign=1 if mistake == "phase_sign" else -1, env=4 if mistake == "env_4pi2" else 2,
              xz_factor=1 if mistake == "xz_factor" else 2)
    cur, chi_cur, lam, lam_used, N, g = th_t.copy(), np.inf, f(lambda0), f(lambda0), None, None
    status, it = None, 0
    while status is None:
        it += 1
        M, J, _ = model(th_t, a, b, f, **kw)
        r = np.stack([V.real - M[0], V.imag - M[1]])
        with np.errstate(all="ignore"):
            chi_t = f(np.sum(ww * (r[0] * r[0] + r[1] * r[1])))
        if it == 1 and (2 * V.size < fr.sum() or not np.isfinite(chi_t)):
            return out
        better = chi_t <= chi_cur if mistake == "accept_le" else chi_t < chi_cur
        acc = bool(psd(th_t) and np.isfinite(chi_t) and better)
        trace[it - 1] = [chi_t, lam_used, float(acc)] + list(th_t)
        if acc:
            cur, chi_cur = th_t.copy(), chi_t
            with np.errstate(all="ignore"):
                wJ = J * ww[None, None, :]
                Nf = np.einsum("ipk,jpk->ij", wJ, J)
                g = np.einsum("ipk,pk->i", wJ, r)
            if mistake != "fixed_moves":
                for i in range(P):
                    if not fr[i]:
                        Nf[i, :] = Nf[:, i] = 0
                        Nf[i, i] = 1
                        g[i] = 0
            N = np.array([Nf[i, j] for i, j in TRI])
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
            delta, ok = cholesky_solve(damped(unpack(N, P), lam, identity=mistake == "lam_identity"), g)
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
    out.update(theta=cur, chi2=chi_cur, cov=N, nvis=int(V.size), niter=it, status=status)
    return out


def follow(data, n_vis, theta0, free, lambda0, xtol, n_iter, out, poison):
    """Checks (a)-(e) of the module docstring on one map: `data` = (V, a, b, w) of the counting
    visibilities as the device read them (`counting`), `n_vis` the size of the whole set, `out` the
    device's (theta, chi2, cov, nvis, niter, status, trace [n_iter, 3 + P]) of a map whose status is
    not 3 -> the worst error / bound.  `poison`: what the trace held before the call."""
    theta0 = np.asarray(theta0, dtype=np.float64)
    P = theta0.size
    fr = np.ones(P, dtype=bool) if free is None else np.asarray(free, dtype=bool)
    trace, niter, status = np.asarray(out["trace"]), int(out["niter"]), int(out["status"])
    assert 2 * data[0].size >= fr.sum() and int(out["nvis"]) == data[0].size, "d_nvis"
    assert 1 <= niter <= n_iter and status in (0, 1, 2), (niter, status)
    assert np.all(trace[niter:] == poison), "a trace row beyond d_niter was written"
    assert np.array_equal(trace[0, 3:], theta0), "row 0 is the start"
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
        good = finite and psd(th_t)
        s_t = Sums(th_t, data, n_vis, fr, want_jac=good) if finite else None
        # (a)
        if s_t is not None and np.isfinite(float(s_t.chi2)) and np.isfinite(float(s_t.bchi)):
            err, bnd = abs(LD(chi_t) - s_t.chi2), s_t.bchi
            ratio = float(err / bnd) if bnd > 0 else (0.0 if err == 0 else np.inf)
            assert ratio <= 1.0, ("chi^2 of trial %d" % t, float(err), float(bnd))
            worst = max(worst, ratio)
            PARTS["chi2"] = max(PARTS.get("chi2", 0.0), ratio)
        # (b)
        if not good or not np.isfinite(chi_t):
            assert acc == 0.0, "a trial that is not positive semi-definite / finite was accepted"
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
            while lam <= LAM_MAX and status == 2 and not pivots_clear(damped(unpack(s_cur.N, P), LD(lam))):
                lam = lam * np.float64(10.0)
            assert (status == 2) == bool(lam > LAM_MAX), ("status 2 iff lambda > 1e12", status, lam)
            if status == 2:
                break
        else:
            j = 0
            while lam != trace[t + 1, 1]:
                assert j < 25 and lam < trace[t + 1, 1] and \
                    not pivots_clear(damped(unpack(s_cur.N, P), LD(lam))), \
                    ("lambda of row %d" % (t + 1), trace[t + 1, 1], lam)
                lam, j = lam * np.float64(10.0), j + 1
            assert lam <= LAM_MAX
        M = damped(unpack(s_cur.N, P), LD(lam))
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
        assert np.array_equal(th_n[~fr], cur[~fr]), "a fixed parameter moved"
        delta = th_n.astype(LD) - cur.astype(LD)
        resid = np.abs(M @ delta - s_cur.g)[fr]
        bnd = step_bound(s_cur, lam, delta, th_n)[fr]
        ratio = float(np.max(resid / bnd))
        assert ratio <= 1.0, ("step %d" % t, ratio)
        worst = max(worst, ratio)
        PARTS["step"] = max(PARTS.get("step", 0.0), ratio)
    # (e)
    assert cur is not None
    assert np.array_equal(np.asarray(out["theta"]), cur), "d_theta is the last accepted trial"
    assert out["chi2"] == chi_cur_dev, "d_chi2 is the last accepted chi^2"
    cov = np.asarray(out["cov"]).astype(LD)
    err = np.abs(cov - s_cur.N)
    exact = s_cur.bN == 0
    assert np.all(err[exact] == 0), "d_cov: the identity's entries of a fixed parameter"
    ratio = float(np.max(err[~exact] / s_cur.bN[~exact])) if np.any(~exact) else 0.0
    assert ratio <= 1.0, ("d_cov", ratio)
    PARTS["cov"] = max(PARTS.get("cov", 0.0), ratio)
    return max(worst, ratio)
