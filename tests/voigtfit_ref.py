"""The reference of K24 (rjp_voigtfit, include/rjprt.h): what the CPU test pins and the GPU test
holds the device to.  Four parts.

1. `w_dev`: the float64 restatement of rajepy_amd/csrc/voigt_w.h, operation for operation (NumPy
   has no fma: the device's contractions are what the factor 2 of kVoigtWEps covers), with the
   device's own exp_any and sincos_2pi restated; `w_exact`: mpmath, exp(-z^2) erfc(-i z).
2. `emulate`: a float64 emulation of the kernel for one pixel, on `w_dev`, with the header's
   products in the header's order.  `mistake=` plants one of the errors the CPU test shows to fall
   outside the bounds.
3. `follow`: follows a trace (the device's or the emulation's) trial by trial in long double with
   `w_exact`, and asserts

   chi^2 of every trial.  With eps = 2^-53 and, per channel and component,
       e_w  = EPS_W |w| + |w'| (4 |u| + 3 a) eps      (w through its own error, and through the
              roundings of rs, q, a (two each) and of d = x - x0, u = d q: |du| <= 4 eps |u|,
              |da| <= 3 eps a, and |dw| <= |w'| |dz| with w' = (Rw, Iw))
       dm_k = |c| (e_w + 4 eps |K|)                   (cn two roundings, c and c K one each)
       dm   = sum_k dm_k + (n_comp + 3) eps (sum_k |c K| + |b0| + |b1 xr|)
   the residual r = y - m carries dr = dm + eps |r|, a term w r^2 carries w (2 |r| dr + dr^2) + 2 eps
   w r^2, and the chain of n terms n eps sum w r^2:
       B_chi = sum_c w (2 |r| dr + dr^2) + (n + 2) eps sum_c w r^2 + n TINY
   (TINY = 2^-1070: a product that underflows is off by up to 2^-1075 absolutely, not relatively;
   the same n TINY is added to every dN_ij and dg_i).
   |chi2_dev - chi2_ref| <= B_chi.

   the accept flag.  Exactly what the rule gives on the device's OWN numbers (feasible, finite,
   chi_t < chi_cur of the trace); and, where the reference's two chi^2 differ by more than the sum
   of their two bounds, the reference's order.  The others are counted as unjudged.

   every proposed step delta = theta_t(next) - theta_cur by its componentwise backward error
   (Oettli-Prager) against the reference's A = N + lambda diag N and g at theta_cur:
       |A delta - g|_i <= sum_j dA_ij |delta_j| + dg_i + sum_j |A_ij| eps |theta_t,j|,
       dA_ij = (1 + lambda) dN_ij + (3 P + 2) eps sqrt(A_ii A_jj)
   (the Cholesky solve: Higham's gamma_{3P+1} |L| |L^T|, and (|L| |L^T|)_ij <= sqrt(A_ii A_jj) by
   Cauchy-Schwarz; the last term is the rounding of theta_cur + delta).  dN and dg carry e_w through
   the Jacobian formulas AS WRITTEN, in absolute terms -- Rw = -2 (u K - a L) cancels in the far
   wing, so its error is bounded by the sizes of its two products, not by its own size:
       dK = dL = e_w
       dRw = 2 (|u| dK + a dL) + 8 eps (|u K| + |a L|)
       dIw = 2 (|u| dL + a dK) + 8 eps (|u L| + |a K| + 1 / sqrt(pi))
       dJ_F = cn (dK + 3 eps |K|);  dJ_x0 = |c q| (dRw + 6 eps |Rw|);  dJ_g = |c q| (dIw + 6 eps |Iw|)
       dJ_s = |c rs| (dK + |u| dRw + a dIw + 8 eps (|K| + |u Rw| + |a Iw|))
       dJ_b0 = 0;  dJ_b1 = eps |xr|
       dN_ij = sum_c w (|J_i| dJ_j + dJ_i |J_j| + dJ_i dJ_j) + (n + 2) eps sum_c w |J_i J_j|
       dg_i  = sum_c w (|J_i| dr + dJ_i |r| + dJ_i dr) + (n + 2) eps sum_c w |J_i r|
   A fixed parameter's step is exactly 0.

   the lambda sequence (exact: powers of ten by the rule, replayed in float64 with the breakdown
   loop on the reference's A where the pivots are clear), the stop, the status, the outputs
   (theta_cur, chi2, nchan, niter; cov within dN of the reference's N) and that trace rows at and
   beyond niter keep the caller's poison.
4. `first_order_shift`: |N^-1 J^T W| applied to a perturbation of the data, for the bound of the
   test that recovers the widths a model cell was given.
"""
import math

import mpmath as mp
import numpy as np

LD = np.longdouble
PI_LD = LD(3.141592653589793) + LD(1.2246467991473532e-16)      # pi to long double
EPS = 2.0 ** -53
TINY = 2.0 ** -1070               # gradual underflow: up to 16 roundings of 2^-1075 per sum, see B_chi
EPS_W = 2.0e-15                 # kVoigtWEps of voigt_w.h
SQRT_PI = math.sqrt(math.pi)
PATHS = ("far", "fraction", "lattice_int", "lattice_mid")

_EXP_C = (2.77658272960759129e-07, 2.76399272005369552e-06, 2.48011840775311536e-05,
          1.98411738635095533e-04, 1.38888891559099128e-03, 8.33333337887889360e-03,
          4.16666666661282964e-02, 1.66666666665949731e-01, 0.5, 1.0, 1.0)
_T2I = np.array([((n + 1) / 2.) ** 2 for n in range(14)])
_T2M = np.array([((n + 0.5) / 2.) ** 2 for n in range(14)])


def _node_weights(t2):
    return np.array([float(mp.exp(-mp.mpf(float(t)))) for t in t2])


_EI, _EM = _node_weights(_T2I), _node_weights(_T2M)


def exp_any(x):
    """rjp_device.h's exp_any: Cody-Waite reduction and the degree-10 polynomial."""
    x = np.asarray(x, dtype=np.float64)
    kd = np.rint(x * 1.4426950408889634074)
    r = x - kd * 6.93147180369123816490e-01
    r = r - kd * 1.90821492927058770002e-10
    p = np.full_like(r, _EXP_C[0])
    for c in _EXP_C[1:]:
        p = p * r + c
    return np.ldexp(p, kd.astype(np.int64))


def sincos_2pi(u):
    """rjp_device.h's sincos_2pi: (sin 2 pi u, cos 2 pi u)."""
    u = np.asarray(u, dtype=np.float64)
    k = np.rint(4.0 * u)
    w = 6.28318530717958647692 * (u - 0.25 * k)
    w2 = w * w
    ps = np.full_like(w, -7.6471637318198164759e-13)
    for c in (1.6059043836821614599e-10, -2.5052108385441718775e-08, 2.7557319223985890653e-06,
              -1.9841269841269841253e-04, 8.3333333333333332177e-03, -1.6666666666666665741e-01):
        ps = ps * w2 + c
    s0 = (ps * w2) * w + w
    pc = np.full_like(w, 4.7794773323873852974e-14)
    for c in (-1.1470745597729724714e-11, 2.0876756987868098979e-09, -2.7557319223985888276e-07,
              2.4801587301587301566e-05, -1.3888888888888889419e-03, 4.1666666666666664354e-02, -0.5):
        pc = pc * w2 + c
    c0 = pc * w2 + 1.0
    q = k.astype(np.int64) & 3
    a = np.where(q & 1, c0, s0)
    b = np.where(q & 1, s0, c0)
    return np.where(q & 2, -a, a), np.where((q == 1) | (q == 2), -b, b)


def w_dev(u, a, with_path=False):
    """voigt_w.h in float64 -> (K, L[, path index into PATHS]) for arrays u, a >= 0."""
    u, a = np.broadcast_arrays(np.asarray(u, dtype=np.float64), np.asarray(a, dtype=np.float64))
    u, a = u.copy(), a.copy()
    isp = 0.56418958354775628695
    with np.errstate(all="ignore"):
        d = u * u + a * a
        lat = (d < 49.0) & (a < 6.0)
        far = ~lat & ~(d < 1e200)
        # far
        s = 1.0 / np.fmax(np.abs(u), a)
        us, as_ = u * s, a * s
        inv = (isp * s) / (us * us + as_ * as_)
        Kf, Lf = as_ * inv, us * inv
        # fraction
        rr, ri = u.copy(), a.copy()
        for k in range(12, 0, -1):
            inv = (0.5 * k) / (rr * rr + ri * ri)
            rr, ri = u - rr * inv, ri * inv + a
        inv = isp / (rr * rr + ri * ri)
        Kc, Lc = ri * inv, rr * inv
        # lattice (evaluated on clipped arguments where another path is taken)
        ul, al = np.where(lat, u, 0.3), np.where(lat, a, 0.1)
        t = 2.0 * ul
        f = t - np.rint(t)
        mid = np.abs(f) <= 0.25
        z2r, z2i = (ul - al) * (ul + al), 2.0 * (ul * al)
        z2i2 = z2i * z2i
        sr, sv = np.zeros_like(ul), np.zeros_like(ul)
        for n in range(14):
            dr = z2r - np.where(mid, _T2M[n], _T2I[n])
            inv = np.where(mid, _EM[n], _EI[n]) / (dr * dr + z2i2)
            sr = dr * inv + sr
            sv = sv + inv
        si = -(z2i * sv)
        zr = 2.0 * (ul * sr - al * si)
        zi = 2.0 * (ul * si + al * sr)
        idd = 1.0 / (ul * ul + al * al)
        zr = np.where(mid, zr, ul * idd + zr)
        zi = np.where(mid, zi, -al * idd + zi)
        hpi = 0.15915494309189533577
        tr, ti = -(hpi * zi), hpi * zr
        sn, cs = sincos_2pi(f)
        sa, ca = sincos_2pi(z2i * hpi)
        mag = exp_any(12.566370614359172954 * al)
        sm = np.where(mid, mag, -mag)
        qr, qi = sm * cs + 1.0, -(sm * sn)
        g = 2.0 * exp_any(-z2r)
        gr, gi = g * ca, -(g * sa)
        iq = 1.0 / (qr * qr + qi * qi)
        Kl = tr + (gr * qr + gi * qi) * iq
        Ll = ti + (gi * qr - gr * qi) * iq
    K = np.where(lat, Kl, np.where(far, Kf, Kc))
    L = np.where(lat, Ll, np.where(far, Lf, Lc))
    if with_path:
        return K, L, np.where(lat, np.where(mid, 3, 2), np.where(far, 0, 1))
    return K, L


def w_exact_mp(u, a):
    z = mp.mpc(mp.mpf(float(u)), mp.mpf(float(a)))
    if abs(z) > 1e6:                                    # erfc's own asymptotics, 6 terms: 1e-66
        s, t = mp.mpf(0), mp.mpf(1)
        for k in range(8):
            s += t
            t *= mp.mpf(2 * k + 1) / (2 * z * z)
        return mp.mpc(0, 1) / (mp.sqrt(mp.pi) * z) * s
    return mp.exp(-z * z) * mp.erfc(mp.mpc(0, -1) * z)


def w_error(u, a, dps=50):
    """|w_dev - w| / |w| for arrays of points, measured in mpmath -> (error, path)."""
    u = np.asarray(u, dtype=np.float64).reshape(-1)
    a = np.broadcast_to(np.asarray(a, dtype=np.float64), u.shape).reshape(-1)
    K, L, path = w_dev(u, a, True)
    err = np.empty(u.size)
    with mp.workdps(dps):
        for i in range(u.size):
            w = w_exact_mp(u[i], a[i])
            err[i] = float(abs(mp.mpc(float(K[i]), float(L[i])) - w) / abs(w))
    return err, path


def _ld(v):
    """an mpf -> long double through two doubles"""
    hi = float(v)
    return LD(hi) + LD(float(v - mp.mpf(hi)))


def _mpf(v):
    """a long double -> mpf, exactly"""
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(LD(v) - LD(hi)))


_W_CACHE = {}


def w_exact_ld(u, a):
    """(K, L) in long double of long-double arrays u and a scalar a (mpmath at 30 digits on the
    arguments rounded to 64 bits of mantissa)."""
    u = np.asarray(u, dtype=LD).reshape(-1)
    K, L = np.empty(u.size, dtype=LD), np.empty(u.size, dtype=LD)
    # |z| >= 12: the Laplace continued fraction, 40 levels, in long double (its error there is below
    # 2e-19: test_w_against_scipy_... holds it to mpmath); mpmath for the rest
    aL = LD(a)
    far = u * u + aL * aL >= 144
    if far.any():
        zr, zi = u[far], np.full(int(far.sum()), aL, dtype=LD)
        rr, ri = zr.copy(), zi.copy()
        for k in range(40, 0, -1):
            inv = (LD(k) / 2) / (rr * rr + ri * ri)
            rr, ri = zr - rr * inv, zi + ri * inv
        inv = 1 / (np.sqrt(PI_LD) * (rr * rr + ri * ri))
        K[far], L[far] = ri * inv, rr * inv
    with mp.workdps(30):
        ah, al = float(a), float(LD(a) - LD(float(a)))
        am = mp.mpf(ah) + mp.mpf(al)
        for i in np.nonzero(~far)[0]:
            hi = float(u[i])
            lo = float(u[i] - LD(hi))
            key = (hi, lo, ah, al)
            if key not in _W_CACHE:
                z = mp.mpc(mp.mpf(hi) + mp.mpf(lo), am)
                w = (mp.exp(-z * z) * mp.erfc(mp.mpc(0, -1) * z)) if abs(z) < 1e6 else \
                    mp.mpc(0, 1) / (mp.sqrt(mp.pi) * z) * (1 + 1 / (2 * z * z) + 3 / (4 * z ** 4))
                _W_CACHE[key] = (_ld(w.real), _ld(w.imag))
            K[i], L[i] = _W_CACHE[key]
    return K, L


def n_params(n_comp):
    return 4 * int(n_comp) + 2


def profile(theta, x, x_ref, n_comp):
    """The model in long double with the exact w -> y [F] (long double)."""
    return _ref_channel(np.asarray(theta, dtype=LD), np.asarray(x, dtype=LD), LD(x_ref), n_comp)[0]


def _ref_channel(th, x, x_ref, nc):
    """model [F], J [P, F] in long double, and the error parts (dm [F], dJ [P, F], mabs) in float64
    by the docstring's formulas."""
    P = 4 * nc + 2
    F = x.size
    m = np.zeros(F, dtype=LD)
    J = np.zeros((P, F), dtype=LD)
    dJ = np.zeros((P, F))
    dm = np.zeros(F)
    mabs = np.zeros(F)
    sq2, sq2pi = np.sqrt(LD(2)), np.sqrt(2 * PI_LD)
    for k in range(nc):
        Fk, x0, s, g = th[4 * k:4 * k + 4]
        rs = 1 / s
        q = rs / sq2
        a = g * q
        cn = rs / sq2pi
        u = (x - x0) * q
        K, L = w_exact_ld(u, a)
        Rw = -2 * (u * K - a * L)
        Iw = -2 * (u * L + a * K) + 2 / np.sqrt(PI_LD)
        c = Fk * cn
        m = m + c * K
        J[4 * k] = K * cn
        J[4 * k + 1] = -(c * q) * Rw
        J[4 * k + 2] = -(c * rs) * (K + u * Rw - a * Iw)
        J[4 * k + 3] = -(c * q) * Iw
        f = lambda v: np.abs(np.asarray(v, dtype=np.float64))
        uf, af, Kf, Lf, Rf, If = f(u), float(abs(a)), f(K), f(L), f(Rw), f(Iw)
        e_w = EPS_W * np.hypot(Kf, Lf) + np.hypot(Rf, If) * (4 * uf + 3 * af) * EPS
        dRw = 2 * (uf * e_w + af * e_w) + 8 * EPS * (uf * Kf + af * Lf)
        dIw = 2 * (uf * e_w + af * e_w) + 8 * EPS * (uf * Lf + af * Kf + 1 / SQRT_PI)
        cf, cqf, crf, cnf = float(abs(c)), float(abs(c * q)), float(abs(c * rs)), float(abs(cn))
        dm += cf * (e_w + 4 * EPS * Kf)
        mabs += cf * Kf
        dJ[4 * k] = cnf * (e_w + 3 * EPS * Kf)
        dJ[4 * k + 1] = cqf * (dRw + 6 * EPS * Rf)
        dJ[4 * k + 2] = crf * (e_w + uf * dRw + af * dIw + 8 * EPS * (Kf + uf * Rf + af * If))
        dJ[4 * k + 3] = cqf * (dIw + 6 * EPS * If)
    xr = x - x_ref
    m = m + (th[P - 1] * xr + th[P - 2])
    J[P - 2] = 1
    J[P - 1] = xr
    dJ[P - 1] = EPS * np.abs(xr.astype(np.float64))
    mabs += float(abs(th[P - 2])) + np.abs((th[P - 1] * xr).astype(np.float64))
    dm += (nc + 3) * EPS * mabs
    return m, J, dm, dJ


def ref_sums(theta, y, x, x_ref, w, n_comp, free):
    """chi^2, N, g of `theta` over the counted channels in long double with their bounds ->
    dict(chi, N [P, P], g [P], B_chi, dN, dg, n, J, r): the fixed parameters' rows by the rule."""
    nc = int(n_comp)
    P = 4 * nc + 2
    y = np.asarray(y, dtype=np.float64)
    w = np.ones_like(y) if w is None else np.asarray(w, dtype=np.float64)
    keep = np.isfinite(y) & (w > 0)
    xs = np.asarray(x, dtype=np.float64)[keep].astype(LD)
    ys, ws = y[keep].astype(LD), w[keep].astype(LD)
    n = int(keep.sum())
    th = np.asarray(theta, dtype=np.float64).astype(LD)
    m, J, dm, dJ = _ref_channel(th, xs, LD(x_ref), nc)
    r = ys - m
    rf, wf = np.abs(r.astype(np.float64)), ws.astype(np.float64)
    dr = dm + EPS * rf
    chi = (ws * r * r).sum()
    B = float((wf * (2 * rf * dr + dr * dr)).sum() + (n + 2) * EPS * float(chi)) + n * TINY
    N = np.einsum("c,ic,jc->ij", ws, J, J)
    g = np.einsum("c,ic,c->i", ws, J, r)
    Jf = np.abs(J.astype(np.float64))
    dN = (np.einsum("c,ic,jc->ij", wf, Jf, dJ) + np.einsum("c,ic,jc->ij", wf, dJ, Jf) +
          np.einsum("c,ic,jc->ij", wf, dJ, dJ) + (n + 2) * EPS * np.einsum("c,ic,jc->ij", wf, Jf, Jf) +
          n * TINY)
    dg = (np.einsum("c,ic,c->i", wf, Jf, dr) + np.einsum("c,ic,c->i", wf, dJ, rf) +
          np.einsum("c,ic,c->i", wf, dJ, dr) + (n + 2) * EPS * np.einsum("c,ic,c->i", wf, Jf, rf) + n * TINY)
    fr = np.ones(P, dtype=bool) if free is None else np.asarray(free).reshape(-1) != 0
    for i in range(P):
        if not fr[i]:
            N[i, :] = 0
            N[:, i] = 0
            N[i, i] = 1
            g[i] = 0
            dN[i, :] = 0
            dN[:, i] = 0
            dg[i] = 0
    return dict(chi=chi, N=N, g=g, B_chi=B, dN=dN, dg=dg, n=n, J=J, r=r, w=ws)


def feasible(theta, n_comp):
    t = np.asarray(theta, dtype=np.float64)
    return all(np.isfinite(t[4 * c + 2]) and t[4 * c + 2] > 0 and np.isfinite(t[4 * c + 3]) and
               t[4 * c + 3] >= 0 for c in range(int(n_comp)))


def scales(theta, n_comp):
    t = np.asarray(theta, dtype=np.float64)
    P = 4 * int(n_comp) + 2
    s = np.empty(P)
    for c in range(int(n_comp)):
        s[4 * c] = max(abs(t[4 * c]), 1e-300)
        s[4 * c + 1:4 * c + 4] = max(t[4 * c + 2], t[4 * c + 3], 1e-300)
    s[P - 2:] = np.maximum(np.abs(t[P - 2:]), 1e-300)
    return s


def _chol_solve(N, g, lam):
    """lm_solve in float64 -> (delta, ok)"""
    P = g.size
    L = np.zeros((P, P))
    ok = True
    with np.errstate(all="ignore"):
        for j in range(P):
            d = lam * N[j, j] + N[j, j]
            for k in range(j):
                d = d - L[j, k] * L[j, k]
            ok = ok and d > 0.0
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, P):
                s = N[j, i]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
        yv = np.zeros(P)
        for i in range(P):
            s = g[i]
            for k in range(i):
                s = s - L[i, k] * yv[k]
            yv[i] = s / L[i, i]
        delta = np.zeros(P)
        for i in range(P - 1, -1, -1):
            s = yv[i]
            for k in range(i + 1, P):
                s = s - L[k, i] * delta[k]
            delta[i] = s / L[i, i]
    return delta, bool(ok)


def _dev_sums(th, y, x, x_ref, w, nc, mistake):
    """chi^2, N, g of a trial in float64 by the header's products (vectorised over the channels;
    the sums are not the device's chains: within (n + 2) eps of them)."""
    P = 4 * nc + 2
    keep = np.isfinite(y) & (w > 0)
    xs, ys, ws = x[keep], y[keep], w[keep]
    if mistake == "drop_weight":
        ws = np.ones_like(ws)
    J = np.zeros((P, xs.size))
    m = np.zeros(xs.size)
    with np.errstate(all="ignore"):
        for k in range(nc):
            Fk, x0, s, g = th[4 * k:4 * k + 4]
            rs = 1.0 / s
            q = rs * 0.70710678118654752440
            a = g * q
            if mistake == "a_gs":
                a = g * rs
            if mistake == "fwhm":
                a = (0.5 * g) * q
            cn = rs * 0.39894228040143267794
            u = (xs - x0) * q
            K, L = w_dev(u, np.full_like(u, abs(a)))
            if a < 0 and mistake != "accept_neg_g":     # (the device's w is not defined there)
                K, L = K * np.nan, L * np.nan
            Rw = -2.0 * (u * K - a * (-L if mistake == "L_sign" else L))
            Iw = -2.0 * (u * L + a * K) + 1.1283791670955125739
            cF = Fk * cn
            cq = cF * q
            m = m + cF * K
            J[4 * k] = K * cn
            J[4 * k + 1] = -(cq * Rw)
            J[4 * k + 2] = -(cF * rs) * ((0.0 if mistake == "dropK" else K) + u * Rw - a * Iw)
            J[4 * k + 3] = -(cq * Iw)
        xr = xs - x_ref
        m = m + (th[P - 1] * xr + th[P - 2])
        J[P - 2] = 1.0
        J[P - 1] = xr
        r = ys - m
        chi = float(np.sum((ws * r) * r))
        N = np.einsum("ic,jc->ij", ws * J, J)
        gv = np.einsum("ic,c->i", ws * J, r)
    return chi, N, gv, int(keep.sum())


def emulate(y, x, x_ref, theta0, n_comp=1, w=None, free=None, lambda0=1e-3, xtol=1e-10, n_iter=40,
            mistake=None):
    """The kernel for one pixel in float64 -> dict(theta, chi2, cov [P, P], nchan, niter, status,
    trace [niter, 3 + P]); status 3: the status alone."""
    nc = int(n_comp)
    P = 4 * nc + 2
    y = np.asarray(y, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    w = np.ones_like(y) if w is None else np.asarray(w, dtype=np.float64)
    fr = np.ones(P, dtype=bool) if free is None else np.asarray(free).reshape(-1) != 0
    th_c = np.array(theta0, dtype=np.float64)
    if not (np.isfinite(th_c).all() and feasible(th_c, nc)):
        return dict(status=3)
    th_t = th_c.copy()
    Nc, gc = np.zeros((P, P)), np.zeros(P)
    chi_c, lam, lam_used = np.inf, lambda0, lambda0
    rows = []
    it = 1
    cnt = 0
    while True:
        chi_t, Nt, gt, n = _dev_sums(th_t, y, x, x_ref, w, nc, mistake)
        if it == 1:
            cnt = n
            if cnt < int(fr.sum()) or not np.isfinite(chi_t):
                return dict(status=3)
        feas = feasible(th_t, nc)
        if mistake == "accept_neg_g":
            feas = all(np.isfinite(th_t[4 * c + 2]) and th_t[4 * c + 2] > 0 for c in range(nc))
        acc = bool(feas and np.isfinite(chi_t) and chi_t < chi_c)
        rows.append(np.concatenate([[chi_t, lam_used, 1.0 if acc else 0.0], th_t]))
        if acc:
            th_c = th_t.copy()
            Nc, gc = Nt.copy(), gt.copy()
            for i in range(P):
                if not fr[i]:
                    Nc[i, :] = 0.0
                    Nc[:, i] = 0.0
                    Nc[i, i] = 1.0
                    gc[i] = 0.0
            chi_c = chi_t
            if it > 1:
                lam = max(lam / 10.0, 1e-12)
        else:
            lam *= 10.0
        if chi_c == 0.0:
            status = 1
            break
        ok = False
        while True:
            if lam > 1e12:
                break
            delta, ok = _chol_solve(Nc, gc, lam)
            if ok:
                break
            lam *= 10.0
        if not ok:
            status = 2
            break
        worst = np.fmax.reduce(np.abs(delta) / scales(th_c, nc), initial=0.0)
        if not np.isnan(delta).any() and worst <= xtol:
            status = 1
            break
        if it == n_iter:
            status = 0
            break
        th_t = th_c + delta
        lam_used = lam
        it += 1
    return dict(theta=th_c, chi2=chi_c, cov=Nc, nchan=cnt, niter=it, status=status,
                trace=np.array(rows))


def tri(P):
    return [(i, j) for i in range(P) for j in range(i, P)]


def unpack(cov, P):
    N = np.zeros((P, P))
    for k, (i, j) in enumerate(tri(P)):
        N[i, j] = N[j, i] = cov[k]
    return N


def follow(res, y, x, x_ref, theta0, n_comp=1, w=None, free=None, lambda0=1e-3, xtol=1e-10,
           n_iter=40, trace_tail=None, stats=None):
    """Hold one pixel's result (`emulate`'s dict; a device pixel brought to that form) to the
    reference, by the module docstring.  `trace_tail`: the rows at and beyond niter as the device
    left them (must all be NaN = the caller's poison).  `stats`: a dict that collects the worst
    measured / bound shares ('chi', 'step', 'cov') and the counts 'decisions', 'unjudged'."""
    nc = int(n_comp)
    P = 4 * nc + 2
    st = stats if stats is not None else {}
    for k in ("chi", "step", "cov"):
        st.setdefault(k, 0.0)
    for k in ("decisions", "unjudged"):
        st.setdefault(k, 0)
    y = np.asarray(y, dtype=np.float64)
    wv = np.ones_like(y) if w is None else np.asarray(w, dtype=np.float64)
    fr = np.ones(P, dtype=bool) if free is None else np.asarray(free).reshape(-1) != 0
    th0 = np.asarray(theta0, dtype=np.float64)
    cnt = int((np.isfinite(y) & (wv > 0)).sum())
    degenerate = not (np.isfinite(th0).all() and feasible(th0, nc)) or cnt < int(fr.sum())
    if not degenerate:
        first = ref_sums(th0, y, x, x_ref, wv, nc, fr)
        # (a first chi^2 that overflows float64 is degenerate too; the cases keep clear of the edge)
        degenerate = not np.isfinite(float(first["chi"]))
    if degenerate:
        assert res["status"] == 3, res["status"]
        return st
    assert res["status"] in (0, 1, 2), res["status"]
    tr = np.asarray(res["trace"], dtype=np.float64)
    niter = int(res["niter"])
    assert 1 <= niter <= n_iter and tr.shape[0] >= niter
    if trace_tail is not None:
        assert np.isnan(trace_tail).all(), "trace rows at and beyond niter were written"
    assert res["nchan"] == cnt
    assert np.array_equal(tr[0, 3:], th0)
    th_c, chi_c_dev, cur = None, np.inf, None
    lam, lam_used = lambda0, lambda0
    status = None
    for it in range(1, niter + 1):
        row = tr[it - 1]
        chi_t, th_t = row[0], row[3:]
        assert row[1] == lam_used, (it, row[1], lam_used)
        fin = np.isfinite(th_t).all()
        ref = ref_sums(th_t, y, x, x_ref, wv, nc, fr) if fin and feasible(th_t, nc) else None
        if ref is not None and np.isfinite(float(ref["chi"])):
            err = abs(float(LD(chi_t) - ref["chi"]))
            assert err <= ref["B_chi"], ("chi2", it, chi_t, float(ref["chi"]), err, ref["B_chi"])
            st["chi"] = max(st["chi"], err / ref["B_chi"]) if ref["B_chi"] > 0 else st["chi"]
        acc = bool(feasible(th_t, nc) and np.isfinite(chi_t) and chi_t < chi_c_dev)
        assert row[2] == (1.0 if acc else 0.0), ("accept", it, row[2], acc)
        st["decisions"] += 1
        if ref is not None and cur is not None and np.isfinite(chi_t):
            gap = abs(float(ref["chi"] - cur["chi"]))
            if gap > ref["B_chi"] + cur["B_chi"]:
                assert acc == bool(ref["chi"] < cur["chi"]), ("order", it)
            else:
                st["unjudged"] += 1
        if acc:
            assert ref is not None
            th_c, chi_c_dev, cur = th_t.copy(), chi_t, ref
            if it > 1:
                lam = max(lam / 10.0, 1e-12)
        else:
            lam *= 10.0
        if chi_c_dev == 0.0:
            status = 1
            break
        # the breakdown loop on the reference's A: a pivot is clear when the float64 factorisation
        # of the reference's N succeeds / fails with a margin (the cases keep clear of the edge)
        Nf, gf = cur["N"].astype(np.float64), cur["g"].astype(np.float64)
        ok = False
        while lam <= 1e12:
            _, ok = _chol_solve(Nf, gf, lam)
            if ok:
                break
            lam *= 10.0
        if not ok:
            status = 2
            break
        last = it == niter
        if last:
            # the stop: either the step test held on the device (status 1) or n_iter ran out
            status = res["status"]
            assert status in (0, 1)
            if status == 0:
                assert niter == n_iter
            if status == 1:
                # a step within xtol of the scales solves the system to its backward error: necessary
                A = cur["N"] + LD(lam) * np.diag(np.diag(cur["N"]))
                Af = np.abs(A.astype(np.float64))
                dA = (1 + lam) * cur["dN"] + (3 * P + 2) * EPS * np.sqrt(np.outer(np.diag(Af), np.diag(Af)))
                small = xtol * scales(th_c, nc) * fr
                lim = (Af + dA) @ small + cur["dg"]
                gabs = np.abs(cur["g"].astype(np.float64))
                assert np.all(gabs <= lim), ("stopped early", it, gabs, lim)
            break
        nxt = tr[it, 3:]
        delta = nxt.astype(LD) - th_c.astype(LD)
        assert np.all(nxt[~fr] == th_c[~fr]), "a fixed parameter moved"
        A = cur["N"] + LD(lam) * np.diag(np.diag(cur["N"]))
        Af = np.abs(A.astype(np.float64))
        dA = (1 + lam) * cur["dN"] + (3 * P + 2) * EPS * np.sqrt(np.outer(np.diag(Af), np.diag(Af)))
        for i in range(P):
            if not fr[i]:
                dA[i, :] = 0
                dA[:, i] = 0
        resid = np.abs((A @ delta - cur["g"]).astype(np.float64))
        df = np.abs(delta.astype(np.float64))
        tol = dA @ df + cur["dg"] + Af @ (EPS * np.abs(nxt))
        bad = resid > tol
        assert not bad.any(), ("step", it, resid, tol)
        with np.errstate(all="ignore"):
            share = np.where(tol > 0, resid / tol, 0.0)
        st["step"] = max(st["step"], float(np.max(share)))
        worst = np.max(df / scales(th_c, nc))
        assert worst > 0.5 * xtol, ("went on after convergence", it, worst)
        lam_used = lam
    assert res["status"] == status, (res["status"], status)
    assert np.array_equal(np.asarray(res["theta"], dtype=np.float64), th_c)
    assert res["chi2"] == chi_c_dev
    cov = np.asarray(res["cov"], dtype=np.float64)
    errN = np.abs((cov.astype(LD) - cur["N"]).astype(np.float64))
    assert np.all(errN <= cur["dN"]), ("cov", errN, cur["dN"])
    with np.errstate(all="ignore"):
        st["cov"] = max(st["cov"], float(np.max(np.where(cur["dN"] > 0, errN / cur["dN"], 0.0))))
    return st


def first_order_shift(theta, y, x, x_ref, n_comp, free, dy):
    """|N^-1 J^T W| |dy|: the first-order bound of the shift of the fitted parameters when channel c
    of the data moves by at most dy[c] -> [P] (0 for fixed parameters)."""
    P = 4 * int(n_comp) + 2
    fr = np.ones(P, dtype=bool) if free is None else np.asarray(free).reshape(-1) != 0
    s = ref_sums(theta, y, x, x_ref, None, n_comp, fr)
    keep = np.isfinite(np.asarray(y, dtype=np.float64))
    J = s["J"].astype(np.float64)[fr]
    Ninv = np.linalg.inv(s["N"].astype(np.float64)[np.ix_(fr, fr)])
    out = np.zeros(P)
    out[fr] = np.abs(Ninv @ J) @ np.abs(np.asarray(dy, dtype=np.float64)[keep])
    return out
