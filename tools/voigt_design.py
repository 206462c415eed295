#!/usr/bin/env python3
"""Design and error budget of K3's wave-uniform Faddeeva paths (rajepy_amd/csrc/rrl_scan.hip).

The reference evaluates the Voigt profile through scipy.special.wofz (maths/rrls.py:350-354);
BASELINE.json's bar on the maps is 1e-5 relative, SURVEY.md section 7 asks for <= 1e-7 on
Re w.  Round 3 spends that budget: the wave-uniform paths are designed for <= 1e-8 relative on
Re w(x + i y) over their whole domain (one order inside SURVEY's bound, three inside the
bar), instead of the 1e-11 of rounds 1-2 -- a wider lattice step, fewer nodes, shorter series
and polynomials.  This script restates every path in NumPy float64 with the kernel's operation
structure and constants, measures it against scipy.special.wofz over the path's domain, and
prints the constants the kernel uses.  (scipy is test / design infrastructure here; the product
never imports it for this.)

    python tools/voigt_design.py            # error table + constants
"""
import numpy as np
from scipy.special import wofz

np.seterr(all="ignore")

H = 0.675                  # lattice step of the wave-uniform paths (generic per-lane path: 0.6)
NPAIR = 8                  # node pairs t_n = n h, n = 0 .. 7 (n = 0 self-paired)
CEN_J = 7                  # centred lattice: nodes on each side of the middle one
CEN_YMAX = 0.03            # below: centred lattice (sum and pole term of the plain one cancel)
FAR = ((6, 64.0), (4, 196.0))     # (series terms K, |z|^2 above which every lane must lie)
TOL_POLE = 3e-8            # pole term skipped where a rigorous bound puts it below this * Re w
POLE_LITE_Y = 1.3          # from here on the pole term is taken to leading order in q (one cosine)
C_FAR = [1.0, 0.5, 0.75, 1.875, 6.5625, 29.53125, 162.421875, 1055.7421875, 7918.06640625]

# near-minimax polynomials (tools/minimax_fit.py): cos on |w| <= pi/2 in s = w^2 (degree 10 in
# w, abs err 1.1e-9), exp on |r| <= ln2/2 (degree 7, rel err 3.9e-10); the names are those of
# the first half of round 3 (degree 12 / 8)
COS12 = [-2.62979486641630506e-07, 2.47753637598607603e-05, -1.38886802208908807e-03,
         4.16666619921366096e-02, -0.5, 1.0]
EXP8 = [1.73659676346479309e-04, 1.39332571536309119e-03, 8.33781514566415451e-03,
        4.16664825818220744e-02, 1.66666480404710465e-01, 0.5, 1.0, 1.0]


def horner(c, x):
    p = np.full_like(x, c[0])
    for k in c[1:]:
        p = p * x + k
    return p


def cos_halfturns(h):
    """cos(pi h) as the kernel evaluates it (cos_2pi_x3): k = rint(h), d = h - k, the polynomial
    in d^2 with pi^2j folded into the coefficients, (-1)^k into the sign bit"""
    k = np.rint(h)
    d = h - k
    c = [COS12[j] * np.pi ** (10 - 2 * j) for j in range(6)]
    p = horner(c, d * d)
    return np.where(k.astype(np.int64) & 1, -p, p)


def exp_neg_k(x2):
    """exp(-x2) as the kernel evaluates it: t = -x2 log2(e) = k + f, 2^f from the exp polynomial
    with ln2^j folded into its coefficients"""
    t = -1.4426950408889634074 * x2
    kd = np.rint(t)
    f = t - kd
    ln2 = np.log(2.0)
    c = [EXP8[j] * ln2 ** (7 - j) for j in range(8)]
    return np.ldexp(horner(c, f), kd.astype(np.int64))


def far_series(x, y, K):
    x2, y2 = x * x, y * y
    r2 = x2 + y2
    inv = 1.0 / (r2 * r2)
    ur, nui = (x2 - y2) * inv, 2.0 * (x * y) * inv
    pr = C_FAR[K - 1] + C_FAR[K] * ur
    pi = -C_FAR[K] * nui
    for k in range(K - 2, -1, -1):
        t = pr * ur + (pi * nui + C_FAR[k])
        pi = -pr * nui + pi * ur
        pr = t
    return (y * pr - x * pi) * (r2 * inv) * 0.56418958354775628695


def plain_wave(x, y, pole):
    """Eight node pairs over one common denominator (voigt_plain_wave)."""
    tau = [(n * H) ** 2 for n in range(NPAIR)]
    w2 = [1.0] + [2.0 * np.exp(-t) for t in tau[1:]]
    x2 = x * x
    r2 = y * y + x2
    X4 = -4.0 * x2
    N, D = [], []
    for a in range(0, NPAIR, 2):
        ma = r2 if a == 0 else tau[a] + r2
        mb = tau[a + 1] + r2
        da = ma * ma if a == 0 else tau[a] * X4 + ma * ma
        db = tau[a + 1] * X4 + mb * mb
        N.append(ma * db + (w2[a + 1] / w2[a]) * (mb * da))
        D.append(da * db)
    N01, D01 = N[0] * D[1] + (w2[2] / w2[0]) * (N[1] * D[0]), D[0] * D[1]
    N23, D23 = N[2] * D[3] + (w2[6] / w2[4]) * (N[3] * D[2]), D[2] * D[3]
    Nall, Dall = N01 * D23 + (w2[4] / w2[0]) * (N23 * D01), D01 * D23
    ky = (w2[0] * H / np.pi) * y
    if not pole:
        return Nall / Dall * ky
    q = np.exp(-2.0 * np.pi * y / H)
    gq = 2.0 * q * np.exp(y * y)               # staged per cell
    u = (2.0 / H) * x                          # half-turns
    ph = 0.63661977236758134308 * (x * y)
    if pole == "lite":                         # y >= POLE_LITE_Y: P = -2 E q cos(theta - phi)
        pq = exp_neg_k(x2) * gq * cos_halfturns(u - ph)
        return (Nall * ky - pq * Dall) / Dall
    cth, cph, cps = cos_halfturns(u), cos_halfturns(ph), cos_halfturns(u - ph)
    den = q * (q - 2.0 * cth) + 1.0
    num = q * cph - cps
    pq = exp_neg_k(x2) * gq * num
    return (Nall * ky * den + pq * Dall) / (Dall * den)


def pole_bound_cq(y, rmax2=67.0):
    """x^2 above which |P| <= 6 e^{y^2-x^2} q / (1-q)^2 is below TOL_POLE * Re w, with
    Re w >= y / (4 (|z|^2 + 1)) and |z|^2 < rmax2 - 1 on this path (cell_line)."""
    lnq = -2.0 * np.pi * y / H
    omq = -np.expm1(lnq)
    return (y * y + lnq + np.log(6.0) - 2.0 * np.log(omq) - np.log(0.25 * y) +
            np.log(1.0 / TOL_POLE) + np.log(rmax2))


def centred_cq(y):
    """x^2 above which the centred lattice leaves its pole term out (cell_line): |P| <= e^{y^2-x^2}
    against Re w >= y / (4 (|z|^2 + 1)) with |z|^2 <= 16^2 + 1."""
    return y * y - np.log(y) + np.log(1.0 / TOL_POLE) + np.log(4.0 * 258.0)


def centred(x, y, pole=True):
    """Lattice centred on x (voigt_centred), y < CEN_YMAX, x <= 16; pole=False: as a lane beyond
    the per-cell bound centred_cq runs it."""
    km = np.rint(-x / H - 0.5)
    tm = (km + 0.5) * H + x
    w = tm * tm
    em = horner([1.0 / 720.0, -1.0 / 120.0, 1.0 / 24.0, -1.0 / 6.0, 0.5, -1.0, 1.0], w)
    v = (-2.0 * H) * tm
    fact = [1.0]
    for k in range(1, 11):
        fact.append(fact[-1] * k)
    uu = horner([1.0 / f for f in fact[::-1]], v)
    kC1, kQ = np.exp(-H * H), np.exp(-2.0 * H * H)
    tab = lambda k: 1.0 / (((k + 0.5) * H) ** 2 + y * y)
    s = em * tab(km)
    e, r = em.copy(), kC1 * uu
    for j in range(1, CEN_J + 1):
        e = e * r
        r = r * kQ
        s = s + e * tab(km + j)
    e, r = em.copy(), kC1 / uu
    for j in range(1, CEN_J + 1):
        e = e * r
        r = r * kQ
        s = s + e * tab(km - j)
    s = s * (y * (H / np.pi))
    q = np.exp(-2.0 * np.pi * y / H)
    th = 2.0 * x * y
    t2 = th * th
    c = horner([1.0 / 40320.0, -1.0 / 720.0, 1.0 / 24.0, -0.5, 1.0], t2)     # cos, degree 8
    gq = 2.0 * q * np.exp(y * y) / (1.0 + q)       # staged per cell
    return s + exp_neg_k(x * x) * c * gq if pole else s


# ---- generic per-lane code (voigt_rew<false>: 16-lane layout, collapse=False, irregular cells) ----
H_GEN = 0.6                # its lattice step
NPAIR_GEN = 10
TOL_POLE_GEN = 1e-13       # pole term kept down to this * Re w


def generic_core(x, y):
    """voigt_rew<false> without its far-field branch (the core formula is valid everywhere, and a
    wave that straddles the far-field boundary runs it on every lane): plain lattice + pole term
    for y >= 0.03, the lattice shifted by h/2 near a node below (voigt_core_shifted)."""
    x, y = np.broadcast_arrays(np.asarray(x, dtype=float), np.asarray(y, dtype=float))
    r2 = x * x + y * y
    U = r2 * r2
    W = 2.0 * (y * y - x * x)
    u = x * (1.0 / H_GEN)
    fr = u - np.floor(u)
    half = (y < CEN_YMAX) & ~((fr >= 0.25) & (fr < 0.75))
    s = np.zeros_like(r2)
    for n in range(NPAIR_GEN):
        t0, t1 = (n * H_GEN) ** 2, ((n + 0.5) * H_GEN) ** 2
        tau = np.where(half, t1, t0)
        c2 = np.where(half, 2.0 * np.exp(-t1), 1.0 if n == 0 else 2.0 * np.exp(-t0))
        s = s + (c2 * r2 + c2 * tau) / (tau * (W + tau) + U)
    s = s * (y * (H_GEN / np.pi))
    lnq = -2.0 * (np.pi / H_GEN) * y
    q = np.exp(lnq)
    e = y * y - x * x
    omq = -np.expm1(lnq)
    cq = (y * y + lnq + np.log(6.0) - 2.0 * np.log(omq) - np.log(0.25 * y) +
          np.log(1.0 / TOL_POLE_GEN) + np.log(67.0))
    th = 2.0 * np.pi * (fr - np.where(half, 0.5, 0.0))
    ph = 2.0 * x * y
    den = q * (q - 2.0 * np.cos(th)) + 1.0
    # y >= 0.03: q cos(phi) - cos(theta - phi); below: the same, written out (cos and sin of both)
    num = q * np.cos(ph) - np.cos(th - ph)
    P = 2.0 * np.exp(e) * q * num / den
    need = np.where(y < CEN_YMAX, e + lnq > np.log(s) - 31.0, (y < np.pi / H_GEN) & (x * x < cq))
    return s + np.where(need, P, 0.0)


def generic_far(x, y):
    """voigt_far: 6 levels of the Laplace continued fraction."""
    wr, wi = x * np.ones_like(y), y * np.ones_like(x)
    for k in range(6, 0, -1):
        s = (0.5 * k) / (wr * wr + wi * wi)
        wr, wi = x - s * wr, y + s * wi
    return 0.56418958354775628695 * wi / (wr * wr + wi * wi)


def rel(a, ref):
    return np.abs(a - ref) / np.abs(ref)


def measure():
    """Worst relative error of every path over its domain against scipy.special.wofz:
    {name: (error, (x, y))} -- the figures of the accuracy budget at the head of rrl_scan.hip."""
    out = {}
    # ---- plain lattice (+ pole term) over its domain: 0.03 <= y, |z|^2 <= 64 or (x^2 <= 64, y <= 1)
    worst = (0, None)
    worst_skip = (0, None)
    for y in np.concatenate([np.geomspace(CEN_YMAX, 1, 80), np.linspace(1, 8.1, 143),
                             POLE_LITE_Y + np.array([0.0, 1e-9, 0.01, 0.03]),
                             (np.pi / H) * np.array([1.0 - 1e-9, 1.0, 1.0 + 1e-9])]):
        x = np.linspace(0, 8.0, 6401)
        x = x[(x * x + y * y <= 64.0) | ((x * x <= 64.0) & (y <= 1.0))]
        if x.size == 0:
            continue
        ref = wofz(x + 1j * y).real
        has_pole = y < np.pi / H
        full = plain_wave(x, y, ("lite" if y >= POLE_LITE_Y else True) if has_pole else False)
        e = rel(full, ref)
        i = int(np.argmax(e))
        if e[i] > worst[0]:
            worst = (e[i], (x[i], y))
        if has_pole:
            # lanes of a wave whose smallest x^2 exceeds cq run WITHOUT the pole term
            cq = pole_bound_cq(y)
            m = x * x >= cq
            if m.any():
                e2 = rel(plain_wave(x[m], y, False), ref[m])
                j = int(np.argmax(e2))
                if e2[j] > worst_skip[0]:
                    worst_skip = (e2[j], (x[m][j], y))
    out["plain"] = worst
    out["plain_skip"] = worst_skip
    # ---- far field
    for K, r2 in FAR:
        worst = (0, None)
        for y in np.geomspace(1e-10, 1e3, 260):
            x0 = np.sqrt(max(r2 - y * y, 64.0 if y <= 1.0 else 0.0))
            x = x0 * (1.0 + 1e-9) + np.concatenate([np.linspace(0, 4, 81), np.geomspace(4, 1e4, 40)])
            ok = x * x + y * y > r2
            ref = wofz(x + 1j * y).real
            e = np.where(ok, rel(far_series(x, y, K), ref), 0.0)
            i = int(np.argmax(e))
            if e[i] > worst[0]:
                worst = (e[i], (x[i], y))
        out["far%d" % K] = worst
    # ---- centred lattice
    worst = (0, None)
    for y in np.geomspace(1e-10, CEN_YMAX, 60):
        x = np.linspace(0, 16.0, 6401)
        ref = wofz(x + 1j * y).real
        e = rel(centred(x, y), ref)
        i = int(np.argmax(e))
        if e[i] > worst[0]:
            worst = (e[i], (x[i], y))
    out["centred"] = worst
    # lanes beyond the per-cell bound run without the pole term
    worst = (0, None)
    for y in np.geomspace(1e-10, CEN_YMAX, 240):
        x0 = np.sqrt(centred_cq(y))
        x = x0 + np.linspace(0.0, 1.0, 401)
        x = x[x <= 16.0]
        ref = wofz(x + 1j * y).real
        e = rel(centred(x, y, pole=False), ref)
        i = int(np.argmax(e))
        if e[i] > worst[0]:
            worst = (e[i], (x[i], y))
    out["centred_skip"] = worst
    # ---- generic per-lane code: the core formula over the whole range of the header of
    # rrl_voigt.h (1e-10 <= y <= 1e3, 0 <= x <= 1e4), the continued fraction over its far field
    worst_core, worst_far = (0, None), (0, None)
    xs = np.concatenate([np.linspace(0, 8.4, 6721), np.geomspace(8.4, 1e4, 400)])
    for y in np.concatenate([np.geomspace(1e-10, 1e3, 131), CEN_YMAX * np.array([1 - 1e-9, 1.0]),
                             (np.pi / H_GEN) * np.array([1 - 1e-9, 1.0])]):
        ref = wofz(xs + 1j * y).real
        e = rel(generic_core(xs, y), ref)
        i = int(np.argmax(e))
        if e[i] > worst_core[0]:
            worst_core = (e[i], (xs[i], y))
        far = (xs * xs + y * y > 64.0) & ((xs * xs > 64.0) | (y > 1.0))
        if far.any():
            e = np.where(far, rel(generic_far(xs, np.full_like(xs, y)), ref), 0.0)
            i = int(np.argmax(e))
            if e[i] > worst_far[0]:
                worst_far = (e[i], (xs[i], y))
    out["generic_core"] = worst_core
    out["generic_far"] = worst_far
    return out


def main():
    print("H = %.4f  pi/H = %.4f  NPAIR = %d  CEN_J = %d" % (H, np.pi / H, NPAIR, CEN_J))
    m = measure()
    print("plain lattice (pole term where y < pi/H): max rel err %.2e at x=%.3f y=%.4f"
          % (m["plain"][0], m["plain"][1][0], m["plain"][1][1]))
    print("plain lattice, pole term skipped beyond cq:  max rel err %.2e at x=%.3f y=%.4f"
          % (m["plain_skip"][0], m["plain_skip"][1][0], m["plain_skip"][1][1]))
    for K, r2 in FAR:
        print("far series K = %d, every lane |z|^2 > %g and (x^2 > 64 or y > 1): max rel err %.2e"
              % (K, r2, m["far%d" % K][0]))
    print("centred lattice (y < %.2f, x <= 16): max rel err %.2e at x=%.3f y=%.3e"
          % (CEN_YMAX, m["centred"][0], m["centred"][1][0], m["centred"][1][1]))
    print("centred lattice, pole term skipped beyond cq: max rel err %.2e at x=%.3f y=%.3e"
          % (m["centred_skip"][0], m["centred_skip"][1][0], m["centred_skip"][1][1]))
    print("generic per-lane core (h = %.1f, %d pairs; 1e-10 <= y <= 1e3, x <= 1e4): max rel err "
          "%.2e at x=%.4f y=%.3e" % (H_GEN, NPAIR_GEN, m["generic_core"][0],
                                     m["generic_core"][1][0], m["generic_core"][1][1]))
    print("generic per-lane far field (continued fraction, 6 levels): max rel err %.2e at x=%.4f "
          "y=%.3e" % (m["generic_far"][0], m["generic_far"][1][0], m["generic_far"][1][1]))
    # ---- constants for the kernel
    tau = [(n * H) ** 2 for n in range(NPAIR)]
    w2 = [1.0] + [2.0 * float(np.exp(-t)) for t in tau[1:]]
    print("tau  = {" + ", ".join(repr(t) for t in tau) + "}")
    print("w2   = {" + ", ".join(repr(t) for t in w2) + "}")
    print("kC1 = exp(-h^2) = %r   kQ = exp(-2 h^2) = %r" % (float(np.exp(-H * H)),
                                                           float(np.exp(-2 * H * H))))
    print("ln(1/TOL_POLE) = %r" % float(np.log(1.0 / TOL_POLE)))


if __name__ == "__main__":
    main()
