"""The reference of rjp_uv_weights (K15): the contract of include/rjprt.h restated on the host.

  * `integer_density`: the fixed-point density in PYTHON INTEGERS -- exact W(c), sum_k w_k, the
    counts and the shift s; the device must give these bit for bit.
  * `longdouble_density`: the same density summed in long double on the UNQUANTISED weights; the
    fixed point differs from it by at most n_c 2^(-s-1) per cell, n_c the contributions to the
    cell (each q_k = rint(w_k 2^s) is off by at most half a unit), plus the long-double sum's own
    rounding.
  * `weights`: w' in long double from the exact W, with a relative bound derived term by term.

The bound (u = 2^-53, relative, first order with gamma(n) = n u / (1 - n u) for the total):
  conversion      the device's W is ONE correctly rounded int64 -> double conversion of the
                  exact integer, the scaling by 2^-s is exact: 1 u;  sum_k w_k likewise: 1 u
  uniform         w / W: the conversion and the divide: 2 u
  sum_c W^2       every W carries 1 u, so W^2 carries 2 u; the products round once each (fused
                  or not): 1 u; the float64 sum of `cells` non-negative terms in ANY fixed order:
                  (cells - 1) u.  Together (cells + 2) u
  c2              (5 10^-R)^2 on the host: pow within 1 ulp = 2 u, times 5: 1 u, squared:
                  2 x 3 u + 1 u = 7 u
  f2              c2 (2 sum w) / sum W^2: 7 u + 1 u (sum w), the doubling exact, the product 1 u,
                  the divide 1 u, sum W^2 (cells + 2) u: (cells + 12) u
  the fma         d = fma(f2, W, 1): the term f2 W carries (cells + 12) u + 1 u (W) and weighs
                  f2 W / (1 + f2 W) <= 1 in d; the fma rounds once: (cells + 14) u
  the divide      w / d: 1 u.  Briggs in total: (cells + 15) u
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53

MSG = {
    "null": "rjp_uv_weights: NULL scales, baselines or output",
    "sizes": "rjp_uv_weights: n_maps, n_vis, nx and nz must be positive",
    "scale": "rjp_uv_weights: non-finite h_su / h_sv",
    "mode": "rjp_uv_weights: mode must be 1 (uniform) or 2 (Briggs)",
    "robust": "rjp_uv_weights: robust must be finite and lie in [-2, 2]",
    "cells": "rjp_uv_weights: more than 2^31 - 1 density cells",
    "grid": "rjp_uv_weights: more than 2^31 - 1 workgroups",
    "work": "rjp_uv_weights: workspace smaller than rjp_uv_weights_workspace()",
}
UNIFORM, BRIGGS = 1, 2


def gamma(n):
    return n * U / (1.0 - n * U)


def n_cells(nx, nz):
    return (2 * (nx // 2) + 1) * (2 * (nz // 2) + 1)


def workspace_bytes(n_maps, nx, nz, n_vis):
    """256 bytes, 32 per map, 8 per tile of 1024 cells and 8 per cell; 0 beyond 2^31 - 1 cells."""
    nc = n_cells(nx, nz)
    if nc > 2 ** 31 - 1:
        return 0
    return 256 + n_maps * (32 + 8 * (-(-nc // 1024)) + 8 * nc)


def workgroups(n_maps, n_vis):
    return n_maps * (-(-n_vis // 256))


def cells(su, sv, u, v, nx, nz, rounding="even"):
    """-> (cell index or -1 [K], in range [K]) of one map; float64 products in the contract's
    order.  `rounding` other than "even" plants a mistake."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    hx, hz = nx // 2, nz // 2
    with np.errstate(invalid="ignore", over="ignore"):
        pu = (np.float64(su) * u) * np.float64(nx)
        pv = (np.float64(sv) * v) * np.float64(nz)
        rnd = {"even": np.rint, "half_up": lambda x: np.floor(x + 0.5), "trunc": np.trunc}[rounding]
        gu, gv = rnd(pu), rnd(pv)
        inside = (np.abs(gu) <= hx) & (np.abs(gv) <= hz)
    idx = np.full(u.shape, -1, dtype=np.int64)
    idx[inside] = ((gu[inside].astype(np.int64) + hx) * (2 * hz + 1) +
                   (gv[inside].astype(np.int64) + hz))
    return idx, inside


def flagged(u, v, w):
    u, v, w = (np.asarray(a, np.float64) for a in (u, v, w))
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(u) & np.isfinite(v) & np.isfinite(w)) | ~(w >= 0)


def shift(w_max, n_vis):
    """s = 62 - e - L, w_max < 2^e (frexp), L = ceil(log2(2 n_vis)); 0 for w_max = 0."""
    if not w_max > 0:
        return 0
    e = int(np.frexp(np.float64(w_max))[1])
    L = (2 * int(n_vis) - 1).bit_length()
    return 62 - e - L


def integer_density(su, sv, u, v, w, nx, nz, mirror=True, origin_twice=True, rounding="even"):
    """The contract in Python integers for the maps (su[m], sv[m]) -> dict of per-map lists:
    `W` (float64 [cells], exact fixed point, correctly rounded once), `Q` (the integers),
    `sum_w` (float), `sum_q`, `counted`, `outside`, `idx` ([K], -1 = not counted), `n_c`
    (contributions per cell), and the scalars `s`, `w_max`.  The keywords plant mistakes."""
    su, sv = np.atleast_1d(np.asarray(su, np.float64)), np.atleast_1d(np.asarray(sv, np.float64))
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    K = u.size
    w = np.ones(K) if w is None else np.asarray(w, np.float64)
    bad = flagged(u, v, w)
    nc = n_cells(nx, nz)
    per = []
    w_max = 0.0
    for m in range(su.size):
        idx, inside = cells(su[m], sv[m], u, v, nx, nz, rounding)
        cnt = inside & ~bad
        per.append((np.where(cnt, idx, -1), int(np.count_nonzero(~inside & ~bad))))
        if cnt.any():
            w_max = max(w_max, float(w[cnt].max()))
    s = shift(w_max, K)
    out = dict(W=[], Q=[], sum_w=[], sum_q=[], counted=[], outside=[], idx=[], n_c=[], s=s,
               w_max=w_max)
    q = [int(x) for x in np.rint(np.ldexp(np.where(bad, 0.0, w), s))] if w_max > 0 else [0] * K
    for idx, outside in per:
        S, n_c = [0] * nc, np.zeros(nc, dtype=np.int64)
        for k in np.nonzero(idx >= 0)[0]:
            c = int(idx[k])
            S[c] += q[k]
            n_c[c] += 1
        if mirror:
            Q = [S[c] + S[nc - 1 - c] for c in range(nc)]
            n_c = n_c + n_c[::-1]
            if not origin_twice:
                Q[nc // 2], n_c[nc // 2] = S[nc // 2], n_c[nc // 2] // 2
        else:
            Q = S
        sum_q = sum(q[k] for k in np.nonzero(idx >= 0)[0])
        assert sum(Q) < 2 ** 62 and all(x < 2 ** 62 for x in Q)
        out["Q"].append(Q)
        out["W"].append(np.array([np.ldexp(float(x), -s) for x in Q], dtype=np.float64))
        out["sum_q"].append(sum_q)
        out["sum_w"].append(float(np.ldexp(float(sum_q), -s)))
        out["counted"].append(int(np.count_nonzero(idx >= 0)))
        out["outside"].append(outside)
        out["idx"].append(idx)
        out["n_c"].append(n_c)
    return out


def longdouble_density(su, sv, u, v, w, nx, nz):
    """W(c) per map in long double on the weights as given (no fixed point) -> list of [cells]."""
    su, sv = np.atleast_1d(np.asarray(su, np.float64)), np.atleast_1d(np.asarray(sv, np.float64))
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    w = np.ones(u.size) if w is None else np.asarray(w, np.float64)
    bad = flagged(u, v, w)
    nc = n_cells(nx, nz)
    out = []
    for m in range(su.size):
        idx, inside = cells(su[m], sv[m], u, v, nx, nz)
        cnt = inside & ~bad
        S = np.zeros(nc, dtype=LD)
        np.add.at(S, idx[cnt], w[cnt].astype(LD))
        out.append(S + S[::-1])
    return out


def as_ld(Q, s):
    """The exact fixed-point values as long doubles (integers below 2^62 fit its 64 bits)."""
    hi = np.array([x >> 31 for x in Q], dtype=np.int64).astype(LD)
    lo = np.array([x & (2 ** 31 - 1) for x in Q], dtype=np.int64).astype(LD)
    return np.ldexp(hi * LD(2 ** 31) + lo, -s)


def c2_of(robust):
    return (LD(5) * LD(10) ** LD(-robust)) ** 2


def weights(dens, w, mode, robust=0.5):
    """-> dict of per-map lists from `integer_density`'s result: `wout` (long double [K]), `f2`,
    `sum_w2` (long double), and the relative bounds `b_wout`, `b_f2`, `b_sum_w2` (floats)."""
    K = dens["idx"][0].size
    w = np.ones(K) if w is None else np.asarray(w, np.float64)
    out = dict(wout=[], f2=[], sum_w2=[], b_wout=[], b_f2=[], b_sum_w2=[])
    for m, Q in enumerate(dens["Q"]):
        nc = len(Q)
        W = as_ld(Q, dens["s"])
        sw2 = (W * W).sum()
        sum_w = as_ld([dens["sum_q"][m]], dens["s"])[0]
        f2 = LD(0)
        if mode == BRIGGS and sw2 > 0:
            f2 = c2_of(robust) * (2 * sum_w) / sw2
        idx = dens["idx"][m]
        ok = idx >= 0
        Wk = np.where(ok, W[np.where(ok, idx, 0)], LD(1))
        wl = np.where(ok, w, 0.0).astype(LD)
        if mode == BRIGGS:
            r = wl / (f2 * Wk + 1)
        else:
            r = np.where(Wk > 0, wl / np.where(Wk > 0, Wk, LD(1)), LD(0))
        out["wout"].append(np.where(ok, r, LD(0)))
        out["f2"].append(f2)
        out["sum_w2"].append(sw2)
        out["b_sum_w2"].append(gamma(nc + 2))
        out["b_f2"].append(gamma(nc + 12))
        out["b_wout"].append(gamma(nc + 15) if mode == BRIGGS else gamma(2))
    return out


def emulate(dens, w, mode, robust=0.5, double_sum_w=True):
    """A float64 NumPy emulation of the device's arithmetic after the integers -> (wout list,
    f2 list, sum_w2 list); `double_sum_w=False` plants a mistake."""
    K = dens["idx"][0].size
    w = np.ones(K) if w is None else np.asarray(w, np.float64)
    outs, f2s, sw2s = [], [], []
    for m, W in enumerate(dens["W"]):
        sw2 = np.float64(0)
        for x in W:                                     # a plain sequential sum
            sw2 = np.float64(sw2 + x * x)
        f2 = np.float64(0)
        if mode == BRIGGS and sw2 > 0:
            f = np.float64(5.0) * np.float64(10.0) ** np.float64(-robust)
            sw = np.float64(dens["sum_w"][m])
            f2 = ((f * f) * ((2.0 if double_sum_w else 1.0) * sw)) / sw2
        idx = dens["idx"][m]
        ok = idx >= 0
        Wk = np.where(ok, W[np.where(ok, idx, 0)], 1.0)
        wl = np.where(ok, w, 0.0)
        if mode == BRIGGS:
            d = (LD(f2) * Wk.astype(LD) + LD(1)).astype(np.float64)     # the fma: one rounding
            r = wl / d
        else:
            r = np.where(Wk > 0, wl / np.where(Wk > 0, Wk, 1.0), 0.0)
        outs.append(np.where(ok, r, 0.0))
        f2s.append(float(f2))
        sw2s.append(float(sw2))
    return outs, f2s, sw2s


def worst_ratio(got, want, bound):
    """max |got - want| / (bound |want|) over the entries with want != 0; entries with
    want == 0 must be exactly 0."""
    got, want = np.asarray(got, np.float64), np.asarray(want, LD)
    zero = want == 0
    assert np.all(got[zero] == 0), "a weight that must be exactly 0 is not"
    if zero.all():
        return 0.0
    err = np.abs(got[~zero].astype(LD) - want[~zero]) / np.abs(want[~zero])
    return float(err.max() / LD(bound))


def noise_factor(wout, w):
    """sqrt(sum(w'^2 / w) sum(w)) / sum(w') over the entries with w' > 0 and w > 0."""
    wout, w = np.asarray(wout, LD), np.asarray(w, LD)
    live = (wout > 0) & (w > 0)
    return float(np.sqrt((wout[live] ** 2 / w[live]).sum() * w[live].sum()) / wout[live].sum())


# ---- the cases the CPU and the GPU tests share -------------------------------------------------------
def case(nx, nz, n_vis, n_maps, seed, amax=0.7, weights="wide", flag=0.1, ties=False):
    """Random visibilities for `n_maps` grids of nx x nz -> (su, sv, u, v, w).  |su u| and |sv v|
    reach `amax` cycles per cell (beyond 0.5: out of range).  `weights`: "wide" = 2^(+-20),
    "ones", None.  `flag`: the fraction flagged, one kind after the other (NaN u, inf v, NaN w,
    inf w, negative w).  `ties`: map 0 gets the scales (1, -1) and the first visibilities products
    that are exact half-integers, the edge |gu| = hx, the first cell beyond it, and +-0."""
    rng = np.random.default_rng(seed)
    su = rng.uniform(0.5, 2.0, n_maps) * rng.choice([-1.0, 1.0], n_maps)
    sv = rng.uniform(0.5, 2.0, n_maps) * rng.choice([-1.0, 1.0], n_maps)
    if ties:
        su[0], sv[0] = 1.0, -1.0
    u = rng.uniform(-amax, amax, n_vis) / np.abs(su).max()
    v = rng.uniform(-amax, amax, n_vis) / np.abs(sv).max()
    if ties:
        hx, hz = nx // 2, nz // 2
        planted = [((k + 0.5) / nx, (j + 0.5) / nz) for k, j in
                   ((0, 0), (1, -2), (-1, 1), (-2, -1), (2, 2), (hx - 1, -hz), (-hx, hz - 1))]
        planted += [(hx / nx, 0.0), (-hx / nx, -0.0), ((hx + 1) / nx, 0.0), (0.0, -(hz + 1) / nz),
                    (0.0, hz / nz), (0.0, 0.0), (-0.0, -0.0), (0.0, 0.0)]
        for i, (a, b) in enumerate(planted[:n_vis]):
            u[i], v[i] = a, b
    if weights is None:
        w = None
    elif weights == "ones":
        w = np.ones(n_vis)
    else:
        w = np.ldexp(rng.uniform(0.5, 1.0, n_vis), rng.integers(-20, 21, n_vis))
    n_bad = int(round(flag * n_vis))
    where = rng.permutation(np.arange(len(planted) if ties else 0, n_vis))[:n_bad]
    for i, k in enumerate(where):
        kind = i % 5
        if kind == 0:
            u[k] = np.nan
        elif kind == 1:
            v[k] = np.inf
        elif w is not None:
            w[k] = (np.nan, np.inf, -1.0)[kind - 2]
        else:
            u[k] = -np.inf
    return su, sv, u, v, w
