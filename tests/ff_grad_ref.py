"""Reference for the burst-parameter sensitivities (rjp_ff_grad, K7): a NumPy restatement in
numpy.longdouble (math.fsum over float64 terms where long double is no wider), from the host
arrays (a0, ts) the device holds, in the style of gpu_util._ref_slab.  Shares nothing with the
kernels: numpy.exp, plain sums.

For the bursts b of a cell's jet (jet = sign bit of a0), d = t - ts, G_b = exp(-(d - t0_b)^2 k_b),
k_b = inv2s2_b, chi = 1 + sum_b amp_b G_b:
    S          = sum_y |a0| chi^2
    dS/dt0_b   = sum_y |a0| 2 chi amp_b G_b 2 k_b (d - t0_b)
    dS/damp_b  = sum_y |a0| 2 chi G_b
    dS/dk_b    = sum_y |a0| 2 chi amp_b G_b (-(d - t0_b)^2)
Plane k = 3 b + c, b counting the red jet's bursts first, then the blue jet's; c = 0 t0, 1 amp_rel,
2 inv2s2.  Rules: a term that is NaN is skipped (nansum); the cells of a jet WITHOUT bursts have
chi = 1 whatever their launch time (they add |a0| to S and nothing to any derivative); a Gaussian
below 2^-1021 counts as zero (the smallest the library's exp2 forms).

Bursts are per-jet lists [(t0_s, amp_rel, sigma_s), ...] for (red, blue), what engine.make_bursts
takes; inv2s2 = 1 / (2 sigma^2) is formed in float64 exactly as make_bursts forms it."""
import math

import numpy as np

LD = np.longdouble
# the synthetic cases tests/test_gpu_ff_grad.py holds to the non-vacuity condition
SEED = 20261018
EPOCHS_YR = (0.8, 1.3, 2.5)
COVER_SHAPES = ((3, 37, 50), (5, 19, 33))
MIN_COVER = 0.4
WIDE = np.finfo(LD).eps < np.finfo(np.float64).eps
G_FLOOR = 2.0 ** -1021
EPS = 2.0 ** -53


def kernel_params(bursts):
    """[(jet, t0, amp_rel, inv2s2)] in plane order (red first), float64 as make_bursts hands over."""
    out = []
    for j in range(2):
        for t0, amp, sg in bursts[j]:
            out.append((j, float(t0), float(amp), 1.0 / (2.0 * float(sg) ** 2.0)))
    return out


def _colsum(term):
    """nansum over axis 1 of [n_x, n_y, n_z] terms -> float64 [n_x, n_z] (and the same of |term|)."""
    term = np.where(np.isnan(term), 0, term)
    if WIDE:
        return (np.add.reduce(term, axis=1, dtype=LD), np.add.reduce(np.abs(term), axis=1, dtype=LD))
    t64 = term.astype(np.float64)
    s = np.empty((term.shape[0], term.shape[2]))
    a = np.empty_like(s)
    for i in range(term.shape[0]):
        for k in range(term.shape[2]):
            s[i, k] = math.fsum(t64[i, :, k])
            a[i, k] = math.fsum(np.abs(t64[i, :, k]))
    return s, a


def planes(a0, ts, bursts, t_epoch):
    """-> dict(S, absS: [n_x, n_z]; D, absD: [n_par, n_x, n_z]) in the working precision (long
    double where wider): the sums and, per plane, the sums of the absolute terms."""
    a0 = np.asarray(a0, dtype=np.float64)
    ts = np.asarray(ts, dtype=np.float64)
    T = LD if WIDE else np.float64
    red = np.signbit(a0)
    w = np.abs(a0).astype(T)
    par = kernel_params(bursts)
    with np.errstate(all="ignore"):
        d = T(t_epoch) - ts.astype(T)
        chi = np.ones(a0.shape, dtype=T)
        G = []
        for j, t0, amp, k in par:
            mask = red if j == 0 else ~red
            dd = d - T(t0)
            g = np.exp(-(dd * dd) * T(k))
            g = np.where(g < G_FLOOR, 0, g)
            g = np.where(mask, g, 0)                     # (NaN launch times stay NaN inside the jet)
            G.append((dd, g))
            chi = chi + T(amp) * g
        # a jet without bursts: chi == 1 whatever the launch time (no Gaussian touched its cells)
        S, absS = _colsum(w * chi * chi)
        npar = 3 * len(par)
        D = np.zeros((npar,) + S.shape, dtype=T)
        absD = np.zeros_like(D)
        for b, ((j, t0, amp, k), (dd, g)) in enumerate(zip(par, G)):
            mask = red if j == 0 else ~red
            base = w * 2 * chi * g
            terms = (base * T(amp) * 2 * T(k) * dd, base, base * T(amp) * (-(dd * dd)))
            for c, term in enumerate(terms):
                term = np.where(mask, term, 0)           # only the cells of burst b's jet
                D[3 * b + c], absD[3 * b + c] = _colsum(term)
    return dict(S=S, absS=absS, D=D, absD=absD)


def totals(ref, tavg, ctau, cflux):
    """The totals stage from reference planes (one epoch): -> dict(F[f], absF[f], dF[f, k],
    absdF[f, k], tau_max) float64; absdF = sum_p |weight| sum_y |term|.  A NaN tavg pixel is
    skipped."""
    T = LD if WIDE else np.float64
    S = ref["S"].ravel().astype(T)
    D = ref["D"].reshape(ref["D"].shape[0], -1).astype(T)
    aD = ref["absD"].reshape(D.shape).astype(T)
    ta = np.asarray(tavg, dtype=np.float64).ravel()
    ta = np.where(np.isnan(ta), 0, ta).astype(T)
    nf, npar = len(ctau), D.shape[0]
    out = dict(F=np.zeros(nf), absF=np.zeros(nf), dF=np.zeros((nf, npar)),
               absdF=np.zeros((nf, npar)), tau_max=0.0)
    for f in range(nf):
        tau = T(ctau[f]) * S
        flux = T(cflux[f]) * ta * (-np.expm1(-tau))
        wgt = T(cflux[f]) * ta * T(ctau[f]) * np.exp(-tau)
        out["F"][f] = float(flux.sum(dtype=T))
        out["absF"][f] = float(np.abs(flux).sum(dtype=T))
        out["dF"][f] = (wgt[None, :] * D).sum(axis=1, dtype=T).astype(np.float64)
        out["absdF"][f] = (np.abs(wgt)[None, :] * aD).sum(axis=1, dtype=T).astype(np.float64)
        live = ta != 0
        if live.any():
            out["tau_max"] = max(out["tau_max"], float(tau[live].max()))
    return out


def map_bound(ny, gauss_rtol):
    """|got - ref| <= this * sum_y |term| per pixel: the project's figure for scans that keep the
    Gaussians plus the worst-case rounding of an f64 sum of n_y terms."""
    return gauss_rtol + ny * EPS


def totals_bound(ny, npix, tau_max, gauss_rtol):
    """... and for the totals: the weight e^-tau carries tau times the relative error of S."""
    return gauss_rtol * (1.0 + tau_max) + (ny + npix) * EPS


def chain_rule(t_0, peak_jml, half_life, ss_jml):
    """(t_0 [s], peak_jml [kg/s], half_life [s]) -> the kernel parameters (t0, amp_rel, inv2s2),
    restated from the reference: sigma = half_life 2 / (2 sqrt(2 ln 2)) (classes.py:442-448)."""
    sigma = half_life * 2. / (2. * math.sqrt(2. * math.log(2.)))
    return t_0, (peak_jml - ss_jml) / ss_jml, 1. / (2. * sigma * sigma)


def coverage(plane):
    """Share of the sightlines on which |plane| exceeds 1e-6 of its own maximum."""
    a = np.abs(np.asarray(plane, dtype=np.float64)).ravel()
    m = a.max()
    return float(np.mean(a > 1e-6 * m)) if m > 0 else 0.0


# ---- the synthetic test fields -------------------------------------------------------------------
def synth_a0_ts(shape, seed, flags="halves"):
    """(a0, ts) [n_x, n_y, n_z] from gpu_util.synth_host with a temperature spread; `flags`:
    "halves" = the generator's own (red where i_z < n_z / 2: waves all red, all blue and, where a
    wave crosses n_z / 2 or a row end, straddling), "cells" = a random jet per CELL (every
    sightline holds both jets, every wave straddles), "red" / "blue" = one jet everywhere."""
    from tests import gpu_util as U
    g = U.synth_host(shape, seed, 1)
    a0 = np.abs(U.golden_a0(g, 0.))
    if flags == "halves":
        red = g["rr"] < 0
    elif flags == "cells":
        red = np.random.default_rng(seed).random(shape) < 0.5
    else:
        red = np.full(shape, flags == "red")
    return np.where(red, -a0, a0), g["ts"].copy()
