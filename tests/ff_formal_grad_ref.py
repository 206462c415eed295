"""Reference for the burst-parameter sensitivities of the formal-solution light curves
(rjp_ff_formal_grad, K9): a NumPy restatement in numpy.longdouble (compensated float64 sums where
long double is no wider), from the host arrays the device holds -- a0 with the jet flag in its sign
bit, ts, temp -- with numpy.exp / numpy.expm1 and a plain loop over y, vectorised over the pixels.
Shares nothing with the kernels.

One sightline, cells i from the observer side (iy = 0) back, one channel with c = ctau[f]:
    b_i = |a0_i| chi_i^2     dtau_i = c b_i     om_i = 1 - e^-dtau_i     Theta_i = exp(-sum_{j<i} dtau_j)
    I   = sum_i T_i om_i Theta_i
    g_ik = db_i/dtheta_k, for the bursts of cell i's jet only (d = t - ts, G = exp(-(d - t0)^2 k)):
           |a0| 2 chi amp G 2 k (d - t0),   |a0| 2 chi G,   |a0| 2 chi amp G (-(d - t0)^2)
    D_ik = sum_{j<i} g_jk
    dI/dtheta_k = sum_i c T_i Theta_i [ e^-dtau_i g_ik - om_i D_ik ]
    abs_k       = sum_i c T_i Theta_i [ e^-dtau_i |g_ik| + om_i sum_{j<i} |g_jk| ]
Plane k = 3 b + c, b counting the red jet's bursts first, then the blue jet's; c = 0 t0, 1 amp_rel,
2 inv2s2.  Rules (K8's and K7's): a NaN a0, or a NaN launch time in a jet that has bursts, drops the
cell; the cells of a jet WITHOUT bursts have chi = 1 whatever their launch time (g = 0, they still
attenuate); a dead cell (b = 0) emits nothing; a Gaussian below 2^-1021 counts as zero; a sightline
without a cell of T > 0 is NaN in every map and adds nothing to a total.  Theta is formed from the
summed optical depth, not as a running product.

THE BOUND, term by term.  b and g carry GAUSS_RTOL = 3e-12 (the degree-8 exp2 of the Gaussians,
gpu_util), so every bracket term carries it once through g, once more through e^-dtau / om (d om =
e^-dtau dtau rel(b) <= rel(b) om-or-e^-dtau-sized for the terms they multiply), and Theta_i carries
it multiplied by the optical depth in front, at most tau_sightline: 3e-12 (2 + tau).  Each of the
n_y updates adds the error of 1 - e^-dtau / e^-dtau (4e-15, one_minus_exp_neg) to the attenuation
and four roundings (the two products of the weight, two FMAs) to the sum:
    |got - ref| <= [ 3e-12 (2 + tau_sightline) + n_y (4e-15 + 4 2^-53) ] abs_k       per pixel, plane
    totals: the sum of the per-pixel bounds + P 2^-53 sum_p abs_k                    (P - 1 additions)
The same expression with abs = I (all its terms are >= 0) bounds F.
Underflow.  The outputs are float64: behind a thick cell abs_k itself can lie below the smallest
normal double (a plane whose first cell with g != 0 sits behind tau > 700), where no float64 result
can carry a relative error.  A float64 product below 2^-1022 is rounded to a multiple of 2^-1074:
the running attenuation loses at most 2^-1075 per update, n_y 2^-1075 in all, its product with
c T one rounding more, the weights e^-dtau / om times that one more, and each multiplies |g_ik| or
sum_{j<i} |g_jk| <= sum_i |g_ik|:
    floor_k = 2^-1074 [ n_y (n_y c T_max + 2) csrc sum_i |g_ik| + 1 ]     (0 where every g_ik is 0)
is added to the bound.  It is below 1e-280 in every test and matters only where abs_k has left the
normal range.

Bursts are per-jet lists [(t0_s, amp_rel, sigma_s), ...] for (red, blue), what engine.make_bursts
takes; inv2s2 = 1 / (2 sigma^2) is formed in float64 exactly as make_bursts forms it."""
import numpy as np

LD = np.longdouble
WIDE = np.finfo(LD).eps < np.finfo(np.float64).eps
G_FLOOR = 2.0 ** -1021
EPS = 2.0 ** -53
GAUSS_RTOL = 3e-12
OM_RTOL = 4e-15
YEAR = 31536000.0
SHAPES = ((3, 37, 50), (5, 19, 33))


def kernel_params(bursts):
    """[(jet, t0, amp_rel, inv2s2)] in plane order (red first), float64 as make_bursts hands over."""
    return [(j, float(t0), float(amp), 1.0 / (2.0 * float(sg) ** 2.0))
            for j in range(2) for t0, amp, sg in bursts[j]]


class _Sum:
    """Running sum of arrays: long double where it is wider, else float64 with Neumaier's
    compensation (the fsum of a running sum)."""

    def __init__(self, shape):
        self.s = np.zeros(shape, dtype=LD if WIDE else np.float64)
        self.c = None if WIDE else np.zeros(shape)

    def add(self, x):
        if WIDE:
            self.s = self.s + x
            return
        t = self.s + x
        big = np.abs(self.s) >= np.abs(x)
        self.c += np.where(big, (self.s - t) + x, (x - t) + self.s)
        self.s = t

    def value(self):
        return self.s if WIDE else self.s + self.c


def cells(a0, ts, bursts, t_epoch):
    """Per cell: b [n_x, n_y, n_z] (0 for a dropped cell) and g [n_par, n_x, n_y, n_z], in the
    working precision."""
    T = LD if WIDE else np.float64
    a0 = np.asarray(a0, dtype=np.float64)
    ts = np.asarray(ts, dtype=np.float64)
    red = np.signbit(a0)
    w = np.abs(a0).astype(T)
    par = kernel_params(bursts)
    has = [any(p[0] == j for p in par) for j in range(2)]
    with np.errstate(all="ignore"):
        d = T(t_epoch) - ts.astype(T)
        chi = np.ones(a0.shape, dtype=T)
        G = []
        for j, t0, amp, k in par:
            mask = red if j == 0 else ~red
            dd = d - T(t0)
            g = np.exp(-(dd * dd) * T(k))
            g = np.where(g < G_FLOOR, 0, g)
            g = np.where(mask, g, 0)                   # (a NaN launch time stays NaN inside the jet)
            G.append((mask, dd, g))
            chi = chi + T(amp) * g
        b = w * chi * chi
        drop = np.isnan(b)                             # NaN a0, or NaN ts in a jet with bursts
        b = np.where(drop, 0, b)
        gs = np.zeros((3 * len(par),) + a0.shape, dtype=T)
        for i, ((j, t0, amp, k), (mask, dd, g)) in enumerate(zip(par, G)):
            base = w * 2 * chi * g
            terms = (base * T(amp) * 2 * T(k) * dd, base, base * T(amp) * (-(dd * dd)))
            for c, term in enumerate(terms):
                gs[3 * i + c] = np.where(mask & ~drop, term, 0)
    assert has[0] or has[1] or not par
    return b, gs


def walk(a0, ts, temp, bursts, t_epoch, ctau, csrc):
    """-> dict: I [F, n_x, n_z], dI and abs [F, n_par, n_x, n_z] (csrc included; NaN where the
    sightline has no T > 0), tau [F, n_x, n_z] (the sightline's optical depth), hot [n_x, n_z];
    working precision."""
    T = LD if WIDE else np.float64
    b, gs = cells(a0, ts, bursts, t_epoch)
    temp = np.asarray(temp, dtype=np.float64)
    nx, ny, nz = b.shape
    npar, F = gs.shape[0], len(ctau)
    c = np.asarray(ctau, dtype=np.float64).astype(T)[:, None, None]
    I, tau = _Sum((F, nx, nz)), _Sum((F, nx, nz))
    dI, ab = _Sum((F, npar, nx, nz)), _Sum((F, npar, nx, nz))
    D, Da = _Sum((npar, nx, nz)), _Sum((npar, nx, nz))
    with np.errstate(all="ignore"):
        for y in range(ny):
            by = b[:, y, :]
            tk = np.where(by != 0, temp[:, y, :], 0).astype(T)
            dt = c * by[None]
            ex, om = np.exp(-dt), -np.expm1(-dt)
            th = np.exp(-tau.value())
            I.add(tk[None] * om * th)
            wgt = (c * tk[None] * th)[:, None]                     # [F, 1, n_x, n_z]
            g = gs[:, :, y, :][None]
            dI.add(wgt * (ex[:, None] * g - om[:, None] * D.value()[None]))
            ab.add(wgt * (ex[:, None] * np.abs(g) + om[:, None] * Da.value()[None]))
            D.add(gs[:, :, y, :])
            Da.add(np.abs(gs[:, :, y, :]))
            tau.add(dt)
    hot = np.any(temp > 0.0, axis=1)
    cs = np.asarray(csrc, dtype=np.float64).astype(T)
    nan = T(np.nan)
    out = dict(hot=hot, tau=tau.value())
    with np.errstate(all="ignore"):
        tmax = np.nanmax(np.where(temp > 0, temp, 0.0))
        sg = (np.abs(cs)[:, None, None, None] * Da.value()[None]).astype(np.float64)
        fl = 2.0 ** -1074 * (ny * (ny * np.asarray(ctau, dtype=np.float64)[:, None, None, None] *
                                   tmax + 2.0) * sg + 1.0)
    out["floor"] = np.where(sg > 0, fl, 0.0)
    out["I"] = np.where(hot[None], cs[:, None, None] * I.value(), nan)
    out["dI"] = np.where(hot[None, None], cs[:, None, None, None] * dI.value(), nan)
    out["abs"] = np.where(hot[None, None], np.abs(cs)[:, None, None, None] * ab.value(), nan)
    return out


def pixel_bound(tau, ny):
    """The factor of abs_k in the per-pixel bound, from the sightline's optical depth."""
    return GAUSS_RTOL * (2.0 + np.asarray(tau, dtype=np.float64)) + ny * (OM_RTOL + 4.0 * EPS)


def totals(res, ny):
    """Totals of one epoch from walk(): F, dF and their own absolute sums, and the bounds on
    |got - ref| (the sum of the per-pixel bounds + P 2^-53 x the absolute sum), float64."""
    T = LD if WIDE else np.float64
    hot = res["hot"]
    P = hot.size
    bf = pixel_bound(res["tau"], ny).astype(T)                     # [F, n_x, n_z]
    z = lambda a: np.where(np.isnan(a), 0, a)
    I, dI, ab = z(res["I"]), z(res["dI"]), z(res["abs"])
    bfh = np.where(hot[None], bf, 0)
    s = lambda a: np.asarray(a.sum(axis=(-2, -1), dtype=T), dtype=np.float64)
    return dict(F=s(I), absF=s(np.abs(I)), dF=s(dI), absdF=s(ab),
                floordF=s(np.where(hot[None, None], res["floor"], 0.0)),
                boundF=s(bfh * np.abs(I)) + P * EPS * s(np.abs(I)),
                bounddF=s(bfh[:, None] * ab) + P * EPS * s(ab))


# ---- float64 emulation of the recurrence a kernel may run (tests of the bound's own power) -------
def emulate(a0, ts, temp, bursts, t_epoch, ctau, csrc, mistake=None):
    """The forward recurrence in plain float64, one update per cell as a kernel would run it:
    dI_k += c T A (e^-dtau g_k - om D_k), D_k += g_k, A *= e^-dtau.  `mistake`: "no_hide" drops the
    -om D term, "late_theta" uses the attenuation after its update.  -> dI [F, n_par, n_x, n_z]."""
    b, gs = cells(a0, ts, bursts, t_epoch)
    b, gs = b.astype(np.float64), gs.astype(np.float64)
    temp = np.asarray(temp, dtype=np.float64)
    nx, ny, nz = b.shape
    npar, F = gs.shape[0], len(ctau)
    c = np.asarray(ctau, dtype=np.float64)[:, None, None]
    A = np.ones((F, nx, nz))
    dI = np.zeros((F, npar, nx, nz))
    D = np.zeros((npar, nx, nz))
    with np.errstate(all="ignore"):
        for y in range(ny):
            by = b[:, y, :]
            tk = np.where(by != 0, temp[:, y, :], 0.0)
            dt = c * by[None]
            ex, om = np.exp(-dt), -np.expm1(-dt)
            att = A * ex if mistake == "late_theta" else A
            wgt = (c * tk[None] * att)[:, None]
            g = gs[:, :, y, :][None]
            hide = 0.0 if mistake == "no_hide" else om[:, None] * D[None]
            dI += wgt * (ex[:, None] * g - hide)
            D += gs[:, :, y, :]
            A = A * ex
    hot = np.any(temp > 0.0, axis=1)
    return np.where(hot[None, None], np.asarray(csrc)[:, None, None, None] * dI, np.nan)


def worst_ratio(got, ref, absref, bound, floor=0.0):
    """max |got - ref| / (bound abs + floor) over the entries where that is > 0 (the others must be
    equal); NaN patterns must agree.  `bound` and `floor` broadcast against `absref`."""
    got = np.asarray(got, dtype=np.float64)
    ref, absref = np.asarray(ref), np.asarray(absref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    err = np.abs(np.where(nan, 0, got).astype(LD) - np.where(nan, 0, ref).astype(LD))
    lim = (np.asarray(bound) * np.where(nan, 0, absref)).astype(LD) + np.asarray(floor)
    pos = lim > 0
    assert np.all(err[~pos] == 0), "a plane differs where the reference's terms are all zero"
    return float((err[pos] / lim[pos]).max()) if pos.any() else 0.0


# ---- the synthetic cases (tests/test_gpu_ff_formal_grad.py; their non-vacuity is held on the CPU)
def synth_fields(shape, seed, narrow=False):
    """Host grids for engine.upload_fields: gpu_util.synth_host with a temperature spread, the jet
    by z-range (first quarter red, last quarter blue, a random jet per CELL between: sightlines of
    one jet and sightlines that hold both), NaN and zero cells, a sparse row, an empty sightline,
    NaN launch times.  `narrow`: the densities' 2.5 decades compressed to 0.4 (sightlines of
    similar optical depth, for the thick case)."""
    from tests import gpu_util as U
    g = U.synth_host(shape, seed, 1)
    if narrow:
        g["nd"] = 1e6 * (g["nd"] / 1e6) ** 0.16
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    iz = np.arange(nz)[None, None, :]
    red = np.where(iz < nz // 4, True, np.where(iz >= nz - nz // 4, False, rng.random(shape) < 0.5))
    g["rr"] = np.where(red, -1.0, 1.0)
    for k, vals in (("nd", [np.nan, 0.0]), ("xi", [np.nan]), ("temp", [np.nan]),
                    ("ff", [np.nan, 0.0]), ("ts", [np.nan])):
        m = rng.random(shape) < 0.03
        g[k] = np.where(m, rng.choice(vals, size=shape), g[k])
    lo, hi = ny // 6, ny - ny // 5                       # empty rows at either end of every sightline
    for k in ("nd", "temp"):
        g[k][:, :lo, :] = np.nan
        g[k][:, hi:, :] = np.nan
    keep = rng.random((ny, nz)) < 0.15                   # a sparse x-row
    g["nd"][nx - 1] = np.where(keep, g["nd"][nx - 1], np.nan)
    g["nd"][0, :, 0] = np.nan                            # an empty sightline
    g["temp"][0, :, 0] = np.nan
    return g


def host_a0(g):
    """The tau field (scalar Gaunt factor) of synth_fields' grids in NumPy, jet flag in the sign."""
    from tests import gpu_util as U
    return U.golden_a0(g, 0.0)


def column(a0):
    """sum_y |a0| per sightline (the optical depth per unit ctau at chi = 1), NaN cells skipped."""
    return np.nansum(np.abs(a0), axis=1)


def channel_tables(a0, F, tau_mid=(0.1, 5.0), col=None):
    """(ctau, csrc) for F channels whose MEDIAN live sightline has tau from tau_mid[0] to
    tau_mid[1] -- at chi = 1, or with `col` = sum_y b per sightline at some epoch."""
    col = column(a0) if col is None else np.asarray(col, dtype=np.float64)
    med = float(np.median(col[col > 0]))
    tau = np.geomspace(tau_mid[0], tau_mid[1], F) if F > 1 else np.array([np.sqrt(tau_mid[0] * tau_mid[1])])
    return tau / med, 1e-3 * (1.0 + np.arange(F))


def epochs(seed, E):
    """Unsorted epochs [s] over the bursts' span, one far outside every burst's support and one
    duplicate (where E leaves room for them)."""
    t = np.random.default_rng(seed).uniform(-0.5, 6.0, E) * YEAR
    if E >= 3:
        t[1] = 500.0 * YEAR
        t[-1] = t[0]
    return [float(v) for v in t]


def _example():
    from tests import gpu_util as U
    return U.example_burst_lists()


def burst_set(name):
    ex = _example()
    if name == "one-red":                                 # (1, 0): chi = 1 in the blue jet
        return [ex[0][0]], []
    if name == "example":                                 # (2, 3)
        return ex
    if name == "dip":                                     # the example with a -0.6 dip
        return [ex[0][0], (ex[0][1][0], -0.6, ex[0][1][2])], ex[1]
    if name == "blue4":                                   # (0, 4)
        return [], ex[1] + [(1.6 * YEAR, 3.0, 0.3 * YEAR)]
    assert name == "full"                                 # (8, 8)
    rng = np.random.default_rng(88)
    mk = lambda: [(rng.uniform(0.0, 3.5) * YEAR, rng.uniform(0.5, 8.0), rng.uniform(0.15, 0.7) * YEAR)
                  for _ in range(8)]
    return mk(), mk()


# name: (shape, seed, E, F, burst set, y-bounds attached).  Axes spread over the cases: E covers
# both lane layouts, their tails and a 64-lane block followed by a 16-lane one; F the register
# blocks (1, 2, 4) and their overflow; (8, 8) the tail of every parameter block.
CASES = {
    "one-red-E1-F1": (SHAPES[0], 9101, 1, 1, "one-red", False),
    "one-red-E64-F1": (SHAPES[1], 9109, 64, 1, "one-red", True),
    "example-E15-F2": (SHAPES[1], 9102, 15, 2, "example", True),
    "example-E17-F5": (SHAPES[0], 9103, 17, 5, "example", False),
    "full-E17-F1": (SHAPES[1], 9104, 17, 1, "full", False),
    "full-E65-F3": (SHAPES[1], 9105, 65, 3, "full", True),
    "dip-E64-F2": (SHAPES[0], 9106, 64, 2, "dip", False),
    "blue4-E65-F1": (SHAPES[0], 9107, 65, 1, "blue4", True),
}
THICK = ("example-thick", SHAPES[0], 9108, 17, 2, "example")
THICK_TAU = (600.0, 1000.0)     # tau of the median sightline at chi = 1, per channel (more inside a burst)
MIN_SHARE = 0.4
