"""Long-double NumPy reference of the isothermal recombination-line map stage (rjp_rrl_maps:
rrl_maps_kernel + sum_partials_kernel), its error bound, the input sets, and a float64 emulation
of the kernel.  Shared by tests/test_rrl_maps_reference_cpu.py (which pins the reference against
50 digits, proves the inputs feasible and shows which input catches which mistake) and
tests/test_gpu_rrl_maps.py (which holds the kernel to it).  Tests only; nothing here imports the
original project.

The quantity, per channel f and pixel p:
    x    = hnu_k[f] / tavg[p]
    line = cflux[f] / expm1(x) * exp(-tau_ff[f, p]) * (1 - exp(-tau_rrl[f, p]))
    flux = line + flux_ff[f, p]   (where a continuum is given)
    ftot[f] = nansum_p flux[f, p]

The bound on one pixel, u = 2^-53 (one rounding to nearest in float64):
    u |line| (kappa(x) + C0) + u |line + flux_ff| + floor

  kappa(x) = x / (1 - e^-x): the one rounding of the quotient hnu_k / tavg (relative error u in
      x) through expm1, whose relative condition number is x e^x / (e^x - 1).
  C0, the roundings of the factors of `line`, in units of u, one line per term.  An error of
  1 ulp is at most 2^-52 = 2 u relative.
      2      expm1: 1 ulp.  HIP's documentation of the double-precision device math functions
             ("HIP math API", table of maximum ULP differences) lists expm1 at 1.
      1      the reciprocal 1.0 / expm1(x): the library is built with -O3 and no fast-math flag
             (rajepy_amd/csrc/Makefile), so the f64 division is IEEE, correctly rounded: 1/2 ulp.
      2      exp: 1 ulp, same table.  Its argument -tau_ff is exact (a sign flip).
      36.03  one_minus_exp_neg: 4e-15 relative for every tau, the figure rjp_device.h states and
             tests/sweep_ref.py budgets for the map stages; 4e-15 / u.
      3      the three products cflux * bnu * e * om, each correctly rounded: 1/2 ulp each.
      -----
      44.03
  u |line + flux_ff|: the one addition of the continuum; absent where no continuum is given
      (nothing is added then, and the bound is the narrower for it).
  floor = TINY (2 + |cflux / expm1(x)| (1 - e^-tau_rrl)), TINY = 2^-1074 the smallest subnormal:
      below the normal range a rounding is absolute, not relative.  Where e^-tau_ff itself is
      subnormal (tau_ff > 708) the library's 1 ulp is one TINY on e, and the line carries it
      times the factors e is multiplied by; the two products after it add 1/2 TINY each when
      their results are subnormal.  The addition of the continuum is exact there.

The bound on a total:  sum_p bound_p + D u sum_p |flux_p|,  D the number of additions a term can
pass through, read from the two kernels (workgroups of 256 lanes = 4 waves of 64 in both):
      6   shuffle levels of the wave reduction in rrl_maps_kernel
      4   lane 0 adding the four per-wave partials of its workgroup (to a 0.0)
      ceil(nblk / 256)   sum_partials_kernel's strided loop over the nblk workgroup partials
      6   its shuffle levels
      4   its four per-wave partials
  so D = 20 + ceil(nblk / 256), nblk = ceil(P / 256).  NaN pixels add nothing (nansum).

No figure above comes from what the device returns."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TINY = 2.0 ** -1074
C0 = 2.0 + 1.0 + 2.0 + 4e-15 / U + 3.0
BLOCK, WAVE = 256, 64

# h / k [K / Hz] (CODATA 2018, both exact by definition), for the radio-band channels
H_OVER_K = 6.62607015e-34 / 1.380649e-23


def _ld(a):
    return None if a is None else np.asarray(a, dtype=LD)


def _parts(tau_rrl, tau_ff, tavg, cflux, hnu_k):
    tau_rrl, tau_ff, tavg = _ld(tau_rrl), _ld(tau_ff), _ld(tavg)
    cflux, hnu_k = _ld(cflux)[:, None], _ld(hnu_k)[:, None]
    with np.errstate(all="ignore"):
        x = hnu_k / tavg[None, :]
        pre = cflux / np.expm1(x) * -np.expm1(-tau_rrl)       # all but e^-tau_ff
        line = cflux / np.expm1(x) * np.exp(-tau_ff) * -np.expm1(-tau_rrl)
    return x, pre, line


def flux_ref(tau_rrl, tau_ff, tavg, flux_ff, cflux, hnu_k):
    """-> flux[F, P] in long double; NaN where tavg is NaN, or flux_ff where it is given."""
    _, _, line = _parts(tau_rrl, tau_ff, tavg, cflux, hnu_k)
    return line if flux_ff is None else line + _ld(flux_ff)


def flux_bound(tau_rrl, tau_ff, tavg, flux_ff, cflux, hnu_k):
    """-> the absolute bound [F, P] of the header, long double (NaN where the reference is)."""
    x, pre, line = _parts(tau_rrl, tau_ff, tavg, cflux, hnu_k)
    with np.errstate(all="ignore"):
        kappa = x / -np.expm1(-x)
        b = U * np.abs(line) * (kappa + C0) + LD(TINY) * (2.0 + np.abs(pre))
        if flux_ff is not None:
            b = b + U * np.abs(line + _ld(flux_ff))
    return b


def n_additions(P):
    nblk = (P + BLOCK - 1) // BLOCK
    return 20 + (nblk + BLOCK - 1) // BLOCK


def ftot_ref(flux):
    return np.nansum(_ld(flux), axis=1)


def ftot_bound(flux, bound):
    """flux, bound [F, P]: the reference and its per-pixel bound -> [F]."""
    P = flux.shape[1]
    return np.nansum(_ld(bound), axis=1) + n_additions(P) * U * np.nansum(np.abs(_ld(flux)), axis=1)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound; inf unless the NaN patterns are identical and, where the bound is
    0, the values equal."""
    got, ref, bound = _ld(got), _ld(ref), _ld(bound)
    assert got.shape == ref.shape == bound.shape
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return np.inf
    ok = ~nan
    if not ok.any():
        return 0.0
    with np.errstate(all="ignore"):
        err = np.abs(got[ok] - ref[ok])
        b = bound[ok]
        if np.isnan(err).any() or np.isnan(b).any() or np.any((b == 0) & (err != 0)):
            return np.inf
        return float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), 0.0)))


# ---- the input sets ---------------------------------------------------------------------------
TAIL_SHAPES = [(1, 1), (63, 2), (64, 1), (255, 17), (256, 2), (257, 3), (4097, 5),
               (256 * 257 + 1, 2)]                           # the last: nblk = 258 > 256

# planted at these pixels of every channel, where the pixel exists and is not P - 1 (which holds
# the channel's largest value)
PLANTS = [("tau_rrl", 0, 0.0), ("tau_rrl", 1, 1e-300), ("tau_rrl", 2, 800.0),
          ("tau_rrl", 3, 1e4), ("tau_rrl", 5, np.inf),
          ("tau_ff", 8, 0.0), ("tau_ff", 13, 745.0), ("tau_ff", 21, 1e4),
          ("tavg", 34, np.nan), ("flux_ff", 55, np.nan)]


def pixel_of(name, value, P):
    """The pixel a planted value sits at, or None where P is too small for it."""
    for n, px, v in PLANTS:
        if n == name and (v == value or (v != v and value != value)):
            return px if px < P - 1 else None
    raise KeyError((name, value))


def _logu(rng, lo, hi, shape):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), shape))


def tail_case(P, F, with_ff):
    """Log-uniform inputs of one (P, F) of TAIL_SHAPES with the edge values planted -> dict of
    float64 arrays (flux_ff None without the continuum).  Deterministic."""
    rng = np.random.default_rng(1000003 * P + 101 * F + int(with_ff))
    c = dict(tau_rrl=_logu(rng, 1e-12, 300.0, (F, P)), tau_ff=_logu(rng, 1e-9, 600.0, (F, P)),
             tavg=_logu(rng, 3.0, 3e4, P), hnu_k=_logu(rng, 1e-3, 15.0, F),
             cflux=1e-6 * np.cumprod(rng.uniform(2.0, 4.0, F)),
             flux_ff=_logu(rng, 1e-8, 1e3, (F, P)) if with_ff else None)
    for name, px, v in PLANTS:
        if px < P - 1 and c[name] is not None:
            c[name][..., px] = v
    px = pixel_of("flux_ff", np.nan, P)
    if px is not None:                      # the NaN continuum lies over a line that counts
        c["tau_rrl"][:, px], c["tau_ff"][:, px], c["tavg"][px] = 1.0, 1e-3, 1e4
    # the channel's largest value in the last pixel (the last lane of a partial workgroup):
    # the hottest, most transparent, optically thickest sightline, on the largest continuum
    c["tavg"][P - 1] = 3e4
    c["tau_ff"][:, P - 1] = 0.0
    c["tau_rrl"][:, P - 1] = 300.0
    if with_ff:
        c["flux_ff"][:, P - 1] = 2e3
    return c


RADIO_GHZ = (1.0, 5.0, 22.0, 50.0)


def radio_case():
    """1, 5, 22, 50 GHz against 5e3 ... 2e4 K (x from 2e-6 to 5e-4), P = 4097; the four quarters
    of the map are thin / thick in the line x thin / thick in the continuum.  No continuum
    added: the line alone shows the Planck factor."""
    P = 4097
    rng = np.random.default_rng(20251020)
    nu = np.array(RADIO_GHZ) * 1e9
    q = np.arange(P) * 4 // P
    thin_l, thin_c = (q % 2 == 0), (q < 2)
    tau_rrl = np.where(thin_l, _logu(rng, 1e-6, 1e-2, (4, P)), _logu(rng, 1.0, 30.0, (4, P)))
    tau_ff = np.where(thin_c, _logu(rng, 1e-6, 1e-2, (4, P)), _logu(rng, 1.0, 30.0, (4, P)))
    return dict(tau_rrl=tau_rrl, tau_ff=tau_ff, tavg=_logu(rng, 5e3, 2e4, P), flux_ff=None,
                hnu_k=H_OVER_K * nu, cflux=1e-9 * (nu / 1e9) ** 3)


def args_of(c):
    return (c["tau_rrl"], c["tau_ff"], c["tavg"], c["flux_ff"], c["cflux"], c["hnu_k"])


# ---- float64 emulation of the kernels ------------------------------------------------------------
def _tree(v):
    """Lane 0 of the shuffle-down reduction over the last axis (64 lanes)."""
    v = v.copy()
    d = WAVE // 2
    while d > 0:
        v[..., :d] = v[..., :d] + v[..., d:2 * d]
        d //= 2
    return v[..., 0]


def _block_sum(v):
    """v [..., 256] -> [...]: four wave reductions, then lane 0 adds the four partials in order."""
    w = _tree(v.reshape(v.shape[:-1] + (BLOCK // WAVE, WAVE)))
    tot = np.zeros(w.shape[:-1])
    for k in range(BLOCK // WAVE):
        tot = tot + w[..., k]
    return tot


def emulate(c, mistake=None):
    """rrl_maps_kernel + sum_partials_kernel in float64, the same operations in the same order
    (Planck through expm1, the line as -expm1(-tau)).  `mistake`: one of MISTAKES planted.
    libm's expm1 is good to 1 ulp where the kernel's one_minus_exp_neg spends most of its
    4e-15 (its polynomial and reduction alone come to 3.4e-15 near tau = 0.1 when evaluated in
    long double), so the emulation sits near 0.1 of the line's bound and the kernel near 0.7.
    -> flux[F, P], ftot[F]."""
    tau_rrl, tau_ff, tavg, flux_ff, cflux, hnu_k = (
        None if a is None else np.asarray(a, dtype=np.float64) for a in args_of(c))
    F, P = tau_rrl.shape
    fi = np.arange(F)
    if mistake == "neighbour channel":
        fi = (fi + 1) % F
    elif mistake == "channel 0":
        fi = np.zeros(F, dtype=int)
    T = np.broadcast_to(tavg[None, :], (F, P))
    if mistake == "tavg at f * P + p":          # past the end of the map: the last value again
        T = tavg[np.minimum(np.arange(F)[:, None] * P + np.arange(P)[None, :], P - 1)]
    with np.errstate(all="ignore"):
        x = hnu_k[fi][:, None] / T
        bnu = 1.0 / ((np.exp(x) - 1.0) if mistake == "exp(x) - 1" else np.expm1(x))
        om = (1.0 - np.exp(-tau_rrl)) if mistake == "1 - exp(-tau_rrl)" else -np.expm1(-tau_rrl)
        e = np.exp(tau_ff if mistake == "exp(+tau_ff)" else -tau_ff)
        line = cflux[fi][:, None] * bnu * e * om
        s = line
        if flux_ff is not None and mistake != "continuum left out":
            s = s + flux_ff
            if mistake == "continuum twice":
                s = s + flux_ff
    v = s if mistake == "NaN into ftot" else np.where(np.isnan(s), 0.0, s)
    if mistake == "NaN continuum counted as its line":
        v = np.where(np.isnan(s), np.where(np.isnan(line), 0.0, line), s)
    nblk = (P + BLOCK - 1) // BLOCK
    pad = np.zeros((F, nblk * BLOCK))
    pad[:, :P] = v
    part = _block_sum(pad.reshape(F, nblk, BLOCK))                       # [F, nblk]
    if mistake == "last partial workgroup left out" and P % BLOCK:
        part = part[:, :nblk - 1]
    n2 = (part.shape[1] + BLOCK - 1) // BLOCK
    p2 = np.zeros((F, n2 * BLOCK))
    p2[:, :part.shape[1]] = part
    lanes = np.zeros((F, BLOCK))
    for k in range(n2):                                                   # the strided loop
        lanes = lanes + p2[:, k * BLOCK:(k + 1) * BLOCK]
    return s, _block_sum(lanes)


MISTAKES = ["exp(x) - 1", "1 - exp(-tau_rrl)", "neighbour channel", "channel 0",
            "tavg at f * P + p", "last partial workgroup left out", "NaN into ftot",
            "NaN continuum counted as its line", "continuum left out", "continuum twice",
            "exp(+tau_ff)"]


def ratios(flux, ftot, c):
    """(worst flux ratio, worst ftot ratio) of a result against the reference of case c."""
    ref = flux_ref(*args_of(c))
    bound = flux_bound(*args_of(c))
    return (worst_ratio(flux, ref, bound),
            worst_ratio(ftot, ftot_ref(ref), ftot_bound(ref, bound)))
