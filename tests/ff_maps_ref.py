"""Long-double NumPy reference of the free-free map stage (K2: rjp_ff_maps and the second half of
rjp_ff_step), its error bounds, the input sets, a host restatement of ff_maps_launch's rule and a
float64 emulation of its four launch shapes (ff_maps_kernel, ff_maps_acc_kernel with KP = 1 and
KP = 4, ff_ftot_kernel, each followed by sum_partials_kernel).  Shared by
tests/test_ff_maps_reference_cpu.py (which pins the reference against 50 digits, proves every GPU
case feasible and shows which input catches which mistake) and tests/test_gpu_ff_maps.py (which
holds the kernels to it).  Tests only; nothing here imports the original project.

The quantities, per epoch e, channel f and pixel p:
    tau  = ctau[f] * A[e, p]
    flux = cflux[f] * tavg[p] * (-expm1(-tau))
    ftot[e, f] = the sum of the flux over the pixels whose flux is not NaN
  tavg NaN: flux NaN, tau still ctau * A, nothing added to the total.  A NaN: tau NaN, flux NaN,
  nothing added.  A = +inf: tau = +inf, flux = cflux * tavg.  A = 0: tau = flux = +0.0.

The bound on one tau, u = 2^-53 (one rounding to nearest in float64), TINY = 2^-1074:
    u |tau| + TINY / 2
  one correctly rounded product; below the normal range its rounding is absolute, half a TINY.
  The long-double product of the reference rounds too, at 2^-64: 2^-11 of this bound, too much
  to ignore at a bound that a correctly rounded product reaches.  tau_ratio therefore measures
  against the EXACT product, p + e by Dekker's two-product (tau_ref, the long-double product,
  feeds the flux, where 2^-64 is 1e-5 of the bound).

The bound on one flux of the cube kernels, s = cflux * (tavg * om(t)), t the rounded tau:
    u |flux| (kappa(t) + C_OM + 2) + TINY / 2 (|cflux tavg| + |cflux| + 1)
  kappa(t) = t e^-t / (1 - e^-t) <= 1: the one rounding of t = ctau * A (relative error u)
      through 1 - e^-t, whose relative condition number it is.
  C_OM = 4e-15 / u = 36.03: one_minus_exp_neg, 4e-15 relative for every tau, the figure
      rjp_device.h states and tests/sweep_ref.py budgets.
  2: the two products tavg * om and cflux * (...), correctly rounded, u each.
  floor: below the normal range a rounding is absolute.  t subnormal: TINY / 2 on t, carried at
      slope d flux / d t <= |cflux tavg|; one_minus_exp_neg returns a subnormal t exactly (its
      r^2 term vanishes).  tavg * om subnormal: TINY / 2 times |cflux|.  The last product
      subnormal: TINY / 2.
  The reference's own roundings (three long-double operations and expm1l, about 2^-62 relative:
  1e-4 of the bound) are not added.

ff_ftot_kernel groups the product as (cflux * tavg) * om and fuses it into the accumulator:
    acc = fma(cflux * tavg, om, acc)
  ONE rounded product (w = cflux * tavg); the product w * om is exact inside the FMA, whose one
  rounding is that of the addition and is counted in D below.  Its per-term bound:
    u |flux| (kappa(t) + C_OM + 1) + TINY / 2 (|cflux tavg| + 1)
  (t subnormal as above; w subnormal: TINY / 2 times om <= 1).

The bound on a total:  sum_p bound_p + D u sum_p |flux_p|,  D the number of additions a term can
pass through, read from ff_scan.hip (workgroups of 256 lanes = 4 waves of 64 in every kernel):
    ff_maps_kernel              VEC        the lane's chain acc += s[v] from 0.0
                                6          shuffle levels of its wave reduction
    ff_maps_acc_kernel<KP>      KP * VEC   the lane's chain acc[j] += s[v], group after group
                                6          shuffle levels, once per channel and lane
    ff_ftot_kernel              4 * VEC    the lane's FMA chain over kFtotKP = 4 pixel groups
                                6          shuffle levels
    then sum_partials_kernel    ceil(nparts / 256)   its strided loop over the wave partials
                                6          its shuffle levels
                                4          lane 0 adding the four per-wave partials (to a 0.0)
  so D = chain + 16 + ceil(nparts / 256), with (VEC, KP, nparts) from launch_rule below:
    small kernel, VEC = 2, 1022 pixels:       2 + 16 + 1 = 19      (nparts = 8)
    KP = 1, VEC = 2, 1030 pixels:             2 + 16 + 1 = 19      (nparts = 12)
    KP = 4, VEC = 2, 2050 pixels:             8 + 16 + 1 = 25      (nparts = 8)
    KP = 4, VEC = 1, 1025 pixels:             4 + 16 + 1 = 21      (nparts = 8)
    totals only, VEC = 2, 131074 pixels:      8 + 16 + 2 = 26      (nparts = 260 > 256)
  NaN pixels add nothing (nansum).

No figure above comes from what the device returns."""
import math
from collections import namedtuple

import numpy as np

from tests.rrl_maps_ref import worst_ratio  # noqa: F401  (the same judgement of a result)

LD = np.longdouble
U = 2.0 ** -53
TINY = 2.0 ** -1074
C_OM = 4e-15 / U
BLOCK, WAVE = 256, 64
WPB = BLOCK // WAVE          # waves (= partials) per workgroup
MAPS_FC = FTOT_FC = 16       # channels per workgroup of the register-accumulator kernels
FTOT_KP = 4

Launch = namedtuple("Launch", "kernel vec kp blocks nparts fchunk")


def _cdiv(a, b):
    return -(-a // b)


# ---- ff_maps_launch's rule --------------------------------------------------------------------
def launch_rule(npix, E, F, want_tau=True, want_flux=True, want_ftot=True, aligned=True):
    """What ff_maps_launch (ff_scan.hip) chooses -> Launch(kernel 'small' | 'acc' | 'ftot', VEC,
    KP, workgroups along the pixel axis, partials per (epoch, channel) -- 0 without totals --,
    channels per workgroup), the six figures of rjp_last_maps_launch.  `aligned`: d_sumA, d_tavg
    and the cubes asked for are all 16-byte aligned."""
    assert want_tau or want_flux or want_ftot
    vec = 2 if (npix % 2 == 0 and aligned) else 1
    lanes = npix // vec
    if not want_tau and not want_flux:
        nb = _cdiv(lanes, BLOCK * FTOT_KP)
        return Launch("ftot", vec, FTOT_KP, nb, nb * WPB, FTOT_FC)
    nblk = _cdiv(lanes, BLOCK)
    nzc = _cdiv(F, MAPS_FC)
    nb4 = _cdiv(lanes, BLOCK * 4)
    kp = 4 if nb4 * E * nzc >= 1024 else 1 if nblk * E * nzc >= 1024 else 0
    if kp:
        nbx = nb4 if kp == 4 else nblk
        return Launch("acc", vec, kp, nbx, nbx * WPB if want_ftot else 0, MAPS_FC)
    fsplit = 1
    while nblk * E * fsplit < 2048 and fsplit < F:
        fsplit *= 2
    return Launch("small", vec, 1, nblk, nblk * WPB if want_ftot else 0, _cdiv(F, fsplit))


def n_additions(L, npix):
    """D of the header for launch L (its nparts as with totals)."""
    nparts = L.blocks * WPB
    return L.kp * L.vec + 6 + _cdiv(nparts, BLOCK) + 6 + 4


# ---- reference and bounds ------------------------------------------------------------------------
def _ld(a):
    return np.asarray(a, dtype=LD)


def tau_ref(ctau, A):
    """-> tau[F, P] of one epoch's sums A[P], long double."""
    with np.errstate(all="ignore"):
        return _ld(ctau)[:, None] * _ld(A)[None, :]


def flux_ref(ctau, cflux, A, tavg):
    """-> flux[F, P] of one epoch, long double: NaN where tavg or A is."""
    with np.errstate(all="ignore"):
        om = -np.expm1(-tau_ref(ctau, A))
        return _ld(cflux)[:, None] * _ld(tavg)[None, :] * om


def flux_bound(ctau, cflux, A, tavg, products=2, ref=None):
    """-> the absolute bound [F, P] of the header (NaN where the reference is).  products = 2: the
    cube kernels; 1: the terms of ff_ftot_kernel.  `ref`: flux_ref of the same arguments, where
    the caller has it."""
    assert products in (1, 2)
    with np.errstate(all="ignore"):
        t = tau_ref(ctau, A)
        if ref is None:
            ref = flux_ref(ctau, cflux, A, tavg)
        # kappa = t e^-t / (1 - e^-t) = t / expm1(t); 1 at 0, 0 at inf.  In float64: its own
        # rounding (2 u of a term <= 1 beside C_OM = 36) moves the bound by 1e-17 of itself
        t = t.astype(np.float64)
        kappa = t / np.expm1(t)
        kappa = np.where(t == 0, 1.0, np.where(np.isinf(t), 0.0, kappa))
        ct = np.abs(_ld(cflux)[:, None] * _ld(tavg)[None, :])
        floor = ct + 1.0 + (np.abs(_ld(cflux))[:, None] if products == 2 else 0.0)
        b = U * np.abs(ref) * (_ld(kappa) + (C_OM + products)) + (LD(TINY) / 2) * floor
    return np.where(np.isnan(ref), LD(np.nan), b)


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def two_product(a, b):
    """(p, e) with p = fl(a b) and p + e = a b exactly (Dekker), away from over- and underflow."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def tau_ratio(got, ctau, A):
    """max |got - ctau A| / (u |ctau A|) of one epoch, got[F, P], against the exact product p + e
    (all in float64: got - p is exact for a value that close, and e is 2^-53 of p).  inf unless
    the values that have no such error term -- 0, inf, NaN -- and those whose error term may itself
    round -- products below 2^-900 or above 2^900 -- ARE fl(ctau A), the correctly rounded product
    (which the bound with its floor TINY / 2 admits; nothing is given away)."""
    got = np.asarray(got, dtype=np.float64)
    shape = (len(ctau), len(A))
    c = np.ascontiguousarray(np.broadcast_to(np.asarray(ctau, dtype=np.float64)[:, None], shape))
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(A, dtype=np.float64)[None, :], shape))
    assert got.shape == shape
    with np.errstate(all="ignore"):
        p, e = two_product(c, a)
        special = ~np.isfinite(p) | (np.abs(p) < 2.0 ** -900) | (np.abs(p) > 2.0 ** 900)
        gs, ps = got[special], p[special]
        if not np.array_equal(np.isnan(gs), np.isnan(ps)) or not np.array_equal(
                gs[~np.isnan(ps)].view(np.int64), ps[~np.isnan(ps)].view(np.int64)):
            return np.inf
        ok = ~special
        if not ok.any():
            return 0.0
        err = np.abs((got[ok] - p[ok]) - e[ok])
        r = np.max(err / (U * np.abs(p[ok])))
        return float(r) if r == r else np.inf


def fsum_ld(values):
    """The sum of long-double values, NaN left out, to far below a long-double rounding: every
    value is split into two doubles, math.fsum adds those exactly (one rounding to double), and a
    second pass recovers that rounding."""
    v = _ld(values)
    v = v[~np.isnan(v)]
    hi = v.astype(np.float64)
    lo = (v - hi).astype(np.float64)
    parts = hi.tolist() + lo.tolist()
    s1 = math.fsum(parts)
    if not math.isfinite(s1):
        return LD(s1)
    return LD(s1) + LD(math.fsum(parts + [-s1]))


def _rowsum_ld(v):
    """v[F, P] long double -> [F], NaN left out.  Few rows: fsum_ld of each.  Many rows: a
    compensated (Neumaier) long-double sum that walks the pixels with all rows abreast -- its
    error is of the order 2^-128 P of the sum of the magnitudes, as good as exact here."""
    if v.shape[0] < 64:
        return np.array([fsum_ld(row) for row in v], dtype=LD)
    v = np.where(np.isnan(v), LD(0), v)
    s = np.zeros(v.shape[0], dtype=LD)
    comp = np.zeros(v.shape[0], dtype=LD)
    for p in range(v.shape[1]):
        x = v[:, p]
        t = s + x
        comp += np.where(np.abs(s) >= np.abs(x), (s - t) + x, (x - t) + s)
        s = t
    return s + comp


def ftot_ref(flux):
    """flux[F, P] (long double) -> [F]"""
    return _rowsum_ld(_ld(flux))


def ftot_bound(flux, bound, D):
    """flux, bound [F, P]: the reference and its per-pixel bound -> [F]."""
    return _rowsum_ld(_ld(bound)) + D * U * _rowsum_ld(np.abs(_ld(flux)))


def judge(c, L, tau=None, flux=None, ftot=None):
    """The worst error / bound of a result of case c under launch L -> dict with the keys given
    ('tau', 'flux' [E, F, P], 'ftot' [E, F]), and with a flux 'flux, normal range': the same over
    the voxels above 2^-960 alone (a subnormal flux sits at its floor, half a TINY of rounding
    against half a TINY of bound, and would hide how much of the relative bound is used).  Epoch
    after epoch: the long-double cubes of the largest cases would not fit beside each other."""
    A, tavg, ctau, cflux = c["A"], c["tavg"], c["ctau"], c["cflux"]
    products = 1 if L.kernel == "ftot" else 2
    D = n_additions(L, A.shape[1])
    out = {k: 0.0 for k, v in (("tau", tau), ("flux", flux), ("ftot", ftot)) if v is not None}
    for e in range(A.shape[0]):
        if tau is not None:
            out["tau"] = max(out["tau"], tau_ratio(tau[e], ctau, A[e]))
        if flux is None and ftot is None:
            continue
        ref = flux_ref(ctau, cflux, A[e], tavg)
        b = flux_bound(ctau, cflux, A[e], tavg, products, ref)
        if flux is not None:
            assert products == 2
            out["flux"] = max(out["flux"], worst_ratio(flux[e], ref, b))
            big = np.abs(ref) > 2.0 ** -960
            if big.any():
                out["flux, normal range"] = max(out.get("flux, normal range", 0.0),
                                                worst_ratio(flux[e][big], ref[big], b[big]))
        if ftot is not None:
            out["ftot"] = max(out["ftot"],
                              worst_ratio(ftot[e], ftot_ref(ref), ftot_bound(ref, b, D)))
    return out


# ---- the input sets ---------------------------------------------------------------------------
LN2 = math.log(2.0)
K_EDGES = (1, 2, 53, 1074)


def _k_edge(k, side):
    """tau an ulp below (-1), at (0) or above (+1) k ln2 - ln2 / 2, where rint(-tau log2 e) flips
    between -(k - 1) and -k."""
    t = (k - 0.5) * LN2
    return float(np.nextafter(t, -np.inf if side < 0 else np.inf)) if side else t


# (name, what is planted, its value): "A" a sum, "tau" a sum chosen so that the plant's channel
# sees that optical depth, "tavg" a temperature
# (the first pixel, which the clamped loads of dead lanes read, holds an optically thick sightline)
PLANTS = ([("tau", v) for v in (1e4, 799.9, 800.0, 800.1)] +
          [("A", v) for v in (0.0, 1e-320, 1e-300, 1e-17, 1e-8)] +
          [("tau", _k_edge(k, s)) for k in K_EDGES for s in (-1, 0, 1)] +
          [("A", np.inf), ("A", np.nan), ("tavg", np.nan)])
N_HEAD = 12                  # plants at the first pixels; the others sit before the last pixel


def plant_pixels(npix, seed=0):
    """{plant index: pixel}.  A map with room for all has the first N_HEAD at pixels 0 ..., the rest
    at the pixels before the last one (the last lanes of the last workgroup); the last pixel holds
    the channel's largest flux.  A smaller map takes as many as fit, starting at plant `seed`, so
    that a family of small cases plants every value somewhere."""
    n = len(PLANTS)
    if npix >= n + 1:
        return {i: (i if i < N_HEAD else npix - 1 - (n - i)) for i in range(n)}
    room = npix - 1 if npix > 1 else 1       # a single pixel holds a plant, not the largest flux
    return {(seed + j) % n: j for j in range(room)}


def _logu(rng, lo, hi, shape):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), shape))


def make_case(npix, E, F, tau_range=None):
    """Log-uniform sums and temperatures of an (npix, E, F) call with the edge values planted ->
    dict of float64 arrays A[E, npix], tavg[npix], ctau[F], cflux[F], and `pix`: plant index ->
    pixel.  tau_range = (lo, hi): NO plants, every optical depth inside the band instead (one
    channel coefficient for all channels).  Deterministic."""
    rng = np.random.default_rng(1000003 * npix + 1009 * E + F)
    ctau = _logu(rng, 1e-3, 1.0, F)
    cflux = _logu(rng, 1e-12, 1e-8, F)
    tavg = _logu(rng, 3.0, 3e4, npix)
    if tau_range is not None:
        ctau[:] = ctau[0]
        return dict(A=_logu(rng, tau_range[0], tau_range[1], (E, npix)) / ctau[0], tavg=tavg,
                    ctau=ctau, cflux=cflux, pix={})
    A = _logu(rng, 1e-9, 1e3, (E, npix))          # tau from 1e-12 to 1e3
    pix = plant_pixels(npix, seed=7 * npix + 3 * E + F)
    for i, px in pix.items():
        kind, v = PLANTS[i]
        if kind == "A":
            A[:, px] = v
        elif kind == "tau":
            A[:, px] = v / ctau[i % F]             # the plant's channel; the others see a multiple
        else:
            tavg[px] = v
    if npix > 1:
        # the channel's largest flux in the last pixel (the last live lane of the last
        # workgroup): the hottest sightline, optically thick in every channel
        tavg[npix - 1] = 3e4
        A[:, npix - 1] = 1e7
    return dict(A=A, tavg=tavg, ctau=ctau, cflux=cflux, pix=pix)


def pixel_of(c, kind, value):
    """The pixel of case c that holds the plant (kind, value), or None."""
    for i, px in c["pix"].items():
        k, v = PLANTS[i]
        if k == kind and (v == value or (v != v and value != value)):
            return px
    return None


# the GPU cases: (npix, E, F, outputs, misaligned) -- outputs "all" (tau, flux, ftot and every
# subset with a cube) or "ftot" (totals only); misaligned: which pointer is offset by 8 bytes
Case = namedtuple("Case", "npix E F outputs misaligned")
SMALL_PIX = (1, 2, 3, 127, 128, 129, 511, 513, 1022)
FTOT_PIX = (1, 2, 2047, 2050, 8193)
GPU_CASES = (
    [Case(n, E, F, "all", None) for n in SMALL_PIX for E in (1, 3) for F in (1, 3, 17)] +
    [Case(16384, 1, 100, "all", None), Case(16385, 1, 100, "all", None)] +
    [Case(1030, 6, 906, "all", None), Case(1031, 6, 906, "all", None)] +
    [Case(2050, 8, 1018, "all", None), Case(1025, 8, 1018, "all", None)] +
    [Case(n, E, F, "ftot", None) for n in FTOT_PIX for F in (1, 16, 17, 33) for E in (1, 3)] +
    [Case(131074, 1, 17, "ftot", None)] +
    [Case(1022, 3, 17, "all", "tavg"), Case(1022, 3, 17, "all", "flux"),
     Case(1022, 3, 17, "all", "tau"), Case(2050, 1, 17, "ftot", "tavg")])


def case_id(k):
    return "%dx%dx%d-%s%s" % (k.npix, k.E, k.F, k.outputs,
                              "-%s+8" % k.misaligned if k.misaligned else "")


def case_launch(k):
    return launch_rule(k.npix, k.E, k.F, k.outputs == "all", k.outputs == "all", True,
                       aligned=k.misaligned is None)


# what each family of cases is there to reach, asserted by the CPU test against launch_rule
EXPECTED_KERNEL = {"small": ("small", 1), "kp1": ("acc", 1), "kp4": ("acc", 4),
                   "ftot": ("ftot", 4)}


# ---- float64 emulation of the kernels ------------------------------------------------------------
L2E = 1.4426950408889634074
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
EXP_C = (2.77658272960759129e-07, 2.76399272005369552e-06, 2.48011840775311536e-05,
         1.98411738635095533e-04, 1.38888891559099128e-03, 8.33333337887889360e-03,
         4.16666666661282964e-02, 1.66666666665949731e-01)         # RJP_EXP_C10 ... C3


def fma_two_roundings(a, b, c):
    return a * b + c


def fma_dekker(a, b, c):
    """a b + c with the product exact (Dekker) and the sum by two-sum: one rounding but for rare
    double roundings of the last bit.  Finite arguments away from over- and underflow; elsewhere
    the plain a * b + c."""
    with np.errstate(all="ignore"):
        p, e = two_product(a, b)
        s = p + c
        bb = s - p
        t = (p - (s - bb)) + (c - bb)
        r = s + (t + e)
        plain = a * b + c
        good = np.isfinite(r) & (np.abs(p) > 2.0 ** -900) & (np.abs(p) < 2.0 ** 900)
        return np.where(good, r, plain)


def one_minus_exp_neg(tau, mistake=None, fma=fma_two_roundings):
    """rjp_device.h's one_minus_exp_neg restated from exp_neg_parts, operation by operation.
    fma_two_roundings: the FMAs as multiply and add (k LN2_HI is exact either way: LN2_HI has 21
    trailing zero bits); fma_dekker: as one rounding."""
    tau = np.asarray(tau, dtype=np.float64)
    with np.errstate(all="ignore"):
        if mistake == "float64 exp":
            return 1.0 - np.exp(np.fmax(-tau, -800.0))
        x = np.fmax(-tau, -800.0)
        kd = np.rint(x * L2E)
        r = fma(-kd, LN2_HI, x)
        if mistake != "LN2_LO dropped":
            r = fma(-kd, LN2_LO, r)
        g = np.full_like(r, EXP_C[0])
        for cf in EXP_C[1:]:
            g = fma(g, r, cf)
        em1 = fma(r * r, fma(r, g, 0.5), r)
        s = np.ldexp(1.0, kd.astype(np.int32))
        return fma(-s, em1, 1.0 - s)


def _tree(v):
    """Lane 0 of the shuffle-down reduction over the last axis (64 lanes)."""
    v = v.copy()
    d = WAVE // 2
    while d > 0:
        v[..., :d] = v[..., :d] + v[..., d:2 * d]
        d //= 2
    return v[..., 0]


def _sum_partials(part):
    """sum_partials_kernel: part[..., nparts] -> [...]"""
    n = part.shape[-1]
    steps = _cdiv(n, BLOCK)
    pad = np.zeros(part.shape[:-1] + (steps * BLOCK,))
    pad[..., :n] = part
    lanes = np.zeros(part.shape[:-1] + (BLOCK,))
    for k in range(steps):                                     # the strided loop
        lanes = lanes + pad[..., k * BLOCK:(k + 1) * BLOCK]
    w = _tree(lanes.reshape(lanes.shape[:-1] + (WPB, WAVE)))
    tot = np.zeros(w.shape[:-1])
    for k in range(WPB):
        tot = tot + w[..., k]
    return tot


MISTAKES = ["float64 exp", "LN2_LO dropped", "NaN sum gives 1", "NaN pixel poisons the total",
            "last pixel group dropped", "dead lane counted", "ragged channel slice",
            "hoisted zeroing in a cube kernel"]
# not a mistake (the totals are the same bits), kept to show it: ff_ftot_kernel zeroing a NaN A
# beside zeroing T_avg where either is NaN
HARMLESS = "ftot kernel zeroes a NaN A as well"


def _lanes(a, L, fill):
    """a[..., npix] -> [..., blocks, KP, 256, VEC]: the pixel a lane reads in group k, element v;
    dead lanes hold `fill` (a scalar, or 'first': pixel 0, what their clamped loads read)."""
    npix = a.shape[-1]
    n = L.blocks * L.kp * BLOCK * L.vec
    pad = np.zeros(a.shape[:-1] + (n,))
    pad[..., :npix] = a
    if n > npix:
        pad[..., npix:] = a[..., :1] if isinstance(fill, str) else fill
    return pad.reshape(a.shape[:-1] + (L.blocks, L.kp, BLOCK, L.vec))


def emulate(c, L, mistake=None, fma=fma_two_roundings):
    """The launch L of case c in float64, the same operations in the same order, the same
    reduction trees -> (tau[E, F, P], flux[E, F, P], ftot[E, F]); no cubes (None) for the
    totals-only kernel.  `mistake`: one of MISTAKES (or HARMLESS) planted."""
    A, tavg, ctau, cflux = (np.asarray(c[k], dtype=np.float64)
                            for k in ("A", "tavg", "ctau", "cflux"))
    E, P = A.shape
    F = len(ctau)
    fill = "first" if mistake == "dead lane counted" else 0.0
    tau = flux = None
    if L.kernel != "ftot":
        tau, flux = np.empty((E, F, P)), np.empty((E, F, P))
    ftot = np.empty((E, F))
    with np.errstate(all="ignore"):
        for e in range(E):
            a, ta = A[e], tavg
            if mistake == "hoisted zeroing in a cube kernel" and L.kernel != "ftot":
                ta = np.where(np.isnan(ta) | np.isnan(a), 0.0, ta)
                a = np.where(np.isnan(a), 0.0, a)
            t = ctau[:, None] * a[None, :]
            om = one_minus_exp_neg(t, mistake, fma)           # a finite 1 where t is NaN
            if mistake != "NaN sum gives 1" and L.kernel != "ftot":
                ta = np.where(np.isnan(a), a, ta)             # maps_tavg: the sum's NaN, once
            if L.kernel == "ftot":
                # the hoisted nansum: the weight cflux * T_avg of a pixel whose T_avg or A is NaN
                # is zeroed once; one_minus_exp_neg itself (no NaN test here) gives a finite 1
                # for a NaN, so the term is a zero
                dead = np.isnan(ta) | np.isnan(a)
                if mistake == "NaN sum gives 1":
                    dead = np.isnan(ta)
                elif mistake == "NaN pixel poisons the total":
                    dead = np.zeros(P, dtype=bool)
                if mistake == HARMLESS:
                    t = ctau[:, None] * np.where(np.isnan(a), 0.0, a)[None, :]
                w = _lanes(cflux[:, None] * np.where(dead, 0.0, ta)[None, :], L, fill)
                o = _lanes(one_minus_exp_neg(t, mistake, fma), L, fill)
                acc = np.zeros((F, L.blocks, BLOCK))
                for k in range(L.kp - (mistake == "last pixel group dropped")):
                    for v in range(L.vec):
                        acc = fma_dekker(w[:, :, k, :, v], o[:, :, k, :, v], acc)
            else:
                s = cflux[:, None] * (ta[None, :] * om)
                tau[e], flux[e] = t, s
                z = s if mistake == "NaN pixel poisons the total" else np.where(np.isnan(s), 0.0, s)
                val = _lanes(z, L, fill)
                acc = np.zeros((F, L.blocks, BLOCK))
                for k in range(L.kp - (mistake == "last pixel group dropped")):
                    for v in range(L.vec):
                        acc = acc + val[:, :, k, :, v]
            part = _tree(acc.reshape(F, L.blocks, WPB, WAVE)).reshape(F, L.blocks * WPB)
            ftot[e] = _sum_partials(part)
        if mistake == "ragged channel slice" and L.kernel != "small":
            # a last slice of nf < 16 channels walked to 16: channel F + j of epoch e is row
            # e * F + F + j of the partials, channel j of epoch e + 1 -- which gets epoch e's sum
            # with the coefficients read past the end of the tables (here: the last ones)
            nf = F % MAPS_FC
            if nf:
                wrong = dict(c, ctau=np.full(F, ctau[-1]), cflux=np.full(F, cflux[-1]))
                spill = emulate(wrong, L, None, fma)[2]
                for e in range(E - 1):
                    j = min(MAPS_FC - nf, F)
                    ftot[e + 1, :j] = spill[e, :j]
    return tau, flux, ftot
