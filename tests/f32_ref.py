"""Reference for `storage="f32"` evaluated on the fields AS THE DEVICE STORES THEM (tests only; plain
NumPy, nothing here imports the GPU package).  Shared by tests/test_f32_reference_cpu.py, which pins
it, and tests/test_gpu_f32_storage.py, which holds the f32 kernels to it.

The suite's other f32 assertions compare with the oracle on the UNROUNDED float64 fields at 1e-5;
rounding the inputs to float moves an optical depth by 1e-7 ... 4e-7, so everything subtler than
that hides in the band.  Here the float fields are read back, widened, and are the reference's
inputs: what is left is the kernels' own arithmetic, which is f64 everywhere except K1's burst
Gaussian (one hardware float exp2 per burst, `exp2_gauss<true>` in rjp_device.h).

Bounds (relative to the reference value unless said otherwise; n_y = cells per sightline):
  K1 tau sums, no bursts   1.5e-13 + (n_y + 8) 2^-53   T^-1.5 / T^-1.35 are < 1e-13 (pow_m1p5,
                                                       pow_m1p35_batch), + the product's roundings
                                                       and an n_y-term f64 sum
  K1 EM, no bursts         (n_y + 4) 2^-53             three roundings of (|nd| xi)^2 pf, the scale
  T_avg                    (n_y + 2) 2^-53             an n_y-term sum and one division
  K1 with bursts           ABSOLUTE, per pixel: chi_dev = 1 + sum_b amp_b g_b (1 + eps_b), |eps_b| <=
                           delta, S = sum_b |amp_b| g_b  =>  |chi_dev^2 - chi^2| <= 2 |chi| delta S +
                           delta^2 S^2, summed with the cells' weights, plus the no-burst bound times
                           the reference sum.  delta = 2^-22: one float exp2 on [2^-1/2, 2^1/2] good
                           to an ulp plus the float rounding of its argument would be 2^-23 + ln2
                           2^-26 = 1.3e-7; the bar is twice that.  Measured on an MI355X: 2.6e-8 ...
                           6.6e-8 on every shape, layout and tile.
  rjp_ff_cells             gpu_util.GAUSS_RTOL + 1.5e-13 + 8 2^-53 per cell
"""
import copy
import types

import numpy as np

from oracle import rt_oracle as orc
from tests import gpu_util as U

DELTA = 2.0 ** -22                    # the bar on one float-accuracy Gaussian of K1
DELTA_ULP = 2.0 ** -23                # ... and what a NumPy float32 exp2 must stay inside
POW = {0: "-1.5", 1: "-1.35"}         # RJP_GFF_SCALAR, RJP_GFF_POWERLAW: exponent of T in a0
EPS = 2.0 ** -53


def tau_rtol(ny):
    return 1.5e-13 + (ny + 8) * EPS


def em_rtol(ny):
    return (ny + 4) * EPS


def tavg_rtol(ny):
    return (ny + 2) * EPS


CELLS_RTOL = U.GAUSS_RTOL + 1.5e-13 + 8 * EPS


def em_scale(csize_au):
    """csize au / pc exactly as the library forms it (ff_scan.hip `em_scale`): an input here."""
    return float(csize_au) * 149597870700.0 / 3.085677581491367e+16


# ---- the stored fields ---------------------------------------------------------------------------
def _host(t):
    if t is None:
        return None
    if hasattr(t, "cpu"):
        t = t.cpu().numpy()
    return np.asarray(t)


def device_fields(fields):
    """A DeviceFields of either dtype (or `host_fields`' stand-in) -> float64 arrays [n_x, n_y, n_z]:
    nd (magnitude), red (sign bit of nd, NaN and zero cells included), xi, temp, pf, ts, vy and,
    when the compact field is attached, em0 (magnitude) + em0_red."""
    shape = tuple(int(s) for s in fields.shape)
    raw = lambda t: None if t is None else _host(t).reshape(shape)
    wide = lambda t: None if t is None else raw(t).astype(np.float64)
    d = dict(shape=shape, csize_au=float(fields.csize_au), dtype=int(fields.dtype))
    d["nd"], d["red"] = np.abs(wide(fields.nd)), np.signbit(raw(fields.nd))
    for k in ("xi", "temp", "pf", "ts", "vy"):
        d[k] = wide(getattr(fields, k, None))
    em0 = getattr(fields, "em0", None)
    if em0 is not None:
        d["em0"], d["em0_red"] = np.abs(wide(em0)), np.signbit(raw(em0))
    return d


def host_fields(g, csize_au, dtype=np.float32):
    """What `RTEngine.upload_fields(..., dtype=4)` leaves on the device, restated in NumPy
    (rjp_pack_field + rjp_compact_fields): every field cast once, pf the cast of the f64 quotient,
    the red flag in nd's sign bit, em0 the cast of the f64 product of the WIDENED fields -- or None
    where the range guard of compact_fields_kernel keeps the wide layout.  dtype=np.float64: the
    unrounded fields in the same container."""
    red = g["rr"] < 0
    with np.errstate(all="ignore"):
        cast = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)
        nd = cast(np.copysign(np.abs(g["nd"]), np.where(red, -1.0, 1.0)))
        xi, temp, ts = cast(g["xi"]), cast(g["temp"]), cast(g["ts"])
        pf = cast(g["ff"] / g["areas"])
        vy = cast(g["vy"]) if g.get("vy") is not None else None
        n0 = np.abs(nd.astype(np.float64)) * xi.astype(np.float64)
        prod = n0 * n0 * pf.astype(np.float64)
        out = prod.astype(dtype)
        back = np.abs(out.astype(np.float64))
        bad = pf.astype(np.float64) < 0.0
        if np.dtype(dtype) == np.float32:
            bad |= ~np.isnan(prod) & (np.abs(prod) <= 1.7e308) & \
                ((back > 3.4e38) | ((prod != 0.0) & (back < 1.2e-38)))
        em0 = None if bad.any() else np.copysign(np.abs(out), np.where(np.signbit(nd), -1, 1)
                                                 ).astype(dtype)
    return types.SimpleNamespace(shape=tuple(g["nd"].shape), dtype=np.dtype(dtype).itemsize,
                                 csize_au=float(csize_au), nd=nd, xi=xi, temp=temp, pf=pf, ts=ts,
                                 vy=vy, em0=em0)


def oracle_of(params, dev, layout="wide"):
    """The oracle on the stored fields: ff = pf, areas = 1, rr = -1 where red, +1 elsewhere.
    layout="compact": on the field the compact scan reads instead -- em0 is a float rounding of its
    own (up to 2^-24 per cell away from the product of the stored nd, xi, pf), so the oracle is
    given nd = sqrt(|em0|), xi = pf = 1 and the flag of em0's sign bit: (nd xi)^2 pf is em0 again to
    2 2^-53."""
    p = copy.deepcopy(params)
    nx, ny, nz = dev["shape"]
    p["grid"].update(n_x=nx, n_y=ny, n_z=nz, c_size=dev["csize_au"])
    one = np.ones(dev["shape"])
    if layout == "compact":
        nd, xi, pf, red = np.sqrt(dev["em0"]), one, one, dev["em0_red"]
    else:
        assert layout == "wide", layout
        nd, xi, pf, red = dev["nd"], dev["xi"], dev["pf"], dev["red"]
    return orc.OracleJet.from_fields(p, nd, xi, dev["temp"], pf, one, dev["ts"],
                                     np.where(red, -1.0, 1.0), dev["vy"])


def burst_lists_of(jet):
    """(red, blue) lists [(t0_s, amp_rel, sigma_s), ...] of an OracleJet (gpu_util.bursts_from_oracle
    without the device struct)."""
    out = []
    for which, ss in (("R", jet._ss_jml_rj), ("B", jet._ss_jml_bj)):
        out.append([(t0, (peak - ss) / ss, hl * 2. / (2. * np.sqrt(2. * np.log(2.))))
                    for t0, peak, hl in jet.bursts[which]])
    return out[0], out[1]


# ---- per-cell weights, formed in long double and rounded once ------------------------------------
def _signed(mag, red):
    return np.copysign(np.asarray(mag, dtype=np.float64), np.where(red, -1.0, 1.0))


def _em_ld(dev, layout):
    ld = lambda a: a.astype(np.longdouble)
    if layout == "compact":
        return ld(dev["em0"]), dev["em0_red"]
    assert layout == "wide", layout
    with np.errstate(all="ignore"):
        n0 = ld(dev["nd"]) * ld(dev["xi"])
        return n0 * n0 * ld(dev["pf"]), dev["red"]


def em0_of(dev, layout):
    """Signed weight of the emission measure: (|nd| xi)^2 pf (wide) or |em0| (compact); the sign bit
    is the red flag (what gpu_util.ref_single_epoch reads the jet from)."""
    g, red = _em_ld(dev, layout)
    return _signed(g, red)


def a0_of(dev, mode, layout):
    """Signed weight of the optical depth: the above times T^-1.5 (scalar Gaunt mode, 0) or T^-1.35
    (power law, 1)."""
    g, red = _em_ld(dev, layout)
    with np.errstate(all="ignore"):
        return _signed(g * np.power(dev["temp"].astype(np.longdouble), np.longdouble(POW[mode])),
                       red)


def _ts(dev):
    return dev["ts"] if dev["ts"] is not None else np.zeros(dev["shape"])


def tau_sums_of(dev, mode, layout, bursts=((), ()), t=0.0):
    """sum_y |a0| chi^2 [n_x, n_z] -- times ctau[f] it is the optical depth."""
    return U.ref_single_epoch(a0_of(dev, mode, layout), _ts(dev), bursts, t, threads=1)


def em_of(dev, layout, bursts=((), ()), t=0.0):
    """Emission measure [pc cm^-6]: sum_y em0 chi^2 times csize au / pc."""
    return U.ref_single_epoch(em0_of(dev, layout), _ts(dev), bursts, t, threads=1) * \
        em_scale(dev["csize_au"])


def tavg_of(dev):
    """nanmean_y(T where T > 0); NaN where a sightline has no such cell."""
    T = dev["temp"]
    hot = T > 0.0
    s = np.add.reduce(np.where(hot, T, 0.0), axis=1, dtype=np.longdouble)
    n = hot.sum(axis=1)
    with np.errstate(all="ignore"):
        return (s / n).astype(np.float64)


def _chi_and_s(dev, red, bursts, t):
    """chi = 1 + sum amp g and S = sum |amp| g per cell (f64, numpy.exp).  A jet without bursts has
    chi = 1 whatever its launch times; a NaN launch time in a jet with bursts gives NaN."""
    ts = _ts(dev)
    chi, S = np.ones(dev["shape"]), np.zeros(dev["shape"])
    with np.errstate(all="ignore"):
        for lst, mask in ((bursts[0], red), (bursts[1], ~red)):
            for t0, amp, sigma in lst:
                g = np.exp(-((t - ts[mask]) - t0) ** 2 / (2. * sigma ** 2))
                chi[mask] += amp * g
                S[mask] += abs(amp) * g
    return chi, S


def cells_of(dev, mode, layout, bursts, t, ctau):
    """Per-cell optical depths [F, n_x, n_y, n_z] = ctau[f] |a0| chi^2, NaN where any factor is."""
    a0 = a0_of(dev, mode, layout)
    chi, _ = _chi_and_s(dev, np.signbit(a0), bursts, float(t))
    with np.errstate(all="ignore"):
        return np.asarray(ctau, dtype=np.float64)[:, None, None, None] * (np.abs(a0) * (chi * chi))


def k1_bound(dev, mode, layout, bursts, t, em=False, delta=DELTA):
    """-> (bound, ref, unit), each [n_x, n_z]: the per-pixel ABSOLUTE bound on a K1 map with bursts
    (module docstring), the reference sums, and unit = sum_y w 2 |chi| S, the quantity the float
    exponential's error multiplies.  `em`: for the emission measure (weights em0, sums times
    csize au / pc) instead of the tau sums."""
    ny = dev["shape"][1]
    w0 = em0_of(dev, layout) if em else a0_of(dev, mode, layout)
    chi, S = _chi_and_s(dev, np.signbit(w0), bursts, float(t))
    w = np.abs(w0)
    with np.errstate(all="ignore"):
        dropped = np.isnan(w * (chi * chi))                 # nansum drops these terms
        lin = np.where(dropped, 0.0, w * (2. * np.abs(chi) * S))
        sq = np.where(dropped, 0.0, w * (S * S))
    scale = em_scale(dev["csize_au"]) if em else 1.0
    ref = U.ref_single_epoch(w0, _ts(dev), bursts, float(t), threads=1) * scale
    unit = lin.sum(axis=1) * scale
    bound = delta * unit + delta * delta * sq.sum(axis=1) * scale + \
        (em_rtol(ny) if em else tau_rtol(ny)) * ref
    return bound, ref, unit


def k1_ratio(got, ref, unit, ny, em=False):
    """Worst |got - ref| / unit over the pixels, the f64 part of the bound taken off first (where no
    burst is alive `unit` is ~0 and the difference is f64 rounding): the observed delta."""
    err = np.abs(got - ref) - (em_rtol(ny) if em else tau_rtol(ny)) * ref
    ok = (unit > 0.0) & (err > 0.0)
    return float(np.max(err[ok] / unit[ok])) if ok.any() else 0.0


def within_abs(got, ref, bound, what):
    """Identical zero / NaN patterns and |got - ref| <= bound; -> worst error / bound."""
    assert np.array_equal(got == 0, ref == 0), what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = np.isfinite(ref) & (ref != 0)
    if not ok.any():
        return 0.0
    frac = float(np.max(np.abs(got[ok] - ref[ok]) / bound[ok]))
    assert frac <= 1.0, (what, frac)
    return frac


# ---- the cases both test files run ---------------------------------------------------------------
# shapes chosen for the f32 lane geometry (ff_scan_vec): 4 sightlines per lane iff n_z % 4 == 0
SHAPES = [(5, 37, 52),          # 4-wide lanes, 65 of them (one past a wave), odd n_y
          (3, 50, 7),           # 1-wide lanes, n_z % 4 == 3
          (2, 41, 6),           # 1-wide lanes, n_z % 4 == 2
          (1, 1, 4),            # one row
          (1, 3, 5),            # fewer rows than any unroll
          (4, 64, 128)]         # the smoke shape: y-split four ways
EPOCH_COUNTS = (1, 2, 3, 4, 5, 8, 9, 13)   # every tile (1, 2, 4 | 8) of both lane widths + tails


def case_fields(shape, seed=None):
    """Host fields for `shape`: gpu_util.synth_host with a temperature spread, NaN and zero cells in
    every field (as test_gpu_random_parity._case plants them), empty rows at both ends of every
    sightline and one empty sightline."""
    nx, ny, nz = shape
    seed = 4100 + nx * 1000 + ny * 10 + nz if seed is None else seed
    rng = np.random.default_rng(seed)
    g = U.synth_host(shape, seed, 1)
    for k, vals in (("nd", [np.nan, 0.0]), ("xi", [np.nan]), ("temp", [np.nan]),
                    ("ff", [np.nan, 0.0]), ("ts", [np.nan])):
        m = rng.random(shape) < 0.04
        g[k] = np.where(m, rng.choice(vals, size=shape), g[k])
    if ny >= 16:
        lo, hi = ny // 8, ny - ny // 5
        for k in ("nd", "temp"):
            g[k][:, :lo, :] = np.nan
            g[k][:, hi:, :] = np.nan
    if nx * nz > 1:
        g["nd"][0, :, 0] = np.nan
        g["temp"][0, :, 0] = np.nan
    return g


def guard_cases(shape=(1, 2, 4)):
    """[(host fields, keeps the compact layout)] either side of compact_fields_kernel's float range
    guard, all factors powers of two (xi = 1): (n x)^2 pf = 2^126 and 2^-124 stay compact, 2^128
    (overflow) and 2^-127 (a non-zero product below the normal range; pf = 1/2) go wide."""
    out = []
    for e, pf, keeps in ((63, 1.0, True), (-62, 1.0, True), (64, 1.0, False), (-63, 0.5, False)):
        g = dict(nd=np.full(shape, 2.0 ** e), xi=np.ones(shape), temp=np.full(shape, 1e4),
                 ff=np.full(shape, pf), areas=np.ones(shape), ts=np.zeros(shape),
                 rr=np.ones(shape), vy=None)
        out.append((g, keeps))
    return out


def _sigma(hl_yr):
    return hl_yr * orc.YEAR * 2. / (2. * np.sqrt(2. * np.log(2.)))


def burst_sets():
    """name -> (red, blue) lists of (t0_s, amp_rel, sigma_s)."""
    rng = np.random.default_rng(2207)
    many = lambda: [(float(rng.uniform(-0.5, 5.5)) * orc.YEAR, float(rng.uniform(0.2, 11.)),
                     _sigma(float(rng.uniform(0.12, 1.2)))) for _ in range(11)]
    dips = lambda: [(float(rng.uniform(0.3, 4.5)) * orc.YEAR, float(rng.uniform(0.6, 0.95)) - 1.0,
                     _sigma(float(rng.uniform(0.2, 1.0)))) for _ in range(3)]
    return {"example": U.example_burst_lists(),
            "eleven": (many(), many()),         # the overflow table (> RJP_SGPR_BURSTS per jet)
            "red-only": U.example_burst_lists(only="R"),
            "dips": (dips(), dips())}


def epoch_lists():
    """13 uniformly spaced and 13 irregular epochs [s]; the tests scan their prefixes."""
    rng = np.random.default_rng(913)
    uniform = [(0.3 + 0.35 * k) * orc.YEAR for k in range(13)]
    irregular = sorted((rng.uniform(0., 5., 13) * orc.YEAR).tolist())
    return {"uniform": uniform, "irregular": irregular}
