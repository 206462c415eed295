"""Host reference of ONE evaluation of the recombination-line optical depth (rjp_rrl_scan, K3):
the term kappa_L * path of one cell and one channel, the error it may carry, and a restatement of
which of the seven Faddeeva paths of rajepy_amd/csrc/rrl_voigt.h the kernel takes for it.

Shared by tests/test_k3_voigt_reference_cpu.py (which pins this file against the oracle, a 40-digit
fixture and the design tool) and tests/test_gpu_k3_evaluations.py (which holds the kernels to it).
Tests only.  No device, and no import of the oracle: NumPy, scipy.special.wofz and the field
values are all it reads.

Fields are a dict of equally shaped float64 arrays, the values the device holds:
    nd   number density, the red-jet flag in its sign bit     xi    ionisation fraction
    temp temperature [K]                                      pf    fill factor / area
    vy   line-of-sight velocity [km/s]                        csize_au   cell size [au] (scalar)
and, for a model with bursts, ts (launch times [s]) and bursts = (red, blue), lists of
(t0_s, amp_rel, sigma_s) as engine.make_bursts takes them.  `line` = rrls.line_constants(...).
"""
import os

import numpy as np
from scipy.special import wofz

LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "k3_voigt.npz")

# rrl_voigt.h
H_WAVE = 0.675               # kHW: lattice step of the wave-uniform paths
CEN_YMAX = 0.03              # kCenYMax
POLE_LITE_Y = 1.3            # kPoleLiteY
SKIP, FAR_A, FAR_B, PLAIN, PLAIN_POLE, CENTRED, GENERIC, PLAIN_POLE_LITE = range(8)
EXP_FLAG = 8                 # kPathExpFlag
PATH_NAMES = {FAR_A: "far series, 6 terms", FAR_B: "far series, 4 terms",
              PLAIN: "plain lattice", PLAIN_POLE: "plain lattice + pole term",
              CENTRED: "centred lattice", GENERIC: "generic per-lane",
              PLAIN_POLE_LITE: "plain lattice + lite pole term"}
C_LIGHT = 299792458.0
AU_CM = 149597870700.0 * 1e2


# ---- the reference term ---------------------------------------------------------------------------
def _chi(fields, time, dtype):
    """1 + sum_b amp_b exp(-(t - ts - t0_b)^2 / (2 sigma_b^2)) of the cell's jet (sign bit of nd)."""
    nd = np.asarray(fields["nd"], dtype=np.float64)
    chi = np.ones(nd.shape, dtype=dtype)
    bursts = fields.get("bursts")
    if not bursts or not (len(bursts[0]) or len(bursts[1])):
        return chi
    red = np.signbit(nd)
    d = dtype(time) - np.asarray(fields["ts"], dtype=np.float64).astype(dtype)
    with np.errstate(all="ignore"):
        for lst, mask in ((bursts[0], red), (bursts[1], ~red)):
            for t0, amp, sigma in lst:
                g = dtype(amp) * np.exp(-(d - dtype(t0)) ** 2 / (2 * dtype(sigma) ** 2))
                chi = chi + np.where(mask, g, dtype(0))
    return chi


def line_term_ref(fields_f64, line, nu, time=0.0):
    """kappa_L * path of every (channel, cell): what the reference sums along y (maths/rrls.py:
    350-354, 383-389; classes.py:1159-1214), term by term.

    x = (nu - nu0) / (sigma sqrt 2), y = (fwhm_L / 2) / (sigma sqrt 2), the LTE prefactor and
    1 - exp(-h nu / k T) (through expm1) are formed in numpy.longdouble from the float64 field
    values; Re w(x + i y) is scipy.special.wofz of x and y rounded to float64.

    -> dict of float64 arrays [len(nu)] + fields' shape: term, x, y, rew, imw, and nu0_is2 (the
    cell's nu0 / (sigma sqrt 2), what `tol` needs), shaped as the fields; term_ld is the term before
    its cast to float64 (tests/rrl_formal_ld_ref.py walks it).  A NaN term is one the reference's
    nansum drops."""
    f = {k: np.asarray(fields_f64[k], dtype=np.float64).astype(LD)
         for k in ("nd", "xi", "temp", "pf", "vy")}
    nu = np.asarray(nu, dtype=np.float64).astype(LD).reshape((-1,) + (1,) * f["nd"].ndim)
    with np.errstate(all="ignore"):
        ne = np.abs(f["nd"]) * _chi(fields_f64, time, LD) * f["xi"]
        nu0 = LD(line["nu_rest"]) * (1 - f["vy"] * 1000 / LD(C_LIGHT))
        sigma = LD(line["kG"]) * np.sqrt(f["temp"]) * nu0 / 2 / np.sqrt(2 * np.log(LD(2)))
        s2 = sigma * np.sqrt(LD(2))
        x = (nu - nu0) / s2
        y = LD(line["kL"]) * ne / 2 / s2 + 0 * x
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        w = wofz(x64 + 1j * y64)
        rew, imw = w.real, w.imag
        lte = (LD(line["kappa0"]) * ne * ne / (f["temp"] * np.sqrt(f["temp"])) *
               np.exp(LD(line["en_over_k"]) / f["temp"]))
        stim = -np.expm1(-LD(line["h_over_k"]) * nu / f["temp"])
        path = LD(fields_f64["csize_au"]) * LD(AU_CM) * f["pf"]
        term = lte * (rew.astype(LD) / (sigma * np.sqrt(2 * LD(np.pi)))) * stim * path
    return dict(term=term.astype(np.float64), term_ld=term, x=x64, y=y64, rew=rew, imw=imw,
                nu0_is2=(nu0 / s2).astype(np.float64))


def tol(bound, x, y, rew, imw, nu0_is2):
    """The allowed error of one term RELATIVE to the term: the caller asserts
    |got - term| <= tol(...) * term.

        tol = bound + 2 |x Re w - y Im w| / Re w * dx,      dx = (|nu0 is2| + 4 |x|) 2^-53

    `bound` is the project's stated bound on Re w for the code under test (gpu_util.K3_RTOL_WAVE or
    K3_RTOL_LANE).  The second summand is not an allowance for the kernel's Voigt code: it is what
    ANY float64 evaluation of x loses before w is called.  Derivation:
      * w'(z) = -2 z w(z) + 2 i / sqrt(pi), so along the real direction
        d Re w / dx = -2 Re(z w) = -2 (x Re w - y Im w): an error dx in x moves Re w by
        2 |x Re w - y Im w| dx, i.e. by that over Re w relative to it.
      * The kernel forms x = fma(nu, is2, c1) with c1 = -nu0 * is2 a ROUNDED product: c1 is off by
        up to half an ulp, |nu0 is2| 2^-53 (nu0 is2 ~ 2e4 .. 1e5 for a thermal width: this is the
        cancellation of nu - nu0 in other words); the fma rounds once more, |x| 2^-53; is2 itself
        comes out of three rounded operations (sqrt, two products and a reciprocal: <= 3 ulp/2),
        which scale nu is2 + c1 = x by a relative 3 * 2^-53: together (|nu0 is2| + 4 |x|) 2^-53.
    The reference's x is formed in longdouble and carries none of this.  In the Gaussian core the
    factor is 2 |x|; in the Lorentzian wings 2 / |x|."""
    x, y = np.abs(np.asarray(x, dtype=np.float64)), np.asarray(y, dtype=np.float64)
    dx = (np.abs(nu0_is2) + 4.0 * x) * 2.0 ** -53
    with np.errstate(all="ignore"):
        cond = 2.0 * np.abs(x * rew - y * imw) / rew
    return bound + cond * dx


# ---- the kernel's layouts and path decision ----------------------------------------------------------
def lanes_per_block(nchan):
    """rrl_launch_lf: lanes along the channel axis of one workgroup."""
    return 256 if nchan > 128 else (64 if nchan > 16 else 16)


def wave_runs(nchan):
    """The channel layout of rrl_scan_kernel for a list of `nchan` channels: one entry per
    (channel block, wave of the block) with live lanes, (even, odd) = the channel indices its even
    and its odd lanes hold.  Lane fl of a block of nblk live channels takes channel
    fbase + (fl odd ? nblk - 1 - (fl >> 1) : fl >> 1) and is live iff fl < nblk."""
    lf = lanes_per_block(nchan)
    out = []
    for fbase in range(0, nchan, lf):
        nblk = min(lf, nchan - fbase)
        for w0 in range(0, lf, 64 if lf >= 64 else lf):
            fl = np.arange(w0, min(w0 + (64 if lf >= 64 else lf), nblk))
            if fl.size == 0:
                continue
            fi = fbase + np.where(fl & 1, nblk - 1 - (fl >> 1), fl >> 1)
            out.append((fi[(fl & 1) == 0], fi[(fl & 1) == 1]))
    return out


def cell_consts(fields_f64, line, time=0.0):
    """cell_line<.., CEN = true> of rrl_voigt.h in float64, operation by operation: the per-cell
    constants the path decision reads (C, nu0, is2, c1, y, a, q, cq of the h = 0.675 lattice)."""
    g = lambda k: np.asarray(fields_f64[k], dtype=np.float64)
    nd, xi, Tk, pf, vy = g("nd"), g("xi"), g("temp"), g("pf"), g("vy")
    with np.errstate(all="ignore"):
        ne = np.abs(nd) * _chi(fields_f64, time, np.float64) * xi
        nu0 = line["nu_rest"] * (1.0 - vy * 1000.0 / C_LIGHT)
        sigma = line["kG"] * np.sqrt(Tk) * nu0 / 2.0 / 1.1774100225154747
        is2 = 1.0 / (sigma * 1.4142135623730951)
        y = 0.5 * (line["kL"] * ne) * is2
        a = line["h_over_k"] / Tk
        C = (line["kappa0"] * (ne * ne / (Tk * np.sqrt(Tk))) * np.exp(line["en_over_k"] / Tk) *
             (fields_f64["csize_au"] * 149597870700.0 * 1e2 * pf) / (sigma * 2.5066282746310002))
        c1 = -nu0 * is2
        pih = np.pi / H_WAVE
        lnq = -2.0 * pih * y
        q = np.where(y < pih, np.exp(lnq), -1.0)
        omq = -np.expm1(lnq)
        cq = (y * y + lnq + 1.7917594692280550 - 2.0 * np.log(omq) - np.log(0.25 * y) +
              17.3221740089 + 4.2046926193909657)
        cq = np.where(y < CEN_YMAX, y * y - np.log(y) + 17.3221740089 + 6.9392539460415, cq)
        C = np.where((C != C) | (C == 0.0) | ~(y > 0.0), 0.0, C)
    return dict(C=C, nu0=nu0, is2=is2, c1=c1, y=y, a=a, q=q, cq=cq)


def _fma(a, b, c):
    """fma(a, b, c) for float64 operands (longdouble product and sum, rounded once more: it differs
    from the fused result only in rare double-rounding ties)."""
    return (np.asarray(a).astype(LD) * np.asarray(b).astype(LD) +
            np.asarray(c).astype(LD)).astype(np.float64)


def band_needs_exp(a, nu_ref, dnu_max):
    """band_needs_exp of rrl_voigt.h, and the ratio it compares with 1."""
    with np.errstate(all="ignore"):
        E0 = np.exp(-a * nu_ref)
        lhs, rhs = 0.5 * (a * dnu_max) * (a * dnu_max), 2e-9 * (1.0 - E0)
        return ~(lhs < rhs), lhs / rhs


def path_codes(cells, nu, nchan=None):
    """path_code() of rrl_voigt.h for every (channel, cell), as rrl_scan_kernel applies it: the code
    of a cell is decided per wave of a channel block from the |x| range of the wave's even and odd
    runs of live channels.  `cells` = cell_consts(...).  -> int array [nchan] + cells' shape; bit 3
    (EXP_FLAG) as the kernel sets it.  Up to 16 channels the kernel has no path codes: every live
    cell runs the generic per-lane code (GENERIC, no flag)."""
    nu = np.asarray(nu, dtype=np.float64)
    nchan = nu.size if nchan is None else int(nchan)
    assert nu.size == nchan
    C, y = cells["C"], cells["y"]
    out = np.zeros((nchan,) + C.shape, dtype=np.int64)
    if lanes_per_block(nchan) == 16:
        out[:] = np.where(C == 0.0, SKIP, GENERIC)
        return out
    nu_ref, dnu_max = 0.5 * (nu.min() + nu.max()), 0.5 * (nu.max() - nu.min())     # fill_line
    fin = lambda v: (v - v) == 0.0
    with np.errstate(all="ignore"):
        E0 = np.exp(-cells["a"] * nu_ref)
        regular = (fin(C) & fin(cells["nu0"]) & fin(cells["is2"]) & fin(y) & (y > 0.0) &
                   fin(cells["a"]) & fin(E0))
        flag, _ = band_needs_exp(cells["a"], nu_ref, dnu_max)
        for even, odd in wave_runs(nchan):
            xmin, xmax = np.full(C.shape, np.inf), np.zeros(C.shape)
            for run in (even, odd):
                if run.size == 0:
                    continue
                lo = _fma(nu[run].min(), cells["is2"], cells["c1"])
                hi = _fma(nu[run].max(), cells["is2"], cells["c1"])
                alo, ahi = np.abs(lo), np.abs(hi)
                xmin = np.fmin(xmin, np.where((lo <= 0.0) & (hi >= 0.0), 0.0, np.fmin(alo, ahi)))
                xmax = np.fmax(xmax, np.fmax(alo, ahi))
            x2min = xmin * xmin
            r2min = _fma(y, y, x2min)
            pole = np.where(y >= POLE_LITE_Y, PLAIN_POLE_LITE, PLAIN_POLE)
            code = np.where((cells["q"] >= 0.0) & (x2min < cells["cq"]), pole, PLAIN)
            code = np.where(y < CEN_YMAX, CENTRED, code)
            code = np.where(xmax > 1e6, GENERIC, code)
            far = (r2min > 64.0) & ((x2min > 64.0) | (y > 1.0))
            code = np.where(far, np.where(r2min > 196.0, FAR_B, FAR_A), code)
            code = np.where(~regular | ~fin(xmax), GENERIC, code)
            code = np.where(flag, code | EXP_FLAG, code)
            code = np.where(C == 0.0, SKIP, code)
            out[np.concatenate([even, odd])] = code
    return out


# ---- Re w: wofz, or the 40-digit fixture where wofz is not good enough ---------------------------------
def load_fixture():
    """tests/golden/k3_voigt.npz -> x [nx], y [ny], rew [ny, nx] (mpmath, 40 digits, rounded)."""
    z = np.load(GOLDEN)
    return z["x"], z["y"], z["rew"]


# ---- the cases of tests/test_gpu_k3_evaluations.py, built on the host ---------------------------------
# (here so that tests/test_k3_voigt_reference_cpu.py can check, without a device, which paths they
# reach and how many evaluations the reference drops)
WAVE_SHAPE = (8, 1, 64)      # n_y = 1: a "sightline sum" is one term
WAVE_TEMPS = (1e3, 1e4, 2e4)
WAVE_NCHAN = (256, 64, 65, 128, 129)
VY = 6.2
XI = 0.2
CSIZE_AU = 0.5
# |x| ranges of the bands of a channel block (one per wave, in rotation over the waves of a list)
WAVE_KINDS = {
    "core": [(0.0, 1.5), (1.5, 3.0), (3.0, 4.5), (4.5, 6.0)],
    "switch": [(8.001, 8.16), (7.84, 7.999), (14.001, 14.28), (13.72, 13.999)],
    "across": [(7.84, 8.16), (13.72, 14.28), (6.0, 16.5), (5.0, 900.0)],
    "wings": [(16.5, 40.0), (40.0, 100.0), (100.0, 300.0), (300.0, 1000.0)],
    # where the pole term is cut: x^2 = cq of the centred lattice (|x| from 5.3 at y = 0.03 to 6.9 at
    # y = 1e-10), and of the plain one around its worst point (x = 1.6, y = 3.75)
    "cut": [(5.2, 5.9), (5.9, 6.5), (6.5, 7.2), (1.0, 2.2)],
    "outlier": [(0.0, 1.5), (1.5, 3.0), (3.0, 4.5), (4.5, 6.0)],   # + one channel at |x| = 2e6
}
X16 = [0.0, 0.15, -0.6, 0.6 + 1e-6, -1.2, 2.0, -3.3, 5.0, -7.9, 8.1, -11.0, 14.2, -20.0, 100.0,
       -1e3, 1e4]
X5 = [0.3, -2.5, 7.99, -8.01, 300.0]
X1 = [1.0]
X40 = list(np.linspace(-9.0, 9.0, 30)) + list(np.geomspace(10.0, 1e4, 5)) + \
    list(-np.geomspace(12.0, 8e3, 5))


def line_centre(line, temp, vy=VY):
    """(nu_c, sigma sqrt 2) of a cell at `temp` and `vy`: x = (nu - nu_c) / (sigma sqrt 2)."""
    nu_c = line["nu_rest"] * (1.0 - vy * 1000.0 / C_LIGHT)
    return nu_c, line["kG"] * np.sqrt(temp) * nu_c / 2.0 / 1.1774100225154747 * np.sqrt(2.0)


def host_fields(y, temp, line, ts=None):
    """Host grids (what RTEngine.upload_fields takes) of cells that share `vy` and have the Voigt
    `y` and the temperature asked for: n_e = 2 y sigma sqrt 2 / kL (y = 0.5 kL n_e / (sigma sqrt 2)),
    n_e = nd * xi with xi = 0.2.  `temp` is a scalar or an array shaped as y."""
    y = np.asarray(y, dtype=np.float64)
    temp = np.broadcast_to(np.asarray(temp, dtype=np.float64), y.shape).copy()
    _, sig2 = line_centre(line, temp)
    ne = 2.0 * y * sig2 / line["kL"]
    one = np.ones(y.shape)
    z = np.arange(y.size).reshape(y.shape) % y.shape[-1]
    return dict(nd=ne / XI, xi=XI * one, temp=temp, ff=one.copy(), areas=one.copy(),
                ts=(np.zeros(y.shape) if ts is None else ts), vy=VY * one,
                rr=np.where(z < y.shape[-1] // 2, -1.0, 1.0))


def as_device_fields(g, bursts=None):
    """The dict line_term_ref / cell_consts take, from host grids in float64 (what an f64 upload
    holds: nd with the red flag in its sign bit, pf = ff / areas)."""
    d = dict(nd=np.where(g["rr"] < 0, -g["nd"], g["nd"]), xi=g["xi"], temp=g["temp"],
             pf=g["ff"] / g["areas"], vy=g["vy"], ts=g["ts"], csize_au=CSIZE_AU)
    if bursts is not None:
        d["bursts"] = bursts
    return d


def wave_cells_y(shape=WAVE_SHAPE):
    """Voigt y per cell: the fixture's y set, in rotation."""
    ys = load_fixture()[1]
    n = int(np.prod(shape))
    return ys[np.arange(n) % ys.size].reshape(shape)


def lane_cells_y(shape=WAVE_SHAPE):
    """Neighbouring cells alternate between the fixture's y < 0.03 and its y > 1: a wave of the
    per-lane code holds lanes that are far-field and lanes that are not."""
    ys = load_fixture()[1]
    small, large = ys[ys < CEN_YMAX], ys[ys > 1.0]
    i = np.arange(int(np.prod(shape)))
    return np.where(i & 1, large[(i >> 1) % large.size], small[(i >> 1) % small.size]).reshape(shape)


def wave_channels(kind, nchan, nu_c, sig2):
    """A channel list of `nchan` frequencies laid out so that the k-th wave (over the blocks of the
    list) holds |x| in WAVE_KINDS[kind][k mod 4]: its even lanes the upper wing, its odd lanes the
    lower one.  "outlier": the last even lane of the first wave of every block sits at x = 2e6."""
    bands = WAVE_KINDS[kind]
    x = np.empty(nchan)
    for k, (even, odd) in enumerate(wave_runs(nchan)):
        lo, hi = bands[k % len(bands)]
        x[even] = np.linspace(lo, hi, even.size) if even.size > 1 else 0.5 * (lo + hi)
        if odd.size:
            x[odd] = -(np.linspace(lo, hi, odd.size) if odd.size > 1 else 0.5 * (lo + hi))
        if kind == "outlier" and k % (lanes_per_block(nchan) // 64) == 0:
            x[even[-1]] = 2e6
    return nu_c + x * sig2


def x_channels(xs, nu_c, sig2):
    return nu_c + np.asarray(xs, dtype=np.float64) * sig2


def band_halfwidth(line, temp, nu_ref, ratio):
    """dnu_max at which band_needs_exp's quotient 0.5 (a dnu_max)^2 / (2e-9 (1 - E0)) is `ratio`
    for a cell at `temp`."""
    a = line["h_over_k"] / temp
    return float(np.sqrt(2.0 * ratio * 2e-9 * -np.expm1(-a * nu_ref)) / a)


BAND_TEMPS = (300.0, 1e4)
BAND_Y = (0.01, 0.3, 2.0, 6.0)


def band_cells(shape=WAVE_SHAPE):
    """(y, temp) per cell of the band-expansion case: 300 K and 1e4 K cells alternate."""
    i = np.arange(int(np.prod(shape)))
    temp = np.where(i & 1, BAND_TEMPS[1], BAND_TEMPS[0]).reshape(shape)
    y = np.asarray(BAND_Y)[(i >> 1) % len(BAND_Y)].reshape(shape)
    return y, temp


def band_channels(line, ratio, nchan=256):
    nu_c, _ = line_centre(line, BAND_TEMPS[0])
    dnu = band_halfwidth(line, BAND_TEMPS[0], nu_c, ratio)
    return np.linspace(nu_c - dnu, nu_c + dnu, nchan), dnu


def check_terms(got, ref, bound):
    """|got - term| <= tol * term for every evaluation the reference keeps; an evaluation may be
    left out only where the reference's term is 0 or not finite (there `got` must be 0, as nansum
    leaves it, or equal to an infinite term), and those stay under 1 % of the case.
    -> (relative errors, mask of the evaluations judged)."""
    term = ref["term"]
    assert got.shape == term.shape
    keep = np.isfinite(term) & (term != 0.0)
    assert (~keep).sum() < 0.01 * keep.size, ((~keep).sum(), keep.size)
    drop_ok = np.where(np.isnan(term) | (term == 0.0), got == 0.0, got == term)
    assert np.all(drop_ok[~keep])
    t = tol(bound, ref["x"], ref["y"], ref["rew"], ref["imw"], ref["nu0_is2"])
    with np.errstate(all="ignore"):
        rel = np.abs(got - term) / term
    bad = keep & ~(rel <= t)
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, rel / t, 0.0)), rel.shape)
        raise AssertionError("%d of %d evaluations outside their tolerance; worst: rel %.3e, tol "
                             "%.3e at x = %.9g, y = %.9g (index %r)"
                             % (bad.sum(), keep.sum(), rel[i], t[i], ref["x"][i], ref["y"][i], i))
    return rel, keep


def worst_by_path(rel, keep, codes, into):
    """Fold the worst relative error per path code (codes & 7) into the dict `into`:
    {code: (worst, evaluations)}."""
    for c in range(1, 8):
        m = keep & ((codes & 7) == c)
        n = int(m.sum())
        if n:
            w0, n0 = into.get(c, (0.0, 0))
            into[c] = (max(w0, float(rel[m].max())), n0 + n)
    return into


def path_table(worst):
    return "\n".join("  path %d  %-32s worst rel. error %.2e over %d evaluations"
                     % (c, PATH_NAMES[c], worst[c][0], worst[c][1]) for c in sorted(worst))
