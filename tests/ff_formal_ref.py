"""Long-double reference of the free-free formal solution (rjp_ff_formal, K5; ff_formal.hip and
formal_b / formal_update / formal_out in ff_formal.h) with a derived per-pixel, per-channel ABSOLUTE
bound, and the hand-made inputs both test files run (tests only; NumPy, nothing here imports the GPU
package).  tests/test_ff_formal_reference_cpu.py pins this module (a 50-digit mpmath evaluation,
closed forms, Richardson differences, a float64 emulation, planted mistakes, non-vacuity),
tests/test_gpu_ff_formal_ld.py holds the kernel to it.

Inputs: the values the device holds.
    tau layout   a0 read back (jet flag in its sign bit), ts, temp: `cells_tau`
    f32 storage, wide / compact layouts   f32_ref.device_fields and f32_ref.cells_of: `cells_fields`
Nothing comes from rjp_ff_cells.  b must be finite or NaN: an infinite b (T = 0 next to a non-zero
density, a product beyond 1.8e308) is out of scope, `cells_*` refuse it.

Per cell i and channel f, in numpy.longdouble: c_i = ctau[f] b_i, b_i = |a0_i| chi_i^2; a NaN term is
dropped (c_i = 0), a cell is live where c_i != 0 and T_i counts only there.  With Theta_i =
exp(-sum_{j<i} c_j) (the summed depth, not a running product) and om_i = -expm1(-c_i):
    I = sum_i T_i om_i Theta_i,   out = csrc[f] I
NaN exactly where no cell of the sightline has T > 0, +0.0 where one has but none is live.

THE BOUND, absolute, per pixel and channel, term by term from the code as it stands (u = 2^-53,
E = 37 >= 4e-15 / u, the relative error rjp_device.h states for one_minus_exp_neg; every term times
|csrc|; `reference` returns them separately, TERMS names them):
  inputs     eps_c,i sum_i c_i |dI/dc_i|, dI/dc_i = T_i e^-c_i Theta_i - sum_{k>i} T_k om_k Theta_k
             = Theta_i e^-c_i (T_i - R_i), R_i = sum_{k>i} T_k om_k exp(-sum_{i<m<k} c_m) by the
             backward recurrence R_{i-1} = T_i om_i + e^-c_i R_i: no two chains are subtracted.
             tau layout: eps_c = u (the product ctau b) where the call or the cell's jet has no
             burst (b = |a0| exactly), else 3 u (a chi^2: two more) + gpu_util.GAUSS_RTOL, the
             project's bound on chi^2 from the degree-8 Gaussians.  Elsewhere f32_ref.CELLS_RTOL,
             or its no-burst part 1.5e-13 + 8 u.
  emission   the term t_i = T_i om_i Theta_i carries E u (om), u (the product T om), u (its FMA)
             and u for every later live cell, whose FMA rounds a partial sum that contains t_i:
             u sum_i t_i (E + 2 + n_later,i).
  attenuation  Theta' = fma(-Theta, om, Theta) is Theta (1 - om (1 + delta)) rounded once: the error
             made AT cell j is ABSOLUTE and relative to Theta_j, not to Theta_{j+1}:
                 g_j = (E om_j + 1) u Theta_j
             (om_j = 1 - e^-30 leaves Theta_{j+1} = e^-30 with a RELATIVE error of e^30 u).  Every
             Theta_k behind is Theta_{j+1} times the later factors, so g_j reaches the pixel as
             g_j S_j / Theta_{j+1} = g_j R_j, and R_j <= T_max behind: a cold thick front before
             hot gas is where this term is large against the pixel.  sum_j g_j R_j.
  floor      where dtau, T om, the sum or Theta leave the normal range a float64 result is a
             multiple of 2^-1074: per live cell 2^-1075 on ctau b (times dI/dc <= T_max; once more
             for f32_ref.cells_of's own float64 product), on T om, on the FMA, and on Theta' (times
             R <= T_max):  2^-1075 n_live (3 T_max + 2), and 2^-1074 for csrc I.  Below 1e-315
             in every test; it matters only for dtau = 1e-320.
  csrc       one rounding: u |csrc I|.
The sum is multiplied by 1 + 2^-20 for the products of two of these errors.  The bound is 0 exactly
where the sightline has no live cell on that channel; the kernel must be exact there.
"""
import numpy as np

from tests import f32_ref as F
from tests import gpu_util as U

LD = np.longdouble
HAVE_LD = bool(np.finfo(LD).eps <= 2.0 ** -63)
LD_REASON = "numpy.longdouble is no wider than float64 on this host"
U0 = 2.0 ** -53
TINY = 2.0 ** -1074
E_EXP = 37                                   # 4e-15 / 2^-53, rounded up
SECOND = 1.0 + 2.0 ** -20
EPS_TAU_BURSTS = 3 * U0 + U.GAUSS_RTOL
EPS_FIELDS_PLAIN = 1.5e-13 + 8 * U0
TERMS = ("inputs (eps_c)", "emission roundings", "attenuation", "subnormal floor", "csrc")
YEAR = 31536000.0


# ---- per-cell depths --------------------------------------------------------------------------------
def _chi(red, ts, bursts, t, T=LD, skip=None):
    """chi per cell in type T and the mask of the cells whose jet has bursts.  A jet without bursts
    has chi = 1 whatever its launch times; a NaN launch time in a jet with bursts gives NaN.
    `skip`: index of a burst left out of every jet (a planted mistake)."""
    chi = np.ones(red.shape, dtype=T)
    has = np.zeros(red.shape, dtype=bool)
    if bursts is None:
        return chi, has
    with np.errstate(all="ignore"):
        d = T(t) - np.asarray(ts, dtype=np.float64).astype(T)
        for lst, mask in ((bursts[0], red), (bursts[1], ~red)):
            if not len(lst):
                continue
            has |= mask
            s = np.ones(red.shape, dtype=T)
            for i, (t0, amp, sg) in enumerate(lst):
                if i == skip:
                    continue
                dd = d - T(t0)
                s = s + T(amp) * np.exp(-(dd * dd) * T(1.0 / (2.0 * float(sg) ** 2.0)))
            chi = np.where(mask, s, chi)
    return chi, has


def b_tau(a0, ts, bursts, t, T=LD, skip=None):
    """b = |a0| chi^2 per cell in type T (0 for a dropped cell) and the has-bursts mask."""
    a0 = np.asarray(a0, dtype=np.float64)
    chi, has = _chi(np.signbit(a0), ts, bursts, t, T, skip)
    with np.errstate(all="ignore"):
        b = np.abs(a0).astype(T) * (chi * chi)
    b = np.where(np.isnan(b), T(0), b)
    assert np.all(np.isfinite(b)), "an infinite b is out of scope"
    return b, has


def cells_tau(a0, ts, bursts, t, ctau):
    """The tau layout -> (c [F, nx, ny, nz] long double, eps_c [nx, ny, nz])."""
    b, has = b_tau(a0, ts, bursts, t)
    c = np.asarray(ctau, dtype=np.float64).astype(LD)[:, None, None, None] * b[None]
    return c, np.where(has, EPS_TAU_BURSTS, U0)


def layout_of(dev):
    return "compact" if dev.get("em0") is not None else "wide"


def cells_fields(dev, mode, bursts, t, ctau, layout=None):
    """f32 storage and the wide / compact layouts, from f32_ref.device_fields' dict -> (c, eps_c)."""
    layout = layout_of(dev) if layout is None else layout
    lists = bursts if bursts is not None else ((), ())
    with np.errstate(all="ignore"):
        c = F.cells_of(dev, mode, layout, lists, t, ctau)
        red = np.signbit(F.a0_of(dev, mode, layout))
    c = np.where(np.isnan(c), 0.0, c)
    assert np.all(np.isfinite(c)), "an infinite b is out of scope"
    has = np.where(red, len(lists[0]) > 0, len(lists[1]) > 0)
    return c.astype(LD), np.where(has, F.CELLS_RTOL, EPS_FIELDS_PLAIN)


# ---- the walk and the bound ----------------------------------------------------------------------------
def _front(a):
    """Exclusive running sum along y: what lies in front of every cell."""
    s = np.cumsum(a, axis=2)
    return np.concatenate([np.zeros_like(s[:, :, :1]), s[:, :, :-1]], axis=2)


def _behind(a):
    """Exclusive running sum along y from the back: what lies behind every cell."""
    s = np.cumsum(a[:, :, ::-1], axis=2)[:, :, ::-1]
    return np.concatenate([s[:, :, 1:], np.zeros_like(s[:, :, :1])], axis=2)


def walk(c, T):
    """sum_i T_i (1 - e^-c_i) exp(-sum_{j<i} c_j) in the arrays' own type -> [F, nx, nz]."""
    return np.sum(T * -np.expm1(-c) * np.exp(-_front(c)), axis=2)


def sensitivities(c, T):
    """-> dict of [F, nx, ny, nz] arrays: t (the terms), om, Th, R (module docstring), dIdc, and
    scale = Theta e^-c (T + R), the magnitude of dIdc's two parts."""
    om, e, Th = -np.expm1(-c), np.exp(-c), np.exp(-_front(c))
    R = np.zeros_like(c)
    acc = np.zeros(c.shape[:2] + c.shape[3:], dtype=c.dtype)
    for i in range(c.shape[2] - 1, -1, -1):
        R[:, :, i] = acc
        acc = T[:, :, i] * om[:, :, i] + e[:, :, i] * acc
    return dict(t=T * om * Th, om=om, Th=Th, R=R, dIdc=Th * e * (T - R), scale=Th * e * (T + R))


def reference(c, eps_c, temp, csrc):
    """c [F, nx, ny, nz] long double (0 = dropped), eps_c and temp [nx, ny, nz] -> dict: ref (float64),
    ref_ld, terms (the five of the bound, float64 [F, nx, nz]), bound, c, T, s (sensitivities)."""
    temp = np.asarray(temp, dtype=np.float64)
    live = c != 0
    assert np.all(temp[np.any(live, axis=0)] > 0.0)
    T = np.where(live, temp[None], 0.0).astype(LD)
    s = sensitivities(c, T)
    I = np.sum(s["t"], axis=2)
    cs = np.asarray(csrc, dtype=np.float64).astype(LD)[:, None, None]
    hot = np.any(temp > 0.0, axis=1)
    out = np.where(hot[None], cs * I, LD("nan"))
    n_live = np.sum(live, axis=2)
    n_later = _behind(live.astype(LD))
    t_max = np.max(T, axis=2)
    terms = [np.sum(np.asarray(eps_c)[None] * c * np.abs(s["dIdc"]), axis=2),
             U0 * np.sum(s["t"] * (E_EXP + 2 + n_later), axis=2),
             U0 * np.sum(np.where(live, (E_EXP * s["om"] + 1) * s["Th"] * s["R"], LD(0)), axis=2),
             LD(2) ** -1075 * n_live * (3 * t_max + 2),
             U0 * np.abs(I)]
    terms = [np.abs(cs) * x for x in terms]
    terms[3] = terms[3] + np.where(n_live > 0, LD(TINY), LD(0))
    terms = [(SECOND * x).astype(np.float64) for x in terms]
    return dict(ref=out.astype(np.float64), ref_ld=out, terms=terms, bound=sum(terms), c=c, T=T, s=s)


def reference_tau(a0, ts, temp, bursts, t, ctau, csrc):
    c, eps = cells_tau(a0, ts, bursts, t, ctau)
    return reference(c, eps, temp, csrc)


def reference_fields(dev, mode, bursts, t, ctau, csrc, layout=None):
    c, eps = cells_fields(dev, mode, bursts, t, ctau, layout)
    return reference(c, eps, dev["temp"], csrc)


def dominant(r, at):
    return TERMS[int(np.argmax([x[at] for x in r["terms"]]))]


def judge(got, r, what=""):
    """Identical NaN and zero patterns (zeros are +0.0) and |got - ref| <= bound on EVERY pixel and
    channel, exactly 0 where the bound is 0 -> (worst share of the bound, name of the term that
    dominates the bound there, index).  Asserts nothing about the share itself."""
    ref, bound = r["ref_ld"], r["bound"]
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert np.array_equal(got == 0, r["ref"] == 0), what
    assert not np.any(np.signbit(got[got == 0])), what
    ok = ~np.isnan(ref)
    err = np.where(ok, np.abs(got.astype(LD) - ref).astype(np.float64), 0.0)
    assert np.all(err[ok & (bound == 0.0)] == 0.0), what
    share = np.where(ok & (bound > 0.0), err / np.where(bound > 0.0, bound, 1.0), 0.0)
    i = np.unravel_index(np.argmax(share), share.shape)
    return float(share[i]), dominant(r, i), i


# ---- float64 emulation of the kernel's update, with the mistakes the bound must catch -----------------
MISTAKES = ("exp64", "clamp30", "float-dtau", "far-end", "theta-first", "slab-reset", "dead-T",
            "ninth-burst")


def emulate(b, temp, ctau, csrc, mistake=None, where=None):
    """formal_update restated in float64 with om = -expm1(-dtau), one update per cell, front to back:
    I += (T om) Theta; Theta -= Theta om (NumPy has no FMA: one rounding more on each, inside E).
    b [nx, ny, nz] float64 (0 = dropped).  `mistake` (applied on the sightlines `where` [nx, nz], all
    by default):
      exp64        om = 1 - exp(-dtau) through float64 exp, for dtau >= 1e-6
      clamp30      the exponential's argument clamped at -30 instead of -800
      float-dtau   ctau b rounded to float
      far-end      observer at the iy = n_y - 1 end
      theta-first  Theta updated before I
      slab-reset   Theta = 1 again at every 16th row
      dead-T       a dead cell's T counted (T NaN there: NaN 0)
    ("ninth-burst" is a mistake in b: b_tau(..., skip=8).)"""
    b = np.asarray(b, dtype=np.float64)
    temp = np.asarray(temp, dtype=np.float64)
    nx, ny, nz = b.shape
    ct = np.asarray(ctau, dtype=np.float64)[:, None, None]
    sel = np.ones((nx, nz), dtype=bool) if where is None else where
    on = lambda m: sel[None] if mistake == m else False
    I = np.zeros((len(ctau), nx, nz))
    Th = np.ones_like(I)
    rows = range(ny - 1, -1, -1) if mistake == "far-end" else range(ny)
    with np.errstate(all="ignore"):
        for y in rows:
            by = b[:, y, :]
            tk = np.where(by != 0, temp[:, y, :], 0.0)
            tk = np.where(on("dead-T"), temp[None, :, y, :], tk[None])
            dt = ct * by[None]
            dt = np.where(on("float-dtau"), dt.astype(np.float32).astype(np.float64), dt)
            om = -np.expm1(-np.minimum(dt, 800.0))
            om = np.where(on("exp64") & (dt >= 1e-6), 1.0 - np.exp(-dt), om)
            om = np.where(on("clamp30"), -np.expm1(-np.minimum(dt, 30.0)), om)
            if mistake == "slab-reset" and y and y % 16 == 0:
                Th = np.where(sel[None], 1.0, Th)
            Th_new = Th - Th * om
            I = I + (tk * om) * np.where(on("theta-first"), Th_new, Th)
            Th = Th_new
    hot = np.any(temp > 0.0, axis=1)
    return np.where(hot[None], np.asarray(csrc, dtype=np.float64)[:, None, None] * I, np.nan)


# ---- the inputs both test files run ---------------------------------------------------------------------
# 17 sightlines are 16 + 1 (the 16-sightline tile) and 2 x 8 + 1 (the 8-sightline tile of the 256-lane
# layout); 70 rows cross the 16- and 32-row slabs mid-sightline
NX, NY, NZ = 2, 70, 17
NYS, NZS = (1, 8, 33), (1, 7, 9)
NCHANS = (1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257)
INPUTS = ("spread", "spread1", "thick", "coldfront", "thin", "faint", "mixed")
CSIZE = 0.5
CTAU = 1e-20                                  # ctau of the channel the depths are designed at
N0, XI0 = 1e6, 0.3
T_EPOCH = 2.5 * YEAR
FAINT = 1e-6
THICK = (1.0, 5.0, 10.0, 20.0, 30.0, 37.0, 40.0, 800.0, 1e4)
THIN = (1e-320, 1e-300, 1e-17, 1e-8)          # sightlines 0-3; the others: 1e-6 ... 1e-4 per cell


def zero_channel(nchan):
    """Index of the channel with ctau = 0 (None for a single channel)."""
    return nchan // 3 if nchan > 1 else None


def channels(nchan):
    """(ctau, csrc): ctau falls from 2 to 0.5 times CTAU (nu^-2.1 over a band), one channel is 0."""
    if nchan == 1:
        return np.array([CTAU]), np.array([1.3])
    ctau = CTAU * np.geomspace(2.0, 0.5, nchan)
    ctau[zero_channel(nchan)] = 0.0
    return ctau, np.linspace(0.7, 1.9, nchan)


def case_bursts(name):
    """The (red, blue) burst lists of input `name`: 11 + 11 ("spread": the device overflow table),
    11 + 0 ("spread1"), the example's red jet alone ("mixed": NaN launch times in a jet with bursts
    and in one without), else the example's 2 + 3."""
    if name in ("spread", "spread1"):
        red, blue = F.burst_sets()["eleven"]
        return (red, blue) if name == "spread" else (red, [])
    if name == "mixed":
        return U.example_burst_lists(only="R")
    return U.example_burst_lists()


def case(name, nchan, ny=NY, nz=NZ, mode=0, bursts=True):
    """Host grids and channel tables of input `name` (INPUTS) -> dict: g (what RTEngine.upload_fields
    takes), bursts ((red, blue) lists, or None with bursts=False), t, ctau, csrc, mode, faint ([nx, nz]
    mask, or None), depth (the designed per-cell depths at ctau = CTAU).

    Every cell is given its T and the depth it is to have at CTAU and the case's epoch; its fill
    factor is what gives it that depth: ff = depth / (CTAU (nd xi)^2 T^-1.5|-1.35 chi^2)."""
    assert name in INPUTS, name
    rng = np.random.default_rng(5100 + 31 * INPUTS.index(name) + 7 * ny + nz)
    shape = (NX, ny, nz)
    row = np.arange(ny)[None, :, None]
    zz = np.arange(nz)[None, None, :]
    xx = np.arange(NX)[:, None, None]
    full = lambda a: np.broadcast_to(a, shape).copy()
    T = 10.0 ** rng.uniform(np.log10(300.0), np.log10(3e4), shape)
    depth = 10.0 ** rng.uniform(-3.5, -1.5, shape)
    ts = rng.uniform(0.0, 5.0 * YEAR, shape)
    red = full(zz < (nz + 1) // 2)
    lists = case_bursts(name) if bursts else None
    chi = np.ones(shape)
    faint = None
    dead = np.zeros(shape, dtype=bool)
    if name == "mixed":
        red = rng.random(shape) < 0.5
    if lists is not None:
        for lst, mask in ((lists[0], red), (lists[1], ~red)):
            if len(lst):
                chi[mask] = U.chi_exact(lst, T_EPOCH - ts[mask])
    if name in ("spread", "spread1"):         # 300 K ... 3e4 K in every sightline, chi^2 up to ~100
        T[:, -1, :] = 3e4
        if ny > 1:
            T[:, 0, :] = 300.0
        depth = depth / 30.0 * chi * chi
    elif name == "thick":
        # sightlines 0-8: one cell of THICK in front of (x = 0) or behind (x = 1) thin gas; 9-12 and
        # 13-16: every cell the same share of tau = 100 and 600, T rising 1e4 -> 3e4 K to the back
        T = 10.0 ** rng.uniform(np.log10(5e3), 4.0, shape)
        depth[:] = 2e-3
        edge = np.where(xx == 0, 0, ny - 1) + 0 * zz
        at = full((row == edge) & (zz < len(THICK)))
        T[at] = 3e4
        depth[at] = full(np.asarray(THICK)[np.minimum(zz, len(THICK) - 1)])[at]
        many = full(zz >= len(THICK))
        T[many] = full(10.0 ** (4.0 + 0.477 * row / max(ny - 1, 1)))[many]
        depth[many] = full(np.where(zz < len(THICK) + 4, 100.0, 600.0) / ny)[many]
    elif name == "coldfront":
        # a 300 K front cell of dtau = 20 (even z) / 30 (odd z) before 3e4 K gas (x = 0); x = 1: the
        # two-cell version, a 3e4 K cell of dtau = 0.5 behind it and nothing else
        T[:] = 3e4
        depth = 10.0 ** rng.uniform(-2.5, -1.5, shape)
        T[:, 0, :] = 300.0
        depth[:, 0, :] = full(np.where(zz % 2 == 0, 20.0, 30.0))[:, 0, :]
        if ny > 1:
            depth[1, 1, :] = 0.5
        dead = full((xx == 1) & (row >= 2))
    elif name == "thin":
        depth = 10.0 ** rng.uniform(-6.0, -4.0, shape)
        for k, v in enumerate(THIN):
            if k < nz:
                depth[:, :, k] = v
    elif name == "faint":                     # odd sightlines at 1e-6 of their even neighbours
        T = 10.0 ** rng.uniform(np.log10(3e3), np.log10(2e4), shape)
        depth = 10.0 ** rng.uniform(-3.0, -1.7, shape)
        faint = full(zz % 2 == 1)[:, 0, :]
        depth = np.where(faint[:, None, :], FAINT * depth, depth)
    p = float(F.POW[mode])
    with np.errstate(all="ignore"):
        ff = depth / (CTAU * (N0 * XI0) ** 2 * T ** p * chi * chi)
    g = dict(nd=np.full(shape, N0), xi=np.full(shape, XI0), temp=T, ff=ff, areas=np.ones(shape),
             ts=ts, rr=np.where(red, -1.0, 1.0), vy=None)
    g["nd"][dead] = np.nan
    if name == "mixed":
        # live and dead cells interleaved; NaN / 0 in each of nd, xi, temp, ff (temp = 0 next to
        # nd = 0: b stays NaN, not infinite); NaN launch times in both jets; an all-dead row inside
        # a slab; a sightline with no T > 0 (NaN) and one with T > 0 and nothing live (+0.0)
        kill = full((row + zz + xx) % 3 == 2)
        how = full((row // 3 + zz) % 8)
        for k, (key, v) in enumerate((("nd", np.nan), ("nd", 0.0), ("xi", np.nan), ("xi", 0.0),
                                      ("temp", np.nan), ("ff", np.nan), ("ff", 0.0), ("temp", 0.0))):
            g[key][kill & (how == k)] = v
        g["nd"][kill & (how == 7)] = 0.0
        g["ts"][full((7 * row + 3 * zz + xx) % 11 == 5)] = np.nan
        if ny > 20:
            g["nd"][:, 20, :] = np.nan
        g["nd"][0, :, 3 % nz] = np.nan
        g["temp"][0, :, 3 % nz] = np.nan
        g["nd"][1, :, 5 % nz] = 0.0
    if ny == 8:                               # the occupied range starts at row 3, mid-slab
        g["nd"][:, :3, :] = np.nan
        g["temp"][:, :3, :] = np.nan
    ctau, csrc = channels(nchan)
    return dict(name=name, g=g, bursts=lists, t=T_EPOCH, ctau=ctau, csrc=csrc, mode=mode,
                faint=faint, depth=depth)


def host_arrays(cs):
    """What the tau layout of an f64 upload holds, restated in NumPy: (a0, ts, temp)."""
    g = cs["g"]
    return U.golden_a0(g, 0.0 if cs["mode"] == 0 else -0.5), g["ts"], g["temp"]


def host_dev(cs, dtype=np.float32):
    """What an upload of the case's grids holds, as f32_ref.device_fields' dict (no device)."""
    return F.device_fields(F.host_fields(cs["g"], CSIZE, dtype))


def reference_of(cs, arrays):
    """The tau-layout reference of a case on (a0, ts, temp)."""
    a0, ts, temp = arrays
    return reference_tau(a0, ts, temp, cs["bursts"], cs["t"], cs["ctau"], cs["csrc"])
