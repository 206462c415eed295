"""Long-double reference of the RRL formal solution (rjp_rrl_formal, K6) with a derived per-pixel,
per-channel ABSOLUTE bound, and the hand-made inputs both test files run (tests only; NumPy and
scipy, nothing here imports the GPU package).  tests/test_rrl_formal_reference_cpu.py pins this
module (finite differences, a 40-digit mpmath evaluation, mutants), tests/test_gpu_rrl_formal_ld.py
holds the kernel to it.  It supplements rrl_formal_ref.within, whose absolute term is normalised to
the channel's brightest pixel and so lets any fainter pixel be wrong by max / |ref| times the bound.

Inputs: the float64 values of the device's field tensors (f32_ref.device_fields), so neither packing
nor f32 rounding is under test.

Per cell i and channel f, in numpy.longdouble:
    l_i   k3_voigt_ref.line_term_ref (its long-double term; Re w is scipy's wofz)
    c_i   f32_ref.cells_of on the wide layout, the continuum reference K5's tests use
    B_i   1 / expm1(hnu_k[f] / T_i)
NaN terms are dropped (nansum); a cell is live where c_i != 0 or l_i != 0; the map is NaN where no
cell of the sightline has T > 0.

The walk (`walk`) is the recurrence front to back, iy = 0 first:
    e_c = e^-c, om_l = 1 - e^-l, u = 1 - e^-(c + l)
    I += B (e_c om_l Theta_C - u D);  D = e_c (D + (Theta_C - D) om_l);  Theta_C *= e_c
`chains` forms I_tot - I_cont for the cross-check where tau_C <= 20.

Bound.  t = c + l; Theta_T,i, Theta_C,i the attenuations in front of cell i, D_i = Theta_C,i -
Theta_T,i; S_T,i = sum_{k > i} B_k (1 - e^-t_k) Theta_T,k, S_C,i the same with l == 0:
    dI/dl_i = B_i Theta_T,i+1 - S_T,i
    dI/dc_i = dI/dl_i - (B_i Theta_C,i+1 - S_C,i)  =  -B_i D_i+1 - sum_{k > i} B_k E_k
    dI/dB_i = E_i = (1 - e^-t_i) Theta_T,i - (1 - e^-c_i) Theta_C,i  =  e_c om_l Theta_T,i - om_c D_i
(the second forms are the ones evaluated: they do not subtract two chains), and
    bound = |csrc| [ sum_i eps_l,i l_i |dI/dl_i| + eps_c sum_i c_i |dI/dc_i| + sum_i eps_B,i B_i |E_i|
                     + rho 2^-53 sum_i B_i (e_c om_l Theta_C + u D)_i ]
  eps_l,i  k3_voigt_ref.tol(gpu_util.k3_rtol(nchan), ...) of that evaluation: the project's Voigt
           bound (1e-8 wave-uniform paths, 1e-9 per-lane code) plus the conditioning of Re w in x.
  eps_c    f32_ref.CELLS_RTOL.
  eps_B,i  the Planck expansion, as the code states it.  About x0 = h nu_ref / k T with
           d = (hnu_k[f] - h nu_ref / k) / T, |d| <= a dnu_max (a = h / k T):
             T e^-x0 expm1(x0 + d) = T ((1 - E0) + d + d^2 / 2 + d^3 / 6 + ...),  E0 = e^-x0.
           The wave-uniform layouts (nchan > 16) keep the first order while band_needs_exp
           (rrl_voigt.h) holds (a dnu_max)^2 / 2 < 2e-9 (1 - E0); the per-lane layout keeps the
           second order while (a dnu_max)^3 < 6e-11 (1 - E0) (rrl_formal.hip), i.e. d^3 / 6 <
           1e-11 (1 - E0).  With q = that quotient of the cell (< 1) the dropped term is below
           EPS_B q of 1 - E0, and the denominator itself is at least (1 - E0)(1 - a dnu_max /
           (1 - E0)):  eps_B,i = EPS_B min(q, 1) / (1 - a dnu_max / (1 - E0)).  Where the criterion
           fails the lanes call expm1 and only roundings are left.  EPS_B_ROUND = 16 * 2^-53 covers
           those on either path (a, its exponent, exp and expm1 at an ulp or two each, T times
           them, the FMA, the hardware reciprocal with its Newton step, the product).  A cell
           within 1e-9 of the threshold counts as expanded: the larger bound.
  rho      roundings.  With E = 37 >= 4e-15 / 2^-53, the relative error one_minus_exp_neg states
           for 1 - e^-x and e^-x (rjp_device.h), in units of 2^-53 and n = the live cells in front:
             Theta_C  gains E + 1 per update (e_c, the product):                 n (E + 1)
             D        = e_c (D (1 - om_l) + Theta_C om_l), both summands >= 0, so its relative
                      error is the larger of D's and Theta_C's plus om_l, e_c, the subtraction,
                      the FMA and the product:                                   n (2 E + 3)
             emission e_c om_l Theta_C: 2 E + 1, Theta_C's, the FMA:             2 E + 2 + n (E + 1)
             absorption u D: u = om_c + e_c om_l is 2 E + 2, the product, D's, the FMA
                                                                                 2 E + 4 + n (2 E + 3)
             the sum I: every later update rounds a partial sum that is at most the sum of the
                      magnitudes so far: one more per live cell behind.
           Every term's magnitude therefore carries at most (2 E + 4)(N + 1) roundings, N = the live
           cells of the sightline:  rho = PER_UPDATE (N + 1) + 1, PER_UPDATE = 2 E + 4 = 78, the
           last 1 for csrc I.  The term uses the magnitudes of emission and absorption, so it stays
           meaningful where a pixel passes through zero.
"""
import numpy as np

from tests import f32_ref as F
from tests import gpu_util as U
from tests import k3_voigt_ref as K

LD = np.longdouble
HAVE_LD = bool(np.finfo(LD).eps <= 2.0 ** -63)
LD_REASON = "numpy.longdouble is no wider than float64 on this host"
U0 = 2.0 ** -53
E_EXP = 37                                   # 4e-15 / 2^-53, rounded up
PER_UPDATE = 2 * E_EXP + 4
EPS_B_WAVE, CRIT_WAVE = 2e-9, 2e-9           # band_needs_exp: 0.5 (a dnu)^2 < 2e-9 (1 - E0)
EPS_B_LANE, CRIT_LANE = 1e-11, 6e-11         # rrl_formal.hip: (a dnu)^3 < 6e-11 (1 - E0)
EPS_B_ROUND = 16 * U0
TERMS = ("Voigt (eps_l)", "continuum (eps_c)", "Planck (eps_B)", "roundings (rho)")


# ---- per-cell quantities ----------------------------------------------------------------------------
def k3_fields(dev, bursts=None):
    """f32_ref.device_fields' dict -> the dict k3_voigt_ref.line_term_ref takes."""
    d = dict(nd=np.copysign(dev["nd"], np.where(dev["red"], -1.0, 1.0)), xi=dev["xi"],
             temp=dev["temp"], pf=dev["pf"], vy=dev["vy"],
             ts=dev["ts"] if dev["ts"] is not None else np.zeros(dev["shape"]),
             csize_au=dev["csize_au"])
    if bursts is not None:
        d["bursts"] = bursts
    return d


def planck_eps(temp, line, nu, nchan):
    """eps_B per cell [nx, ny, nz] (module docstring); nu_ref, dnu_max as fill_line forms them."""
    nu = np.asarray(nu, dtype=np.float64)
    nu_ref, dnu_max = 0.5 * (nu.min() + nu.max()), 0.5 * (nu.max() - nu.min())
    lane = K.lanes_per_block(nchan) == 16
    with np.errstate(all="ignore"):
        a = line["h_over_k"] / temp
        om = -np.expm1(-a * nu_ref)
        ad = a * dnu_max
        q = ad * ad * ad / (CRIT_LANE * om) if lane else 0.5 * ad * ad / (CRIT_WAVE * om)
        eps = (EPS_B_LANE if lane else EPS_B_WAVE) * np.minimum(q, 1.0) / (1.0 - ad / om)
        eps = np.where(q < 1.0 + 1e-9, eps, 0.0)
    return EPS_B_ROUND + np.where(np.isfinite(eps) & (eps > 0.0), eps, 0.0), q


def cell_quantities(dev, line, nu, ctau, hnu_k, mode, bursts=None, t=0.0):
    """-> dict: c, l, B (long double, [F, nx, ny, nz]; dropped terms are 0, B = 0 on dead cells),
    eps_l [F, nx, ny, nz], eps_B [nx, ny, nz], hot [nx, nz]."""
    nu = np.asarray(nu, dtype=np.float64)
    ref = K.line_term_ref(k3_fields(dev, bursts), line, nu, t)
    l = ref["term_ld"]
    with np.errstate(all="ignore"):
        eps_l = K.tol(U.k3_rtol(nu.size), ref["x"], ref["y"], ref["rew"], ref["imw"],
                      ref["nu0_is2"])
        c = F.cells_of(dev, mode, "wide", bursts if bursts is not None else ((), ()), t,
                       ctau).astype(LD)
        l = np.where(np.isnan(l), LD(0), l)
        c = np.where(np.isnan(c), LD(0), c)
        live = (c != 0) | (l != 0)
        B = 1 / np.expm1(np.asarray(hnu_k, dtype=np.float64).astype(LD)[:, None, None, None] /
                         dev["temp"].astype(LD)[None])
        B = np.where(live, B, LD(0))
    eps_B, _ = planck_eps(dev["temp"], line, nu, nu.size)
    return dict(c=c, l=l, B=B, eps_l=np.where(np.isfinite(eps_l), eps_l, 0.0), eps_B=eps_B,
                hot=np.any(dev["temp"] > 0.0, axis=1))


# ---- the walk -----------------------------------------------------------------------------------------
def walk(c, l, B):
    """The recurrence in the arrays' own type, front to back -> I [F, nx, nz]."""
    I = np.zeros(c.shape[:2] + c.shape[3:], dtype=c.dtype)
    D = np.zeros_like(I)
    Th = np.ones_like(I)
    for iy in range(c.shape[2]):
        ci, li, Bi = c[:, :, iy], l[:, :, iy], B[:, :, iy]
        e_c, om_l, u = np.exp(-ci), -np.expm1(-li), -np.expm1(-(ci + li))
        I = I + Bi * (e_c * om_l * Th - u * D)
        D = e_c * (D + (Th - D) * om_l)
        Th = Th * e_c
    return I


def _front(a):
    """Exclusive running sum along y: what lies in front of every cell."""
    s = np.cumsum(a, axis=2)
    return np.concatenate([np.zeros_like(s[:, :, :1]), s[:, :, :-1]], axis=2)


def _behind(a):
    """Exclusive running sum along y from the back: what lies behind every cell."""
    s = np.cumsum(a[:, :, ::-1], axis=2)[:, :, ::-1]
    return np.concatenate([s[:, :, 1:], np.zeros_like(s[:, :, :1])], axis=2)


def chains(c, l, B):
    """I_tot - I_cont, the two formal solutions formed and subtracted -> (difference, |I_tot|)."""
    tot = np.sum(B * -np.expm1(-(c + l)) * np.exp(-_front(c + l)), axis=2)
    cont = np.sum(B * -np.expm1(-c) * np.exp(-_front(c)), axis=2)
    return tot - cont, np.abs(tot)


def sensitivities(c, l, B):
    """One pass over the cells -> dict of [F, nx, ny, nz] arrays: dIdl, dIdc, E (= dI/dB) and mag =
    B (e_c om_l Theta_C + u D), the magnitudes of a cell's emission and absorption terms."""
    e_c, om_c, om_l = np.exp(-c), -np.expm1(-c), -np.expm1(-l)
    u = -np.expm1(-(c + l))
    ThC, tauL = np.exp(-_front(c)), _front(l)
    ThT = ThC * np.exp(-tauL)
    D = ThC * -np.expm1(-tauL)
    E = e_c * om_l * ThT - om_c * D
    own, rest = B * ThT * np.exp(-(c + l)), _behind(B * u * ThT)
    D_next = ThC * e_c * -np.expm1(-(tauL + l))
    dIdc = -B * D_next - _behind(B * E)
    # (scale_l, scale_c: the summands' magnitudes, for the finite-difference check of the formulas)
    return dict(dIdl=own - rest, dIdc=dIdc, E=E, mag=B * (e_c * om_l * ThC + u * D),
                scale_l=own + rest, scale_c=B * D_next + _behind(B * np.abs(E)))


def bound_terms(q, csrc, eps_l=None, eps_c=F.CELLS_RTOL, eps_B=None):
    """The four terms of the bound, each [F, nx, nz] float64 and times |csrc|: Voigt, continuum,
    Planck, roundings.  eps_* default to the cells' own (q = cell_quantities(...))."""
    c, l, B = q["c"], q["l"], q["B"]
    s = sensitivities(c, l, B)
    eps_l = q["eps_l"] if eps_l is None else eps_l
    eps_B = q["eps_B"][None] if eps_B is None else eps_B
    cs = np.abs(np.asarray(csrc, dtype=np.float64)).astype(LD)[:, None, None]
    n_live = np.sum((c != 0) | (l != 0), axis=2)
    rho = PER_UPDATE * (n_live + 1) + 1
    terms = (np.sum(eps_l * l * np.abs(s["dIdl"]), axis=2),
             eps_c * np.sum(c * np.abs(s["dIdc"]), axis=2),
             np.sum(eps_B * B * np.abs(s["E"]), axis=2),
             rho * U0 * np.sum(s["mag"], axis=2))
    return [(cs * t).astype(np.float64) for t in terms]


def reference(dev, line, nu, ctau, csrc, hnu_k, mode, bursts=None, t=0.0):
    """-> dict: ref [F, nx, nz] float64 (NaN where the sightline has no T > 0), ref_ld, terms (the
    four of the bound), bound, q (the per-cell quantities)."""
    q = cell_quantities(dev, line, nu, ctau, hnu_k, mode, bursts, t)
    I = np.asarray(csrc, dtype=np.float64).astype(LD)[:, None, None] * walk(q["c"], q["l"], q["B"])
    I = np.where(q["hot"][None], I, LD("nan"))
    terms = bound_terms(q, csrc)
    return dict(ref=I.astype(np.float64), ref_ld=I, terms=terms, bound=sum(terms), q=q)


def judge(got, r, what=""):
    """Identical NaN patterns and |got - ref| <= bound on every pixel and channel (exactly 0 where the
    bound is 0) -> (worst share of the bound, name of the term that dominates the bound there)."""
    ref, bound = r["ref_ld"], r["bound"]
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    err = np.where(ok, np.abs(got.astype(LD) - ref).astype(np.float64), 0.0)
    assert np.all(err[ok & (bound == 0.0)] == 0.0), what
    share = np.where(ok & (bound > 0.0), err / np.where(bound > 0.0, bound, 1.0), 0.0)
    i = np.unravel_index(np.argmax(share), share.shape)
    top = TERMS[int(np.argmax([t[i] for t in r["terms"]]))]
    return float(share[i]), top, i


# ---- the inputs both test files run ---------------------------------------------------------------------
# 70 rows cross the slabs of 8, 16 and 32 rows mid-sightline; 17 sightlines are 16 + 1 (ZT = 16) and
# 4 x 4 + 1 (ZT = 4)
NX, NY, NZ = 2, 70, 17
CSIZE = K.CSIZE_AU
MODE = 0                     # RJP_GFF_SCALAR: T^-1.5
YEAR = 31536000.0
NCHANS = (1, 16, 17, 64, 65, 128, 129, 256, 257)
INPUTS = ("spread", "thick", "thickline", "faint", "mixed", "band0.9", "band1.1", "wide")
FAINT = 1e-6
THICK_C = (1.0, 5.0, 10.0, 20.0, 30.0)


def _unit(line, T, y, nu_c):
    """(l, b) of one cell at (T, y) with pf = 1 at the line centre: line depth and (|nd| xi)^2 T^-1.5."""
    g = K.host_fields(np.array([[[float(y)]]]), float(T), line)
    l = K.line_term_ref(K.as_device_fields(g), line, [nu_c])["term"][0, 0, 0, 0]
    return float(l), float((g["nd"] * g["xi"])[0, 0, 0] ** 2 * T ** -1.5)


def channels(line, nchan, band):
    """`band`: "narrow" = +-1e-3 about the line centre, "wide" = 0.7 ... 1.3 of it, a number = the
    half width at which band_needs_exp's quotient is that number for a 300 K cell."""
    nu_c, _ = K.line_centre(line, 1e4)
    if nchan == 1:
        return nu_c, np.array([nu_c])
    if band == "narrow":
        return nu_c, nu_c * (1.0 + np.linspace(-1e-3, 1e-3, nchan))
    if band == "wide":
        return nu_c, nu_c * np.linspace(0.7, 1.3, nchan)
    dnu = K.band_halfwidth(line, 300.0, nu_c, float(band))
    return nu_c, np.linspace(nu_c - dnu, nu_c + dnu, nchan)


def case(name, line, nchan, ny=NY, band=None):
    """Host grids and channel tables of input `name` (INPUTS) for `nchan` channels.
    -> dict: g (what RTEngine.upload_fields takes), bursts ((red, blue) lists or None), t, nu, ctau,
    csrc, hnu_k, mode, faint ([nx, nz] mask of the sightlines made faint, or None).

    Every cell is given its temperature, its Voigt y (k3_voigt_ref.host_fields turns y into a
    density) and the continuum depth `c` it is to have at the line centre; its fill factor is what
    gives it that depth once ctau is fixed by `ratio`, the c / l of a (1e4 K, y = 0.1) cell at the
    line centre.  l follows: roughly c / l ~ ratio (T / 1e4) Re w(0, 0.1) / Re w(x, y)."""
    rng = np.random.default_rng(6000 + 17 * INPUTS.index(name) + ny)
    shape = (NX, ny, NZ)
    row = np.arange(ny)[None, :, None]
    zz = np.arange(NZ)[None, None, :]
    xx = np.arange(NX)[:, None, None]
    T = 10.0 ** rng.uniform(np.log10(300.0), np.log10(3e4), shape)
    y = 10.0 ** rng.uniform(-2.5, 0.7, shape)
    c = 10.0 ** rng.uniform(-3.5, -1.5, shape) * (T / 3e4)       # (l then spreads as evenly as c)
    vy = K.VY + rng.normal(0.0, 5.0, shape)
    ts, bursts, t, ratio, faint = np.zeros(shape), None, 0.0, 1.0, None
    if band is None:
        band = {"band0.9": 0.9, "band1.1": 1.1, "wide": "wide"}.get(name, "narrow")
    if name == "spread":                      # (a): 300 K ... 3e4 K in every sightline, 11 + 11 bursts
        ts = rng.uniform(0.0, 5.0 * YEAR, shape)
        bursts, t = F.burst_sets()["eleven"], 2.5 * YEAR
        T[:, -1, :] = 3e4
        T[:, 0, :] = 300.0
        c = c / 30.0                          # (chi^2 reaches ~100)
    elif name == "thick":
        # (b): one thick cell (3e4 K, y = 10, c / l = 100) in front of (x = 0) or behind (x = 1) thin
        # gas, c = THICK_C by sightline; sightlines 10-12 and 13-15: 70 cells of tau_C = 100 and 600
        nu_c = K.line_centre(line, 1e4)[0]
        l_hot, b_hot = _unit(line, 3e4, 10.0, nu_c)
        l_ref, b_ref = _unit(line, 1e4, 0.1, nu_c)
        ratio = 100.0 * (l_hot / b_hot) * (b_ref / l_ref)
        T[:] = 10.0 ** rng.uniform(np.log10(5e3), 4.0, shape)
        y[:], c[:], vy[:] = 0.1, 2e-3, K.VY
        edge = np.where(xx == 0, 0, ny - 1) + 0 * zz
        at = (row == edge) & (zz < 10) | (row == edge) & (zz == 16)
        T[at], y[at] = 3e4, 10.0
        c[at] = np.broadcast_to(np.asarray(THICK_C)[zz % 5], shape)[at]
        many = np.broadcast_to((zz >= 10) & (zz < 16) & (row >= 0), shape)
        T[many] = np.broadcast_to(10.0 ** (4.0 + 0.477 * row / max(ny - 1, 1)), shape)[many]
        y[many] = 10.0
        c[many] = np.broadcast_to(np.where(zz < 13, 100.0, 600.0) / ny, shape)[many]
    elif name == "thickline":                 # (c): per-cell l up to 50, cold gas in front of hot gas
        cold = np.broadcast_to((row >= ny // 2 - 3) & (row < ny // 2 + 2), shape)
        hot = np.broadcast_to(row >= ny // 2 + 2, shape)
        T[:] = np.where(hot, 2e4, np.where(cold, 300.0 + 100.0 * (row % 8), 1e3))
        y[:], vy[:] = 0.1, K.VY
        nu_c = K.line_centre(line, 1e4)[0]
        l300, b300 = _unit(line, 300.0, 0.1, nu_c)
        l_ref, b_ref = _unit(line, 1e4, 0.1, nu_c)
        c_for_50 = 50.0 * (b300 / l300) * (l_ref / b_ref)                 # c of a 300 K cell with l = 50
        c[:] = np.where(hot, 0.05, np.where(cold, c_for_50 * 10.0 ** (-zz / 4.0), 1e-4))
    elif name in ("faint", "band0.9", "band1.1", "wide"):
        # (d), (f): odd sightlines at 1e-6 of their neighbours; every seventh row at 300 K
        T[:] = 10.0 ** rng.uniform(np.log10(300.0 if name != "faint" else 3e3), np.log10(2e4), shape)
        T[:, ::7, :] = 300.0
        c[:] = 10.0 ** rng.uniform(-3.0, -1.7, shape) * (T / 3e4)
        faint = np.broadcast_to((zz % 2 == 1), shape)[:, 0, :].copy()
        c = np.where(faint[:, None, :], FAINT * c, c)
    else:
        assert name == "mixed", name          # (e): live, continuum-only and dead cells interleaved
    g = K.host_fields(y, T, line, ts=ts)
    g["vy"] = vy
    nu_c, nu = channels(line, nchan, band)
    l_ref, b_ref = _unit(line, 1e4, 0.1, nu_c)
    ctau_c = ratio * l_ref / b_ref
    with np.errstate(all="ignore"):
        g["ff"] = c / (ctau_c * (g["nd"] * g["xi"]) ** 2 * T ** -1.5)     # (depths are those of chi = 1)
    if name == "mixed":
        kind = (row + zz + xx) % 4
        g["vy"] = np.where(kind == 1, np.nan, g["vy"])                    # C = 0, b != 0
        dead = np.broadcast_to(kind == 2, shape)
        how = np.broadcast_to((row // 4 + zz) % 6, shape)
        g["nd"] = np.where(dead & (how == 0), np.nan, np.where(dead & (how == 1), 0.0, g["nd"]))
        g["temp"] = np.where(dead & (how == 2), np.nan, g["temp"])
        g["ff"] = np.where(dead & (how == 3), np.nan, np.where(dead & (how == 4), 0.0, g["ff"]))
        g["xi"] = np.where(dead & (how == 5), np.nan, g["xi"])
        g["nd"][0, :, 3] = np.nan                                         # NaN: no cell with T > 0
        g["temp"][0, :, 3] = np.nan
        g["nd"][1, :, 5] = 0.0                                            # 0: T > 0, nothing live
    if ny == 8:                               # the occupied range starts mid-slab
        g["nd"][:, :3, :] = np.nan
        g["temp"][:, :3, :] = np.nan
    ctau = ctau_c * (nu / nu_c) ** -2.1
    if name == "mixed" and nchan > 1:
        # line-only cells: the fields admit none (every factor of b is one of C), a channel does
        ctau[-1] = 0.0
    return dict(g=g, bursts=bursts, t=t, nu=nu, ctau=ctau, csrc=(nu / nu_c) ** 3,
                hnu_k=line["h_over_k"] * nu, mode=MODE, faint=faint)


def host_dev(cs, dtype=np.float64):
    """What an upload of the case's grids holds, as f32_ref.device_fields' dict (no device)."""
    return F.device_fields(F.host_fields(cs["g"], CSIZE, dtype))


def reference_of(cs, dev, line):
    return reference(dev, line, cs["nu"], cs["ctau"], cs["csrc"], cs["hnu_k"], cs["mode"],
                     cs["bursts"], cs["t"])
