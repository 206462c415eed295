"""Reference and derived bounds for the EPOCH SWEEPS (tests only; plain NumPy, nothing here imports
the GPU package): the epoch tiles of ff_scan_kernels.h (direct evaluation, the two- and the
three-operation uniform-spacing recurrences), K1m (ff_moments.hip), K1m-LT (ff_lt.hip), the cached
contraction and the light curves K2 makes of their sums.  tests/test_epoch_sweep_reference_cpu.py
pins this module, tests/test_gpu_epoch_sweep_reference.py holds the kernels to it.

Reference: gpu_util.ref_single_epoch looped over the epochs, on the arrays read back from the device
(long-double sums, numpy.exp, nansum semantics).  It shares nothing with the kernels.

Bound, per pixel and epoch, ABSOLUTE (tests/f32_ref.py's form, generalised to one delta per burst):
    chi_dev = 1 + sum_b amp_b g_b (1 + eps_b),  |eps_b| <= delta_b,   D = sum_b |amp_b| g_b delta_b
    |chi_dev^2 - chi^2| <= 2 |chi| D + D^2
    B = sum_y w (2 |chi| D + D^2) + r sum_y w chi^2
It stays meaningful where a dip takes chi through 0.  u = 2^-53 is one rounding; ln g = -d^2 inv,
inv = 1 / (2 sigma^2), d = (t - ts) - t0.  Arguments of exponentials carry RELATIVE errors, so an
exponential's error is (relative error of its argument) x |ln of its value|.

Common to every tile path
  the reference's own g   -(d^2) / (2 sigma^2) has three roundings beside the one of 2 sigma^2 that
                          make_bursts shares, numpy.exp is good to an ulp: (4 ln g + 2) u.
  inv2s2 as handed over   1 / (2 sigma^2) in Python: <= 3 u (e_i).  EVERY exponent of a path is
                          proportional to it, so it moves the product by e_i ln g: 3 u ln g.
  k2 = -inv2s2 log2(e)    the constant's representation and one product: 2 u (e_L), on the
                          exponents formed from k2.
  the sum over bursts     n_b FMAs (or adds), each rounding a partial sum <= 1 + S, S = sum |amp| g:
                          D += n_b u (1 + S).
  r                       tau layout: chi chi, the FMA into the accumulator, a sum of n_y terms and
                          of the y-ranges: (n_y + 4) u.  Compact / wide layouts form the weight on
                          the device (pow_m1p5 < 1e-13): f32_ref.tau_rtol / em_rtol.

direct tiles (chi_batch, exp2_gauss: no `un`)
  d is formed exactly as the reference forms it, (t - ts) - t0.  exp2_gauss((d d) k2): two roundings
  of the argument + e_L + e_i = 7 u ln g, the degree-8 polynomial 1.1e-12 (rjp_device.h), its last
  FMA.  With the reference's share:
      delta_direct = 1.1e-12 + (11 ln g + 4) u
  -- 1.14e-12 at g = 1e-17 (ln g = 39); the clamp at 2^-1021 is 4e-308 absolute.

recurrence, two-operation path (chi_batch_uniform, waves inside one jet)
  E_{m+-j} = amp E_m rup^{+-j} T_j with E_m = exp2(k2 vm^2), rup = exp2(a1 (vm + hdt)),
  a1 = 2 k2 dt, T_j = exp(-inv dt^2 j (j -+ 1)) from the host's step table, vm = (t_m - ts) - t0.
  ln E_m = vm^2 inv, ln rup = 2 inv dt |vm + dt / 2|, ln T_j = inv dt^2 j (j -+ 1); the three
  exponents add up to ln g of the implied argument d' = vm +- j dt.
    E_m            (vm vm) k2: 2 u ln E_m; degree-10 polynomial 4e-16 + its last FMA
    rup^j          (vm + hdt) a1 with a1 itself rounded: 3 u per step = 3 u j ln rup; the polynomial
                   and its FMA per factor: j (4e-16 + u); j multiplications: j u
    Newton 1/rup   v_rcp_f64 (an ulp) + one step: 2 u per factor of the chain to earlier epochs: 2 j u
    e_L            on E_m rup^j only, whose exponents sum to ln g - ln T_j: 2 u |ln T_j - ln g|
    T_j            -inv dt dt (double)(j (j -+ 1)): 3 u ln T_j; std::exp: 2 u
    amp E_m, the FMA, the reference's 2 u: 4 u
    d' against d   the implied argument is vm +- j dt with the HOST's dt = (t_last - t_first) /
                   (ET - 1); the reference rounds (t_e - ts) - t0 at epoch e itself.  |d' - d| <=
                   dd = 2 dev + u (|t_e - ts| + |d| + |t_m - ts| + |vm|) + 2 u j |dt|, dev = the
                   tile's measured departure from uniform spacing (uniform_tile admits 8 ulp of the
                   largest epoch; the bound takes what the epochs have).  dg / g = 2 inv |d| dd.
      delta_2 = u (7 ln g + 2 |ln T_j - ln g| + 2 ln E_m + 3 j ln rup + 3 ln T_j)
                + (j + 1) 4e-16 + (4 j + 8) u + 2 inv |d| dd
    At the 28 sigma limit (j dt = 28 sigma) with the burst peaking at the tile's edge (g = 1,
    vm = 28 sigma): u (2 392 + 2 392 + 3 784 + 3 392) = 5100 u = 5.7e-13.  An anchor below
    2^-1009 (kDead) adds exactly nothing at every epoch of the tile: delta = 1 there; the 28 sigma
    rule keeps such a cell's g below e^-44.

recurrence, three-operation path (waves that straddle the red / blue plane)
  the same anchors, but q^(j (j -+ 1) / 2) comes from the chains ru *= q, rd *= q: j (j -+ 1) / 2
  factors q, each with std::exp's 2 u and one multiplication -- QUADRATIC in j -- and rdn = q / rup
  costs one more rounding per step:
      delta_3 = delta_2 + 1.5 u j (j + 1) + j u                  (4.7e-14 more at j = 16)

moment paths (K1m, K1m-LT, cached)
  B = RJP_MOM_TOL sum_y w F                                     the project's acceptance threshold
      + (n_y + 2 N + 8) u sum_bins M0_bin sum_n |W_n,bin|       moments, recurrence, contraction
      + sum_y w |dF/ds| ds                                      the launch-time coordinate
  The last two are the "rounding term".  Its first part is computed from mom_tables_host's
  coefficients and the per-bin weights of the sightline.  Its second part: the bin coordinate
  (ts - s0) inv_h and the table's nodes round the launch time by ds <= 8 u (span + |s0| + |t_e|)
  (three roundings of the coordinate, two of a node, the reference's own two), and
  |dF/ds| <= 2 |chi| sum_b |amp_b| g_b 2 inv_b |d_b|.

light curves
  flux_p = cflux T_avg (1 - e^-tau_p), tau_p = ctau A_p: |dflux_p| <= cflux |T_avg| e^-tau_p ctau B_p;
  the map stage's 1 - e^-tau is good to 4e-15, the total is a sum of P terms:
      B_F = sum_p cflux |T_avg| e^-tau_p ctau B_p + (4e-15 + (P + 4) u) sum_p |flux_p|
"""
import math

import numpy as np

from oracle import rt_oracle as orc
from tests import ff_grad_ref as G
from tests import gpu_util as U

EPS = 2.0 ** -53
POLY8 = 1.1e-12                  # exp2_gauss: degree 8 on |f| <= 1/2 (rjp_device.h)
POLY10 = 4e-16                   # exp2_poly: degree 10
MOM_TOL = 1e-11                  # RJP_MOM_TOL (rjp_host.h)
MOM_SHAPES = ((80, 8), (53, 12), (39, 16))      # kMomShapes, cheapest first
MOM_NMAX = 32                    # RJP_MOM_NMAX
SIGMA_LIMIT = 28.0               # uniform_tile: half-span <= 28 sigma of the narrowest burst
LN_DEAD = 1009.0 * math.log(2.0)                # kDead, as a natural logarithm
DIRECT, TWO_OP, THREE_OP = 0, 2, 3


def inv2s2(sigma):
    """1 / (2 sigma^2) exactly as engine.make_bursts forms it."""
    return 1.0 / (2.0 * float(sigma) ** 2.0)


def sigma_of(hl_yr):
    return hl_yr * orc.YEAR * 2. / (2. * np.sqrt(2. * np.log(2.)))


# ---- reference -----------------------------------------------------------------------------------
def ref_sweep(a0, ts, bursts, epochs, threads=8):
    """[E, n_x, n_z]: gpu_util.ref_single_epoch at every epoch."""
    return np.stack([U.ref_single_epoch(a0, ts, bursts, float(t), threads=threads) for t in epochs])


def ref_sweep_em(em0, ts, bursts, epochs, csize_au, threads=8):
    """The emission-measure maps: the same sums over em0, times csize au / pc as the library forms
    it (ff_scan.hip `em_scale`)."""
    return ref_sweep(em0, ts, bursts, epochs, threads) * \
        (float(csize_au) * 149597870700.0 / 3.085677581491367e+16)


def light_curves(sums, tavg, ctau, cflux):
    """Map formulas + long-double totals (ff_grad_ref.totals) on [E, n_x, n_z] sums ->
    (F[E, n_f], absF[E, n_f])."""
    F, A = [], []
    for s in sums:
        none = np.zeros((1,) + s.shape)                          # (no derivative planes here)
        tot = G.totals({"S": s, "D": none, "absD": none}, tavg, ctau, cflux)
        F.append(tot["F"])
        A.append(tot["absF"])
    return np.array(F), np.array(A)


def light_curve_bound(sums, bound, tavg, ctau, cflux):
    """B_F[E, n_f] of the module docstring from the reference sums and their pixel bounds."""
    ta = np.asarray(tavg, dtype=np.float64).ravel()
    ta = np.abs(np.where(np.isnan(ta), 0.0, ta))
    P = ta.size
    out = np.zeros((len(sums), len(ctau)))
    for e in range(len(sums)):
        A, B = sums[e].ravel(), bound[e].ravel()
        for f in range(len(ctau)):
            tau = ctau[f] * A
            flux = cflux[f] * ta * (-np.expm1(-tau))
            out[e, f] = np.sum(cflux[f] * ta * np.exp(-tau) * ctau[f] * B) + \
                (4e-15 + (P + 4) * EPS) * np.sum(np.abs(flux))
    return out


# ---- host restatement of ff_scan_plan / uniform_tile -----------------------------------------------
def _all_inv(bursts):
    return [inv2s2(sg) for lst in bursts for _, _, sg in lst]


def tile_spacing(t):
    """(dt, dev) of a tile as uniform_tile measures them."""
    et = len(t)
    dt = (t[et - 1] - t[0]) / (et - 1)
    dev = max(abs(t[e] - (t[0] + e * dt)) for e in range(et))
    return dt, dev


def uniform_tile_host(t, bursts):
    """May the tile of epochs `t` use the recurrence?  (et >= 4, uniform to 8 ulp of the largest
    epoch, half-span <= 28 sigma of every burst.)"""
    et = len(t)
    invs = _all_inv(bursts)
    if et < 4 or not invs:
        return False
    dt, dev = tile_spacing(t)
    tmax = max(abs(x) for x in t)
    if not dev <= 8.0 * 2.220446049250313e-16 * tmax:
        return False
    m = et // 2
    half = max(m, et - 1 - m) * abs(dt)
    for inv in invs:
        if not inv > 0.0:
            return False
        if not half <= SIGMA_LIMIT * math.sqrt(0.5 / inv):
            return False
    return True


def tile_plan_host(epochs, bursts, dtype=8, layout="tau", want_em=False, nz=2, aligned=True):
    """[(e0, et, uniform, vec)] as ff_scan_plan cuts a sweep: long tiles (16 / 32 epochs, uniform
    spacing only) for f64 storage on the tau and compact layouts; 8-epoch tiles unless the lanes are
    4 sightlines wide; `vec` = the lane width dispatched (1 for et >= 16).  `want_em` does not change
    the plan (the 32-epoch tile with EM maps is a kernel of its own)."""
    epochs = [float(t) for t in epochs]
    n = len(epochs)
    full = 2 if dtype == 8 else 4
    vec = full if (nz % full == 0 and aligned) else 1
    if not _all_inv(bursts):
        return [(0, 1, 0, vec)]
    long_tiles = dtype == 8 and layout != "wide"
    out, e0 = [], 0
    while e0 < n:
        left = n - e0
        et = 8 if (left >= 8 and vec != 4) else 4 if left >= 4 else 2 if left >= 2 else 1
        if left >= 16 and long_tiles and uniform_tile_host(epochs[e0:e0 + 16], bursts):
            et = 16
        if left >= 32 and long_tiles and uniform_tile_host(epochs[e0:e0 + 32], bursts):
            et = 32
        un = uniform_tile_host(epochs[e0:e0 + et], bursts)
        out.append((e0, et, int(un), vec if et < 16 else 1))
        e0 += et
    return out


def wave_mixed(red_pix, vec):
    """[n_x, n_z] bool: does the wave that owns the sightline hold both jets?  A wave is 64 lanes of
    `vec` consecutive sightlines (p = x n_z + z); `red_pix` [n_x, n_z] is the jet of each sightline
    (sightlines whose jet changes along y: pass None -- every wave straddles)."""
    flat = np.asarray(red_pix, dtype=bool).ravel()
    grp = np.arange(flat.size) // (64 * vec)
    n = grp.max() + 1
    any_red = np.bincount(grp, weights=flat, minlength=n) > 0
    any_blue = np.bincount(grp, weights=~flat, minlength=n) > 0
    return (any_red & any_blue)[grp].reshape(np.shape(red_pix))


# ---- the tile bound --------------------------------------------------------------------------------
def delta_direct(lng):
    return POLY8 + (11.0 * lng + 4.0) * EPS


def delta_recurrence(j, d, vm, tl, tlm, inv, dt, dev, three):
    """delta_2 / delta_3 of the module docstring for the epoch j steps from the anchor (signed)."""
    J = abs(j)
    lng = d * d * inv
    lnEm = vm * vm * inv
    lnrup = 2.0 * inv * abs(dt) * np.abs(vm + 0.5 * dt)
    lnT = inv * dt * dt * J * (J - 1 if j > 0 else J + 1)
    dd = 2.0 * dev + EPS * (np.abs(tl) + np.abs(d) + np.abs(tlm) + np.abs(vm)) + 2.0 * EPS * J * abs(dt)
    dl = EPS * (7.0 * lng + 2.0 * np.abs(lnT - lng) + 2.0 * lnEm + 3.0 * J * lnrup + 3.0 * lnT) + \
        (J + 1) * POLY10 + (4 * J + 8) * EPS + 2.0 * inv * np.abs(d) * dd
    if three:
        dl = dl + EPS * (1.5 * J * (J + 1) + J)
    # an anchor at (or, to rounding, near) kDead: the cell may add exactly nothing
    return np.where(lnEm >= LN_DEAD - 0.5, 1.0, dl)


def tile_bound(w0, ts, bursts, epochs, tiles, ref, round_rel, mixed=None):
    """-> (B[E, n_x, n_z], path[E, n_x, n_z]): the pixel bound for a sweep cut into `tiles`
    (tile_plan_host's rows, or the device's), and the path each (epoch, pixel) ran: DIRECT, TWO_OP or
    THREE_OP.  `w0`: the signed weights (jet in the sign bit); `ref`: the reference sums (already
    scaled like the device's output; `w0` is scaled with `scale` = ref's scale by the caller);
    `round_rel`: r of the module docstring; `mixed`: None = sightlines of one jet each (the waves'
    jets follow from wave_mixed), True = every wave straddles."""
    w0 = np.asarray(w0, dtype=np.float64)
    ts = np.asarray(ts, dtype=np.float64)
    red = np.signbit(w0)
    w = np.abs(w0)
    E = len(epochs)
    B = np.zeros((E,) + ref.shape[1:])
    path = np.zeros(B.shape, dtype=np.int64)
    par = [[(float(t0), float(amp), inv2s2(sg)) for t0, amp, sg in lst] for lst in bursts]
    for row in tiles:
        e0, et, uniform, vec = row[0], row[1], row[2], row[-1]
        t_tile = [float(t) for t in epochs[e0:e0 + et]]
        if uniform:
            dt, dev = tile_spacing(t_tile)
            m = et // 2
            if mixed is None:
                assert np.array_equal(red, np.broadcast_to(red[:, :1, :], red.shape)), \
                    "the jet changes along y: pass mixed=True"
                three = wave_mixed(red[:, 0, :], vec)[:, None, :] & np.ones(w.shape, dtype=bool)
            else:
                three = np.ones(w.shape, dtype=bool)
        for k, t in enumerate(t_tile):
            with np.errstate(all="ignore"):
                tl = t - ts
                chi, S, D = np.ones(w.shape), np.zeros(w.shape), np.zeros(w.shape)
                for lst, mask in ((par[0], red), (par[1], ~red)):
                    for t0, amp, inv in lst:
                        d = tl[mask] - t0
                        lng = d * d * inv
                        g = np.exp(-lng)
                        if uniform:
                            tlm = t_tile[m] - ts[mask]
                            vm = tlm - t0
                            a = (d, vm, tl[mask], tlm, inv, dt, dev)
                            dl = np.where(three[mask], delta_recurrence(k - m, *a, True),
                                          delta_recurrence(k - m, *a, False))
                        else:
                            dl = delta_direct(lng)
                        chi[mask] += amp * g
                        S[mask] += abs(amp) * g
                        D[mask] += abs(amp) * g * np.minimum(dl, 1.0)
                    if lst:
                        D[mask] += len(lst) * EPS * (1.0 + S[mask]) + 1e-300
                dropped = np.isnan(w * (chi * chi)) | np.isinf(w)       # nansum drops these terms
                term = np.where(dropped, 0.0, w * (2.0 * np.abs(chi) * D + D * D))
            B[e0 + k] = term.sum(axis=1) + round_rel * ref[e0 + k]
            if uniform:
                path[e0 + k] = np.where(three[:, 0, :], THREE_OP, TWO_OP)
    return B, path


# ---- NumPy emulation of chi_batch_uniform ---------------------------------------------------------------
LOG2E = 1.4426950408889634074


def emulate_recurrence(tlm, t0, amp, sigma, dt, et, three, rng=None, step_err=0.0, drop_hdt=False):
    """amp g at the `et` epochs of a uniform tile for cells with anchor arguments `tlm` = t_m - ts,
    in float64 in the order of chi_batch_uniform (rjp_device.h): the two-operation path (step table)
    or, `three`, the q chains.  numpy.exp2 stands in for the device polynomials, perturbed by their
    stated relative size (4e-16, uniformly drawn from `rng`; None: unperturbed).  Planted mistakes:
    `step_err` multiplies the step ratio by 1 + step_err; `drop_hdt` forms it from vm a1 instead of
    (vm + hdt) a1.  -> [et, n_cells]."""
    tlm = np.asarray(tlm, dtype=np.float64)
    inv = inv2s2(sigma)
    k2 = -inv * LOG2E
    a1 = 2.0 * k2 * dt
    hdt = 0.5 * dt
    M = et // 2
    wob = (lambda n: 1.0 + POLY10 * rng.uniform(-1.0, 1.0, n)) if rng is not None else (lambda n: 1.0)
    out = np.zeros((et, tlm.size))
    with np.errstate(all="ignore"):
        vm = tlm - t0
        tm = (vm * vm) * k2
        dead = tm < -1009.0
        em = np.exp2(np.maximum(tm, -1021.0)) * wob(tlm.size)
        rup = np.exp2((vm if drop_hdt else (vm + hdt)) * a1) * wob(tlm.size) * (1.0 + step_err)
        ir = 1.0 / rup
        ir = ir * (2.0 - rup * ir)
        if not three:
            tab = [math.exp(-inv * dt * dt * float(k * (k + 1))) for k in range(1, 17)]
            ae = np.where(dead, 0.0, amp * em)
            out[M] = ae
            eu, ed = ae.copy(), ae.copy()
            ru, rd = np.where(dead, 0.0, rup), np.where(dead, 0.0, ir)
            for j in range(1, M + 1):
                if M + j < et:
                    eu = eu * ru
                    out[M + j] = eu if j == 1 else eu * tab[j - 2]
                ed = ed * rd
                out[M - j] = ed * tab[j - 1]
        else:
            q = math.exp(-2.0 * inv * dt * dt)
            a = np.where(dead, 0.0, amp)
            em0 = np.where(dead, 0.0, em)
            out[M] = a * em0
            eu, ed = em0.copy(), em0.copy()
            ru, rd = np.where(dead, 0.0, rup), np.where(dead, 0.0, q * ir)
            for j in range(1, M + 1):
                if M + j < et:
                    eu = eu * ru
                    ru = ru * q
                    out[M + j] = a * eu
                ed = ed * rd
                rd = rd * q
                out[M - j] = a * ed
    return out


# ---- host restatement of mom_tables_kernel and of the shape choice -----------------------------------
def _burst_F(lst, tl):
    chi = np.ones_like(tl)
    for t0, amp, sg in lst:
        d = tl - t0
        chi = chi + amp * np.exp(-d * d * inv2s2(sg))
    return chi * chi


def mom_table(bursts, epochs, ts_range, K, N, dense=None):
    """One (K, N) shape: -> (W[2, K, N, E], worst) as mom_tables_kernel builds and checks them (the
    DCT of N node values per (jet, bin, epoch); the interpolant against F at 2 N + 1 equispaced
    points, relative); `dense`: check at dense N + 1 points instead."""
    lo, hi = ts_range
    span = hi - lo
    h = span / K
    te = np.asarray(epochs, dtype=np.float64)
    xn = np.cos(np.pi * (np.arange(N) + 0.5) / N)
    cs = np.cos(np.pi * np.arange(N)[:, None] * (np.arange(N)[None, :] + 0.5) / N)      # [n, m]
    ck = lo + (np.arange(K) + 0.5) * h
    W = np.zeros((2, K, N, len(te)))
    worst = 0.0
    NT = (dense * N + 1) if dense else 2 * N + 1
    xv = -1.0 + 2.0 * np.arange(NT) / (NT - 1)
    for j in range(2):
        if not bursts[j]:
            W[j, :, 0, :] = 1.0
            continue
        s = ck[:, None] + 0.5 * h * xn[None, :]                                         # [K, m]
        f = _burst_F(bursts[j], te[None, None, :] - s[:, :, None])                       # [K, m, E]
        cf = np.einsum("nm,kme->kne", cs, f) * (2.0 / N)
        cf[:, 0, :] *= 0.5
        W[j] = cf
        sv = ck[:, None] + 0.5 * h * xv[None, :]
        refv = _burst_F(bursts[j], te[None, None, :] - sv[:, :, None])                   # [K, NT, E]
        val = np.polynomial.chebyshev.chebval(xv, np.moveaxis(cf, 1, 0))                 # [K, E, NT]
        with np.errstate(all="ignore"):
            er = np.abs(np.moveaxis(val, 2, 1) - refv) / refv
        worst = float("nan") if np.isnan(er).any() else max(worst, float(er.max()))
    return W, worst


def mom_tables_host(bursts, epochs, ts_range, shapes=MOM_SHAPES):
    """The shape moments_plan / moments_build take: the first of `shapes` whose node spacing h / N
    does not exceed the narrowest burst's sigma and whose worst error is <= RJP_MOM_TOL.
    -> dict(K, N, worst, W, tried=[(K, N, worst | None)]) or None when none passes."""
    invs = _all_inv(bursts)
    sigma_min = math.sqrt(0.5 / max(invs))
    span = ts_range[1] - ts_range[0]
    tried = []
    for K, N in shapes:
        if not sigma_min >= (span / K if span > 0 else 0.0) / N:
            tried.append((K, N, None))
            continue
        W, worst = mom_table(bursts, epochs, ts_range, K, N)
        tried.append((K, N, worst))
        if worst <= MOM_TOL:
            return dict(K=K, N=N, worst=worst, W=W, tried=tried)
    return None


def lt_shapes(K):
    """The candidates of the launch-time-ordered layout: its K bins at orders 8, 12 .. 32."""
    return tuple((K, N) for N in range(8, MOM_NMAX + 1, 4))


def moment_bound(w0, ts, bursts, epochs, ts_range, K, N, W, ref, scale=1.0):
    """B[E, n_x, n_z] of the module docstring for a moment path of shape (K, N) with coefficients W
    (mom_table's); `w0` the signed weights, `ref` the reference sums, `scale` their common factor.
    -> (B, rounding term), each [E, n_x, n_z]."""
    w0 = np.asarray(w0, dtype=np.float64)
    ts = np.asarray(ts, dtype=np.float64)
    nx, ny, nz = w0.shape
    red = np.signbit(w0)
    w = np.abs(w0)
    lo, hi = ts_range
    span = hi - lo
    inv_h = K / span if span > 0 else 1.0
    has = [len(bursts[0]) > 0, len(bursts[1]) > 0]
    # per-bin weights of every sightline: M0[pixel, jet K + bin]
    with np.errstate(all="ignore"):
        wz = np.where(np.isnan(w), 0.0, w)
        tv = ts.copy()
        nan_t = np.isnan(tv)
        jet_has = np.where(red, has[0], has[1])
        wz = np.where(nan_t & jet_has, 0.0, wz)
        tv = np.where(nan_t, lo, tv)
        kb = np.clip(np.floor((tv - lo) * inv_h), 0, K - 1).astype(np.int64)
    pix = (np.arange(nx)[:, None, None] * nz + np.arange(nz)[None, None, :]) + np.zeros_like(kb)
    idx = pix * (2 * K) + np.where(red, 0, K) + kb
    finite = np.isfinite(wz)
    M0 = np.bincount(idx[finite], weights=wz[finite], minlength=nx * nz * 2 * K).reshape(nx * nz, 2 * K)
    absW = np.abs(W).sum(axis=2).reshape(2 * K, -1)                       # [2 K, E]
    R = (ny + 2 * N + 8) * EPS * (M0 @ absW).T.reshape(-1, nx, nz) * scale
    par = [[(float(t0), float(amp), inv2s2(sg)) for t0, amp, sg in lst] for lst in bursts]
    B, Rt = np.zeros(ref.shape), np.zeros(ref.shape)
    for e, t in enumerate(epochs):
        ds = 8.0 * EPS * (abs(span) + abs(lo) + abs(float(t)))
        with np.errstate(all="ignore"):
            tl = float(t) - ts
            chi, Dd = np.ones(w.shape), np.zeros(w.shape)
            for lst, mask in ((par[0], red), (par[1], ~red)):
                for t0, amp, inv in lst:
                    d = tl[mask] - t0
                    g = np.exp(-d * d * inv)
                    chi[mask] += amp * g
                    Dd[mask] += abs(amp) * g * 2.0 * inv * np.abs(d)
            dropped = np.isnan(w * (chi * chi)) | np.isinf(w)
            term = np.where(dropped, 0.0, w * 2.0 * np.abs(chi) * Dd * ds)
        Rt[e] = R[e] + term.sum(axis=1) * scale
        B[e] = MOM_TOL * ref[e] + Rt[e]
    return B, Rt


# ---- comparison ----------------------------------------------------------------------------------------
def within(got, ref, bound, what, where=None):
    """gpu_util.against's pattern rules (identical zero / NaN / inf patterns) and |got - ref| <= bound
    on every finite, non-zero reference value (of `where`, if given); -> worst error / bound."""
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    assert np.array_equal(got == 0, ref == 0), what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert np.array_equal(np.isinf(got), np.isinf(ref)), what
    ok = np.isfinite(ref) & (ref != 0)
    if where is not None:
        ok &= where
    if not ok.any():
        return 0.0
    frac = np.abs(got[ok] - ref[ok]) / bound[ok]
    worst = float(frac.max())
    assert worst <= 1.0, (what, worst, float(np.abs(got[ok] - ref[ok]).max()))
    return worst


def ratio(got, ref, bound, where=None):
    """Worst |got - ref| / bound without asserting (for the figures a test prints first)."""
    ok = np.isfinite(ref) & (ref != 0) & np.isfinite(got)
    if where is not None:
        ok &= where
    return float((np.abs(got[ok] - ref[ok]) / bound[ok]).max()) if ok.any() else 0.0


# ---- the cases both test files run ---------------------------------------------------------------------
SHAPES = [(3, 37, 16),           # two-wide lanes, two y-ranges
          (3, 37, 15),           # one-wide lanes
          (2, 200, 64)]          # twelve y-ranges


def year():
    return orc.YEAR


def irregular_epochs():
    """17 irregular epochs [s] on 0 .. 5 yr."""
    rng = np.random.default_rng(1713)
    return sorted((rng.uniform(0., 5., 17) * year()).tolist())


def uniform_epochs(n, t0_yr=0.0, t1_yr=5.0):
    return (np.linspace(t0_yr, t1_yr, n) * year()).tolist()


def narrow_case(et, ratio_sigma, first_yr=0.4, dt_yr=0.02):
    """Burst sets (b) / (c): `et` uniformly spaced epochs from `first_yr`, `dt_yr` apart, and one
    burst per jet whose sigma puts the tile's half-span at `ratio_sigma` sigma.  Its t0 is a typical
    launch-time offset, so that cells peak all over the tile; the test plants two cells that peak at
    the first and at the last epoch.  -> (epochs [s], (red, blue), t0 [s])."""
    Y = year()
    ep = [(first_yr + k * dt_yr) * Y for k in range(et)]
    dt, _ = tile_spacing(ep)
    m = et // 2
    half = max(m, et - 1 - m) * abs(dt)
    sigma = half / ratio_sigma
    t0 = 0.1 * Y
    return ep, ([(t0, 4.0, sigma)], [(t0, 2.5, sigma)]), t0


def eleven_and_three():
    """Burst set (d): 11 bursts in the red jet (three in the overflow table), 3 in the blue one, wide
    enough for the recurrence on the 32-epoch tile of a 0 .. 5 yr sweep (half-span 2.6 yr)."""
    rng = np.random.default_rng(1103)
    mk = lambda n: [(float(rng.uniform(-0.5, 5.5)) * year(), float(rng.uniform(0.2, 6.)),
                     sigma_of(float(rng.uniform(0.12, 0.6)))) for _ in range(n)]
    return mk(11), mk(3)


def dip_set():
    """Burst set (e): a dip of amplitude -0.9 beside a positive burst, in both jets."""
    Y = year()
    return ([(1.2 * Y, -0.9, sigma_of(0.3)), (2.2 * Y, 3.0, sigma_of(0.2))],
            [(2.0 * Y, -0.9, sigma_of(0.25)), (3.2 * Y, 1.5, sigma_of(0.4))])


def tile_burst_sets():
    return {"example": U.example_burst_lists(), "eleven+three": eleven_and_three(),
            "dip": dip_set(), "red-only": U.example_burst_lists(only="R")}


def scaled_example(k):
    """The example's bursts with every half-life times k (the K1m shapes: 1 -> (53, 12), 2.5 ->
    (80, 8), 0.8 -> (39, 16) on a 0 .. 5 yr launch-time range)."""
    red, blue = U.example_burst_lists()
    return [(t0, a, sg * k) for t0, a, sg in red], [(t0, a, sg * k) for t0, a, sg in blue]
