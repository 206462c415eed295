"""Shared helpers for the GPU parity tests (tests only: may import the oracle)."""
import json
import os

import numpy as np

from oracle import rt_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# K3 against scipy.special.wofz (through the oracle / the reference's golden cubes).  The
# kernels whose waves work on one cell (more than 16 channels: the 64- and 256-lane layouts)
# evaluate Re w(x + i y) to <= 1e-8 relative by design since round 3 (worst path 4.1e-9,
# tools/voigt_design.py; SURVEY.md section 7 asks <= 1e-7, the bar on the maps is 1e-5); an
# optical depth is a sum of same-signed terms, so the bound carries over to tau unamplified.
# The generic per-lane code (<= 16 channels, collapse=False) keeps 1.3e-11 per evaluation in its
# core and 3e-10 in its far field (continued fraction), same tool.
K3_RTOL_WAVE = 1e-8
K3_RTOL_LANE = 1e-9


def k3_rtol(nchan):
    return K3_RTOL_WAVE if nchan > 16 else K3_RTOL_LANE


def load_golden(tag):
    z = np.load(os.path.join(GOLDEN, tag + ".npz"))
    meta = json.loads(str(z["meta"]))
    p = meta["params"]
    for k in ("t_0", "hl", "chi", "which"):
        p["ejection"][k] = np.array(p["ejection"][k])
    return z, meta, p


def golden_dense(tag):
    """Reference grids of a golden model as dense float64 arrays + an oracle object."""
    z, meta, p = load_golden(tag)
    shape = tuple(meta["shape"])
    idx = z["f_idx"]
    d = lambda k, fill=np.nan: orc.dense_from_sparse(shape, idx, z["f_" + k], fill)
    g = dict(nd=d("nd"), xi=d("xi"), temp=d("temp"), ff=d("ff"), areas=d("areas"),
             ts=d("ts0", 0.), rr=d("rr", 1.), vy=d("vy"))
    jet = orc.OracleJet.from_fields(p, g["nd"], g["xi"], g["temp"], g["ff"], g["areas"],
                                    g["ts"], g["rr"], g["vy"])
    return z, meta, p, g, jet


def bursts_from_oracle(jet):
    """rjp_bursts parameters out of an OracleJet's burst list (classes.py:442-448)."""
    from rajepy_amd.engine import make_bursts
    out = []
    for which, ss in (("R", jet._ss_jml_rj), ("B", jet._ss_jml_bj)):
        lst = []
        for t0, peak, hl in jet.bursts[which]:
            sigma = hl * 2. / (2. * np.sqrt(2. * np.log(2.)))
            lst.append((t0, (peak - ss) / ss, sigma))
        out.append(lst)
    return make_bursts(out[0], out[1])


def synth_host(shape, seed, temp_mode=0, cell0=0, cells=None, nz_full=None):
    """Host restatement of rjp_synth_fields -- splitmix64 counter hash.
    With `cells` (flat indices into a grid whose z-extent is `nz_full`) it generates exactly
    those cells, returned in `shape`."""
    nx, ny, nz = shape
    n = nx * ny * nz
    if cells is None:
        cell = (np.arange(n, dtype=np.uint64) + np.uint64(cell0))
    else:
        cell = np.asarray(cells, dtype=np.uint64).ravel()
        assert cell.size == n
        nz = nz_full

    def u01(field):
        x = np.uint64(seed) ^ (np.uint64(field) << np.uint64(60)) ^ cell
        with np.errstate(over="ignore"):
            x = x + np.uint64(0x9E3779B97F4A7C15)
            x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            x = x ^ (x >> np.uint64(31))
        return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)

    iz = (cell % np.uint64(nz)).astype(np.int64)
    red = iz < nz // 2
    nd = 10.0 ** (5.0 + 2.5 * u01(1))
    xi = 0.05 + 0.45 * u01(2)
    temp = np.full(n, 1e4) if temp_mode == 0 else 5e3 + 1.5e4 * u01(3)
    pf = np.where(u01(4) < 0.25, 0.5, 1.0)
    ts = 5.0 * u01(5) * 31536000.0
    vy = 6.2 + 60.0 * (u01(6) - 0.5)
    nx, ny, nz = shape
    r = lambda a: a.reshape(shape)
    return dict(nd=r(nd), xi=r(xi), temp=r(temp), ff=r(pf), areas=r(np.ones(n)), ts=r(ts),
                rr=r(np.where(red, -1.0, 1.0)), vy=r(vy))


def example_bursts_params():
    """The four bursts of the reference's example model (files/example-model-params.py:51-54)."""
    return {"t_0": np.array([0.5, 0.75, 1., 2.]), "hl": np.array([0.15, 0.15, 0.45, 0.5]),
            "chi": np.array([5., 5., 2.5, 10.]), "which": np.array(["R", "B", "B", "RB"])}


# ---- single-epoch scans: an independent f64 reference and host restatements of the plans -------
# (tests/test_gpu_single_epoch_reference.py, tests/test_single_epoch_reference_cpu.py).  Bursts are
# plain per-jet lists [(t0_s, amp_rel, sigma_s), ...] for (red, blue), what engine.make_bursts takes.
SRT_MOM_TOL = 2e-14          # kSrtMomTol (ff_scan_tab.hip): a contracted bin against its cells
CHI_TOL = 1e-13              # kChiTol: |chi - table|
CHI_MAX_NI = 460             # kChiMaxNI: intervals of the LDS table
SRT_SHARE = 0.9              # srt_plan: the bucketed layout is read iff <= 90 % of the cells are


GAUSS_RTOL = 3e-12           # scans that keep the Gaussians (tests/test_gpu_random_parity.py)


def single_epoch_bound(ny):
    """Bound on a single-epoch table / sorted / hybrid map against ref_single_epoch (derived at
    the top of tests/test_gpu_single_epoch_reference.py): kChiTol on chi >= 1 gives 2e-13 on
    chi^2, kSrtMomTol for a contracted bin, plus the rounding of an f64 sum of n_y terms."""
    return 2.2e-13 + ny * 2.0 ** -53


def against(got, ref, rtol, what):
    """Identical zero / NaN / inf patterns and |got - ref| <= rtol ref; -> worst relative diff."""
    assert np.array_equal(got == 0, ref == 0), what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert np.array_equal(np.isinf(got), np.isinf(ref)), what
    ok = np.isfinite(ref) & (ref != 0)
    rel = float(np.max(np.abs(got[ok] - ref[ok]) / ref[ok])) if ok.any() else 0.0
    assert rel <= rtol, (what, rel, rtol)
    return rel


def example_burst_lists(only=None):
    """The reference example's four bursts as (red, blue) lists; `only` = "R" / "B": that jet's."""
    p = example_bursts_params()
    red, blue = [], []
    for t0, hl, chi, which in zip(p["t_0"], p["hl"], p["chi"], p["which"]):
        sig = hl * orc.YEAR * 2. / (2. * np.sqrt(2. * np.log(2.)))
        for jet, lst in (("R", red), ("B", blue)):
            if jet in str(which) and (only is None or only == jet):
                lst.append((t0 * orc.YEAR, chi - 1., sig))
    return red, blue


def chi_exact(jet_bursts, d):
    """1 + sum_b amp_b exp(-(d - t0_b)^2 / (2 sigma_b^2)) with numpy.exp, f64."""
    chi = np.ones_like(d)
    for t0, amp, sigma in jet_bursts:
        chi += amp * np.exp(-(d - t0) ** 2 / (2. * sigma ** 2))
    return chi


def _ref_slab(a0, ts, bursts, t_epoch):
    """One x-slab [n, n_y, n_z] -> [n, n_z] of ref_single_epoch."""
    red = np.signbit(a0)                             # include/rjprt.h: red-jet flag = sign bit
    w = np.abs(a0)
    chi = np.ones(a0.shape)
    with np.errstate(all="ignore"):
        for lst, mask in ((bursts[0], red), (bursts[1], ~red)):
            if len(lst):                             # (a jet without bursts: chi == 1, NaN ts too)
                chi[mask] = chi_exact(lst, t_epoch - ts[mask])
        term = w * (chi * chi)
    term[np.isnan(term)] = 0.                        # nansum: NaN terms are skipped
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        with np.errstate(all="ignore"):              # (inf - inf never occurs: all terms >= 0)
            return np.add.reduce(term, axis=1, dtype=np.longdouble).astype(np.float64)
    import math
    out = np.empty((a0.shape[0], a0.shape[2]))
    for i in range(a0.shape[0]):
        for k in range(a0.shape[2]):
            col = term[i, :, k]
            out[i, k] = math.fsum(col) if np.isfinite(col).all() else np.inf
    return out


def ref_single_epoch(a0, ts, bursts, t_epoch, slab_cells=1 << 21, threads=8):
    """sum_y |a0| chi_j(t_epoch - ts)^2 per sightline, [n_x, n_z] float64, from the arrays the
    device holds ([n_x, n_y, n_z]).  Jet from the sign bit of a0; numpy.exp; nansum semantics
    (NaN terms skipped, a jet without bursts has chi == 1 whatever its launch times, an infinite
    weight with a finite chi gives inf); sums in numpy.longdouble where that is wider than f64,
    else math.fsum.  x-slabs of `slab_cells` cells on `threads` threads (NumPy releases the GIL):
    <= ~100 bytes of temporaries per cell of a slab, below 1 GB in all."""
    from concurrent.futures import ThreadPoolExecutor
    nx, ny, nz = a0.shape
    step = max(1, int(slab_cells) // (ny * nz))
    cuts = list(range(0, nx, step))
    run = lambda x0: _ref_slab(a0[x0:x0 + step], ts[x0:x0 + step], bursts, float(t_epoch))
    if threads > 1 and len(cuts) > 1:
        with ThreadPoolExecutor(threads) as ex:
            parts = list(ex.map(run, cuts))
    else:
        parts = [run(x0) for x0 in cuts]
    return np.concatenate(parts, axis=0)


def _chi_reach(amp):
    import math
    return math.sqrt(2.0 * math.log(max(amp, 1.0) * 1e17))


def _support(jet_bursts):
    """[s_lo, s_hi] of one jet's bursts, with the widths as engine.make_bursts hands them over
    (1 / (2 sigma^2)) and the library takes them back."""
    import math
    s_lo, s_hi = math.inf, -math.inf
    for t0, amp, sg in jet_bursts:
        sigma = math.sqrt(0.5 / (1.0 / (2.0 * float(sg) ** 2.0)))
        s_lo = min(s_lo, t0 - _chi_reach(amp) * sigma)
        s_hi = max(s_hi, t0 + _chi_reach(amp) * sigma)
    return s_lo, s_hi


def srt_plan_host(hist, ts_range, K, bursts, t_epoch):
    """Host restatement of srt_plan (ff_scan_tab.hip): per jet the bins [b0, b1) that meet the
    bursts' support at `t_epoch`, the share of the cells (hist[2 K]) inside them, and the layout:
    "sorted" iff share <= 0.9."""
    import math
    lo, hi = ts_range
    span = hi - lo
    inv_h = K / span if span > 0.0 else 1.0
    hist = [int(v) for v in hist]
    b0, b1, n_all, n_read = [0, 0], [0, 0], 0, 0
    for j in range(2):
        if len(bursts[j]):
            s_lo, s_hi = _support(bursts[j])
            w0 = math.floor((t_epoch - s_hi - lo) * inv_h)
            w1 = math.floor((t_epoch - s_lo - lo) * inv_h) + 1.0
            c0, c1 = int(min(max(w0, 0.0), float(K))), int(min(max(w1, 0.0), float(K)))
            if c1 > c0:
                b0[j], b1[j] = c0, c1
        n_all += sum(hist[j * K:(j + 1) * K])
        n_read += sum(hist[j * K + b0[j]:j * K + b1[j]])
    share = n_read / n_all if n_all > 0 else 0.0
    return {"b0": b0, "b1": b1, "share": share, "layout": "sorted" if share <= SRT_SHARE else "grid"}


def chi_table_host(shape, ts_range, bursts, t_epoch):
    """Host restatement of chi_table_plan's rules for an f64 tau-layout scan of one epoch: the
    number of table intervals, or None where the scan keeps the Gaussians (map too small, a dip,
    more than 460 intervals)."""
    import math
    nx, ny, nz = shape
    if not (len(bursts[0]) or len(bursts[1])) or (nx * nz) // 2 < 64 * 256 or ny < 64:
        return None
    lo_t, hi_t = ts_range
    s_lo, s_hi, B = math.inf, -math.inf, 0.0
    for j in range(2):
        Bj = 0.0
        for t0, amp, sg in bursts[j]:
            inv = 1.0 / (2.0 * float(sg) ** 2.0)
            if not (inv > 0.0 and math.isfinite(inv) and amp >= 0.0 and math.isfinite(amp)):
                return None
            s2 = math.sqrt(0.5 / inv) ** 2
            Bj += amp * 105.0 / (s2 * s2 * s2 * s2)
        if len(bursts[j]):
            a, b = _support(bursts[j])
            s_lo, s_hi = min(s_lo, a), max(s_hi, b)
        B = max(B, Bj)
    lo, hi = max(s_lo, t_epoch - hi_t), min(s_hi, t_epoch - lo_t)
    if not hi > lo:
        return 1
    h = 2.0 * (CHI_TOL * 5160960.0 / B) ** (1.0 / 8.0)
    n = math.ceil((hi - lo) / h)
    return max(1, int(n)) if n <= CHI_MAX_NI else None


def srt_bin_passes(jet_bursts, ts_range, K, N, b, t_epoch, tol):
    """Does the degree-(N - 1) Chebyshev interpolant of the exact chi^2 on launch-time bin `b`
    match it at the 4 N check points of srt_coef_kernel to `tol` relative?  Host f64."""
    lo, hi = ts_range
    h = (hi - lo) / K if hi > lo else 1.0
    F = lambda x: chi_exact(jet_bursts, t_epoch - (lo + (b + 0.5 * (x + 1.0)) * h)) ** 2
    nodes = np.cos(np.pi * (np.arange(N) + 0.5) / N)
    T = np.polynomial.chebyshev.chebvander(nodes, N - 1)             # [m, n]
    W = (2.0 / N) * (T.T @ F(nodes))
    W[0] *= 0.5
    x = -1.0 + 2.0 * np.arange(4 * N) / (4 * N - 1)
    p, f = np.polynomial.chebyshev.chebval(x, W), F(x)
    return bool(np.all(np.abs(p - f) <= tol * f))


def srt_group_stats(start, K):
    """From the layout's start rows ([2 K + 1, P] int array), per group of 64 sightlines:
    (held[2, G]: some lane holds a cell of that jet; longest[2 K, G]: the longest lane run of
    every key)."""
    P = start.shape[1]
    G = (P + 63) // 64
    cnt = np.zeros((2 * K, G * 64), dtype=np.int64)
    cnt[:, :P] = np.diff(start.astype(np.int64), axis=0)
    cnt = cnt.reshape(2 * K, G, 64)
    held = np.stack([cnt[j * K:(j + 1) * K].sum(axis=0).max(axis=1) > 0 for j in range(2)])
    return held, cnt.max(axis=2)


def srt_counts_host(stats, K, N, plan, bursts, ts_range, t_epoch):
    """From srt_group_stats and the host plan: (triples, cap) -- `triples` = the (group, jet, bin)
    triples a scan with moments must count, bin in [b0, b1) over the groups in which some lane
    holds a cell of that jet; `cap` = how many of them the byte rule (longest lane run x 16 >
    (N - 1) x 8) allows AND whose interpolant of the exact chi^2 passes at ten times the device's
    tolerance: an upper bound on the contracted ones."""
    held, longest = stats
    triples = cap = 0
    for j in range(2):
        b0, b1 = plan["b0"][j], plan["b1"][j]
        triples += int(held[j].sum()) * max(0, b1 - b0)
        for b in range(b0, b1):
            if srt_bin_passes(bursts[j], ts_range, K, N, b, t_epoch, 10 * SRT_MOM_TOL):
                cap += int((held[j] & (longest[j * K + b] * 16 > (N - 1) * 8)).sum())
    return triples, cap


def golden_a0(g, q_T):
    """The tau scan field of include/rjprt.h from a golden model's dense grids, in NumPy:
    (n x)^2 ff / areas T^-1.5 (one Gaunt factor per channel, q_T == 0) or T^-1.35, red-jet flag in
    the sign bit.  Cells outside the jet are NaN."""
    with np.errstate(all="ignore"):
        a = (g["nd"] * g["xi"]) ** 2. * (g["ff"] / g["areas"]) * \
            g["temp"] ** (-1.5 if q_T == 0. else -1.35)
    return np.where(g["rr"] < 0, -a, a)
