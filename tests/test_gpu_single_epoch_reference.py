"""The bucketed single-epoch scans (ff_scan_sorted_kernel, srt_coef_kernel + ff_scan_hybrid_kernel<U, N>;
ff_scan_tab.hip, ff_lt.hip) and the grid-order table scan against a reference that shares nothing
with them: tests/gpu_util.ref_single_epoch, a plain float64 / long-double sum of |a0| chi(t - ts)^2
with numpy.exp over the device's own a0 and ts (pinned to the reference project's golden maps in
tests/test_single_epoch_reference_cpu.py).  Every case also holds the library to a host restatement
of its plan: the layout taken, the exact number of (group, jet, bin) triples the hybrid scan counts,
an upper bound on the contracted ones.

Bound on every map (derived, not measured): kChiTol = 1e-13 on chi >= 1 gives 2e-13 on chi^2,
kSrtMomTol = 2e-14 for a contracted bin, plus the worst-case rounding of an f64 sum of n_y
same-signed terms:  |got - ref| <= (2.2e-13 + n_y 2^-53) ref.  Scans that keep the Gaussians (the
table refused: more than 460 intervals) are held to the 3e-12 of tests/test_gpu_random_parity.py."""
import copy
import time

import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
YEAR = orc.YEAR
SEED = 20250301
MID = (128, 480, 256)              # 32768 sightlines x 480 rows = 1.6e7 cells: the sweeps' map
GAUSS_RTOL = U.GAUSS_RTOL
T0 = time.time()
bound = U.single_epoch_bound       # (shared with tests/test_gpu_model_life.py)


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    e.cache_moments = False
    yield e
    e.close()
    print("wall time of this module so far: %.0f s" % (time.time() - T0))


class Model:
    """Synthetic fields with the bucketed layout attached + what the host checks need of them."""

    def __init__(self, eng, shape, seed, temp_mode=0, K=32, N=20, dirty=None, ts_const=None):
        import torch
        from rajepy_amd import engine as E
        self.eng, self.shape, self.K = eng, shape, K
        self.mode = E.RJP_GFF_SCALAR if temp_mode == 0 else E.RJP_GFF_POWERLAW
        f = eng.synth_fields(shape, seed, temp_mode, 8, csize_au=0.5, tau_mode=self.mode,
                             wide=False, with_em0=False)
        if ts_const is not None:
            f.ts = torch.full_like(f.ts, ts_const)       # (a new tensor: the range is re-measured)
        if dirty is not None:
            dirty(f)
        self.fields = f
        self.attach(K, N)
        self.a0 = f.a0.cpu().numpy().reshape(shape)
        self.ts = f.ts.cpu().numpy().reshape(shape)
        self._refs = {}

    def attach(self, K, N):
        eng = self.eng
        eng.srt_N = N
        try:
            srt = eng.build_sorted(self.fields, K)
        finally:
            eng.srt_N = 20
        assert srt is not None and srt["mom"] is not None and (srt["K"], srt["N"]) == (K, N)
        self.K, self.N, self.srt = K, N, srt
        self.hist = [int(v) for v in srt["hist"]]
        self.ts_range = self.fields.ts_range
        start = srt["start"].cpu().numpy().reshape(2 * K + 1, self.fields.npix)
        self.start = start
        self.stats = U.srt_group_stats(start, K)

    def ref(self, bursts, t):
        key = (repr(bursts), float(t))
        if key not in self._refs:
            self._refs[key] = U.ref_single_epoch(self.a0, self.ts, bursts, t).ravel()
        return self._refs[key]


def _scan(m, bursts, t, sorted_=True, moments=True):
    from rajepy_amd import engine as E
    eng = m.eng
    eng.use_sorted, eng.use_srt_moments = sorted_, moments
    try:
        a = eng.ff_scan(m.fields, E.make_bursts(*bursts), [t], m.mode, want_em=False,
                        want_tavg=False)[0].clone()
    finally:
        eng.use_sorted = eng.use_srt_moments = True
    eng.synchronize()
    assert not eng.range_guard()
    return a.cpu().numpy()[0], eng.last_scan_path()[0], eng.last_scan_layout(), eng.last_srt_bins()


_against = U.against


def check_case(m, bursts, t, what=""):
    """The hybrid, the moment-free sorted and the grid-order scan of `m` at `t` against the
    reference, each on the path and layout the host restatement predicts, with the counters."""
    plan = U.srt_plan_host(m.hist, m.ts_range, m.K, bursts, t)
    ni = U.chi_table_host(m.shape, m.ts_range, bursts, t)
    ref = m.ref(bursts, t)
    ny = m.shape[1]
    out = {"plan": plan, "ni": ni, "sorted": False, "bins": (0, 0), "triples": 0}
    rels = []
    for name, kw in (("hybrid", {}), ("sorted", {"moments": False}), ("grid", {"sorted_": False})):
        got, path, layout, bins = _scan(m, bursts, t, **kw)
        tag = (what, name, t / YEAR)
        if ni is None:
            # the table would not fit the LDS: the Gaussian scan, which never reads the layout
            assert (path, layout, bins) == ("tiles", "grid", (0, 0)), tag
            rels.append(_against(got, ref, GAUSS_RTOL, tag))
            continue
        assert path == "table", tag
        assert m.eng.last_moment_shape == (ni, 8), (tag, m.eng.last_moment_shape, ni)
        if name == "grid":
            assert (layout, bins) == ("grid", (0, 0)), tag
        else:
            assert layout == plan["layout"], (tag, layout, plan)
            if name == "hybrid" and layout == "sorted":
                triples, cap = U.srt_counts_host(m.stats, m.K, m.N, plan, bursts, m.ts_range, t)
                assert bins[0] + bins[1] == triples, (tag, bins, triples)
                assert bins[0] <= cap, (tag, bins, cap)
                out.update(sorted=True, bins=bins, triples=triples, cap=cap)
            else:
                assert bins == (0, 0), tag
        rels.append(_against(got, ref, bound(ny), tag))
    out["rel"] = rels
    return out


# ---- random burst sets x epochs ------------------------------------------------------------------
def random_bursts(seed):
    """1-8 bursts: spread over both jets (seed % 3 == 0), one jet only (1), piled on one another
    (2); sigma 0.08-0.9 yr, relative amplitude 0.1-50 (both log-uniform)."""
    rng = np.random.default_rng(7000 + seed)
    nb = int(rng.integers(1, 9))
    lists = ([], [])
    centre = rng.uniform(0.3, 2.0)
    only = int(rng.integers(0, 2))
    for _ in range(nb):
        kind = seed % 3
        t0 = rng.normal(centre, 0.05) if kind == 2 else rng.uniform(-0.5, 2.5)
        sigma = 10.0 ** rng.uniform(np.log10(0.08), np.log10(0.9))
        amp = 10.0 ** rng.uniform(-1.0, np.log10(50.0))
        if kind == 2:                                    # piled up: mostly narrow and strong
            sigma, amp = min(sigma, rng.uniform(0.08, 0.2)), max(amp, rng.uniform(5.0, 50.0))
        j = only if kind == 1 else int(rng.integers(0, 2))
        lists[j].append((t0 * YEAR, amp, sigma * YEAR))
    return lists


# seed 12: a narrow strong burst whose table interval (~0.009 yr) over the support of a wide one
# (the whole launch-time range) needs more than 460 intervals at every epoch inside the range
REFUSED = ([(1.0 * YEAR, 50.0, 0.08 * YEAR), (1.5 * YEAR, 40.0, 0.9 * YEAR)], [])


def choose_epochs(seed, bursts, hist, ts_range, K, shape):
    """Six epochs per burst set: one before the first launch time meets a burst (b1 == 0: every
    sum comes from d_srt_cum), one beyond ts_hi plus the support, one with the upper edge of a
    jet's support (t - s_lo) exactly on a bin edge, three drawn from 0.2-2.5 yr -- the edge and
    the drawn ones picked with the host plan so that they take the bucketed layout where some
    candidate does (a late epoch under wide bursts reads > 90 % of the cells: grid order)."""
    rng = np.random.default_rng(9000 + seed)
    lo, hi = ts_range
    sup = [U._support(b) for b in bursts if len(b)]
    s_lo, s_hi = min(s[0] for s in sup), max(s[1] for s in sup)
    def takes(t):
        # (the bucketed layout, on the table path, with at least one bin in a support)
        plan = U.srt_plan_host(hist, ts_range, K, bursts, t)
        return (plan["layout"] == "sorted" and plan["b1"] != [0, 0] and
                U.chi_table_host(shape, ts_range, bursts, t) is not None)

    epochs = [lo + s_lo - 0.1 * YEAR, hi + s_hi + 0.1 * YEAR]
    h = (hi - lo) / K
    j = 0 if len(bursts[0]) else 1
    edges = [lo + k * h + U._support(bursts[j])[0] for k in rng.permutation(np.arange(2, K))]
    epochs.append(next((t for t in edges if takes(t)), edges[0]))
    for _ in range(3):
        draws = [rng.uniform(0.2, 2.5) * YEAR for _ in range(12)]
        epochs.append(next((t for t in draws if takes(t)), draws[0]))
    return epochs


def test_random_bursts_and_epochs_against_the_reference(eng):
    """13 burst sets x 6 epochs on 128 x 480 x 256.  At its end: at least three quarters of the
    cases took the bucketed layout and at least half of those contracted a bin or more."""
    m = Model(eng, MID, SEED)
    cases = sorted_ = contracting = refused = 0
    worst = [0.0, 0.0, 0.0]
    for seed in range(13):
        bursts = REFUSED if seed == 12 else random_bursts(seed)
        for i, t in enumerate(choose_epochs(seed, bursts, m.hist, m.ts_range, m.K, m.shape)):
            r = check_case(m, bursts, t, "seed %d" % seed)
            cases += 1
            sorted_ += r["sorted"]
            contracting += r["sorted"] and r["bins"][0] > 0
            refused += r["ni"] is None
            if r["ni"] is not None:
                worst = [max(a, b) for a, b in zip(worst, r["rel"])]
            if i == 0 and r["ni"] is not None:           # before every launch time: no bin is read
                assert r["plan"]["b1"] == [0, 0] and r["sorted"] and r["triples"] == 0
            if i == 1 and r["ni"] is not None:
                assert r["plan"]["b1"] == [0, 0] and r["sorted"]
            print("seed %2d (%d + %d bursts) %7.3f yr: ni %s, plan %s share %.2f, (contracted, "
                  "read) %s of %d, rel %s" % (seed, len(bursts[0]), len(bursts[1]), t / YEAR,
                                              r["ni"], r["plan"]["layout"], r["plan"]["share"],
                                              r["bins"], r["triples"],
                                              " ".join("%.2e" % v for v in r["rel"])))
    print("random bursts: %d cases, %d on the bucketed layout, %d of them contracting, %d kept the "
          "Gaussians; worst relative difference vs the f64 reference: hybrid %.3g, sorted %.3g, "
          "grid order %.3g (bound %.3g)" % (cases, sorted_, contracting, refused, *worst,
                                            bound(MID[1])))
    assert cases >= 48 and refused >= 1
    assert sorted_ >= 0.75 * cases, (sorted_, cases)
    assert contracting >= 0.5 * sorted_, (contracting, sorted_)


# ---- K x N ------------------------------------------------------------------------------------------
def check_moments(m, pixels):
    """d_srt_mom of the attached (K, N) against a host f64 restatement, on `pixels`."""
    srt, K, N, P = m.srt, m.K, m.N, m.fields.npix
    lo, hi = m.ts_range
    inv_h = K / (hi - lo) if hi > lo else 1.0
    cum = srt["cum"].cpu().numpy().reshape(2 * K + 1, P)
    rowbase = srt["rowbase"].cpu().numpy()
    mom = srt["mom"].view(2 * K, N - 1, P)
    for p in pixels:
        g, lane = divmod(p, 64)
        n_cells = int(m.start[2 * K, p])
        rows = srt["cells"].view(-1, 64, 2)[int(rowbase[g]):int(rowbase[g]) + n_cells, lane]
        a, t = rows[:, 0].cpu().numpy(), rows[:, 1].cpu().numpy()
        got = mom[:, :, p].cpu().numpy()
        for q in range(2 * K):
            s0, s1 = int(m.start[q, p]), int(m.start[q + 1, p])
            w = (t[s0:s1] - lo) * inv_h
            k = np.clip(np.floor(w), 0, K - 1)
            assert np.all(k == q % K)
            T = np.polynomial.chebyshev.chebvander(2.0 * (w - k) - 1.0, N - 1)
            scale = a[s0:s1].sum()
            assert abs(scale - (cum[q + 1, p] - cum[q, p])) <= 1e-13 * cum[2 * K, p]
            assert np.all(np.abs(got[q] - a[s0:s1] @ T[:, 1:]) <= 1e-13 * scale), (p, q)


def test_every_K_and_N_against_the_reference(eng):
    """K in {1, 5, 16, 32} x N in {16, 20, 24}: the moments against the host restatement, the scans
    against the reference.  With K = 1 and K = 5 the bins are far wider than the bursts: at K = 1
    bursts in both jets put every cell in the support (grid order) and bursts in one jet leave one
    bin that cannot pass; at K = 5 only the bins far from every burst pass -- the read runs carry
    the map."""
    m = Model(eng, MID, SEED + 1)
    P = m.fields.npix
    sets = {"both": U.example_burst_lists(), "red": U.example_burst_lists("R")}
    seen = {}
    for K in (1, 5, 16, 32):
        for N in (16, 20, 24):
            m.attach(K, N)
            check_moments(m, [0, 63, 64, P - 1, 12345])
            for name, bursts in sets.items():
                for years in (1.0, 0.3):
                    r = check_case(m, bursts, years * YEAR, "K %d N %d %s" % (K, N, name))
                    seen.setdefault(K, []).append(r)
                    print("K %2d N %2d %-4s %.1f yr: plan %s, (contracted, read) %s of %d (cap %s), "
                          "rel %s" % (K, N, name, years, r["plan"]["layout"], r["bins"],
                                      r["triples"], r.get("cap"),
                                      " ".join("%.2e" % v for v in r["rel"])))
    for K, rs in seen.items():
        assert any(r["sorted"] for r in rs), K             # every K ran the hybrid kernel ...
    assert any(r["bins"][0] > 0 for r in seen[16]) and any(r["bins"][0] > 0 for r in seen[32])
    assert all(r["bins"][1] > 0 for K in (1, 5) for r in seen[K] if r["sorted"])   # ... reading


def test_all_launch_times_equal(eng):
    """ts_hi == ts_lo: the layout's bins are one second wide (the `span > 0 ? ... : 1` branch),
    every cell sits in bin 0 at x = -1.  Bursts in one jet (with both, all cells are in the
    support: grid order, checked too).  At 1.8 yr the cells sit on a burst: chi changes by ~1e-9
    over the one-second bin while the table (one interval, clamped below the cells' own time)
    is constant there, so bin 0 is refused and read; at 6.9 yr they sit in the last sigma of the
    widest burst's support, chi - 1 ~ 1e-15: bin 0 passes and is contracted in every group.  The
    31 empty bins of the support are "read" either way."""
    m = Model(eng, (128, 320, 256), SEED + 2, ts_const=1.3 * YEAR)
    assert m.ts_range == (1.3 * YEAR, 1.3 * YEAR)
    assert m.hist[0] > 0 and m.hist[32] > 0 and sum(m.hist) == m.hist[0] + m.hist[32]
    check_moments(m, [0, 77, m.fields.npix - 1])
    G = m.fields.npix // 64 // 2                           # groups per jet (n_z / 2 = 2 x 64)
    for name in ("R", "B", None):
        for years in (1.8, 6.9):
            r = check_case(m, U.example_burst_lists(name), years * YEAR, "equal ts %s" % name)
            assert r["sorted"] == (name is not None)
            if r["sorted"]:
                assert r["bins"] == ((0, 32 * G) if years == 1.8 else (G, 31 * G)), r["bins"]
            print("equal launch times, bursts %s, %.1f yr: %s rel %s" % (name, years, r["bins"],
                                                                        r["rel"]))


# ---- sightline counts that are not multiples of 64 ---------------------------------------------------
@pytest.mark.parametrize("shape", [(131, 320, 254), (145, 320, 226)])
def test_dead_lanes_of_the_last_group(eng, shape):
    """33274 sightlines (58 live lanes in the last group) and 32770 (two)."""
    m = Model(eng, shape, SEED + 3)
    P = m.fields.npix
    assert P % 64 == (58 if shape[0] == 131 else 2)
    for bursts in (U.example_burst_lists(), random_bursts(8)):
        for years in (1.0, 0.3):
            t = years * YEAR
            r = check_case(m, bursts, t, "P = %d" % P)
            assert r["sorted"], r
            if bursts == U.example_burst_lists():
                assert r["bins"][0] > 0 and r["bins"][1] > 0, r
            # the last live sightline, by name
            got = _scan(m, bursts, t)[0]
            ref = m.ref(bursts, t)
            assert got.shape == (P,) and np.isfinite(got[P - 1]) and got[P - 1] > 0
            assert abs(got[P - 1] - ref[P - 1]) <= bound(shape[1]) * ref[P - 1]
            print("P = %d, %.1f yr: (contracted, read) %s of %d, rel %s" % (
                P, years, r["bins"], r["triples"], r["rel"]))


# ---- occupied y-ranges on the two grid-order table scans ---------------------------------------------
@pytest.mark.parametrize("layout", ["tau", "wide"])
def test_grid_order_table_scans_with_occupied_y_ranges(eng, layout):
    """ff_scan_table_kernel (tau layout) and ff_scan_table_wide_kernel (the five model fields) with
    d_ylo / d_yhi attached: the same bits as without them, and without them within the table bound
    of the reference.  The smallest map the table scans take (32768 sightlines, 64 rows) grown to
    n_y = 65 (no multiple of the rows in flight, one y-range per sightline is not forced), n_z = 254
    (no multiple of 16) and 33274 sightlines (58 live lanes in the last wave, dead lanes in the last
    workgroup); 60 % holes, empty rows at both ends, an empty sightline and a first workgroup whose
    512 sightlines are all empty.
    Bound: U.single_epoch_bound(n_y) against ref_single_epoch on the device's own |a0|; the wide scan
    forms |a0| = (|nd| xi)^2 pf T^-1.5 itself -- four roundings, 4 * 2^-53 on every term, added."""
    import torch
    from rajepy_amd import engine as E
    shape = (131, 65, 254)
    nx, ny, nz = shape
    mode = E.RJP_GFF_SCALAR
    f = eng.synth_fields(shape, SEED + 11, 0, 8, csize_au=0.5, wide=True, tau_mode=mode)
    assert f.npix % 64 == 58 and (f.npix // 2) % 256 != 0
    g = torch.Generator(device=eng.device)
    g.manual_seed(29)
    hole = (torch.rand(f.ncells, device=eng.device, generator=g) < 0.6).view(nx, ny, nz)
    hole[:, :9, :] = True                          # empty rows at both ends
    hole[:, ny - 6:, :] = True
    hole[70, :, 33] = True                         # an empty sightline
    hole[:3, :, :] = True                          # 762 sightlines: the whole first workgroup
    hole = hole.reshape(-1)
    nan = float("nan")
    for t in (f.nd, f.xi, f.temp, f.pf, f.em0, f.a0):
        t[hole] = nan
    a0 = f.a0.cpu().numpy().reshape(shape)
    ts = f.ts.cpu().numpy().reshape(shape)
    if layout == "wide":
        f.a0 = f.em0 = None                        # scan the five model fields
    bursts = U.example_burst_lists()
    t_epoch = 1.0 * YEAR
    ref = U.ref_single_epoch(a0, ts, bursts, t_epoch).ravel()
    assert ref[70 * nz + 33] == 0.0 and not ref[:512].any() and (ref > 0).sum() > f.npix // 2

    def scan():
        eng.use_sorted = False
        try:
            a = eng.ff_scan(f, E.make_bursts(*bursts), [t_epoch], mode, want_em=False,
                            want_tavg=False)[0].clone()
        finally:
            eng.use_sorted = True
        eng.synchronize()
        assert not eng.range_guard()
        assert (eng.last_scan_path()[0], eng.last_scan_layout()) == ("table", "grid")
        assert eng.last_scan_tiles() == []
        return a.cpu().numpy()[0]

    free = scan()
    lo, hi = eng.compute_y_bounds(f)
    assert f.ylo is not None
    lo, hi = lo.cpu().numpy(), hi.cpu().numpy()
    assert (lo[:512] == ny).all() and (hi[:512] == 0).all()          # [n_y, 0): empty
    assert lo[70 * nz + 33] == ny and lo[lo < ny].min() >= 9 and hi.max() <= ny - 6
    clipped = scan()
    rtol = bound(ny) + (4 * 2.0 ** -53 if layout == "wide" else 0.0)
    rel = _against(free, ref, rtol, layout)
    print("%s table scan, %s: worst relative difference %.3g of %.3g" % (layout, shape, rel, rtol))
    assert np.array_equal(clipped.view(np.int64), free.view(np.int64)), layout


# ---- n_y across the byte rule ------------------------------------------------------------------------
@pytest.mark.parametrize("ny", [96, 320, 480, 2048])
def test_ny_across_the_byte_rule(eng, ny):
    """K = 32, N = 20: a bin is contracted where its longest lane run in the group exceeds 9.5
    cells.  n_y = 96 gives 3 cells per bin and lane on average (a Poisson tail reaches 10 in a few
    per cent of the (group, bin) pairs: nearly every accepted bin is still read), 320 and 480 mix
    contracted and read bins inside one support, 2048 is the bench-like map."""
    m = Model(eng, (128, ny, 256), SEED + 4 + ny)
    for years in (1.0, 0.3):
        r = check_case(m, U.example_burst_lists(), years * YEAR, "n_y %d" % ny)
        assert r["sorted"], r
        con, read = r["bins"]
        if ny == 96:
            # P(Poisson(3) >= 10) = 1.1e-3 per lane, x 64 lanes: < 8 % of the pairs
            assert con <= 0.1 * r["triples"] < read, r
        else:
            assert con > 0 and read > 0, r
        print("n_y %4d, %.1f yr: (contracted, read) %s of %d (cap %d), rel %s" % (
            ny, years, r["bins"], r["triples"], r["cap"], r["rel"]))


# ---- both jets in one sightline, dirty cells -----------------------------------------------------------
def _dirty(eng, shape):
    def edit(f):
        import torch
        g = torch.Generator(device=eng.device)
        g.manual_seed(12)
        n = f.ncells
        nx, ny, nz = shape
        r = lambda: torch.rand(n, device=eng.device, generator=g)
        # a quarter of the sightlines get cells of both jets (the other groups stay single-jet)
        col = torch.arange(n, device=eng.device) % nz
        flip = (r() < 0.3) & (col < nz // 4)
        f.a0[flip] = -f.a0[flip]
        f.a0[r() < 0.02] = float("nan")
        f.a0[r() < 0.02] = 0.0
        f.ts[r() < 0.02] = float("nan")
        for (x, y, z, t_nan) in ((3, 10, 5, False), (7, 20, nz - 56, True), (nx - 28, 0, nz - 1, False)):
            c = (x * ny + y) * nz + z
            f.a0[c] = float("inf") * (1 if z >= nz // 2 else -1)
            if t_nan:
                f.ts[c] = float("nan")
        for x, z, v in ((5, 7, float("nan")), (6, 9, 0.0)):
            f.a0[(x * ny + torch.arange(ny, device=eng.device)) * nz + z] = v
    return edit


def test_both_jets_and_dirty_cells_against_the_reference(eng):
    """Sign flips along y, NaN / zero / infinite a0, NaN ts, whole sightlines zero or NaN; the
    example bursts and random sets, in both jets or one."""
    m = Model(eng, MID, SEED + 5, temp_mode=1, dirty=_dirty(eng, MID))
    nx, ny, nz = MID
    sets = [U.example_burst_lists(), U.example_burst_lists("R"), U.example_burst_lists("B"),
            random_bursts(0), random_bursts(1), random_bursts(7)]
    for i, bursts in enumerate(sets):
        for years in (1.0, 0.3):
            t = years * YEAR
            r = check_case(m, bursts, t, "dirty %d" % i)
            ref = m.ref(bursts, t)
            assert ref[5 * nz + 7] == 0.0 and ref[6 * nz + 9] == 0.0 and np.isinf(ref).sum() >= 1
            # (7, 20, nz - 56): infinite weight, NaN launch time -- inf only if its jet has no burst
            assert np.isinf(ref[7 * nz + nz - 56]) == (len(bursts[1]) == 0)
            print("dirty, set %d (%d + %d bursts), %.1f yr: plan %s, (contracted, read) %s of %d, "
                  "rel %s" % (i, len(bursts[0]), len(bursts[1]), years, r["plan"]["layout"],
                              r["bins"], r["triples"], r["rel"]))
            assert r["sorted"] or r["plan"]["layout"] == "grid"


# ---- rjp_ff_step ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("temp_mode", [0, 1])
def test_ff_step_cubes_against_the_reference(eng, temp_mode):
    """tau and flux cubes of a hybrid step: ctau ref and cflux T_avg (1 - e^-tau) in NumPy, both
    Gaunt modes.  The map stage's 1 - e^-tau is good to 4e-15 (rjp_device.h), T_avg is a mean of
    n_y terms: the flux bound is the tau bound + 4e-15 + (n_y + 4) 2^-53."""
    from rajepy_amd import engine as E
    from rajepy_amd.maths import physics as ph
    m = Model(eng, MID, SEED + 6, temp_mode=temp_mode)
    bursts = U.example_burst_lists()
    nu = np.array([1e9, 5e9, 2e10, 4.3e10])
    ctau, cflux = E.ff_channel_coeffs(nu, 0.5, 120., m.mode,
                                      [ph.gff(f, 1e4) for f in nu] if temp_mode == 0 else None)
    tavg = eng.tavg(m.fields)
    temp = m.fields.temp.cpu().numpy().reshape(MID)
    tavg_ref = np.nanmean(np.where(temp > 0., temp, np.nan), axis=1).ravel()
    P, F, ny = m.fields.npix, len(nu), MID[1]
    for years in (1.0, 0.3):
        t = years * YEAR
        out = (eng._f64(1, P), None, eng._f64(1, F, P), eng._f64(1, F, P), eng._f64(1, F))
        eng.ff_step(m.fields, E.make_bursts(*bursts), [t], m.mode, tavg, ctau, cflux, out)
        eng.synchronize()
        plan = U.srt_plan_host(m.hist, m.ts_range, m.K, bursts, t)
        assert eng.last_scan_path()[0] == "table" and eng.last_scan_layout() == plan["layout"] == "sorted"
        bins = eng.last_srt_bins()
        triples, cap = U.srt_counts_host(m.stats, m.K, m.N, plan, bursts, m.ts_range, t)
        assert bins[0] + bins[1] == triples and 0 < bins[0] <= cap
        ref = m.ref(bursts, t)
        rel_a = _against(out[0].cpu().numpy()[0], ref, bound(ny), "sumA")
        tau, flux = out[2].cpu().numpy()[0], out[3].cpu().numpy()[0]
        rel_t = rel_f = 0.0
        for f in range(F):
            tau_ref = ctau[f] * ref
            rel_t = max(rel_t, _against(tau[f], tau_ref, bound(ny) + 2.0 ** -52, "tau"))
            flux_ref = cflux[f] * tavg_ref * (-np.expm1(-tau_ref))
            rel_f = max(rel_f, _against(flux[f], flux_ref,
                                        bound(ny) + 4e-15 + (ny + 4) * 2.0 ** -53, "flux"))
        ftot = out[4].cpu().numpy()[0]
        # (the map's total: the flux bound + the worst-case rounding of a sum of P terms)
        np.testing.assert_allclose(ftot, [np.sum(cflux[f] * tavg_ref * -np.expm1(-ctau[f] * ref))
                                          for f in range(F)],
                                   rtol=bound(ny) + 4e-15 + (ny + 4 + P) * 2.0 ** -53)
        print("ff_step, Gaunt mode %d, %.1f yr: rel sumA %.3g, tau %.3g, flux %.3g" % (
            m.mode, years, rel_a, rel_t, rel_f))


# ---- the layout itself, over a whole map ---------------------------------------------------------------
@pytest.mark.parametrize("shape,dirty", [(MID, True), ((145, 320, 226), True), ((131, 320, 254), False)])
def test_layout_against_a_restatement_over_the_whole_map(eng, shape, dirty):
    """d_srt_start, h_srt_hist, d_srt_cells (as multisets per sightline and key, every row in the
    bin its position claims, the padding), d_srt_cum, d_srt_aux and d_srt_rowbase against torch
    restatements of lt_keeps / lt_key over a0 and ts."""
    import torch
    m = Model(eng, shape, SEED + 7, temp_mode=1, dirty=_dirty(eng, shape) if dirty else None)
    K, P = m.K, m.fields.npix
    nx, ny, nz = shape
    dev = eng.device
    lo, hi = m.ts_range
    inv_h = K / (hi - lo)
    a0, ts = m.fields.a0.view(nx, ny, nz), m.fields.ts.view(nx, ny, nz)
    am = a0.abs()
    keep = (am > 0) & torch.isfinite(am) & ~torch.isnan(ts)
    red = torch.signbit(a0)
    pix = (torch.arange(nx, device=dev).view(nx, 1, 1) * nz +
           torch.arange(nz, device=dev).view(1, 1, nz)).expand(nx, ny, nz)
    binf = torch.clamp(torch.floor((ts - lo) * inv_h), 0, K - 1)
    key = torch.where(red, 0, K) + torch.nan_to_num(binf, nan=0.0).long()
    kp, kq, ka, kt = pix[keep], key[keep], am[keep], ts[keep]
    # counts, start rows, histogram: exact
    cnt = torch.bincount(kq * P + kp, minlength=2 * K * P).view(2 * K, P)
    start_ref = torch.zeros(2 * K + 1, P, dtype=torch.int64, device=dev)
    start_ref[1:] = torch.cumsum(cnt, 0)
    start = m.srt["start"].view(2 * K + 1, P).long()
    assert torch.equal(start, start_ref)
    assert m.hist == [int(v) for v in cnt.sum(1).cpu()]
    # the groups' rows: each as long as its longest lane
    G = (P + 63) // 64
    length = torch.zeros(G * 64, dtype=torch.int64, device=dev)
    length[:P] = start_ref[2 * K]
    rowbase = m.srt["rowbase"]
    assert rowbase[0].item() == 0 and rowbase.numel() == G + 1
    assert torch.equal(rowbase[1:] - rowbase[:-1], length.view(G, 64).max(1).values)
    assert m.srt["rows"] == rowbase[G].item()
    # every sightline's rows, in layout order (p, then row): the key its position claims
    total = int(length.sum().item())
    assert total == ka.numel()
    lp = torch.repeat_interleave(torch.arange(P, device=dev), length[:P])
    first = torch.cumsum(length[:P], 0) - length[:P]
    lr = torch.arange(total, device=dev) - torch.repeat_interleave(first, length[:P])
    addr = (rowbase[lp // 64] + lr) * 64 + lp % 64
    cells = m.srt["cells"].view(-1, 2)
    assert cells.shape[0] == max(1, m.srt["rows"]) * 64
    la, lt = cells[addr, 0], cells[addr, 1]
    lq = torch.repeat_interleave(torch.arange(2 * K, device=dev).repeat(P), cnt.t().reshape(-1))
    assert torch.equal(torch.clamp(torch.floor((lt - lo) * inv_h), 0, K - 1).long(), lq % K)
    # ... and as multisets per (sightline, key) exactly the grid's kept cells

    def canon(p, q, a, t):
        # (stable sorts from the least to the most significant key)
        for sel in (2, 3, None):
            k = (p, q, a, t)[sel] if sel is not None else p * (2 * K) + q
            o = torch.sort(k, stable=True).indices
            p, q, a, t = p[o], q[o], a[o], t[o]
        return p, q, a, t

    for x, y in zip(canon(kp, kq, ka, kt), canon(lp, lq, la, lt)):
        assert torch.equal(x, y)
    # the padding: (0, ts_lo) everywhere else
    pad = torch.ones(cells.shape[0], dtype=torch.bool, device=dev)
    pad[addr] = False
    if m.srt["rows"] > 0:
        assert bool((cells[pad, 0] == 0).all()) and bool((cells[pad, 1] == lo).all())
    # prefix sums of |a0|: to the rounding of two f64 sums of <= n_y terms
    sums = torch.zeros(2 * K * P, dtype=torch.float64, device=dev)
    sums.index_add_(0, kq * P + kp, ka)
    cum_ref = torch.zeros(2 * K + 1, P, dtype=torch.float64, device=dev)
    cum_ref[1:] = torch.cumsum(sums.view(2 * K, P), 0)
    cum = m.srt["cum"].view(2 * K + 1, P)
    assert bool((cum[0] == 0).all())
    tol = 2 * (ny + 2 * K) * 2.0 ** -53
    assert bool(((cum - cum_ref).abs() <= tol * cum_ref[2 * K]).all())
    # aux: |a0| of the cells with a NaN launch time per jet (infinite weights included), and the
    # flag of an infinite weight with a finite launch time
    aux = m.srt["aux"].view(3, P)
    nan_t = (am > 0) & torch.isnan(ts)
    for j, mask in ((0, nan_t & red), (1, nan_t & ~red)):
        want = torch.where(mask, am, torch.zeros_like(am)).sum(1).reshape(P)
        assert torch.equal(torch.isinf(aux[j]), torch.isinf(want))
        fin = torch.isfinite(want)
        assert bool(((aux[j] - want).abs()[fin] <= 2 * ny * 2.0 ** -53 * want[fin]).all())
    has_inf = (torch.isinf(am) & ~torch.isnan(ts)).any(1).reshape(P)
    assert torch.equal(aux[2] != 0, has_inf)
    if dirty:
        assert int(has_inf.sum()) >= 1 and bool(torch.isinf(aux[1]).any()) and int(nan_t.sum()) > 1000


# ---- a K4-built jet on the production route ------------------------------------------------------------
def _k4_params(ejection=None):
    from tests.test_host_logic import example_params
    p = example_params()
    # the example's box (25 x 200 x 25 au) on cells 3.64 times finer across the jet
    p["grid"].update(n_x=182, n_y=512, n_z=182, c_size=0.5 * 50.0 / 182.0)
    if ejection is not None:
        p["ejection"] = ejection
    return p


@pytest.mark.parametrize("which", ["example", "random"])
def test_k4_built_jet_on_the_production_route(eng, tmp_path, which):
    """JetModel -> K4 -> tau layout -> the bucketed layout attached by the producer -> hybrid scan,
    182 x 512 x 182 (33124 sightlines: 36 live lanes in the last group): whole maps of
    optical_depth_ff and flux_ff against the oracle on the downloaded K4 fields at 1e-11, exact
    zero pattern.  Epochs: three across the model's launch-time range and two chosen with the host
    plan.  The launch times of this box span a few tenths of a year, far less than the bursts'
    supports (years), so at every epoch inside the range all cells are in the support and the
    plan keeps the grid order; the bucketed layout is taken only where an edge of a support,
    t - s_hi or t - s_lo, cuts through the launch-time range -- the two chosen epochs put it
    there, at the first positions (in steps of a tenth of the range) that leave <= 90 % of the
    cells to read."""
    from rajepy_amd import classes, logger
    ej = None
    if which == "random":
        rng = np.random.default_rng(77)
        ej = {"t_0": rng.uniform(0.2, 2.0, 5), "hl": rng.uniform(0.1, 0.6, 5),
              "chi": rng.uniform(1.5, 20.0, 5), "which": np.array(["R", "B", "RB", "B", "R"])}
    p = _k4_params(ej)
    jm = classes.JetModel(copy.deepcopy(p), log=logger.Log(str(tmp_path / "a.log"), verbose=False),
                          engine=eng)
    dev = jm._wide_fields()
    assert (jm.nx, jm.ny, jm.nz) == (182, 512, 182) and dev.npix % 64 == 36
    assert dev.srt is not None and dev.srt["mom"] is not None and dev.srt["K"] == 32
    K, N = dev.srt["K"], dev.srt["N"]
    hist = [int(v) for v in dev.srt["hist"]]
    lo, hi = dev.ts_range
    stats = U.srt_group_stats(dev.srt["start"].cpu().numpy().reshape(2 * K + 1, dev.npix), K)
    grid = lambda t: t.cpu().numpy().astype(np.float64).reshape(jm.nx, jm.ny, jm.nz)
    nd, pf = grid(dev.nd), grid(dev.pf)
    jet = orc.OracleJet.from_fields(copy.deepcopy(p), np.abs(nd), grid(dev.xi), grid(dev.temp), pf,
                                    np.ones_like(pf), grid(dev.ts),
                                    np.where(np.signbit(nd), -1.0, 1.0))
    bursts = (jm._bursts["R"], jm._bursts["B"])
    sup = [U._support(b) for b in bursts]
    epochs = [float(t) for t in np.linspace(lo, hi, 5)[1:4]]
    cands = [s + lo + f * (hi - lo) for s in (max(s[1] for s in sup), min(s[0] for s in sup))
             for f in np.arange(0.1, 1.0, 0.1)]
    picked = [t for t in cands if (lambda pl: pl["layout"] == "sorted" and pl["b1"] != [0, 0])(
        U.srt_plan_host(hist, (lo, hi), K, bursts, t))]
    assert len(picked) >= 2, "no epoch leaves <= 90 % of the cells to read"
    epochs += [picked[0], picked[-1]]
    freqs = np.array([1e9, 5e9])
    n_sorted = 0
    for t in epochs:
        jm.time = jet.time = t
        tau = jm.optical_depth_ff(freqs)
        plan = U.srt_plan_host(hist, (lo, hi), K, bursts, t)
        assert eng.last_scan_path()[0] == "table"
        assert eng.last_scan_layout() == plan["layout"], (t / YEAR, plan)
        bins = eng.last_srt_bins()
        if plan["layout"] == "sorted":
            n_sorted += 1
            triples, cap = U.srt_counts_host(stats, K, N, plan, bursts, (lo, hi), t)
            assert bins[0] + bins[1] == triples and bins[0] <= cap, (bins, triples, cap)
        else:
            assert bins == (0, 0)
        flux = jm.flux_ff(freqs)
        with np.errstate(all="ignore"):
            tau_ref, flux_ref = jet.optical_depth_ff(freqs), jet.flux_ff(freqs)
        assert np.array_equal(tau == 0, tau_ref == 0)
        np.testing.assert_allclose(tau, tau_ref, rtol=1e-11, atol=0)
        assert np.array_equal(np.isnan(flux), np.isnan(flux_ref))
        assert np.array_equal(flux == 0, flux_ref == 0)
        # (the oracle forms 1 - exp(-tau) as the reference does: its own rounding is 2^-53 / tau
        # on thin columns, which the bound on the flux has to carry)
        ok = np.isfinite(flux_ref) & (flux_ref != 0)
        rel_f = np.abs(flux[ok] - flux_ref[ok]) / flux_ref[ok]
        assert np.all(rel_f <= 1e-11 + 2.0 ** -52 / tau_ref[ok]), rel_f.max()
        nz_ = tau_ref != 0
        print("K4 jet (%s bursts), %.3f yr: plan %s, share of cells read %.3f, (contracted, read) "
              "%s, worst rel tau %.3g" % (which, t / YEAR, plan["layout"], plan["share"], bins,
                                          np.max(np.abs(tau[nz_] - tau_ref[nz_]) / tau_ref[nz_])))
    assert n_sorted >= 2, n_sorted
