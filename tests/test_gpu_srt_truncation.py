"""The hybrid single-epoch scan with truncated coefficient counts and 16-byte moment loads
(ff_scan_tab.hip: srt_coef_kernel's m, ff_scan_hybrid_kernel's plane pairs) against
tests/gpu_util.ref_single_epoch under the derived bound of tests/test_gpu_single_epoch_reference.py,
|got - ref| <= (2.2e-13 + n_y 2^-53) ref -- kChiTol = 1e-13 on chi >= 1 gives 2e-13 on chi^2, 2e-14
(kSrtMomTol) are budgeted for a contracted bin, of which the truncation takes at most a quarter on
top of what the checks saw, plus the rounding of a sum of n_y same-signed terms -- and against the
moment-free sorted scan and the grid-order scan at 1e-13.  The (contracted, read) counters must be
what the host restatement of the plan allows: the truncation moves no bin between the two.

Cases: the example bursts at 1.0 / 0.3 yr for N = 16 / 20 / 24; a map with two live lanes in the last
group (the edge of the 16-byte loads); NaN / zero / infinite cells with both jets in a sightline;
random burst sets; a burst just wide enough for its bins to pass, where some bin keeps all N
coefficients (tests/test_srt_truncation_cpu.py asserts that verdict for the restatement)."""
import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
YEAR = orc.YEAR
SEED = 20241016
MID = (128, 1024, 256)             # 32768 sightlines, 32 cells per bin and lane at K = 32


def bound(ny):
    return 2.2e-13 + ny * 2.0 ** -53


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    e.cache_moments = False
    yield e
    e.close()


class Model:
    """Synthetic fields with the bucketed layout attached, and their host copies."""

    def __init__(self, eng, shape, seed, temp_mode=0, K=32, N=20, dirty=None):
        from rajepy_amd import engine as E
        self.eng, self.shape = eng, shape
        self.mode = E.RJP_GFF_SCALAR if temp_mode == 0 else E.RJP_GFF_POWERLAW
        f = eng.synth_fields(shape, seed, temp_mode, 8, csize_au=0.5, tau_mode=self.mode,
                             wide=False, with_em0=False)
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
        self.K, self.N = K, N
        self.hist = [int(v) for v in srt["hist"]]
        self.ts_range = self.fields.ts_range
        start = srt["start"].cpu().numpy().reshape(2 * K + 1, self.fields.npix)
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
    return a.cpu().numpy()[0], eng.last_scan_layout(), eng.last_srt_bins()


def _against(got, ref, rtol, what):
    assert np.array_equal(got == 0, ref == 0), what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert np.array_equal(np.isinf(got), np.isinf(ref)), what
    ok = np.isfinite(ref) & (ref != 0)
    rel = float(np.max(np.abs(got[ok] - ref[ok]) / ref[ok])) if ok.any() else 0.0
    print("%s: worst relative difference %.3g (bound %.3g)" % (what, rel, rtol))
    assert rel <= rtol, (what, rel, rtol)
    return rel


def check(m, bursts, t, what):
    """The hybrid scan of `m` at `t`: counters against the host plan, maps against the reference
    and the two other orders.  -> (contracted, read)"""
    tag = "%s, N = %d, %.1f yr" % (what, m.N, t / YEAR)
    plan = U.srt_plan_host(m.hist, m.ts_range, m.K, bursts, t)
    assert plan["layout"] == "sorted", (tag, plan)
    got, layout, bins = _scan(m, bursts, t)
    assert layout == "sorted", tag
    triples, cap = U.srt_counts_host(m.stats, m.K, m.N, plan, bursts, m.ts_range, t)
    print("%s: (contracted, read) %s of %d triples, cap %d" % (tag, bins, triples, cap))
    assert bins[0] + bins[1] == triples, (tag, bins, triples)
    assert bins[0] <= cap, (tag, bins, cap)
    _against(got, m.ref(bursts, t), bound(m.shape[1]), tag + " vs reference")
    plain, lay_p, bins_p = _scan(m, bursts, t, moments=False)
    assert lay_p == "sorted" and bins_p == (0, 0), tag
    _against(got, plain, 1e-13, tag + " vs moment-free")
    grid, lay_g, _ = _scan(m, bursts, t, sorted_=False)
    assert lay_g == "grid", tag
    _against(got, grid, 1e-13, tag + " vs grid order")
    return bins


def test_example_bursts_all_orders(eng):
    m = Model(eng, MID, SEED)
    bursts = U.example_burst_lists()
    for N in (16, 20, 24):
        m.attach(32, N)
        for years in (1.0, 0.3):
            con, read = check(m, bursts, years * YEAR, "example")
            assert con > 0, (N, years)


def test_two_live_lanes_in_the_last_group(eng):
    """32770 sightlines: the last group's pair 0 is live, pairs 1-31 must not be loaded."""
    shape = (145, 320, 226)
    m = Model(eng, shape, SEED + 1)
    P = m.fields.npix
    assert P % 64 == 2
    bursts = U.example_burst_lists()
    for years in (1.0, 0.3):
        t = years * YEAR
        con, _ = check(m, bursts, t, "P = %d" % P)
        assert con > 0
        got, ref = _scan(m, bursts, t)[0], m.ref(bursts, t)
        for p in (P - 2, P - 1):
            assert np.isfinite(got[p]) and got[p] > 0
            assert abs(got[p] - ref[p]) <= bound(shape[1]) * ref[p], (p, got[p], ref[p])


def _dirty(eng, shape):
    def edit(f):
        import torch
        g = torch.Generator(device=eng.device)
        g.manual_seed(31)
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


def test_dirty_cells_and_both_jets_in_a_sightline(eng):
    m = Model(eng, MID, SEED + 2, temp_mode=1, dirty=_dirty(eng, MID))
    nx, ny, nz = MID
    for bursts in (U.example_burst_lists(), U.example_burst_lists("B")):
        for years in (1.0, 0.3):
            t = years * YEAR
            con, _ = check(m, bursts, t, "dirty, %d + %d bursts" % (len(bursts[0]), len(bursts[1])))
            assert con > 0
            got, ref = _scan(m, bursts, t)[0], m.ref(bursts, t)
            assert got[5 * nz + 7] == 0.0 and got[6 * nz + 9] == 0.0
            assert np.isinf(got[3 * nz + 5]) and np.isinf(ref[3 * nz + 5])


def random_bursts(seed):
    """1-6 bursts over both jets, sigma 0.1-0.9 yr, relative amplitude 0.1-50 (log-uniform)."""
    rng = np.random.default_rng(SEED + seed)
    lists = ([], [])
    for _ in range(int(rng.integers(1, 7))):
        sigma = 10.0 ** rng.uniform(-1.0, np.log10(0.9))
        amp = 10.0 ** rng.uniform(-1.0, np.log10(50.0))
        lists[int(rng.integers(0, 2))].append((rng.uniform(-0.5, 2.5) * YEAR, amp, sigma * YEAR))
    return lists


def test_random_burst_sets(eng):
    m = Model(eng, MID, SEED + 3)
    done = 0
    for seed in range(12):
        bursts = random_bursts(seed)
        t = (0.3, 1.0, 1.7)[seed % 3] * YEAR
        if U.chi_table_host(MID, m.ts_range, bursts, t) is None or \
                U.srt_plan_host(m.hist, m.ts_range, m.K, bursts, t)["layout"] != "sorted":
            continue                                     # (the Gaussians, or the grid order: not this scan)
        check(m, bursts, t, "random %d" % seed)
        done += 1
        if done == 4:
            break
    assert done == 4


def test_a_burst_just_wide_enough(eng):
    """One burst per jet of 0.40 / 0.42 bin widths: three or four bins per jet pass, and the
    restatement keeps all N = 20 coefficients on one of them (m == N: nothing dropped)."""
    m = Model(eng, MID, SEED + 4)
    lo, hi = m.ts_range
    h = 5.0 * YEAR / 32
    assert abs((hi - lo) / 32 - h) < 1e-4 * h            # the bins of the restatement
    bursts = ([(0.5 * YEAR, 4.0, 0.40 * h)], [(0.5 * YEAR, 2.0, 0.42 * h)])
    con, read = check(m, bursts, 1.0 * YEAR, "just wide enough")
    assert con > 0 and read > 0
