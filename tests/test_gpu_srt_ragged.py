"""The bucketed single-epoch scans (ff_scan_sorted_kernel, ff_scan_hybrid_kernel; ff_scan_tab.hip)
on groups whose lanes' runs are as ragged as a layout allows, and the scan's per-group bin
counters (rjp_last_srt_bins).

A wave streams the rows from the smallest start to the largest end of its lanes' runs; a lane loads
and sums the rows of ITS OWN run only.  The cases below are built by moving cells to other launch
times before the layout is built: one lane of a group with every cell in the bins a scan reads and
63 with none, the reverse, runs of 1 .. 7 rows, runs of 0, 5, 10, ... 315 rows, epochs whose first
bin is not bin 0 (ragged starts), 58 and 2 live lanes in the last group.  The maps are the smallest
the table path and the layout take (32768 sightlines, 320 rows).

Every case: the hybrid and the moment-free sorted scan against tests/gpu_util.ref_single_epoch
within single_epoch_bound(n_y) (derived in tests/test_gpu_single_epoch_reference.py), the layout
against the host's restatement of the plan, contracted + read == the (group, jet, bin) triples of
the host and contracted <= its cap.  The poison test overwrites every cell OUTSIDE the lanes' runs
with NaN: the map must not change by a bit.  (That held before loads were restricted to a lane's
own run as well -- the clamp of the table lookup absorbs a NaN launch time and a select dropped
the weight of a foreign row; now that the select is gone the property rests on the load predicate
alone, and this test guards it.)"""
import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
YEAR = orc.YEAR
SEED = 20251001
NY = 320
FULL = (128, NY, 256)             # 32768 sightlines: 512 full groups, every group in one jet
LAST58 = (131, NY, 254)           # 33274 = 519 x 64 + 58; groups that hold both jets
LAST2 = (145, NY, 226)            # 32770 = 512 x 64 + 2


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    e.cache_moments = False
    yield e
    e.close()


def _ragged_ts(ts, shape, rng):
    """Move the cells of a few groups to other launch times (host array [n_x, n_y, n_z], in
    place).  `early`: half in bins 0-3, half in bin 12 -- inside both jets' support at 1.0 and
    0.3 yr, and where the narrow burst of _narrow() sits; `late`: bins 23-31, which neither those
    scans nor the narrow one read.  Both stay inside the field's launch-time range (0 .. 5 yr,
    K = 32 bins of 0.15625 yr)."""
    nx, ny, nz = shape
    P = nx * nz
    G = (P + 63) // 64
    early = lambda n: np.where(rng.random(n) < 0.5, rng.uniform(0.01, 0.55, n),
                               rng.uniform(1.885, 2.02, n)) * YEAR
    late = lambda n: rng.uniform(3.6, 4.9, n) * YEAR

    def column(p, n_early):
        x, z = divmod(p, nz)
        col = late(ny)
        col[:n_early] = early(n_early)
        ts[x, :, z] = rng.permutation(col)

    for lane in range(64):
        column(5 * 64 + lane, ny if lane == 0 else 0)            # one lane holds it all
        column(6 * 64 + lane, 0 if lane == 17 else ny)           # ... the reverse
        column(7 * 64 + lane, 1 + (3 * lane) % 7)                # runs of 1 .. 7 rows
        column(8 * 64 + lane, 5 * lane)                          # 0, 5, ... 315 rows
        column((G // 2) * 64 + lane, 1 + (3 * lane) % 7)         # (the middle of the map)
        p = (G - 1) * 64 + lane                                  # the last group: 3 rows a lane
        if p < P:
            column(p, 3 * (lane % 20))


class Model:
    def __init__(self, eng, shape, seed):
        import torch
        from rajepy_amd import engine as E
        self.eng, self.shape, self.mode = eng, shape, E.RJP_GFF_SCALAR
        f = eng.synth_fields(shape, seed, 0, 8, csize_au=0.5, tau_mode=self.mode, wide=False,
                             with_em0=False)
        ts = f.ts.cpu().numpy().reshape(shape).copy()
        _ragged_ts(ts, shape, np.random.default_rng(seed))
        f.ts.copy_(torch.from_numpy(ts.ravel()).to(eng.device))
        srt = eng.build_sorted(f)
        assert srt is not None and srt["mom"] is not None and srt["K"] == 32 and srt["N"] == 20
        self.fields, self.srt, self.K, self.N = f, srt, srt["K"], srt["N"]
        self.a0, self.ts = f.a0.cpu().numpy().reshape(shape), ts
        self.hist = [int(v) for v in srt["hist"]]
        self.ts_range = f.ts_range
        self.start = srt["start"].cpu().numpy().reshape(2 * self.K + 1, f.npix)
        self.stats = U.srt_group_stats(self.start, self.K)
        self._refs = {}

    def ref(self, bursts, t):
        key = (repr(bursts), float(t))
        if key not in self._refs:
            self._refs[key] = U.ref_single_epoch(self.a0, self.ts, bursts, t).ravel()
        return self._refs[key]


_models = {}


@pytest.fixture(scope="module")
def model(eng):
    def get(shape):
        if shape not in _models:
            _models[shape] = Model(eng, shape, SEED + shape[0])
        return _models[shape]
    yield get
    _models.clear()


def _scan(m, bursts, t, moments=True):
    """-> (map [P] on the device, layout, (contracted, read))"""
    from rajepy_amd import engine as E
    eng = m.eng
    eng.use_srt_moments = moments
    try:
        a = eng.ff_scan(m.fields, E.make_bursts(*bursts), [t], m.mode, want_em=False,
                        want_tavg=False)[0].clone()
    finally:
        eng.use_srt_moments = True
    eng.synchronize()
    assert not eng.range_guard()
    assert eng.last_scan_path()[0] == "table"
    return a[0], eng.last_scan_layout(), eng.last_srt_bins()


def _narrow(m):
    """test_narrow_burst_contracts_nothing's burst (tests/test_gpu_srt_moments.py): far narrower
    than a bin, both jets' peaks launched at the centre of bin 12 at 1.0 yr."""
    lo, hi = m.ts_range
    h = (hi - lo) / m.K
    t0 = 1.0 * YEAR - (lo + 12.5 * h)
    return ([(t0, 5.0, h / 40)], [(t0, 3.0, h / 40)])


def _check(m, bursts, t, what):
    """Both bucketed scans against the reference, the plan and the counters; -> the maps."""
    plan = U.srt_plan_host(m.hist, m.ts_range, m.K, bursts, t)
    assert plan["layout"] == "sorted", (what, plan)
    ref = m.ref(bursts, t)
    hyb, lay_h, bins = _scan(m, bursts, t)
    srt, lay_s, bins_s = _scan(m, bursts, t, moments=False)
    assert lay_h == plan["layout"] and lay_s == plan["layout"], (what, lay_h, lay_s, plan)
    assert bins_s == (0, 0), (what, bins_s)
    triples, cap = U.srt_counts_host(m.stats, m.K, m.N, plan, bursts, m.ts_range, t)
    assert bins[0] + bins[1] == triples, (what, bins, triples)
    assert bins[0] <= cap, (what, bins, cap)
    rel_h = U.against(hyb.cpu().numpy(), ref, U.single_epoch_bound(NY), (what, "hybrid"))
    rel_s = U.against(srt.cpu().numpy(), ref, U.single_epoch_bound(NY), (what, "sorted"))
    print("%s: plan %s, (contracted, read) %s of %d (cap %d), rel. hybrid %.2e sorted %.2e" %
          (what, (plan["b0"], plan["b1"]), bins, triples, cap, rel_h, rel_s))
    return plan, hyb, srt, bins


CASES = {"example_1.0": (None, 1.0), "example_0.3": (None, 0.3), "red_4.0": ("R", 4.0),
         "red_6.5": ("R", 6.5)}


@pytest.mark.parametrize("shape", [FULL, LAST58, LAST2], ids=["full", "last58", "last2"])
@pytest.mark.parametrize("case", list(CASES))
def test_ragged_runs_against_the_reference(model, shape, case):
    only, years = CASES[case]
    m = model(shape)
    plan, _, _, bins = _check(m, U.example_burst_lists(only), years * YEAR, (case, shape))
    if case == "red_6.5":
        # the red bursts' support ends 5.86 yr after launch: the first bins are past it, every
        # lane's run starts at its own row
        assert plan["b0"][0] > 0 and plan["b1"][0] == m.K and plan["b1"][1] == 0, plan
    if case.startswith("example"):
        assert bins[0] > 0 and bins[1] > 0, bins          # both kinds of bins in one scan


@pytest.mark.parametrize("shape", [FULL, LAST58, LAST2], ids=["full", "last58", "last2"])
def test_nothing_contracted_is_the_sorted_scan_bit_for_bit(model, shape):
    import torch
    m = model(shape)
    _, hyb, srt, bins = _check(m, _narrow(m), 1.0 * YEAR, ("narrow", shape))
    assert bins[0] == 0 and bins[1] > 0, bins
    assert torch.equal(hyb.view(torch.int64), srt.view(torch.int64))


def _poison_outside_runs(m, plan):
    """(NaN, NaN) into every cell of the layout that is outside [start(b0), start(b1)) of its
    lane for both jets, the padding rows included; -> the number of cells kept."""
    import torch
    srt, K, P = m.srt, m.K, m.fields.npix
    dev = srt["cells"].device
    cells = srt["cells"].view(-1, 64, 2)
    rowbase = srt["rowbase"].long()
    G = rowbase.numel() - 1
    start = torch.zeros(2 * K + 1, G * 64, dtype=torch.int64, device=dev)
    start[:, :P] = srt["start"].view(2 * K + 1, P).long()
    R = torch.arange(cells.shape[0], device=dev)
    g = torch.bucketize(R, rowbase[1:].contiguous(), right=True).clamp(max=G - 1)
    r = (R - rowbase[g])[:, None]                                   # row within the group
    p = g[:, None] * 64 + torch.arange(64, device=dev)[None, :]     # [rows, 64] sightlines
    keep = torch.zeros_like(p, dtype=torch.bool)
    for j in range(2):
        b0, b1 = plan["b0"][j], plan["b1"][j]
        keep |= (r >= start[j * K + b0][p]) & (r < start[j * K + b1][p])
    cells[~keep] = float("nan")
    return int(keep.sum().item())


def test_cells_outside_the_runs_never_reach_the_sums(eng):
    """Nothing a row outside a lane's run holds reaches the lane's sum: with every such cell
    (NaN, NaN) the moment-free scan and the hybrid scan that contracts nothing give the same map
    bit for bit.  (The bins that are not read come from the layout's prefix sums.)  A regression
    guard: the kernels no longer mask a foreign row's weight, they do not load it -- a wrong load
    predicate would put NaN x chi^2 into the sum."""
    import torch
    m = Model(eng, FULL, SEED + 7)          # (its own model: the layout is ruined afterwards)
    for bursts, t, what in ((_narrow(m), 1.0 * YEAR, "narrow"),
                            (U.example_burst_lists("R"), 6.5 * YEAR, "red_6.5")):
        plan = U.srt_plan_host(m.hist, m.ts_range, m.K, bursts, t)
        clean_s, lay, _ = _scan(m, bursts, t, moments=False)
        assert lay == "sorted"
        clean_h = _scan(m, bursts, t)[0] if what == "narrow" else None
        saved = m.srt["cells"].clone()
        kept = _poison_outside_runs(m, plan)
        assert 0 < kept < saved.numel() // 2
        got_s = _scan(m, bursts, t, moments=False)[0]
        assert torch.equal(got_s.view(torch.int64), clean_s.view(torch.int64)), what
        if clean_h is not None:
            got_h, _, bins = _scan(m, bursts, t)
            assert bins[0] == 0 and bins[1] > 0, bins
            assert torch.equal(got_h.view(torch.int64), clean_h.view(torch.int64)), what
        m.srt["cells"].copy_(saved)


def test_counters_are_each_scans_own(model):
    """The counters live in one pair of words per group, written (not added to) by the scan: a
    map of 512 groups scanned after one of 520 reports its own triples, and a scan repeated
    reports the same pair."""
    big, small = model(LAST58), model(FULL)
    bursts, t = U.example_burst_lists(), 1.0 * YEAR
    want = {}
    for m in (big, small):
        plan = U.srt_plan_host(m.hist, m.ts_range, m.K, bursts, t)
        want[m] = U.srt_counts_host(m.stats, m.K, m.N, plan, bursts, m.ts_range, t)[0]
    assert want[big] != want[small]
    b1 = _scan(big, bursts, t)[2]
    s1 = _scan(small, bursts, t)[2]
    s2 = _scan(small, bursts, t)[2]
    b2 = _scan(big, bursts, t)[2]
    assert sum(b1) == want[big] and sum(s1) == want[small], (b1, s1, want)
    assert s2 == s1 and b2 == b1, (b1, b2, s1, s2)
    # a scan without moments in between reports (0, 0), the next hybrid scan its own again
    assert _scan(small, bursts, t, moments=False)[2] == (0, 0)
    assert _scan(small, bursts, t)[2] == s1
