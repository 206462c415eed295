"""Table-residual bins of the hybrid single-epoch scan (ff_scan_hybrid_kernel, srt_err_kernel,
srt_coef_kernel's check (b'); the packed state of ff_lt.hip's srt_pack_kernel) on the device.

A bin that passes check (a) and fails check (b) only by the table's own interpolation error is
contracted from its moments, and sum |a0| E~(ts) over its cells is streamed from the packed state
(launch time + 16-bit weight).  Every case compares
  (i)  the same engine with `use_srt_packed = False` (those bins read cell by cell through the
       table), per sightline, at 2 kSrtMomTol + 2^-9 x 2.2e-13: each of the two maps is within
       kSrtMomTol of the table path per contracted bin, and the 16-bit weight multiplies a term
       that is <= 2.2e-13 of the bin's sum;
  (ii) tests/gpu_util.ref_single_epoch at single_epoch_bound(n_y),
and asserts the residual count (rjp_last_srt_resid) and that rjp_last_srt_bins is the same with the
switch on and off.  The host's expectation of which bins can be residual comes from the NumPy
restatement in tests/test_srt_residual_cpu.py.

The maps are the smallest the table path takes (32768 sightlines).  Their launch times are drawn so
that most cells fall into the bins the restatement calls residual (a lane's run there is longer
than the 25 rows the byte rule asks for, starts at any row offset mod 8, and sits between
contracted bins), a sixteenth of the groups keeps uniform launch times (their short runs stay on
the 16-byte path: read bins beside residual ones), and a quarter of the sightlines hold both jets."""
import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U
from tests import test_srt_residual_cpu as R

pytestmark = pytest.mark.gpu
YEAR = orc.YEAR
SEED = 20261020
K, N = R.K, R.N
ONOFF_RTOL = 2 * U.SRT_MOM_TOL + 2.0 ** -9 * 2.2e-13
S320, S480 = (128, 320, 256), (128, 480, 256)
ODD = (131, 320, 254)             # 33274 sightlines = 519 x 64 + 58: dead lanes in the last group
S96 = (128, 96, 256)


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    e.cache_moments = False
    yield e
    e.close()


_verdicts = {}


def res_bins(bursts, t):
    """Per jet the bins the restatement calls residual at epoch t (launch times over 0 .. 5 yr)."""
    key = (repr(bursts), float(t))
    if key not in _verdicts:
        v = R.verdicts(bursts, t)
        _verdicts[key] = [[b for b, (k, _, _) in v[j].items() if k == "res"] for j in range(2)]
    return _verdicts[key]


class Model:
    """Synthetic fields whose launch times are redrawn on the host (see the module's docstring);
    `ts_fn(red [n_x, n_y, n_z] bool, rng) -> ts` replaces the default draw; `a0_edit(a0)` edits the
    weights in place before the layout is built."""

    def __init__(self, eng, shape, seed, ts_fn=None, a0_edit=None, both_jets=True):
        import torch
        from rajepy_amd import engine as E
        self.eng, self.shape, self.mode = eng, shape, E.RJP_GFF_SCALAR
        nx, ny, nz = shape
        f = eng.synth_fields(shape, seed, 0, 8, csize_au=0.5, tau_mode=self.mode, wide=False,
                             with_em0=False)
        rng = np.random.default_rng(seed)
        a0 = f.a0.cpu().numpy().reshape(shape).copy()
        if both_jets:                      # every fourth sightline: its first rows in the other jet
            a0.reshape(nx, ny, nz)[:, :ny // 2, ::4] *= -1.0
        if a0_edit is not None:
            a0_edit(a0)
        red = np.signbit(a0)
        ts = (ts_fn or self._draw)(red, rng)
        ts[0, 0, 0], ts[0, 1, 0] = 0.0, 5.0 * YEAR           # the range is 0 .. 5 yr exactly
        f.a0.copy_(torch.from_numpy(a0.ravel()).to(eng.device))
        f.ts.copy_(torch.from_numpy(ts.ravel()).to(eng.device))
        f.ts_range = None
        srt = eng.build_sorted(f)
        assert srt is not None and srt["mom"] is not None and srt["K"] == K and srt["N"] == N
        assert tuple(f.ts_range) == R.TS_RANGE, f.ts_range
        self.fields, self.srt, self.a0, self.ts = f, srt, a0, ts
        self.start = srt["start"].cpu().numpy().reshape(2 * K + 1, f.npix)
        self.stats = U.srt_group_stats(self.start, K)
        self._refs = {}

    @staticmethod
    def _draw(red, rng):
        nx, ny, nz = red.shape
        h = 5.0 * YEAR / K
        want = res_bins(U.example_burst_lists(), 1.0 * YEAR)
        ts = rng.uniform(0.001, 4.999, red.shape) * YEAR
        for j, mask in ((0, red), (1, ~red)):
            bins = np.array(want[j])
            pick = rng.random(red.shape) < 0.75
            # a sixteenth of the groups of 64 sightlines keeps the uniform draw
            grp = (np.arange(nx * nz).reshape(nx, 1, nz) // 64) % 16 == 3
            sel = mask & pick & ~grp
            n = int(sel.sum())
            ts[sel] = (rng.choice(bins, n) + rng.uniform(0.001, 0.999, n)) * h
        return ts

    def ref(self, bursts, t):
        key = (repr(bursts), float(t))
        if key not in self._refs:
            self._refs[key] = U.ref_single_epoch(self.a0, self.ts, bursts, t).ravel()
        return self._refs[key]

    def cap(self, bursts, t):
        """The (group, jet, bin) triples that can be residual: the restatement's residual bins in
        the groups that hold the jet and pass the byte rule (longest run x 6 B > (N - 1) x 8 B)."""
        held, longest = self.stats
        return sum(int((held[j] & (longest[j * K + b] * 6 > (N - 1) * 8)).sum())
                   for j in range(2) for b in res_bins(bursts, t)[j])


def scan(m, bursts, t, packed=True):
    """-> (map [P] on the device, (contracted, read), residual count)"""
    from rajepy_amd import engine as E
    eng = m.eng
    eng.use_srt_packed = packed
    try:
        a = eng.ff_scan(m.fields, E.make_bursts(*bursts), [t], m.mode, want_em=False,
                        want_tavg=False)[0].clone()
    finally:
        eng.use_srt_packed = True
    eng.synchronize()
    assert not eng.range_guard()
    assert eng.last_scan_path()[0] == "table" and eng.last_scan_layout() == "sorted"
    return a[0], eng.last_srt_bins(), eng.last_srt_resid()


def check(m, bursts, t, what, expect_resid=True):
    on, bins_on, n_res = scan(m, bursts, t)
    off, bins_off, n_off = scan(m, bursts, t, packed=False)
    assert n_off == 0 and bins_on == bins_off, (what, n_off, bins_on, bins_off)
    cap = m.cap(bursts, t)
    print("%s: (contracted, read) %s, residual %d (host: <= %d)" % (what, bins_on, n_res, cap))
    assert n_res <= min(cap, bins_on[1]), (what, n_res, cap, bins_on)
    if expect_resid:
        assert n_res > 0, (what, cap)
    else:
        assert n_res == 0, (what, n_res)
    a, b = on.cpu().numpy(), off.cpu().numpy()
    rel = U.against(a, b, ONOFF_RTOL, (what, "on / off"))
    ny = m.shape[1]
    rel_ref = U.against(a, m.ref(bursts, t), U.single_epoch_bound(ny), (what, "reference"))
    print("%s: rel. on / off %.2e (<= %.2e), reference %.2e (<= %.2e)"
          % (what, rel, ONOFF_RTOL, rel_ref, U.single_epoch_bound(ny)))
    return on, off, n_res


_models = {}


@pytest.fixture(scope="module")
def model(eng):
    def get(shape):
        if shape not in _models:
            _models[shape] = Model(eng, shape, SEED + shape[0] + shape[1])
        return _models[shape]
    yield get
    _models.clear()


@pytest.mark.parametrize("years", [1.0, 0.3])
@pytest.mark.parametrize("shape", [S320, S480, ODD], ids=["320", "480", "dead_lanes"])
def test_residual_bins_against_the_cell_path_and_the_reference(model, shape, years):
    m = model(shape)
    bursts = U.example_burst_lists()
    check(m, bursts, years * YEAR, (shape, years))


def test_runs_start_at_every_row_offset_and_sit_between_read_and_contracted_bins(model):
    m = model(S320)
    bursts, t = U.example_burst_lists(), 1.0 * YEAR
    want = res_bins(bursts, t)
    held, longest = m.stats
    offs = set()
    for j in range(2):
        for b in want[j]:
            offs |= set(np.unique(m.start[j * K + b] % 8).tolist())
            # in some groups the bin pays, in others (the uniform ones) it stays on the cell path
            pays = longest[j * K + b][held[j]] * 6 > (N - 1) * 8
            assert pays.any() and not pays.all(), (j, b)
    assert offs == set(range(8)), offs


def _equal_ts(t_launch):
    def fn(red, rng):
        ts = np.full(red.shape, t_launch)
        # a fifth of every sightline is launched at 4.5 yr, outside both jets' support at 1.0 yr:
        # with every cell inside it the plan would keep the grid order (> 90 % of the cells read)
        ts[:, red.shape[1] * 4 // 5:, :] = 4.5 * YEAR
        # one sightline spans the range, so the bins and the table are the example's
        ts[0, :, 1] = np.linspace(0.0, 5.0 * YEAR, red.shape[1])
        return ts
    return fn


@pytest.mark.parametrize("where", ["inside", "boundary"])
def test_all_launch_times_equal(eng, where):
    """Every cell the scan reads (but one sightline's) launched at the same time, in a bin that is
    residual for the red jet: once inside a table piece, once exactly on a piece boundary of the
    epoch's table."""
    bursts, t = U.example_burst_lists(), 1.0 * YEAR
    ni, lo, inv_h, _ = R.S.chi_table(bursts, R.TS_RANGE, t)
    b = res_bins(bursts, t)[0][len(res_bins(bursts, t)[0]) // 2]
    h = 5.0 * YEAR / K
    # the first table piece boundary inside the bin: t - ts - lo = k / inv_h
    k = int(np.floor((t - (b + 0.5) * h - lo) * inv_h))
    ts0 = t - lo - k / inv_h
    if where == "inside":
        ts0 -= 0.37 / inv_h
    assert b * h < ts0 < (b + 1) * h
    m = Model(eng, S320, SEED + 5, ts_fn=_equal_ts(ts0), both_jets=False)
    check(m, bursts, t, ("equal", where))


def test_short_sightlines_stay_on_the_sixteen_byte_path(eng):
    """n_y = 96 with uniform launch times: no lane's run reaches the 26 rows of the byte rule."""
    import torch
    uniform = lambda red, rng: rng.uniform(0.001, 4.999, red.shape) * YEAR
    m = Model(eng, S96, SEED + 96, ts_fn=uniform)
    assert m.srt["packed"] is not None
    assert (m.stats[1] * 6 <= (N - 1) * 8).all()
    on, off, _ = check(m, U.example_burst_lists(), 1.0 * YEAR, "n_y 96", expect_resid=False)
    assert torch.equal(on.view(torch.int64), off.view(torch.int64))


def test_packed_rows_outside_the_residual_runs_never_reach_the_sums(eng):
    """NaN launch times and NaN weights in every packed row outside the residual bins' runs of its
    lane (the padding included): the map does not change by a bit."""
    import torch
    m = Model(eng, S320, SEED + 11)
    bursts, t = U.example_burst_lists(), 1.0 * YEAR
    clean, _, n_clean = scan(m, bursts, t)
    assert n_clean > 0
    srt, P = m.srt, m.fields.npix
    dev = srt["cells"].device
    rowbase = srt["rowbase"].long()
    G = rowbase.numel() - 1
    prow = ((rowbase[:-1] + 7) // 8) * 8 + 8 * torch.arange(G, device=dev)      # first packed rows
    rows = srt["packed"]["rows"]
    start = torch.zeros(2 * K + 1, G * 64, dtype=torch.int64, device=dev)
    start[:, :P] = srt["start"].view(2 * K + 1, P).long()
    Rr = torch.arange(rows, device=dev)
    g = torch.bucketize(Rr, prow.contiguous(), right=True) - 1
    r = (Rr - prow[g])[:, None]
    p = g[:, None] * 64 + torch.arange(64, device=dev)[None, :]
    keep = torch.zeros_like(p, dtype=torch.bool)
    for j in range(2):
        for b in res_bins(bursts, t)[j]:
            keep |= (r >= start[j * K + b][p]) & (r < start[j * K + b + 1][p])
    assert 0 < int(keep.sum()) < keep.numel()
    # pts[(row / 2) * 64 + lane] = (ts[row], ts[row + 1]); pw[(row / 8) * 64 + lane] = 8 x 16 bits
    pts = srt["packed"]["pts"].view(rows // 2, 64, 2)
    pw = srt["packed"]["pw"].view(rows // 8, 64, 8)
    pts[~keep.view(rows // 2, 2, 64).transpose(1, 2)] = float("nan")
    pw[~keep.view(rows // 8, 8, 64).transpose(1, 2)] = -1            # 0xffff: a NaN once decoded
    got, _, n_res = scan(m, bursts, t)
    assert n_res == n_clean
    assert torch.equal(got.view(torch.int64), clean.view(torch.int64))


def test_a_weight_outside_the_sixteen_bit_range_refuses_the_packed_state(eng):
    import torch

    def huge(a0):
        a0[3, 7, 5] = 1e39
    m = Model(eng, S320, SEED + 13, a0_edit=huge)
    assert m.srt["packed"] is None
    on, off, _ = check(m, U.example_burst_lists(), 1.0 * YEAR, "1e39", expect_resid=False)
    assert torch.equal(on.view(torch.int64), off.view(torch.int64))


def test_a_table_too_large_beside_its_error_table_keeps_the_cell_path(model):
    """A weak burst 0.35 times as wide as the example's narrowest, added to both jets, sets the
    table's step while the wide bursts set its span: more than 320 pieces, so chi table + error
    table would leave the CU one workgroup and the call runs without residual bins."""
    import torch
    m = model(S320)
    ex = U.example_burst_lists()
    sg = min(s for lst in ex for _, _, s in lst)
    bursts = tuple(list(lst) + [(0.5 * YEAR, 0.5, 0.35 * sg)] for lst in ex)
    t = 1.0 * YEAR
    ni = U.chi_table_host(m.shape, R.TS_RANGE, bursts, t)
    assert ni is not None and 2 * ni * (80 + 48) > 80 * 1024 and ni <= U.CHI_MAX_NI, ni
    on, bins_on, n_res = scan(m, bursts, t)
    off, bins_off, _ = scan(m, bursts, t, packed=False)
    assert n_res == 0 and bins_on == bins_off
    assert torch.equal(on.view(torch.int64), off.view(torch.int64))
    U.against(on.cpu().numpy(), m.ref(bursts, t), U.single_epoch_bound(m.shape[1]), "narrow table")


def test_cells_edited_in_place_detach_the_packed_state(eng):
    m = Model(eng, S320, SEED + 17)
    bursts, t = U.example_burst_lists(), 1.0 * YEAR
    assert scan(m, bursts, t)[2] > 0
    m.srt["cells"].mul_(1.0)                     # (the same values: only the version moves)
    assert scan(m, bursts, t)[2] == 0
