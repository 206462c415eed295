"""Tables ahead of the scan (ff_scan_tab.hip, TabRing): a context builds the chi table and the bin
coefficients / verdicts of a single-epoch scan on a side stream of its own, into a ring of four
table slots, ordered against the caller's stream by events alone.  Nothing of that may change a
result: every test below compares calls that were enqueued back to back (behind a few
milliseconds of other work on the caller's stream, so that they really pile up and the side stream
runs ahead) with the same calls made one at a time, bit for bit.

Map: 128 x 480 x 256 -- 32768 sightlines, the smallest map the table path takes; n_y = 480 is past
the byte rule of the hybrid scan (a bin is contracted only where its longest lane run x 16 B exceeds
(N - 1) x 8 B), so scans at 0.3 / 1.0 / 1.7 yr both contract and read bins.  The producer's own
bucketed layout and moments (K = 32, N = 20).

sum_a is also held against tests/gpu_util.ref_single_epoch within single_epoch_bound(n_y) (derived
in tests/test_gpu_single_epoch_reference.py); tau, flux and ftot are K2's functions of sum_a and
are compared bit for bit between the two ways of calling.  Nine steps wrap the ring twice: a slot
written again before the scan that reads it has finished shows up as a wrong map."""
import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
YEAR = orc.YEAR
SEED = 20261020
SHAPE = (128, 480, 256)
NU = np.array([1e9, 5e9, 4.3e10])
# 2 R + 1 = 9 steps: four epochs, the same four in another order, and one more
EPOCHS = [0.3, 1.0, 1.7, 2.6, 1.7, 0.3, 2.6, 1.0, 1.0]
NAMES = ("sum_a", "tau", "flux", "ftot")


def _engine():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    e.cache_moments = False
    return e


class Model:
    def __init__(self, eng):
        from rajepy_amd import engine as E
        from rajepy_amd.maths import physics as ph
        self.mode = E.RJP_GFF_SCALAR
        f = eng.synth_fields(SHAPE, SEED, 0, 8, csize_au=0.5, tau_mode=self.mode, wide=False,
                             with_em0=False)
        assert f.srt is not None and f.srt["mom"] is not None
        assert f.srt["K"] == 32 and f.srt["N"] == 20
        self.fields = f
        self.ctau, self.cflux = E.ff_channel_coeffs(NU, 0.5, 120., self.mode,
                                                    [ph.gff(nu, 1e4) for nu in NU])
        self.tavg = eng.tavg(f)
        eng.synchronize()
        self.a0 = f.a0.cpu().numpy().reshape(SHAPE)
        self.ts = f.ts.cpu().numpy().reshape(SHAPE)
        self._refs = {}

    def ref(self, bursts, t):
        key = (repr(bursts), float(t))
        if key not in self._refs:
            self._refs[key] = U.ref_single_epoch(self.a0, self.ts, bursts, t).ravel()
        return self._refs[key]


def _step(eng, m, bursts, t):
    """One rjp_ff_step into buffers of its own, not synchronised; -> (sum_a, tau, flux, ftot)"""
    from rajepy_amd import engine as E
    P, F = m.fields.npix, len(NU)
    out = (eng._f64(1, P), None, eng._f64(1, F, P), eng._f64(1, F, P), eng._f64(1, F))
    eng.ff_step(m.fields, E.make_bursts(*bursts), [t], m.mode, m.tavg, m.ctau, m.cflux, out)
    return out[0], out[2], out[3], out[4]


def _plug(eng):
    """A few milliseconds of other work on the current stream: the calls enqueued behind it are
    all waiting when the first of them starts, and the side stream is ahead of every one."""
    import torch
    x = torch.zeros(1 << 28, dtype=torch.float32, device=eng.device)
    for _ in range(6):
        x.add_(1.0)
    return x


def _same(a, b, what):
    import torch
    for name, x, y in zip(NAMES, a, b):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64)), (what, name)


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def model(eng):
    return Model(eng)


@pytest.fixture(scope="module")
def one_by_one(eng, model):
    """The nine steps of EPOCHS with the example bursts, each followed by a synchronisation; the
    paths they took and the bin counters after the last."""
    bursts = U.example_burst_lists()
    outs, paths = [], []
    for years in EPOCHS:
        outs.append(_step(eng, model, bursts, years * YEAR))
        eng.synchronize()
        paths.append((eng.last_scan_path()[0], eng.last_scan_layout()))
    assert not eng.range_guard()
    return outs, paths, eng.last_srt_bins()


def test_one_by_one_against_the_reference(model, one_by_one):
    outs, paths, bins = one_by_one
    bursts = U.example_burst_lists()
    assert all(p[0] == "table" for p in paths), paths
    assert ("table", "sorted") in paths, paths
    assert bins[0] > 0 and bins[1] > 0, bins              # the last step contracts and reads
    for years, out in zip(EPOCHS, outs):
        rel = U.against(out[0].cpu().numpy().ravel(), model.ref(bursts, years * YEAR),
                        U.single_epoch_bound(SHAPE[1]), ("one by one", years))
        print("%.1f yr: rel. %.2e" % (years, rel))


def test_back_to_back_steps_equal_the_synchronised_ones(eng, model, one_by_one):
    want, _, bins = one_by_one
    bursts = U.example_burst_lists()
    x = _plug(eng)
    outs = [_step(eng, model, bursts, years * YEAR) for years in EPOCHS]
    eng.synchronize()
    assert not eng.range_guard()
    for i, (a, b) in enumerate(zip(outs, want)):
        _same(a, b, ("back to back", i, EPOCHS[i]))
        U.against(a[0].cpu().numpy().ravel(), model.ref(bursts, EPOCHS[i] * YEAR),
                  U.single_epoch_bound(SHAPE[1]), ("back to back", i, EPOCHS[i]))
    # the counters are the last scan's, whichever way it was enqueued
    assert eng.last_srt_bins() == bins
    del x


def _burst_lists():
    """A different burst list for every call, so that every call stages a new burst table: in
    turn one that takes the hybrid scan, one that chi_table_plan refuses (a dip: chi < 1 keeps the
    Gaussians) and one that keeps the grid order (its support holds every launch time)."""
    red, blue = U.example_burst_lists()
    calls = []
    for k in range(3):
        s = 1.0 + 0.125 * k
        calls.append((([(t0, a * s, sg) for t0, a, sg in red], [(t0, a * s, sg) for t0, a, sg in blue]),
                      1.0 * YEAR, ("table", "sorted")))
        calls.append((([(0.5 * YEAR, -0.25 * s, 0.1 * YEAR)], list(blue)), 1.0 * YEAR,
                      ("tiles", "grid")))
        calls.append((([(1.0 * YEAR, 2.0 * s, 2.0 * YEAR)], [(1.5 * YEAR, 1.0, 2.0 * YEAR)]),
                      1.0 * YEAR, ("table", "grid")))
    return calls


def test_changing_bursts_equal_the_calls_made_alone(eng, model):
    calls = _burst_lists()
    x = _plug(eng)
    outs = [_step(eng, model, b, t) for b, t, _ in calls]
    eng.synchronize()
    assert not eng.range_guard()
    del x
    for i, (b, t, path) in enumerate(calls):
        fresh = _engine()
        try:
            alone = _step(fresh, model, b, t)
            fresh.synchronize()
            assert (fresh.last_scan_path()[0], fresh.last_scan_layout()) == path, (i, path)
            assert not fresh.range_guard()
            _same(outs[i], alone, ("changing bursts", i, path))
        finally:
            fresh.close()


def test_on_another_stream(eng, model, one_by_one):
    import torch
    want = one_by_one[0]
    bursts = U.example_burst_lists()
    side = torch.cuda.Stream(device=eng.device)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        x = _plug(eng)
        outs = [_step(eng, model, bursts, years * YEAR) for years in EPOCHS]
    side.synchronize()
    torch.cuda.synchronize()
    assert not eng.range_guard()
    for i, (a, b) in enumerate(zip(outs, want)):
        _same(a, b, ("another stream", i, EPOCHS[i]))
    del x


def test_two_engines_in_turn_and_one_closed_in_between(eng, model, one_by_one):
    want = one_by_one[0]
    bursts = U.example_burst_lists()
    other = _engine()
    try:
        x = _plug(eng)
        outs = [_step(other if i % 2 else eng, model, bursts, years * YEAR)
                for i, years in enumerate(EPOCHS)]
        eng.synchronize()
        for i, (a, b) in enumerate(zip(outs, want)):
            _same(a, b, ("two engines", i, EPOCHS[i]))
        # a step enqueued on the other engine, that engine closed while the step may still run
        # (rjp_ctx_destroy waits for the device), and the next call on this one
        x = _plug(eng)
        last = _step(other, model, bursts, EPOCHS[1] * YEAR)
    finally:
        other.close()
    after = _step(eng, model, bursts, EPOCHS[2] * YEAR)
    eng.synchronize()
    assert not eng.range_guard()
    _same(last, want[1], "the closed engine's last step")
    _same(after, want[2], "the step after another engine's close")
    del x
