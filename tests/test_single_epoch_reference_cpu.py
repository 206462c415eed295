"""Pins tests/gpu_util.ref_single_epoch -- the independent f64 reference the single-epoch GPU tests
are judged by -- to the reference project's golden optical-depth maps, and the host restatement of
the bin plan to hand-worked cases.  CPU only."""
import numpy as np
import pytest

from oracle import rt_oracle as orc
from rajepy_amd import engine as E
from rajepy_amd.maths import physics as ph
from tests import gpu_util as U


def _burst_lists(p):
    red, blue = [], []
    e = p["ejection"]
    for t0, hl, chi, which in zip(e["t_0"], e["hl"], e["chi"], e["which"]):
        sig = hl * orc.YEAR * 2. / (2. * np.sqrt(2. * np.log(2.)))
        for jet, lst in (("R", red), ("B", blue)):
            if jet in str(which):
                lst.append((t0 * orc.YEAR, chi - 1., sig))
    return red, blue


@pytest.mark.parametrize("tag", ["cfg1_example", "tilted"])
def test_reference_equals_the_golden_optical_depths(tag):
    z, meta, p, g, jet = U.golden_dense(tag)
    q_T = p["power_laws"]["q_T"]
    mode = E.RJP_GFF_SCALAR if q_T == 0. else E.RJP_GFF_POWERLAW
    freqs = z["freqs"]
    gv = [ph.gff(nu, p["properties"]["T_0"]) for nu in freqs] if q_T == 0. else None
    ctau, _ = E.ff_channel_coeffs(freqs, jet.csize, p["target"]["dist"], mode, gv)
    a0 = U.golden_a0(g, q_T)
    bursts = _burst_lists(p)
    worst = 0.0
    for e, yr in enumerate(z["years"]):
        for threads in (1, 4):
            ref = U.ref_single_epoch(a0, g["ts"], bursts, yr * orc.YEAR, slab_cells=200000,
                                     threads=threads)
            for f in range(len(freqs)):
                want = z["tau_ff"][e, f]
                got = ctau[f] * ref
                assert np.array_equal(got == 0, want == 0)
                nz = want != 0
                worst = max(worst, np.max(np.abs(got[nz] - want[nz]) / want[nz]))
                np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)
    print("%s: ctau * ref_single_epoch vs the golden tau maps, worst relative difference %.3g"
          % (tag, worst))


def test_reference_nansum_semantics():
    """NaN terms are skipped; a jet without bursts has chi == 1 whatever its launch times; an
    infinite weight gives inf (when its term is not NaN); the sign bit picks the jet."""
    yr = orc.YEAR
    a0 = np.array([2., -3., np.nan, 0., -0., 5., -7.]).reshape(1, 7, 1)
    ts = np.array([0., 0., 0., np.nan, 0., np.nan, np.nan]).reshape(1, 7, 1) * yr
    both = ([(1. * yr, 4., .1 * yr)], [(1. * yr, 1., .1 * yr)])
    # at t = 1 yr: red chi = 5, blue chi = 2; the NaN launch times drop their cells
    assert U.ref_single_epoch(a0, ts, both, 1. * yr)[0, 0] == 2. * 4. + 3. * 25.
    # blue without bursts: its NaN-time cell counts with chi = 1; red's NaN-time cell is dropped
    assert U.ref_single_epoch(a0, ts, (both[0], []), 1. * yr)[0, 0] == 2. + 3. * 25. + 5.
    assert U.ref_single_epoch(a0, ts, ([], both[1]), 1. * yr)[0, 0] == 2. * 4. + 3. + 7.
    a0[0, 0, 0] = np.inf
    assert np.isinf(U.ref_single_epoch(a0, ts, both, 1. * yr)[0, 0])
    a0[0, 0, 0], ts[0, 0, 0] = -np.inf, np.nan       # inf x NaN: skipped with bursts, inf without
    assert U.ref_single_epoch(a0, ts, both, 1. * yr)[0, 0] == 3. * 25.
    assert np.isinf(U.ref_single_epoch(a0, ts, ([], both[1]), 1. * yr)[0, 0])


def test_plan_restatement_on_hand_worked_cases():
    """Launch times on [0, 4] yr in K = 8 bins of 0.5 yr; one red burst launched at 1 yr with
    amplitude 1: its support is +-r sigma with r = sqrt(2 ln 1e17) = 8.8482..."""
    yr = orc.YEAR
    r = np.sqrt(2. * np.log(1e17))
    sig = 0.1 * yr
    hist = [10] * 8 + [30] * 8
    plan = lambda t: U.srt_plan_host(hist, (0., 4. * yr), 8, ([(1. * yr, 1., sig)], []), t * yr)
    # t = 3 yr: ts in [2 - 0.885, 2 + 0.885] yr = bins 2 .. 5 -> [2, 6): 40 of 320 cells
    p = plan(3.0)
    assert (p["b0"], p["b1"], p["layout"]) == ([2, 0], [6, 0], "sorted") and p["share"] == 40 / 320
    # before any launch time meets the support: nothing is read
    assert plan(-1.0)["b1"] == [0, 0] and plan(-1.0)["share"] == 0.
    # beyond ts_hi + the support: clamped to [K, K), stored as no bins
    assert plan(6.0)["b0"] == [0, 0] and plan(6.0)["b1"] == [0, 0]
    # the support's upper edge (t - s_lo) just below / above the edge between bins 3 and 4
    t_edge = 2.0 + 1.0 - r * 0.1
    assert plan(t_edge - 1e-9)["b1"] == [4, 0] and plan(t_edge + 1e-9)["b1"] == [5, 0]
    # one jet holding everything the bursts reach: more than 90 % read -> grid order
    full = U.srt_plan_host([10] * 8 + [0] * 8, (0., 4. * yr), 8, ([(1. * yr, 1., yr)], []), 3. * yr)
    assert full["share"] == 1.0 and full["layout"] == "grid"
    # a smooth bin passes the interpolation check, a bin with a burst far narrower than it fails
    assert U.srt_bin_passes([(1. * yr, 1., 0.5 * yr)], (0., 4. * yr), 8, 20, 4, 3. * yr, 2e-13)
    assert not U.srt_bin_passes([(1. * yr, 5., 0.01 * yr)], (0., 4. * yr), 8, 20, 3, 3. * yr, 2e-13)
    # table rule: the interval follows the narrowest burst, the table spans every burst's support
    wide_ok = U.chi_table_host((128, 256, 256), (0., 5. * yr), ([(1. * yr, 4., .2 * yr)], []), 2. * yr)
    assert wide_ok is not None and 1 < wide_ok <= 460
    assert U.chi_table_host((128, 256, 256), (0., 5. * yr),
                            ([(1. * yr, 50., .002 * yr), (3. * yr, 1., .1 * yr)], []), 2. * yr) is None
    assert U.chi_table_host((64, 256, 256), (0., 5. * yr), ([(1. * yr, 4., .2 * yr)], []), 2. * yr) is None
