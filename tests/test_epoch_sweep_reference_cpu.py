"""Pins tests/sweep_ref.py -- the reference, the derived bounds and the host restatements the GPU
epoch-sweep tests are judged by -- without a GPU: the reference against the oracle on the golden
models, the recurrence bounds against a NumPy emulation of chi_batch_uniform, two planted mistakes
that the old 1e-11 let through, the tile plan, the moment tables, and the hard cap on every burst set
the GPU file uses."""
import copy

import numpy as np
import pytest

from oracle import rt_oracle as orc
from rajepy_amd import engine as E
from rajepy_amd.maths import physics as ph
from tests import gpu_util as U
from tests import sweep_ref as R
from tests.test_single_epoch_reference_cpu import _burst_lists

YEAR = orc.YEAR


@pytest.mark.parametrize("tag", ["cfg1_example", "tilted"])
def test_ref_sweep_equals_the_oracle_on_the_golden_models(tag):
    """Optical depths and emission measures at every golden epoch, 1e-13 as
    test_single_epoch_reference_cpu.py states for the single-epoch reference."""
    z, meta, p, g, jet = U.golden_dense(tag)
    q_T = p["power_laws"]["q_T"]
    mode = E.RJP_GFF_SCALAR if q_T == 0. else E.RJP_GFF_POWERLAW
    freqs = z["freqs"]
    gv = [ph.gff(nu, p["properties"]["T_0"]) for nu in freqs] if q_T == 0. else None
    ctau, _ = E.ff_channel_coeffs(freqs, jet.csize, p["target"]["dist"], mode, gv)
    bursts = _burst_lists(p)
    epochs = [float(yr) * YEAR for yr in z["years"]]
    sums = R.ref_sweep(U.golden_a0(g, q_T), g["ts"], bursts, epochs, threads=4)
    with np.errstate(all="ignore"):
        em0 = (g["nd"] * g["xi"]) ** 2. * (g["ff"] / g["areas"])
    ems = R.ref_sweep_em(np.where(g["rr"] < 0, -em0, em0), g["ts"], bursts, epochs, jet.csize,
                         threads=4)
    worst = 0.0
    for e, t in enumerate(epochs):
        jet.time = t
        with np.errstate(all="ignore"):
            want_tau, want_em = jet.optical_depth_ff(freqs), jet.emission_measure()
        for f in range(len(freqs)):
            worst = max(worst, U.against(ctau[f] * sums[e], np.nan_to_num(want_tau[f]), 1e-13, tag))
        worst = max(worst, U.against(ems[e], np.nan_to_num(want_em), 1e-13, tag + " em"))
    print("%s: ref_sweep vs the oracle, %d epochs, worst relative difference %.3g"
          % (tag, len(epochs), worst))


def test_device_polynomials_have_their_stated_size():
    """The two figures of rjp_device.h the bounds rest on: the degree-8 2^f of exp2_gauss is within
    1.1e-12 on |f| <= 1/2, the degree-10 one of exp2_poly within 4e-16 (coefficients copied from the
    header as data, Horner in long double so that only the approximation error is seen)."""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(U.GOLDEN.rstrip(os.sep)), os.pardir, "rajepy_amd",
                            "csrc", "rjp_device.h")).read()
    co = lambda fam, n: [float(re.search(r"#define RJP_EXP2_%s%d (\S+)" % (fam, k), hdr).group(1))
                         for k in range(n, 0, -1)]
    f = np.linspace(-0.5, 0.5, 20001).astype(np.longdouble)
    for fam, n, stated in (("D", 8, R.POLY8), ("C", 10, R.POLY10)):
        p = np.zeros_like(f)
        for c in co(fam, n):
            p = (p + np.longdouble(c)) * f
        err = float(np.max(np.abs((p + 1) / np.exp2(f) - 1)))
        print("degree %d: worst relative error %.3g (stated %.3g)" % (n, err, stated))
        assert err <= stated


def _grid(et, ratio_sigma, sigma, t_mid):
    """A uniform tile with its half-span at `ratio_sigma` sigma, and cells whose launch times put the
    anchor argument on a grid of -40 .. 40 sigma around a burst at t0 = 0.1 yr."""
    m = et // 2
    dt = ratio_sigma * sigma / max(m, et - 1 - m)
    ep = [t_mid + (k - m) * dt for k in range(et)]
    t0 = 0.1 * YEAR
    vm = np.linspace(-40.0, 40.0, 1601) * sigma
    ts = ep[m] - (vm + t0)
    return ep, t0, ts


@pytest.mark.parametrize("three", [False, True])
@pytest.mark.parametrize("et", [4, 8, 16, 32])
@pytest.mark.parametrize("ratio_sigma", [27.9, 9.0, 0.5])
def test_emulated_recurrence_lies_inside_the_derived_bound(et, ratio_sigma, three):
    """Every (j, distance) of a grid: the float64 recurrence in the order of chi_batch_uniform, with
    numpy.exp2 perturbed by the stated size of the device polynomials, against amp g as the reference
    forms it (numpy.exp of -(d^2) / (2 sigma^2) at the epoch itself), inside |amp| g delta(j, d)."""
    rng = np.random.default_rng(et * 1000 + int(ratio_sigma * 10) + three)
    worst = 0.0
    for sigma, t_mid, amp in ((R.sigma_of(0.02), 1.0 * YEAR, 4.0), (R.sigma_of(0.5), 4.0 * YEAR, -0.9)):
        ep, t0, ts = _grid(et, ratio_sigma, sigma, t_mid)
        assert R.uniform_tile_host(ep, ([(t0, amp, sigma)], []))
        dt, dev = R.tile_spacing(ep)
        m = et // 2
        tlm = ep[m] - ts
        got = R.emulate_recurrence(tlm, t0, amp, sigma, dt, et, three, rng)
        inv = R.inv2s2(sigma)
        for k in range(et):
            tl = ep[k] - ts
            d = tl - t0
            with np.errstate(all="ignore"):
                ref = amp * np.exp(-(d) ** 2 / (2. * sigma ** 2))
            dl = R.delta_recurrence(k - m, d, tlm - t0, tl, tlm, inv, dt, dev, three)
            frac = np.abs(got[k] - ref) / (np.abs(ref) * dl + 1e-300)
            assert frac.max() <= 1.0, (et, ratio_sigma, three, k, float(frac.max()))
            # (a cell whose anchor is below kDead adds nothing: delta = 1 and the ratio is 1 exactly;
            # the figure printed is the worst of the others)
            worst = max(worst, float(frac[dl < 1.0].max()))
            # ... and the bound is no loose one: below 3e-12 wherever the Gaussian matters
            live = np.abs(ref) >= 1e-17
            assert dl[live].max() <= 3e-12, (et, k, float(dl[live].max()))
    print("ET %d, half-span %.1f sigma, %s: worst error / bound %.3f"
          % (et, ratio_sigma, "three-op" if three else "two-op", worst))


def _sightline(et, ratio_sigma, sigma, amp, **planted):
    """One sightline of 1601 cells (weights 1, one jet) through tile_bound: -> (got, ref, bound)."""
    ep, t0, ts = _grid(et, ratio_sigma, sigma, 1.0 * YEAR)
    ts = ts[np.abs(ep[et // 2] - ts - t0) < 12 * sigma]              # the cells the burst reaches
    bursts = ([], [(t0, amp, sigma)])
    w0 = np.ones((1, ts.size, 1))
    ts3 = ts.reshape(1, -1, 1)
    ref = R.ref_sweep(w0, ts3, bursts, ep, threads=1)
    tiles = R.tile_plan_host(ep, bursts, nz=1)
    assert tiles == [(0, et, 1, 1)]
    B, path = R.tile_bound(w0, ts3, bursts, ep, tiles, ref, (ts.size + 4) * R.EPS)
    assert (path == R.TWO_OP).all()
    dt, _ = R.tile_spacing(ep)
    g = R.emulate_recurrence(ep[et // 2] - ts, t0, amp, sigma, dt, et, False, None, **planted)
    got = ((1.0 + g) ** 2).sum(axis=1).reshape(et, 1, 1)
    return got, ref, B


def test_two_planted_mistakes_pass_the_old_bound_and_fail_the_new():
    """What the tighter bound buys: (1) the step ratio off by 3e-12 per step, (2) hdt dropped from a
    burst's ratio (on a sweep whose spacing makes that a 2e-12 error per step).  Both stay inside the
    1e-11 the suite held the recurrence tiles to, both lie outside the derived bound; the unplanted
    recurrence lies inside it."""
    sigma = R.sigma_of(0.3)
    cases = [("clean", dict(), 8, 9.0), ("step ratio + 3e-12", dict(step_err=3e-12), 8, 9.0),
             ("clean", dict(), 8, 4 * 2e-6), ("hdt dropped", dict(drop_hdt=True), 8, 4 * 2e-6)]
    for what, planted, et, ratio_sigma in cases:
        got, ref, B = _sightline(et, ratio_sigma, sigma, 1.0, **planted)
        rel = float(np.max(np.abs(got - ref) / ref))
        frac = float(np.max(np.abs(got - ref) / B))
        print("%-20s half-span %.3g sigma: worst relative error %.3g, worst error / new bound %.3g"
              % (what, ratio_sigma, rel, frac))
        assert rel <= 1e-11, (what, rel)
        if planted:
            assert frac > 1.0, (what, frac)
        else:
            assert frac <= 1.0, (what, frac)


def test_tile_plan_of_the_existing_recurrence_test():
    """test_gpu_kernels.py::test_uniform_epoch_sweeps_use_the_recurrence_correctly plants a burst with
    hl = 0.02 yr (sigma = 0.017 yr, 28 sigma = 0.476 yr): of its four epoch lists only (12, 0.55) runs
    a recurrence -- one tile of 8 and one of 4.  The cases added to it run one at ET = 4 and 8."""
    p = copy.deepcopy(U.load_golden("cfg1_example")[2])
    p["ejection"] = U.example_bursts_params()
    p["ejection"]["hl"] = np.array([0.02, 0.15, 0.45, 0.5])
    bursts = _burst_lists(p)
    assert abs(R.sigma_of(0.02) / YEAR - 0.017) < 1e-4
    plan = lambda n, t1, **k: R.tile_plan_host(np.linspace(0., t1, n) * YEAR, bursts, nz=16, **k)
    for layout in ("tau", "cmp"):
        assert plan(8, 3.5, layout=layout) == [(0, 8, 0, 2)]
        assert plan(16, 5.0, layout=layout) == [(0, 8, 0, 2), (8, 8, 0, 2)]
        assert plan(4, 2.0, layout=layout) == [(0, 4, 0, 2)]
        assert plan(12, 0.55, layout=layout) == [(0, 8, 1, 2), (8, 4, 1, 2)]
        assert plan(4, 0.15, layout=layout) == [(0, 4, 1, 2)]
        assert plan(8, 0.35, layout=layout) == [(0, 8, 1, 2)]
    # f32 storage: 4-wide lanes take 4-epoch tiles; `uniform` is what uniform_tile says
    assert plan(12, 0.55, dtype=4) == [(0, 4, 1, 4), (4, 4, 1, 4), (8, 4, 1, 4)]
    assert plan(16, 5.0, dtype=4) == [(k, 4, 0, 4) for k in (0, 4, 8, 12)]


def test_tile_plan_rules():
    ex = U.example_burst_lists()
    Y = YEAR
    u = lambda n: R.uniform_epochs(n)
    # long tiles: f64 on the tau / compact layouts only; wide and f32 fall back
    assert R.tile_plan_host(u(45), ex) == [(0, 32, 1, 1), (32, 8, 1, 2), (40, 4, 1, 2), (44, 1, 0, 2)]
    assert R.tile_plan_host(u(23), ex) == [(0, 16, 1, 1), (16, 4, 1, 2), (20, 2, 0, 2), (22, 1, 0, 2)]
    assert [r[1] for r in R.tile_plan_host(u(45), ex, layout="wide")] == [8] * 5 + [4, 1]
    assert [r[1] for r in R.tile_plan_host(u(45), ex, dtype=4, nz=16)] == [4] * 11 + [1]
    assert [r[1] for r in R.tile_plan_host(u(45), ex, dtype=4, nz=15)] == [8] * 5 + [4, 1]
    # odd n_z or unaligned fields: one-wide lanes
    assert R.tile_plan_host(u(8), ex, nz=15) == [(0, 8, 1, 1)]
    assert R.tile_plan_host(u(8), ex, nz=16, aligned=False) == [(0, 8, 1, 1)]
    # irregular epochs: tiles of 8, direct
    irr = R.irregular_epochs()
    assert R.tile_plan_host(irr, ex) == [(0, 8, 0, 2), (8, 8, 0, 2), (16, 1, 0, 2)]
    # the 8-ulp uniformity rule, either side
    t = np.array(u(8))
    ulp = 2.220446049250313e-16 * t[-1]
    for k, want in ((6.0, 1), (12.0, 0)):
        bent = t.copy()
        bent[3] += k * ulp
        assert R.tile_plan_host(bent, ex)[0][2] == want, k
    # the 28 sigma rule, either side, at every tile size
    for et in (4, 8, 16, 32):
        ep, b, _ = R.narrow_case(et, 27.9)
        assert R.tile_plan_host(ep, b) == [(0, et, 1, 2 if et < 16 else 1)]
        ep, b, _ = R.narrow_case(et, 28.1)
        assert all(r[2] == 0 or r[1] < et for r in R.tile_plan_host(ep, b))
        assert all(r[1] <= 8 for r in R.tile_plan_host(ep, b, layout="wide"))
    # no bursts: one tile of one epoch, replicated
    assert R.tile_plan_host(u(9), ([], [])) == [(0, 1, 0, 2)]
    assert Y == 31536000.0


def test_wave_mixed():
    red = np.zeros((3, 16), dtype=bool)
    assert not R.wave_mixed(red, 2).any()
    red[:, :8] = True                                    # the generator's halves: 48 sightlines, one wave
    assert R.wave_mixed(red, 2).all() and R.wave_mixed(red, 1).all()
    rows = np.zeros((2, 64), dtype=bool)
    rows[0] = True                                       # a jet per x-row of 64 sightlines
    assert not R.wave_mixed(rows, 1).any() and R.wave_mixed(rows, 2).all()


TS_RANGE = (0.0, 5.0 * YEAR)


@pytest.mark.parametrize("scale,shape", [(1.0, (53, 12)), (2.5, (80, 8)), (0.8, (39, 16))])
def test_moment_tables_take_the_shapes_the_device_takes(scale, shape):
    """The example's bursts take (53, 12), half-lives x 2.5 (80, 8), x 0.8 (39, 16), as
    test_gpu_moments.py asserts on the device; every accepted table stays inside RJP_MOM_TOL on
    64 N + 1 dense points as well (the acceptance rule samples 2 N + 1)."""
    bursts = R.scaled_example(scale)
    for epochs in (R.uniform_epochs(32), R.irregular_epochs()):
        tab = R.mom_tables_host(bursts, epochs, TS_RANGE)
        assert tab is not None and (tab["K"], tab["N"]) == shape, tab and tab["tried"]
        assert tab["worst"] <= R.MOM_TOL
        _, dense = R.mom_table(bursts, epochs, TS_RANGE, tab["K"], tab["N"], dense=64)
        print("x%.1f %s: %d epochs, worst %.3g at the check points, %.3g on 64 N + 1 points"
              % (scale, shape, len(epochs), tab["worst"], dense))
        assert tab["worst"] <= dense <= R.MOM_TOL


def test_moment_tables_of_the_layout_and_degenerate_cases():
    ex = U.example_burst_lists()
    for K in (1, 20, 32):
        tab = R.mom_tables_host(ex, R.uniform_epochs(12), TS_RANGE, R.lt_shapes(K))
        if K == 1:
            assert tab is None                       # one bin cannot hold the example's bursts
        else:
            assert tab["K"] == K and tab["worst"] <= R.MOM_TOL
            _, dense = R.mom_table(ex, R.uniform_epochs(12), TS_RANGE, K, tab["N"], dense=64)
            assert dense <= R.MOM_TOL
    # a jet without bursts: F == 1, the zeroth coefficient alone
    W, worst = R.mom_table(U.example_burst_lists(only="R"), R.uniform_epochs(12), TS_RANGE, 53, 12)
    assert (W[1, :, 0, :] == 1.0).all() and (W[1, :, 1:, :] == 0.0).all() and worst <= R.MOM_TOL
    # the node-spacing guard: a burst narrower than h / N is not even tried
    thin = ([(1.0 * YEAR, 2.0, R.sigma_of(0.002))], [])
    assert R.mom_tables_host(thin, R.uniform_epochs(12), TS_RANGE) is None


def _synth(shape, seed, jets="halves"):
    g = U.synth_host(shape, seed, 1)
    a0 = np.abs(U.golden_a0(g, 0.))
    if jets == "halves":
        red = g["rr"] < 0
    elif jets == "rows":
        red = np.zeros(shape, dtype=bool)
        red[0::2] = True
    else:
        red = np.full(shape, jets == "red")
    return np.where(red, -a0, a0), g["ts"]


def test_hard_cap_on_every_burst_set_of_the_gpu_file():
    """No derived bound exceeds the project's stated figures: GAUSS_RTOL = 3e-12 relative for tiles
    on burst sets with chi >= 1 (every path: the halves' straddling waves run the three-operation
    recurrence, one jet per row the two-operation one), 1e-11 plus the rounding term for moments."""
    ny = 37
    for name, bursts in R.tile_burst_sets().items():
        if name == "dip":
            continue                                  # chi passes near 0: no relative figure
        for jets in ("halves", "red"):
            a0, ts = _synth((3, ny, 16), 77, jets)
            for epochs in (R.uniform_epochs(45), R.irregular_epochs()):
                ref = R.ref_sweep(a0, ts, bursts, epochs, threads=1)
                tiles = R.tile_plan_host(epochs, bursts, nz=16)
                B, path = R.tile_bound(a0, ts, bursts, epochs, tiles, ref, (ny + 4) * R.EPS)
                cap = float(np.max(B / ref))
                print("%-12s %-6s %2d epochs: worst bound / reference %.3g" % (name, jets, len(epochs), cap))
                assert cap <= U.GAUSS_RTOL, (name, jets, cap)
    for et in (4, 8, 16, 32):
        for rs in (27.9, 28.1):
            ep, bursts, _ = R.narrow_case(et, rs)
            for jets in ("halves", "blue"):
                a0, ts = _synth((3, ny, 16), 78, jets)
                ts = ts * 0.2                          # launch times the narrow burst reaches
                ref = R.ref_sweep(a0, ts, bursts, ep, threads=1)
                B, _ = R.tile_bound(a0, ts, bursts, ep, R.tile_plan_host(ep, bursts, nz=16), ref,
                                    (ny + 4) * R.EPS)
                cap = float(np.max(B / ref))
                print("narrow ET %2d at %.1f sigma %-6s: worst bound / reference %.3g" % (et, rs, jets, cap))
                assert cap <= U.GAUSS_RTOL, (et, rs, cap)
    for scale in (1.0, 2.5, 0.8):
        bursts = R.scaled_example(scale)
        a0, ts = _synth((5, 90, 23), 79)
        rng = (float(np.nanmin(ts)), float(np.nanmax(ts)))
        for epochs in (R.uniform_epochs(33), R.irregular_epochs()):
            tab = R.mom_tables_host(bursts, epochs, rng)
            ref = R.ref_sweep(a0, ts, bursts, epochs, threads=1)
            B, Rd = R.moment_bound(a0, ts, bursts, epochs, rng, tab["K"], tab["N"], tab["W"], ref)
            assert np.array_equal(B, R.MOM_TOL * ref + Rd)
            # (the rounding term stays a fraction of the threshold: (n_y + 2 N + 8) u = 1.4e-14 times
            # sum |W| / F of a few, and the coordinate term's 8 u (span + |t|) 9 / sigma_min < 1.5e-12)
            assert (Rd <= 2e-12 * ref).all()
            print("moments x%.1f (%d, %d) %2d epochs: rounding term <= %.3g of the reference, bound <= %.3g"
                  % (scale, tab["K"], tab["N"], len(epochs), float(np.max(Rd / ref)), float(np.max(B / ref))))
