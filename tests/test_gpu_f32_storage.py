"""`storage="f32"` held to a reference evaluated on the device's OWN rounded fields (tests/f32_ref.py,
pinned on the CPU by tests/test_f32_reference_cpu.py), through the C-ABI.  The fields are uploaded
with dtype=4, read back and widened; against sums over those every f32 kernel must meet the bounds
of its f64 twin -- it widens its loads and does f64 arithmetic -- except K1's burst factor, whose one
float exp2 per burst is bounded by f32_ref.k1_bound (delta = 2^-22).  The suite's other f32
assertions (1e-5 against the oracle on the unrounded fields) state a different claim and stay.

Every case prints its worst error as a fraction of its bound; the K1 cases with bursts also print
the observed delta, worst |got - ref| / sum_y w 2 |chi| S (DESIGN.md section 7 records it)."""
import contextlib

import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import f32_ref as R
from tests import gpu_util as U
from tests import rrl_formal_ref as RR
from tests.test_gpu_formal_rt import _coeffs, _host, _random_case, _upload, np_formal

pytestmark = pytest.mark.gpu

_ID = lambda s: "x".join(map(str, s))
_CASES = {}              # shape -> (host fields, DeviceFields, read-back dict): uploaded once


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    e.cache_moments = False
    yield e
    e.close()


def _case(eng, shape):
    if shape not in _CASES:
        g = R.case_fields(shape)
        f = eng.upload_fields(g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"],
                              g["rr"] < 0, vy=g["vy"], csize_au=0.5, dtype=4)
        eng.synchronize()
        assert f.em0 is not None and f.a0 is None
        _CASES[shape] = (g, f, R.device_fields(f))
    return _CASES[shape]


@contextlib.contextmanager
def _layout(f, name):
    """Scan `f` on the wide or the compact layout; occupied y-ranges attached inside are dropped."""
    em0 = f.em0
    if name == "wide":
        f.em0 = None
    try:
        yield f
    finally:
        f.em0 = em0
        f.ylo = f.yhi = None
        f.occupied_cells = 0


def _maps(t, shape):
    return t.cpu().numpy().reshape(-1, shape[0], shape[2])


def _same_bits(a, b):
    """Equal bit for bit; NaNs equal whatever their payload."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(a)
    return (a.dtype == b.dtype and np.array_equal(nan, np.isnan(b)) and
            np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


# ---- a: stored values -----------------------------------------------------------------------------
def test_a_pack_field_rounds_like_numpy(eng):
    """rjp_pack_field to float == NumPy's astype(float32) on normal-range values, +-0, NaN, +-inf and
    overflow to inf; with a denominator it is the rounding of the f64 quotient; with the red flags
    the sign bit is the flag, also on NaN and zero cells."""
    import torch
    rng = np.random.default_rng(5)
    vals = np.concatenate([
        10.0 ** rng.uniform(-37, 38, 4000) * rng.choice([-1.0, 1.0], 4000),
        rng.uniform(0.0, 5.0, 1000) * orc.YEAR,
        [0.0, -0.0, np.nan, np.inf, -np.inf, 1e39, -1e39, 3.5e38, -3.5e38, 3.4028234e38,
         3.4028235677973366e38, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 3 * 2.0 ** -24,
         1.1754944e-38, 1e300, -1e300]])
    n = vals.size
    den = np.where(rng.random(n) < 0.5, 1.0, rng.choice([2.0, 3.0, 7.0, 0.3], n))
    den[-17:] = 1.0                   # (no quotient below the normal range)
    red = rng.random(n) < 0.5
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(eng.device)
    src, d_den, d_red = dev(vals, np.float64), dev(den, np.float64), dev(red, np.uint8)

    def pack(den_t, red_t):
        dst = torch.empty(n, dtype=torch.float32, device=eng.device)
        eng._check(eng.lib.rjp_pack_field(eng.ctx, src.data_ptr(),
                                          den_t.data_ptr() if den_t is not None else None,
                                          red_t.data_ptr() if red_t is not None else None,
                                          dst.data_ptr(), n, 4, eng._stream()), eng.ctx, "pack")
        eng.synchronize()
        return dst.cpu().numpy()

    with np.errstate(all="ignore"):
        assert _same_bits(pack(None, None), vals.astype(np.float32))
        assert _same_bits(pack(d_den, None), (vals / den).astype(np.float32))
        got = pack(None, d_red)
        assert np.array_equal(np.signbit(got), red)
        assert _same_bits(np.abs(got), np.abs(vals).astype(np.float32))


@pytest.mark.parametrize("shape", R.SHAPES, ids=_ID)
def test_a_uploaded_fields_equal_the_host_restatement(eng, shape):
    """upload_fields(dtype=4): every stored field, pf (the rounding of the f64 quotient), the red
    flag in nd's sign bit (NaN and zero cells included) and em0 equal f32_ref.host_fields bit for
    bit -- so the CPU file's inputs are the device's."""
    g, f, dev = _case(eng, shape)
    h = R.host_fields(g, 0.5)
    for k in ("nd", "xi", "temp", "pf", "ts", "vy", "em0"):
        got = getattr(f, k).cpu().numpy().reshape(shape)
        assert got.dtype == np.float32
        assert _same_bits(got, getattr(h, k)), k
    assert np.array_equal(dev["red"], g["rr"] < 0)
    assert np.array_equal(dev["em0_red"], g["rr"] < 0)
    assert np.isnan(dev["nd"][dev["red"]]).any() or shape[1] < 16
    assert np.array_equal(dev["pf"], (g["ff"] / g["areas"]).astype(np.float32).astype(np.float64),
                          equal_nan=True)


def test_a_em0_range_guard_either_side_of_its_thresholds(eng):
    """(n x)^2 pf = 2^126 and 2^-124 keep the compact layout, 2^128 and 2^-127 leave em0 None."""
    for g, keeps in R.guard_cases():
        f = eng.upload_fields(g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"],
                              g["rr"] < 0, csize_au=1.0, dtype=4)
        assert (f.em0 is not None) == keeps, float(g["nd"].flat[0])
        if keeps:
            want = (g["nd"] * g["nd"] * g["ff"]).astype(np.float32)
            assert _same_bits(f.em0.cpu().numpy().reshape(want.shape), want)


# ---- b: K1 without bursts ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", R.SHAPES, ids=_ID)
def test_b_k1_without_bursts(eng, shape, mode):
    """tau sums, EM and T_avg on the wide and the compact layout, with and without EM maps, with and
    without occupied y-ranges (bit-identical), and rjp_tavg: identical zero / NaN patterns and the
    f64 bounds of f32_ref against sums over the stored fields."""
    g, f, dev = _case(eng, shape)
    ny = shape[1]
    tavg_ref = R.tavg_of(dev)
    for layout in ("wide", "compact"):
        ref, em_ref = R.tau_sums_of(dev, mode, layout), R.em_of(dev, layout)
        outs = {}
        with _layout(f, layout):
            for bounds in (False, True):
                if bounds:
                    eng.compute_y_bounds(f)
                    assert f.ylo is not None
                for want_em in (True, False):
                    sumA, em, tavg = eng.ff_scan(f, None, [0.0], mode, want_em=want_em)
                    eng.synchronize()
                    assert eng.last_scan_path()[0] == "tiles"
                    outs[bounds, want_em] = (_maps(sumA, shape)[0], _maps(tavg, shape)[0],
                                             _maps(em, shape)[0] if want_em else None)
                outs[bounds, "tavg"] = _maps(eng.tavg(f), shape)[0]
        fr = [U.against(outs[False, True][0], ref, R.tau_rtol(ny), "tau") / R.tau_rtol(ny),
              U.against(outs[False, True][2], em_ref, R.em_rtol(ny), "em") / R.em_rtol(ny),
              U.against(outs[False, True][1], tavg_ref, R.tavg_rtol(ny), "tavg") / R.tavg_rtol(ny)]
        print("%s mode %d %s: tau %.3f, EM %.3f, T_avg %.3f of their bounds"
              % (shape, mode, layout, fr[0], fr[1], fr[2]))
        for key, (a, t, e) in ((k, v) for k, v in outs.items() if k[1] != "tavg"):
            assert np.array_equal(a, outs[False, True][0]), key
            assert np.array_equal(t, outs[False, True][1], equal_nan=True), key
            assert e is None or np.array_equal(e, outs[False, True][2]), key
        U.against(outs[False, "tavg"], tavg_ref, R.tavg_rtol(ny), "rjp_tavg")
        assert np.array_equal(outs[True, "tavg"], outs[False, "tavg"], equal_nan=True)


# ---- c: K1 with bursts ------------------------------------------------------------------------------
def _check_k1(got, refs, ny, what, em=False):
    """Every epoch map of `got` [E, nx, nz] against its (bound, ref, unit); -> (worst error / bound,
    worst observed delta)."""
    frac = ratio = 0.0
    for e in range(got.shape[0]):
        bound, ref, unit = refs[e]
        frac = max(frac, R.within_abs(got[e], ref, bound, what + (e,)))
        ratio = max(ratio, R.k1_ratio(got[e], ref, unit, ny, em=em))
    return frac, ratio


@pytest.mark.parametrize("name", list(R.burst_sets()))
@pytest.mark.parametrize("shape", R.SHAPES, ids=_ID)
def test_c_k1_with_bursts(eng, shape, name):
    """Both Gaunt modes on the wide and the compact layout; prefixes of 1, 2, 3, 4, 5, 8, 9 and 13
    epochs of a uniform and of an irregular list (every tile of both lane widths and their tails;
    f32 evaluates both directly); the 5-epoch scans with EM maps.  Every epoch map against
    f32_ref.k1_bound: absolute, no pixel left out."""
    from rajepy_amd.engine import make_bursts
    g, f, dev = _case(eng, shape)
    ny = shape[1]
    lists = R.burst_sets()[name]
    bursts = make_bursts(*lists)
    epochs = R.epoch_lists()
    worst_frac = worst_delta = 0.0
    for layout in ("wide", "compact"):
        em_refs = {k: [R.k1_bound(dev, 0, layout, lists, t, em=True) for t in ep[:5]]
                   for k, ep in epochs.items()}
        for mode in (0, 1):
            refs = {k: [R.k1_bound(dev, mode, layout, lists, t) for t in ep]
                    for k, ep in epochs.items()}
            with _layout(f, layout):
                for kind, ep in epochs.items():
                    for n in R.EPOCH_COUNTS:
                        want_em = n == 5
                        sumA, em, _ = eng.ff_scan(f, bursts, ep[:n], mode, want_em=want_em,
                                                  want_tavg=False)
                        eng.synchronize()
                        assert eng.last_scan_path()[0] == "tiles"
                        what = (shape, name, layout, mode, kind, n)
                        fr, dl = _check_k1(_maps(sumA, shape), refs[kind], ny, what)
                        worst_frac, worst_delta = max(worst_frac, fr), max(worst_delta, dl)
                        if want_em:
                            fr, dl = _check_k1(_maps(em, shape), em_refs[kind], ny, what + ("em",),
                                               em=True)
                            worst_frac, worst_delta = max(worst_frac, fr), max(worst_delta, dl)
    print("%s %s: worst error %.3f of the bound; observed delta %.3g (bar 2^-22 = %.3g)"
          % (shape, name, worst_frac, worst_delta, R.DELTA))


# ---- d: misaligned bases ----------------------------------------------------------------------------
def _shifted(f):
    """The fields of `f` as views one float into slightly larger allocations: 4-byte but not 16-byte
    aligned, wholly inside their allocation.  ff_scan_plan and tavg_launch take their lane width
    from ff_scan_vec, which tests every pointer: only rjp_ff_scan and rjp_tavg are given these."""
    import torch
    from rajepy_amd.engine import DeviceFields
    keep = []

    def shift(t):
        buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
        v = buf[1:1 + t.numel()]
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        keep.append(buf)
        return v

    m = DeviceFields(f.shape, f.dtype, f.csize_au, shift(f.nd), shift(f.xi), shift(f.temp),
                     shift(f.pf), shift(f.ts))
    m.em0 = shift(f.em0)
    m._keep = keep
    return m


@pytest.mark.parametrize("mode", [0, 1])
def test_d_misaligned_bases_take_the_narrow_lanes(eng, mode):
    """The n_z % 4 == 0 shape with every field 4-byte but not 16-byte aligned: rjp_ff_scan (no
    bursts; the example's bursts over 5 irregular epochs) and rjp_tavg meet the bounds of the
    aligned run."""
    from rajepy_amd.engine import make_bursts
    shape = R.SHAPES[0]
    assert shape[2] % 4 == 0
    g, f, dev = _case(eng, shape)
    ny = shape[1]
    m = _shifted(f)
    lists = R.burst_sets()["example"]
    ep = R.epoch_lists()["irregular"][:5]
    tavg_ref = R.tavg_of(dev)
    for layout in ("wide", "compact"):
        with _layout(m, layout):
            sumA, em, tavg = eng.ff_scan(m, None, [0.0], mode, want_em=True)
            only = eng.tavg(m)
            s5, e5, _ = eng.ff_scan(m, make_bursts(*lists), ep, mode, want_em=True, want_tavg=False)
            eng.synchronize()
        a = U.against(_maps(sumA, shape)[0], R.tau_sums_of(dev, mode, layout), R.tau_rtol(ny), "tau")
        b = U.against(_maps(em, shape)[0], R.em_of(dev, layout), R.em_rtol(ny), "em")
        c = U.against(_maps(tavg, shape)[0], tavg_ref, R.tavg_rtol(ny), "tavg")
        U.against(_maps(only, shape)[0], tavg_ref, R.tavg_rtol(ny), "rjp_tavg")
        fr, dl = _check_k1(_maps(s5, shape), [R.k1_bound(dev, mode, layout, lists, t) for t in ep],
                           ny, (layout, mode))
        fe, _ = _check_k1(_maps(e5, shape), [R.k1_bound(dev, mode, layout, lists, t, em=True)
                                             for t in ep], ny, (layout, mode, "em"), em=True)
        print("misaligned %s mode %d: tau %.3f, EM %.3f, T_avg %.3f, bursts %.3f / %.3f of their "
              "bounds; observed delta %.3g" % (layout, mode, a / R.tau_rtol(ny), b / R.em_rtol(ny),
                                               c / R.tavg_rtol(ny), fr, fe, dl))


# ---- e: rjp_ff_cells --------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bursts", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[1]], ids=_ID)
def test_e_ff_cells(eng, shape, mode, with_bursts):
    """Per-cell optical depths of the f32 fields against f32_ref.cells_of at GAUSS_RTOL + 1.5e-13 +
    8 2^-53 per cell, NaN and zero patterns identical."""
    from rajepy_amd import engine as E
    g, f, dev = _case(eng, shape)
    lists = R.burst_sets()["example"] if with_bursts else ([], [])
    bursts = E.make_bursts(*lists) if with_bursts else None
    ctau, _ = E.ff_channel_coeffs([1e9, 4.3e10], 0.5, 120., E.RJP_GFF_POWERLAW)
    t = 1.1 * orc.YEAR
    got = eng.ff_cells(f, bursts, t, mode, ctau).cpu().numpy().reshape((2,) + shape)
    ref = R.cells_of(dev, mode, "wide", lists, t, ctau)
    assert np.isnan(ref).any() and (ref == 0).any()
    rel = U.against(got, ref, R.CELLS_RTOL, "cells")
    print("%s mode %d bursts %s: %.3f of the bound" % (shape, mode, with_bursts, rel / R.CELLS_RTOL))


# ---- f: K5 ------------------------------------------------------------------------------------------
def _k5_model(eng, which):
    key = ("k5", which)
    if key not in _CASES:
        if which == "tilted":
            z, meta, p, g, jet = U.golden_dense("tilted")
            t = float(z["years"][1]) * orc.YEAR
        else:
            rng, shape, g, jet = _random_case(4242)
            t = float(rng.uniform(0., 5.)) * orc.YEAR
        f = _upload(eng, g, jet.csize, 4)
        eng.synchronize()
        _CASES[key] = (jet, f, R.device_fields(f), t)
    return _CASES[key]


@pytest.mark.parametrize("nchan", [1, 17, 65])
@pytest.mark.parametrize("which", ["tilted", "random"])
def test_f_formal_solution(eng, which, nchan):
    """rjp_ff_formal in f32 against NumPy's formal solution on f32_ref.cells_of (not on the device's
    cells) at 1e-11: `tilted`, and a random model with > 8 bursts per jet; the compact and the wide
    layout each against its own reference, each with and without occupied y-ranges, bit-identical."""
    from rajepy_amd.engine import make_bursts
    jet, f, dev, t = _k5_model(eng, which)
    nx, ny, nz = dev["shape"]
    lists = R.burst_lists_of(jet)
    if which == "random":
        assert len(lists[0]) > 8 and len(lists[1]) > 8 and f.em0 is not None
    freqs = np.geomspace(1e9, 5e10, nchan) if nchan > 1 else np.array([5e9])
    mode, ctau, cflux = _coeffs(jet, freqs)
    bursts = make_bursts(*lists)
    for layout in ["wide"] + (["compact"] if f.em0 is not None else []):
        with np.errstate(all="ignore"):
            ref = np_formal(R.cells_of(dev, mode, layout, lists, t, ctau), dev["temp"], cflux)
        with _layout(f, layout):
            got = _host(eng.ff_formal(f, bursts, t, mode, ctau, cflux), nchan, nx, nz)
            eng.compute_y_bounds(f)
            assert f.ylo is not None
            bounded = _host(eng.ff_formal(f, bursts, t, mode, ctau, cflux), nchan, nx, nz)
        assert np.isfinite(ref).any()
        rel = U.against(got, ref, 1e-11, (which, layout, nchan))
        print("%s %s %d channels: %.3f of 1e-11" % (which, layout, nchan, rel / 1e-11))
        assert np.array_equal(got, bounded, equal_nan=True), (which, layout)


# ---- g: K6 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchan", [6, 65])
def test_g_rrl_formal_solution(eng, nchan):
    """rjp_rrl_formal in f32 on `tilted` against the NumPy recurrence on rjp_rrl_cells' and
    rjp_ff_cells' per-cell depths of the same f32 fields (and the stored temperatures), within
    gpu_util.k3_rtol(F): the f64 bar."""
    from rajepy_amd import _lib, engine as E
    from rajepy_amd.maths import rrls
    from rajepy_amd.engine import make_bursts
    jet, f, dev, t = _k5_model(eng, "tilted")
    z, meta, _ = U.load_golden("tilted")
    nx, ny, nz = dev["shape"]
    if nchan == 6:
        rf = np.asarray(z["rrl_freqs"], dtype=np.float64)
    else:
        rf = rrls.rrl_nu_0(*rrls.rrl_parser(meta["rrl"])) * (1.0 + np.linspace(-1e-3, 1e-3, nchan))
    assert len(rf) == nchan
    line = _lib.Line(**rrls.line_constants(meta["rrl"]))
    mode, ctau, _ = _coeffs(jet, rf)
    csrc, hnu_k = E.rrl_channel_coeffs(rf, jet.csize, jet.params["target"]["dist"])
    bursts = make_bursts(*R.burst_lists_of(jet))
    c = eng.ff_cells(f, bursts, t, mode, ctau).cpu().numpy().reshape(nchan, nx, ny, nz)
    l = eng.rrl_cells(f, bursts, t, line, rf).cpu().numpy().reshape(nchan, nx, ny, nz)
    ref = RR.np_rrl_formal(c, l, dev["temp"], hnu_k, csrc)
    got = _host(eng.rrl_formal(f, bursts, t, mode, line, rf, ctau, csrc, hnu_k), nchan, nx, nz)
    assert np.isfinite(ref).any()
    worst = RR.within(got, ref, U.k3_rtol(nchan))
    print("K6 f32, %d channels: %.3f of the bound" % (nchan, worst))
    assert worst <= 1.0


# ---- h: JetModel ------------------------------------------------------------------------------------
def test_h_jetmodel_f32_against_the_oracle_on_its_own_fields(eng, tmp_path):
    """JetModel(storage="f32") on the example parameters: optical_depth_ff, emission_measure, flux_ff
    and a 13-epoch flux_vs_time against the oracle built from the model's own device fields -- from
    the field its scans read: the model is on the compact layout, whose em0 carries a float rounding
    of its own (the same for every cell of this model's uniform jets: 2.5e-8 ... 5e-8 on tau against
    the oracle on nd, xi, pf, measured).
    Bounds: k1_bound for the sums, plus the oracle's own f64 error ((n_y + 8) 2^-53: ~8 roundings per
    cell and a plain n_y-term sum); on the flux the propagated tau bound (d(1 - e^-tau) = e^-tau dtau),
    T_avg's bound, K2's 1e-13 and the cancellation in the oracle's own 1 - exp(-tau) (2^-53 absolute);
    on the light curve the pixel bounds summed plus a P-term f64 sum."""
    from rajepy_amd import classes, logger
    from tests.test_host_logic import example_params
    jm = classes.JetModel(example_params(), log=logger.Log(str(tmp_path / "a.log"), verbose=False),
                          engine=eng, storage="f32")
    devf = jm.device_fields
    assert devf.dtype == 4 and devf.a0 is None
    dev = R.device_fields(devf)
    layout = "compact" if devf.em0 is not None else "wide"
    nx, ny, nz = dev["shape"]
    jet = R.oracle_of(jm.params, dev, layout)
    lists = R.burst_lists_of(jet)
    freqs, (ctau, cflux) = jm._channel_coeffs([5e9, 2.2e10])
    mode = jm.gff_mode
    own = (ny + 8) * R.EPS

    def flux_bound(t, fq, ct):
        """(oracle flux maps [F, nx, nz], their absolute bounds) at model time t."""
        jet.time = t
        with np.errstate(all="ignore"):
            tau, flux = jet.optical_depth_ff(fq), jet.flux_ff(fq)
            bsum, _, _ = R.k1_bound(dev, mode, layout, lists, t)
            btau = np.asarray(ct)[:, None, None] * bsum[None] + own * tau
            rel = R.tavg_rtol(ny) + 1e-13 + own + btau / np.expm1(tau) - R.EPS / np.expm1(-tau)
            return tau, btau, flux, np.abs(flux) * rel

    jm.time = 1.0 * orc.YEAR
    tau, btau, flux, bflux = flux_bound(jm.time, freqs, ctau)
    fr_tau = R.within_abs(jm.optical_depth_ff(freqs), tau, btau, "tau")
    assert eng.last_scan_path()[0] == "tiles"
    bem, _, _ = R.k1_bound(dev, mode, layout, lists, jm.time, em=True)
    with np.errstate(all="ignore"):
        em = jet.emission_measure()
    fr_em = R.within_abs(jm.emission_measure(), em, bem + own * em, "em")
    fr_flux = R.within_abs(jm.flux_ff(freqs), flux, bflux, "flux")
    times = R.epoch_lists()["uniform"]
    lc = jm.flux_vs_time(times, [5e9])
    assert eng.last_scan_path()[0] == "tiles" and lc.shape == (13, 1)
    fr_lc = 0.0
    for e, t in enumerate(times):
        _, _, fl, bf = flux_bound(t, freqs[:1], ctau[:1])
        want = float(np.nansum(fl))
        bound = float(np.nansum(bf)) + nx * nz * R.EPS * want
        fr_lc = max(fr_lc, abs(lc[e, 0] - want) / bound)
        assert abs(lc[e, 0] - want) <= bound, (e, lc[e, 0], want, bound)
    print("JetModel f32 (%s layout): tau %.3f, EM %.3f, flux %.3f, light curve %.3f of their bounds"
          % (layout, fr_tau, fr_em, fr_flux, fr_lc))
