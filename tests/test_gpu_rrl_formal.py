"""The RRL formal solution along the line of sight (rjp_rrl_formal, K6): every cell's line emission
minus its absorption of what lies behind it, observer at the iy = 0 end of axis 1.  The reference
is the float64 NumPy recurrence of tests/rrl_formal_ref.py (pinned on the CPU by
tests/test_rrl_formal_reference_cpu.py) on per-cell optical depths that do not come from the kernel
under test: the oracle's, or rjp_rrl_cells + rjp_ff_cells.

Tolerance: |got - ref| <= r |ref| + r max_p |ref[f]| with r = gpu_util.k3_rtol(nchan), the
project's Voigt bound (1e-8 on the wave-uniform paths, 1e-9 on the per-lane path).  The absolute
term is needed because a pixel is a difference of emission and absorption: a relative Voigt error
on either does not scale with their difference.  NaN patterns must match exactly.

That absolute term is normalised to the channel's brightest pixel, so a fainter pixel may be off by
max / |ref| times the bound: tests/test_gpu_rrl_formal_ld.py holds every pixel to a bound of its own
against a long-double reference."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U
from tests import rrl_formal_ref as R
from tests.test_gpu_formal_rt import _coeffs, _host, _params_files, _upload

pytestmark = pytest.mark.gpu

_CASES = {}              # random case -> its figures (test 3: computed once, shared)
NCHANS = [1, 16, 17, 64, 65, 256, 300]


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()


def _line(rrl):
    from rajepy_amd import _lib
    from rajepy_amd.maths import rrls
    return _lib.Line(**rrls.line_constants(rrl))


def _nu_rest(rrl):
    from rajepy_amd.maths import rrls
    return rrls.rrl_nu_0(*rrls.rrl_parser(rrl))


def _line_coeffs(jet, freqs, intensity=False):
    from rajepy_amd import engine as E
    csrc, hnu_k = E.rrl_channel_coeffs(freqs, jet.csize, jet.params["target"]["dist"])
    if intensity:
        csrc = csrc / (E.solid_angle(jet.csize, jet.params["target"]["dist"]) / 1e-26)
    return csrc, hnu_k


# ---- 1: isothermal equals the reference ---------------------------------------------------------
@pytest.mark.parametrize("dtype", [8, 4])
def test_isothermal_model_equals_the_reference_products(eng, dtype):
    """cfg1_example (q_T = q^d_T = 0), its 8 rrl_freqs: the formal line flux equals rjp_rrl_maps'
    isothermal product and the golden flux_rrl_contsub; with d_add = the formal continuum, the
    golden flux_rrl_total."""
    z, meta, p, g, jet = U.golden_dense("cfg1_example")
    rf = np.asarray(z["rrl_freqs"], dtype=np.float64)
    F, nx, nz = len(rf), jet.nx, jet.nz
    P = nx * nz
    r = U.k3_rtol(F) if dtype == 8 else 1e-5
    fields = _upload(eng, g, jet.csize, dtype)
    bursts = U.bursts_from_oracle(jet)
    t0 = float(z["years"][0]) * orc.YEAR
    line = _line(meta["rrl"])
    mode, ctau, cflux = _coeffs(jet, rf)
    csrc, hnu_k = _line_coeffs(jet, rf)
    got = _host(eng.rrl_formal(fields, bursts, t0, mode, line, rf, ctau, csrc, hnu_k), F, nx, nz)

    tau_rrl = eng.rrl_scan(fields, bursts, t0, line, rf)
    sumA, _, tavg = eng.ff_scan(fields, bursts, [t0], mode)
    tau_ff, _, _ = eng.ff_maps(sumA, tavg, ctau, cflux)
    iso, _ = eng.rrl_maps(tau_rrl, tau_ff.reshape(F, P), tavg, None, csrc, hnu_k, want_ftot=False)
    print("vs rrl_maps:", R.within(got, _host(iso, F, nx, nz), r), "of the bound")
    print("vs golden contsub:", R.within(got, z["flux_rrl_contsub"], r), "of the bound")
    assert R.within(got, _host(iso, F, nx, nz), r) <= 1.0
    assert R.within(got, z["flux_rrl_contsub"], r) <= 1.0

    cont = eng.ff_formal(fields, bursts, t0, mode, ctau, cflux)
    tot = _host(eng.rrl_formal(fields, bursts, t0, mode, line, rf, ctau, csrc, hnu_k, add=cont),
                F, nx, nz)
    print("vs golden total:", R.within(tot, z["flux_rrl_total"], r), "of the bound")
    assert R.within(tot, z["flux_rrl_total"], r) <= 1.0
    np.testing.assert_allclose(tot, got + _host(cont, F, nx, nz), rtol=1e-12, atol=0)


# ---- 2: gradients -----------------------------------------------------------------------------------
def test_temperature_gradients_match_numpy_and_differ_from_the_isothermal_product(eng):
    """tilted (q_T = -0.05, q^d_T = -0.1), its 6 rrl_freqs, H58a: against NumPy on the oracle's
    per-cell optical depths, and different from the golden isothermal flux_rrl_contsub by more than
    1e-3 on at least half of its non-zero finite pixels (74 % on the CPU)."""
    z, meta, p, g, jet = U.golden_dense("tilted")
    rf = np.asarray(z["rrl_freqs"], dtype=np.float64)
    F, nx, nz = len(rf), jet.nx, jet.nz
    fields = _upload(eng, g, jet.csize, 8)
    bursts = U.bursts_from_oracle(jet)
    jet.time = float(z["years"][0]) * orc.YEAR
    mode, ctau, _ = _coeffs(jet, rf)
    csrc, hnu_k = _line_coeffs(jet, rf)
    got = _host(eng.rrl_formal(fields, bursts, jet.time, mode, _line(meta["rrl"]), rf, ctau, csrc,
                               hnu_k), F, nx, nz)
    with np.errstate(all="ignore"):
        ref = R.np_rrl_formal(jet.optical_depth_ff(rf, collapse=False),
                              jet.optical_depth_rrl(meta["rrl"], rf, collapse=False),
                              jet.temperature, hnu_k, csrc)
    print("vs NumPy on the oracle's cells:", R.within(got, ref, U.k3_rtol(F)), "of the bound")
    assert R.within(got, ref, U.k3_rtol(F)) <= 1.0
    gold = z["flux_rrl_contsub"]
    pix = np.isfinite(gold) & (gold != 0.0)
    assert pix.sum() > 100
    rel = np.abs(got[pix] / gold[pix] - 1.0)
    print("share of line pixels off the isothermal product by > 1e-3:", np.mean(rel > 1e-3))
    assert np.mean(rel > 1e-3) >= 0.5, np.mean(rel > 1e-3)


# ---- 3: every lane layout -------------------------------------------------------------------------
def _random_case(seed):
    """K5's random models (tests/test_gpu_formal_rt.py::_random_case) with a temperature spread
    forced: > 8 bursts in EACH jet, NaN / zero cells in every field, sparse y-ranges, one empty
    sightline; n_y in 33...140 (the kernel's slabs of 16 and of 64 rows are crossed mid-sightline),
    n_z no multiple of 8."""
    rng = np.random.default_rng(seed)
    shape = [int(rng.integers(1, 5)), int(rng.integers(20, 140)), int(rng.integers(3, 40))]
    shape[1] = 33 + (shape[1] - 20) % 108
    if shape[2] % 8 == 0:
        shape[2] += 1
    shape = tuple(shape)
    nb = int(rng.integers(9, 14))
    ej = {"t_0": rng.uniform(-0.5, 5.5, nb), "hl": rng.uniform(0.12, 1.2, nb),
          "chi": np.where(rng.random(nb) < 0.25, rng.uniform(0.2, 0.9, nb), rng.uniform(1.2, 12., nb)),
          "which": np.array(["RB"] * nb)}
    rng.integers(0, 2)                          # (K5 draws its temp_mode here)
    g = U.synth_host(shape, 500 + seed, 1)
    for k, vals in (("nd", [np.nan, 0.0]), ("xi", [np.nan]), ("temp", [np.nan]),
                    ("ff", [np.nan, 0.0]), ("ts", [np.nan])):
        m = rng.random(shape) < 0.04
        g[k] = np.where(m, rng.choice(vals, size=shape), g[k])
    ny = shape[1]
    lo, hi = int(rng.integers(0, ny // 3)), int(rng.integers(2 * ny // 3, ny))
    for k in ("nd", "temp"):
        g[k][:, :lo, :] = np.nan
        g[k][:, hi:, :] = np.nan
    g["nd"][0, :, 0] = np.nan                   # an empty sightline
    g["temp"][0, :, 0] = np.nan
    p = copy.deepcopy(U.load_golden("cfg1_example")[2])
    p["ejection"] = ej
    p["power_laws"]["q_T"] = -0.5
    p["grid"].update(n_x=shape[0], n_y=shape[1], n_z=shape[2])
    jet = orc.OracleJet.from_fields(p, g["nd"], g["xi"], g["temp"], g["ff"], g["areas"],
                                    g["ts"], g["rr"], g["vy"])
    return rng, shape, g, jet


def _random_against_cells(eng, seed, freqs, key):
    """-> {worst error in units of the bound, bounds give the same bits, a negative pixel}."""
    if key in _CASES:
        return _CASES[key]
    rng, shape, g, jet = _random_case(seed)
    nx, ny, nz = shape
    assert 33 <= ny <= 140 and nz % 8 != 0
    F = len(freqs)
    mode, ctau, _ = _coeffs(jet, freqs)
    csrc, hnu_k = _line_coeffs(jet, freqs)
    bursts = U.bursts_from_oracle(jet)
    assert bursts.n[0] > 8 and bursts.n[1] > 8
    fields = _upload(eng, g, jet.csize, 8)
    line = _line("H66a")
    t = float(rng.uniform(0., 5.)) * orc.YEAR
    c = eng.ff_cells(fields, bursts, t, mode, ctau).cpu().numpy().reshape(F, nx, ny, nz)
    l = eng.rrl_cells(fields, bursts, t, line, freqs).cpu().numpy().reshape(F, nx, ny, nz)
    ref = R.np_rrl_formal(c, l, g["temp"], hnu_k, csrc)
    assert np.isnan(ref[:, 0, 0]).all() and np.isfinite(ref).any()
    got = _host(eng.rrl_formal(fields, bursts, t, mode, line, freqs, ctau, csrc, hnu_k), F, nx, nz)
    eng.compute_y_bounds(fields)
    assert fields.ylo is not None
    bounded = _host(eng.rrl_formal(fields, bursts, t, mode, line, freqs, ctau, csrc, hnu_k),
                    F, nx, nz)
    worst = R.within(got, ref, U.k3_rtol(F))
    print(key, shape, "worst error:", worst, "of the bound; tau_C <=", np.nanmax(np.nansum(c, axis=2)),
          "tau_L <=", np.nanmax(np.nansum(l, axis=2)), "negative pixels:", int(np.sum(ref < 0)))
    _CASES[key] = dict(worst=worst, same_bits=np.array_equal(got, bounded, equal_nan=True),
                       negative=bool(np.any(got < 0)) and bool(np.any(ref < 0)))
    return _CASES[key]


def _h66a_band(nchan):
    beta = np.linspace(-1e-3, 1e-3, nchan) if nchan > 1 else np.array([-2e-5])
    return _nu_rest("H66a") * (1.0 + beta)


@pytest.mark.parametrize("nchan", NCHANS)
def test_random_models_against_numpy_on_every_layout(eng, nchan):
    """Channels H66a +- 300 km/s on random models with a temperature spread, for every lane layout
    of the kernel: against NumPy on rjp_rrl_cells' and rjp_ff_cells' per-cell optical depths, and
    bit for bit the same with occupied y-ranges."""
    case = _random_against_cells(eng, 700 + nchan, _h66a_band(nchan), nchan)
    assert case["worst"] <= 1.0, case
    assert case["same_bits"]


@pytest.mark.parametrize("nchan", [12, 96, 200])
def test_random_model_with_a_band_from_0p7_to_1p3_of_the_rest_frequency(eng, nchan):
    """Channels spanning nu_rest (0.7 ... 1.3): the far-field paths, and h nu / kT not small over
    the band, so the lanes call exp / expm1 -- on the per-lane, the 64-lane and the 256-lane
    (rotated bands) layouts."""
    case = _random_against_cells(eng, 640 + nchan, _nu_rest("H66a") * np.linspace(0.7, 1.3, nchan),
                                 "wide%d" % nchan)
    assert case["worst"] <= 1.0, case
    assert case["same_bits"]


def test_some_random_model_shows_net_absorption(eng):
    """The isothermal product is never negative; with a temperature spread the formal solution is
    wherever colder gas absorbs the line of hotter gas behind it.  (The models of the layout test,
    computed once for both.)"""
    neg = {n: _random_against_cells(eng, 700 + n, _h66a_band(n), n)["negative"] for n in NCHANS}
    assert any(neg.values()), neg


# ---- 4: absorption sign ---------------------------------------------------------------------------
@pytest.mark.parametrize("nchan", [5, 21])
def test_cold_gas_in_front_of_hot_gas_absorbs(eng, nchan):
    """Two cells on every sightline, both with line and continuum opacity, the hot one optically
    thick in the continuum: cold in front of hot gives I_L < 0 at line centre, the mirror case
    I_L > 0; values against the closed form of the two-cell recurrence."""
    from rajepy_amd import engine as E
    from rajepy_amd.maths import physics as ph
    nx, ny, nz = 2, 41, 3
    shape = (nx, ny, nz)
    nan = np.full(shape, np.nan)
    nd, xi, temp = nan.copy(), nan.copy(), nan.copy()
    one, zero = np.ones(shape), np.zeros(shape)
    hot, cold = (2.0e4, 1.3e8), (5.0e3, 1.0e7)             # (T [K], n [cm^-3])
    cold_front = np.zeros((nx, nz), dtype=bool)
    for x in range(nx):
        for zz in range(nz):
            cold_front[x, zz] = (x + zz) % 2 == 0
            front, back = (cold, hot) if cold_front[x, zz] else (hot, cold)
            for iy, (tk, n) in ((3, front), (ny - 2, back)):
                nd[x, iy, zz], xi[x, iy, zz], temp[x, iy, zz] = n, 1.0, tk
    fields = eng.upload_fields(nd, xi, temp, one, one, None, zero > 0, zero, csize_au=0.5, dtype=8)
    nu0 = _nu_rest("H66a")
    freqs = nu0 * (1.0 + np.linspace(-2e-4, 2e-4, nchan))
    mid = nchan // 2
    gv = [ph.gff(nu, 1e4) for nu in freqs]
    mode = E.RJP_GFF_SCALAR
    ctau, _ = E.ff_channel_coeffs(freqs, 0.5, 120., mode, gv)
    csrc, hnu_k = E.rrl_channel_coeffs(freqs, 0.5, 120.)
    line = _line("H66a")
    c = eng.ff_cells(fields, None, 0.0, mode, ctau).cpu().numpy().reshape(nchan, nx, ny, nz)
    l = eng.rrl_cells(fields, None, 0.0, line, freqs).cpu().numpy().reshape(nchan, nx, ny, nz)
    got = _host(eng.rrl_formal(fields, None, 0.0, mode, line, freqs, ctau, csrc, hnu_k),
                nchan, nx, nz)
    c1, c2, l1, l2 = c[:, :, 3], c[:, :, ny - 2], l[:, :, 3], l[:, :, ny - 2]
    thick = np.where(cold_front[None], c2, c1)
    assert 3.0 < thick.min() and thick.max() < 20.0 and min(l1.min(), l2.min()) > 0.0
    B1 = 1.0 / np.expm1(hnu_k[:, None, None] / temp[None, :, 3])
    B2 = 1.0 / np.expm1(hnu_k[:, None, None] / temp[None, :, ny - 2])
    om = lambda v: -np.expm1(-v)
    # first cell: I = B1 e^-c1 om(l1), D = e^-c1 om(l1), Theta_C = e^-c1; then the second
    e1 = np.exp(-c1)
    D1 = e1 * om(l1)
    ref = csrc[:, None, None] * (B1 * D1 + B2 * (np.exp(-c2) * om(l2) * e1 - om(c2 + l2) * D1))
    assert R.within(got, ref, U.k3_rtol(nchan)) <= 1.0
    assert np.all(ref[mid][cold_front] < 0) and np.all(got[mid][cold_front] < 0)
    assert np.all(ref[mid][~cold_front] > 0) and np.all(got[mid][~cold_front] > 0)


# ---- 5: public surface ----------------------------------------------------------------------------
def test_jetmodel_pipeline_and_cli(tmp_path):
    """JetModel.flux_rrl / intensity_rrl(formal=True) on the (isothermal) example model equal the
    isothermal products; `main.py -rt --formal-rrl` on a table with one RRL run writes a Flux FITS
    equal to flux_rrl(contsub=False, formal=True) with the HISTORY line, the continuum runs' cubes
    stay isothermal; `--formal --formal-rrl` completes."""
    from rajepy_amd import fits, main as cli
    model, pline, out = _params_files(tmp_path, [0.])
    pl = cli.main(["-rt", "--formal-rrl", str(model), str(pline)])
    m = pl.model
    found = 0
    for run in pl.runs:
        assert run.completed
        data, cards = fits.read(run.fits_flux)
        if run.obs_type == "continuum":
            assert "Formal solution" not in str(cards)
            continue
        found += 1
        assert "Formal solution along the line of sight" in str(cards)
        assert "Formal solution" not in str(fits.read(run.fits_tau)[1])
        m.time = run.year * orc.YEAR
        rf = run.chan_freqs
        r = U.k3_rtol(len(rf))
        want = m.flux_rrl(run.line, rf, contsub=False, formal=True)
        np.testing.assert_array_equal(np.nan_to_num(data),
                                      np.nan_to_num(np.swapaxes(want, -1, -2)))
        np.testing.assert_allclose(run.results["flux"], np.nansum(want, axis=(1, 2)), rtol=1e-12)
        assert R.within(want, m.flux_rrl(run.line, rf, contsub=False), r) <= 1.0
        assert R.within(m.flux_rrl(run.line, rf, formal=True), m.flux_rrl(run.line, rf), r) <= 1.0
        assert R.within(m.intensity_rrl(run.line, rf, formal=True),
                        m.intensity_rrl(run.line, rf), r) <= 1.0
        one = m.flux_rrl(run.line, float(rf[1]), formal=True)
        assert one.shape == (m.nx, m.nz)
        with pytest.raises(ValueError):
            m.flux_rrl(run.line, rf, lte=False, formal=True)
    assert found == 1

    os.makedirs(tmp_path / "both")
    model, pline, out = _params_files(tmp_path / "both", [0.])
    pl = cli.main(["-rt", "--formal", "--formal-rrl", str(model), str(pline)])
    for run in pl.runs:
        assert run.completed
        assert "Formal solution along the line of sight" in str(fits.read(run.fits_flux)[1])


# ---- 6: ABI refusals ------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments_with_nothing_enqueued(eng):
    """rjp_rrl_formal: a NULL d_out, line, h_nu, h_ctau, h_csrc or h_hnu_k, n_chan <= 0, a bad
    Gaunt mode, fields lacking any of d_nd, d_xi, d_temp, d_pf, d_vy -> RJP_ERR_ARG, and the output
    buffer keeps its contents."""
    from rajepy_amd import _lib, engine as E
    import torch
    g = U.synth_host((2, 16, 4), 3, 1)
    fields = eng.upload_fields(g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"],
                               g["rr"] < 0, g["vy"], csize_au=0.5, dtype=8)
    out = torch.full((2, 8), 7.0, dtype=torch.float64, device=eng.device)
    nu0 = _nu_rest("H66a")
    tabs = dict(nu=_lib.dbl_array([nu0, nu0 * 1.0001]), ct=_lib.dbl_array([1e-20, 2e-20]),
                cs=_lib.dbl_array([1.0, 2.0]), hk=_lib.dbl_array([1.07, 1.08]))
    line = _line("H66a")
    lib = eng.lib

    def call(fs, mode=E.RJP_GFF_SCALAR, n=2, d_out=out.data_ptr(), ln=C.byref(line), **null):
        t = {k: (None if k in null else v) for k, v in tabs.items()}
        return lib.rjp_rrl_formal(eng.ctx, C.byref(fs), None, 0.0, mode, ln, t["nu"], t["ct"],
                                  t["cs"], t["hk"], n, None, d_out, eng._stream())

    fs = fields.struct()
    assert call(fs, d_out=None) == _lib.RJP_ERR_ARG
    assert call(fs, ln=None) == _lib.RJP_ERR_ARG
    for k in tabs:
        assert call(fs, **{k: True}) == _lib.RJP_ERR_ARG, k
    assert call(fs, n=0) == _lib.RJP_ERR_ARG
    assert call(fs, n=-3) == _lib.RJP_ERR_ARG
    assert call(fs, mode=7) == _lib.RJP_ERR_ARG
    for member in ("d_nd", "d_xi", "d_temp", "d_pf", "d_vy"):
        bad = fields.struct()
        assert getattr(bad, member)
        setattr(bad, member, None)
        assert call(bad) == _lib.RJP_ERR_ARG, member
    eng.synchronize()
    assert bool((out == 7.0).all())
    assert call(fs) == _lib.RJP_OK
    eng.synchronize()
    assert not bool((out == 7.0).any())
