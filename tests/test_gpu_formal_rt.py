"""The formal solution along the line of sight (rjp_ff_formal, K5): every cell's free-free emission
T (1 - e^-dtau) attenuated by the cells in front of it, observer at the iy = 0 end of axis 1.
Checked against the reference's isothermal maps where T is constant along the sightline (the sum
telescopes to T_avg (1 - e^-tau) there), against a float64 NumPy restatement built from the
oracle's / the library's per-cell optical depths elsewhere, and through JetModel, Pipeline and the
command line."""
import copy
import ctypes as C
import os
import warnings

import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U

pytestmark = pytest.mark.gpu

K_B, C_LIGHT = 1.380649e-23, 299792458.0


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()


def np_formal(tau_cells, temp, csrc):
    """float64 NumPy formal solution: tau_cells [F, nx, ny, nz] per-cell optical depths (NaN =
    the cell is dropped, as nansum drops it), temp [nx, ny, nz]; observer at iy = 0.  NaN where
    no cell of the sightline has T > 0 (where the reference's T_avg is NaN)."""
    dt = np.where(np.isnan(tau_cells), 0.0, tau_cells)
    om = -np.expm1(-dt)
    csum = np.cumsum(dt, axis=2)
    front = np.concatenate([np.zeros_like(csum[:, :, :1]), csum[:, :, :-1]], axis=2)
    tl = np.where(dt != 0.0, temp[None], 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        out = np.asarray(csrc)[:, None, None] * np.sum(tl * om * np.exp(-front), axis=2)
    hot = np.any(temp > 0.0, axis=1)
    out[:, ~hot] = np.nan
    return out


def _coeffs(jet, freqs):
    from rajepy_amd import engine as E
    from rajepy_amd.maths import physics as ph
    p = jet.params
    mode = E.RJP_GFF_SCALAR if p["power_laws"]["q_T"] == 0. else E.RJP_GFF_POWERLAW
    gv = [ph.gff(nu, p["properties"]["T_0"]) for nu in freqs] if mode == E.RJP_GFF_SCALAR else None
    ctau, cflux = E.ff_channel_coeffs(freqs, jet.csize, p["target"]["dist"], mode, gv)
    return mode, ctau, cflux


def _upload(eng, g, csize, dtype):
    return eng.upload_fields(g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"],
                             g["rr"] < 0, g["vy"], csize_au=csize, dtype=dtype)


def _host(t, F, nx, nz):
    return t.cpu().numpy().reshape(F, nx, nz)


@pytest.mark.parametrize("store", ["f64-tau", "f64", "f64-wide", "f32"])
def test_isothermal_model_equals_the_reference_maps(eng, store):
    """cfg1_example (q_T = q^d_T = 0) at every golden epoch and frequency: the formal flux and
    intensity equal the shipped isothermal maps (K1 + K2) to 1e-12 and the reference's golden
    flux_ff to 1e-10, with identical NaN and zero patterns."""
    z, meta, p, g, jet = U.golden_dense("cfg1_example")
    dtype = 4 if store == "f32" else 8
    freqs = np.asarray(z["freqs"], dtype=np.float64)
    mode, ctau, cflux = _coeffs(jet, freqs)
    fields = _upload(eng, g, jet.csize, dtype)
    if store == "f64-tau":
        eng.tau_layout(fields, mode)
        assert fields.a0 is not None
    elif store == "f64-wide":
        fields.em0 = None
    bursts = U.bursts_from_oracle(jet)
    F, nx, nz = len(freqs), jet.nx, jet.nz
    cint = 2. * freqs ** 2. * K_B / C_LIGHT ** 2.
    tavg = eng.tavg(fields)
    for e, yr in enumerate(z["years"]):
        t = float(yr) * orc.YEAR
        flux = _host(eng.ff_formal(fields, bursts, t, mode, ctau, cflux), F, nx, nz)
        inten = _host(eng.ff_formal(fields, bursts, t, mode, ctau, cint), F, nx, nz)
        gold = z["flux_ff"][e]
        assert np.array_equal(np.isnan(flux), np.isnan(gold))
        assert np.array_equal(flux == 0.0, gold == 0.0)
        if dtype == 4:
            np.testing.assert_allclose(flux, gold, rtol=1e-5)
            continue
        sumA, _, _ = eng.ff_scan(fields, bursts, [t], mode, want_em=False, want_tavg=False)
        _, s_flux, _ = eng.ff_maps(sumA, tavg, ctau, cflux, want_tau=False, want_ftot=False)
        _, s_int, _ = eng.ff_maps(sumA, tavg, ctau, cint, want_tau=False, want_ftot=False)
        s_flux, s_int = _host(s_flux, F, nx, nz), _host(s_int, F, nx, nz)
        np.testing.assert_allclose(flux, s_flux, rtol=1e-12, atol=0)
        np.testing.assert_allclose(inten, s_int, rtol=1e-12, atol=0)
        np.testing.assert_allclose(flux, gold, rtol=1e-10, atol=0)


def test_temperature_gradients_match_numpy_and_differ_from_the_isothermal_maps(eng):
    """tilted (q_T = -0.05, q^d_T = -0.1, inc = 60 deg, bursts in both jets) at every golden epoch
    and frequency: the formal solution against NumPy on the oracle's per-cell tau and T to 1e-11,
    and different from the isothermal flux_ff by > 1e-3 on at least half of the jet pixels."""
    z, meta, p, g, jet = U.golden_dense("tilted")
    freqs = np.asarray(z["freqs"], dtype=np.float64)
    mode, ctau, cflux = _coeffs(jet, freqs)
    fields = _upload(eng, g, jet.csize, 8)
    eng.tau_layout(fields, mode)
    bursts = U.bursts_from_oracle(jet)
    F, nx, nz = len(freqs), jet.nx, jet.nz
    for e, yr in enumerate(z["years"]):
        jet.time = float(yr) * orc.YEAR
        got = _host(eng.ff_formal(fields, bursts, jet.time, mode, ctau, cflux), F, nx, nz)
        with np.errstate(all="ignore"):
            ref = np_formal(jet.optical_depth_ff(freqs, collapse=False), jet.temperature, cflux)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.array_equal(got == 0.0, ref == 0.0)
        np.testing.assert_allclose(got, ref, rtol=1e-11, atol=0)
        iso = z["flux_ff"][e]
        jetpix = np.isfinite(iso) & (iso > 0)
        assert jetpix.sum() > 100
        rel = np.abs(got[jetpix] / iso[jetpix] - 1.0)
        assert np.mean(rel > 1e-3) >= 0.5, np.mean(rel > 1e-3)


def test_observer_sits_at_iy_zero(eng):
    """Two optically thick cells on a sightline, hot at iy = 0 and cold at iy = n_y - 1, and the
    mirror case: the map shows the FRONT cell's temperature, csrc * T_front."""
    from rajepy_amd import engine as E
    from rajepy_amd.maths import physics as ph
    nx, ny, nz = 2, 9, 3
    shape = (nx, ny, nz)
    nan = np.full(shape, np.nan)
    nd, xi, temp = nan.copy(), nan.copy(), nan.copy()
    ff, areas = np.ones(shape), np.ones(shape)
    hot, cold = 2.0e4, 5.0e3
    for x in range(nx):
        for zz in range(nz):
            front, back = (hot, cold) if (x + zz) % 2 == 0 else (cold, hot)
            for iy, tk in ((0, front), (ny - 1, back)):
                nd[x, iy, zz], xi[x, iy, zz], temp[x, iy, zz] = 1e9, 1.0, tk
    red = np.zeros(shape, dtype=bool)
    fields = eng.upload_fields(nd, xi, temp, ff, areas, None, red, csize_au=1.0, dtype=8)
    freqs = np.array([1e9, 5e9])
    gv = [ph.gff(nu, 1e4) for nu in freqs]
    ctau, cflux = E.ff_channel_coeffs(freqs, 1.0, 100., E.RJP_GFF_SCALAR, gv)
    got = _host(eng.ff_formal(fields, None, 0.0, E.RJP_GFF_SCALAR, ctau, cflux), 2, nx, nz)
    for x in range(nx):
        for zz in range(nz):
            front = hot if (x + zz) % 2 == 0 else cold
            for f in range(2):
                assert got[f, x, zz] == pytest.approx(cflux[f] * front, rel=1e-12)


def _random_case(seed):
    """Random grid, > 8 bursts in EACH jet (the device overflow table), NaN / zero cells in every
    field, sparse y-ranges (a random slab of empty rows at either end of every sightline)."""
    rng = np.random.default_rng(seed)
    shape = (int(rng.integers(1, 5)), int(rng.integers(20, 140)), int(rng.integers(3, 40)))
    nb = int(rng.integers(9, 14))
    which = np.array(["RB"] * nb)
    ej = {"t_0": rng.uniform(-0.5, 5.5, nb), "hl": rng.uniform(0.12, 1.2, nb),
          "chi": np.where(rng.random(nb) < 0.25, rng.uniform(0.2, 0.9, nb), rng.uniform(1.2, 12., nb)),
          "which": which}
    temp_mode = int(rng.integers(0, 2))
    g = U.synth_host(shape, 500 + seed, temp_mode)
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
    if temp_mode:
        p["power_laws"]["q_T"] = -0.5
    p["grid"].update(n_x=shape[0], n_y=shape[1], n_z=shape[2])
    jet = orc.OracleJet.from_fields(p, g["nd"], g["xi"], g["temp"], g["ff"], g["areas"],
                                    g["ts"], g["rr"], g["vy"])
    return rng, shape, g, jet


@pytest.mark.parametrize("nchan", [1, 16, 17, 64, 65, 256, 300])
def test_random_models_against_numpy_on_every_layout(eng, nchan):
    """Random models (> 8 bursts per jet, both jets, NaN / zero cells, sparse rows) for every
    lane layout of the kernel: against NumPy built from rjp_ff_cells' per-cell optical depths,
    and the tau, compact and wide layouts bit for bit, with and without occupied y-ranges."""
    rng, shape, g, jet = _random_case(700 + nchan)
    nx, ny, nz = shape
    freqs = np.geomspace(1e9, 5e10, nchan)
    mode, ctau, cflux = _coeffs(jet, freqs)
    bursts = U.bursts_from_oracle(jet)
    assert bursts.n[0] > 8 and bursts.n[1] > 8
    fields = _upload(eng, g, jet.csize, 8)
    eng.tau_layout(fields, mode)
    t = float(rng.uniform(0., 5.)) * orc.YEAR
    cells = eng.ff_cells(fields, bursts, t, mode, ctau).cpu().numpy().reshape(nchan, nx, ny, nz)
    ref = np_formal(cells, g["temp"], cflux)
    a0, em0 = fields.a0, fields.em0
    outs = {}
    for bounds in (False, True):
        if bounds:
            eng.compute_y_bounds(fields)
            assert fields.ylo is not None
        for name in ("tau", "compact", "wide"):
            fields.a0 = a0 if name == "tau" else None
            fields.em0 = None if name == "wide" else em0
            outs[name, bounds] = _host(eng.ff_formal(fields, bursts, t, mode, ctau, cflux),
                                       nchan, nx, nz)
        fields.a0, fields.em0 = a0, em0
    got = outs["tau", False]
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(got == 0.0, ref == 0.0)
    np.testing.assert_allclose(got, ref, rtol=1e-11, atol=0)
    for key, val in outs.items():
        assert np.array_equal(val, got, equal_nan=True), key


@pytest.mark.parametrize("temp_mode", [0, 1])
def test_cfg4_full_size(eng, temp_mode):
    """512 x 4096 x 512 cells, 256 channels (cfg4): isothermal fields equal ff_step's flux cube
    to 1e-12 everywhere; with a temperature spread, 28 sampled sightlines match NumPy on the
    oracle's per-cell tau to 1e-11."""
    from rajepy_amd import engine as E
    from rajepy_amd.maths import physics as ph
    shape = (512, 4096, 512)
    nx, ny, nz = shape
    seed = 20240507
    q_T = 0. if temp_mode == 0 else -0.5
    mode = E.RJP_GFF_SCALAR if temp_mode == 0 else E.RJP_GFF_POWERLAW
    fields = eng.synth_fields(shape, seed, temp_mode, 8, csize_au=0.5, wide=False, tau_mode=mode)
    freqs = np.geomspace(1e9, 5e10, 256)
    gv = [ph.gff(nu, 1e4) for nu in freqs] if mode == E.RJP_GFF_SCALAR else None
    ctau, cflux = E.ff_channel_coeffs(freqs, 0.5, 120., mode, gv)
    rng = np.random.default_rng(11)
    pix = [(int(rng.integers(nx)), int(rng.integers(nz))) for _ in range(24)]
    pix += [(0, 0), (nx - 1, nz - 1), (17, nz // 2 - 1), (17, nz // 2)]
    cells = np.array([(x * ny + y) * nz + z for (x, z) in pix for y in range(ny)], dtype=np.uint64)
    g = U.synth_host((len(pix), ny, 1), seed, temp_mode, cells=cells, nz_full=nz)
    p = copy.deepcopy(U.load_golden("cfg1_example")[2])
    p["ejection"] = U.example_bursts_params()
    p["power_laws"]["q_T"] = q_T
    p["grid"].update(n_x=len(pix), n_y=ny, n_z=1)
    jet = orc.OracleJet.from_fields(p, g["nd"], g["xi"], g["temp"], g["ff"], g["areas"],
                                    g["ts"], g["rr"], g["vy"])
    bursts = U.bursts_from_oracle(jet)
    t = 1.0 * orc.YEAR
    out = eng.ff_formal(fields, bursts, t, mode, ctau, cflux)
    if temp_mode == 0:
        tavg = eng.tavg(fields)
        P, F = nx * nz, len(freqs)
        sumA, flux = eng._f64(1, P), eng._f64(1, F, P)
        eng.ff_step(fields, bursts, [t], mode, tavg, ctau, cflux, (sumA, None, None, flux, None))
        eng.synchronize()
        import torch
        a, b = out.reshape(-1), flux.reshape(-1)
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        ok = ~torch.isnan(b)
        rel = ((a[ok] - b[ok]).abs() / b[ok].abs()).max().item()
        assert rel <= 1e-12, rel
        del flux, sumA
    xs, zs = [x for x, _ in pix], [z for _, z in pix]
    got = out.reshape(len(freqs), nx, nz)[:, xs, zs].cpu().numpy()      # [F, len(pix)]
    jet.time = t
    with np.errstate(all="ignore"):
        ref = np_formal(jet.optical_depth_ff(freqs, collapse=False), jet.temperature, cflux)
    np.testing.assert_allclose(got, ref[:, :, 0], rtol=1e-11, atol=0)


def _params_files(tmp_path, rrl_times):
    from tests.test_host_logic import example_params
    model = tmp_path / "model-params.py"
    p = example_params()

    def lit(v):
        return "np.array(%r)" % v.tolist() if isinstance(v, np.ndarray) else repr(v)

    body = ",\n".join("  %r: {%s}" % (sec, ", ".join("%r: %s" % (k, lit(v)) for k, v in d.items()))
                      for sec, d in p.items())
    model.write_text("import numpy as np\nparams = {\n" + body + "\n}\n")
    out = tmp_path / "cli_out"
    pline = tmp_path / "pipeline-params.py"
    pline.write_text(
        "import numpy as np\nparams = {'min_el': 20., 'dcys': {'model_dcy': %r},\n"
        " 'continuum': {'times': np.array([0., 1.]), 'freqs': np.array([5e9]), 't_obs': np.array([1200]),\n"
        "   'tscps': np.array([('VLA', 'A')]), 't_ints': np.array([5]), 'bws': np.array([4e8]), 'chanws': np.array([2e8])},\n"
        " 'rrls': {'times': np.array(%r), 'lines': np.array(['H66a']), 't_obs': np.array([1200]),\n"
        "   'tscps': np.array([('VLA', 'A')]), 't_ints': np.array([60]), 'bws': np.array([4e5]), 'chanws': np.array([1e5])}}\n"
        % (str(out), list(rrl_times)))
    return model, pline, out


def test_pipeline_and_cli_write_formal_flux_cubes(tmp_path):
    """`main.py -rt --formal` on the example model with a continuum-only run table: the Flux FITS
    data equal flux_ff(formal=True) of the model at the run's epoch, the header says so, and
    results['flux'] follows from the cube; intensity_ff(formal=True) of this isothermal model
    equals the isothermal map.  A run table with an RRL run is refused before any product."""
    from rajepy_amd import fits, main as cli
    model, pline, out = _params_files(tmp_path, [])
    pl = cli.main(["-rt", "--formal", str(model), str(pline)])
    m = pl.model
    found = 0
    for run in pl.runs:
        assert run.completed
        data, cards = fits.read(run.fits_flux)
        assert "Formal solution along the line of sight" in str(cards)
        m.time = run.year * orc.YEAR
        want = m.flux_ff(run.chan_freqs, formal=True)
        np.testing.assert_array_equal(np.nan_to_num(data),
                                      np.nan_to_num(np.swapaxes(want, -1, -2)))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            total = np.nansum(np.nanmean(want, axis=0))
        np.testing.assert_allclose(run.results["flux"], total, rtol=1e-12)
        iso = m.intensity_ff(run.chan_freqs)
        np.testing.assert_allclose(m.intensity_ff(run.chan_freqs, formal=True), iso, rtol=1e-12)
        _, cards_tau = fits.read(run.fits_tau)
        assert "Formal solution" not in str(cards_tau)
        found += 1
    assert found == 2

    os.makedirs(tmp_path / "rrl")
    model, pline, out = _params_files(tmp_path / "rrl", [0.])
    with pytest.raises(ValueError):
        cli.main(["-rt", "--formal", str(model), str(pline)])
    products = [f for r, _, fs in os.walk(out) for f in fs if f.endswith(".fits")]
    assert products == []


def test_abi_rejects_bad_arguments_with_nothing_enqueued(eng):
    """rjp_ff_formal: NULL d_out, n_chan <= 0, fields without temperature, a bad Gaunt mode ->
    RJP_ERR_ARG, and the output buffer keeps its contents."""
    from rajepy_amd import _lib, engine as E
    import torch
    g = U.synth_host((2, 16, 4), 3, 0)
    fields = eng.upload_fields(g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"],
                               g["rr"] < 0, csize_au=0.5, dtype=8)
    out = torch.full((2, 8), 7.0, dtype=torch.float64, device=eng.device)
    ct, cs = _lib.dbl_array([1e-20, 2e-20]), _lib.dbl_array([1.0, 2.0])
    lib = eng.lib

    def call(fs, mode=E.RJP_GFF_SCALAR, n=2, d_out=out.data_ptr()):
        return lib.rjp_ff_formal(eng.ctx, C.byref(fs), None, 0.0, mode, ct, cs, n, d_out,
                                 eng._stream())

    fs = fields.struct()
    assert call(fs, d_out=None) == _lib.RJP_ERR_ARG
    assert call(fs, n=0) == _lib.RJP_ERR_ARG
    assert call(fs, n=-3) == _lib.RJP_ERR_ARG
    assert call(fs, mode=7) == _lib.RJP_ERR_ARG
    no_t = fields.struct()
    no_t.d_temp = None
    assert call(no_t) == _lib.RJP_ERR_ARG
    eng.synchronize()
    assert bool((out == 7.0).all())
    assert call(fs) == _lib.RJP_OK
    eng.synchronize()
    assert not bool((out == 7.0).any())
