"""Epoch sweeps of the formal solution (rjp_ff_formal_sweep, K8): the maps of rjp_ff_formal at E
epochs and their per-channel totals from one walk of the grid, lanes over epochs.  Every map is
held to K5's at that epoch bit for bit (both lane layouts, their tails, the channel blocks, every
field layout), to a float64 NumPy restatement on the oracle's per-cell optical depths, the totals to
an exact sum of the device's own maps, and the light curves through JetModel."""
import copy
import ctypes as C
import math

import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U
from tests.test_gpu_formal_rt import _coeffs, _random_case, _upload, np_formal

pytestmark = pytest.mark.gpu
YEAR = orc.YEAR


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()


def _epochs(rng, E):
    """Unsorted epochs [s] over the bursts' span, one far outside every burst's support and one
    duplicate (where E leaves room for them)."""
    t = rng.uniform(-0.5, 6.0, E) * YEAR
    if E >= 3:
        t[1] = 500.0 * YEAR
        t[-1] = t[0]
    return [float(v) for v in t]


def _case(eng, seed, E, F, dtype=8):
    rng, shape, g, jet = _random_case(seed)
    freqs = np.geomspace(1e9, 5e10, F)
    mode, ctau, cflux = _coeffs(jet, freqs)
    bursts = U.bursts_from_oracle(jet)
    assert bursts.n[0] > 8 and bursts.n[1] > 8
    fields = _upload(eng, g, jet.csize, dtype)
    if dtype == 8:
        eng.tau_layout(fields, mode)
        assert fields.a0 is not None
    return rng, shape, g, jet, fields, bursts, mode, ctau, cflux, _epochs(rng, E)


def _k5(eng, fields, bursts, epochs, mode, ctau, cflux):
    """rjp_ff_formal once per distinct epoch -> host array [E, F, P]."""
    done = {}
    for t in epochs:
        if t not in done:
            done[t] = eng.ff_formal(fields, bursts, t, mode, ctau, cflux).cpu().numpy()
    return np.stack([done[t] for t in epochs])


# epoch tails of both lane layouts (16 and 64 lanes), a 64-lane block followed by 16-lane blocks,
# the overflow of the 4-channel register block, several epoch blocks
SHAPES = [(1, 1), (15, 1), (16, 3), (17, 4), (63, 1), (64, 5), (65, 2), (130, 9)]


@pytest.mark.parametrize("E,F", SHAPES)
def test_every_map_is_k5_bit_for_bit_on_every_layout(eng, E, F):
    """Random models (> 8 bursts per jet, NaN / zero cells, sparse rows, an empty sightline): each
    [e, f] map of the sweep equals rjp_ff_formal at that epoch exactly, on the tau, compact and wide
    layouts, with and without occupied y-ranges."""
    rng, shape, g, jet, fields, bursts, mode, ctau, cflux, epochs = _case(eng, 900 + 7 * E + F, E, F)
    P = shape[0] * shape[2]
    a0, em0 = fields.a0, fields.em0
    want = _k5(eng, fields, bursts, epochs, mode, ctau, cflux)
    assert np.isnan(want[:, :, 0]).all()                       # the empty sightline
    assert np.isfinite(want).any() and (want[np.isfinite(want)] > 0).any()
    for bounds in (False, True):
        if bounds:
            eng.compute_y_bounds(fields)
            assert fields.ylo is not None
        for name in ("tau", "compact", "wide"):
            fields.a0 = a0 if name == "tau" else None
            fields.em0 = None if name == "wide" else em0
            maps, ftot = eng.ff_formal_sweep(fields, bursts, epochs, mode, ctau, cflux,
                                             want_maps=True)
            got = maps.cpu().numpy()
            assert got.shape == (E, F, P) and tuple(ftot.shape) == (E, F)
            assert np.array_equal(got, want, equal_nan=True), (name, bounds)
            # K5 on this very layout, at three of the epochs
            for e in sorted({0, E // 2, E - 1}):
                one = eng.ff_formal(fields, bursts, epochs[e], mode, ctau, cflux).cpu().numpy()
                assert np.array_equal(got[e], one, equal_nan=True), (name, bounds, e)
        fields.a0, fields.em0 = a0, em0


@pytest.mark.parametrize("E,F", [(17, 4), (65, 2)])
def test_f32_storage_is_k5_on_the_same_fields(eng, E, F):
    rng, shape, g, jet, fields, bursts, mode, ctau, cflux, epochs = _case(eng, 1200 + E, E, F,
                                                                          dtype=4)
    em0 = fields.em0
    for name in ("compact", "wide"):
        fields.em0 = em0 if name == "compact" else None
        if name == "compact" and em0 is None:
            continue
        want = _k5(eng, fields, bursts, epochs, mode, ctau, cflux)
        got = eng.ff_formal_sweep(fields, bursts, epochs, mode, ctau, cflux, want_maps=True,
                                  want_totals=False)[0].cpu().numpy()
        assert np.isfinite(want).any()
        assert np.array_equal(got, want, equal_nan=True), name
    fields.em0 = em0


def test_tilted_golden_against_numpy_on_the_oracles_cells(eng):
    """tests/golden/tilted (q_T = -0.05, q^d_T = -0.1, bursts in both jets), all golden epochs and
    frequencies in ONE call: the maps against NumPy on the oracle's per-cell tau and T to 1e-11
    (K5's bound), equal NaN and exact-zero patterns; the totals against its nansum."""
    z, meta, p, g, jet = U.golden_dense("tilted")
    freqs = np.asarray(z["freqs"], dtype=np.float64)
    mode, ctau, cflux = _coeffs(jet, freqs)
    fields = _upload(eng, g, jet.csize, 8)
    eng.tau_layout(fields, mode)
    bursts = U.bursts_from_oracle(jet)
    F, nx, nz = len(freqs), jet.nx, jet.nz
    epochs = [float(yr) * YEAR for yr in z["years"]]
    maps, ftot = eng.ff_formal_sweep(fields, bursts, epochs, mode, ctau, cflux, want_maps=True)
    got = maps.cpu().numpy().reshape(len(epochs), F, nx, nz)
    tot = ftot.cpu().numpy()
    for e, t in enumerate(epochs):
        jet.time = t
        with np.errstate(all="ignore"):
            ref = np_formal(jet.optical_depth_ff(freqs, collapse=False), jet.temperature, cflux)
        assert np.array_equal(np.isnan(got[e]), np.isnan(ref))
        assert np.array_equal(got[e] == 0.0, ref == 0.0)
        np.testing.assert_allclose(got[e], ref, rtol=1e-11, atol=0)
        np.testing.assert_allclose(tot[e], np.nansum(ref, axis=(1, 2)), rtol=1e-11, atol=0)


def test_totals_are_the_fixed_order_nansum_of_the_maps(eng):
    """ftot[e, f] against math.fsum over the finite pixels of the device's own map: all terms are
    >= 0 and the order is fixed, so the error is below P 2^-53 relative.  The same bits with the
    maps NULL and on a second call; against NumPy's formal solution to 1e-11; exactly 0 where no
    pixel is finite."""
    E, F = 70, 5                              # a 64-lane block and a 16-lane block, two channel blocks
    rng, shape, g, jet, fields, bursts, mode, ctau, cflux, epochs = _case(eng, 1301, E, F)
    nx, ny, nz = shape
    P = nx * nz
    maps, ftot = eng.ff_formal_sweep(fields, bursts, epochs, mode, ctau, cflux, want_maps=True)
    m, tot = maps.cpu().numpy(), ftot.cpu().numpy()
    assert (m[np.isfinite(m)] >= 0).all()
    for e in range(E):
        for f in range(F):
            v = m[e, f]
            exact = math.fsum(v[np.isfinite(v)])
            assert exact > 0
            assert abs(tot[e, f] - exact) <= P * 2.0 ** -53 * exact, (e, f, tot[e, f], exact)
    _, only = eng.ff_formal_sweep(fields, bursts, epochs, mode, ctau, cflux, want_maps=False)
    assert np.array_equal(only.cpu().numpy(), tot)
    _, again = eng.ff_formal_sweep(fields, bursts, epochs, mode, ctau, cflux, want_maps=True)
    assert np.array_equal(again.cpu().numpy(), tot)
    for e in (0, 1, E - 1):
        cells = eng.ff_cells(fields, bursts, epochs[e], mode, ctau).cpu().numpy()
        ref = np_formal(cells.reshape(F, nx, ny, nz), g["temp"], cflux)
        np.testing.assert_allclose(tot[e], np.nansum(ref, axis=(1, 2)), rtol=1e-11, atol=0)
    # no sightline with T > 0: every map is NaN everywhere, every total exactly 0
    cold = dict(g, temp=np.full(shape, np.nan))
    dark = _upload(eng, cold, jet.csize, 8)
    maps, ftot = eng.ff_formal_sweep(dark, bursts, epochs[:18], mode, ctau, cflux, want_maps=True)
    assert bool(maps.isnan().all())
    t0 = ftot.cpu().numpy()
    assert np.array_equal(t0, np.zeros((18, F))) and not np.signbit(t0).any()


def test_without_bursts_every_epoch_is_the_single_epoch_map(eng):
    """bursts = NULL: the maps do not depend on the epoch.  Bursts in the red jet only: the blue
    jet's cells keep chi = 1 whatever their launch time (NaN included), as in K5."""
    from rajepy_amd.engine import make_bursts
    E, F = 20, 2
    rng, shape, g, jet, fields, bursts, mode, ctau, cflux, epochs = _case(eng, 1402, E, F)
    one = eng.ff_formal(fields, None, 0.0, mode, ctau, cflux).cpu().numpy()
    assert np.isfinite(one).any()
    maps, ftot = eng.ff_formal_sweep(fields, None, epochs, mode, ctau, cflux, want_maps=True)
    got = maps.cpu().numpy()
    for e in range(E):
        assert np.array_equal(got[e], one, equal_nan=True), e
    tot = ftot.cpu().numpy()
    assert (tot == tot[0]).all()
    ts, fields.ts = fields.ts, None            # ... and the launch times are not needed at all
    try:
        again = eng.ff_formal_sweep(fields, None, epochs, mode, ctau, cflux, want_maps=True)[0]
        assert np.array_equal(again.cpu().numpy(), got, equal_nan=True)
    finally:
        fields.ts = ts
    red = []
    for t0, peak, hl in jet.bursts["R"]:
        red.append((t0, (peak - jet._ss_jml_rj) / jet._ss_jml_rj,
                    hl * 2. / (2. * np.sqrt(2. * np.log(2.)))))
    red_only = make_bursts(red, [])
    assert red_only.n[0] > 8 and red_only.n[1] == 0
    want = _k5(eng, fields, red_only, epochs, mode, ctau, cflux)
    got = eng.ff_formal_sweep(fields, red_only, epochs, mode, ctau, cflux, want_maps=True,
                              want_totals=False)[0].cpu().numpy()
    assert np.array_equal(got, want, equal_nan=True)
    assert not np.array_equal(want[0], want[2], equal_nan=True)     # the red jet does vary


def _raw(eng, fs, bursts, epochs, mode, ctau, cflux, d_out, d_ftot, d_work, work_bytes, n_ep=None,
         n_ch=None, null_ctau=False, null_epochs=False):
    from rajepy_amd import _lib
    return eng.lib.rjp_ff_formal_sweep(
        eng.ctx, C.byref(fs), C.byref(bursts) if bursts is not None else None,
        None if null_epochs else _lib.dbl_array(epochs), len(epochs) if n_ep is None else n_ep,
        mode, None if null_ctau else _lib.dbl_array(ctau), _lib.dbl_array(cflux),
        len(ctau) if n_ch is None else n_ch, d_out, d_ftot, d_work, work_bytes, eng._stream())


def test_workspace_of_exactly_the_stated_size_and_an_untouched_guard_band(eng):
    import torch
    from rajepy_amd import _lib
    E, F = 70, 5
    rng, shape, g, jet, fields, bursts, mode, ctau, cflux, epochs = _case(eng, 1503, E, F)
    nx, ny, nz = shape
    wb = eng.lib.rjp_ff_formal_sweep_workspace(nx, ny, nz, E, F)
    assert wb > 0
    guard = 1 << 16
    buf = torch.full((wb + guard,), 0xA5, dtype=torch.uint8, device=eng.device)
    ftot = torch.full((E, F), -7.0, dtype=torch.float64, device=eng.device)
    fs = fields.struct()
    assert _raw(eng, fs, bursts, epochs, mode, ctau, cflux, None, ftot.data_ptr(), buf.data_ptr(),
                wb) == _lib.RJP_OK
    eng.synchronize()
    assert bool((buf[wb:] == 0xA5).all())
    _, want = eng.ff_formal_sweep(fields, bursts, epochs, mode, ctau, cflux)
    assert torch.equal(ftot, want)


def test_abi_refusals_leave_the_outputs_untouched(eng):
    """Every refusal rjprt.h lists returns its status with nothing enqueued: the outputs keep the
    sentinel they were filled with."""
    import torch
    from rajepy_amd import _lib
    E, F = 5, 2
    rng, shape, g, jet, fields, bursts, mode, ctau, cflux, epochs = _case(eng, 1604, E, F)
    nx, ny, nz = shape
    P = nx * nz
    out = torch.full((E, F, P), 7.0, dtype=torch.float64, device=eng.device)
    ftot = torch.full((E, F), 7.0, dtype=torch.float64, device=eng.device)
    wb = eng.lib.rjp_ff_formal_sweep_workspace(nx, ny, nz, E, F)
    work = torch.zeros(wb, dtype=torch.uint8, device=eng.device)
    fs = fields.struct()
    o, t, w = out.data_ptr(), ftot.data_ptr(), work.data_ptr()

    def call(fs=fs, b=bursts, ep=epochs, m=mode, d_out=o, d_ftot=t, d_work=w, nbytes=wb, **kw):
        return _raw(eng, fs, b, ep, m, ctau, cflux, d_out, d_ftot, d_work, nbytes, **kw)

    ARG, WS = _lib.RJP_ERR_ARG, _lib.RJP_ERR_WORKSPACE
    assert call(m=7) == ARG
    assert call(null_ctau=True) == ARG
    assert call(null_epochs=True) == ARG
    assert call(n_ep=0) == ARG
    assert call(n_ep=-2) == ARG
    assert call(n_ch=0) == ARG
    assert call(n_ch=-1) == ARG
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(ep=epochs[:2] + [bad] + epochs[3:]) == ARG
    assert call(d_out=None, d_ftot=None) == ARG
    no_ts = fields.struct()
    no_ts.d_ts = None
    assert call(fs=no_ts) == ARG
    no_t = fields.struct()
    no_t.d_temp = None
    assert call(fs=no_t) == ARG
    assert call(nbytes=wb - 1) == WS
    assert call(d_work=None) == WS
    assert call(nbytes=0) == WS
    eng.synchronize()
    assert bool((out == 7.0).all()) and bool((ftot == 7.0).all())
    # maps alone need no workspace; then the whole call
    assert call(d_ftot=None, d_work=None, nbytes=0) == _lib.RJP_OK
    eng.synchronize()
    assert not bool((out == 7.0).any()) and bool((ftot == 7.0).all())
    assert call() == _lib.RJP_OK
    eng.synchronize()
    assert not bool((ftot == 7.0).any())
    assert eng.lib.rjp_ff_formal_sweep_workspace(nx, ny, nz, 0, F) == 0
    with pytest.raises(ValueError):
        eng.ff_formal_sweep(fields, bursts, epochs, mode, ctau, cflux, want_maps=False,
                            want_totals=False)


def _tilted_params():
    p = copy.deepcopy(U.load_golden("tilted")[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


def test_jetmodel_flux_vs_time_formal(tmp_path):
    """The example model (isothermal): flux_vs_time(formal=True) equals the per-epoch
    nansum(flux_ff(formal=True)) to 1e-12 and the isothermal curve at the 5 golden epochs (fewer
    than 12: the epoch tiles) to 1e-10 -- the sum telescopes, and 1e-10 is K5's bound against the
    golden maps.  A model with a temperature gradient: the two curves differ by > 1e-3."""
    from rajepy_amd import classes, logger
    from tests.test_host_logic import example_params
    z, meta, _ = U.load_golden("cfg1_example")
    log = logger.Log(str(tmp_path / "a.log"), verbose=False)
    jm = classes.JetModel(example_params(), log=log)
    times = np.asarray(z["years"], dtype=np.float64) * YEAR
    freqs = np.asarray(z["freqs"], dtype=np.float64)
    assert len(times) < 12
    lc = jm.flux_vs_time(times, freqs, formal=True)
    assert lc.shape == (len(times), len(freqs)) and np.isfinite(lc).all() and (lc > 0).all()
    for e, t in enumerate(times):
        jm.time = t
        one = np.nansum(jm.flux_ff(freqs, formal=True), axis=(1, 2))
        np.testing.assert_allclose(lc[e], one, rtol=1e-12, atol=0)
    iso = jm.flux_vs_time(times, freqs)
    assert jm.engine.last_scan_path()[0] == "tiles"
    np.testing.assert_allclose(lc, iso, rtol=1e-10, atol=0)
    np.testing.assert_array_equal(jm.flux_vs_time(times, freqs), iso)      # the default is as it was

    z2 = U.load_golden("tilted")[0]
    jt = classes.JetModel(_tilted_params(), log=log)
    t2 = np.asarray(z2["years"], dtype=np.float64) * YEAR
    f2 = np.asarray(z2["freqs"], dtype=np.float64)
    formal, iso2 = jt.flux_vs_time(t2, f2, formal=True), jt.flux_vs_time(t2, f2)
    assert np.max(np.abs(formal / iso2 - 1.0)) > 1e-3
