"""rjp_ff_formal_grad (K9, ff_formal_grad.hip): the sensitivities of the formal-solution light curves
to the burst parameters, through the C-ABI, RTEngine.ff_formal_grad and
JetModel.flux_vs_time_jac(formal=True), against tests/ff_formal_grad_ref.py -- a long-double NumPy
restatement run on the arrays read back from the device, which
tests/test_ff_formal_grad_reference_cpu.py pins to NumPy's formal solution, to K7's formula in the
isothermal limit, to Richardson differences and to hand-worked cells, and whose cases it holds to a
non-vacuity condition.

Bounds (derived in the reference module, not measured): per pixel and plane
    |got - ref| <= [3e-12 (2 + tau_sightline) + n_y (4e-15 + 4 2^-53)] abs_k  (+ the float64
    underflow floor, < 1e-280),
abs_k the sum of the absolute terms; totals: the sum of the per-pixel bounds + P 2^-53 sum_p abs_k.
The d_ftot output is held to rjp_ff_formal_sweep's bit for bit.  The module prints the worst
|got - ref| / bound per output."""
import copy
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import ff_formal_grad_ref as R
from tests import ff_grad_ref as R7
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
YEAR = orc.YEAR
WORST = {}


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()
    print("\nworst |got - ref| / bound per output: " +
          ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def note(kind, got, ref, absref, bound, floor=0.0):
    r = R.worst_ratio(got, ref, absref, bound, floor)
    WORST[kind] = max(WORST.get(kind, 0.0), r)
    print("%-8s worst |got - ref| / bound = %.3f" % (kind, r))
    assert r <= 1.0, (kind, r)


def upload(eng, g, mode=0):
    """upload_fields (-> wide + compact layouts) + the tau layout; -> fields and the arrays the
    device holds: a0 (jet flag in the sign bit), ts, temp."""
    f = eng.upload_fields(g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"], g["rr"] < 0,
                          g["vy"], csize_au=0.5, dtype=8)
    assert f.em0 is not None
    eng.tau_layout(f, mode)
    assert f.a0 is not None
    return f, device_arrays(f)


def device_arrays(f):
    rd = lambda t: t.cpu().numpy().astype(np.float64).reshape(f.shape)
    return rd(f.a0), rd(f.ts), rd(f.temp)


def walk_boxed(a0, ts, temp, bursts, t, ctau, csrc):
    """R.walk on the x-rows and y-range that hold a finite a0 (the others add nothing), put back
    into whole maps: 0 on a sightline without a live cell, NaN where it has no T > 0."""
    nx, ny, nz = a0.shape
    live = np.isfinite(a0)
    xs = np.where(live.any(axis=(1, 2)))[0]
    ys = np.where(live.any(axis=(0, 2)))[0]
    hot = np.any(temp > 0.0, axis=1)
    sl = (slice(xs.min(), xs.max() + 1), slice(ys.min(), ys.max() + 1))
    # (a T > 0 outside the box belongs to a dead cell: it makes the sightline hot, no more)
    tb = temp[sl].copy()
    tb[:, 0, :] = np.where(hot[sl[0]] & ~np.any(tb > 0, axis=1), 1.0, tb[:, 0, :])
    a0b = a0[sl].copy()
    res = R.walk(a0b, ts[sl], tb, bursts, t, ctau, csrc)
    F, npar = len(ctau), res["dI"].shape[1]
    out = dict(hot=hot)
    for k, shp in (("I", (F,)), ("tau", (F,)), ("dI", (F, npar)), ("abs", (F, npar)),
                   ("floor", (F, npar))):
        full = np.zeros(shp + (nx, nz), dtype=res[k].dtype)
        full[..., sl[0], :] = res[k]
        if k in ("I", "dI", "abs"):
            full = np.where(hot, full, np.nan)
        out[k] = full
    return out


def raw(eng, f, bursts, epochs, mode, ctau, csrc, ftot, dftot, dout, work=None, nbytes=None,
        n_ep=None, n_ch=None, fs=None):
    from rajepy_amd import _lib
    nx, ny, nz = f.shape
    npar = 3 * (int(bursts.n[0]) + int(bursts.n[1])) if bursts is not None else 0
    need = eng.lib.rjp_ff_formal_grad_workspace(nx, ny, nz, len(epochs), max(npar, 3), len(ctau))
    if work is None:
        work = eng._workspace(max(need, 1))
    fs = f.struct() if fs is None else fs
    ptr = lambda t: t.data_ptr() if t is not None else None
    return eng.lib.rjp_ff_formal_grad(
        eng.ctx, C.byref(fs), C.byref(bursts) if bursts is not None else None,
        _lib.dbl_array(epochs), len(epochs) if n_ep is None else n_ep, mode, _lib.dbl_array(ctau),
        _lib.dbl_array(csrc), len(ctau) if n_ch is None else n_ch, ptr(ftot), ptr(dftot), ptr(dout),
        work.data_ptr(), need if nbytes is None else nbytes, eng._stream())


def check(eng, f, arrays, bursts, epochs, ctau, csrc, mode=0, refs=None, what=""):
    """One call with every output against the reference and against K8 / K5; -> (host outputs,
    refs)."""
    from rajepy_amd import engine as E
    a0, ts, temp = arrays
    nx, ny, nz = f.shape
    P, nE, F = nx * nz, len(epochs), len(ctau)
    b = E.make_bursts(*bursts)
    npar = 3 * (len(bursts[0]) + len(bursts[1]))
    ftot, dftot, dmaps = eng.ff_formal_grad(f, b, epochs, mode, ctau, csrc, want_maps=True)
    eng.synchronize()
    ftot, dftot, dmaps = (t.cpu().numpy() for t in (ftot, dftot, dmaps))
    assert ftot.shape == (nE, F) and dftot.shape == (nE, F, npar) and dmaps.shape == (nE, F, npar, P)
    # F: K8's totals bit for bit
    _, k8 = eng.ff_formal_sweep(f, b, epochs, mode, ctau, csrc)
    assert np.array_equal(ftot, k8.cpu().numpy()), what
    if refs is None:
        refs = {}
    for e, t in enumerate(epochs):
        if t not in refs:
            refs[t] = walk_boxed(a0, ts, temp, bursts, t, ctau, csrc)
            refs[t]["tot"] = R.totals(refs[t], ny)
        ref = refs[t]
        bound = R.pixel_bound(ref["tau"], ny)[:, None]
        got = dmaps[e].reshape(F, npar, nx, nz)
        for c, kind in enumerate(("dI/dt0", "dI/damp", "dI/dinv")):
            note(kind, got[:, c::3], ref["dI"][:, c::3], ref["abs"][:, c::3], bound,
                 ref["floor"][:, c::3])
        tot = ref["tot"]
        note("F", ftot[e], tot["F"], np.ones_like(tot["F"]), tot["boundF"])
        note("dF", dftot[e], tot["dF"], np.ones_like(tot["dF"]), tot["bounddF"], tot["floordF"])
        if e in (0, nE - 1):
            # the NaN pattern is K5's map's
            k5 = eng.ff_formal(f, b, t, mode, ctau, csrc).cpu().numpy().reshape(F, 1, nx, nz)
            assert np.array_equal(np.isnan(got), np.broadcast_to(np.isnan(k5), got.shape)), what
    return (ftot, dftot, dmaps), refs


_CASE = {}


def case(eng, name):
    """Fields, device arrays, tables and the reference of one synthetic case, made once."""
    if name not in _CASE:
        shape, seed, E, F, bs, yb = R.CASES[name]
        g = R.synth_fields(shape, seed)
        f, arrays = upload(eng, g)
        ctau, csrc = R.channel_tables(R.host_a0(g), F)
        _CASE[name] = dict(f=f, arrays=arrays, ctau=ctau, csrc=csrc, bursts=R.burst_set(bs),
                           epochs=R.epochs(seed, E), yb=yb, refs={})
    return _CASE[name]


# ---- 1-3: every output on every code path ----------------------------------------------------------
@pytest.mark.parametrize("name", list(R.CASES))
def test_maps_and_totals_against_the_reference_on_every_layout(eng, name):
    """Ragged 16-sightline tiles and 16-row slab tails, NaN / zero cells, a sparse row, an empty
    sightline, sightlines of one jet and of both; the axes of ff_formal_grad_ref.CASES.  The tau
    layout against the reference (every plane, pixel, epoch and channel; NaN pattern K5's; exact
    zeros where the reference's terms are all zero), d_ftot bit for bit K8's, and the compact and
    wide layouts bit for bit the tau layout's."""
    c = case(eng, name)
    f = c["f"]
    if c["yb"]:
        eng.compute_y_bounds(f)
        assert f.ylo is not None
    out, c["refs"] = check(eng, f, c["arrays"], c["bursts"], c["epochs"], c["ctau"], c["csrc"],
                           refs=c["refs"], what=name)
    P = f.shape[0] * f.shape[2]
    dm = out[2].reshape(len(c["epochs"]), len(c["ctau"]), -1, *[f.shape[0], f.shape[2]])
    assert np.isnan(dm[..., 0, 0]).all()                                  # the empty sightline
    assert np.isfinite(dm).any() and (dm[np.isfinite(dm)] > 0).any() and (dm[np.isfinite(dm)] < 0).any()
    nz = f.shape[2]
    if len(c["bursts"][0]) and nz >= 8:
        # a red burst's planes are exact zeros on the all-blue sightlines (the last quarter of z)
        assert np.all(dm[:, :, :3, :, nz - nz // 4:][np.isfinite(dm[:, :, :3, :, nz - nz // 4:])] == 0)
    from rajepy_amd import engine as E
    b = E.make_bursts(*c["bursts"])
    a0, em0 = f.a0, f.em0
    try:
        for lay in ("compact", "wide"):
            f.a0 = None
            f.em0 = em0 if lay == "compact" else None
            again = eng.ff_formal_grad(f, b, c["epochs"], 0, c["ctau"], c["csrc"], want_maps=True)
            for x, y in zip(again, out):
                assert np.array_equal(x.cpu().numpy(), y, equal_nan=True), (name, lay)
    finally:
        f.a0, f.em0 = a0, em0
    if c["yb"]:
        # ... and without the occupied y-ranges
        ylo, yhi, f.ylo, f.yhi = f.ylo, f.yhi, None, None
        try:
            again = eng.ff_formal_grad(f, b, c["epochs"], 0, c["ctau"], c["csrc"], want_maps=True)
            for x, y in zip(again, out):
                assert np.array_equal(x.cpu().numpy(), y, equal_nan=True), name
        finally:
            f.ylo, f.yhi = ylo, yhi
    assert P == out[2].shape[-1]


def test_null_output_combinations_and_reproducibility(eng):
    """All seven non-empty NULL combinations reproduce the full call's outputs bit for bit, as does
    a second full call; d_ftot is K8's with d_dout NULL and with d_dftot NULL."""
    import torch
    from rajepy_amd import engine as E
    c = case(eng, "example-E17-F5")
    f, b = c["f"], E.make_bursts(*c["bursts"])
    full = eng.ff_formal_grad(f, b, c["epochs"], 0, c["ctau"], c["csrc"], want_maps=True)
    full = [t.clone() for t in full]
    k8 = eng.ff_formal_sweep(f, b, c["epochs"], 0, c["ctau"], c["csrc"])[1]
    assert torch.equal(full[0], k8)
    for mask in itertools.product((False, True), repeat=3):
        outs = [torch.full_like(t, -7.0) if m else None for t, m in zip(full, mask)]
        st = raw(eng, f, b, c["epochs"], 0, c["ctau"], c["csrc"], *outs)
        eng.synchronize()
        if not any(mask):
            assert st == E._lib.RJP_ERR_ARG
            continue
        assert st == 0, (mask, eng.lib.rjp_last_error(eng.ctx))
        for o, want in zip(outs, full):
            if o is not None:
                assert torch.equal(o.nan_to_num(nan=-1.0), want.nan_to_num(nan=-1.0)), mask
                assert torch.equal(o.isnan(), want.isnan()), mask
    again = eng.ff_formal_grad(f, b, c["epochs"], 0, c["ctau"], c["csrc"], want_maps=True)
    for x, y in zip(again, full):
        assert torch.equal(x.nan_to_num(nan=-1.0), y.nan_to_num(nan=-1.0))


# ---- 4: the isothermal golden model against K7 ------------------------------------------------------
def _oracle_burst_lists(jet):
    out = []
    for which, ss in (("R", jet._ss_jml_rj), ("B", jet._ss_jml_bj)):
        out.append([(t0, (peak - ss) / ss, hl * 2. / (2. * np.sqrt(2. * np.log(2.))))
                    for t0, peak, hl in jet.bursts[which]])
    return out[0], out[1]


def _golden(eng, tag):
    from tests.test_gpu_formal_rt import _coeffs, _upload
    z, meta, p, g, jet = U.golden_dense(tag)
    freqs = np.asarray(z["freqs"], dtype=np.float64)
    mode, ctau, cflux = _coeffs(jet, freqs)
    f = _upload(eng, g, jet.csize, 8)
    eng.tau_layout(f, mode)
    assert f.a0 is not None
    return z, jet, f, mode, ctau, cflux, _oracle_burst_lists(jet)


def test_isothermal_golden_model_equals_k7(eng):
    """cfg1_example (constant T): d_dftot equals rjp_ff_grad's d_dftot within the sum of the two
    calls' bounds (K7's: ff_grad_ref.totals_bound x its absolute sum)."""
    from rajepy_amd import engine as E
    z, jet, f, mode, ctau, cflux, bursts = _golden(eng, "cfg1_example")
    epochs = [float(y) * YEAR for y in z["years"][1:4]]
    b = E.make_bursts(*bursts)
    ftot, dftot, _ = eng.ff_formal_grad(f, b, epochs, mode, ctau, cflux)
    tavg = eng.tavg(f)
    _, _, f7, d7 = eng.ff_grad(f, b, epochs, mode, tavg, ctau, cflux)
    got, want = dftot.cpu().numpy(), d7.cpu().numpy()
    a0, ts, temp = device_arrays(f)
    nx, ny, nz = f.shape
    tav = tavg.cpu().numpy()
    for e, t in enumerate(epochs):
        ref9 = R.totals(walk_boxed(a0, ts, temp, bursts, t, ctau, cflux), ny)
        ref7 = R7.totals(R7.planes(a0, ts, bursts, t), tav, ctau, cflux)
        lim = ref9["bounddF"] + ref9["floordF"] + \
            R7.totals_bound(ny, nx * nz, ref7["tau_max"], U.GAUSS_RTOL) * ref7["absdF"]
        err = np.abs(got[e] - want[e])
        assert (lim > 0).all() and (np.abs(want[e]) > 0).all()
        r = float((err / lim).max())
        WORST["dF-vs-K7"] = max(WORST.get("dF-vs-K7", 0.0), r)
        assert r <= 1.0, (e, r)
        np.testing.assert_allclose(ftot.cpu().numpy()[e], f7.cpu().numpy()[e], rtol=1e-10)


# ---- 5: the tilted golden model ----------------------------------------------------------------------
def test_tilted_golden_model_against_the_reference(eng):
    """tests/golden/tilted (q_T = -0.05, q^d_T = -0.1, bursts in both jets), the oracle's fields:
    maps and totals at every golden epoch and frequency."""
    z, jet, f, mode, ctau, cflux, bursts = _golden(eng, "tilted")
    epochs = [float(y) * YEAR for y in z["years"]]
    out, _ = check(eng, f, device_arrays(f), bursts, epochs, ctau, cflux, mode=mode, what="tilted")
    assert (np.abs(out[1]) > 0).all()


# ---- 6: JetModel -----------------------------------------------------------------------------------
def _tilted_params():
    p = copy.deepcopy(U.load_golden("tilted")[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


def test_jetmodel_flux_vs_time_jac_formal(eng, tmp_path):
    from rajepy_amd import classes, logger
    log = logger.Log(str(tmp_path / "m.log"), verbose=False)
    jm = classes.JetModel(_tilted_params(), log=log, engine=eng)
    z = U.load_golden("tilted")[0]
    times = np.asarray(z["years"], dtype=np.float64)[1:] * YEAR
    freqs = np.asarray(z["freqs"], dtype=np.float64)[:2]
    flux, jac = jm.flux_vs_time_jac(times, freqs, formal=True)
    ej = list(jm.ejections.values())
    assert flux.shape == (len(times), 2) and jac.shape == (len(times), 2, len(ej), 3) and len(ej) >= 2
    assert np.array_equal(flux, jm.flux_vs_time(times, freqs, formal=True))
    dev = jm.device_fields
    assert dev.a0 is not None
    a0, ts, temp = device_arrays(dev)
    bursts = (jm._bursts["R"], jm._bursts["B"])
    _, (ctau, cflux) = jm._channel_coeffs(freqs)
    slots = jm._ejection_slots()
    iso = jm.flux_vs_time_jac(times, freqs)[1]
    differs = False
    for e, t in enumerate(times):
        tot = R.totals(walk_boxed(a0, ts, temp, bursts, float(t), ctau, cflux), jm.ny)
        for i, (k, chain) in enumerate(slots):
            ch = np.asarray(chain)[None]
            # (one more rounding on the host: the product with the chain factor)
            note("jac", jac[e, :, i, :], tot["dF"][:, k:k + 3] * ch, np.ones((2, 3)),
                 (tot["bounddF"][:, k:k + 3] + R.EPS * tot["absdF"][:, k:k + 3]) * np.abs(ch),
                 tot["floordF"][:, k:k + 3] * np.abs(ch))
            differs |= bool((np.abs(jac[e, :, i, :] - iso[e, :, i, :]) >
                             1e-3 * tot["absdF"][:, k:k + 3] * np.abs(ch)).any())
    assert differs, "the formal and the isothermal Jacobian must not come from the same kernel"
    # n_ej = 0 and no epochs: through flux_vs_time(formal=True)
    q = _tilted_params()
    q["ejection"] = {"t_0": np.array([]), "hl": np.array([]), "chi": np.array([]),
                     "which": np.array([])}
    j0 = classes.JetModel(q, log=log, engine=eng)
    fl0, jac0 = j0.flux_vs_time_jac(times, freqs, formal=True)
    assert jac0.shape == (len(times), 2, 0, 3)
    assert np.array_equal(fl0, j0.flux_vs_time(times, freqs, formal=True))
    fl1, jac1 = jm.flux_vs_time_jac([], freqs, formal=True)
    assert fl1.shape == (0, 2) and jac1.shape == (0, 2, len(ej), 3)
    # f32 storage raises
    f32 = classes.JetModel(_tilted_params(), log=log, engine=eng, storage="f32")
    with pytest.raises(ValueError, match="f64 storage"):
        f32.flux_vs_time_jac(times, freqs, formal=True)


def test_jetmodel_on_the_wide_layout(eng, tmp_path):
    """A model whose fields carry negative path factors stays on the wide layout (no em0, no a0):
    flux_vs_time_jac(formal=True) still runs, its flux is flux_vs_time(formal=True) bit for bit,
    and the tau-layout-only route refuses."""
    from rajepy_amd import classes, logger
    p = copy.deepcopy(U.load_golden("cfg1_example")[2])
    p["ejection"] = U.example_bursts_params()
    jm = classes.JetModel(p, log=logger.Log(str(tmp_path / "w.log"), verbose=False), engine=eng)
    shape = (3, 37, 50)
    g = U.synth_host(shape, 77, 1)
    g["ff"] = np.where(g["ff"] == 0.5, -0.37, 1.0)
    f = eng.upload_fields(g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"], g["rr"] < 0,
                          g["vy"], csize_au=jm.csize, dtype=8)
    assert f.em0 is None and f.a0 is None
    jm._dev = f
    times = np.array([0.6, 1.1, 2.2]) * YEAR
    freqs = np.array([5e9, 4e10])
    flux, jac = jm.flux_vs_time_jac(times, freqs, formal=True)
    assert np.array_equal(flux, jm.flux_vs_time(times, freqs, formal=True))
    assert np.isfinite(jac).all() and (np.abs(jac).max(axis=(0, 1)) > 0).all()
    with pytest.raises(ValueError, match="tau layout"):
        jm.flux_vs_time_jac(times, freqs)


# ---- 7: thick sightlines ---------------------------------------------------------------------------
def test_thick_sightlines(eng):
    """ctau scaled so that the median sightline has tau = 600 / 1000 at chi = 1 (more inside a
    burst): every output is finite where the reference is, and inside the bound -- no special
    regime, the terms are dominated by the front cells."""
    name, shape, seed, E, F, bs = R.THICK
    g = R.synth_fields(shape, seed, narrow=True)
    f, arrays = upload(eng, g)
    ctau, csrc = R.channel_tables(R.host_a0(g), F, R.THICK_TAU)
    out, refs = check(eng, f, arrays, R.burst_set(bs), R.epochs(seed, E), ctau, csrc, what=name)
    tau = np.stack([r["tau"] for r in refs.values()]).astype(np.float64)
    assert np.median(tau[tau > 0]) > 500 and tau.max() > 1400
    hot = np.broadcast_to(next(iter(refs.values()))["hot"].ravel(), out[2].shape)
    assert np.isfinite(out[2][hot]).all() and np.isfinite(out[1]).all()


# ---- 8: workspace and refusals ---------------------------------------------------------------------
def test_workspace_of_exactly_the_stated_size_and_an_untouched_guard_band(eng):
    import torch
    from rajepy_amd import engine as E, _lib
    c = case(eng, "example-E17-F5")
    f, b = c["f"], E.make_bursts(*c["bursts"])
    nx, ny, nz = f.shape
    nE, F, npar = len(c["epochs"]), len(c["ctau"]), 15
    wb = eng.lib.rjp_ff_formal_grad_workspace(nx, ny, nz, nE, npar, F)
    assert wb > 0
    guard = 1 << 16
    buf = torch.full((wb + guard,), 0xA5, dtype=torch.uint8, device=eng.device)
    ftot = torch.full((nE, F), -7.0, dtype=torch.float64, device=eng.device)
    dftot = torch.full((nE, F, npar), -7.0, dtype=torch.float64, device=eng.device)
    assert raw(eng, f, b, c["epochs"], 0, c["ctau"], c["csrc"], ftot, dftot, None, work=buf,
               nbytes=wb) == _lib.RJP_OK
    eng.synchronize()
    assert bool((buf[wb:] == 0xA5).all())
    want = eng.ff_formal_grad(f, b, c["epochs"], 0, c["ctau"], c["csrc"])
    assert torch.equal(ftot, want[0]) and torch.equal(dftot, want[1])
    assert raw(eng, f, b, c["epochs"], 0, c["ctau"], c["csrc"], ftot, dftot, None, work=buf,
               nbytes=wb - 1) == _lib.RJP_ERR_WORKSPACE


def test_refusals_leave_poisoned_outputs_untouched(eng):
    import torch
    from rajepy_amd import engine as E, _lib
    c = case(eng, "example-E17-F5")
    f, good = c["f"], E.make_bursts(*c["bursts"])
    ctau, csrc, epochs = c["ctau"], c["csrc"], c["epochs"][:5]
    P, F, npar = f.npix, len(ctau), 48
    mk = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device=eng.device)
    outs = [mk(5, F), mk(5, F, npar), mk(5, F, npar, P)]
    ex = U.example_burst_lists()
    nine = E.make_bursts([(0.1 * i * YEAR, 1.0, 0.2 * YEAR) for i in range(9)], ex[1])
    none = E.make_bursts([], [])
    bad = E.make_bursts([(float("inf"), 1.0, 0.2 * YEAR)], [])
    full = E.make_bursts(*R.burst_set("full"))
    g32 = R.synth_fields(f.shape, 9103)
    f32 = eng.upload_fields(g32["nd"], g32["xi"], g32["temp"], g32["ff"], g32["areas"], g32["ts"],
                            g32["rr"] < 0, g32["vy"], csize_au=0.5, dtype=4)
    no_ts = f.struct()
    no_ts.d_ts = None
    ARG, WS = _lib.RJP_ERR_ARG, _lib.RJP_ERR_WORKSPACE
    call = lambda b=good, ep=epochs, ff=f, o=outs, **kw: raw(eng, ff, b, ep, 0, ctau, csrc, *o, **kw)
    cases = [
        ("no burst at all", call(b=none), ARG),
        ("no burst struct", call(b=None), ARG),
        ("nine bursts in a jet", call(b=nine), ARG),
        ("a non-finite epoch", call(ep=epochs[:2] + [float("nan")] + epochs[3:]), ARG),
        ("an infinite epoch", call(ep=epochs[:2] + [float("inf")] + epochs[3:]), ARG),
        ("a non-finite burst parameter", call(b=bad), ARG),
        ("all three outputs NULL", call(o=[None, None, None]), ARG),
        ("n_epochs = 0", call(n_ep=0), ARG),
        ("n_epochs < 0", call(n_ep=-2), ARG),
        ("n_chan = 0", call(n_ch=0), ARG),
        ("n_chan < 0", call(n_ch=-1), ARG),
        ("E F n_par beyond 2^31 - 1", call(b=full, n_ch=9000000), ARG),
        ("f32 fields", call(ff=f32), ARG),
        ("bursts without d_ts", call(fs=no_ts), ARG),
        ("a bad gff_mode", raw(eng, f, good, epochs, 7, ctau, csrc, *outs), ARG),
        ("a short workspace", call(nbytes=eng.lib.rjp_ff_formal_grad_workspace(
            *f.shape, 5, 15, F) - 1), WS),
        ("no workspace", call(nbytes=0), WS),
    ]
    eng.synchronize()
    for what, st, want in cases:
        assert st == want, (what, st)
    for o in outs:
        assert bool((o == 7.0).all())
    msg = eng.lib.rjp_last_error(eng.ctx)
    assert msg and len(msg) > 10
    # the context still serves a valid call; the maps alone need no workspace
    assert raw(eng, f, good, epochs, 0, ctau, csrc, None, None, outs[2][:, :, :15].contiguous(),
               nbytes=0) == _lib.RJP_OK
    assert call() == _lib.RJP_OK
    eng.synchronize()
    assert not bool((outs[0] == 7.0).any())
    with pytest.raises(_lib.RjprtError):
        eng.ff_formal_grad(f, none, epochs, 0, ctau, csrc)
