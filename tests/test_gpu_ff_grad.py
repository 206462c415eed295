"""rjp_ff_grad (K7: ff_grad_kernel, grad_reduce_kernel, ff_grad_totals_kernel, ff_grad_sum_kernel;
ff_grad.hip) through the C-ABI against tests/ff_grad_ref.py, a long-double NumPy restatement that
tests/test_ff_grad_reference_cpu.py pins to ref_single_epoch, to Richardson differences of it and to
hand-worked cases.

Bounds (derived, not measured).  Maps: |got - ref| <= (GAUSS_RTOL + n_y 2^-53) sum_y |term| per
pixel, for S and every derivative plane -- relative to the sum of the ABSOLUTE terms, since the t0
plane has terms of both signs; GAUSS_RTOL = 3e-12 is the project's figure for scans that keep the
Gaussians (degree-8 exp2, gpu_util).  Totals: against the long-double reduction of the reference
maps, |got - ref| <= (GAUSS_RTOL (1 + max tau) + (n_y + P) 2^-53) x the corresponding absolute sum
(sum_p |weight| sum_y |term|; the weight e^-tau carries tau times the relative error of S).
No pixel is excluded; zero and NaN patterns must be the reference's.  The module prints the worst
ratio to its bound per plane kind."""
import copy
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import ff_grad_ref as R
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
YEAR = orc.YEAR
EPOCHS = [t * YEAR for t in R.EPOCHS_YR]
WORST = {}                                  # plane kind -> worst |got - ref| / bound seen


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()
    print("\nworst |got - ref| / bound per plane kind: " +
          ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def upload(eng, a0, ts, bounds=False):
    """DeviceFields holding only the tau layout (a0, ts) of host arrays [n_x, n_y, n_z]."""
    import torch
    from rajepy_amd import engine as E
    dev = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device, dt)
    f = E.DeviceFields(a0.shape, E.RJP_F64, 0.5, None, None, None, None, ts=dev(ts.ravel()))
    f.a0, f.a0_mode = dev(a0.ravel()), E.RJP_GFF_SCALAR
    if bounds:
        # the occupied y-range per sightline: rows outside hold only cells that cannot contribute
        live = ~np.isnan(a0)
        any_ = live.any(axis=1)
        ny = a0.shape[1]
        lo = np.where(any_, live.argmax(axis=1), ny)
        hi = np.where(any_, ny - live[:, ::-1, :].argmax(axis=1), 0)
        f.ylo, f.yhi = dev(lo.ravel(), torch.int32), dev(hi.ravel(), torch.int32)
    return f


def channels(S, nf):
    """(ctau, cflux) for nf channels whose largest optical depth on the map S runs from 1e-3 to
    a few (3.2)."""
    top = float(S.max()) if (S > 0).any() else 1.0
    tau = np.logspace(-3, 0.5, nf) if nf > 1 else np.array([0.3])
    return tau / top, 1e-3 * (1.0 + np.arange(nf))


def note(kind, got, ref, absref, bound):
    """Zero / NaN patterns of the reference, |got - ref| <= bound * absref everywhere."""
    got = np.asarray(got, dtype=np.float64)
    r64 = np.asarray(ref, dtype=np.float64)
    assert got.shape == r64.shape, (kind, got.shape, r64.shape)
    assert not np.isnan(r64).any()
    assert np.array_equal(np.isnan(got), np.isnan(r64)), kind
    assert np.array_equal(got == 0, r64 == 0), kind
    err = np.abs(got.astype(R.LD) - np.asarray(ref, dtype=R.LD)).astype(np.float64)
    lim = bound * np.asarray(absref, dtype=np.float64)
    pos = lim > 0
    ratio = float((err[pos] / lim[pos]).max()) if pos.any() else 0.0
    WORST[kind] = max(WORST.get(kind, 0.0), ratio)
    print("%-8s worst |got - ref| / bound = %.3f" % (kind, ratio))
    assert ratio <= 1.0, (kind, ratio)
    assert np.all(err[~pos] == 0), kind


KINDS = ("dS/dt0", "dS/damp", "dS/dinv")


def check(eng, a0, ts, bursts, epochs, nf=0, bounds=False, nan_tavg=True, cover=False,
          thick=None):
    """One rjp_ff_grad call with every output against the reference; -> the device tensors."""
    from rajepy_amd import engine as E
    import torch
    shape = a0.shape
    nx, ny, nz = shape
    P = nx * nz
    refs = [R.planes(a0, ts, bursts, t) for t in epochs]
    tavg = ctau = cflux = None
    if nf:
        rng = np.random.default_rng(P + nf)
        tav = 5e3 + 1.5e4 * rng.random(P)
        if nan_tavg:
            tav[rng.integers(0, P, max(1, P // 16))] = np.nan       # empty sightlines' T_avg
        tavg = torch.from_numpy(tav).to(eng.device)
        ctau, cflux = channels(np.max([r["S"].astype(np.float64) for r in refs], axis=0), nf)
        if thick is not None:
            # every pixel optically thick: ctau so that the THINNEST sightline has these depths
            low = min(float(r["S"][r["S"] > 0].min()) for r in refs)
            ctau = np.asarray(thick, dtype=np.float64) / low
    f = upload(eng, a0, ts, bounds)
    sumA, dsumA, ftot, dftot = eng.ff_grad(f, E.make_bursts(*bursts), epochs, E.RJP_GFF_SCALAR,
                                           tavg, ctau, cflux, want_maps=True)
    eng.synchronize()
    mb = R.map_bound(ny, U.GAUSS_RTOL)
    S, D = sumA.cpu().numpy(), dsumA.cpu().numpy()
    npar = 3 * (len(bursts[0]) + len(bursts[1]))
    assert D.shape == (len(epochs), npar, P)
    for e, ref in enumerate(refs):
        note("S", S[e], ref["S"].ravel(), ref["absS"].ravel(), mb)
        for c in range(3):
            note(KINDS[c], D[e, c::3], ref["D"][c::3].reshape(-1, P),
                 ref["absD"][c::3].reshape(-1, P), mb)
        if cover:
            cov = [R.coverage(pl) for pl in ref["D"]]
            assert min(cov) >= R.MIN_COVER, (shape, e, cov)
        if nf:
            tot = R.totals(ref, tav, ctau, cflux)
            assert 1e-4 < tot["tau_max"] and (thick is not None or tot["tau_max"] < 10.0)
            tb = R.totals_bound(ny, P, tot["tau_max"], U.GAUSS_RTOL)
            note("F", ftot.cpu().numpy()[e], tot["F"], tot["absF"], tb)
            note("dF", dftot.cpu().numpy()[e], tot["dF"], tot["absdF"], tb)
    return f, (sumA, dsumA, ftot, dftot), (tavg, ctau, cflux)


EX = U.example_burst_lists()                 # 2 red, 3 blue
ONE = ([EX[0][0]], [EX[1][2]])               # one burst per jet: 1 slot, tiles of 4 epochs
TWO = (EX[0], EX[1][:2])                     # two per jet: 2 slots, tiles of 4 epochs
FIVE = EPOCHS + [0.2 * YEAR, 1.9 * YEAR]


@pytest.mark.parametrize("shape", R.COVER_SHAPES, ids=["3x37x50", "5x19x33"])
def test_example_bursts_three_epochs(eng, shape):
    """P = 150 (no multiple of 64, straddling waves, y-split) and an odd n_z (the 1-wide lane
    path): every plane is non-trivial on >= 40 % of the sightlines; 17 channels, a NaN T_avg."""
    a0, ts = R.synth_a0_ts(shape, R.SEED, "halves")
    check(eng, a0, ts, EX, EPOCHS, nf=17, cover=True)


@pytest.mark.parametrize("shape,bursts,epochs,flags,nf", [
    ((2, 1, 64), EX, EPOCHS[1:2], "halves", 1),          # one term per sum; n_y below the row unroll
    ((2, 3, 64), EX, EPOCHS[:1], "cells", 1),            # n_y just above the row unroll
    ((9, 18, 80), EX, FIVE, "cells", 17),                # several blocks; both jets per sightline; E = 5
    ((2, 9, 512), EX, EPOCHS, "halves", 1),              # waves all red and all blue
    ((2, 9, 512), ONE, FIVE, "halves", 0),               # 1 slot: tiles 4 + 1, 2-wide lanes
    ((5, 19, 33), ONE, FIVE, "cells", 1),                # ... 1-wide lanes
    ((2, 9, 512), TWO, EPOCHS, "cells", 1),              # 2 slots: tiles 2 + 1
    ((3, 37, 50), TWO, FIVE, "halves", 0),               # ... 4 + 1, 1-wide lanes (tile of 4)
    ((3, 37, 50), EX, EPOCHS[:1], "red", 1),             # one jet everywhere
    ((3, 37, 50), EX, EPOCHS[:1], "blue", 1),
], ids=["2x1x64", "2x3x64", "9x18x80-cells-E5", "2x9x512", "one-E5-vec2", "one-E5-vec1", "two-E3",
        "two-E5", "all-red", "all-blue"])
def test_shapes_tiles_and_jets(eng, shape, bursts, epochs, flags, nf):
    a0, ts = R.synth_a0_ts(shape, R.SEED + 1, flags)
    check(eng, a0, ts, bursts, epochs, nf=nf)


def test_thick_maps_weights_below_the_smallest_double(eng):
    """Every sightline at tau >= 650 / 720 / 900: the weights e^-tau of the Jacobian run from 1e-283
    down past the smallest double, the derivative sums are ~1e20 and larger, and the totals are
    still judged relative to their own (tiny) absolute sums -- no clamp of e^-tau may show."""
    a0, ts = R.synth_a0_ts((3, 37, 50), R.SEED + 5, "halves")
    check(eng, a0, ts, EX, EPOCHS, nf=3, thick=(650.0, 720.0, 900.0))


@pytest.mark.parametrize("only", [0, 1], ids=["red-only", "blue-only"])
def test_bursts_in_one_jet_nan_launch_times_in_the_other(eng, only):
    """The jet without bursts has chi = 1 whatever its launch times: its cells -- a third of them
    with a NaN launch time -- add |a0| to S; NaN launch times in the jet WITH bursts drop the cell."""
    shape = (3, 37, 50)
    a0, ts = R.synth_a0_ts(shape, R.SEED + 2, "cells")
    rng = np.random.default_rng(5)
    other = np.signbit(a0) == (only == 1)                # cells of the jet without bursts
    ts[other & (rng.random(shape) < 1 / 3)] = np.nan
    ts[~other & (rng.random(shape) < 0.1)] = np.nan
    bursts = (EX[0], []) if only == 0 else ([], EX[1])
    check(eng, a0, ts, bursts, EPOCHS, nf=17)


def test_eight_bursts_and_a_negative_amplitude(eng):
    rng = np.random.default_rng(8)
    red = [(rng.uniform(0.0, 2.5) * YEAR, rng.uniform(0.5, 8.0), rng.uniform(0.1, 0.6) * YEAR)
           for _ in range(8)]
    red[3] = (red[3][0], -0.6, red[3][2])                # a dip
    a0, ts = R.synth_a0_ts((5, 19, 33), R.SEED + 3, "cells")
    check(eng, a0, ts, (red, EX[1]), EPOCHS, nf=17)
    a0, ts = R.synth_a0_ts((2, 9, 512), R.SEED + 3, "halves")
    check(eng, a0, ts, (EX[1], red), EPOCHS[:2], nf=1)


def test_y_bounds_empty_sightlines_and_nan_cells(eng):
    """d_ylo / d_yhi attached: sightlines occupied over a part of y only, some empty ([n_y, 0)),
    NaN a0 cells inside the occupied range as well."""
    shape = (9, 18, 80)
    a0, ts = R.synth_a0_ts(shape, R.SEED + 4, "halves")
    rng = np.random.default_rng(11)
    lo = rng.integers(0, 10, (shape[0], shape[2]))
    hi = lo + rng.integers(0, 9, (shape[0], shape[2]))   # hi == lo: an empty sightline
    y = np.arange(shape[1])[None, :, None]
    a0[(y < lo[:, None, :]) | (y >= hi[:, None, :])] = np.nan
    a0[rng.random(shape) < 0.05] = np.nan
    assert (np.isnan(a0).all(axis=1)).sum() > 20
    f, out, _ = check(eng, a0, ts, EX, EPOCHS, nf=17, bounds=True)
    # ... and the same numbers without the bounds attached, bit for bit
    _, out2, _ = check(eng, a0, ts, EX, EPOCHS, nf=17, bounds=False)
    for a, b in zip(out, out2):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


# ---- the C-ABI directly: NULL outputs, refusals ----------------------------------------------
def raw_call(eng, f, bursts, epochs, tavg, ctau, cflux, outs, short=False, mode=0, nchan=None):
    from rajepy_amd import _lib
    nx, ny, nz = f.shape
    npar = 3 * (int(bursts.n[0]) + int(bursts.n[1])) if bursts is not None else 0
    nf = (len(ctau) if ctau is not None else 0) if nchan is None else nchan
    need = eng.lib.rjp_ff_grad_workspace(nx, ny, nz, len(epochs), max(npar, 3), nf)
    work = eng._workspace(max(need, 1 << 20))
    fs = f.struct()
    ptr = lambda t: t.data_ptr() if t is not None else None
    return eng.lib.rjp_ff_grad(
        eng.ctx, C.byref(fs), C.byref(bursts) if bursts is not None else None,
        _lib.dbl_array(epochs), len(epochs), mode, ptr(tavg),
        _lib.dbl_array(ctau) if ctau is not None else None,
        _lib.dbl_array(cflux) if cflux is not None else None, nf, *[ptr(o) for o in outs],
        work.data_ptr(), need - 1 if short else need, eng._stream()), need


def test_null_output_combinations_and_reproducibility(eng):
    import torch
    from rajepy_amd import engine as E
    a0, ts = R.synth_a0_ts((3, 37, 50), R.SEED, "halves")
    f, full, (tavg, ctau, cflux) = check(eng, a0, ts, EX, EPOCHS, nf=17)
    full = [t.clone() for t in full]
    b = E.make_bursts(*EX)
    for mask in itertools.product((False, True), repeat=4):
        outs = [torch.full_like(t, -7.0) if m else None for t, m in zip(full, mask)]
        st, _ = raw_call(eng, f, b, EPOCHS, tavg, ctau, cflux, outs)
        eng.synchronize()
        if not any(mask):
            assert st == E._lib.RJP_ERR_ARG
            continue
        assert st == 0, (mask, eng.lib.rjp_last_error(eng.ctx))
        for o, want in zip(outs, full):          # fixed summation order: bit for bit, run to run
            if o is not None:
                assert torch.equal(o, want), mask
    # maps only: no channel tables, no T_avg, n_chan = 0
    outs = [torch.full_like(full[0], -7.0), torch.full_like(full[1], -7.0), None, None]
    st, _ = raw_call(eng, f, b, EPOCHS, None, None, None, outs)
    eng.synchronize()
    assert st == 0 and torch.equal(outs[0], full[0]) and torch.equal(outs[1], full[1])


def test_refusals_enqueue_nothing(eng):
    import torch
    from rajepy_amd import engine as E, _lib
    a0, ts = R.synth_a0_ts((3, 37, 50), R.SEED, "halves")
    f = upload(eng, a0, ts)
    good = E.make_bursts(*EX)
    P, nf = f.npix, 3
    tavg = torch.full((P,), 1e4, dtype=torch.float64, device=eng.device)
    ctau, cflux = channels(R.planes(a0, ts, EX, EPOCHS[0])["S"].astype(np.float64), nf)

    def outs_for(b, E_):
        npar = max(3, 3 * (int(b.n[0]) + int(b.n[1]))) if b is not None else 3
        mk = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device=eng.device)
        return [mk(E_, P), mk(E_, npar, P), mk(E_, nf), mk(E_, nf, npar)]

    nine = E.make_bursts([(0.1 * i * YEAR, 1.0, 0.2 * YEAR) for i in range(9)], EX[1])
    none = E.make_bursts([], [])
    bad = E.make_bursts([(float("inf"), 1.0, 0.2 * YEAR)], [])
    wrong_mode = copy.copy(f)
    wrong_mode.a0_mode = E.RJP_GFF_POWERLAW
    cases = [
        ("nine bursts in a jet", f, nine, EPOCHS, {}, _lib.RJP_ERR_ARG),
        ("no bursts", f, none, EPOCHS, {}, _lib.RJP_ERR_ARG),
        ("no bursts struct", f, None, EPOCHS, {}, _lib.RJP_ERR_ARG),
        ("a non-finite epoch", f, good, [EPOCHS[0], float("nan")], {}, _lib.RJP_ERR_ARG),
        ("a non-finite burst parameter", f, bad, EPOCHS, {}, _lib.RJP_ERR_ARG),
        ("a short workspace", f, good, EPOCHS, {"short": True}, _lib.RJP_ERR_WORKSPACE),
        ("a0_mode != gff_mode", wrong_mode, good, EPOCHS, {}, _lib.RJP_ERR_ARG),
        ("all outputs NULL", f, good, EPOCHS, {"null": True}, _lib.RJP_ERR_ARG),
        ("totals without tables", f, good, EPOCHS, {"notab": True}, _lib.RJP_ERR_ARG),
    ]
    for what, ff, b, ep, kw, want in cases:
        outs = outs_for(b, len(ep))
        passed = [None] * 4 if kw.get("null") else outs
        tabs = (None, None, None) if kw.get("notab") else (tavg, ctau, cflux)
        st, _ = raw_call(eng, ff, b, ep, *tabs, passed, short=bool(kw.get("short")),
                         nchan=nf if kw.get("notab") else None)
        eng.synchronize()
        assert st == want, (what, st)
        msg = eng.lib.rjp_last_error(eng.ctx)
        assert msg and len(msg) > 10, what
        for o in outs:
            assert bool((o == -7.0).all()), what          # nothing was written
        # the context still serves a valid call
        outs = outs_for(good, len(EPOCHS))
        st, _ = raw_call(eng, f, good, EPOCHS, tavg, ctau, cflux, outs)
        eng.synchronize()
        assert st == 0, (what, eng.lib.rjp_last_error(eng.ctx))
        assert not bool((outs[0] == -7.0).any()) and not bool((outs[3] == -7.0).any())
    with pytest.raises(_lib.RjprtError):
        eng.ff_grad(f, none, EPOCHS, E.RJP_GFF_SCALAR)


# ---- the model level ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(tmp_path_factory, eng):
    from rajepy_amd import classes, logger
    p = copy.deepcopy(U.load_golden("cfg1_example")[2])
    p["ejection"] = U.example_bursts_params()
    log = logger.Log(str(tmp_path_factory.mktemp("k7") / "m.log"), verbose=False)
    return classes.JetModel(p, log=log, engine=eng), p, log


def test_model_jacobians(model, eng):
    """cfg1_example through JetModel.flux_vs_time_jac / optical_depth_ff_jac against the helper run
    on a0, ts and T_avg read back from the device (K4 and rjp_tavg wrote them, not the code under
    test), the host chain rule applied; axis order against model.ejections."""
    from rajepy_amd import classes, engine as E
    jm, p, _ = model
    freqs = np.array([1e9, 5e9, 5e10])
    flux, jac = jm.flux_vs_time_jac(EPOCHS, freqs)
    dev = jm.device_fields
    shape = (jm.nx, jm.ny, jm.nz)
    a0 = dev.a0.cpu().numpy().reshape(shape)
    ts = dev.ts.cpu().numpy().reshape(shape)
    tavg = jm._model_tavg().cpu().numpy()
    bursts = (jm._bursts["R"], jm._bursts["B"])
    _, (ctau, cflux) = jm._channel_coeffs(freqs)
    ej = list(jm.ejections.values())
    assert jac.shape == (3, 3, len(ej), 3) and flux.shape == (3, 3) and len(ej) == 5
    # model.ejections order -> kernel plane: the red jet's bursts first
    order, seen = [], {"R": 0, "B": 0}
    for e_ in ej:
        order.append(seen[e_["which"]] + (len(bursts[0]) if e_["which"] == "B" else 0))
        seen[e_["which"]] += 1
    chain = np.array([classes.ejection_chain_rule(e_["t_0"], e_["peak_jml"], e_["half_life"],
                                                  jm.ss_jml(e_["which"]))[1] for e_ in ej])
    lc = jm.flux_vs_time(EPOCHS, freqs)
    P = jm.nx * jm.nz
    for e, t in enumerate(EPOCHS):
        ref = R.planes(a0, ts, bursts, t)
        tot = R.totals(ref, tavg, ctau, cflux)
        tb = R.totals_bound(jm.ny, P, tot["tau_max"], U.GAUSS_RTOL)
        idx = np.array([[3 * b + c for c in range(3)] for b in order])        # [n_ej, 3]
        note("F", flux[e], tot["F"], tot["absF"], tb)
        note("F", lc[e], tot["F"], tot["absF"], tb)                           # flux_vs_time itself
        # (one more rounding on the host: the product with the chain factor)
        note("dF", jac[e], tot["dF"][:, idx] * chain[None],
             tot["absdF"][:, idx] * np.abs(chain[None]), tb + R.EPS)
        if abs(t - EPOCHS[1]) < 1:
            jm.time = t
            dtau = jm.optical_depth_ff_jac(freqs)
            assert dtau.shape == (len(ej), 3, 3, jm.nx, jm.nz)
            mb = R.map_bound(jm.ny, U.GAUSS_RTOL)
            for i, b in enumerate(order):
                for c in range(3):
                    for f_ in range(3):
                        s = ctau[f_] * chain[i, c]
                        # (two more roundings on the host: the products with ctau and the chain factor)
                        note(KINDS[c], dtau[i, c, f_], s * ref["D"][3 * b + c],
                             abs(s) * ref["absD"][3 * b + c], mb + 2 * R.EPS)
    assert np.isfinite(jac).all() and (np.abs(jac).max(axis=(0, 1)) > 0).all()


def test_model_without_ejections_and_f32(model, eng):
    from rajepy_amd import classes
    _, p, log = model
    q = copy.deepcopy(p)
    q["ejection"] = {"t_0": np.array([]), "hl": np.array([]), "chi": np.array([]),
                     "which": np.array([])}
    jm = classes.JetModel(q, log=log, engine=eng)
    freqs = np.array([1e9, 5e10])
    flux, jac = jm.flux_vs_time_jac(EPOCHS[:2], freqs)
    assert jac.shape == (2, 2, 0, 3) and flux.shape == (2, 2)
    np.testing.assert_allclose(flux, jm.flux_vs_time(EPOCHS[:2], freqs), rtol=1e-12)
    assert jm.optical_depth_ff_jac(freqs).shape == (0, 3, 2, jm.nx, jm.nz)
    f32 = classes.JetModel(copy.deepcopy(p), log=log, engine=eng, storage="f32")
    with pytest.raises(ValueError, match="f64 storage"):
        f32.flux_vs_time_jac(EPOCHS, freqs)
    with pytest.raises(ValueError, match="tau layout"):
        f32.optical_depth_ff_jac(freqs)
