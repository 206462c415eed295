"""The reference of the formal-solution sensitivities (tests/ff_formal_grad_ref.py, for
rjp_ff_formal_grad, K9) held to NumPy's formal solution, to K7's reference in the isothermal limit,
to Richardson-extrapolated central differences of its own I and to hand-worked cells; the
non-vacuity of the cases tests/test_gpu_ff_formal_grad.py runs; the ABI, the workspace query and the
Python path of JetModel.flux_vs_time_jac(formal=True) with a recording engine; and the power of the
bound itself on planted mistakes.  No GPU."""
import copy
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import rt_oracle as orc
from tests import ff_formal_grad_ref as R
from tests import ff_grad_ref as R7
from tests import gpu_util as U
from tests.test_gpu_formal_rt import _coeffs, np_formal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YEAR = orc.YEAR


def _oracle_burst_lists(jet):
    out = []
    for which, ss in (("R", jet._ss_jml_rj), ("B", jet._ss_jml_bj)):
        out.append([(t0, (peak - ss) / ss, hl * 2. / (2. * np.sqrt(2. * np.log(2.))))
                    for t0, peak, hl in jet.bursts[which]])
    return out[0], out[1]


def _synth(shape, seed, F, bs):
    g = R.synth_fields(shape, seed)
    a0 = R.host_a0(g)
    ctau, csrc = R.channel_tables(a0, F)
    return g, a0, ctau, csrc, R.burst_set(bs)


# ---- I of the reference ---------------------------------------------------------------------------
def test_reference_intensity_is_numpys_formal_solution_random_grid():
    shape = (4, 41, 23)
    g, a0, ctau, csrc, bursts = _synth(shape, 4711, 3, "example")
    for t in (0.8 * YEAR, 1.7 * YEAR):
        res = R.walk(a0, g["ts"], g["temp"], bursts, t, ctau, csrc)
        b = R.cells(a0, g["ts"], bursts, t)[0].astype(np.float64)
        want = np_formal(np.asarray(ctau)[:, None, None, None] * b[None], g["temp"], csrc)
        got = res["I"].astype(np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any()
        assert (got[np.isfinite(got)] > 0).any()
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=0)


def test_reference_intensity_on_the_tilted_golden_model():
    """tests/golden/tilted: the same per-cell depths through np_formal to 1e-13, and the oracle's
    own per-cell optical depths to 1e-11 (K5's bound against them)."""
    z, meta, p, g, jet = U.golden_dense("tilted")
    freqs = np.asarray(z["freqs"], dtype=np.float64)
    mode, ctau, cflux = _coeffs(jet, freqs)
    a0 = U.golden_a0(g, p["power_laws"]["q_T"])
    bursts = _oracle_burst_lists(jet)
    assert len(bursts[0]) and len(bursts[1])
    jet.time = float(z["years"][1]) * YEAR
    res = R.walk(a0, g["ts"], g["temp"], bursts, jet.time, ctau, cflux)
    got = res["I"].astype(np.float64)
    b = R.cells(a0, g["ts"], bursts, jet.time)[0].astype(np.float64)
    same = np_formal(np.asarray(ctau)[:, None, None, None] * b[None], g["temp"], cflux)
    np.testing.assert_allclose(got, same, rtol=1e-13, atol=0)
    with np.errstate(all="ignore"):
        want = np_formal(jet.optical_depth_ff(freqs, collapse=False), jet.temperature, cflux)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=1e-11, atol=0)
    assert np.isfinite(res["dI"]).any() and (np.abs(np.nan_to_num(res["dI"].astype(np.float64))) > 0).any()


# ---- the isothermal limit: K7's formula ----------------------------------------------------------
def test_isothermal_limit_is_k7s_formula():
    """cfg1_example (constant T): the sum collapses to csrc T ctau e^-tau dS/dtheta_k with dS from
    ff_grad_ref.planes -- to 1e-12 of abs_k."""
    z, meta, p, g, jet = U.golden_dense("cfg1_example")
    freqs = np.asarray(z["freqs"], dtype=np.float64)
    mode, ctau, cflux = _coeffs(jet, freqs)
    # (the six x-rows that hold the most cells: the walk is per sightline)
    rows = np.sort(np.argsort(np.isfinite(g["nd"]).sum(axis=(1, 2)))[-6:])
    a0, ts, temp = U.golden_a0(g, 0.0)[rows], g["ts"][rows], g["temp"][rows]
    bursts = _oracle_burst_lists(jet)
    T0 = float(np.nanmax(temp))
    assert np.all((temp == T0) | np.isnan(temp))
    worst = 0.0
    for yr in z["years"][1:3]:
        t = float(yr) * YEAR
        res = R.walk(a0, ts, temp, bursts, t, ctau, cflux)
        k7 = R7.planes(a0, ts, bursts, t)
        for f in range(len(freqs)):
            tau = R.LD(ctau[f]) * k7["S"]
            want = R.LD(cflux[f]) * R.LD(T0) * R.LD(ctau[f]) * np.exp(-tau)[None] * k7["D"]
            hot = res["hot"]
            err = np.abs(res["dI"][f][:, hot] - want[:, hot])
            ab = res["abs"][f][:, hot]
            pos = ab > 0
            assert pos.any() and np.all(err[~pos] == 0)
            worst = max(worst, float((err[pos] / ab[pos]).max()))
    print("isothermal limit: worst |dI - K7's formula| / abs = %.2e" % worst)
    assert worst <= 1e-12


# ---- finite differences --------------------------------------------------------------------------
def _perturbed(bursts, b, c, rel):
    out = [list(bursts[0]), list(bursts[1])]
    j, i = (0, b) if b < len(bursts[0]) else (1, b - len(bursts[0]))
    t0, amp, sg = out[j][i]
    k = 1.0 / (2.0 * sg ** 2)
    if c == 0:
        step = rel * sg
        out[j][i] = (t0 + step, amp, sg)
    elif c == 1:
        step = rel * amp
        out[j][i] = (t0, amp + step, sg)
    else:
        step = rel * k
        out[j][i] = (t0, amp, math.sqrt(1.0 / (2.0 * (k + step))))
    return out, step


@pytest.mark.parametrize("shape", R.SHAPES, ids=["3x37x50", "5x19x33"])
def test_planes_against_richardson_differences_of_the_references_own_intensity(shape):
    """Every plane against (4 D(h / 2) - D(h)) / 3 of central differences of the reference's I at
    relative steps 1e-3 and 5e-4 (of sigma for t0), judged where |ref| >= 1e-3 abs_k (a burst
    whose Gaussian is ~1e-29 at every cell cannot be differenced): <= 1e-9 of the plane's largest
    value, K7's bar -- the h^4 term that is left.  Measured worst: 6.7e-13 (3x37x50) and 7.6e-13
    (5x19x33), 1300 x inside."""
    g, a0, ctau, csrc, bursts = _synth(shape, 5150, 2, "example")
    t = 1.3 * YEAR
    ref = R.walk(a0, g["ts"], g["temp"], bursts, t, ctau, csrc)
    hot = ref["hot"]
    I = lambda bl: R.walk(a0, g["ts"], g["temp"], bl, t, ctau, csrc)["I"][:, hot]
    nb = len(bursts[0]) + len(bursts[1])
    worst, judged = 0.0, 0
    for b in range(nb):
        for c in range(3):
            est = []
            for rel in (1e-3, 5e-4):
                up, step = _perturbed(bursts, b, c, +rel)
                dn, _ = _perturbed(bursts, b, c, -rel)
                est.append((I(up) - I(dn)) / R.LD(2.0 * step))
            rich = (4.0 * est[1] - est[0]) / 3.0
            got, ab = ref["dI"][:, 3 * b + c][:, hot], ref["abs"][:, 3 * b + c][:, hot]
            sel = np.abs(got) >= 1e-3 * ab
            sel &= ab > 0
            assert sel.any(), (b, c)
            judged += int(sel.sum())
            scale = np.abs(got).max()
            err = float((np.abs(got - rich)[sel]).max() / scale)
            worst = max(worst, err)
            assert err <= 1e-9, (b, c, err)
    print("worst plane against Richardson differences: %.2e of its largest value (%d entries)"
          % (worst, judged))


# ---- hand-worked cells ---------------------------------------------------------------------------
def test_two_cells_on_one_sightline():
    """Front cell red with one red burst, back cell blue with one blue burst.  dI/damp of the front
    burst = c [T_f e^-dtau_f - T_b om_b e^-dtau_f] g_f: negative with a colder front cell and a
    thick back cell, positive with a hotter one; the back burst's is c T_b e^-dtau_f e^-dtau_b g_b,
    always positive."""
    t, c, cs = 1.2, 0.7, 1.0
    rb, bb = (1.0, 3.0, 0.5), (0.9, 1.5, 0.4)
    a_f, a_b, ts_f, ts_b = -0.4, 2.5, 0.3, 0.1

    def one(T_f, T_b):
        a0 = np.array([[[a_f], [a_b]]])
        ts = np.array([[[ts_f], [ts_b]]])
        temp = np.array([[[T_f], [T_b]]])
        r = R.walk(a0, ts, temp, ([rb], [bb]), t, [c], [cs])
        return [float(v) for v in r["dI"][0, :, 0, 0]], [float(v) for v in r["abs"][0, :, 0, 0]], \
            float(r["I"][0, 0, 0])

    def cell(a, ts, burst):
        t0, amp, sg = burst
        k = 1.0 / (2.0 * sg ** 2)
        dd = (t - ts) - t0
        G = math.exp(-dd * dd * k)
        chi = 1.0 + amp * G
        return abs(a) * chi ** 2, abs(a) * 2 * chi * G

    b_f, g_f = cell(a_f, ts_f, rb)
    b_b, g_b = cell(a_b, ts_b, bb)
    e_f, e_b = math.exp(-c * b_f), math.exp(-c * b_b)
    for T_f, T_b in ((5e3, 2e4), (2e4, 5e3)):
        dI, ab, I = one(T_f, T_b)
        np.testing.assert_allclose(I, T_f * (1 - e_f) + T_b * (1 - e_b) * e_f, rtol=1e-14)
        front = c * (T_f * e_f - T_b * (1 - e_b) * e_f) * g_f
        back = c * T_b * e_f * e_b * g_b
        np.testing.assert_allclose(dI[1], front, rtol=1e-13)
        np.testing.assert_allclose(dI[4], back, rtol=1e-13)
        np.testing.assert_allclose(ab[1], c * (T_f * e_f + T_b * (1 - e_b) * e_f) * g_f, rtol=1e-13)
        np.testing.assert_allclose(ab[4], back, rtol=1e-13)
        assert (dI[1] < 0) == (T_f < T_b) and dI[1] != 0
        assert dI[4] > 0
        # the back cell's burst carries the factor e^-dtau_front: remove the front cell's opacity
        # (a -> tiny) and the plane grows by exactly that factor
    thin = R.walk(np.array([[[-1e-300], [a_b]]]), np.array([[[ts_f], [ts_b]]]),
                  np.array([[[5e3], [2e4]]]), ([rb], [bb]), t, [c], [cs])
    np.testing.assert_allclose(one(5e3, 2e4)[0][4], float(thin["dI"][0, 4, 0, 0]) * e_f, rtol=1e-13)
    # a burst of the other jet: the plane is an exact zero; a sightline without T > 0 is NaN
    r = R.walk(np.array([[[a_b], [a_b]]]), np.array([[[ts_f], [ts_b]]]), np.array([[[5e3], [2e4]]]),
               ([rb], [bb]), t, [c], [cs])
    assert np.all(r["dI"][0, :3] == 0) and np.all(r["abs"][0, :3] == 0) and r["dI"][0, 4, 0, 0] != 0
    r = R.walk(np.array([[[a_f], [a_b]]]), np.array([[[ts_f], [ts_b]]]),
               np.array([[[np.nan], [np.nan]]]), ([rb], [bb]), t, [c], [cs])
    assert np.isnan(r["I"]).all() and np.isnan(r["dI"]).all()
    # a jet without bursts: chi = 1 whatever its launch time, g = 0, and it still attenuates
    r1 = R.walk(np.array([[[a_f], [a_b]]]), np.array([[[np.nan], [ts_b]]]),
                np.array([[[5e3], [2e4]]]), ([], [bb]), t, [c], [cs])
    np.testing.assert_allclose(float(r1["dI"][0, 1, 0, 0]),
                               c * 2e4 * math.exp(-c * abs(a_f)) * e_b * g_b, rtol=1e-13)


# ---- the GPU cases are not vacuous ---------------------------------------------------------------
def _case_stats(shape, seed, E, F, bs, thick=False):
    g = R.synth_fields(shape, seed, narrow=thick)
    a0 = R.host_a0(g)
    bursts = R.burst_set(bs)
    eps = R.epochs(seed, E)[:8]          # (the first eight, the one outside every burst included)
    ctau, csrc = R.channel_tables(a0, F, R.THICK_TAU if thick else (0.1, 5.0))
    live = pos = big = 0
    signs = False
    seen = {}
    for te in eps:
        if te in seen:
            res = seen[te]
        else:
            res = seen[te] = R.walk(a0, g["ts"], g["temp"], bursts, te, ctau, csrc)
        h = np.broadcast_to(res["hot"][None, None], res["abs"].shape)
        ab, d = res["abs"][h], res["dI"][h]
        live += ab.size
        pos += int((ab > 0).sum())
        big += int((np.abs(d) >= 1e-3 * ab)[ab > 0].sum())
        dk = res["dI"][:, :, res["hot"]]
        signs |= bool(((dk > 0).any(axis=-1) & (dk < 0).any(axis=-1)).any())
    return pos / live, big / max(pos, 1), signs, seen[eps[min(1, len(eps) - 1)]]


@pytest.mark.parametrize("name", list(R.CASES))
def test_gpu_cases_are_not_vacuous(name):
    """For every random case of the GPU file (same seeds, same generator): at least 40 % of the
    live (pixel, plane) pairs have abs > 0, at least 40 % of those |ref| >= 1e-3 abs, and both
    signs occur in at least one plane -- over all channels and the first eight epochs of the case
    (the one far outside every burst, where every plane is zero, among them)."""
    shape, seed, E, F, bs, _ = R.CASES[name]
    share, big, signs, _ = _case_stats(shape, seed, E, F, bs)
    print("%s: abs > 0 on %.2f of the live pairs, |ref| >= 1e-3 abs on %.2f of those" %
          (name, share, big))
    assert share >= R.MIN_SHARE and big >= R.MIN_SHARE and signs


def test_thick_gpu_case_is_thick_and_not_vacuous():
    name, shape, seed, E, F, bs = R.THICK
    share, big, signs, res = _case_stats(shape, seed, E, F, bs, thick=True)
    tau = res["tau"][:, res["hot"]].astype(np.float64)          # at the epoch outside every burst
    tau = tau[tau > 0]
    med = np.median(tau)
    inside = np.mean((tau > 500) & (tau < 1400))
    print("thick: median tau %.0f, %.2f of the sightlines in (500, 1400)" % (med, inside))
    assert 500 < med < 1400 and inside >= 0.5
    assert share >= R.MIN_SHARE and big >= R.MIN_SHARE and signs


# ---- ABI -----------------------------------------------------------------------------------------
def test_header_symbols_and_argtypes():
    from rajepy_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    assert int(re.search(r"#define RJP_VERSION (\d+)", hdr).group(1)) == _lib.RJP_VERSION == 117
    assert "size_t rjp_ff_formal_grad_workspace(" in hdr and "int rjp_ff_formal_grad(" in hdr
    res, args = _lib.SIGNATURES["rjp_ff_formal_grad_workspace"]
    assert res is C.c_size_t and args == [C.c_int32] * 6
    res, args = _lib.SIGNATURES["rjp_ff_formal_grad"]
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    assert res is C.c_int
    assert args == [vp, C.POINTER(_lib.Fields), C.POINTER(_lib.Bursts), dp, C.c_int32, C.c_int32,
                    dp, dp, C.c_int32, vp, vp, vp, vp, C.c_size_t, vp]
    lib = _lib.load()
    assert lib.rjp_version() == 117
    assert lib.rjp_ff_formal_grad.argtypes == args
    assert lib.rjp_ff_formal_grad_workspace.restype is C.c_size_t


def test_workspace_query():
    from rajepy_amd import _lib
    ws = _lib.load().rjp_ff_formal_grad_workspace
    good = (4, 100, 37, 32, 15, 3)
    assert ws(*good) > 0
    for i in range(6):
        for bad in (0, -1):
            a = list(good)
            a[i] = bad
            assert ws(*a) == 0, a
    # one partial per (epoch, channel, parameter + 1, 16 sightlines of an x-row) at the least
    assert ws(*good) >= 4 * 3 * 32 * 3 * (15 + 1) * 8
    for axis, values in ((3, (1, 2, 15, 16, 17, 63, 64, 65, 130, 1000)), (5, (1, 2, 3, 4, 5, 8, 9, 300)),
                         (4, (3, 6, 9, 15, 24, 27, 48))):
        last = 0
        for v in values:
            a = list(good)
            a[axis] = v
            assert ws(*a) >= last
            last = ws(*a)
    assert ws(512, 4096, 512, 121, 48, 8) >= 512 * 32 * 121 * 8 * 49 * 8


# ---- the Python path -----------------------------------------------------------------------------
class _RecordingEngine:
    def __init__(self):
        self.calls = []

    def ff_formal_grad(self, fields, bursts, epochs_s, gff_mode, ctau, csrc, want_maps=False):
        E, F = len(epochs_s), len(ctau)
        n_par = 3 * (int(bursts.n[0]) + int(bursts.n[1]))
        self.calls.append(("ff_formal_grad", dict(fields=fields, epochs=list(epochs_s), mode=gff_mode,
                                                   ctau=np.array(ctau), csrc=np.array(csrc),
                                                   want_maps=want_maps, n=(bursts.n[0], bursts.n[1]))))
        ftot = torch.arange(E * F, dtype=torch.float64).reshape(E, F)
        dftot = 1.0 + torch.arange(E * F * n_par, dtype=torch.float64).reshape(E, F, n_par)
        return ftot, dftot, None

    def ff_grad(self, fields, bursts, epochs_s, gff_mode, tavg=None, ctau=None, cflux=None,
                want_maps=False):
        E, F = len(epochs_s), len(ctau)
        n_par = 3 * (int(bursts.n[0]) + int(bursts.n[1]))
        self.calls.append(("ff_grad", None))
        return None, None, torch.zeros(E, F, dtype=torch.float64), \
            torch.zeros(E, F, n_par, dtype=torch.float64)


def test_flux_vs_time_jac_formal_python_path(tmp_path):
    from rajepy_amd import _lib, classes, logger
    assert inspect.signature(classes.JetModel.flux_vs_time_jac).parameters["formal"].default is False
    p = copy.deepcopy(U.load_golden("cfg1_example")[2])
    p["ejection"] = U.example_bursts_params()
    log = logger.Log(str(tmp_path / "m.log"), verbose=False)
    rec = _RecordingEngine()
    jm = classes.JetModel(p, log=log, engine=rec)
    fields = jm._dev = type("F", (), {"a0": object(), "a0_mode": jm.gff_mode, "ts": object()})()
    jm._model_tavg = lambda: None
    times = np.array([3., 1., 2., 1.]) * YEAR
    freqs = np.array([5e9, 2e10, 4e10])
    flux, jac = jm.flux_vs_time_jac(times, freqs, formal=True)
    assert [c[0] for c in rec.calls] == ["ff_formal_grad"]
    c = rec.calls[0][1]
    assert c["fields"] is fields and c["epochs"] == [float(t) for t in times]
    assert c["want_maps"] is False and c["n"] == (2, 3) and c["mode"] == jm.gff_mode
    _, (ctau, cflux) = jm._channel_coeffs(freqs)
    assert np.array_equal(c["ctau"], np.array(ctau)) and np.array_equal(c["csrc"], np.array(cflux))
    assert np.array_equal(flux, np.arange(12, dtype=np.float64).reshape(4, 3))
    # the chain rule per ejection, in model.ejections order (events R, B, B, R, B -> planes 0, 6, 9, 3, 12)
    ej = list(jm.ejections.values())
    assert [e["which"] for e in ej] == ["R", "B", "B", "R", "B"] and jac.shape == (4, 3, 5, 3)
    raw = 1.0 + np.arange(4 * 3 * 15, dtype=np.float64).reshape(4, 3, 15)
    for i, (k, e_) in enumerate(zip([0, 6, 9, 3, 12], ej)):
        chain = classes.ejection_chain_rule(e_["t_0"], e_["peak_jml"], e_["half_life"],
                                            jm.ss_jml(e_["which"]))[1]
        assert np.array_equal(jac[:, :, i, :], raw[:, :, k:k + 3] * np.asarray(chain))
    # the default still reaches rjp_ff_grad
    jm.flux_vs_time_jac(times, freqs)
    assert [c[0] for c in rec.calls] == ["ff_formal_grad", "ff_grad"]
    # f32 storage raises before anything is called
    f32 = classes.JetModel(copy.deepcopy(p), log=log, engine=_RecordingEngine(), storage="f32")
    with pytest.raises(ValueError, match="f64 storage"):
        f32.flux_vs_time_jac(times, freqs, formal=True)
    assert f32.engine.calls == []


# ---- the bound has teeth -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["example-E15-F2", "example-E17-F5"])
def test_planted_mistakes_fail_the_bound(name):
    """A float64 NumPy emulation of the recurrence: correct, it passes the per-pixel bound; without
    the -om D term, or with Theta taken after its update, it fails it."""
    shape, seed, E, F, bs, _ = R.CASES[name]
    g, a0, ctau, csrc, bursts = _synth(shape, seed, F, bs)
    t = R.epochs(seed, E)[0]
    ref = R.walk(a0, g["ts"], g["temp"], bursts, t, ctau, csrc)
    bound = R.pixel_bound(ref["tau"], shape[1])[:, None]
    ratio = {m: R.worst_ratio(R.emulate(a0, g["ts"], g["temp"], bursts, t, ctau, csrc, m),
                              ref["dI"], ref["abs"], bound, ref["floor"])
             for m in (None, "no_hide", "late_theta")}
    print("worst |got - ref| / bound: correct %.3f, without -om D %.3g, Theta after its update %.3g"
          % (ratio[None], ratio["no_hide"], ratio["late_theta"]))
    assert ratio[None] <= 1.0
    assert ratio["no_hide"] > 1e3 and ratio["late_theta"] > 1e3
