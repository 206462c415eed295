"""JetModel.fit_ejections_flux / fit_ejections_vis (K23) on the device, on the oracle's `tilted`
model with the epochs, channels, ties, start and noise seed that tests/fit_ejections_ref.py
holds and at TEN TIMES the recovery error it measured there with the same loop on the long-double
K7 reference (the device differs from that run by rounding and at most an iteration, not by
method): noise-free fits of light curves (isothermal and formal) and of visibilities (one (u, v)
coverage, and one per epoch) on about 40 baselines of the 27-antenna fixture reach status 1 with
strictly decreasing accepted chi^2 and recover the truth; the model is untouched unless `update`;
the first trial's N, g and chi^2 agree with tests/normal_eq_ref.py on the host arrays of
`visibilities_vs_time_jac` at the derived bound plus the chain rule's; a held parameter keeps its
bits and a tied pair stays equal; the refusals.  The module prints every figure it judges; on one
MI355X: light curves 4.3e-12 (isothermal) and 1.1e-12 (formal) in 9 trials, visibilities 2.7e-14 and
3.2e-14 in 7 trials, against the bar of 1.1e-11; the first trial at 0.002 of its bound; the noisy
visibility fit status 1 after 12 trials, reduced chi^2 1.031 (0.16 of its limit), worst pull 2.5 sigma."""
import copy

import numpy as np
import pytest

from tests import gpu_util as U
from tests import lm_ref
from tests import normal_eq_ref as K
from tests import fit_ejections_ref as C

pytestmark = pytest.mark.gpu
YEAR = C.YEAR
FIXTURE = C.FIXTURE
BAR = 10.0 * C.RECOVERY
TIMES = np.array(C.EPOCHS_YR) * YEAR
U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def jm(eng, tmp_path_factory):
    return C.tilted(tmp_path_factory.mktemp("fit"), eng)


@pytest.fixture(scope="module")
def setup(jm):
    """(freqs, u, v [K ~ 40], truth): every ninth baseline of one integration of the fixture."""
    freqs = np.asarray(U.load_golden("tilted")[0]["freqs"], dtype=np.float64)[:C.CHANNELS]
    tr = jm.uv_tracks(FIXTURE, 60.0, 60.0)
    host = lambda t: np.asarray(t.cpu() if hasattr(t, "cpu") else t, dtype=np.float64).reshape(-1)
    u, v = host(tr.u_m)[:351:9].copy(), host(tr.v_m)[:351:9].copy()
    assert u.size == 39
    return freqs, u, v, C.truth_of(jm)


def state(jm):
    return copy.deepcopy(jm.ejections), copy.deepcopy(jm._bursts), jm._version


def judge(kind, R, truth, n_free=6):
    chis = [r["chi2"] for r in R.trace if r["accepted"]]
    err = float(np.max(np.abs(R.theta / truth - 1.0)))
    print("\n%s: status %d after %d trials, chi2 %.3g, worst relative error %.3g (bar %.3g)"
          % (kind, R.status, R.niter, R.chi2, err, BAR))
    assert R.status == 1
    assert all(b < a for a, b in zip(chis, chis[1:])) and len(chis) >= 3
    assert err <= BAR
    assert R.theta[0, 0] == R.theta[1, 0] and R.theta[0, 2] == R.theta[1, 2]          # the tie
    assert R.theta[1, 1] / R.theta[0, 1] == pytest.approx(truth[1, 1] / truth[0, 1], rel=4 * U53)
    assert R.cov.shape == (n_free, n_free)


@pytest.mark.parametrize("formal", [False, True])
def test_noise_free_light_curves(jm, setup, formal):
    freqs, _, _, truth = setup
    data = jm.flux_vs_time(TIMES, freqs, formal=formal)
    before = state(jm)
    R = jm.fit_ejections_flux(TIMES, freqs, data, formal=formal, tie=C.RB_TIE, theta0=truth * C.START,
                              n_iter=C.N_ITER, xtol=C.XTOL, trace=True)
    assert state(jm) == before, "the model was touched"
    assert R.ndata == data.size
    judge("light curves, formal %s" % formal, R, truth)


def test_a_held_parameter_keeps_its_bits(jm, setup):
    freqs, _, _, truth = setup
    data = jm.flux_vs_time(TIMES, freqs)
    start = truth * C.START
    start[2, 2] = truth[2, 2]
    free = np.ones((3, 3), dtype=bool)
    free[2, 2] = False
    R = jm.fit_ejections_flux(TIMES, freqs, data, tie=C.RB_TIE, theta0=start, free=free, n_iter=C.N_ITER,
                              xtol=C.XTOL, trace=True)
    assert all(r["theta"][5] == truth[2, 2] for r in R.trace) and R.ejections["3"]["e_half_life"] == 0.0
    judge("light curves, half_life of 3 held", R, truth, n_free=5)


def test_update_writes_the_fit_back(jm, setup):
    freqs, _, _, truth = setup
    data = jm.flux_vs_time(TIMES, freqs)
    jac = jm.flux_vs_time_jac(TIMES, freqs)[1]                             # [E, F, n_ej, 3] at the truth
    try:
        R = jm.fit_ejections_flux(TIMES, freqs, data, tie=C.RB_TIE, theta0=truth * C.START, n_iter=C.N_ITER,
                                  xtol=C.XTOL, update=True, trace=True)
        judge("light curves, update", R, truth)
        assert C.truth_of(jm).tobytes() == R.theta.tobytes()
        again = jm.flux_vs_time(TIMES, freqs)
        # every parameter is within BAR of the truth (asserted above), so to first order a flux moves by at
        # most BAR sum_p |dF/dtheta_p theta_p|; twice that for the higher orders, and 8 u for the roundings
        # of two evaluations
        lim = 2.0 * BAR * np.sum(np.abs(jac * truth[None, None]), axis=(2, 3)) + 8 * U53 * np.abs(data)
        worst = float(np.max(np.abs(again - data) / lim))
        print("flux_vs_time after update against the data: %.3g of the first-order limit" % worst)
        assert worst <= 1.0
    finally:
        for i, k in enumerate(jm.ejections):
            jm.set_ejection_event(k, *truth[i])
    assert C.truth_of(jm).tobytes() == truth.tobytes()
    assert np.array_equal(jm.flux_vs_time(TIMES, freqs), data)


def per_epoch(u, v):
    s = 1.0 + 0.02 * np.arange(len(TIMES))[:, None]
    return u[None, :] * s, v[None, :] * s


@pytest.mark.parametrize("coverage", ["shared", "per epoch"])
def test_noise_free_visibilities(jm, setup, coverage):
    freqs, u, v, truth = setup
    if coverage == "shared":
        uu, vv = u, v
        data = jm.visibilities_vs_time(TIMES, u, v, freqs, formal=True)
    else:
        uu, vv = per_epoch(u, v)
        data = np.concatenate([jm.visibilities_vs_time(TIMES[e:e + 1], uu[e], vv[e], freqs, formal=True)
                               for e in range(len(TIMES))])
    before = state(jm)
    R = jm.fit_ejections_vis(TIMES, uu, vv, freqs, data, tie=C.RB_TIE, theta0=truth * C.START, n_iter=C.N_ITER,
                             xtol=C.XTOL, trace=True)
    assert state(jm) == before, "the model was touched"
    assert R.ndata == 2 * data.size
    judge("visibilities, %s coverage" % coverage, R, truth)


def test_a_noisy_visibility_fit_obeys_the_chi2_and_normal_laws(jm, setup, eng):
    """Thermal noise from `vis_noise` with the one seed tests/test_fit_ejections_reference_cpu.py chose on
    the device-free emulation of this very fit, sigma = 1e-3 of the largest |V|, weights 1 / sigma^2:
    reduced chi2 within 1 +- 5 sqrt(2 / nu), nu = 2 count - P_free, and every parameter within 5 of its
    reported standard errors -- the chi^2 and normal laws."""
    import torch
    freqs, u, v, truth = setup
    V = jm.visibilities_vs_time(TIMES, u, v, freqs, formal=True)
    E, F, Kv = V.shape
    sigma = C.NOISE_REL * float(np.abs(V).max())
    D = eng.vis_noise(torch.from_numpy(V.reshape(E * F, Kv)).to(eng.device), sigma, seed=C.NOISE_SEED)
    R = jm.fit_ejections_vis(TIMES, u, v, freqs, D.reshape(E, F, Kv), weights=np.full(Kv, 1.0 / sigma ** 2),
                             tie=C.RB_TIE, theta0=truth * C.START, n_iter=C.NOISY_ITER, xtol=C.NOISY_XTOL)
    chi, pull = C.laws(R, truth, 6)
    print("\nnoisy visibilities: status %d after %d trials, reduced chi2 %.3f (%.2f of its limit), worst pull "
          "%.2f of 5 sigma" % (R.status, R.niter, R.reduced_chi2, chi, pull))
    assert R.ndata == 2 * V.size and R.status != 3
    assert chi <= 1.0 and pull <= 1.0


def test_the_first_trial_against_the_reference_on_the_host_jacobian(jm, setup):
    """N, g and chi^2 of the first trial (at the model's own parameters) against tests/normal_eq_ref.py
    on `visibilities_vs_time_jac`'s host arrays, through T^T . T.  The bound: the reference's own per
    entry (derived there), plus the chain rule's -- the device multiplies the sums of the raw planes
    by the two chain factors, the host Jacobian multiplied every derivative by one first: three
    roundings per factor pair on either side and the factors' own (a quotient and a product more),
    16 u of the sum of the absolute terms covers both -- both carried through |T|, plus 8 u of the
    absolute products for T^T . T itself."""
    freqs, u, v, truth = setup
    V, dV = jm.visibilities_vs_time_jac(TIMES, u, v, freqs)
    E, F, Kv = V.shape
    rng = np.random.default_rng(3)
    data = V * (1.0 + 0.01 * rng.standard_normal(V.shape)) + 1e-6 * rng.standard_normal(V.shape)
    w = rng.uniform(0.5, 2.0, size=Kv)
    w[::7] = 0.0
    R = jm.fit_ejections_vis(TIMES, u, v, freqs, data, weights=w, tie=C.RB_TIE, n_iter=1, trace=True)
    row = R.trace[0]
    ref = K.sums(data.reshape(E * F, Kv), V.reshape(E * F, Kv), dV.reshape(E * F, 9, Kv), range(9), w, 2)
    assert R.ndata == 2 * ref["count"] and ref["count"] == E * F * int((w > 0).sum())
    b = K.bounds(ref, 2)
    from rajepy_amd import inference
    lay = inference.BurstFit(jm).layout(None, C.RB_TIE, None)
    T = np.asarray(lay["T"], dtype=lm_ref.LD)
    N = T.T @ lm_ref.unpack(ref["N"], 9) @ T
    g = T.T @ ref["g"]
    aN = np.abs(T).T @ lm_ref.unpack(ref["a_N"], 9) @ np.abs(T)
    ag = np.abs(T).T @ ref["a_g"]
    bN = np.abs(T).T @ lm_ref.unpack(b["N"], 9) @ np.abs(T) + (16 + 8) * U53 * aN
    bg = np.abs(T).T @ b["g"] + (16 + 8) * U53 * ag
    rN = float(np.max(np.abs(row["N"] - N) / bN))
    rg = float(np.max(np.abs(row["g"] - g) / bg))
    rc = float(abs(row["chi2"] - ref["chi2"]) / b["chi2"])
    print("\nfirst trial against the reference, error / bound: N %.3f, g %.3f, chi2 %.3f" % (rN, rg, rc))
    assert rN <= 1.0 and rg <= 1.0 and rc <= 1.0


def test_refusals(jm, setup, eng, tmp_path):
    from rajepy_amd import classes, logger
    freqs, u, v, truth = setup
    data = jm.flux_vs_time(TIMES, freqs)
    before = state(jm)
    bad = truth.copy()
    bad[2, 2] = -1.0
    R = jm.fit_ejections_flux(TIMES, freqs, data, tie=C.RB_TIE, theta0=bad, update=True)
    assert R.status == 3 and R.ejections is None and R.cov is None and state(jm) == before
    p = C.tilted(tmp_path).params
    f32 = classes.JetModel(copy.deepcopy(p), log=logger.Log(str(tmp_path / "f32.log"), verbose=False), engine=eng,
                           storage="f32")
    with pytest.raises(ValueError, match="f64 storage"):
        f32.fit_ejections_vis(TIMES, u, v, freqs, np.ones((len(TIMES), len(freqs), u.size), dtype=complex))
    with pytest.raises(ValueError, match="f64 storage"):
        f32.fit_ejections_flux(TIMES, freqs, data)
    q = copy.deepcopy(p)
    for k in ("t_0", "hl", "chi", "which"):
        q["ejection"][k] = q["ejection"][k][:0]
    none = classes.JetModel(q, log=logger.Log(str(tmp_path / "none.log"), verbose=False), engine=eng)
    for call in (lambda: none.fit_ejections_flux(TIMES, freqs, data),
                 lambda: none.fit_ejections_vis(TIMES, u, v, freqs, np.ones((8, 2, u.size), dtype=complex))):
        with pytest.raises(ValueError, match="no ejections"):
            call()
