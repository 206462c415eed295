"""CLEAN major cycles (`major_cycles` >= 1 of `clean_image_*` / `observe_*`; `Imager._major_chunk`) on
the device, through `Imager` on an `RTEngine` and through `JetModel`: the 33 x 33, 300-baseline
experiment of tests/major_cycles_ref.py (pinned on the CPU by tests/test_major_cycles_reference_cpu.py)
plus a second channel at 0.8 of the frequency and half the flux.

What the device is held to, every tolerance derived (none measured), u = 2^-53:
  * a re-imaged residual is K11 of V - K18(list) over the sum of the weights.  Against the long-double
    residual of the same list and data (tests/vis_adjoint_ref.py of tests/vis_components_ref.py):
        |got - ref| <= [b11 sum_k |Vres_k| + (1 + b11) sqrt(2) sum_k b18_k S18_k + u sum_k |Vres_k|] / K
                       + u max |ref|
    b11, b18 the two references' own bounds, S18_k = sum_c |f_c| + |V_k|; sqrt(2): a part's error to
    a modulus; the u terms: the reference's visibilities rounded to float64 and the division;
  * a run's picks are followed on the residual the device handed the minor cycle (tests/clean_ref.py
    `follow`, as tests/test_gpu_clean.py does), and that residual is held to the bound above at the
    list prefix; its threshold follows the rule from the REFERENCE's residual within frac x that bound;
  * the true peak -- the reference's residual of the device's list -- after 8 re-imagings is at most
    1 / 100 of minor-only's on both channels (the CPU emulation, tests/major_cycles_ref.py, gives
    1 / 511 on the experiment's channel and 1 / 631 on the second one with this window)."""
import copy
import os

import numpy as np
import pytest

from tests import clean_ref as C
from tests import gpu_util as U
from tests import major_cycles_ref as MR
from tests import vis_adjoint_ref as VA
from tests import vis_components_ref as VC
from tests import vis_ref as VR

pytestmark = pytest.mark.gpu
LD = np.longdouble
YEAR = 31557600.0
N, K = 33, 300
NITER, GAIN, THR = 2000, 0.1, 1e-6
PSF = (9, 9)
FREQS = np.array([1.0e9, 0.8e9])
FIXTURE = os.path.join(U.GOLDEN, "antenna_configs", "vla.a.cfg")


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def case(eng):
    """The experiment as an `Imager` sees it: a grid of 1 au cells at 1 pc, baselines in metres such
    that channel 0 has the experiment's (a, b) in cycles per cell and channel 1 0.8 of them; the
    visibilities are K10's of the two skies.  Computed once, never changed."""
    import torch
    from rajepy_amd import imaging
    e = MR.experiment()
    im = imaging.Imager(eng, N, N, 1.0, 1.0, 1 << 30)
    cell = im._image_grid(None, None)[2]
    su, sv = imaging.image_scales(FREQS, cell)
    u, v = e["a"] / su[0], e["b"] / sv[0]
    maps = torch.from_numpy(np.stack([e["sky"], 0.5 * e["sky"]]).reshape(2, -1)).to(eng.device)
    V = im.model_vis(maps, FREQS, u, v)
    u_d, v_d = eng._device_f64(u), eng._device_f64(v)
    cell_as = np.degrees(cell) * 3600.
    beam = (MR.BEAM_FWHM * cell_as, MR.BEAM_FWHM * cell_as, 0.)
    ab = [(su[f] * u, sv[f] * v) for f in range(2)]          # the device's own float64 products
    return dict(im=im, V=V, hV=V.cpu().numpy(), u=u_d, v=v_d, beam=beam, ab=ab, cell=cell)


def clean(case, major_cycles, psf=PSF, **kw):
    c = case
    args = dict(niter=NITER, gain=GAIN, thr=THR, mfs=False, mask=None, weights=None)
    args.update({k: kw.pop(k) for k in list(kw) if k in args})
    return c["im"]._clean_images(c["V"], c["u"], c["v"], FREQS, args["weights"], None, None, args["mfs"],
                                 args["niter"], args["gain"], args["thr"], args["mask"], c["beam"], psf,
                                 major_cycles=major_cycles, **kw)


_RESULTS = {}


def result(case, major_cycles, psf=PSF):
    key = (major_cycles, psf)
    if key not in _RESULTS:
        _RESULTS[key] = clean(case, major_cycles, psf)
    return _RESULTS[key]


def comp_list(res, m):
    comp = res.components[m]
    return (comp[:, 0] * N + comp[:, 1]).astype(np.int64), np.ascontiguousarray(comp[:, 2])


def ref_residual(case, m, cpix, cflux):
    """The long-double residual of a list and the data, and the derived bound on a device residual
    of the same list (the module's head) -> (ref float64 [N, N], tol)."""
    a, b = case["ab"][m]
    V = case["hV"][m]
    vres, S18 = VC.vis_components_ref(cpix, cflux, None, len(cpix), N, N, a, b, vin=V, sign=-1)
    b18 = VC.bound(a, b, N, N, len(cpix))
    v64 = vres.astype(np.complex128)
    ref = VA.vis_adjoint_ref(v64, a, b, N, N) / LD(K)
    b11 = VA.bound(v64, a, b, N, N)
    s11 = float(np.abs(v64).sum())
    tol = (b11 * s11 + (1. + b11) * np.sqrt(2.) * float((b18 * S18).sum()) + VR.U * s11) / K + \
        VR.U * float(np.abs(ref).max())
    return ref.astype(np.float64), tol


def hand_made(case, psf):
    """K11 + K12 + K13 composed by hand, as `_clean_images` composes them without major cycles."""
    import torch
    from rajepy_amd import engine as E
    c, eng = case, case["im"].engine
    im = c["im"]
    dirty = im._dirty_images(c["V"], c["u"], c["v"], FREQS, None, (N, N), None, False, device=True)
    beam = im._dirty_images(im._unit_vis(2, K), c["u"], c["v"], FREQS, None, psf, None, False, device=True)
    model = torch.zeros_like(dirty)
    cpix, cflux, ncomp, peak = eng.clean(dirty, N, N, beam, psf[0], psf[1], NITER, GAIN, THR, model=model)
    abc = [E.beam_quadratic(*c["beam"], c["cell"])] * 2
    image = eng.restore(cpix, cflux, ncomp, abc, N, N, add=dirty)
    return dirty, model, image, cpix, cflux, ncomp, peak, beam


# ---- major_cycles = 0 and 1 ----------------------------------------------------------------------------
def test_no_major_cycle_gives_todays_bits(case):
    res = result(case, 0)
    dirty, model, image, cpix, cflux, ncomp, peak, _ = hand_made(case, PSF)
    assert res.major is None
    assert res.image.tobytes() == image.cpu().numpy().tobytes()
    assert res.residual.tobytes() == dirty.cpu().numpy().tobytes()
    assert res.model.tobytes() == model.cpu().numpy().tobytes()
    assert res.peak_residual.tobytes() == peak.cpu().numpy().tobytes()
    hp, hf, hn = cpix.cpu().numpy(), cflux.cpu().numpy(), ncomp.cpu().numpy()
    for m in range(2):
        n = int(hn[m])
        assert np.array_equal(res.components[m], np.stack([hp[m, :n] // N, hp[m, :n] % N, hf[m, :n]], axis=1))


@pytest.mark.parametrize("psf", [PSF, (2 * N - 1, 2 * N - 1)])
def test_one_major_cycle_keeps_the_components_and_re_images_the_residual(case, psf):
    """N = 1: one run at the user's threshold -- the components of minor-only bit for bit, the model too
    -- and a residual recomputed from the visibilities.  With the full window it agrees with the
    minor cycles' own residual; with the 9 x 9 window it is the data's where minor-only's misses the
    identity by > 0.1."""
    old, new = result(case, 0, psf), result(case, 1, psf)
    _, _, _, _, _, _, _, beam = hand_made(case, psf)
    hb = beam.cpu().numpy().reshape(2, psf[0], psf[1])
    for m in range(2):
        assert new.components[m].tobytes() == old.components[m].tobytes()
        assert new.model[m].tobytes() == old.model[m].tobytes(), "components_image is rjp_clean's model"
        runs = new.major[m]["runs"]
        assert len(runs) == 1 and runs[0]["start"] == 0 and runs[0]["n"] == len(old.components[m])
        assert runs[0]["threshold"] == THR
        assert abs(new.major[m]["sidelobe"] - MR.sidelobe(hb[m], MR.CLEAN_BEAM)) <= 1e-15
        cpix, cflux = comp_list(new, m)
        ref, tol = ref_residual(case, m, cpix, cflux)
        err = float(np.abs(new.residual[m] - ref).max())
        print("psf %s map %d: |residual - ref| = %.2e, bound %.2e" % (psf, m, err, tol))
        assert err <= tol
        assert new.peak_residual[m] == np.abs(new.residual[m]).max()
        a, b = case["ab"][m]
        if psf == PSF:
            assert float(np.abs(old.residual[m] - ref).max()) > 0.1, "minor-only misses the identity"
        else:
            # the old residual is D - sum f B on the device: D and B each inside K11's bound (of sums of
            # |V| / K = at most max |V|, and of 1), and one rounding per update of at most
            # u (|D| + sum |f| |B|) (tests/clean_ref.py `conservation`)
            n, sf = len(cflux), float(np.abs(cflux).sum())
            V = case["hV"][m]
            extra = VA.bound(V, a, b, N, N) * float(np.abs(V).sum()) / K + \
                sf * VA.bound(np.ones(K, dtype=np.complex128), a, b, 2 * N - 1, 2 * N - 1) + \
                n * VR.U * (float(np.abs(V).sum()) / K + sf)
            assert float(np.abs(old.residual[m] - new.residual[m]).max()) <= tol + extra
        # the restored image is K13 of the list plus THIS residual
        assert np.abs(new.image[m] - new.residual[m] - (old.image[m] - old.residual[m])).max() <= \
            4 * VR.U * float(np.abs(old.image[m]).max() + np.abs(new.image[m]).max())


# ---- major_cycles = 8 ----------------------------------------------------------------------------------
def test_eight_major_cycles_run_by_run(case, monkeypatch):
    eng = case["im"].engine
    seen = []
    real = eng.clean

    def spy(res, nx, nz, psf, px, pz, n_iter, gain, thresh, mask=None, model=None):
        before = res.cpu().numpy().copy()
        out = real(res, nx, nz, psf, px, pz, n_iter, gain, thresh, mask=mask, model=model)
        seen.append(dict(D=before, R=res.cpu().numpy().copy(), B=psf.cpu().numpy().reshape(-1, px, pz).copy(),
                         n_iter=n_iter, thresh=np.array(thresh, dtype=np.float64), cpix=out[0].cpu().numpy(),
                         cflux=out[1].cpu().numpy(), ncomp=out[2].cpu().numpy()))
        return out

    monkeypatch.setattr(eng, "clean", spy)
    res = clean(case, 8)
    monkeypatch.undo()
    _RESULTS[(8, PSF)] = res
    minor = result(case, 0)
    assert 1 <= len(seen) <= 8
    for m in range(2):
        runs = res.major[m]["runs"]
        side = res.major[m]["sidelobe"]
        frac = min(max(1.5 * side, 0.05), 0.8)
        cpix, cflux = comp_list(res, m)
        assert sum(r["n"] for r in runs) == len(cpix) <= NITER
        assert len(cpix) == NITER or res.peak_residual[m] <= THR, "equality where thr was not reached"
        start = 0
        for i, r in enumerate(runs):
            s = seen[i]
            assert r["start"] == start and s["thresh"][m] == r["threshold"]
            assert s["n_iter"] == min(NITER, int(max(NITER - sum(q["n"] for q in res.major[k]["runs"][:i])
                                                    for k in range(2))))
            # the residual the run started from: the reference's own at the list prefix, the bound
            ref, tol = ref_residual(case, m, cpix[:start], cflux[:start])
            D = s["D"][m].reshape(N, N)
            assert float(np.abs(D - ref).max()) <= tol, (m, i)
            assert r["peak"] == np.abs(D).max()
            last = i == 7
            want = MR.run_threshold(THR, float(np.abs(ref).max()), side, 1.5, 0.05, 0.8, last)
            assert abs(r["threshold"] - want) <= (0. if last else frac * tol + VR.U * want), (m, i)
            # the picks: Hogbom's on that residual, the first `n` of what the run found kept
            n = r["n"]
            assert n == min(int(s["ncomp"][m]), NITER - start)
            assert np.array_equal(s["cpix"][m, :n], cpix[start:start + n])
            assert np.array_equal(s["cflux"][m, :n], cflux[start:start + n])
            C.follow(D, s["B"][m], None, r["threshold"], GAIN, s["n_iter"], s["cpix"][m], s["cflux"][m],
                     int(s["ncomp"][m]), s["R"][m].reshape(N, N))
            start += n
        # the final residual, and the true peak against minor-only's
        ref, tol = ref_residual(case, m, cpix, cflux)
        assert float(np.abs(res.residual[m] - ref).max()) <= tol
        mp, mf = comp_list(minor, m)
        true_minor = float(np.abs(ref_residual(case, m, mp, mf)[0]).max())
        true_major = float(np.abs(ref).max())
        print("map %d: runs %s; true peak %.3e, minor-only's %.3e (reported %.3e): 1 / %.0f"
              % (m, [(r["n"], float("%.2e" % r["threshold"])) for r in runs], true_major, true_minor,
                 minor.peak_residual[m], true_minor / true_major))
        assert true_major <= true_minor / 100.
        assert res.major[m]["vis_residual"].shape == (K,)
        vres, S18 = VC.vis_components_ref(cpix, cflux, None, len(cpix), N, N, *case["ab"][m],
                                          vin=case["hV"][m], sign=-1)
        assert VC.worst_ratio(res.major[m]["vis_residual"], vres, S18,
                              VC.bound(*case["ab"][m], N, N, len(cpix))) <= 1.0
    # cycleniter bounds every run, niter the list; a second call gives the same bits
    short = clean(case, 5, niter=100, cycleniter=30)
    for m in range(2):
        ns = [r["n"] for r in short.major[m]["runs"]]
        assert all(n <= 30 for n in ns) and sum(ns) == len(short.components[m]) <= 100, ns
    again = clean(case, 8)
    for name in ("image", "residual", "model", "peak_residual"):
        assert getattr(again, name).tobytes() == getattr(res, name).tobytes(), name
    for m in range(2):
        assert again.components[m].tobytes() == res.components[m].tobytes()
        assert again.major[m]["vis_residual"].tobytes() == res.major[m]["vis_residual"].tobytes()
        assert again.major[m]["runs"] == res.major[m]["runs"]


def test_a_map_that_is_finished_does_nothing(case):
    """A threshold per map: map 1's lies above its peak, so it takes the largest finite double and
    finds nothing, while map 0 goes on; with both above, no run is made at all."""
    res = clean(case, 3, thr=np.array([1e-3, 10.0]))
    assert len(res.components[1]) == 0 and res.major[1]["runs"] == []
    assert len(res.major[0]["runs"]) == 3 and len(res.components[0]) > 0
    assert np.array_equal(res.major[1]["vis_residual"], case["hV"][1])
    assert np.all(res.model[1] == 0.) and np.array_equal(res.image[1], res.residual[1])
    none = clean(case, 3, thr=10.0)
    c = case
    dirty = c["im"]._dirty_images(c["V"], c["u"], c["v"], FREQS, None, (N, N), None, False)
    assert none.residual.tobytes() == dirty.tobytes() and all(len(x) == 0 for x in none.components)


# ---- multi-scale, mfs, weights, observe, imfit ------------------------------------------------------------
def _re_imaged(case, res, mfs=False, weights=None, weighting=None):
    """`_dirty_images` of `CleanResult.major[.]['vis_residual']`: what the residual must be, to the bit."""
    import torch
    c = case
    vres = torch.from_numpy(np.stack([d["vis_residual"] for d in res.major])).to(c["im"].engine.device)
    if mfs:
        vres = vres.reshape(2, K)
    return c["im"]._dirty_images(vres, c["u"], c["v"], FREQS, weights, (N, N), None, mfs, weighting=weighting)


def test_multi_scale_raw_residual_is_the_adjoint_of_the_datas_rest(case):
    """scales=[0, 2, 4] on the 9 x 9 window: the raw residual is the dirty image of V minus the
    transform of the model image (K10 of `model`, in long double here), where minor-only's is not.
    The tolerance adds, to the residual's bound with S18_k = sum |f| + |V_k|, what separates K18's
    G from K10 of the convolved model: K10's own bound on a unit-sum kernel and one rounding per
    kernel term (at most 7 x 7) of the convolution, each times sum |f|."""
    scales = [0, 2, 4]
    old = clean(case, 0, scales=scales, niter=300, thr=1e-4)
    new = clean(case, 4, scales=scales, niter=300, thr=1e-4)
    assert tuple(new.residual[0].shape) == (N, N) and new.components[0].shape[1] == 4
    assert _re_imaged(case, new).tobytes() == new.residual.tobytes()
    for m in range(2):
        a, b = case["ab"][m]
        V = case["hV"][m]
        for res, inside in ((new, True), (old, False)):
            f = res.components[m][:, 2]
            vres = V.astype(np.clongdouble) - VR.vis_ref(res.model[m], a, b)
            v64 = vres.astype(np.complex128)
            ref = (VA.vis_adjoint_ref(v64, a, b, N, N) / LD(K)).astype(np.float64)
            sf = float(np.abs(f).sum())
            b11, s11 = VA.bound(v64, a, b, N, N), float(np.abs(v64).sum())
            b18 = VC.bound(a, b, N, N, len(f), 3)
            tol = (b11 * s11 + (1. + b11) * np.sqrt(2.) * float((b18 * (sf + np.abs(V))).sum()) + VR.U * s11 +
                   K * sf * (float(np.max(VR.bound(a, b, 7, 7))) + 51 * VR.U)) / K + VR.U * float(np.abs(ref).max())
            err = float(np.abs(res.residual[m] - ref).max())
            print("multi-scale map %d, %s: |raw residual - ref| = %.2e (bound %.2e)"
                  % (m, "major" if inside else "minor only", err, tol))
            assert (err <= tol) if inside else (err > 1e-3)
        assert len(set(new.components[m][:, 3])) > 1
        assert sum(r["n"] for r in new.major[m]["runs"]) == len(new.components[m]) <= 300


def test_mfs_briggs_and_weights_re_image_with_the_dirty_images_weights(case):
    rng = np.random.default_rng(1)
    w = rng.uniform(0.5, 2.0, K)
    for kw, args in ((dict(mfs=True), dict(mfs=True)),
                     (dict(weighting="briggs", robust=0.5), dict(weighting="briggs")),
                     (dict(weights=w), dict(weights=w)),
                     (dict(mfs=True, weighting="briggs", weights=w), dict(mfs=True, weighting="briggs", weights=w))):
        res = clean(case, 3, niter=200, **kw)
        n_out = 1 if kw.get("mfs") else 2
        assert res.residual.shape == (n_out, N, N) and len(res.major) == n_out
        assert res.major[0]["vis_residual"].shape == ((2 * K,) if kw.get("mfs") else (K,))
        # (with imaging weights `_re_imaged` makes its own set: the same call, the same numbers)
        assert _re_imaged(case, res, **args).tobytes() == res.residual.tobytes(), kw
        for m in range(n_out):
            assert res.peak_residual[m] == np.abs(res.residual[m]).max()
            assert 0 < sum(r["n"] for r in res.major[m]["runs"]) == len(res.components[m]) <= 200
            peaks = [r["peak"] for r in res.major[m]["runs"]]
            assert len(peaks) == 1 or peaks[-1] < peaks[0], "re-imaging brings the peak down"


def _params(tag):
    p = copy.deepcopy(U.load_golden(tag)[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


def test_observe_ff_and_clean_image_ff_on_the_example_model(eng, tmp_path_factory):
    from rajepy_amd import classes, logger
    from rajepy_amd import engine as E
    log = logger.Log(str(tmp_path_factory.mktemp("major") / "model.log"), verbose=False)
    jm = classes.JetModel(_params("cfg1_example"), log=log, engine=eng)
    jm.time = 1.0 * YEAR
    freqs = np.array([4.9e9, 5.1e9])
    tr = jm.uv_tracks(FIXTURE, 1200., 60., min_el_deg=20.)
    cell = E.observation_grid(tr.max_baseline_m, 5e9, 1.0)[0]
    peak = float(np.abs(jm.visibilities_ff([0.], [0.], freqs)).max())
    kw = dict(shape=(48, 40), cell_as=cell, niter=60, weighting="briggs", robust=0.5, psf_shape=(21, 21))
    obs = jm.observe_ff(tr, freqs, 1200., 60., sigma_jy=0.5 * peak, seed=5, nsigma=3., imfit=True,
                        major_cycles=2, **kw)
    res = obs.clean
    assert len(res.major) == 2 and len(res.imfit) == 2 and res.imfit[0]["Ierr"]["val"] is not None
    for m in range(2):
        runs = res.major[m]["runs"]
        assert 1 <= len(runs) <= 2 and sum(r["n"] for r in runs) == len(res.components[m]) <= 60
        assert res.major[m]["vis_residual"].shape == (tr.u_m.numel(),)
        assert len(res.components[m]) == 60 or res.peak_residual[m] <= 3. * obs.image_rms[m]
        assert np.isfinite(res.image[m]).all()
    plain = jm.observe_ff(tr, freqs, 1200., 60., sigma_jy=0.5 * peak, seed=5, nsigma=3., imfit=True, **kw)
    assert plain.clean.major is None and np.array_equal(plain.vis, obs.vis)
    ff = jm.clean_image_ff(tr.u_m, tr.v_m, freqs, major_cycles=2, mfs=True, **kw)
    assert len(ff.major) == 1 and ff.major[0]["vis_residual"].shape == (2 * tr.u_m.numel(),)
    again = jm.clean_image_ff(tr.u_m, tr.v_m, freqs, major_cycles=2, mfs=True, **kw)
    assert again.image.tobytes() == ff.image.tobytes() and again.residual.tobytes() == ff.residual.tobytes()


def test_bad_keywords_raise(case):
    for bad in (dict(major_cycles=-1), dict(major_cycles=1.5), dict(cyclefactor=0.), dict(cyclefactor=-1.),
                dict(cyclefactor=float("nan")), dict(cyclefactor=float("inf")), dict(cycleniter=0),
                dict(cycleniter=-3), dict(min_psf_fraction=-0.1), dict(max_psf_fraction=1.1),
                dict(min_psf_fraction=0.9, max_psf_fraction=0.8)):
        mc = bad.pop("major_cycles", 1)
        with pytest.raises(ValueError):
            clean(case, mc, niter=5, **bad)
        if "major_cycles" not in bad and mc == 1:
            with pytest.raises(ValueError):          # checked whether or not a major cycle is asked for
                clean(case, 0, niter=5, **bad)
