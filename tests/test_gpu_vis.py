"""rjp_vis (K10, vis.hip): model visibilities of map stacks at given (u, v) points, through the
C-ABI, RTEngine.vis and JetModel.visibilities_*, against tests/vis_ref.py -- a long-double NumPy
direct sum on the maps read back from the device, which tests/test_vis_reference_cpu.py pins to the
FFT, to analytic transforms and to symmetries, and whose bound it holds to a float64 emulation
(inside) and three planted mistakes (outside).

The bound is derived in tests/vis_ref.py, not measured: per visibility and component
    |got - ref| <= [2 pi (|a| (nx-1)/2 + |b| (nz-1)/2) u + 2 (2.01e-14 + 6 u) + (nx + nz + 24) u] sum |I|
(u = 2^-53; a, b in cycles per cell).  The module prints the worst |got - ref| / bound per group."""
import copy

import numpy as np
import pytest

from tests import gpu_util as U
from tests import vis_ref as R

pytestmark = pytest.mark.gpu
YEAR = 31557600.0
WORST = {}


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()
    print("\nworst |got - ref| / bound per group: " +
          ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def note(kind, got, ref, S, bnd):
    r = R.worst_ratio(got, ref, S, bnd) if S > 0 else 0.0
    WORST[kind] = max(WORST.get(kind, 0.0), r)
    assert r <= 1.0, (kind, r)
    return r


def dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(eng.device)


def raw(eng, maps, n_maps, nx, nz, su, sv, u, v, n_vis, out, work, nbytes):
    from rajepy_amd import _lib
    ptr = lambda t: t.data_ptr() if t is not None else None
    return eng.lib.rjp_vis(eng.ctx, ptr(maps), n_maps, nx, nz,
                           _lib.dbl_array(su) if su is not None else None,
                           _lib.dbl_array(sv) if sv is not None else None,
                           ptr(u), ptr(v), n_vis, ptr(out), ptr(work), nbytes, eng._stream())


# ---- 1: random maps at the bound -----------------------------------------------------------------
FACTORS = (1.0, -0.37, 0.61)          # every map its own scale, signs included


@pytest.mark.parametrize("nx,nz", R.SHAPES)
def test_random_maps_against_the_reference(eng, nx, nz):
    """Both tile heights (nx <= 64: 64 rows, else 128), one and two row tiles, 1-5 visibility
    tiles with ragged ends, nz below, at and beyond a 16-cell chunk; 20 % NaN pixels, an all-NaN
    map, the zero spacing in every set, a scale per map."""
    rng = np.random.default_rng(1000 * nx + nz)
    stack = np.stack([R.random_map(rng, nx, nz) for _ in range(3)])
    stack[1] = np.nan
    worst = 0.0
    for n_maps in (1, 3):
        maps = stack[[0]] if n_maps == 1 else stack
        d_maps = dev(eng, maps.reshape(n_maps, -1))
        for n_vis in R.N_VIS:
            for amax in (0.5, 8.0):
                u, v = R.random_points(rng, n_vis, 1.0)
                su = amax * np.array(FACTORS[:n_maps])
                sv = -amax * np.array(FACTORS[:n_maps][::-1])
                got = eng.vis(d_maps, nx, nz, su, sv, u, v).cpu().numpy()
                assert got.shape == (n_maps, n_vis) and got.dtype == np.complex128
                for m in range(n_maps):
                    a, b = su[m] * u, sv[m] * v           # the device's own float64 products
                    S = R.sum_abs(maps[m])
                    if S == 0:
                        assert np.all(got[m] == 0), "an all-NaN map transforms to exact zeros"
                        continue
                    worst = max(worst, note("random |a| <= %g" % amax, got[m],
                                            R.vis_ref(maps[m], a, b), S, R.bound(a, b, nx, nz)))
                    assert abs(got[m, 0] - np.nansum(maps[m])) <= (nx * nz + 8) * R.U * S
    print("%d x %d: worst |got - ref| / bound = %.3f" % (nx, nz, worst))


# ---- 2: repeat, guard bands, a non-finite baseline -------------------------------------------------
def test_repeat_guard_bands_and_a_non_finite_baseline(eng):
    import torch
    nx, nz, M, K = 130, 65, 3, 65
    rng = np.random.default_rng(7)
    maps = np.stack([R.random_map(rng, nx, nz) for _ in range(M)])
    d_maps = dev(eng, maps.reshape(M, -1))
    u, v = R.random_points(rng, K, 1.0)
    su, sv = 0.5 * np.array(FACTORS), 0.4 * np.array(FACTORS)
    wb = eng.lib.rjp_vis_workspace(M, nx, nz, K)
    assert wb >= M * 2 * K * 16
    guard, n_out = 4096, M * K * 2
    out = torch.full((guard + n_out + guard,), -7.0, dtype=torch.float64, device=eng.device)
    work = torch.full((wb + guard,), 0xA5, dtype=torch.uint8, device=eng.device)
    call = lambda uu, o: raw(eng, d_maps, M, nx, nz, su, sv, dev(eng, uu), dev(eng, v), K,
                             o[guard:], work, wb)
    assert call(u, out) == 0, eng.lib.rjp_last_error(eng.ctx)
    eng.synchronize()
    assert bool((out[:guard] == -7.0).all()) and bool((out[guard + n_out:] == -7.0).all())
    assert bool((work[wb:] == 0xA5).all())
    first = out[guard:guard + n_out].clone()
    assert bool(torch.isfinite(first).all())
    assert torch.equal(torch.view_as_real(eng.vis(d_maps, nx, nz, su, sv, u, v)).reshape(-1), first)
    out2 = torch.full_like(out, -7.0)
    assert call(u, out2) == 0
    eng.synchronize()
    assert torch.equal(out2, out), "a repeated call gives the same bits"
    # one non-finite u: that visibility is NaN in every map, every other one keeps its bits
    for bad in (np.nan, np.inf):
        ub = u.copy()
        ub[17] = bad
        out3 = torch.full_like(out, -7.0)
        assert call(ub, out3) == 0
        eng.synchronize()
        got, want = out3[guard:guard + n_out].reshape(M, K, 2), first.reshape(M, K, 2)
        assert bool(torch.isnan(got[:, 17]).all())
        keep = [k for k in range(K) if k != 17]
        assert torch.equal(got[:, keep], want[:, keep])
    vb = v.copy()
    vb[0] = -np.inf
    got = eng.vis(d_maps, nx, nz, su, sv, u, vb)
    assert bool(torch.isnan(torch.view_as_real(got)[:, 0]).all())
    assert torch.equal(torch.view_as_real(got)[:, 1:].reshape(M, -1), first.reshape(M, K * 2)[:, 2:])


# ---- 3: refusals -------------------------------------------------------------------------------------
def test_refusals_leave_poisoned_outputs_untouched(eng):
    import torch
    from rajepy_amd import _lib
    nx, nz, M, K = 5, 3, 2, 7
    d_maps = dev(eng, np.ones((M, nx * nz)))
    u, v = dev(eng, np.linspace(0, 1, K)), dev(eng, np.linspace(-1, 0, K))
    su, sv = [0.1, 0.2], [0.3, -0.4]
    wb = eng.lib.rjp_vis_workspace(M, nx, nz, K)
    out = torch.full((M * K * 2,), 7.0, dtype=torch.float64, device=eng.device)
    work = torch.full((wb,), 0xA5, dtype=torch.uint8, device=eng.device)
    good = dict(maps=d_maps, n_maps=M, nx=nx, nz=nz, su=su, sv=sv, u=u, v=v, n_vis=K, out=out,
                work=work, nbytes=wb)
    ARG, WS = _lib.RJP_ERR_ARG, _lib.RJP_ERR_WORKSPACE
    cases = [("NULL maps", dict(maps=None), ARG), ("NULL h_su", dict(su=None), ARG),
             ("NULL h_sv", dict(sv=None), ARG), ("NULL d_u", dict(u=None), ARG),
             ("NULL d_v", dict(v=None), ARG), ("n_maps = 0", dict(n_maps=0), ARG),
             ("n_maps < 0", dict(n_maps=-1), ARG), ("nx = 0", dict(nx=0), ARG),
             ("nz < 0", dict(nz=-3), ARG), ("n_vis = 0", dict(n_vis=0), ARG),
             ("n_vis < 0", dict(n_vis=-1), ARG), ("NaN h_su", dict(su=[0.1, np.nan]), ARG),
             ("infinite h_sv", dict(sv=[np.inf, 0.1]), ARG),
             ("a short workspace", dict(nbytes=wb - 1), WS), ("no workspace", dict(work=None), WS)]
    for what, kw, want in cases:
        assert raw(eng, **dict(good, **kw)) == want, what
    assert raw(eng, **dict(good, out=None)) == ARG
    eng.synchronize()
    assert bool((out == 7.0).all()) and bool((work == 0xA5).all())
    msg = eng.lib.rjp_last_error(eng.ctx)
    assert msg and len(msg) > 10
    assert raw(eng, **good) == _lib.RJP_OK                # the context still serves a valid call
    eng.synchronize()
    assert not bool((out == 7.0).any())
    with pytest.raises(ValueError):
        eng.vis(d_maps, nx, nz, su[:1], sv, u, v)
    with pytest.raises(ValueError):
        eng.vis(d_maps, nx, 4, su, sv, u, v)
    with pytest.raises(_lib.RjprtError):
        eng.vis(d_maps, nx, nz, [np.nan, 1.], sv, u, v)


# ---- 4: the golden models through JetModel ----------------------------------------------------------
def _params(tag):
    p = copy.deepcopy(U.load_golden(tag)[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


_MODELS = {}


def model(eng, tag, tmp_path_factory):
    from rajepy_amd import classes, logger
    if tag not in _MODELS:
        log = logger.Log(str(tmp_path_factory.mktemp("vis") / (tag + ".log")), verbose=False)
        _MODELS[tag] = classes.JetModel(_params(tag), log=log, engine=eng)
    return _MODELS[tag]


def baselines(jm, freqs, n=5, amax=0.5, seed=3):
    """Baselines in metres that reach `amax` cycles per cell at the highest frequency; the zero
    spacing first."""
    su, sv = jm._vis_scales(freqs)
    rng = np.random.default_rng(seed)
    u, v = R.random_points(rng, n, amax / np.abs(su).max())
    return u, v, su, sv


def check_maps(kind, V, maps, u, v, su, sv):
    """V[F, K] against the reference on the host maps[F, nx, nz]."""
    for f in range(maps.shape[0]):
        a, b = su[f] * u, sv[f] * v
        S = R.sum_abs(maps[f])
        assert S > 0
        note(kind, V[f], R.vis_ref(maps[f], a, b), S, R.bound(a, b, *maps[f].shape))


def test_visibilities_ff_on_the_example_model(eng, tmp_path_factory):
    jm = model(eng, "cfg1_example", tmp_path_factory)
    z = U.load_golden("cfg1_example")[0]
    freqs = np.asarray(z["freqs"], dtype=np.float64)[:3]
    jm.time = 1.0 * YEAR
    u, v, su, sv = baselines(jm, freqs)
    V = jm.visibilities_ff(u, v, freqs)
    flux = jm.flux_ff(freqs)
    assert V.shape == (3, 5) and V.dtype == np.complex128 and flux.shape == (3, jm.nx, jm.nz)
    assert np.isnan(flux).any()
    # the zero spacing is the total flux: nansum of the map, and flux_vs_time's value
    lc = jm.flux_vs_time([jm.time], freqs)[0]
    P = jm.nx * jm.nz
    for f in range(3):
        S = R.sum_abs(flux[f])
        assert V[f, 0].imag == 0.0
        assert abs(V[f, 0].real - np.nansum(flux[f])) <= P * R.U * S
        assert abs(V[f, 0].real - lc[f]) <= P * R.U * S
    check_maps("flux_ff", V, flux, u, v, su, sv)
    assert np.abs(V[:, 1:].imag).max() > 0 and np.abs(V[:, 1:]).max() < np.abs(V[:, 0]).max()


def test_visibilities_ff_formal_on_the_tilted_model(eng, tmp_path_factory):
    jm = model(eng, "tilted", tmp_path_factory)
    z = U.load_golden("tilted")[0]
    freqs = np.asarray(z["freqs"], dtype=np.float64)
    jm.time = 0.4 * YEAR
    u, v, su, sv = baselines(jm, freqs)
    Vf = jm.visibilities_ff(u, v, freqs, formal=True)
    Vi = jm.visibilities_ff(u, v, freqs)
    flux = jm.flux_ff(freqs, formal=True)
    check_maps("formal", Vf, flux, u, v, su, sv)
    check_maps("flux_ff", Vi, jm.flux_ff(freqs), u, v, su, sv)
    lc = jm.flux_vs_time([jm.time], freqs, formal=True)[0]
    for f in range(len(freqs)):
        S = R.sum_abs(flux[f])
        assert abs(Vf[f, 0].real - lc[f]) <= jm.nx * jm.nz * R.U * S
        # a temperature gradient along the sightlines: the two solutions are different maps
        assert np.abs(Vf[f] - Vi[f]).max() > 1e3 * R.bound(su[f] * u, sv[f] * v, jm.nx, jm.nz).max() * S


def test_visibilities_rrl_on_one_line(eng, tmp_path_factory):
    jm = model(eng, "cfg1_example", tmp_path_factory)
    z, meta, _ = U.load_golden("cfg1_example")
    rf = np.asarray(z["rrl_freqs"], dtype=np.float64)[3:5]
    jm.time = 1.0 * YEAR
    u, v, su, sv = baselines(jm, rf)
    for contsub in (True, False):
        V = jm.visibilities_rrl(meta["rrl"], u, v, rf, contsub=contsub)
        assert V.shape == (2, 5)
        check_maps("flux_rrl", V, jm.flux_rrl(meta["rrl"], rf, contsub=contsub), u, v, su, sv)
    Vf = jm.visibilities_rrl(meta["rrl"], u, v, rf, formal=True)
    flux = jm.flux_rrl(meta["rrl"], rf, formal=True)
    check_maps("flux_rrl", Vf, flux, u, v, su, sv)


@pytest.mark.parametrize("formal", [False, True])
def test_visibilities_vs_time(eng, tmp_path_factory, formal):
    jm = model(eng, "tilted", tmp_path_factory)
    freqs = np.asarray(U.load_golden("tilted")[0]["freqs"], dtype=np.float64)[:2]
    times = np.array([0.9, 0.2, 0.4]) * YEAR
    u, v, su, sv = baselines(jm, freqs)
    V = jm.visibilities_vs_time(times, u, v, freqs, formal=formal)
    assert V.shape == (3, 2, 5) and V.dtype == np.complex128
    for e, t in enumerate(times):
        jm.time = float(t)
        check_maps("vs_time formal" if formal else "vs_time", V[e], jm.flux_ff(freqs, formal=formal),
                   u, v, su, sv)
        assert np.array_equal(V[e], jm.visibilities_ff(u, v, freqs, formal=formal))
    # chunks of one epoch give the same bits
    jm.VIS_STACK_BYTES = 1
    try:
        assert np.array_equal(jm.visibilities_vs_time(times, u, v, freqs, formal=formal), V)
    finally:
        del jm.VIS_STACK_BYTES
    assert np.abs(V[0] - V[1]).max() > 0


def test_visibilities_vs_time_jac(eng, tmp_path_factory):
    jm = model(eng, "tilted", tmp_path_factory)
    freqs = np.asarray(U.load_golden("tilted")[0]["freqs"], dtype=np.float64)[:2]
    times = np.array([0.9, 0.2, 0.4]) * YEAR
    u, v, su, sv = baselines(jm, freqs)
    V, dV = jm.visibilities_vs_time_jac(times, u, v, freqs)
    slots = jm._ejection_slots()
    assert len(slots) >= 2 and dV.shape == (3, 2, len(slots), 3, 5) and dV.dtype == np.complex128
    assert np.array_equal(V, jm.visibilities_vs_time(times, u, v, freqs, formal=True))
    # the derivative maps the call transformed, read back
    _, (ctau, cflux) = jm._channel_coeffs(freqs)
    dmaps = eng.ff_formal_grad(jm.device_fields, jm._rjp_bursts(), [float(t) for t in times],
                               jm.gff_mode, ctau, cflux, want_maps=True)[2].cpu().numpy()
    dmaps = dmaps.reshape(3, 2, -1, jm.nx, jm.nz)
    jac = jm.flux_vs_time_jac(times, freqs, formal=True)[1]
    P = jm.nx * jm.nz
    for e in range(3):
        for f in range(2):
            a, b = su[f] * u, sv[f] * v
            bnd = R.bound(a, b, jm.nx, jm.nz) + R.U          # + the product with the chain factor
            for i, (k, chain) in enumerate(slots):
                for c in range(3):
                    dm = dmaps[e, f, k + c]
                    S = R.sum_abs(dm) * abs(chain[c])
                    assert S > 0
                    # zero spacing: the total's derivative, summed in another order
                    assert dV[e, f, i, c, 0].imag == 0.0
                    assert abs(dV[e, f, i, c, 0].real - jac[e, f, i, c]) <= (P + 4) * R.U * S
                    note("dV", dV[e, f, i, c], R.vis_ref(dm, a, b) * R.LD(chain[c]), S, bnd)
    assert np.abs(dV[..., 1:].imag).max() > 0
    # chunks of one epoch give the same bits
    jm.VIS_STACK_BYTES = 1
    try:
        V1, dV1 = jm.visibilities_vs_time_jac(times, u, v, freqs)
    finally:
        del jm.VIS_STACK_BYTES
    assert np.array_equal(V1, V) and np.array_equal(dV1, dV)
