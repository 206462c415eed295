"""rjp_uv_tracks and rjp_vis_noise (K16, observe.hip) through the C-ABI, RTEngine, JetModel's
`uv_tracks` / `observe_ff` and `Pipeline.execute(simobserve=True, antenna_configs=...)`, against
tests/observe_ref.py: Philox4x32-10 in integers, everything that rounds in long double, at the
bounds derived there ((12 u + 2.1e-14)(|bx| + |by| + |bz|) per track component;
u |out| + sigma s r (12 u + 2.1e-14) per noise part; u = 2^-53), which
tests/test_observe_reference_cpu.py holds to a float64 emulation (inside) and nine planted mistakes
(outside).  The module prints the worst |got - ref| / bound per group."""
import copy
import os

import numpy as np
import pytest

from tests import gpu_util as U
from tests import observe_ref as R

pytestmark = pytest.mark.gpu
YEAR = 31557600.0
LD = np.longdouble
WORST = {}
POISON = -7.5
PAD = 64                                  # doubles of guard band on either side of every output
FIXTURE = os.path.join(U.GOLDEN, "antenna_configs", "vla.a.cfg")
N_T = (1, 2, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()
    print("\nworst |got - ref| / bound per group: " +
          ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def note(kind, got, want, bound):
    """NaN exactly where the reference has NaN, +-inf equal, the rest inside the bound."""
    got, want, bound = (np.asarray(x) for x in (got, want, bound))
    nan = np.isnan(want.astype(np.float64))
    assert np.array_equal(np.isnan(got), nan), (kind, "NaN pattern")
    inf = np.isinf(want.astype(np.float64))
    assert np.array_equal(got[inf], want[inf].astype(np.float64)), (kind, "infinities")
    ok = ~nan & ~inf
    err = np.abs(got[ok].astype(LD) - want[ok]).astype(np.float64)
    b = np.broadcast_to(bound, got.shape)[ok]
    assert np.all(err[b == 0.0] == 0.0), (kind, "exact entries")
    r = float(np.max(err[b > 0.0] / b[b > 0.0])) if np.any(b > 0.0) else 0.0
    WORST[kind] = max(WORST.get(kind, 0.0), r)
    assert r <= 1.0, (kind, r)


def dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(eng.device)


def guarded(eng, n):
    import torch
    return torch.full((n + 2 * PAD,), POISON, dtype=torch.float64, device=eng.device)


def inner(t, n):
    assert bool((t[:PAD] == POISON).all()) and bool((t[PAD + n:] == POISON).all()), "guard band"
    return t[PAD:PAD + n].cpu().numpy()


def arr(a):
    from rajepy_amd import _lib
    return None if a is None else _lib.dbl_array(a)


def ptr(t):
    return None if t is None else t.data_ptr()


# ---- 1: tracks ---------------------------------------------------------------------------------------
def raw_tracks(eng, xyz, n_ant, gha, n_t, sd, cd, up, sme, u, v, w, ctx=True):
    return eng.lib.rjp_uv_tracks(eng.ctx if ctx else None, arr(xyz), n_ant, arr(gha), n_t, sd, cd,
                                 arr(up), sme, ptr(u), ptr(v), ptr(w), eng._stream())


def call_tracks(eng, xyz, gha, sd, cd, up=None, sme=0.0, want_w=True):
    A, T = len(xyz), len(gha)
    n = T * (A * (A - 1) // 2)
    g = [guarded(eng, n) for _ in range(3 if want_w else 2)]
    r = raw_tracks(eng, xyz, A, gha, T, sd, cd, up, sme, g[0][PAD:], g[1][PAD:],
                   g[2][PAD:] if want_w else None)
    assert r == T * ((A * (A - 1) // 2 + 255) // 256), eng.lib.rjp_last_error(eng.ctx)
    eng.synchronize()
    return [inner(t, n).reshape(T, -1) for t in g]


def array_of(n_ant):
    if n_ant == 27:
        xyz = R.read_fixture(FIXTURE)[1]
        from rajepy_amd import engine as E
        return xyz, E.geodetic(xyz).up
    return R.random_array(n_ant, seed=100 + n_ant)


def hour_angles(n_t, seed):
    """Greenwich hour angles [turns] around the array's meridian (lon -107.6 deg: GHA = H + 0.299),
    some beyond a turn, so that the exact reduction is used."""
    rng = np.random.default_rng(seed)
    return 107.6 / 360. + rng.uniform(-0.45, 0.45, n_t) + rng.integers(-3, 4, n_t)


@pytest.mark.parametrize("n_ant", (2, 3, 27, 65, 255))
def test_tracks_against_the_reference(eng, n_ant):
    """2 to 255 antennas (1 to 32385 pairs: one thread, one ragged workgroup, 127 workgroups; past
    2^15 pairs a single-precision pair decode fails), 1 to 257 integrations, with and without
    d_w and h_up; the elevation limit flags some antennas at some times."""
    xyz, up = array_of(n_ant)
    dec = np.radians(20.0 + n_ant % 7)
    sd, cd = float(np.sin(dec)), float(np.cos(dec))
    for c, n_t in enumerate(N_T if n_ant <= 65 else (1, 65)):
        gha = hour_angles(n_t, 7 * n_ant + n_t)
        lim = float(np.sin(np.radians(8.0)))
        for with_up in (False, True):
            want_w = (c + with_up) % 2 == 0 or n_t == 65
            ref = R.tracks_ref(xyz, gha, sd, cd, up if with_up else None, lim)
            got = call_tracks(eng, xyz, gha, sd, cd, up if with_up else None, lim, want_w)
            for name, g in zip("uvw", got):
                note("tracks " + name, g, ref[name], ref["bound"][None, :])
            if with_up:
                assert ref["margin"] > 1e-9, "no antenna sits on the limit"
                if n_t >= 63:
                    assert ref["flag"].any() and not ref["flag"].all(), "both kinds are present"
    # the fixture's rigid fact on the device: |(u, v, w)| = |b|
    u, v, w = call_tracks(eng, xyz, hour_angles(2, 1), sd, cd)
    b = np.linalg.norm(xyz[R.pairs(n_ant)[1]] - xyz[R.pairs(n_ant)[0]], axis=1)
    assert np.allclose(np.sqrt(u ** 2 + v ** 2 + w ** 2), b[None, :], rtol=1e-12, atol=0)


def test_tracks_flags_nan_hour_angle_and_repeat(eng):
    """A limit high enough to flag antennas at the ends of the track, a NaN and an infinite hour
    angle (their integrations are flagged whole, nothing else is), and the same bits again."""
    xyz, up = array_of(27)
    dec = np.radians(-20.0)
    sd, cd = float(np.sin(dec)), float(np.cos(dec))
    gha = 107.6184 / 360. + np.linspace(-0.3, 0.3, 65)
    gha[7], gha[40] = np.nan, np.inf
    # the limit: between the 13th and the 14th of the antennas' elevations at integration 12 (the
    # array is 36 km across: its antennas see the source 0.3 deg apart), so that this integration
    # has antennas, and baselines, on both sides
    G = 2 * np.pi * gha[12]
    e12 = np.sort(up @ np.array([cd * np.cos(G), -cd * np.sin(G), sd]))
    lim = float(0.5 * (e12[12] + e12[13]))
    ref = R.tracks_ref(xyz, gha, sd, cd, up, lim)
    assert ref["margin"] > 1e-9
    fin = np.isfinite(gha)
    assert ref["flag"][~fin].all() and ref["flag"][fin].any() and not ref["flag"][fin].all()
    partly = [t for t in range(65) if ref["flag"][t].any() and not ref["flag"][t].all()]
    assert partly, "an integration with some antennas below the limit and some above"
    a = call_tracks(eng, xyz, gha, sd, cd, up, lim)
    b = call_tracks(eng, xyz, gha, sd, cd, up, lim)
    for name, x, y in zip("uvw", a, b):
        assert np.array_equal(x.view(np.int64), y.view(np.int64)), "a repeated call: the same bits"
        assert np.array_equal(np.isnan(x), ref["flag"])
        note("tracks flagged " + name, x, ref[name], ref["bound"][None, :])


def test_tracks_refusals(eng):
    """Every refusal with its message, before anything is enqueued: no output byte is touched."""
    from rajepy_amd import _lib
    xyz, up = array_of(3)
    gha = np.array([0.1, 0.2])
    n = 2 * 3
    g = [guarded(eng, n) for _ in range(3)]
    o = [t[PAD:] for t in g]
    s, c = float(np.sin(0.3)), float(np.cos(0.3))
    bad_xyz = xyz.copy()
    bad_xyz[2, 1] = np.inf
    cases = [
        ("null", (None, 3, gha, 2, s, c, up, 0.1, o[0], o[1], o[2])),
        ("null", (xyz, 3, None, 2, s, c, up, 0.1, o[0], o[1], o[2])),
        ("null", (xyz, 3, gha, 2, s, c, up, 0.1, None, o[1], o[2])),
        ("null", (xyz, 3, gha, 2, s, c, up, 0.1, o[0], None, o[2])),
        ("n_ant", (xyz, 1, gha, 2, s, c, up, 0.1, o[0], o[1], o[2])),
        ("n_t", (xyz, 3, gha, 0, s, c, up, 0.1, o[0], o[1], o[2])),
        ("xyz", (bad_xyz, 3, gha, 2, s, c, up, 0.1, o[0], o[1], o[2])),
        ("dec", (xyz, 3, gha, 2, float("nan"), c, up, 0.1, o[0], o[1], o[2])),
        ("dec", (xyz, 3, gha, 2, s, float("inf"), up, 0.1, o[0], o[1], o[2])),
        ("unit", (xyz, 3, gha, 2, s, c * (1 + 1e-11), up, 0.1, o[0], o[1], o[2])),
    ]
    for key, a in cases:
        assert raw_tracks(eng, *a) == _lib.RJP_ERR_ARG, key
        assert eng.lib.rjp_last_error(eng.ctx).decode() == R.TRACKS_MESSAGES[key]
    # 65536 antennas have 2^31 - 32768 pairs: two integrations are one too many (checked before
    # any table is read beyond the positions, which are 1.5 MB of zeros here)
    big = np.zeros((65536, 3))
    assert raw_tracks(eng, big, 65536, gha, 2, s, c, None, 0.0, o[0], o[1], o[2]) == _lib.RJP_ERR_ARG
    assert eng.lib.rjp_last_error(eng.ctx).decode() == R.TRACKS_MESSAGES["size"]
    assert raw_tracks(eng, xyz, 3, gha, 2, s, c, up, 0.1, o[0], o[1], o[2], ctx=False) == _lib.RJP_ERR_ARG
    eng.synchronize()
    for t in g:
        assert bool((t == POISON).all()), "a refusal writes nothing"
    with pytest.raises(ValueError, match="n_ant >= 2"):
        eng.uv_tracks(xyz[:1], gha, 0.3)
    with pytest.raises(ValueError, match="go together"):
        eng.uv_tracks(xyz, gha, 0.3, up=up)
    # the wrapper: tensors stay on the device, the same numbers as the raw call
    u, v, w = eng.uv_tracks(xyz, gha, 0.3, up=up, min_el_rad=0.1)
    ref = call_tracks(eng, xyz, gha, s, c, up, float(np.sin(0.1)))
    assert u.is_cuda and np.array_equal(u.cpu().numpy(), ref[0], equal_nan=True)
    assert np.array_equal(w.cpu().numpy(), ref[2], equal_nan=True) and eng.last_uv_tracks_tiles == 2
    assert eng.uv_tracks(xyz, gha, 0.3, want_w=False)[2] is None


# ---- 2: noise ----------------------------------------------------------------------------------------
def raw_noise(eng, vis, n_maps, n_vis, sigma, s, seed, k0, m0, out, ctx=True):
    return eng.lib.rjp_vis_noise(eng.ctx if ctx else None, ptr(vis), n_maps, n_vis, arr(sigma),
                                 ptr(s), seed, k0, m0, ptr(out), eng._stream())


def call_noise(eng, V, sigma, s, seed, k0=0, m0=0, in_place=False):
    M, K = V.shape[:2]
    g = guarded(eng, 2 * M * K)
    src = dev(eng, V.reshape(-1))
    if in_place:
        g[PAD:PAD + 2 * M * K] = src
        src = g[PAD:]
    r = raw_noise(eng, src, M, K, sigma, None if s is None else dev(eng, s), seed, k0, m0, g[PAD:])
    assert r == M * ((K + 255) // 256), eng.lib.rjp_last_error(eng.ctx)
    eng.synchronize()
    return inner(g, 2 * M * K).reshape(M, K, 2)


def vis_case(M, K, seed, specials=True):
    rng = np.random.default_rng(seed)
    V = rng.normal(0, 3, (M, K, 2)) * 10.0 ** rng.integers(-3, 3, (M, K, 1))
    if specials and K >= 63:
        V[0, 3] = (np.nan, 1.0)
        V[-1, 5] = (np.inf, -np.inf)
        V[0, 9] = (-0.0, 0.0)
        V[-1, 11] = (-0.0, -0.0)
    elif specials:
        V[0, 0] = (-0.0, 0.0)
    return V


SIGMAS = {1: [0.7], 2: [0.0, 2.5e-3], 3: [1.25, 0.0, 40.0]}


@pytest.mark.parametrize("n_vis", (1, 63, 64, 65, 255, 256, 257, 2 ** 18))
def test_noise_against_the_reference(eng, n_vis):
    """1 to 3 maps with their own sigma, one of them 0 (copied bit for bit, -0.0 included), with
    and without d_s, one thread to 1024 workgroups per map; NaN and infinite visibilities; in
    place and a repeated call give the same bits."""
    for c, M in enumerate((1, 2, 3) if n_vis < 2 ** 18 else (2,)):
        V = vis_case(M, n_vis, 31 * n_vis + M)
        s = None if (c + n_vis) % 2 else np.random.default_rng(n_vis).uniform(0.5, 2.0, n_vis)
        sigma = SIGMAS[M]
        ref, bound, copy_ = R.noise_ref(V, sigma, s, R.SEED)
        got = call_noise(eng, V, sigma, s, R.SEED)
        note("noise", got, ref, bound)
        for m in np.nonzero(copy_)[0]:
            assert np.array_equal(got[m].view(np.int64), V[m].view(np.int64)), "sigma = 0: the input's bits"
        if M > 1 and n_vis > 1:
            live = ~copy_
            assert np.any(got[live] != V[live]), "noise was added"
        again = call_noise(eng, V, sigma, s, R.SEED, in_place=True)
        assert np.array_equal(got.view(np.int64), again.view(np.int64)), "in place: the same bits"


def test_noise_offsets_chunks_and_the_carry(eng):
    """k0 = 2^32 - 100 with 257 visibilities crosses into the second counter word; m0 > 0; three
    uneven chunks in k and two in m reproduce the bits of the whole; another seed, other bits."""
    M, K = 3, 257
    V = vis_case(M, K, 5)
    sigma = [0.5, 1.5, 2.5]
    s = np.random.default_rng(2).uniform(0.5, 2.0, K)
    k0, m0 = 2 ** 32 - 100, 5
    seed = (0x9abcdef0 << 32) | 0x12345678              # both key words in use
    ref, bound, _ = R.noise_ref(V, sigma, s, seed, k0, m0)
    whole = call_noise(eng, V, sigma, s, seed, k0, m0)
    note("noise carry", whole, ref, bound)
    nocarry = R.noise_ref(V, sigma, s, seed, k0, m0, carry=False)[0]
    fin_k = np.isfinite(V[:, 100:]).all(axis=(0, 2))
    assert np.abs(nocarry[:, 100:][:, fin_k] - ref[:, 100:][:, fin_k]).max() > 1e-3, "the carry matters from k = 100 on"
    parts = np.zeros_like(whole)
    for a, b in ((0, 1), (1, 130), (130, 257)):
        for ma, mb in ((0, 2), (2, 3)):
            parts[ma:mb, a:b] = call_noise(eng, np.ascontiguousarray(V[ma:mb, a:b]), sigma[ma:mb],
                                           s[a:b], seed, k0 + a, m0 + ma)
    assert np.array_equal(parts.view(np.int64), whole.view(np.int64)), "chunks: the bits of the whole"
    other = call_noise(eng, V, sigma, s, seed + 1, k0, m0)
    fin = np.isfinite(V)
    assert np.all(other[fin] != whole[fin])
    # far along the counter: k0 + n_vis = 2^63 - 1, the largest admitted
    far = 2 ** 63 - 1 - K
    note("noise far", call_noise(eng, V, sigma, s, seed, far, 2 ** 31 - 1 - M),
         *R.noise_ref(V, sigma, s, seed, far, 2 ** 31 - 1 - M)[:2])


def test_noise_non_finite_scale(eng):
    """A NaN or infinite d_s[k] makes visibility k NaN in every map, the one with sigma = 0 too;
    its neighbours are untouched by it."""
    M, K = 3, 65
    V = vis_case(M, K, 9, specials=False)
    s = np.ones(K)
    s[4], s[64] = np.nan, np.inf
    ref, bound, _ = R.noise_ref(V, SIGMAS[3], s, R.SEED)
    got = call_noise(eng, V, SIGMAS[3], s, R.SEED)
    assert np.isnan(got[:, [4, 64]]).all() and np.isfinite(np.delete(got, [4, 64], axis=1)).all()
    note("noise flagged", got, ref, bound)


def test_noise_refusals(eng):
    """Every refusal with its message; nothing is written."""
    import torch
    from rajepy_amd import _lib
    M, K = 2, 5
    g = guarded(eng, 2 * M * K)
    o = g[PAD:]
    vis = dev(eng, np.zeros(2 * M * K))
    sg = [1.0, 2.0]
    cases = [
        ("null", (None, M, K, sg, None, 1, 0, 0, o)),
        ("null", (vis, M, K, None, None, 1, 0, 0, o)),
        ("null", (vis, M, K, sg, None, 1, 0, 0, None)),
        ("sizes", (vis, 0, K, sg, None, 1, 0, 0, o)),
        ("sizes", (vis, M, 0, sg, None, 1, 0, 0, o)),
        ("sigma", (vis, M, K, [1.0, -1e-300], None, 1, 0, 0, o)),
        ("sigma", (vis, M, K, [np.nan, 1.0], None, 1, 0, 0, o)),
        ("sigma", (vis, M, K, [1.0, np.inf], None, 1, 0, 0, o)),
        ("k0", (vis, M, K, sg, None, 1, -1, 0, o)),
        ("k0", (vis, M, K, sg, None, 1, 2 ** 63 - K, 0, o)),
        ("m0", (vis, M, K, sg, None, 1, 0, -1, o)),
        ("m0", (vis, M, K, sg, None, 1, 0, 2 ** 31 - M, o)),
    ]
    for key, a in cases:
        assert raw_noise(eng, *a) == _lib.RJP_ERR_ARG, key
        assert eng.lib.rjp_last_error(eng.ctx).decode() == R.NOISE_MESSAGES[key], key
    assert raw_noise(eng, vis, M, K, sg, None, 1, 0, 0, o, ctx=False) == _lib.RJP_ERR_ARG
    eng.synchronize()
    assert bool((g == POISON).all()), "a refusal writes nothing"
    # the wrapper: complex in, complex out; in place returns the tensor it was given
    Vc = torch.view_as_complex(dev(eng, vis_case(2, 65, 1, False).reshape(-1)).reshape(2, 65, 2))
    out = eng.vis_noise(Vc, [0.0, 1.0], seed=R.SEED)
    assert out.dtype == torch.complex128 and out.data_ptr() != Vc.data_ptr()
    assert bool((out[0] == Vc[0]).all()) and bool((out[1] != Vc[1]).all())
    keep = out.clone()
    same = eng.vis_noise(Vc, [0.0, 1.0], seed=R.SEED, out=Vc)
    assert same.data_ptr() == Vc.data_ptr() and bool((Vc == keep).all())
    with pytest.raises(ValueError, match="one per map"):
        eng.vis_noise(Vc, [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="one entry per visibility"):
        eng.vis_noise(Vc, 1.0, s=np.ones(3))


# ---- 3: the golden example model through JetModel ------------------------------------------------------
def _params(tag):
    p = copy.deepcopy(U.load_golden(tag)[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


_MODELS = {}
T_OBS, T_INT, MIN_EL = 1200., 60., 20.
SHAPE = (48, 40)


def model(eng, tmp_path_factory):
    from rajepy_amd import classes, logger
    if "jm" not in _MODELS:
        log = logger.Log(str(tmp_path_factory.mktemp("observe") / "model.log"), verbose=False)
        _MODELS["jm"] = classes.JetModel(_params("cfg1_example"), log=log, engine=eng)
        _MODELS["jm"].time = 1.0 * YEAR
    return _MODELS["jm"]


def target_and_site(jm):
    """(dec [rad], lat0, lon0 [deg], xyz, up) without `JetModel.uv_tracks`."""
    from rajepy_amd import engine as E
    from rajepy_amd.miscellaneous import functions as miscf
    tg = jm.params["target"]
    dec = np.radians(miscf.sexagesimal_to_deg(tg["ra"], tg["dec"])[1])
    xyz = R.read_fixture(FIXTURE)[1]
    g = E.geodetic(xyz)
    return dec, g.lat0_deg, g.lon0_deg, xyz, g.up


def grid_of(jm, tracks, freq):
    from rajepy_amd import engine as E
    return E.observation_grid(tracks.max_baseline_m, freq, 1.0)[0]


def test_model_uv_tracks_against_the_reference_fed_the_same_plan(eng, tmp_path_factory):
    jm = model(eng, tmp_path_factory)
    dec, lat0, lon0, xyz, up = target_and_site(jm)
    tr = jm.uv_tracks(FIXTURE, T_OBS, T_INT, min_el_deg=MIN_EL)
    assert len(tr.ha_h) == 20 and np.all(tr.day == 0) and tr.u_m.is_cuda
    assert np.allclose(tr.ha_h, (np.arange(20) - 9.5) * 60. / 86164.0905 * 24., rtol=0, atol=1e-15)
    a1, a2 = R.pairs(27)
    assert np.array_equal(tr.ant1, a1) and np.array_equal(tr.ant2, a2)
    assert tr.max_baseline_m == np.linalg.norm(xyz[a2] - xyz[a1], axis=1).max()
    ref = R.tracks_ref(xyz, tr.ha_h / 24. - lon0 / 360., float(np.sin(dec)), float(np.cos(dec)), up,
                       float(np.sin(np.radians(MIN_EL))))
    assert not ref["flag"].any() and ref["margin"] > 1e-9
    for name, t in (("u", tr.u_m), ("v", tr.v_m), ("w", tr.w_m)):
        note("model tracks " + name, t.cpu().numpy().reshape(20, 351), ref[name], ref["bound"][None, :])
    # None: the horizon for the plan, and no flags
    free = jm.uv_tracks(FIXTURE, T_OBS, T_INT)
    assert np.array_equal(free.u_m.cpu().numpy(), tr.u_m.cpu().numpy())


def test_observe_ff_without_noise_is_clean_image_ff_at_the_tracks(eng, tmp_path_factory):
    jm = model(eng, tmp_path_factory)
    freqs = np.array([4.9e9, 5.1e9])
    tr = jm.uv_tracks(FIXTURE, T_OBS, T_INT, min_el_deg=MIN_EL)
    kw = dict(shape=SHAPE, cell_as=grid_of(jm, tr, 5e9), niter=40, mfs=True, imfit=True,
              weighting="briggs", robust=0.5, mask=(8, 40, 6, 34))
    obs = jm.observe_ff(FIXTURE, freqs, T_OBS, T_INT, min_el_deg=MIN_EL, sigma_jy=0., seed=3, **kw)
    want = jm.clean_image_ff(tr.u_m, tr.v_m, freqs, **kw)
    for name in ("image", "residual", "model", "peak_residual"):
        a, b = getattr(obs.clean, name), getattr(want, name)
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), name
    assert obs.clean.imfit[0]["peak"] == want.imfit[0]["peak"] and obs.clean.imfit[0]["Ierr"]["val"] is None
    assert np.array_equal(obs.vis, obs.vis_clean) and obs.vis.shape == (2, 7020)
    assert np.array_equal(obs.vis_clean, jm.visibilities_ff(tr.u_m, tr.v_m, freqs))
    assert np.all(obs.sigma == 0.) and np.all(obs.image_rms == 0.)
    # a UVTracks made earlier is taken as it is; no noise parameters at all is noise-free too
    again = jm.observe_ff(tr, freqs, T_OBS, T_INT, **kw)
    assert np.array_equal(again.clean.image.view(np.int64), want.image.view(np.int64))
    with pytest.raises(ValueError, match="not both"):
        jm.observe_ff(tr, freqs, T_OBS, T_INT, sigma_jy=1., sefd_jy=1., chanwidth_hz=1e6, **kw)
    with pytest.raises(ValueError, match="chanwidth_hz"):
        jm.observe_ff(tr, freqs, T_OBS, T_INT, sefd_jy=1., **kw)


def test_observe_ff_with_noise(eng, tmp_path_factory):
    """vis - vis_clean is the reference's noise; image_rms follows sqrt(sum w'^2 sigma^2) / sum w'
    of the weights actually used; CLEAN stops at nsigma image_rms or at niter; imfit's errors come
    from image_rms."""
    jm = model(eng, tmp_path_factory)
    freqs = np.array([4.9e9, 5.1e9])
    tr = jm.uv_tracks(FIXTURE, T_OBS, T_INT, min_el_deg=MIN_EL)
    cell = grid_of(jm, tr, 5e9)
    peak = float(np.abs(jm.visibilities_ff([0.], [0.], freqs)).max())
    sigma = np.array([2.0, 0.5]) * peak                 # per visibility: 0.024 and 0.006 peak per image
    kw = dict(shape=SHAPE, cell_as=cell, niter=60, weighting="briggs", robust=0.5)
    obs = jm.observe_ff(tr, freqs, T_OBS, T_INT, sigma_jy=sigma, seed=R.SEED, nsigma=3., imfit=True, **kw)
    v0 = np.stack([obs.vis_clean.real, obs.vis_clean.imag], axis=-1)
    ref, bound, _ = R.noise_ref(v0, sigma, None, R.SEED)
    note("observe_ff noise", np.stack([obs.vis.real, obs.vis.imag], axis=-1), ref, bound)
    iw, _ = jm.imaging_weights(tr.u_m, tr.v_m, freqs, shape=SHAPE, cell_as=cell, weighting="briggs")
    want = np.sqrt((iw ** 2 * sigma[:, None] ** 2).sum(axis=1)) / iw.sum(axis=1)
    assert np.allclose(obs.image_rms, want, rtol=1e-13, atol=0) and np.all(obs.image_rms > 0)
    for f in range(2):
        n = len(obs.clean.components[f])
        assert n == 60 or obs.clean.peak_residual[f] <= 3. * obs.image_rms[f], (f, n)
        assert obs.clean.imfit[f]["Ierr"]["val"] is not None
    assert len(obs.clean.components[0]) < 60, "the noisier image stops at its threshold"
    # threshold_jy above nsigma image_rms decides; nsigma = 0 leaves threshold_jy alone
    high = jm.observe_ff(tr, freqs, T_OBS, T_INT, sigma_jy=sigma, seed=R.SEED, nsigma=3.,
                         threshold_jy=0.9 * peak, **kw)
    assert all(len(c) <= 2 for c in high.clean.components)
    mfs = jm.observe_ff(tr, freqs, T_OBS, T_INT, sigma_jy=sigma, seed=R.SEED, nsigma=3., mfs=True, **kw)
    iwm, _ = jm.imaging_weights(tr.u_m, tr.v_m, freqs, shape=SHAPE, cell_as=cell, weighting="briggs", mfs=True)
    assert mfs.image_rms.shape == (1,) and np.allclose(
        mfs.image_rms[0], np.sqrt((iwm ** 2 * sigma[:, None] ** 2).sum()) / iwm.sum(), rtol=1e-13)
    assert np.array_equal(mfs.vis, obs.vis), "the same seed, the same visibilities"


def test_flagged_baselines_drop_out_of_image_and_beam(eng, tmp_path_factory):
    """A track that runs into the elevation limit: the flagged baselines are NaN in (u, v, w) and
    in the visibilities, and image and beam leave them out alike -- the beam is 1 at its centre."""
    jm = model(eng, tmp_path_factory)
    dec, lat0, lon0, xyz, up = target_and_site(jm)
    lat, el = np.radians(lat0), np.radians(MIN_EL)
    h_el = np.degrees(np.arccos((np.sin(el) - np.sin(lat) * np.sin(dec)) / (np.cos(lat) * np.cos(dec)))) / 15.
    tr = jm.uv_tracks(FIXTURE, T_OBS, T_INT, min_el_deg=MIN_EL, hourangle_h=h_el - 0.1)
    flag = np.isnan(tr.u_m.cpu().numpy())
    ref = R.tracks_ref(xyz, tr.ha_h / 24. - lon0 / 360., float(np.sin(dec)), float(np.cos(dec)), up,
                       float(np.sin(el)))
    assert ref["margin"] > 1e-9 and np.array_equal(flag.reshape(20, 351), ref["flag"])
    assert flag.any() and not flag.all()
    freqs = np.array([5e9])
    cell = grid_of(jm, tr, 5e9)
    for weighting in (None, "briggs"):
        psf = jm.dirty_beam(tr.u_m, tr.v_m, freqs, shape=(33, 31), cell_as=cell, weighting=weighting)
        assert abs(psf[0, 16, 15] - 1.0) <= 1e-12 and np.isfinite(psf).all()
        obs = jm.observe_ff(tr, freqs, T_OBS, T_INT, sigma_jy=0., shape=(33, 31), cell_as=cell, niter=20,
                            weighting=weighting)
        assert np.array_equal(np.isnan(obs.vis_clean[0]), flag) and np.isfinite(obs.clean.image).all()
        # the same image as from the unflagged baselines alone (other sums, so not the same bits:
        # 1e-9 of the flux is 10^6 roundings of it), on the flux scale of the model (the source
        # spans 0.6 of the beam: its peak lies within a tenth of its flux)
        total = float(np.abs(jm.visibilities_ff([0.], [0.], freqs))[0, 0])
        keep = dev(eng, (~flag).astype(np.float64)).bool()
        want = jm.clean_image_ff(tr.u_m[keep], tr.v_m[keep], freqs, shape=(33, 31), cell_as=cell, niter=20,
                                 weighting=weighting)
        assert np.abs(obs.clean.image - want.image).max() <= 1e-9 * total
        assert abs(obs.clean.image[0].max() - total) < 0.1 * total


# ---- 4: the pipeline -----------------------------------------------------------------------------------
def test_pipeline_simobserve_products(tmp_path, monkeypatch):
    from rajepy_amd import classes, fits, logger
    monkeypatch.delenv("RAJEPY_ANTENNA_CONFIGS", raising=False)
    from tests.test_host_logic import example_params, pline_params
    cfg_dir = os.path.join(U.GOLDEN, "antenna_configs")

    def run(tag, seed, **kw):
        dcy = str(tmp_path / tag)
        os.makedirs(dcy)
        log = logger.Log(os.path.join(dcy, "p.log"), verbose=False)
        pp = pline_params(dcy)
        pp["continuum"]["t_ints"] = np.array([60])
        pl = classes.Pipeline(classes.JetModel(example_params(), log=log), pp, log=log)
        pl.execute(simobserve=True, verbose=False, resume=False, seed=seed, **kw)
        return pl, log

    pl, log = run("a", 7, antenna_configs=cfg_dir, sefd_jy=300.)
    assert [x.obs_type for x in pl.runs] == ["continuum", "continuum", "rrl"]
    for x in pl.runs:
        for k in ("ms_clean", "ms_noisy", "clean_image"):
            assert os.path.exists(x.products[k]), k
    line = pl.runs[2]
    assert "imfit" not in line.results and fits.read(line.products["clean_image"])[0].shape == (4, 500, 500)
    r = pl.runs[1]
    img, cards = fits.read(r.products["clean_image"])
    kv = {c[:8].strip(): c[10:30].strip() for c in cards if c[8:10] == "= "}
    ms = np.load(r.products["ms_noisy"])
    assert ms["vis"].shape == (2, 7020) and ms["u"].shape == (7020,) and ms["ant2"][350] == 26
    bmax = np.sqrt(ms["u"] ** 2 + ms["v"] ** 2 + ms["w"] ** 2).max()
    from rajepy_amd import _constants as con
    cell = float("%.6f" % (np.degrees(con.c / 5e9 / bmax) * 3600. / 4.))
    assert img.shape == (1, 500, 500) and float(kv["CDELT2"]) == pytest.approx(cell / 3600., rel=1e-12)
    # (a card holds 20 characters: the sign costs the negative increment a digit)
    assert float(kv["CDELT1"]) == pytest.approx(-cell / 3600., rel=1e-12) and kv["BUNIT"].strip("' ") == "Jy/beam"
    fit = r.results["imfit"]
    assert {"peak", "I", "Ierr", "maj_as", "min_as", "pa_deg", "deconvolved", "x0", "z0"} <= set(fit)
    assert set(fit["I"]) == {"val", "unit"} and fit["Ierr"]["val"] > 0
    print("imfit I = %.4e +- %.1e Jy, flux %.4e Jy" % (fit["I"]["val"], fit["Ierr"]["val"], r.results["flux"]))
    assert abs(fit["I"]["val"] - r.results["flux"]) <= 5. * fit["Ierr"]["val"]
    # the same seed: identical files; another seed: another ms_noisy, the same ms_clean
    same, _ = run("b", 7, antenna_configs=cfg_dir, sefd_jy=300.)
    other, _ = run("c", 8, antenna_configs=cfg_dir, sefd_jy=300.)
    rd = lambda p, k: b"".join(open(x.products[k], "rb").read() for x in p.runs)
    for k in ("ms_clean", "ms_noisy", "clean_image"):
        assert rd(same, k) == rd(pl, k), k
    assert rd(other, "ms_clean") == rd(pl, "ms_clean") and rd(other, "ms_noisy") != rd(pl, "ms_noisy")
    # without a directory: the old warning, no product
    none, log0 = run("d", 7)
    assert "ms_noisy" not in none.runs[0].products and "imfit" not in none.runs[0].results
    assert any("CASA synthetic observations are outside the radiative-transfer core and are skipped"
               in str(e) for e in _entries(log0))
    # an array the directory does not hold: an ERROR entry, imfit None, the run still completes
    dcy = str(tmp_path / "e")
    os.makedirs(dcy)
    log = logger.Log(os.path.join(dcy, "p.log"), verbose=False)
    pp = pline_params(dcy)
    pp["continuum"].update(times=np.array([1.]), tscps=np.array([("ALMA", "9")]))
    pp["rrls"]["times"] = np.array([])
    bad = classes.Pipeline(classes.JetModel(example_params(), log=log), pp, log=log)
    bad.execute(simobserve=True, verbose=False, resume=False, antenna_configs=cfg_dir)
    assert bad.runs[0].results["imfit"] is None and bad.runs[0].completed
    assert any("synthetic observation failed" in str(e) for e in _entries(log))


def _entries(log):
    """The text of a Log's entries, however it keeps them."""
    with open(log.filename) as f:
        return f.read().splitlines()


def test_main_cli_writes_the_observation(tmp_path, monkeypatch):
    """python -m rajepy_amd.main -rt -so --antenna-configs DIR --sefd 300 --seed 5 on the example jet:
    the clean image and the two visibility files; without --antenna-configs, none."""
    from rajepy_amd import main as cli
    from tests.test_host_logic import example_params
    monkeypatch.delenv("RAJEPY_ANTENNA_CONFIGS", raising=False)
    model = tmp_path / "model-params.py"

    def lit(v):
        return "np.array(%r)" % v.tolist() if isinstance(v, np.ndarray) else repr(v)

    body = ",\n".join("  %r: {%s}" % (sec, ", ".join("%r: %s" % (k, lit(v)) for k, v in d.items()))
                      for sec, d in example_params().items())
    model.write_text("import numpy as np\nparams = {\n" + body + "\n}\n")

    def pline(out):
        f = tmp_path / (out.name + "-pipeline-params.py")
        f.write_text(
            "import numpy as np\nparams = {'min_el': 20., 'dcys': {'model_dcy': %r},\n"
            " 'continuum': {'times': np.array([1.]), 'freqs': np.array([5e9]), 't_obs': np.array([1200]),\n"
            "   'tscps': np.array([('VLA', 'A')]), 't_ints': np.array([60]), 'bws': np.array([4e8]), 'chanws': np.array([2e8])},\n"
            " 'rrls': {'times': np.array([]), 'lines': np.array(['H66a']), 't_obs': np.array([1200]),\n"
            "   'tscps': np.array([('VLA', 'A')]), 't_ints': np.array([60]), 'bws': np.array([4e5]), 'chanws': np.array([1e5])}}\n"
            % str(out))
        return str(f)
    out = tmp_path / "so"
    pl = cli.main(["-rt", "-so", "--antenna-configs", os.path.join(U.GOLDEN, "antenna_configs"), "--sefd", "300",
                   "--seed", "5", str(model), pline(out)])
    d = out / "Day365" / "5GHz"
    assert os.path.exists(d / "SynObs.vla.a.noisy.imaging.fits")
    assert os.path.exists(d / "SynObs" / "SynObs.vla.a.ms.npz") and os.path.exists(d / "SynObs" / "SynObs.vla.a.noisy.ms.npz")
    assert pl.runs[0].products["clean_image"] == str(d / "SynObs.vla.a.noisy.imaging.fits")
    assert pl.runs[0].results["imfit"]["Ierr"]["val"] > 0
    noisy, clean = np.load(d / "SynObs" / "SynObs.vla.a.noisy.ms.npz"), np.load(d / "SynObs" / "SynObs.vla.a.ms.npz")
    assert np.all(noisy["sigma"] == 300. / np.sqrt(2 * 2 * 2e8 * 60)) and np.all(noisy["vis"] != clean["vis"])
    plain = cli.main(["-rt", "-so", str(model), pline(tmp_path / "plain")])
    assert "clean_image" not in plain.runs[0].products and not os.path.exists(tmp_path / "plain" / "Day365" / "5GHz" / "SynObs")
