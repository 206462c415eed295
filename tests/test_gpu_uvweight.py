"""rjp_uv_weights (K15, uv_weight.hip): uniform and Briggs imaging weights from the (u, v) density,
through the C-ABI, RTEngine.uv_weights and JetModel's imaging methods, against tests/uvweight_ref.py:
the contract restated in Python integers -- the density, sum w and the shift must match BIT FOR
BIT -- and the weights, f2 and sum W^2 in long double at a relative bound derived term by term there
(uniform 2 u, Briggs (cells + 15) u, f2 (cells + 12) u, sum W^2 (cells + 2) u; u = 2^-53), which
tests/test_uvweight_reference_cpu.py holds to a float64 emulation (inside) and five planted
mistakes (outside).  The module prints the worst |got - ref| / bound per group."""
import copy

import numpy as np
import pytest

from tests import gpu_util as U
from tests import uvweight_ref as K
from tests import vis_adjoint_ref as A

pytestmark = pytest.mark.gpu
YEAR = 31557600.0
LD = np.longdouble
WORST = {}
POISON = -7.5
PAD = 64                                  # doubles of guard band on either side of every output
GRIDS = [(1, 1), (5, 3), (16, 8), (64, 64), (67, 131)]
N_VIS = (1, 63, 257, 1000, 5000)
ROBUST = (0.5, -2.0, 2.0, 0.0)


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()
    print("\nworst |got - ref| / bound per group: " +
          ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def note(kind, got, want, bound):
    r = K.worst_ratio(got, want, bound)
    WORST[kind] = max(WORST.get(kind, 0.0), r)
    assert r <= 1.0, (kind, r)


def dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(eng.device)


def raw(eng, n_maps, n_vis, su, sv, u, v, w, nx, nz, mode, robust, wout, stats, dens, work, nbytes,
        ctx=True):
    from rajepy_amd import _lib
    ptr = lambda t: t.data_ptr() if t is not None else None
    return eng.lib.rjp_uv_weights(eng.ctx if ctx else None, n_maps, n_vis,
                                  _lib.dbl_array(su) if su is not None else None,
                                  _lib.dbl_array(sv) if sv is not None else None,
                                  ptr(u), ptr(v), ptr(w), nx, nz, mode, robust, ptr(wout), ptr(stats),
                                  ptr(dens), ptr(work), nbytes, eng._stream())


def guarded(eng, n):
    import torch
    return torch.full((n + 2 * PAD,), POISON, dtype=torch.float64, device=eng.device)


def inner(t, n):
    assert bool((t[:PAD] == POISON).all()) and bool((t[PAD + n:] == POISON).all()), "guard band"
    return t[PAD:PAD + n].cpu().numpy()


def call(eng, su, sv, u, v, w, nx, nz, mode, robust, want=True):
    """One guarded call through the C-ABI -> (wout [M, K], stats [M, 6] or None, density [M, cells]
    or None): guard bands around every output and behind a workspace of exactly the queried size."""
    import torch
    M, Kv, nc = len(su), len(u), K.n_cells(nx, nz)
    wb = eng.lib.rjp_uv_weights_workspace(M, nx, nz, Kv)
    assert wb == K.workspace_bytes(M, nx, nz, Kv)
    work = torch.full((wb + 512,), 0xA5, dtype=torch.uint8, device=eng.device)
    g_w = guarded(eng, M * Kv)
    g_s, g_d = (guarded(eng, M * 6), guarded(eng, M * nc)) if want else (None, None)
    r = raw(eng, M, Kv, su, sv, dev(eng, u), dev(eng, v), None if w is None else dev(eng, w), nx, nz,
            mode, robust, g_w[PAD:], None if g_s is None else g_s[PAD:],
            None if g_d is None else g_d[PAD:], work, wb)
    assert r == K.workgroups(M, Kv), eng.lib.rjp_last_error(eng.ctx)
    eng.synchronize()
    assert bool((work[wb:] == 0xA5).all()), "the workspace's guard band"
    return (inner(g_w, M * Kv).reshape(M, Kv), inner(g_s, M * 6).reshape(M, 6) if want else None,
            inner(g_d, M * nc).reshape(M, nc) if want else None)


def check(kind, eng, su, sv, u, v, w, nx, nz, mode, robust, d=None):
    """The call against the integer restatement (bit for bit) and the long-double weights (bound);
    `d`: the restatement of these inputs when an earlier call made it."""
    wout, stats, dens = call(eng, su, sv, u, v, w, nx, nz, mode, robust)
    d = d or K.integer_density(su, sv, u, v, w, nx, nz)
    r = K.weights(d, w, mode, robust)
    for m in range(len(su)):
        assert np.array_equal(dens[m].view(np.int64), d["W"][m].view(np.int64)), (kind, m, "density")
        assert stats[m, 0] == d["sum_w"][m] and stats[m, 5] == d["s"], (kind, m, stats[m], d["s"])
        assert stats[m, 3] == d["counted"][m] and stats[m, 4] == d["outside"][m], (kind, m)
        note(kind + " sum W^2", [stats[m, 1]], [r["sum_w2"][m]], r["b_sum_w2"][m])
        if mode == K.BRIGGS:
            note(kind + " f2", [stats[m, 2]], [r["f2"][m]], r["b_f2"][m])
        else:
            assert stats[m, 2] == 0.0
        note(kind + (" briggs" if mode == K.BRIGGS else " uniform"), wout[m], r["wout"][m], r["b_wout"][m])
    return wout, stats, dens, d


# ---- 1: shapes and inputs at the bound ---------------------------------------------------------------
@pytest.mark.parametrize("nx,nz", GRIDS)
def test_random_visibilities_against_the_reference(eng, nx, nz):
    """1 x 1 to 67 x 131 cells (odd and even sizes, one tile of the sum of W^2 and several), 1-5000
    visibilities (one workgroup, ragged ones, twenty), 1-3 maps with a scale each, signs included;
    |a| up to 0.7 cycles per cell, so some are out of range; weights over 2^+-20, all ones, none;
    10 % flagged, every kind; 16 x 8 with exact half-integer products, the edge cells, the first
    cell beyond them and +-0."""
    case = 0
    for n_vis in N_VIS:
        for weights in ("wide", None):
            case += 1
            n_maps = 1 + case % 3
            su, sv, u, v, w = K.case(nx, nz, n_vis, n_maps, seed=1000 * nx + nz + case, weights=weights,
                                     ties=(nx, nz) == (16, 8) and n_vis >= 63)
            d = None
            for mode, robust in ((K.UNIFORM, 0.0), (K.BRIGGS, ROBUST[case % 4])):
                d = check("random", eng, su, sv, u, v, w, nx, nz, mode, robust, d)[3]
            if n_vis >= 257 and (nx, nz) != (1, 1):
                assert 0 < min(d["counted"]) and max(d["outside"]) > 0, "both kinds are present"


def test_the_engine_path_gives_the_same_bits(eng):
    su, sv, u, v, w = K.case(16, 8, 257, 3, seed=7, ties=True)
    want, stats, dens = call(eng, su, sv, u, v, w, 16, 8, K.BRIGGS, 0.5)
    got = eng.uv_weights(u, v, su, sv, 16, 8, w=w, want_density=True)
    assert got.shape == (3, 257) and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(eng.last_uv_weight_stats.cpu().numpy(), stats)
    assert np.array_equal(eng.last_uv_weight_density.cpu().numpy(), dens)
    assert eng.last_uv_weight_tiles == K.workgroups(3, 257) == 6
    uni = eng.uv_weights(dev(eng, u), dev(eng, v), su, sv, 16, 8, w=dev(eng, w), mode="uniform")
    assert eng.last_uv_weight_density is None
    assert np.array_equal(uni.cpu().numpy(), call(eng, su, sv, u, v, w, 16, 8, K.UNIFORM, 0.0, want=False)[0])
    for bad in (dict(mode="natural"), dict(robust=2.5), dict(robust=float("nan")), dict(w=w[:5])):
        with pytest.raises(ValueError):
            eng.uv_weights(u, v, su, sv, 16, 8, **bad)
    with pytest.raises(ValueError):
        eng.uv_weights(u, v[:9], su, sv, 16, 8)
    with pytest.raises(ValueError):
        eng.uv_weights(u, v, su, sv[:2], 16, 8)


def test_contention_the_edge_and_the_empty_maps(eng):
    # 5000 points into 4 cells (two mirror pairs) of 64 x 64, weights over 2^+-20
    rng = np.random.default_rng(11)
    u = rng.choice([-1.0, 1.0], 5000) * rng.uniform(0.8, 1.2, 5000) / 64
    v = rng.choice([-1.0, 1.0], 5000) * rng.uniform(0.8, 1.2, 5000) / 64
    w = np.ldexp(rng.uniform(0.5, 1.0, 5000), rng.integers(-20, 21, 5000))
    _, _, dens, d = check("contention", eng, [1.0], [1.0], u, v, w, 64, 64, K.BRIGGS, 0.5)
    assert np.count_nonzero(dens) == 4 and d["counted"] == [5000]
    # |gu| = hx counts, hx + 1 does not -- both signs, both axes, odd and even sizes
    for nx, nz in ((16, 8), (5, 3), (67, 131)):
        hx, hz = nx // 2, nz // 2
        gu = np.array([hx, -hx, hx + 1, -hx - 1, 0, 0, 0, 0, hx, -hx], dtype=np.float64)
        gv = np.array([0, 0, 0, 0, hz, -hz, hz + 1, -hz - 1, hz, hz], dtype=np.float64)
        _, stats, _, d = check("edge", eng, [1.0], [-1.0], gu / nx, gv / nz, None, nx, nz, K.UNIFORM, 0.0)
        assert d["counted"] == [6] and d["outside"] == [4]
    # a map without a counted visibility beside a live one: zeros and f2 = 0.  (The flags belong to
    # the visibilities, which all maps share, so a map can be empty beside a live one only through
    # its scale: everything out of range.  Everything FLAGGED is the call after it.)
    su, sv, u, v, w = K.case(16, 8, 257, 1, seed=5)
    wout, stats, dens, d = check("empty map", eng, [su[0], 1e6], [sv[0], 1e6], u, v, w, 16, 8, K.BRIGGS, 0.5)
    assert d["counted"][1] == 0 and not wout[1].any() and not dens[1].any() and not stats[1, :4].any()
    assert wout[0].any() and stats[1, 4] > 0
    # everything flagged: no scale at all
    wout, stats, dens, d = check("empty map", eng, su, sv, np.full(257, np.nan), v, w, 16, 8, K.BRIGGS, 0.5)
    assert d["s"] == 0 and not wout.any() and not stats.any() and not dens.any()
    # w_max = 0: counted, and all outputs 0
    wout, stats, dens, d = check("empty map", eng, su, sv, u, v, np.zeros(257), 16, 8, K.UNIFORM, 0.0)
    assert d["s"] == 0 and d["counted"][0] > 0 and not wout.any() and not dens.any()
    # -0.0 is a weight of 0, not a flag and not the largest bit pattern: alone (w_max = 0) and among
    # positive weights, where the integer maximum on the bits must not see its sign bit
    wout, stats, dens, d = check("empty map", eng, su, sv, u, v, np.full(257, -0.0), 16, 8, K.BRIGGS, 0.5)
    assert d["s"] == 0 and d["counted"][0] > 0 and not wout.any() and not dens.any()
    wz = np.where(np.arange(257) % 3 == 0, -0.0, np.nan_to_num(w, nan=1.0, posinf=1.0))
    wz[wz < 0] = -0.0
    for mode in (K.UNIFORM, K.BRIGGS):
        wout, stats, dens, d = check("minus zero", eng, su, sv, u, v, wz, 16, 8, mode, 0.5)
        assert d["w_max"] > 0 and not wout[0][::3].any() and wout[0].any()


# ---- 2: the three bitwise invariances ----------------------------------------------------------------
@pytest.mark.parametrize("mode", [K.UNIFORM, K.BRIGGS])
def test_repeat_permutation_and_mirror_change_no_bit(eng, mode):
    su, sv, u, v, w = K.case(67, 131, 5000, 2, seed=23)
    base = call(eng, su, sv, u, v, w, 67, 131, mode, 0.5)
    again = call(eng, su, sv, u, v, w, 67, 131, mode, 0.5)
    for a, b in zip(base, again):
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), "a repeated call"
    rng = np.random.default_rng(2)
    p = rng.permutation(5000)
    perm = call(eng, su, sv, u[p], v[p], w[p], 67, 131, mode, 0.5)
    assert np.array_equal(perm[0].view(np.int64), base[0][:, p].view(np.int64)), "a permutation permutes"
    flip = np.where(rng.random(5000) < 0.5, -1.0, 1.0)
    mirr = call(eng, su, sv, u * flip, v * flip, w, 67, 131, mode, 0.5)
    for other, what in ((perm, "permutation"), (mirr, "(u, v) -> (-u, -v)")):
        assert np.array_equal(other[1].view(np.int64), base[1].view(np.int64)), what
        assert np.array_equal(other[2].view(np.int64), base[2].view(np.int64)), what
    assert np.array_equal(mirr[0].view(np.int64), base[0].view(np.int64)), "(u, v) -> (-u, -v)"
    assert base[0].any()


# ---- 3: refusals ---------------------------------------------------------------------------------------
def test_refusals_leave_poisoned_outputs_untouched(eng):
    import torch
    from rajepy_amd import _lib
    nx, nz, M, Kv = 5, 3, 2, 70
    u, v, w = dev(eng, np.linspace(0, .4, Kv)), dev(eng, np.linspace(-.4, 0, Kv)), dev(eng, np.ones(Kv))
    su, sv = [1.0, 0.5], [0.3, -0.4]
    wb = eng.lib.rjp_uv_weights_workspace(M, nx, nz, Kv)
    assert wb == 256 + M * (32 + 8 + 15 * 8)
    wout = torch.full((M * Kv,), 7.0, dtype=torch.float64, device=eng.device)
    stats = torch.full((M * 6,), 7.0, dtype=torch.float64, device=eng.device)
    dens = torch.full((M * 15,), 7.0, dtype=torch.float64, device=eng.device)
    work = torch.full((wb,), 0xA5, dtype=torch.uint8, device=eng.device)
    good = dict(n_maps=M, n_vis=Kv, su=su, sv=sv, u=u, v=v, w=w, nx=nx, nz=nz, mode=2, robust=0.5,
                wout=wout, stats=stats, dens=dens, work=work, nbytes=wb)
    ARG, WS = _lib.RJP_ERR_ARG, _lib.RJP_ERR_WORKSPACE
    big = 2 ** 31 - 1
    cases = [("NULL h_su", dict(su=None), ARG, "null"), ("NULL h_sv", dict(sv=None), ARG, "null"),
             ("NULL d_u", dict(u=None), ARG, "null"), ("NULL d_v", dict(v=None), ARG, "null"),
             ("NULL d_wout", dict(wout=None), ARG, "null"),
             ("n_maps = 0", dict(n_maps=0), ARG, "sizes"), ("n_vis < 0", dict(n_vis=-5), ARG, "sizes"),
             ("nx = 0", dict(nx=0), ARG, "sizes"), ("nz < 0", dict(nz=-3), ARG, "sizes"),
             ("NaN h_su", dict(su=[1.0, np.nan]), ARG, "scale"),
             ("infinite h_sv", dict(sv=[np.inf, 0.1]), ARG, "scale"),
             ("mode 0", dict(mode=0), ARG, "mode"), ("mode 3", dict(mode=3), ARG, "mode"),
             ("robust 2.5", dict(robust=2.5), ARG, "robust"), ("robust -3", dict(robust=-3.0), ARG, "robust"),
             ("robust NaN", dict(robust=float("nan")), ARG, "robust"),
             ("robust inf", dict(robust=float("inf")), ARG, "robust"),
             ("too many cells", dict(nx=big, nz=big), ARG, "cells"),
             ("a short workspace", dict(nbytes=wb - 1), WS, "work"),
             ("no workspace", dict(work=None), WS, "work")]
    for what, kw, want, msg in cases:
        assert raw(eng, **dict(good, **kw)) == want, what
        assert eng.lib.rjp_last_error(eng.ctx).decode() == K.MSG[msg], what
    assert raw(eng, **dict(good, ctx=False)) == ARG
    assert eng.lib.rjp_last_error(None).decode() == "null context"
    eng.synchronize()
    for t in (wout, stats, dens):
        assert bool((t == 7.0).all())
    assert bool((work == 0xA5).all())
    # uniform mode does not look at robust; NULL weights, statistics and density are no refusal
    assert raw(eng, **dict(good, mode=1, robust=float("nan"), w=None, stats=None, dens=None)) == 2
    eng.synchronize()
    assert not bool((wout == 7.0).any()) and bool((stats == 7.0).all()) and bool((dens == 7.0).all())
    with pytest.raises(_lib.RjprtError):
        eng.uv_weights(u, v, [np.nan, 1.], sv, nx, nz)


def test_the_workgroup_limit_is_refused(eng):
    """More than 2^31 - 1 workgroups in the scatter launch: 2^20 maps x 2048 workgroups each."""
    import torch
    from rajepy_amd import _lib
    M, Kv = 2 ** 20, 2047 * 256 + 1
    assert K.workgroups(M, Kv) > 2 ** 31 - 1 >= K.workgroups(M, Kv - 1)
    su = np.ones(M)
    one = torch.zeros(8, dtype=torch.float64, device=eng.device)
    r = raw(eng, M, Kv, su, su, one, one, None, 1, 1, 1, 0.0, one, None, None, one, 64)
    assert r == _lib.RJP_ERR_ARG and eng.lib.rjp_last_error(eng.ctx).decode() == K.MSG["grid"]
    eng.synchronize()
    assert not bool(one.any())


# ---- 4: the golden models through JetModel -------------------------------------------------------------
def _params(tag):
    p = copy.deepcopy(U.load_golden(tag)[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


_MODELS = {}
SHAPE = (9, 13)


def model(eng, tag, tmp_path_factory):
    from rajepy_amd import classes, logger
    if tag not in _MODELS:
        log = logger.Log(str(tmp_path_factory.mktemp("uvweight") / (tag + ".log")), verbose=False)
        _MODELS[tag] = classes.JetModel(_params(tag), log=log, engine=eng)
    return _MODELS[tag]


def baselines(jm, freqs, n=40, amax=0.45, seed=3):
    """Baselines in metres, clustered at short spacings, that reach `amax` cycles per model cell at
    the highest frequency; the zero spacing first; weights over a decade."""
    su, sv = jm._vis_scales(freqs)
    rng = np.random.default_rng(seed)
    r = amax / np.abs(su).max() * rng.uniform(0, 1, n) ** 2
    th = rng.uniform(0, 2 * np.pi, n)
    u, v = r * np.cos(th), r * np.sin(th)
    u[0] = v[0] = 0.0
    return u, v, rng.lognormal(0.0, 0.5, n), su, sv


def ref_weights(su, sv, u, v, w, mode, robust):
    d = K.integer_density(su, sv, u, v, w, SHAPE[0], SHAPE[1])
    r = K.weights(d, w, mode, robust)
    return [np.asarray(x, dtype=np.float64) for x in r["wout"]], max(r["b_wout"])


def test_dirty_image_ff_against_the_weights_path_fed_the_reference_weights(eng, tmp_path_factory):
    from rajepy_amd import classes
    jm = model(eng, "cfg1_example", tmp_path_factory)
    freqs = np.asarray(U.load_golden("cfg1_example")[0]["freqs"], dtype=np.float64)[:3]
    jm.time = 1.0 * YEAR
    u, v, w, su, sv = baselines(jm, freqs)
    V = jm.visibilities_ff(u, v, freqs)
    for scheme, mode, robust in (("briggs", K.BRIGGS, 0.5), ("uniform", K.UNIFORM, 0.5), ("briggs", K.BRIGGS, -1.0)):
        D = jm.dirty_image_ff(u, v, freqs, weights=classes.Weighting(scheme, robust, w), shape=SHAPE)
        assert D.shape == (3,) + SHAPE and np.isfinite(D).all()
        wr, bw = ref_weights(su, sv, u, v, w, mode, robust)
        t = A.tiling(3, SHAPE[0], SHAPE[1], len(u))
        changed = []
        for f in range(3):
            assert np.count_nonzero(wr[f]) == len(u), "every baseline lies on the image's Fourier grid"
            a, b = su[f] * u, sv[f] * v
            S = A.sum_abs(V[f], a, b, wr[f])
            # K11's bound, + the weights' own (numerator and normalisation) and the division
            bnd = A.bound(V[f], a, b, SHAPE[0], SHAPE[1], wr[f], t["k_splits"], t["k_per_split"]) + 2 * bw + 4 * A.U
            r = A.worst_ratio(D[f] * wr[f].sum(), A.vis_adjoint_ref(V[f], a, b, SHAPE[0], SHAPE[1], wr[f]), S, bnd)
            WORST["dirty_image_ff " + scheme] = max(WORST.get("dirty_image_ff " + scheme, 0.0), r)
            assert r <= 1.0
            # the existing path fed the reference's weights, one channel at a time: two K11 results
            nat = jm.dirty_image_ff(u, v, freqs[f], weights=wr[f], shape=SHAPE)[0]
            assert np.abs(D[f] - nat).max() <= 2 * bnd * S / wr[f].sum()
            changed.append(np.abs(D[f] - jm.dirty_image_ff(u, v, freqs[f], weights=w, shape=SHAPE)[0]).max() >
                           1e3 * bnd * S / wr[f].sum())
        # (at the lowest frequency every baseline lies in the origin cell: any scheme is natural there)
        assert any(changed), "the scheme changes the image"
    same = jm.dirty_image_ff(u, v, freqs, weights=w, shape=SHAPE)
    for spec in (classes.Weighting(None, weights=w), classes.Weighting("natural", 0.5, w)):
        assert np.array_equal(jm.dirty_image_ff(u, v, freqs, weights=spec, shape=SHAPE), same)


def test_mfs_weighs_all_channels_in_one_density(eng, tmp_path_factory):
    from rajepy_amd import classes
    jm = model(eng, "cfg1_example", tmp_path_factory)
    freqs = np.asarray(U.load_golden("cfg1_example")[0]["freqs"], dtype=np.float64)[:2]
    jm.time = 1.0 * YEAR
    u, v, w, su, sv = baselines(jm, freqs)
    V = jm.visibilities_ff(u, v, freqs).ravel()
    aa = np.concatenate([su[f] * u for f in range(2)])
    bb = np.concatenate([sv[f] * v for f in range(2)])
    ww = np.tile(w, 2)
    pub = jm.dirty_image_ff(u, v, freqs, weights=classes.Weighting("uniform", weights=w), shape=SHAPE, mfs=True)
    assert pub.shape == (1,) + SHAPE
    wr, bw = ref_weights([1.0], [1.0], aa, bb, ww, K.UNIFORM, 0.5)
    S = A.sum_abs(V, aa, bb, wr[0])
    bnd = A.bound(V, aa, bb, SHAPE[0], SHAPE[1], wr[0]) + 2 * bw + 4 * A.U
    r = A.worst_ratio(pub[0] * wr[0].sum(), A.vis_adjoint_ref(V, aa, bb, SHAPE[0], SHAPE[1], wr[0]), S, bnd)
    WORST["mfs"] = r
    assert r <= 1.0
    iw, st = jm.imaging_weights(u, v, freqs, weights=w, shape=SHAPE, weighting="uniform", mfs=True)
    assert iw.shape == (2, len(u)) and st["counted"].tolist() == [2.0 * len(u)]
    note("imaging_weights", iw.ravel(), K.weights(K.integer_density([1.0], [1.0], aa, bb, ww, *SHAPE), ww,
                                                  K.UNIFORM)["wout"][0], K.gamma(2))


def test_dirty_beam_peaks_at_one_and_imaging_weights_match_the_reference(eng, tmp_path_factory):
    jm = model(eng, "cfg1_example", tmp_path_factory)
    freqs = np.asarray(U.load_golden("cfg1_example")[0]["freqs"], dtype=np.float64)[:3]
    u, v, w, su, sv = baselines(jm, freqs)
    for kw in (dict(weighting="briggs"), dict(weighting="uniform"), dict(weighting="briggs", robust=-2.0, mfs=True)):
        beam = jm.dirty_beam(u, v, freqs, weights=w, shape=SHAPE, **kw)
        # sum w' (K11: (2 n + splits + 4) u) over sum w' (torch: (n - 1) u) at the centre pixel
        n = len(u) * (3 if kw.get("mfs") else 1)
        assert np.abs(beam[:, 4, 6] - 1.0).max() <= (3 * n + 16) * A.U
        assert np.all(np.abs(beam) <= 1.0 + 1e-13) and np.abs(beam).min() < 0.99
    nat = jm.dirty_beam(u, v, freqs, weights=w, shape=SHAPE)
    assert np.array_equal(jm.dirty_beam(u, v, freqs, weights=w, shape=SHAPE, weighting="natural"), nat)
    # uniform weights lift the long spacings of this clustered set: a narrower main lobe
    uni = jm.dirty_beam(u, v, freqs, weights=w, shape=SHAPE, weighting="uniform")
    # (not at the lowest frequency, where every baseline lies in the origin cell)
    for a, b in ((uni[:, 4, 7], nat[:, 4, 7]), (uni[:, 5, 6], nat[:, 5, 6])):
        assert np.all(a <= b + 1e-12) and np.count_nonzero(a < b - 1e-3) >= 2
    for scheme, mode, robust in (("briggs", K.BRIGGS, 0.5), ("uniform", K.UNIFORM, 0.5)):
        iw, st = jm.imaging_weights(u, v, freqs, weights=w, shape=SHAPE, weighting=scheme, robust=robust)
        d = K.integer_density(su, sv, u, v, w, *SHAPE)
        r = K.weights(d, w, mode, robust)
        for f in range(3):
            note("imaging_weights", iw[f], r["wout"][f], r["b_wout"][f])
            assert st["sum_w"][f] == d["sum_w"][f] and st["counted"][f] == len(u) and st["shift"][f] == d["s"]
            nf = K.noise_factor(r["wout"][f], w)
            assert abs(st["noise_factor"][f] - nf) <= 1e-13 * nf and st["noise_factor"][f] >= 1.0 - 1e-13
        assert st["noise_factor"].max() > 1.0001


def test_clean_image_ff_with_briggs_weights_runs_through_to_imfit(eng, tmp_path_factory):
    from rajepy_amd import classes
    jm = model(eng, "cfg1_example", tmp_path_factory)
    freqs = np.asarray(U.load_golden("cfg1_example")[0]["freqs"], dtype=np.float64)[:2]
    jm.time = 1.0 * YEAR
    u, v, w, su, sv = baselines(jm, freqs, n=60)
    from rajepy_amd import engine as E
    shape = (21, 25)
    cell_as = np.degrees(np.arctan(jm.csize * E.con.au / (jm.params["target"]["dist"] * E.con.parsec))) * 3600.
    kw = dict(weights=w, shape=shape, niter=30, imfit=True, beam=(3.0 * cell_as, 2.5 * cell_as, 30.0))
    res = jm.clean_image_ff(u, v, freqs, weighting="briggs", robust=0.5, **kw)
    nat = jm.clean_image_ff(u, v, freqs, **kw)
    assert res.image.shape == (2,) + shape and np.isfinite(res.image).all() and np.isfinite(res.residual).all()
    assert len(res.imfit) == 2 and all(f["status"] in (0, 1, 2, 3) for f in res.imfit)
    assert all(np.isfinite(f["I"]["val"]) for f in res.imfit if f["status"] != 3)
    assert len(res.beam) == 2 and all(len(c) > 0 for c in res.components)
    # the weights are the image's, shared with the beam: the dirty image of the components' beam
    # is normalised, so the first component is gain x the dirty image's peak
    D = jm.dirty_image_ff(u, v, freqs, weights=classes.Weighting("briggs", 0.5, w), shape=shape)
    for f in range(2):
        ix, iz, flux = res.components[f][0]
        assert abs(D[f]).max() == abs(D[f, int(ix), int(iz)]) and abs(flux - 0.1 * D[f, int(ix), int(iz)]) <= \
            1e-12 * abs(flux)
    assert any(np.abs(res.image[f] - nat.image[f]).max() > 1e-6 * np.abs(nat.image[f]).max() for f in range(2))
