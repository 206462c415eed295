"""rjp_vis_adjoint (K11, vis_adjoint.hip): dirty images from visibilities, the transpose of rjp_vis,
through the C-ABI, RTEngine.vis_adjoint and JetModel.dirty_image_* / dirty_beam, against
tests/vis_adjoint_ref.py -- a long-double NumPy direct sum on the inputs as the device holds them,
which tests/test_vis_adjoint_reference_cpu.py pins to the inverse FFT, to hand-worked fringes and to
the transpose identity, and whose bound it holds to a float64 emulation (inside) and four planted
mistakes (outside).

The bound is derived in tests/vis_adjoint_ref.py, not measured: per pixel, relative to
S = sum |w_k| |V_k| over the unflagged visibilities,
    |got - ref| <= [sum_k |w_k V_k| 2 pi (|a_k| (nx-1)/2 + |b_k| (nz-1)/2) u / S + 2 (2.01e-14 + 6 u)
                    + 6 u + (2 n_k + n_split + 4) u] S
(u = 2^-53; a, b in cycles per cell; n_k the visibilities of the longest k-split).  The module
prints the worst |got - ref| / bound per group."""
import copy

import numpy as np
import pytest

from tests import gpu_util as U
from tests import vis_adjoint_ref as A
from tests import vis_ref as R

pytestmark = pytest.mark.gpu
YEAR = 31557600.0
LD = np.longdouble
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
    r = A.worst_ratio(got, ref, S, bnd) if S > 0 else 0.0
    WORST[kind] = max(WORST.get(kind, 0.0), r)
    assert r <= 1.0, (kind, r)
    return r


def dev(eng, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(eng.device)


def dev_vis(eng, V):
    """complex [M, K] host array -> float64 [M, K, 2] device tensor."""
    V = np.asarray(V, dtype=np.complex128)
    return dev(eng, np.stack([V.real, V.imag], axis=-1))


def raw(eng, vis, n_maps, n_vis, su, sv, u, v, w, nx, nz, img, work, nbytes, ctx=True):
    from rajepy_amd import _lib
    ptr = lambda t: t.data_ptr() if t is not None else None
    return eng.lib.rjp_vis_adjoint(eng.ctx if ctx else None, ptr(vis), n_maps, n_vis,
                                   _lib.dbl_array(su) if su is not None else None,
                                   _lib.dbl_array(sv) if sv is not None else None,
                                   ptr(u), ptr(v), ptr(w), nx, nz, ptr(img), ptr(work), nbytes,
                                   eng._stream())


# ---- 1: random visibilities at the bound ----------------------------------------------------------
FACTORS = (1.0, -0.37, 0.61)          # every map its own scale, signs included


@pytest.mark.parametrize("nx,nz", A.SHAPES)
def test_random_visibilities_against_the_reference(eng, nx, nz):
    """Both tile heights (nx <= 64: 64 rows, else 128), one and two row and column tiles with their
    tails, 1-1000 visibilities (one chunk, ragged chunks, and the k-split: these shapes have few
    tiles, so 65 visibilities and more are split over workgroups -- asserted through the tile count);
    20 % of the visibilities flagged through Re V, Im V or w, an all-flagged map, a scale per map,
    random weights and none."""
    rng = np.random.default_rng(1000 * nx + nz)
    worst, case = 0.0, 0
    for n_vis in A.N_VIS:
        for n_maps in (1, 3):
            for amax in (0.5, 8.0):
                if n_vis == A.N_VIS[-1] and (n_maps, amax) != (3, 0.5):
                    continue                               # the long set once
                case += 1
                V = np.empty((n_maps, n_vis), dtype=np.complex128)
                for m in range(n_maps):
                    V[m], w = A.random_vis(rng, n_vis)
                if n_maps == 3:
                    V[1] = complex(np.nan, 1.0)
                if case % 2:
                    w = None
                u, v = R.random_points(rng, n_vis, 1.0)
                su = amax * np.array(FACTORS[:n_maps])
                sv = -amax * np.array(FACTORS[:n_maps][::-1])
                got = eng.vis_adjoint(dev_vis(eng, V), nx, nz, su, sv, u, v, w).cpu().numpy()
                assert got.shape == (n_maps, nx * nz) and got.dtype == np.float64
                t = A.tiling(n_maps, nx, nz, n_vis)
                assert eng.last_vis_adjoint_tiles == t["workgroups"] > 0
                assert (t["k_splits"] > 1) == (n_vis > 64), "these shapes split beyond 64"
                for m in range(n_maps):
                    a, b = su[m] * u, sv[m] * v               # the device's own float64 products
                    S = A.sum_abs(V[m], a, b, w)
                    if S == 0:
                        assert np.all(got[m] == 0), "an all-flagged map images to exact zeros"
                        continue
                    bnd = A.bound(V[m], a, b, nx, nz, w, t["k_splits"], t["k_per_split"])
                    worst = max(worst, note("random |a| <= %g" % amax, got[m].reshape(nx, nz),
                                            A.vis_adjoint_ref(V[m], a, b, nx, nz, w), S, bnd))
    assert A.tiling(3, nx, nz, A.N_VIS[-1])["k_splits"] > 1
    print("%d x %d: worst |got - ref| / bound = %.3f" % (nx, nz, worst))


# ---- 2: the transpose identity on the device --------------------------------------------------------
@pytest.mark.parametrize("nx,nz,K,amax", [(67, 131, 257, 0.5), (130, 65, 64, 8.0), (5, 3, 63, 0.5)])
def test_transpose_identity_with_rjp_vis(eng, nx, nz, K, amax):
    """sum_k w_k Re(conj(Y_k) V_k) = sum_p I_p D_p for V = rjp_vis(I), D = rjp_vis_adjoint(Y, w):
    both sums in long double on the host, NaN pixels and flagged visibilities counted as 0."""
    rng = np.random.default_rng(nx + 7 * nz + K)
    I = R.random_map(rng, nx, nz)
    Y, w = A.random_vis(rng, K)
    u, v = R.random_points(rng, K, 1.0)
    su, sv = [amax], [-0.8 * amax]
    a, b = su[0] * u, sv[0] * v
    Vd = eng.vis(dev(eng, I.reshape(1, -1)), nx, nz, su, sv, u, v).cpu().numpy()[0]
    D = eng.vis_adjoint(dev_vis(eng, Y[None, :]), nx, nz, su, sv, u, v, w).cpu().numpy()[0]
    ok = A.unflagged(Y, a, b, w)
    assert 0 < ok.sum() < K
    lhs = (w[ok].astype(LD) * (Y.real[ok].astype(LD) * Vd.real[ok].astype(LD) +
                               Y.imag[ok].astype(LD) * Vd.imag[ok].astype(LD))).sum()
    rhs = (np.where(np.isnan(I), 0.0, I).astype(LD).ravel() * D.astype(LD)).sum()
    t = A.tiling(1, nx, nz, K)
    bnd = float(R.bound(a, b, nx, nz).max()) + A.bound(Y, a, b, nx, nz, w, t["k_splits"], t["k_per_split"])
    scale = R.sum_abs(I) * A.sum_abs(Y, a, b, w)
    r = abs(float(lhs - rhs)) / (bnd * scale)
    WORST["transpose identity"] = max(WORST.get("transpose identity", 0.0), r)
    print("%d x %d x %d: |<Y, A I> - <A^T Y, I>| / bound = %.4f" % (nx, nz, K, r))
    assert r <= 1.0


# ---- 3: repeat, guard bands, non-finite baselines and weights -----------------------------------------
def test_repeat_guard_bands_and_flagged_baselines(eng):
    import torch
    nx, nz, M, K = 130, 65, 3, 257
    rng = np.random.default_rng(7)
    V = np.stack([A.random_vis(rng, K, flagged=0.0)[0] for _ in range(M)])
    w = A.random_vis(rng, K, flagged=0.0)[1]
    u, v = R.random_points(rng, K, 1.0)
    su, sv = 0.5 * np.array(FACTORS), 0.4 * np.array(FACTORS)
    d_vis = dev_vis(eng, V)
    t = A.tiling(M, nx, nz, K)
    wb = eng.lib.rjp_vis_adjoint_workspace(M, nx, nz, K)
    assert t["k_splits"] == 5 and wb == A.workspace_bytes(M, nx, nz, K) == M * 5 * nx * nz * 8
    guard, n_out = 4096, M * nx * nz
    out = torch.full((guard + n_out + guard,), -7.0, dtype=torch.float64, device=eng.device)
    work = torch.full((wb + guard,), 0xA5, dtype=torch.uint8, device=eng.device)
    call = lambda uu, vv, ww, o: raw(eng, d_vis, M, K, su, sv, dev(eng, uu), dev(eng, vv),
                                     dev(eng, ww) if ww is not None else None, nx, nz, o[guard:],
                                     work, wb)
    assert call(u, v, w, out) == t["workgroups"] == 30, eng.lib.rjp_last_error(eng.ctx)
    eng.synchronize()
    assert bool((out[:guard] == -7.0).all()) and bool((out[guard + n_out:] == -7.0).all())
    assert bool((work[wb:] == 0xA5).all())
    first = out[guard:guard + n_out].clone()
    assert bool(torch.isfinite(first).all())
    assert torch.equal(eng.vis_adjoint(d_vis, nx, nz, su, sv, u, v, w).reshape(-1), first)
    assert torch.equal(eng.vis_adjoint(torch.view_as_complex(d_vis), nx, nz, su, sv, u, v, w).reshape(-1),
                       first)
    out2 = torch.full_like(out, -7.0)
    assert call(u, v, w, out2) == 30
    eng.synchronize()
    assert torch.equal(out2, out), "a repeated call gives the same bits"
    # d_w = NULL is all ones
    ones = torch.full_like(out, -7.0)
    none = torch.full_like(out, -7.0)
    assert call(u, v, np.ones(K), ones) == 30 and call(u, v, None, none) == 30
    eng.synchronize()
    assert torch.equal(ones, none) and not torch.equal(ones, out)
    # a non-finite baseline or weight removes exactly its visibility: the same bits as weight 0
    for which, k, bad in (("u", 17, np.nan), ("u", 100, np.inf), ("v", 0, -np.inf), ("w", 200, np.nan),
                          ("w", 64, np.inf)):
        arrs = dict(u=u.copy(), v=v.copy(), w=w.copy())
        arrs[which][k] = bad
        w0 = w.copy()
        w0[k] = 0.0
        o_bad, o_zero = torch.full_like(out, -7.0), torch.full_like(out, -7.0)
        assert call(arrs["u"], arrs["v"], arrs["w"], o_bad) == 30 and call(u, v, w0, o_zero) == 30
        eng.synchronize()
        assert bool(torch.isfinite(o_bad).all()), (which, k)
        assert torch.equal(o_bad, o_zero), (which, k, bad)
        assert not torch.equal(o_bad, out)
    # ... and what is left is the reference without it
    ub = u.copy()
    ub[17] = np.nan
    got = eng.vis_adjoint(d_vis, nx, nz, su, sv, ub, v, w).cpu().numpy()
    for m in range(M):
        a, b = su[m] * ub, sv[m] * v
        note("flagged baseline", got[m].reshape(nx, nz), A.vis_adjoint_ref(V[m], a, b, nx, nz, w),
             A.sum_abs(V[m], a, b, w), A.bound(V[m], a, b, nx, nz, w, t["k_splits"], t["k_per_split"]))


# ---- 4: refusals -------------------------------------------------------------------------------------
NULLS = "rjp_vis_adjoint: NULL visibilities, scales, baselines or output"
COUNTS = "rjp_vis_adjoint: n_maps, n_vis, nx and nz must be positive"
SCALES = "rjp_vis_adjoint: non-finite h_su / h_sv"
GRID = "rjp_vis_adjoint: more than 2^31 - 1 workgroups"
SHORT = "rjp_vis_adjoint: workspace smaller than rjp_vis_adjoint_workspace()"


def test_refusals_leave_poisoned_outputs_untouched(eng):
    import torch
    from rajepy_amd import _lib
    nx, nz, M, K = 5, 3, 2, 70                            # two k-splits: the workspace is in use
    u, v, w = dev(eng, np.linspace(0, 1, K)), dev(eng, np.linspace(-1, 0, K)), dev(eng, np.ones(K))
    d_vis = dev(eng, np.ones((M, K, 2)))
    su, sv = [0.1, 0.2], [0.3, -0.4]
    wb = eng.lib.rjp_vis_adjoint_workspace(M, nx, nz, K)
    assert wb == M * 2 * nx * nz * 8
    img = torch.full((M * nx * nz,), 7.0, dtype=torch.float64, device=eng.device)
    work = torch.full((wb,), 0xA5, dtype=torch.uint8, device=eng.device)
    good = dict(vis=d_vis, n_maps=M, n_vis=K, su=su, sv=sv, u=u, v=v, w=w, nx=nx, nz=nz, img=img,
                work=work, nbytes=wb)
    ARG, WS = _lib.RJP_ERR_ARG, _lib.RJP_ERR_WORKSPACE
    big = 2 ** 31 - 1
    cases = [("NULL d_vis", dict(vis=None), ARG, NULLS), ("NULL h_su", dict(su=None), ARG, NULLS),
             ("NULL h_sv", dict(sv=None), ARG, NULLS), ("NULL d_u", dict(u=None), ARG, NULLS),
             ("NULL d_v", dict(v=None), ARG, NULLS), ("NULL d_img", dict(img=None), ARG, NULLS),
             ("n_maps = 0", dict(n_maps=0), ARG, COUNTS), ("n_maps < 0", dict(n_maps=-1), ARG, COUNTS),
             ("n_vis = 0", dict(n_vis=0), ARG, COUNTS), ("n_vis < 0", dict(n_vis=-5), ARG, COUNTS),
             ("nx = 0", dict(nx=0), ARG, COUNTS), ("nx < 0", dict(nx=-1), ARG, COUNTS),
             ("nz = 0", dict(nz=0), ARG, COUNTS), ("nz < 0", dict(nz=-3), ARG, COUNTS),
             ("NaN h_su", dict(su=[0.1, np.nan]), ARG, SCALES),
             ("infinite h_sv", dict(sv=[np.inf, 0.1]), ARG, SCALES),
             ("too many workgroups", dict(nx=big, nz=big), ARG, GRID),
             ("a short workspace", dict(nbytes=wb - 1), WS, SHORT),
             ("no workspace", dict(work=None), WS, SHORT)]
    for what, kw, want, msg in cases:
        assert raw(eng, **dict(good, **kw)) == want, what
        assert eng.lib.rjp_last_error(eng.ctx).decode() == msg, what
    assert raw(eng, **dict(good, ctx=False)) == ARG
    assert eng.lib.rjp_last_error(None).decode() == "null context"
    eng.synchronize()
    assert bool((img == 7.0).all()) and bool((work == 0xA5).all())
    for a in ((0, nx, nz, K), (M, -1, nz, K), (M, nx, 0, K), (M, nx, nz, -2)):
        assert eng.lib.rjp_vis_adjoint_workspace(*a) == 0
    # the context still serves a valid call; NULL weights are no refusal
    assert raw(eng, **dict(good, w=None)) == 4 == A.tiling(M, nx, nz, K)["workgroups"]
    eng.synchronize()
    assert not bool((img == 7.0).any())
    V = torch.view_as_complex(d_vis)
    with pytest.raises(ValueError):
        eng.vis_adjoint(V, nx, nz, su[:1], sv, u, v)
    with pytest.raises(ValueError):
        eng.vis_adjoint(V, nx, 0, su, sv, u, v)
    with pytest.raises(ValueError):
        eng.vis_adjoint(V, nx, nz, su, sv, u[:5], v)
    with pytest.raises(ValueError):
        eng.vis_adjoint(V, nx, nz, su, sv, u, v, w[:3])
    with pytest.raises(ValueError):
        eng.vis_adjoint(V.to(torch.complex64), nx, nz, su, sv, u, v)
    with pytest.raises(_lib.RjprtError):
        eng.vis_adjoint(V, nx, nz, [np.nan, 1.], sv, u, v)


# ---- 5: the golden models through JetModel ----------------------------------------------------------
def _params(tag):
    p = copy.deepcopy(U.load_golden(tag)[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


_MODELS = {}
SHAPE = (9, 13)                        # an odd-sized image: the centre pixel is the phase centre


def model(eng, tag, tmp_path_factory):
    from rajepy_amd import classes, logger
    if tag not in _MODELS:
        log = logger.Log(str(tmp_path_factory.mktemp("visadj") / (tag + ".log")), verbose=False)
        _MODELS[tag] = classes.JetModel(_params(tag), log=log, engine=eng)
    return _MODELS[tag]


def baselines(jm, freqs, n=7, amax=0.5, seed=3):
    """Baselines in metres that reach `amax` cycles per model cell at the highest frequency; the
    zero spacing first; weights over a decade."""
    su, sv = jm._vis_scales(freqs)
    rng = np.random.default_rng(seed)
    u, v = R.random_points(rng, n, amax / np.abs(su).max())
    return u, v, rng.lognormal(0.0, 0.5, n), su, sv


def check_images(kind, D, V, u, v, w, su, sv):
    """D[F, ni, nj] in Jy / beam against the reference on the host visibilities V[F, K]."""
    wsum = np.ones(len(u)).sum() if w is None else w.sum()
    for f in range(D.shape[0]):
        a, b = su[f] * u, sv[f] * v
        S = A.sum_abs(V[f], a, b, w)
        assert S > 0
        t = A.tiling(D.shape[0], D.shape[1], D.shape[2], len(u))
        # (+ u: the division by sum w)
        note(kind, D[f] * wsum, A.vis_adjoint_ref(V[f], a, b, D.shape[1], D.shape[2], w), S,
             A.bound(V[f], a, b, D.shape[1], D.shape[2], w, t["k_splits"], t["k_per_split"]) + 2 * A.U)


def test_dirty_beam_is_one_at_the_centre_and_point_symmetric(eng, tmp_path_factory):
    jm = model(eng, "cfg1_example", tmp_path_factory)
    freqs = np.asarray(U.load_golden("cfg1_example")[0]["freqs"], dtype=np.float64)[:3]
    u, v, w, su, sv = baselines(jm, freqs)
    beam = jm.dirty_beam(u, v, freqs, shape=SHAPE)
    assert beam.shape == (3,) + SHAPE and beam.dtype == np.float64
    assert np.all(beam[:, 4, 6] == 1.0), "every phase is 0 at the centre pixel"
    assert np.all(np.abs(beam) <= 1.0 + 1e-13) and np.abs(beam).min() < 0.99
    bnd = 2.0 * (2 * np.pi * 0.5 * (4 + 6) * A.U + 2 * (R.SINCOS_TRUNC + R.SINCOS_ROUND) + 40 * A.U)
    assert np.abs(beam - beam[:, ::-1, ::-1]).max() <= bnd
    check_images("beam", beam, np.ones((3, len(u)), dtype=np.complex128), u, v, None, su, sv)
    # weighted: 1 to the rounding of two sums of 7 weights; mfs: one beam for the three channels
    bw = jm.dirty_beam(u, v, freqs, weights=w, shape=SHAPE)
    assert np.abs(bw[:, 4, 6] - 1.0).max() <= 16 * A.U
    check_images("beam", bw, np.ones((3, len(u)), dtype=np.complex128), u, v, w, su, sv)
    bm = jm.dirty_beam(u, v, freqs, weights=w, shape=SHAPE, mfs=True)
    assert bm.shape == (1,) + SHAPE and abs(bm[0, 4, 6] - 1.0) <= 48 * A.U
    assert np.abs(bm[0] - bw.mean(axis=0)).max() <= 3 * bnd


def test_dirty_image_ff_on_the_example_model(eng, tmp_path_factory):
    jm = model(eng, "cfg1_example", tmp_path_factory)
    freqs = np.asarray(U.load_golden("cfg1_example")[0]["freqs"], dtype=np.float64)[:3]
    jm.time = 1.0 * YEAR
    u, v, w, su, sv = baselines(jm, freqs)
    V = jm.visibilities_ff(u, v, freqs)
    D = jm.dirty_image_ff(u, v, freqs, weights=w, shape=SHAPE)
    assert D.shape == (3,) + SHAPE and D.dtype == np.float64 and np.isfinite(D).all()
    check_images("dirty_image_ff", D, V, u, v, w, su, sv)
    # the model's own grid by default, and another cell size through image_scales
    D0 = jm.dirty_image_ff(u, v, freqs)
    assert D0.shape == (3, jm.nx, jm.nz)
    check_images("dirty_image_ff", D0, V, u, v, None, su, sv)
    from rajepy_amd import engine as E
    cell_as = 0.25 * np.degrees(np.arctan(jm.csize * E.con.au / (jm.params["target"]["dist"] * E.con.parsec))) * 3600.
    Dq = jm.dirty_image_ff(u, v, freqs, weights=w, shape=(31, 27), cell_as=cell_as)
    qu, qv = E.image_scales(freqs, np.radians(cell_as / 3600.))
    assert np.allclose(qu, su / 4, rtol=1e-14)
    check_images("dirty_image_ff", Dq, V, u, v, w, qu, qv)
    # zero-spacing-only data: the image is flat at the total flux flux_vs_time returns
    lc = jm.flux_vs_time([jm.time], freqs)[0]
    Dz = jm.dirty_image_ff([0.0], [0.0], freqs, shape=SHAPE)
    flux = jm.flux_ff(freqs)
    for f in range(3):
        S = R.sum_abs(flux[f])
        tol = (jm.nx * jm.nz * R.U + 2 * (R.SINCOS_TRUNC + R.SINCOS_ROUND) + 16 * A.U) * S
        assert abs(Dz[f, 4, 6] - lc[f]) <= tol
        assert np.abs(Dz[f] - lc[f]).max() <= tol


def test_mfs_is_the_weighted_mean_of_the_channel_images(eng, tmp_path_factory):
    """Two channels' visibilities imaged at ONE frequency's (u, v) / lambda -- the same baselines in
    cycles per cell for both: the mfs image is the mean of the two channel images."""
    jm = model(eng, "cfg1_example", tmp_path_factory)
    freqs = np.asarray(U.load_golden("cfg1_example")[0]["freqs"], dtype=np.float64)[:2]
    jm.time = 1.0 * YEAR
    u, v, w, su, sv = baselines(jm, freqs)
    u_d, v_d = eng._device_f64(u), eng._device_f64(v)
    maps = jm._ff_products(freqs, flux=True, device=True)
    V = eng.vis(maps.reshape(2, -1), jm.nx, jm.nz, su, sv, u_d, v_d)
    same = np.array([freqs[1], freqs[1]])
    per = jm._imager._dirty_images(V, u_d, v_d, same, w, SHAPE, None, False)
    mfs = jm._imager._dirty_images(V, u_d, v_d, same, w, SHAPE, None, True)
    assert per.shape == (2,) + SHAPE and mfs.shape == (1,) + SHAPE
    assert np.abs(per[0] - per[1]).max() > 0
    Vh = V.cpu().numpy()
    a, b = su[1] * u, sv[1] * v
    S = 0.5 * (A.sum_abs(Vh[0], a, b, w) + A.sum_abs(Vh[1], a, b, w)) / w.sum()
    bnd = 2 * (A.bound(Vh[0], a, b, SHAPE[0], SHAPE[1], w) + 8 * A.U)
    r = np.abs(mfs[0] - 0.5 * (per[0] + per[1])).max() / (bnd * S)
    WORST["mfs"] = r
    assert r <= 1.0
    # through the public call: the channels at their own (u, v) / lambda in one image
    Vff = jm.visibilities_ff(u, v, freqs)
    pub = jm.dirty_image_ff(u, v, freqs, weights=w, shape=SHAPE, mfs=True)
    aa = np.concatenate([su[f] * u for f in range(2)])
    bb = np.concatenate([sv[f] * v for f in range(2)])
    ww = np.tile(w, 2)
    note("mfs", pub[0] * ww.sum(), A.vis_adjoint_ref(Vff.ravel(), aa, bb, SHAPE[0], SHAPE[1], ww),
         A.sum_abs(Vff.ravel(), aa, bb, ww),
         A.bound(Vff.ravel(), aa, bb, SHAPE[0], SHAPE[1], ww) + 2 * A.U)


def test_dirty_image_formal_on_the_tilted_model(eng, tmp_path_factory):
    jm = model(eng, "tilted", tmp_path_factory)
    freqs = np.asarray(U.load_golden("tilted")[0]["freqs"], dtype=np.float64)
    jm.time = 0.4 * YEAR
    u, v, w, su, sv = baselines(jm, freqs)
    Df = jm.dirty_image_ff(u, v, freqs, weights=w, shape=SHAPE, formal=True)
    Di = jm.dirty_image_ff(u, v, freqs, weights=w, shape=SHAPE)
    Vf = jm.visibilities_ff(u, v, freqs, formal=True)
    check_images("formal", Df, Vf, u, v, w, su, sv)
    check_images("dirty_image_ff", Di, jm.visibilities_ff(u, v, freqs), u, v, w, su, sv)
    for f in range(len(freqs)):
        # a temperature gradient along the sightlines: the two solutions are different images
        S = A.sum_abs(Vf[f], su[f] * u, sv[f] * v, w) / w.sum()
        assert np.abs(Df[f] - Di[f]).max() > 1e3 * A.bound(Vf[f], su[f] * u, sv[f] * v, *SHAPE, w) * S


def test_dirty_image_rrl_on_one_line(eng, tmp_path_factory):
    jm = model(eng, "cfg1_example", tmp_path_factory)
    z, meta, _ = U.load_golden("cfg1_example")
    rf = np.asarray(z["rrl_freqs"], dtype=np.float64)[3:5]
    jm.time = 1.0 * YEAR
    u, v, w, su, sv = baselines(jm, rf)
    D = jm.dirty_image_rrl(meta["rrl"], u, v, rf, weights=w, shape=SHAPE, contsub=False)
    assert D.shape == (2,) + SHAPE
    check_images("dirty_image_rrl", D, jm.visibilities_rrl(meta["rrl"], u, v, rf, contsub=False),
                 u, v, w, su, sv)
