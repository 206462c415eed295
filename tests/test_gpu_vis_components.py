"""rjp_vis_components (K18, vis_components.hip) and rjp_components_image through the C-ABI and
RTEngine, against tests/vis_components_ref.py -- a long-double direct sum over the list, which
tests/test_vis_components_reference_cpu.py pins to K10's reference, to a float64 emulation of the
stated order (inside the bound) and to four planted mistakes (outside).

The bound is derived in tests/vis_components_ref.py, not measured: per visibility and part
    |got - ref| <= [2 pi (|a| (nx-1)/2 + |b| (nz-1)/2) u + sqrt(2) (2 (2.01e-14 + 6 u) + 2 u)
                    + sqrt(2) d u / (1 - d u) + 2 n_s u + 4 u] (sum_c |f_c| |G_c| + |in|)
(u = 2^-53, d = 64 ceil(n / 256); a, b in cycles per cell).  The module prints the worst ratio per
group."""
import numpy as np
import pytest

from tests import clean_ref as C
from tests import msclean_ref as K
from tests import vis_components_ref as R
from tests import vis_ref as VR

pytestmark = pytest.mark.gpu
WORST = {}
STRIDE = 1000
FACTORS = (1.0, -0.37, 0.61)          # every map its own scale, signs included


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()
    print("\nworst |got - ref| / bound per group: " +
          ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def note(kind, got, ref, S, bnd):
    r = R.worst_ratio(got, ref, S, bnd)
    WORST[kind] = max(WORST.get(kind, 0.0), r)
    print("%s: |got - ref| / bound = %.3f" % (kind, r))
    assert r <= 1.0, (kind, r)
    return r


def dev(eng, a, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(eng.device)


def lists(rng, M, nx, nz, n_s, stride=STRIDE):
    rows = [R.random_list(rng, nx, nz, stride, n_s) for _ in range(M)]
    return (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
            np.stack([r[2] for r in rows]))


def raw(eng, cpix, cscale, cflux, ncomp, M, stride, n_s, nx, nz, su, sv, u, v, K_, gvis, vin, sign, out):
    from rajepy_amd import _lib
    ptr = lambda t: t.data_ptr() if t is not None else None
    return eng.lib.rjp_vis_components(
        eng.ctx, ptr(cpix), ptr(cscale), ptr(cflux), ptr(ncomp), M, stride, n_s, nx, nz,
        _lib.dbl_array(su) if su is not None else None, _lib.dbl_array(sv) if sv is not None else None,
        ptr(u), ptr(v), K_, ptr(gvis), ptr(vin), sign, ptr(out), eng._stream())


# ---- 1: random lists at the bound -----------------------------------------------------------------------
# per visibility count: (maps, scales (1 = G NULL), ncomp per map, `in`: None / "given" / "alias", sign)
CASES = {1: (1, 1, (1,), None, 1),
         63: (3, 3, (0, 63, 1000), "given", -1),
         64: (3, 1, (64, 1200, 65), "alias", -1),
         65: (2, 3, (1200, 1), "alias", 1),
         257: (3, 3, (65, 64, 0), None, -1)}


@pytest.mark.parametrize("nx,nz", R.SHAPES)
def test_random_lists_against_the_reference(eng, nx, nz):
    """1-5 visibility tiles with ragged ends; lists that end inside the first slice, at a slice's
    end, one past it, four chunks long and beyond the stride (clamped), differing per map; G NULL
    with one scale and given with three; `in` NULL, given and aliased to `out`; both signs; up to
    0.5 and 8 cycles per cell; duplicated pixels, fluxes of both signs, a scale per map."""
    import torch
    rng = np.random.default_rng(1000 * nx + nz)
    for n_vis in R.N_VIS:
        M, n_s, ncomp, mode, sign = CASES[n_vis]
        p, f, s = lists(rng, M, nx, nz, n_s)
        d_p, d_f, d_s = dev(eng, p, np.int32), dev(eng, f), dev(eng, s, np.int32)
        d_n = dev(eng, np.array(ncomp), np.int32)
        G = np.stack([R.random_g(rng, n_s, n_vis) for _ in range(M)]) if n_s > 1 else None
        for amax in (0.5, 8.0):
            u, v = VR.random_points(rng, n_vis, 1.0)
            su = amax * np.array(FACTORS[:M])
            sv = -amax * np.array(FACTORS[:M][::-1])
            vin = (rng.standard_normal((M, n_vis)) + 1j * rng.standard_normal((M, n_vis))) \
                if mode else None
            d_in = dev(eng, vin, np.complex128) if mode else None
            got = eng.vis_components(d_p, d_f, d_n, nx, nz, su, sv, u, v,
                                     cscale=d_s if n_s > 1 else None, n_s=n_s,
                                     gvis=dev(eng, G, np.complex128) if G is not None else None,
                                     vis_in=d_in, sign=sign, out=d_in if mode == "alias" else None)
            if mode == "alias":
                assert got.data_ptr() == d_in.data_ptr()
            elif mode:
                assert torch.equal(d_in, dev(eng, vin, np.complex128)), "`in` is read only"
            assert eng.last_vis_components_workgroups == R.workgroups(M, n_vis)
            got = got.cpu().numpy()
            assert got.shape == (M, n_vis) and got.dtype == np.complex128
            for m in range(M):
                n = R.clamp(ncomp[m], STRIDE)
                a, b = su[m] * u, sv[m] * v               # the device's own float64 products
                ref, S = R.vis_components_ref(p[m], f[m], s[m] if n_s > 1 else None, n, nx, nz, a, b,
                                              n_s, G[m] if G is not None else None,
                                              vin[m] if mode else None, sign)
                if n == 0:
                    want = vin[m] if mode else np.zeros(n_vis, dtype=np.complex128)
                    assert got[m].tobytes() == want.tobytes(), "ncomp = 0 copies `in` bit for bit"
                    continue
                note("%s |a| <= %g" % ("G" if n_s > 1 else "hogbom", amax), got[m], ref, S,
                     R.bound(a, b, nx, nz, n, n_s))


# ---- 2: what adds nothing, flags, the bit-for-bit copy ------------------------------------------------------
def test_components_that_add_nothing_flags_and_the_copy(eng):
    nx, nz, n_s, M, K_ = 5, 3, 2, 2, 65
    rng = np.random.default_rng(2)
    p, f, s = lists(rng, M, nx, nz, n_s, stride=70)
    # map 0: a NaN flux, an infinite flux, pixels outside the grid, scales outside [0, n_s)
    f[0, 3], f[0, 66] = np.nan, -np.inf
    p[0, 5], p[0, 64] = -1, nx * nz
    s[0, 7], s[0, 65] = n_s, -1
    ncomp = np.array([70, 0], dtype=np.int32)
    u, v = VR.random_points(rng, K_, 1.0)
    su, sv = np.array([0.4, -0.3]), np.array([0.2, 0.45])
    G = np.stack([R.random_g(rng, n_s, K_) for _ in range(M)])
    vin = rng.standard_normal((M, K_)) + 1j * rng.standard_normal((M, K_))
    vin[1, 4] = complex(-0.0, 0.0)
    vin[1, 5] = complex(0.0, -0.0)
    vin[0, 9] = complex(np.nan, 1.0)                  # a flagged visibility stays flagged
    vin[0, 10] = complex(2.0, np.inf)
    call = lambda pp, ff, ss, uu, nn=ncomp: eng.vis_components(
        dev(eng, pp, np.int32), dev(eng, ff), dev(eng, nn, np.int32), nx, nz, su, sv, uu, v,
        cscale=dev(eng, ss, np.int32), n_s=n_s, gvis=dev(eng, G, np.complex128),
        vis_in=dev(eng, vin, np.complex128), sign=-1)
    got = call(p, f, s, u)
    ref, S = R.vis_components_ref(p[0], f[0], s[0], 70, nx, nz, su[0] * u, sv[0] * v, n_s, G[0], vin[0], -1)
    g = got.cpu().numpy()
    keep = [k for k in range(K_) if k not in (9, 10)]
    note("dead components", g[0][keep], ref[keep], S[keep], R.bound(su[0] * u, sv[0] * v, nx, nz, 70, n_s)[keep])
    assert np.isnan(g[0, 9].real) and np.isinf(g[0, 10].imag) and not np.isnan(g[0, 9].imag)
    assert g[1].tobytes() == vin[1].tobytes(), "ncomp = 0 copies `in` bit for bit, -0.0 included"
    # a negative count is 0 too
    g2 = call(p, f, s, u, np.array([70, -4], dtype=np.int32)).cpu().numpy()
    assert g2.tobytes() == g.tobytes()
    # one non-finite baseline: that visibility is NaN in EVERY map (the empty one too), no other changes
    for bad in (np.nan, -np.inf):
        ub = u.copy()
        ub[17] = bad
        gb = call(p, f, s, ub).cpu().numpy()
        assert np.isnan(gb[:, 17].real).all() and np.isnan(gb[:, 17].imag).all()
        rest = [k for k in range(K_) if k != 17]
        assert gb[:, rest].tobytes() == g[:, rest].tobytes()
    # (bytes: the flagged visibilities hold NaN, which no == finds equal)
    assert call(p, f, s, u).cpu().numpy().tobytes() == g.tobytes(), "a repeated call gives the same bits"


# ---- 3: the list's image: K10 of components_image, and the models of real cleans ---------------------------
def test_k10_of_the_delta_image_agrees_within_both_bounds(eng):
    nx, nz, M, K_ = 67, 131, 2, 65
    rng = np.random.default_rng(4)
    p, f, _ = lists(rng, M, nx, nz, 1)
    ncomp = np.array([1000, 65], dtype=np.int32)
    d_p, d_f, d_n = dev(eng, p, np.int32), dev(eng, f), dev(eng, ncomp, np.int32)
    img = eng.components_image(d_p, d_f, d_n, nx, nz)
    assert tuple(img.shape) == (M, 1, nx * nz)
    h_img = img.cpu().numpy()
    for m in range(M):
        want = R.components_image_ref(p[m], f[m], None, int(ncomp[m]), nx, nz)
        assert h_img[m].tobytes() == want.tobytes(), "the delta image is the sequential sum"
    for amax in (0.5, 8.0):
        u, v = VR.random_points(rng, K_, 1.0)
        su, sv = amax * np.array([1.0, -0.37]), amax * np.array([0.61, 1.0])
        dense = eng.vis(img.reshape(M, nx * nz).contiguous(), nx, nz, su, sv, u, v).cpu().numpy()
        got = eng.vis_components(d_p, d_f, d_n, nx, nz, su, sv, u, v).cpu().numpy()
        for m in range(M):
            n, a, b = int(ncomp[m]), su[m] * u, sv[m] * v
            S = float(np.abs(f[m, :n]).sum())
            # K10's bound on sum |I| <= sum |f|, K18's on sum |f|, and the image's own float64 sums of
            # duplicated pixels: at most n roundings of at most u sum |f|
            tol = (VR.bound(a, b, nx, nz) + R.bound(a, b, nx, nz, n) + n * R.U) * S
            err = np.maximum(np.abs(dense[m].real - got[m].real), np.abs(dense[m].imag - got[m].imag))
            r = float((err / tol).max())
            WORST["K10 of the image |a| <= %g" % amax] = max(r, WORST.get("K10 of the image |a| <= %g" % amax, 0))
            assert r <= 1.0, (m, amax, r)


def test_components_image_equals_the_models_of_real_cleans(eng):
    import torch
    rng = np.random.default_rng(6)
    nx, nz, M = 33, 21, 2
    B = C.random_beam(rng, 2 * nx - 1, 2 * nz - 1)
    D = np.stack([C.random_image(rng, nx, nz, B) for _ in range(M)])
    res = dev(eng, D.reshape(M, -1))
    model = torch.zeros_like(res)
    cpix, cflux, ncomp, _ = eng.clean(res, nx, nz, dev(eng, B.reshape(-1)), 2 * nx - 1, 2 * nz - 1, 300, 0.2,
                                      [1e-3, 0.2], model=model)
    n = ncomp.cpu().numpy()
    assert n[0] > 100 and 0 < n[1] < n[0], n
    assert len(set(cpix[0, :n[0]].cpu().numpy().tolist())) < n[0], "pixels repeat: the order matters"
    img = eng.components_image(cpix, cflux, ncomp, nx, nz)
    assert torch.equal(img.reshape(M, -1), model), "rjp_clean's d_model, bit for bit"
    assert eng.lib.rjp_version() == 117
    # multi-scale: three planes, the delta model of each
    scales, psf = [0.0, 2.0, 4.0], (31, 31)
    parts = [K.scale_problem(rng, nx, nz, scales, psf=psf) for _ in range(M)]
    R0 = dev(eng, np.stack([q[0] for q in parts]).reshape(M, -1))
    X = dev(eng, np.stack([q[1] for q in parts]).reshape(M, -1))
    w = np.stack([q[2] for q in parts])
    model = torch.zeros_like(R0)
    cpix, cscale, cflux, ncomp, _ = eng.msclean(R0, 3, nx, nz, X, 31, 31, w, 200, 0.2, 1e-3, model=model)
    n = ncomp.cpu().numpy()
    assert n.min() > 20 and len(set(cscale[0, :n[0]].cpu().numpy().tolist())) > 1, n
    img = eng.components_image(cpix, cflux, ncomp, nx, nz, cscale=cscale, n_s=3)
    assert torch.equal(img.reshape(M, -1), model), "rjp_msclean's d_model, bit for bit"
    again = eng.components_image(cpix, cflux, ncomp, nx, nz, cscale=cscale, n_s=3)
    assert torch.equal(img, again)


# ---- 4: repeat, guard bands, refusals ----------------------------------------------------------------------
def test_repeat_and_guard_bands(eng):
    import torch
    nx, nz, M, K_, n_s = 67, 131, 3, 257, 3
    rng = np.random.default_rng(8)
    p, f, s = lists(rng, M, nx, nz, n_s)
    d_p, d_f, d_s = dev(eng, p, np.int32), dev(eng, f), dev(eng, s, np.int32)
    d_n = dev(eng, np.array([1000, 65, 300]), np.int32)
    u, v = VR.random_points(rng, K_, 1.0)
    su, sv = 0.5 * np.array(FACTORS), 0.4 * np.array(FACTORS)
    G = dev(eng, np.stack([R.random_g(rng, n_s, K_) for _ in range(M)]), np.complex128)
    d_u, d_v = dev(eng, u), dev(eng, v)
    guard, n_out = 4096, M * K_ * 2
    out = torch.full((guard + n_out + guard,), -7.0, dtype=torch.float64, device=eng.device)
    call = lambda o: raw(eng, d_p, d_s, d_f, d_n, M, STRIDE, n_s, nx, nz, su, sv, d_u, d_v, K_,
                         torch.view_as_real(G), None, 1, o[guard:])
    assert call(out) == R.workgroups(M, K_), eng.lib.rjp_last_error(eng.ctx)
    eng.synchronize()
    assert bool((out[:guard] == -7.0).all()) and bool((out[guard + n_out:] == -7.0).all())
    first = out[guard:guard + n_out]
    assert bool(torch.isfinite(first).all())
    via = eng.vis_components(d_p, d_f, d_n, nx, nz, su, sv, u, v, cscale=d_s, n_s=n_s, gvis=G)
    assert torch.equal(torch.view_as_real(via).reshape(-1), first)
    out2 = torch.full_like(out, -7.0)
    assert call(out2) == R.workgroups(M, K_)
    eng.synchronize()
    assert torch.equal(out2, out), "a repeated call gives the same bits"
    # the image: guard bands round [M][n_s][nx nz]
    n_img = M * n_s * nx * nz
    img = torch.full((guard + n_img + guard,), -7.0, dtype=torch.float64, device=eng.device)
    ret = eng.lib.rjp_components_image(eng.ctx, d_p.data_ptr(), d_s.data_ptr(), d_f.data_ptr(),
                                       d_n.data_ptr(), M, STRIDE, n_s, nx, nz, img[guard:].data_ptr(),
                                       eng._stream())
    assert ret == R.image_workgroups(M, n_s, nx, nz), eng.lib.rjp_last_error(eng.ctx)
    eng.synchronize()
    assert bool((img[:guard] == -7.0).all()) and bool((img[guard + n_img:] == -7.0).all())
    got = img[guard:guard + n_img].cpu().numpy().reshape(M, n_s, nx * nz)
    for m, n in enumerate((1000, 65, 300)):
        assert got[m].tobytes() == R.components_image_ref(p[m], f[m], s[m], n, nx, nz, n_s).tobytes()


def test_refusals_leave_poisoned_outputs_untouched(eng):
    import torch
    from rajepy_amd import _lib
    nx, nz, M, K_, n_s, stride = 5, 3, 2, 7, 2, 4
    d_p = dev(eng, np.zeros((M, stride)), np.int32)
    d_f = dev(eng, np.ones((M, stride)))
    d_n = dev(eng, np.full(M, stride), np.int32)
    d_u, d_v = dev(eng, np.linspace(0, 1, K_)), dev(eng, np.linspace(-1, 0, K_))
    G = dev(eng, np.ones((M, n_s, K_, 2)))
    su, sv = np.array([0.5, 0.25]), np.array([0.125, -0.5])
    out = torch.full((M * K_ * 2,), -7.0, dtype=torch.float64, device=eng.device)
    ok = dict(cpix=d_p, cscale=None, cflux=d_f, ncomp=d_n, M=M, stride=stride, n_s=n_s, nx=nx, nz=nz,
              su=su, sv=sv, u=d_u, v=d_v, K_=K_, gvis=G, vin=None, sign=1, out=out)
    nan = float("nan")
    bad = [("null", dict(cpix=None)), ("null", dict(cflux=None)), ("null", dict(ncomp=None)),
           ("null", dict(su=None)), ("null", dict(sv=None)), ("null", dict(u=None)), ("null", dict(v=None)),
           ("sizes", dict(M=0)), ("sizes", dict(stride=0)), ("sizes", dict(n_s=0)), ("sizes", dict(nx=0)),
           ("sizes", dict(nz=-1)), ("sizes", dict(K_=0)), ("sign", dict(sign=0)), ("sign", dict(sign=-2)),
           ("gvis", dict(gvis=None)), ("scales", dict(su=np.array([0.5, nan]))),
           ("scales", dict(sv=np.array([np.inf, 0.1]))), ("npix", dict(nx=46341, nz=46341)),
           # (64 x 2^25 workgroups: refused before anything is enqueued, so the small buffers do)
           ("wgs", dict(M=64, K_=2 ** 31 - 1, su=np.full(64, 0.5), sv=np.full(64, 0.25)))]
    for key, change in bad:
        args = dict(ok, **change)
        assert raw(eng, **args) == _lib.RJP_ERR_ARG, (key, change)
        assert eng.lib.rjp_last_error(eng.ctx).decode() == R.MSG[key], (key, change)
    args = dict(ok, out=None)
    assert raw(eng, **args) == _lib.RJP_ERR_ARG and eng.lib.rjp_last_error(eng.ctx).decode() == R.MSG["null"]
    eng.synchronize()
    assert bool((out == -7.0).all()), "a refusal touches nothing"
    assert raw(eng, **ok) == R.workgroups(M, K_)
    img = torch.full((M * n_s * nx * nz,), -7.0, dtype=torch.float64, device=eng.device)
    iok = [d_p.data_ptr(), None, d_f.data_ptr(), d_n.data_ptr(), M, stride, n_s, nx, nz, img.data_ptr()]
    for key, pos, val in (("img_null", 0, None), ("img_null", 2, None), ("img_null", 3, None),
                          ("img_null", 9, None), ("img_sizes", 4, 0), ("img_sizes", 5, 0),
                          ("img_sizes", 6, -1), ("img_sizes", 7, 0), ("img_sizes", 8, 0)):
        a = list(iok)
        a[pos] = val
        assert eng.lib.rjp_components_image(eng.ctx, *a, eng._stream()) == _lib.RJP_ERR_ARG, (key, pos)
        assert eng.lib.rjp_last_error(eng.ctx).decode() == R.MSG[key], (key, pos)
    a = list(iok)
    a[7] = a[8] = 46341
    assert eng.lib.rjp_components_image(eng.ctx, *a, eng._stream()) == _lib.RJP_ERR_ARG
    assert eng.lib.rjp_last_error(eng.ctx).decode() == R.MSG["img_npix"]
    a = list(iok)
    a[6], a[7], a[8] = 300, 46340, 46340             # 2 x 300 x 8388246 workgroups
    assert eng.lib.rjp_components_image(eng.ctx, *a, eng._stream()) == _lib.RJP_ERR_ARG
    assert eng.lib.rjp_last_error(eng.ctx).decode() == R.MSG["img_wgs"]
    eng.synchronize()
    assert bool((img == -7.0).all()), "a refusal touches nothing"
    assert eng.lib.rjp_components_image(eng.ctx, *iok, eng._stream()) == R.image_workgroups(M, n_s, nx, nz)
    # the engine's own checks
    for call in (lambda: eng.vis_components(d_p, d_f, d_n, nx, nz, su, sv, d_u, d_v[:3]),
                 lambda: eng.vis_components(d_p, d_f.to(torch.float32), d_n, nx, nz, su, sv, d_u, d_v),
                 lambda: eng.vis_components(d_p, d_f, d_n, nx, nz, su[:1], sv, d_u, d_v),
                 lambda: eng.vis_components(d_p, d_f, d_n, nx, nz, su, sv, d_u, d_v, n_s=2,
                                            gvis=G[:, :1].contiguous()),
                 lambda: eng.components_image(d_p, d_f, d_n[:1], nx, nz),
                 lambda: eng.components_image(d_p, d_f, d_n, 0, nz)):
        with pytest.raises(ValueError):
            call()
