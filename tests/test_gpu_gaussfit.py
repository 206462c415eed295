"""rjp_gaussfit (K14, imfit.hip: Levenberg-Marquardt fits of one elliptical Gaussian per map) through
the C-ABI, RTEngine.gaussfit and JetModel.clean_image_ff(imfit=...) / JetModel.imfit, against
tests/gaussfit_ref.py -- a long-double NumPy reference that FOLLOWS the device's trace (checks
(a)-(e) of its docstring, every bound derived there, none measured), which
tests/test_gaussfit_reference_cpu.py pins to hand-worked cases, to a float64 emulation (inside the
bounds) and to planted mistakes (outside).

The shapes are K12's: 5 x 3 (one tile, maps 8 bytes off a 16-byte line), 67 x 131 (9 tiles with a
ragged last one, an odd product), 130 x 65, and 600 x 600 (352 tiles: two reduction passes).  The
1e-9 on the noise-free fits is a sanity cap, not the accuracy judgement: that is the trace.  The
module prints the worst error / bound per group."""
import copy
import ctypes

import numpy as np
import pytest

from tests import gaussfit_ref as K
from tests import gpu_util as U
from tests import vis_ref as R

pytestmark = pytest.mark.gpu
YEAR = 31557600.0
WORST = {}
P_F, P_I, P_T = 7.25, -77, -7.5        # poison of the float outputs, the int outputs, the trace
GUARD = 33                             # elements of guard band on either side (odd: the payload of
                                       # a float64 buffer then starts 8 bytes off a 16-byte line)
LAM0, XTOL = 1e-3, 1e-12


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()
    print("\nworst error / bound per group: " +
          ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def note(kind, r):
    WORST[kind] = max(WORST.get(kind, 0.0), float(r))
    assert r <= 1.0, (kind, r)


class Band:
    """A device buffer of `n` elements between two guard bands of `guard` poisoned elements."""

    def __init__(self, eng, n, dtype, fill, guard=GUARD):
        import torch
        self.t = torch.full((guard + n + guard,), fill, dtype=dtype, device=eng.device)
        self.n, self.g, self.fill = n, guard, fill
        self.ptr = self.t.data_ptr() + guard * self.t.element_size()

    def set(self, host):
        import torch
        self.t[self.g:self.g + self.n] = torch.from_numpy(np.array(host).ravel()).to(self.t.device)
        return self

    def get(self):
        h = self.t.cpu().numpy()
        for band in (h[:self.g], h[self.g + self.n:]):
            assert np.array_equal(band, np.full(band.shape, self.fill, dtype=h.dtype)), "a guard band was written"
        return h[self.g:self.g + self.n].copy()


def run_fit(eng, D, box, mask, theta0, n_iter, lambda0=LAM0, xtol=XTOL, want_trace=True, guard=GUARD):
    """One raw rjp_gaussfit call on D [M, nx, nz], every buffer between guard bands -> dict of host
    arrays (theta, chi2, cov, npix, niter, status, trace, work, ret)."""
    import torch
    M, nx, nz = D.shape
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    img = Band(eng, D.size, f64, -1e300, guard).set(D)
    theta = Band(eng, M * 6, f64, P_F).set(np.broadcast_to(np.asarray(theta0, dtype=np.float64), (M, 6)))
    chi2, cov = Band(eng, M, f64, P_F), Band(eng, M * 21, f64, P_F)
    npix, niter, status = (Band(eng, M, i32, P_I) for _ in range(3))
    trace = Band(eng, M * n_iter * 9, f64, P_T)
    nb = K.box_pixels(box)
    wb = eng.lib.rjp_gaussfit_workspace(M, nb)
    assert wb == K.workspace_bytes(M, nb)
    work = Band(eng, wb, u8, 0xA5, 64)
    dmask = Band(eng, nx * nz, u8, 1, 3).set(np.asarray(mask != 0, dtype=np.uint8)) if mask is not None else None
    ret = eng.lib.rjp_gaussfit(eng.ctx, img.ptr, M, nx, nz, (ctypes.c_int32 * 4)(*box),
                               dmask.ptr if dmask else None, theta.ptr, lambda0, xtol, n_iter, chi2.ptr,
                               cov.ptr, npix.ptr, niter.ptr, status.ptr, trace.ptr if want_trace else None,
                               work.ptr, wb, eng._stream())
    eng.synchronize()
    assert ret == K.tiling(M, nb)["workgroups"], (ret, eng.lib.rjp_last_error(eng.ctx))
    back = img.get().reshape(D.shape)
    assert back.tobytes() == np.ascontiguousarray(D).tobytes(), "the images were written"
    if dmask:
        dmask.get()
    return dict(theta=theta.get().reshape(M, 6), chi2=chi2.get(), cov=cov.get().reshape(M, 21),
                npix=npix.get(), niter=niter.get(), status=status.get(),
                trace=trace.get().reshape(M, n_iter, 9), work=work.get(), ret=ret)


def one(out, m):
    return {k: out[k][m] for k in ("theta", "chi2", "cov", "npix", "niter", "status", "trace")}


def untouched(out, m, theta0):
    """Map m ended degenerate: status 3 and nothing else written."""
    assert out["status"][m] == 3
    assert np.array_equal(out["theta"][m], np.broadcast_to(theta0, out["theta"].shape)[m], equal_nan=True)
    assert out["chi2"][m] == P_F and np.all(out["cov"][m] == P_F)
    assert out["npix"][m] == P_I and out["niter"][m] == P_I and np.all(out["trace"][m] == P_T)


def follow_all(kind, D, box, mask, theta0, n_iter, out, lambda0=LAM0, xtol=XTOL):
    th0 = np.broadcast_to(np.asarray(theta0, dtype=np.float64), (D.shape[0], 6))
    for m in range(D.shape[0]):
        if out["status"][m] == 3:
            untouched(out, m, th0)
        else:
            note(kind, K.follow(D[m], box, mask, th0[m], lambda0, xtol, n_iter, one(out, m), P_T))


def same_bits(a, b):
    for k in ("theta", "chi2", "cov", "npix", "niter", "status", "trace", "work"):
        assert a[k].tobytes() == b[k].tobytes(), "a repeated call changed " + k


def gauss(nx, nz, th):
    ix, iz = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    return K.model(th, ix.ravel(), iz.ravel(), np.float64, with_jac=False)[0].reshape(nx, nz)


def truths(nx, nz):
    """Three sources for an nx x nz image: elongated and rotated, a negative peak, sub-pixel centres;
    widths that the image resolves (FWHM about a quarter of the shorter side)."""
    w = 0.25 * min(nx, nz)
    a = 4.0 * np.log(2.0) / w ** 2
    cx, cz = 0.5 * (nx - 1), 0.5 * (nz - 1)
    return np.array([[1.3, cx + 0.3, cz - 0.2, 1.9 * a, 0.6 * a, 0.8 * a],
                     [-0.7, cx - 0.45, cz + 0.35, 0.7 * a, -0.3 * a, 1.6 * a],
                     [2.5, cx + 0.05, cz + 0.49, a, 0.0, a]])


def start_of(eng, D, box, mask, abc):
    """engine.gauss_start on the device -> host [M, 6]."""
    import torch
    from rajepy_amd import engine as E
    M, nx, nz = D.shape
    t = torch.from_numpy(np.ascontiguousarray(D)).to(eng.device)
    return E.gauss_start(t, nx, nz, abc, box=box, mask=mask).cpu().numpy()


def beam_for(nx, nz):
    a = 4.0 * np.log(2.0) / (0.25 * min(nx, nz)) ** 2
    return (1.2 * a, 0.0, 1.2 * a)


def whole(nx, nz):
    return (0, nx - 1, 0, nz - 1)


def noise_free(eng, kind, nx, nz, box, mask=None, nan=False, guard=GUARD):
    tr = truths(nx, nz)
    D = np.stack([gauss(nx, nz, t) for t in tr])
    if nan:
        rng = np.random.default_rng(nx)
        D.reshape(3, -1)[:, rng.choice(nx * nz, nx * nz // 50, replace=False)] = np.nan
        D[:, 0, 0] = np.inf
    th0 = start_of(eng, D, box, mask, beam_for(nx, nz))
    out = run_fit(eng, D, box, mask, th0, 60, guard=guard)
    follow_all(kind, D, box, mask, th0, 60, out)
    assert np.all(out["status"] == 1), out["status"]
    err = np.abs(out["theta"] - tr) / np.stack([K.scales(t) for t in tr]).astype(np.float64)
    print("%s noise-free: iterations %s, worst |theta - truth| / s %.2e" % (kind, out["niter"], err.max()))
    assert err.max() <= 1e-9, err
    return D, th0, out


def noisy(eng, kind, nx, nz, box, mask, n_iter, level, seed, want_status=True):
    tr = truths(nx, nz)
    rng = np.random.default_rng(seed)
    D = np.stack([gauss(nx, nz, t) + level * abs(t[0]) * rng.standard_normal((nx, nz)) for t in tr])
    th0 = start_of(eng, D, box, mask, beam_for(nx, nz))
    out = run_fit(eng, D, box, mask, th0, n_iter)
    follow_all(kind, D, box, mask, th0, n_iter, out)
    print("%s noisy: iterations %s, status %s" % (kind, out["niter"], out["status"]))
    if want_status:
        assert np.all(out["status"] == 1), out["status"]
    return D, th0, out


# ---- 1: the shapes, at the bounds ----------------------------------------------------------------
def test_five_by_three(eng):
    """15 pixels, one tile; 15 doubles per map, so every other map of the stack starts 8 bytes off
    a 16-byte line whatever the guard."""
    nx, nz = 5, 3
    tr = np.array([[1.0, 2.2, 1.1, 0.30, 0.05, 0.50], [-0.8, 1.8, 0.9, 0.45, -0.10, 0.35],
                   [2.0, 2.1, 0.9, 0.42, 0.02, 0.38]])
    D = np.stack([gauss(nx, nz, t) for t in tr])
    for guard in (GUARD, GUARD + 1):
        th0 = start_of(eng, D, whole(nx, nz), None, (0.4, 0.0, 0.4))
        out = run_fit(eng, D, whole(nx, nz), None, th0, 60, guard=guard)
        follow_all("5 x 3", D, whole(nx, nz), None, th0, 60, out)
        assert np.all(out["status"] == 1) and np.all(out["npix"] == 15), (out["status"], out["npix"])
        err = np.abs(out["theta"] - tr) / np.stack([K.scales(t) for t in tr]).astype(np.float64)
        print("5 x 3 noise-free: iterations %s, worst |theta - truth| / s %.2e" % (out["niter"], err.max()))
        assert err.max() <= 1e-9, err


@pytest.mark.parametrize("nx,nz", [(67, 131), (130, 65)])
def test_tails_and_tiles_against_the_reference(eng, nx, nz):
    """The whole image, a strict sub-box and a mask with NaN pixels; noise-free and noisy; with
    and without the trace; a repeated call."""
    kind = "%d x %d" % (nx, nz)
    sub = (nx // 6, nx - nx // 7, nz // 5, nz - nz // 8)
    mask = np.ones((nx, nz), dtype=bool)
    mask[::7, ::5] = False
    D, th0, a = noise_free(eng, kind, nx, nz, whole(nx, nz))
    same_bits(a, run_fit(eng, D, whole(nx, nz), None, th0, 60))
    b = run_fit(eng, D, whole(nx, nz), None, th0, 60, guard=GUARD + 1)      # maps 8 bytes further on
    for k in ("theta", "chi2", "cov", "npix", "niter", "status", "trace"):
        assert a[k].tobytes() == b[k].tobytes(), k
    c = run_fit(eng, D, whole(nx, nz), None, th0, 60, want_trace=False)     # d_trace = NULL
    assert np.all(c["trace"] == P_T) and c["theta"].tobytes() == a["theta"].tobytes()
    assert c["cov"].tobytes() == a["cov"].tobytes() and c["niter"].tobytes() == a["niter"].tobytes()
    noise_free(eng, kind + " (box)", nx, nz, sub)
    noise_free(eng, kind + " (mask, NaN)", nx, nz, whole(nx, nz), mask=mask, nan=True)
    noisy(eng, kind + " (noisy)", nx, nz, whole(nx, nz), None, 60, 0.01, 11)
    noisy(eng, kind + " (noisy, box, mask)", nx, nz, sub, mask, 60, 0.02, 12)


def test_more_tiles_than_one_reduction_pass(eng):
    nx = nz = 600
    assert K.tiling(1, nx * nz)["tiles"] == 352 > K.REDUCE_PASS
    # a source of FWHM 6 x 9 pixels in the tiles beyond the first pass
    tr = np.array([[1.3, 571.3, 588.6, 0.077, 0.012, 0.034]])
    assert 571 * nz > K.REDUCE_PASS * K.TILE
    rng = np.random.default_rng(600)
    D = gauss(nx, nz, tr[0])[None] + 0.01 * rng.standard_normal((1, nx, nz))
    th0 = start_of(eng, D, whole(nx, nz), None, (0.05, 0.0, 0.05))
    out = run_fit(eng, D, whole(nx, nz), None, th0, 10)
    follow_all("600 x 600", D, whole(nx, nz), None, th0, 10, out)
    assert out["npix"][0] == nx * nz and out["status"][0] in (0, 1)


# ---- 2: behaviour per map -------------------------------------------------------------------------
def test_fixed_point_degenerate_maps_and_the_rest_of_the_stack(eng):
    """A map at its fixed point (one pixel of 1.5, a Gaussian so narrow that every other pixel's
    exponent lies below -700: chi^2 is an exact 0) ends after one trial; an all-NaN map and a map
    with five counting pixels end with status 3 and nothing written; a bad start likewise; the
    good map between them is fitted as if alone."""
    nx, nz = 67, 131
    good = gauss(nx, nz, truths(nx, nz)[0])
    spike = np.zeros((nx, nz))
    spike[30, 70] = 1.5
    few = np.full((nx, nz), np.nan)
    few[30, 68:73] = 1.0
    D = np.stack([spike, np.full((nx, nz), np.nan), good, few, good])
    th_good = start_of(eng, good[None], whole(nx, nz), None, beam_for(nx, nz))[0]
    th0 = np.stack([[1.5, 30.0, 70.0, 800.0, 0.0, 800.0], th_good, th_good, th_good,
                    [1.0, 30.0, 70.0, 0.01, 0.02, 0.01]])                   # the last: A C < B^2
    out = run_fit(eng, D, whole(nx, nz), None, th0, 60)
    follow_all("per map", D, whole(nx, nz), None, th0, 60, out)
    assert list(out["status"]) == [1, 3, 1, 3, 3]
    assert out["niter"][0] == 1 and out["chi2"][0] == 0.0 and np.array_equal(out["theta"][0], th0[0])
    alone = run_fit(eng, good[None], whole(nx, nz), None, th_good, 60)
    for k in ("theta", "chi2", "cov", "npix", "niter", "trace"):
        assert out[k][2].tobytes() == alone[k][0].tobytes(), k
    # a non-finite start
    bad = th0.copy()
    bad[2, 1] = np.nan
    out = run_fit(eng, D, whole(nx, nz), None, bad, 60)
    assert list(out["status"]) == [1, 3, 3, 3, 3]
    follow_all("per map", D, whole(nx, nz), None, bad, 60, out)


def test_a_box_of_five_pixels_leaves_every_map_untouched(eng):
    """A 1 x 5 box (one ragged tile, i0 = i1) holds fewer than 6 counting pixels whatever the
    images: every map of the stack ends with status 3 and nothing else of it is written; a 1 x 6
    box of which the mask takes one pixel likewise; the 1 x 6 box itself counts 6 and is fitted."""
    nx, nz = 67, 131
    D = np.stack([gauss(nx, nz, t) for t in truths(nx, nz)])
    th0 = start_of(eng, D, whole(nx, nz), None, beam_for(nx, nz))
    out = run_fit(eng, D, (33, 33, 63, 67), None, th0, 20)
    assert list(out["status"]) == [3, 3, 3] and out["ret"] == 3
    follow_all("small box", D, (33, 33, 63, 67), None, th0, 20, out)
    mask = np.ones((nx, nz), dtype=bool)
    mask[33, 65] = False
    out = run_fit(eng, D, (33, 33, 63, 68), mask, th0, 20)
    assert list(out["status"]) == [3, 3, 3]
    follow_all("small box", D, (33, 33, 63, 68), mask, th0, 20, out)
    out = run_fit(eng, D, (33, 33, 63, 68), None, th0, 20)
    assert np.all(out["status"] != 3) and np.all(out["npix"] == 6)
    follow_all("small box", D, (33, 33, 63, 68), None, th0, 20, out)


def test_exhausted_and_continued(eng):
    nx, nz = 67, 131
    tr = truths(nx, nz)
    D = np.stack([gauss(nx, nz, t) for t in tr])
    th0 = start_of(eng, D, whole(nx, nz), None, beam_for(nx, nz))
    first = run_fit(eng, D, whole(nx, nz), None, th0, 3)
    follow_all("exhausted", D, whole(nx, nz), None, th0, 3, first)
    assert np.all(first["status"] == 0) and np.all(first["niter"] == 3)
    second = run_fit(eng, D, whole(nx, nz), None, first["theta"], 60)
    follow_all("continued", D, whole(nx, nz), None, first["theta"], 60, second)
    long = run_fit(eng, D, whole(nx, nz), None, th0, 60)
    assert np.all(second["status"] == 1) and np.all(long["status"] == 1)
    sc = np.stack([K.scales(t) for t in tr]).astype(np.float64)
    assert np.max(np.abs(second["theta"] - long["theta"]) / sc) <= 1e-9
    assert np.max(np.abs(second["theta"] - tr) / sc) <= 1e-9


def test_engine_gaussfit(eng):
    import torch
    nx, nz = 67, 131
    sub = (5, 60, 10, 120)
    mask = np.ones((nx, nz), dtype=bool)
    mask[::7, ::5] = False
    D, th0, _ = noisy(eng, "engine", nx, nz, sub, mask, 40, 0.01, 5)
    raw = run_fit(eng, D, sub, mask, th0, 40)
    img = torch.from_numpy(D.reshape(3, -1)).to(eng.device)
    fit = eng.gaussfit(img, nx, nz, th0, box=sub, mask=mask, n_iter=40, trace=True)
    assert eng.last_gaussfit_tiles == raw["ret"] == 3 * 7
    assert fit["status"].dtype == torch.int32 and fit["trace"].shape == (3, 40, 9)
    for k in ("theta", "chi2", "cov", "npix", "niter", "status"):
        assert fit[k].cpu().numpy().tobytes() == raw[k].tobytes(), k
    tr = fit["trace"].cpu().numpy()
    for m in range(3):
        n = raw["niter"][m]
        assert tr[m, :n].tobytes() == raw["trace"][m, :n].tobytes() and np.all(np.isnan(tr[m, n:]))
    assert "trace" not in eng.gaussfit(img, nx, nz, th0[0], n_iter=2)
    for bad in (dict(n_iter=0), dict(box=(5, 67, 0, 3)), dict(box=(6, 5, 0, 3)), dict(lambda0=0.0),
                dict(xtol=float("nan")), dict(mask=np.ones(5))):
        with pytest.raises(ValueError):
            eng.gaussfit(img, nx, nz, th0, **bad)
    with pytest.raises(ValueError):
        eng.gaussfit(img[:, :-1].contiguous(), nx, nz, th0)
    with pytest.raises(ValueError):
        eng.gaussfit(img, nx, nz, th0[:2])


# ---- 3: refusals ----------------------------------------------------------------------------------
G_NULLS, G_SIZES, G_NPIX, G_BOX, G_TOL, G_ITER, G_WGS, G_SHORT = (K.MSG[k] for k in (
    "nulls", "sizes", "npix", "box", "tol", "iter", "wgs", "short"))


def test_refusals_leave_poisoned_outputs_untouched(eng):
    import torch
    from rajepy_amd import _lib
    M, nx, nz, n_iter = 2, 5, 3, 4
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    full = lambda n, v, dt: torch.full((n,), v, dtype=dt, device=eng.device)
    wb = eng.lib.rjp_gaussfit_workspace(M, nx * nz)
    bufs = dict(img=full(M * nx * nz, 7.0, f64), mask=full(nx * nz, 1, u8), theta=full(M * 6, 0.5, f64),
                chi2=full(M, P_F, f64), cov=full(M * 21, P_F, f64), npix=full(M, P_I, i32),
                niter=full(M, P_I, i32), status=full(M, P_I, i32), trace=full(M * n_iter * 9, P_T, f64),
                work=full(wb, 0xA5, u8))
    before = {k: t.clone() for k, t in bufs.items()}
    good = dict(bufs, n_maps=M, nx=nx, nz=nz, box=(0, 4, 0, 2), lam=1e-3, xtol=1e-12, n_iter=n_iter,
                nbytes=wb, ctx=True)
    ptr = lambda t: t.data_ptr() if t is not None else None

    def fit(a):
        box = (ctypes.c_int32 * 4)(*a["box"]) if a["box"] is not None else None
        return eng.lib.rjp_gaussfit(eng.ctx if a["ctx"] else None, ptr(a["img"]), a["n_maps"], a["nx"], a["nz"],
                                    box, ptr(a["mask"]), ptr(a["theta"]), a["lam"], a["xtol"], a["n_iter"],
                                    ptr(a["chi2"]), ptr(a["cov"]), ptr(a["npix"]), ptr(a["niter"]),
                                    ptr(a["status"]), ptr(a["trace"]), ptr(a["work"]), a["nbytes"],
                                    eng._stream())

    ARG, WS = _lib.RJP_ERR_ARG, _lib.RJP_ERR_WORKSPACE
    inf, nan = float("inf"), float("nan")
    many = dict(n_maps=2 ** 30 + 1, nx=1025, nz=1, box=(0, 1024, 0, 0))
    cases = [("NULL " + k, {k: None}, ARG, G_NULLS)
             for k in ("img", "box", "theta", "chi2", "cov", "npix", "niter", "status")]
    cases += [("n_maps 0", dict(n_maps=0), ARG, G_SIZES), ("nx 0", dict(nx=0), ARG, G_SIZES),
              ("nz -1", dict(nz=-1), ARG, G_SIZES),
              ("nx nz 2^31", dict(nx=2 ** 16, nz=2 ** 15), ARG, G_NPIX),
              ("i0 < 0", dict(box=(-1, 4, 0, 2)), ARG, G_BOX), ("i1 = nx", dict(box=(0, 5, 0, 2)), ARG, G_BOX),
              ("i1 < i0", dict(box=(3, 2, 0, 2)), ARG, G_BOX), ("j0 < 0", dict(box=(0, 4, -1, 2)), ARG, G_BOX),
              ("j1 = nz", dict(box=(0, 4, 0, 3)), ARG, G_BOX), ("j1 < j0", dict(box=(0, 4, 2, 1)), ARG, G_BOX),
              ("lambda0 0", dict(lam=0.0), ARG, G_TOL), ("lambda0 inf", dict(lam=inf), ARG, G_TOL),
              ("lambda0 nan", dict(lam=nan), ARG, G_TOL), ("xtol -1", dict(xtol=-1.0), ARG, G_TOL),
              ("xtol nan", dict(xtol=nan), ARG, G_TOL), ("xtol inf", dict(xtol=inf), ARG, G_TOL),
              ("n_iter 0", dict(n_iter=0), ARG, G_ITER),
              # 1025 x 1 with the whole image as the box: 2 tiles; 2^30 + 1 maps: 2^31 + 2 workgroups
              # (nothing is dereferenced before the refusal, so the small buffers do)
              ("2^31 + 2 workgroups", dict(many), ARG, G_WGS),
              ("workgroups beat the workspace", dict(many, nbytes=0, work=None), ARG, G_WGS),
              ("n_iter beats the workgroups", dict(many, n_iter=0), ARG, G_ITER),
              ("2^31 - 1 workgroups are allowed", dict(n_maps=2 ** 31 - 1, nbytes=0), WS, G_SHORT),
              ("short workspace", dict(nbytes=wb - 1), WS, G_SHORT),
              ("NULL workspace", dict(work=None), WS, G_SHORT),
              # which one wins: the order of check_gaussfit, the workspace last
              ("NULL beats sizes", dict(img=None, nx=0), ARG, G_NULLS),
              ("sizes beat the box", dict(nx=0, box=(3, 2, 0, 2)), ARG, G_SIZES),
              ("npix beats the box", dict(nx=2 ** 16, nz=2 ** 15, box=(-1, 0, 0, 0)), ARG, G_NPIX),
              ("box beats lambda0", dict(box=(3, 2, 0, 2), lam=0.0), ARG, G_BOX),
              ("lambda0 beats n_iter", dict(lam=0.0, n_iter=0), ARG, G_TOL),
              ("n_iter beats the workspace", dict(n_iter=0, nbytes=0), ARG, G_ITER)]
    for what, change, code, msg in cases:
        assert fit(dict(good, **change)) == code, what
        assert eng.lib.rjp_last_error(eng.ctx).decode() == msg, what
    assert fit(dict(good, ctx=False)) == ARG
    eng.synchronize()
    for k, t in bufs.items():
        assert torch.equal(t, before[k]), "a refusal wrote " + k
    assert eng.lib.rjp_gaussfit_workspace(0, 15) == 0 and eng.lib.rjp_gaussfit_workspace(2, 0) == 0
    # optional pointers may be NULL
    assert fit(dict(good, mask=None, trace=None)) == 2
    eng.synchronize()


# ---- 4: the model level ---------------------------------------------------------------------------
def _params(tag):
    p = copy.deepcopy(U.load_golden(tag)[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


SHAPE = (31, 41)


def test_clean_image_ff_imfit_on_the_example_model(eng, tmp_path_factory):
    """The example jet at 50, 40 and 32 GHz, imaged on cells four times the model's with beams of
    8 to 13 cells (the jet is barely resolved, as in the reference's synthetic observations): the
    fitted integrated flux against the flux CLEAN found."""
    from rajepy_amd import classes, logger
    from rajepy_amd import engine as E
    log = logger.Log(str(tmp_path_factory.mktemp("imfit") / "m.log"), verbose=False)
    jm = classes.JetModel(_params("cfg1_example"), log=log, engine=eng)
    freqs = 5e10 * np.array([1.0, 0.8, 0.64])
    jm.time = 1.0 * YEAR
    cell = 4.0 * np.arctan(jm.csize * E.con.au / (jm.params["target"]["dist"] * E.con.parsec))
    cell_as = np.degrees(cell) * 3600.0
    su, _ = jm._vis_scales(freqs)
    rng = np.random.default_rng(3)
    u, v = R.random_points(rng, 60, 0.02 / np.abs(su).max())
    w = rng.lognormal(0.0, 0.5, 60)
    kw = dict(weights=w, shape=SHAPE, cell_as=cell_as, niter=300, threshold_jy=0.0)
    plain = jm.clean_image_ff(u, v, freqs, **kw)
    assert plain.imfit is None and len(plain) == 6 and "imfit" not in plain._fields
    res = jm.clean_image_ff(u, v, freqs, imfit=True, **kw)
    # imfit=None takes the path of the code before the keyword: the same bits in every product
    for k in ("image", "residual", "model", "peak_residual"):
        assert getattr(plain, k).tobytes() == getattr(res, k).tobytes(), k
    assert len(res.imfit) == 3
    for m, fit in enumerate(res.imfit):
        assert fit["status"] == 1 and fit["npix"] == SHAPE[0] * SHAPE[1], fit
        A, B, C = E.beam_quadratic(*res.beam[m], cell)
        omega = np.pi / np.sqrt(A * C - B * B)                       # the beam area in cells
        flux = res.components[m][:, 2].sum() + res.residual[m].sum() / omega
        rel = abs(fit["I"]["val"] - flux) / abs(flux)
        print("map %d: fitted I %.6e Jy, components + residual / beam area %.6e Jy, relative difference "
              "%.3e; centre (%.2f, %.2f), fitted %s, beam %s, deconvolved %s"
              % (m, fit["I"]["val"], flux, rel, fit["x0"], fit["z0"],
                 (fit["maj_as"], fit["min_as"], fit["pa_deg"]), res.beam[m], fit["deconvolved"]))
        # The margin: MEASURED on the first run of this test, 6.8e-3, 4.8e-3 and 3.0e-3 for the
        # three channels.  It is no rounding bound: the restored jet is not one Gaussian (two
        # lobes under a beam of 8 to 13 cells), so the integral of the best single Gaussian
        # differs from the sum of the image by the misfit, which grows as the beam resolves the
        # jet (1e-2 to 4e-2 at 4 cells per beam).  1.5e-2 is twice the worst of the three.
        assert rel <= 1.5e-2, (m, rel)
        assert abs(fit["x0"] - 15.0) <= 1.0 and abs(fit["z0"] - 20.0) <= 4.0      # on the jet
        assert fit["maj_as"] >= res.beam[m][1] and not fit["point_source"]
    # JetModel.imfit on the images reproduces CleanResult.imfit: the beam goes through
    # beam_from_quadratic / beam_quadratic (1e-9 relative, tests/test_gpu_clean.py), the fit stops
    # at steps of 1e-12 of the scale
    again = jm.imfit(res.image, res.beam, cell_as=cell_as)
    one_ = jm.imfit(res.image[1], res.beam[1], cell_as=cell_as)
    for m in range(3):
        for k in ("peak", "x0", "z0", "maj_as", "min_as"):
            assert abs(again[m][k] - res.imfit[m][k]) <= 1e-7 * abs(res.imfit[m][k]), (m, k)
        assert abs(again[m]["I"]["val"] - res.imfit[m]["I"]["val"]) <= 1e-7 * abs(res.imfit[m]["I"]["val"])
    assert abs(one_[0]["I"]["val"] - res.imfit[1]["I"]["val"]) <= 1e-7 * abs(res.imfit[1]["I"]["val"])
    # options: a box, an iteration count, a start and an rms per map as device tensors; chunks of
    # one map
    import torch
    start = torch.tensor([[f["peak"], f["x0"], f["z0"], *E.beam_quadratic(*b, cell)]
                          for f, b in zip(res.imfit, res.beam)], dtype=torch.float64, device=eng.device)
    rms = torch.full((3,), 1e-6, dtype=torch.float64, device=eng.device)
    old = jm.VIS_STACK_BYTES
    try:
        jm.VIS_STACK_BYTES = 8 * (3 * SHAPE[0] * SHAPE[1] + 61 * 81)
        opt = jm.clean_image_ff(u, v, freqs, imfit=dict(box=(5, 25, 8, 32), n_iter=40, rms=rms,
                                                        theta0=start), **kw)
    finally:
        jm.VIS_STACK_BYTES = old
    assert opt.image.tobytes() == res.image.tobytes()
    assert all(f["npix"] == 21 * 25 and f["status"] == 1 and f["Ierr"]["val"] > 0 for f in opt.imfit)
    with pytest.raises(ValueError):
        jm.clean_image_ff(u, v, freqs, imfit=dict(box=(2, 31, 3, 18)), **kw)
    with pytest.raises(ValueError):
        jm.clean_image_ff(u, v, freqs, imfit=dict(boxx=(2, 12, 3, 18)), **kw)
