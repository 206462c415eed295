"""rjp_convolve2d (convolve.hip) and rjp_msclean (K17, msclean.hip) through the C-ABI,
RTEngine.convolve2d / msclean and JetModel.clean_image_ff(scales=...), against tests/msclean_ref.py:
the long-double convolution in the stated term order, and the long-double multi-scale CLEAN that
FOLLOWS the device's component list.  tests/test_msclean_reference_cpu.py pins both to hand-worked
cases, to a float64 emulation (inside the bounds) and to planted mistakes (outside).

The bounds are derived in tests/msclean_ref.py, not measured:
    convolution, per pixel:   (kx kz + 1) 2^-53 (|add| + sum |ker| |in|)
    plane l, pixel q:         (updates of q) x 2^-53 x (|R0_l[q]| + sum_c |f_c| |X[k_c][l]|)
The module prints the worst error / bound per group."""
import copy

import numpy as np
import pytest

from tests import clean_ref as C
from tests import gpu_util as U
from tests import msclean_ref as K
from tests import test_gpu_clean as G

pytestmark = pytest.mark.gpu
YEAR = 31557600.0
LD = np.longdouble
WORST = {}
POISON_PIX, POISON_F = -77, 7.25
GUARD = 33
Band = G.Band


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


# ---- 1: the convolution ------------------------------------------------------------------------------
def run_conv(eng, img, ker, add=None, guard=GUARD):
    """One raw rjp_convolve2d call on img [M, nx, nz] with ker [n_ker, kx, kz], every buffer between
    guard bands -> out [M, nx, nz]; the returned count is held to the tile rule."""
    import torch
    M, nx, nz = img.shape
    n_ker, kx, kz = ker.shape
    f64 = torch.float64
    din = Band(eng, img.size, f64, 1e300, guard).set(img)
    dker = Band(eng, ker.size, f64, 1e300, guard).set(ker)
    dadd = Band(eng, img.size, f64, 1e300, guard).set(add) if add is not None else None
    out = Band(eng, img.size, f64, -1e300, guard)
    ret = eng.lib.rjp_convolve2d(eng.ctx, din.ptr, M, nx, nz, dker.ptr, n_ker, kx, kz,
                                 dadd.ptr if dadd else None, out.ptr, eng._stream())
    eng.synchronize()
    assert ret == K.conv_workgroups(M, nx, nz), (ret, eng.lib.rjp_last_error(eng.ctx))
    assert din.get().tobytes() == np.ascontiguousarray(img).tobytes()
    dker.get()
    return out.get().reshape(img.shape)


CONV_CASES = [  # nx, nz, kx, kz
    (1, 1, 1, 1), (1, 1, 3, 5), (5, 3, 1, 1), (5, 3, 3, 5), (5, 3, 9, 9), (67, 131, 3, 5),
    (67, 131, 31, 31), (67, 131, 129, 129), (130, 65, 3, 5), (130, 65, 31, 31), (130, 65, 1, 1)]


@pytest.mark.parametrize("nx,nz,kx,kz", CONV_CASES)
def test_convolution_against_the_long_double_sum(eng, nx, nz, kx, kz):
    """Kernels with random signs (asymmetric), n_ker = 1 and = n_maps, `add` NULL and given, a NaN and
    an infinite pixel (the NaN pattern exactly the reference's), guard bands, a repeated call."""
    rng = np.random.default_rng(1000 * nx + 10 * kx + kz)
    M = 1 if kx == 129 else 2
    img = rng.standard_normal((M, nx, nz))
    add = rng.standard_normal((M, nx, nz))
    kind = "conv %d x %d" % (kx, kz)
    for n_ker in sorted({1, M}):
        ker = rng.standard_normal((n_ker, kx, kz))
        for with_add in ((False, True) if kx < 129 else (True,)):
            got = run_conv(eng, img, ker, add if with_add else None)
            for m in range(M):
                note(kind, K.check_conv(got[m], img[m], ker[m if n_ker > 1 else 0], add[m] if with_add else None))
    again = run_conv(eng, img, ker, add)
    assert again.tobytes() == got.tobytes(), "a repeated call changed the bits"
    assert run_conv(eng, img, ker, add, guard=GUARD + 1).tobytes() == got.tobytes()   # 8 bytes off
    if nx * nz > 1:
        bad = img.copy()
        bad[0].ravel()[(nx * nz) // 3] = np.nan
        bad[M - 1].ravel()[(2 * nx * nz) // 3] = np.inf
        bad[0, nx - 1, nz - 1] = -np.inf
        got = run_conv(eng, bad, ker, add)
        for m in range(M):
            note(kind + " (NaN, inf)", K.check_conv(got[m], bad[m], ker[m if n_ker > 1 else 0], add[m]))
        assert np.isnan(got).any()


def test_convolution_identity_and_engine_path(eng):
    import torch
    rng = np.random.default_rng(8)
    nx, nz = 67, 131
    img = rng.standard_normal((3, nx, nz))
    one = np.ones((1, 1, 1))
    assert run_conv(eng, img, one).tobytes() == img.tobytes()               # fma(1, x, 0) = x
    delta = np.zeros((1, 5, 7))
    delta[0, 2, 3] = 1.0
    assert np.array_equal(run_conv(eng, img, delta), img)                      # (0 x + x: -0 aside)
    shift = np.zeros((1, 5, 7))
    shift[0, 0, 1] = 1.0                                       # ker[a, b] moves a source by (a - ca, b - cb)
    got = run_conv(eng, img, shift)
    want = np.zeros_like(img)
    want[:, :nx - 2, :nz - 2] = img[:, 2:, 2:]
    assert np.array_equal(got, want)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(eng.device)
    ker = rng.standard_normal((3, 5))
    out = eng.convolve2d(dev(img.reshape(3, -1)), nx, nz, dev(ker), 3, 5)
    assert eng.last_convolve2d_workgroups == 3 * 5 * 3 and out.shape == (3, nx * nz)
    assert out.cpu().numpy().tobytes() == run_conv(eng, img, ker[None]).tobytes()
    chained = eng.convolve2d(dev(img.reshape(3, -1)), nx, nz, dev(ker), 3, 5, add=out)
    assert chained.cpu().numpy().tobytes() == run_conv(eng, img, ker[None], out.cpu().numpy().reshape(img.shape)).tobytes()
    for bad in (lambda: eng.convolve2d(dev(img.reshape(3, -1)), nx, nz, dev(ker), 5, 5),
                lambda: eng.convolve2d(dev(img.reshape(3, -1))[:, :-1].contiguous(), nx, nz, dev(ker), 3, 5),
                lambda: eng.convolve2d(dev(img.reshape(3, -1)), nx, nz, dev(ker), 3, 5, add=dev(img[0])),
                lambda: eng.convolve2d(dev(img.reshape(3, -1)), 0, nz, dev(ker), 3, 5)):
        with pytest.raises(ValueError):
            bad()


# ---- 2: the multi-scale CLEAN ---------------------------------------------------------------------------
def run_ms(eng, R0, X, weight, mask, thresh, gain, n_iter, model0=None, want_peak=True, guard=GUARD):
    """One raw rjp_msclean call on R0 [M, n_s, nx, nz] with X [n_psf, tri, px, pz] and weight [M, n_s],
    every buffer between guard bands -> dict of host arrays."""
    import torch
    from rajepy_amd import _lib
    M, n_s, nx, nz = R0.shape
    n_psf, ntri, px, pz = X.shape
    assert ntri == n_s * (n_s + 1) // 2
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    res = Band(eng, R0.size, f64, -1e300, guard).set(R0)
    psf = Band(eng, X.size, f64, 1e300, guard).set(X)
    cpix = Band(eng, M * n_iter, i32, POISON_PIX)
    cscale = Band(eng, M * n_iter, i32, POISON_PIX)
    cflux = Band(eng, M * n_iter, f64, POISON_F)
    ncomp = Band(eng, M, i32, POISON_PIX)
    model = Band(eng, R0.size, f64, -1e300).set(np.zeros(R0.size) if model0 is None else model0)
    peak = Band(eng, M, f64, POISON_F)
    wb = eng.lib.rjp_msclean_workspace(M, n_s, nx, nz)
    assert wb == K.ms_workspace_bytes(M, n_s, nx, nz)
    work = Band(eng, wb, u8, 0xA5, 64)
    dmask = Band(eng, nx * nz, u8, 1, 3).set(np.asarray(mask != 0, dtype=np.uint8)) if mask is not None else None
    w = np.ascontiguousarray(np.broadcast_to(np.asarray(weight, dtype=np.float64).reshape(-1, n_s), (M, n_s)))
    ret = eng.lib.rjp_msclean(eng.ctx, res.ptr, M, n_s, nx, nz, psf.ptr, n_psf, px, pz, _lib.dbl_array(w),
                              dmask.ptr if dmask else None, _lib.dbl_array(np.broadcast_to(thresh, (M,))),
                              float(gain), n_iter, cpix.ptr, cscale.ptr, cflux.ptr, ncomp.ptr, model.ptr,
                              peak.ptr if want_peak else None, work.ptr, wb, eng._stream())
    eng.synchronize()
    assert ret == K.ms_workgroups(M, n_s, nx, nz), (ret, eng.lib.rjp_last_error(eng.ctx))
    psf.get()
    if dmask:
        dmask.get()
    return dict(res=res.get().reshape(R0.shape), cpix=cpix.get().reshape(M, n_iter),
                cscale=cscale.get().reshape(M, n_iter), cflux=cflux.get().reshape(M, n_iter),
                ncomp=ncomp.get(), model=model.get().reshape(R0.shape), peak=peak.get(), work=work.get(),
                ret=ret, weight=w)


def follow_all(kind, R0, X, weight, mask, thresh, gain, n_iter, out, model0=None, want_peak=True):
    M, n_s = R0.shape[:2]
    th = np.broadcast_to(thresh, (M,))
    w = np.broadcast_to(np.asarray(weight, dtype=np.float64).reshape(-1, n_s), (M, n_s))
    for m in range(M):
        Xm = X[m if X.shape[0] > 1 else 0]
        r = K.follow(R0[m], Xm, w[m], mask, th[m], gain, n_iter, out["cpix"][m], out["cscale"][m],
                     out["cflux"][m], out["ncomp"][m], out["res"][m], peak=out["peak"][m] if want_peak else None,
                     model=out["model"][m], model0=None if model0 is None else model0[m],
                     poison_pix=POISON_PIX, poison_flux=POISON_F)
        note(kind, r)
        note(kind + " (identity)", K.conservation(R0[m], Xm, out["cpix"][m], out["cscale"][m], out["cflux"][m],
                                                  out["ncomp"][m], out["res"][m]))
    if not want_peak:
        assert np.all(out["peak"] == POISON_F), "d_peak = NULL was written"


def same_bits(a, b):
    for k in ("res", "cpix", "cscale", "cflux", "ncomp", "model", "peak", "work"):
        assert a[k].tobytes() == b[k].tobytes(), "a repeated call changed " + k


_PROBLEMS = {}


def problems(seed, M, n_psf, nx, nz, scales, psf=None, nan=False):
    """M maps of `msclean_ref.scale_problem`, computed once per key and never changed: (R0 [M, n_s, nx,
    nz], X [n_psf, tri, px, pz], weight [M, n_s])."""
    key = (seed, M, n_psf, nx, nz, tuple(scales), psf, nan)
    if key not in _PROBLEMS:
        rng = np.random.default_rng(seed)
        parts = [K.scale_problem(rng, nx, nz, scales, psf=psf) for _ in range(M)]
        R0 = np.stack([p[0] for p in parts])
        X = np.stack([p[1] for p in parts])[:n_psf]
        cx, cz = (X.shape[2] - 1) // 2, (X.shape[3] - 1) // 2
        n_s = len(scales)
        w = np.array([[1.0 / X[m if n_psf > 1 else 0, K.tri(k, k, n_s), cx, cz] for k in range(n_s)]
                      for m in range(M)])
        if nan:
            for m in range(M):
                R0[m].reshape(n_s, -1)[:, rng.choice(nx * nz, max(1, nx * nz // 60), replace=False)] = np.nan
                R0[m, n_s - 1, nx // 2, nz // 2] = np.inf
        for a in (R0, X, w):
            a.setflags(write=False)
        _PROBLEMS[key] = (R0, X, w)
    return _PROBLEMS[key]


@pytest.mark.parametrize("nx,nz,px,pz", [(5, 3, 9, 5), (67, 131, 133, 261), (67, 131, 31, 31)])
def test_one_scale_equals_rjp_clean_bit_for_bit(eng, nx, nz, px, pz):
    """n_s = 1, weight 1, a beam whose centre is exactly 1.0: s = |R| and f = gain R exactly, so every
    output -- the workspace included -- equals rjp_clean's, with full and windowed beams."""
    for i, (M, n_psf, masked, n_iter, gain, nan) in enumerate(((1, 1, False, 60, 0.1, False),
                                                               (3, 3, True, 37, 0.1, True),
                                                               (3, 1, False, 12, 1.0, False))):
        D, B = G.inputs(31 * nx + px + i, M, n_psf, nx, nz, px, pz, nan=nan, corners=i == 0)
        assert np.all(B[:, (px - 1) // 2, (pz - 1) // 2] == 1.0)
        mask = G.box(nx, nz) if masked else None
        top = np.array([np.abs(D[m][C.candidates(D[m], mask)]).max() for m in range(M)])
        thresh = 0.3 * top if i == 1 else 0.0
        a = G.run_clean(eng, D, B, mask, thresh, gain, n_iter)
        b = run_ms(eng, D[:, None], B[:, None], np.ones((M, 1)), mask, thresh, gain, n_iter)
        assert not b["cscale"][b["cpix"] != POISON_PIX].any()
        assert np.array_equal(b["cscale"] == POISON_PIX, b["cpix"] == POISON_PIX)
        for k in ("cpix", "cflux", "ncomp", "peak", "work"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert a["res"].tobytes() == b["res"].tobytes() and a["model"].tobytes() == b["model"].tobytes()


def test_one_pixel(eng):
    # one pixel, two planes: X_00 = 1, X_01 = 0.5, X_11 = 2, weights (1, 0.5), gain 0.5; exact in binary
    X = np.array([1.0, 0.5, 2.0]).reshape(1, 3, 1, 1)
    R0 = np.array([1.0, 4.0]).reshape(1, 2, 1, 1)
    out = run_ms(eng, R0, X, [1.0, 0.5], None, 0.0, 0.5, 2)
    # scores (1, 2): plane 1, f = 0.5 * 4 / 2 = 1 -> R = (0.5, 2); scores (0.5, 1): plane 1, f = 0.5
    assert list(out["cscale"][0]) == [1, 1] and list(out["cflux"][0]) == [1.0, 0.5] and list(out["cpix"][0]) == [0, 0]
    assert list(out["res"].ravel()) == [0.25, 1.0] and out["peak"][0] == 0.5 and out["ncomp"][0] == 2
    assert list(out["model"].ravel()) == [0.0, 1.5]
    follow_all("1 x 1", R0, X, [1.0, 0.5], None, 0.0, 0.5, 2, out)
    stop = run_ms(eng, R0, X, [1.0, 0.5], None, 0.5, 0.5, 5)                 # the third best score, 0.5, is not > 0.5
    assert stop["ncomp"][0] == 2 and stop["peak"][0] == 0.5 and np.all(stop["cpix"][0, 2:] == POISON_PIX)
    assert stop["res"].tobytes() == out["res"].tobytes()
    follow_all("1 x 1", R0, X, [1.0, 0.5], None, 0.5, 0.5, 5, stop)
    tie = run_ms(eng, R0, X, [1.0, 0.25], None, 0.0, 0.5, 1)                 # a tie: the lower scale
    assert tie["cscale"][0, 0] == 0 and tie["cflux"][0, 0] == 0.5
    follow_all("1 x 1", R0, X, [1.0, 0.25], None, 0.0, 0.5, 1, tie)
    # a zero X_kk(centre) under a weight > 0: finished from the start; under weight 0 it is never read
    X0 = X.copy()
    X0[0, 2] = 0.0
    dead = run_ms(eng, R0, X0, [1.0, 0.5], None, 0.0, 0.5, 3)
    assert dead["ncomp"][0] == 0 and dead["res"].tobytes() == R0.tobytes() and dead["peak"][0] == 0.0
    assert np.all(dead["cpix"] == POISON_PIX) and np.all(dead["model"] == 0)
    follow_all("1 x 1", R0, X0, [1.0, 0.5], None, 0.0, 0.5, 3, dead)
    live = run_ms(eng, R0, X0, [1.0, 0.0], None, 0.0, 0.5, 3)
    assert live["ncomp"][0] == 3 and not live["cscale"].any()
    follow_all("1 x 1", R0, X0, [1.0, 0.0], None, 0.0, 0.5, 3, live)


MS_CASES = [  # nx, nz, psf window (None = full)
    (5, 3, None), (67, 131, None), (67, 131, (31, 31)), (130, 65, (41, 25))]


@pytest.mark.parametrize("nx,nz,psf", MS_CASES)
def test_follow_the_device(eng, nx, nz, psf):
    """n_s of 2 and 3, 1 and 3 maps, shared and per-map beams, a box mask, a zero-weight plane, NaN and
    infinite pixels, thresholds of 0, mid-way and above the peak, d_peak NULL, a repeated call."""
    kind = "%d x %d%s" % (nx, nz, "" if psf is None else " window %d x %d" % psf)
    small = nx * nz < 100
    sc2, sc3 = ((0, 1.5), (0, 1.5, 2.0)) if small else ((0, 3.0), (0, 2.5, 4.0))
    combos = [  # scales, M, n_psf, mask, n_iter, gain, thresh, zero weight, nan
        (sc2, 1, 1, False, 60, 0.1, "zero", False, False),
        (sc3, 3, 3, True, 37, 0.2, "mid", False, False),
        (sc3, 3, 1, False, 37, 0.1, "zero", True, True),
        (sc2, 3, 3, False, 5, 1.0, "above", False, False),
    ]
    for i, (scales, M, n_psf, masked, n_iter, gain, th, zero_w, nan) in enumerate(combos):
        R0, X, w = problems(7000 + 10 * nx + i, M, n_psf, nx, nz, scales, psf, nan)
        n_s = len(scales)
        if zero_w:
            w = w.copy()
            w[:, 1] = 0.0
        mask = G.box(nx, nz) if masked else None
        top = np.array([(w[m][:, None, None] * np.abs(R0[m]))[K._cands(R0[m], w[m], mask)].max() for m in range(M)])
        thresh = {"zero": 0.0, "mid": 0.4 * top, "above": 1.5 * top}[th]
        out = run_ms(eng, R0, X, w, mask, thresh, gain, n_iter)
        follow_all(kind, R0, X, w, mask, thresh, gain, n_iter, out)
        if th == "above":
            assert np.all(out["ncomp"] == 0) and out["res"].tobytes() == R0.tobytes()
            assert np.all(out["model"] == 0) and np.array_equal(out["peak"], top)
        if th == "mid":
            # (a map may also run out of iterations: sources near the border of the zero-padded planes
            # converge slowly, which is why the imaging chain erodes its mask; `follow` holds every
            # map to the stopping rule either way)
            assert np.all(out["ncomp"] > 0) and np.all((out["ncomp"] == n_iter) | (out["peak"] <= thresh))
        if th == "zero" and not nan:
            assert np.all(out["ncomp"] == n_iter)
        if zero_w:
            live = out["cscale"][out["cscale"] != POISON_PIX]
            assert not (live == 1).any() and not np.array_equal(out["res"][:, 1], R0[:, 1])   # updated, never picked
        if i in (1, 2):
            same_bits(out, run_ms(eng, R0, X, w, mask, thresh, gain, n_iter))
    # the 16-byte path and the 8-byte one (a plane base 8 bytes off) give the same bits
    R0, X, w = problems(7000 + 10 * nx, 1, 1, nx, nz, sc2, psf, False)
    a = run_ms(eng, R0, X, w, None, 0.0, 0.1, 37, guard=GUARD)
    b = run_ms(eng, R0, X, w, None, 0.0, 0.1, 37, guard=GUARD + 1)
    for k in ("res", "cpix", "cscale", "cflux", "ncomp", "model", "peak"):
        assert a[k].tobytes() == b[k].tobytes(), k
    c = run_ms(eng, R0, X, w, None, 0.0, 0.1, 37, want_peak=False)
    follow_all(kind, R0, X, w, None, 0.0, 0.1, 37, c, want_peak=False)
    assert c["res"].tobytes() == a["res"].tobytes() and c["cflux"].tobytes() == a["cflux"].tobytes()


def test_more_partials_than_one_reduction_pass(eng):
    nx = nz = 600
    assert K.ms_workgroups(1, 2, nx, nz) == 704 > 2 * K.REDUCE_PASS
    rng = np.random.default_rng(600)
    from rajepy_amd.imaging import scale_kernel
    ker = [np.ones((1, 1)), scale_kernel(2.5)]
    big = C.random_beam(rng, 15 + 8, 15 + 8)
    one = [big, K.conv64(big, ker[1])]
    X = np.stack([K.conv64(one[k], ker[l])[4:19, 4:19] for k in range(2) for l in range(k, 2)])[None]
    # the strongest sources in tiles beyond the first pass of either plane, and in the last tile
    D = C.random_image(rng, nx, nz, big[4:19, 4:19],
                       sources=[(599, 599, 1.0), (450, 17, -0.9), (0, 0, 0.8), (300, 300, 0.7), (437, 0, 0.6)])
    R0 = np.stack([D, K.conv64(D, ker[1])])[None]
    w = np.array([[1.0 / X[0, 0, 7, 7], 0.9 / X[0, 2, 7, 7]]])
    out = run_ms(eng, R0, X, w, None, 0.0, 0.5, 12)
    assert out["ncomp"][0] == 12 and out["cpix"][0, 0] > K.REDUCE_PASS * K.TILE      # found beyond the first pass
    follow_all("600 x 600 x 2", R0, X, w, None, 0.0, 0.5, 12, out)


def test_all_zero_mask_touches_nothing(eng):
    R0, X, w = problems(5, 3, 1, 67, 131, (0, 2.5, 4.0), (31, 31))
    m0 = np.arange(R0.size, dtype=np.float64)
    out = run_ms(eng, R0, X, w, np.zeros((67, 131)), 0.0, 0.1, 37, model0=m0)
    assert np.all(out["ncomp"] == 0) and np.all(out["peak"] == 0.0)
    assert out["res"].tobytes() == R0.tobytes() and np.array_equal(out["model"].ravel(), m0)
    assert np.all(out["cpix"] == POISON_PIX) and np.all(out["cscale"] == POISON_PIX) and np.all(out["cflux"] == POISON_F)


def test_a_continued_call_equals_one_long_call(eng):
    R0, X, w = problems(9, 3, 3, 67, 131, (0, 2.5, 4.0), (31, 31))
    n1, n2, gain = 37, 63, 0.1
    first = run_ms(eng, R0, X, w, None, 0.0, gain, n1)
    assert np.all(first["ncomp"] == n1)
    second = run_ms(eng, first["res"], X, w, None, 0.0, gain, n2, model0=first["model"])
    long = run_ms(eng, R0, X, w, None, 0.0, gain, n1 + n2)
    joined = dict(second, ncomp=first["ncomp"] + second["ncomp"],
                  **{k: np.concatenate([first[k], second[k]], axis=1) for k in ("cpix", "cscale", "cflux")})
    follow_all("continued", R0, X, w, None, 0.0, gain, n1 + n2, joined)
    follow_all("continued", R0, X, w, None, 0.0, gain, n1 + n2, long)
    for k in ("cpix", "cscale", "cflux"):
        assert joined[k].tobytes() == long[k].tobytes(), k
    assert second["res"].tobytes() == long["res"].tobytes() and second["model"].tobytes() == long["model"].tobytes()


def test_engine_msclean(eng):
    import torch
    nx, nz = 67, 131
    R0, X, w = problems(21, 3, 1, nx, nz, (0, 2.5, 4.0), (31, 31))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(eng.device)
    res, model = dev(R0.reshape(3, 3, -1)), torch.zeros(3, 3, nx * nz, dtype=torch.float64, device=eng.device)
    mask = G.box(nx, nz)
    cpix, cscale, cflux, ncomp, peak = eng.msclean(res, 3, nx, nz, dev(X), 31, 31, w[0], 37, 0.1, 0.0, mask=mask,
                                                   model=model)
    assert eng.last_msclean_workgroups == 81
    assert cpix.shape == cscale.shape == (3, 37) and cscale.dtype == torch.int32 and ncomp.dtype == torch.int32
    raw = run_ms(eng, R0, X, w[0], mask, 0.0, 0.1, 37)
    for name, t in (("cpix", cpix), ("cscale", cscale), ("cflux", cflux), ("res", res), ("model", model), ("peak", peak)):
        assert t.cpu().numpy().tobytes() == raw[name].tobytes(), name
    for bad in (lambda: eng.msclean(res, 3, nx, nz, dev(X), 31, 31, w[0], 0, 0.1, 0.0),
                lambda: eng.msclean(res, 2, nx, nz, dev(X), 31, 31, w[0, :2], 5, 0.1, 0.0),
                lambda: eng.msclean(res, 3, nx, nz, dev(X[:, :5]), 31, 31, w[0], 5, 0.1, 0.0),
                lambda: eng.msclean(res, 3, nx, nz, dev(X), 31, 31, w[0, :2], 5, 0.1, 0.0),
                lambda: eng.msclean(res, 3, nx, nz, dev(X), 31, 31, w[0], 5, 0.1, [0.0, 0.0]),
                lambda: eng.msclean(res, 3, nx, nz, dev(X), 31, 31, w[0], 5, 0.1, 0.0, mask=np.ones(5))):
        with pytest.raises(ValueError):
            bad()


# ---- 3: refusals --------------------------------------------------------------------------------------
def test_refusals_leave_poisoned_outputs_untouched(eng):
    import torch
    from rajepy_amd import _lib
    M, n_s, nx, nz, px, pz, n_iter = 2, 2, 5, 3, 9, 5, 4
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    full = lambda n, v, dt: torch.full((n,), v, dtype=dt, device=eng.device)
    wb = eng.lib.rjp_msclean_workspace(M, n_s, nx, nz)
    bufs = dict(res=full(M * n_s * nx * nz, 7.0, f64), psf=full(M * 3 * px * pz, 0.5, f64),
                mask=full(nx * nz, 1, u8), cpix=full(M * n_iter, POISON_PIX, i32),
                cscale=full(M * n_iter, POISON_PIX, i32), cflux=full(M * n_iter, POISON_F, f64),
                ncomp=full(M, POISON_PIX, i32), model=full(M * n_s * nx * nz, 3.0, f64),
                peak=full(M, POISON_F, f64), work=full(wb, 0xA5, u8), out=full(M * nx * nz, 7.0, f64),
                ker=full(M * 3 * 5, 0.25, f64))
    before = {k: t.clone() for k, t in bufs.items()}
    good = dict(bufs, n_maps=M, n_s=n_s, nx=nx, nz=nz, n_psf=M, px=px, pz=pz, weight=[1.0, 0.5, 0.0, 2.0],
                thresh=[0.0, 0.1], gain=0.1, n_iter=n_iter, nbytes=wb, ctx=True)
    ptr = lambda t: t.data_ptr() if t is not None else None
    arr = lambda v: _lib.dbl_array(v) if v is not None else None

    def ms(a):
        return eng.lib.rjp_msclean(eng.ctx if a["ctx"] else None, ptr(a["res"]), a["n_maps"], a["n_s"], a["nx"],
                                   a["nz"], ptr(a["psf"]), a["n_psf"], a["px"], a["pz"], arr(a["weight"]),
                                   ptr(a["mask"]), arr(a["thresh"]), a["gain"], a["n_iter"], ptr(a["cpix"]),
                                   ptr(a["cscale"]), ptr(a["cflux"]), ptr(a["ncomp"]), ptr(a["model"]),
                                   ptr(a["peak"]), ptr(a["work"]), a["nbytes"], eng._stream())

    ARG, WS = _lib.RJP_ERR_ARG, _lib.RJP_ERR_WORKSPACE
    big = 2 ** 31 - 1
    T = K.MSG
    cases = [("NULL d_res", dict(res=None), ARG, "null"), ("NULL d_xpsf", dict(psf=None), ARG, "null"),
             ("NULL h_weight", dict(weight=None), ARG, "null"), ("NULL h_thresh", dict(thresh=None), ARG, "null"),
             ("NULL d_cpix", dict(cpix=None), ARG, "null"), ("NULL d_cscale", dict(cscale=None), ARG, "null"),
             ("NULL d_cflux", dict(cflux=None), ARG, "null"), ("NULL d_ncomp", dict(ncomp=None), ARG, "null"),
             ("n_maps = 0", dict(n_maps=0), ARG, "sizes"), ("n_s = 0", dict(n_s=0), ARG, "sizes"),
             ("n_s < 0", dict(n_s=-2), ARG, "sizes"), ("nx < 0", dict(nx=-1), ARG, "sizes"),
             ("nz = 0", dict(nz=0), ARG, "sizes"), ("px = 0", dict(px=0), ARG, "sizes"),
             ("pz < 0", dict(pz=-5), ARG, "sizes"),
             ("even px", dict(px=8), ARG, "even"), ("even pz", dict(pz=4), ARG, "even"),
             ("n_psf = 0", dict(n_psf=0), ARG, "npsf"), ("n_psf = 3", dict(n_psf=3), ARG, "npsf"),
             ("too many pixels", dict(nx=big, nz=big), ARG, "npix"),
             ("gain = 0", dict(gain=0.0), ARG, "gain"), ("gain > 1", dict(gain=1.0000001), ARG, "gain"),
             ("NaN gain", dict(gain=np.nan), ARG, "gain"),
             ("n_iter = 0", dict(n_iter=0), ARG, "niter"),
             ("negative threshold", dict(thresh=[0.0, -1e-9]), ARG, "thresh"),
             ("NaN threshold", dict(thresh=[np.nan, 0.0]), ARG, "thresh"),
             ("negative weight", dict(weight=[1.0, 0.5, -0.0001, 2.0]), ARG, "weight"),
             ("NaN weight", dict(weight=[np.nan, 0.5, 0.0, 2.0]), ARG, "weight"),
             ("infinite weight", dict(weight=[1.0, 0.5, 0.0, np.inf]), ARG, "weight"),
             ("too many workgroups", dict(n_s=600, nx=46340, nz=46340, weight=[1.0] * 1200), ARG, "wgs"),
             ("a short workspace", dict(nbytes=wb - 1), WS, "work"),
             ("no workspace", dict(work=None), WS, "work")]
    for what, kw, want, key in cases:
        assert ms(dict(good, **kw)) == want, what
        assert eng.lib.rjp_last_error(eng.ctx).decode() == T[key], what
    assert ms(dict(good, ctx=False)) == ARG
    assert eng.lib.rjp_last_error(None).decode() == "null context"

    def conv(**kw):
        a = dict(inp=bufs["res"], n_maps=M, nx=nx, nz=nz, ker=bufs["ker"], n_ker=M, kx=3, kz=5, add=bufs["model"],
                 out=bufs["out"], ctx=True)
        a.update(kw)
        return eng.lib.rjp_convolve2d(eng.ctx if a["ctx"] else None, ptr(a["inp"]), a["n_maps"], a["nx"], a["nz"],
                                      ptr(a["ker"]), a["n_ker"], a["kx"], a["kz"], ptr(a["add"]), ptr(a["out"]),
                                      eng._stream())

    ccases = [("NULL d_in", dict(inp=None), "conv_null"), ("NULL d_ker", dict(ker=None), "conv_null"),
              ("NULL d_out", dict(out=None), "conv_null"),
              ("n_maps = 0", dict(n_maps=0), "conv_sizes"), ("nx = 0", dict(nx=0), "conv_sizes"),
              ("nz < 0", dict(nz=-1), "conv_sizes"), ("kx = 0", dict(kx=0), "conv_sizes"),
              ("kz < 0", dict(kz=-5), "conv_sizes"),
              ("even kx", dict(kx=4), "conv_even"), ("even kz", dict(kz=2), "conv_even"),
              ("kx = 257", dict(kx=257), "conv_max"), ("kz = 257", dict(kz=257), "conv_max"),
              ("n_ker = 0", dict(n_ker=0), "conv_nker"), ("n_ker = 3", dict(n_ker=3), "conv_nker"),
              ("too many pixels", dict(nx=46341, nz=46341), "conv_npix"),
              ("too many workgroups", dict(nx=46340, nz=46340, n_maps=2000, n_ker=1), "conv_wgs")]
    for what, kw, key in ccases:
        assert conv(**kw) == ARG, what
        assert eng.lib.rjp_last_error(eng.ctx).decode() == T[key], what
    assert conv(ctx=False) == ARG
    eng.synchronize()
    for k, t in bufs.items():
        assert torch.equal(t, before[k]), k + " was touched by a refusal"
    # the context still serves a valid call of each; NULL mask, model, peak and add are no refusals
    assert ms(dict(good, mask=None, model=None, peak=None)) == K.ms_workgroups(M, n_s, nx, nz) == 4
    eng.synchronize()
    assert not bool((bufs["ncomp"] == POISON_PIX).any()) and torch.equal(bufs["model"], before["model"])
    assert conv(add=None) == 2
    eng.synchronize()
    assert not bool((bufs["out"] == 7.0).any())


# ---- 4: the golden example model through JetModel ------------------------------------------------------
def _params(tag):
    p = copy.deepcopy(U.load_golden(tag)[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


SHAPE = (41, 45)
PSF = (31, 31)


@pytest.fixture(scope="module")
def example(eng, tmp_path_factory):
    from rajepy_amd import classes, logger
    log = logger.Log(str(tmp_path_factory.mktemp("msclean") / "cfg1.log"), verbose=False)
    jm = classes.JetModel(_params("cfg1_example"), log=log, engine=eng)
    jm.time = 1.0 * YEAR
    freqs = np.asarray(U.load_golden("cfg1_example")[0]["freqs"], dtype=np.float64)[:2]
    u, v, w = G.baselines(jm, freqs)
    return jm, freqs, u, v, w


def test_clean_image_ff_with_scales_on_the_example_model(eng, example, monkeypatch):
    """clean_image_ff(scales=[0, 4, 10]): the reference follows the components on the planes and cross
    beams the device was handed (recorded at the call); those are themselves held to the long-double
    convolution of the dirty image; the model's total flux equals the sum of the component fluxes."""
    from rajepy_amd.imaging import scale_kernel
    jm, freqs, u, v, w = example
    seen = {}
    real = eng.msclean

    def spy(res, n_s, nx, nz, xpsf, px, pz, weight, n_iter, gain, thresh, mask=None, model=None):
        seen.update(R0=res.cpu().numpy().copy(), X=xpsf.cpu().numpy().copy(), w=np.array(weight), n_s=n_s,
                    mask=mask.cpu().numpy().copy(), shape=(nx, nz, px, pz), thresh=thresh)
        return real(res, n_s, nx, nz, xpsf, px, pz, weight, n_iter, gain, thresh, mask=mask, model=model)

    monkeypatch.setattr(eng, "msclean", spy)
    D = jm.dirty_image_ff(u, v, freqs, weights=w, shape=SHAPE)
    thresh = 0.01 * float(np.abs(D).max())
    niter, gain = 80, 0.2
    res = jm.clean_image_ff(u, v, freqs, weights=w, shape=SHAPE, niter=niter, gain=gain, threshold_jy=thresh,
                            psf_shape=PSF, scales=[10, 0, 4])
    M, (ni, nj) = 2, SHAPE
    assert seen["n_s"] == 3 and seen["shape"] == (ni, nj) + PSF and seen["w"].shape == (M, 3)
    R0 = seen["R0"].reshape(M, 3, ni, nj)
    X = seen["X"].reshape(M, 6, *PSF)
    mask = seen["mask"].reshape(ni, nj) != 0
    want = np.zeros(SHAPE, dtype=bool)
    want[9:ni - 9, 9:nj - 9] = True
    assert np.array_equal(mask, want)
    kers = [scale_kernel(s) for s in (0, 4, 10)]
    scales = np.array([0.0, 4.0, 10.0])
    bias = np.array([1.0, 0.76, 0.4])
    assert R0[:, 0].tobytes() == D.tobytes()
    for m in range(M):
        for l in (1, 2):
            note("planes", K.check_conv(R0[m, l], D[m], kers[l]))
        xkk = np.array([X[m, K.tri(k, k, 3), 15, 15] for k in range(3)])
        assert np.allclose(seen["w"][m], bias / xkk, rtol=1e-15)
        comp = res.components[m]
        n = len(comp)
        assert comp.shape == (n, 4) and n > 0 and set(comp[:, 3]) <= set(scales)
        cpix = (comp[:, 0] * nj + comp[:, 1]).astype(np.int64)
        cscale = np.searchsorted(scales, comp[:, 3])
        rows = lambda a, fill: np.concatenate([a, np.full(niter - n, fill)])
        planes = None
        # (only the raw plane comes back: the follow rule runs on it and on the list; the other planes'
        # ends are rebuilt by the identity R_l = R0_l - sum f X, which `follow` checks against `res`)
        S = R0[m].astype(LD).copy()
        for c in range(n):
            im, bm = C.window(ni, nj, PSF[0], PSF[1], int(cpix[c]) // nj, int(cpix[c]) % nj)
            for l in range(3):
                S[l][im] -= LD(comp[c, 2]) * X[m, K.tri(int(cscale[c]), l, 3)].astype(LD)[bm]
        planes = S.astype(np.float64)
        planes[0] = res.residual[m]
        note("clean_image_ff(scales)", K.follow(R0[m], X[m], seen["w"][m], mask, thresh, gain, niter,
                                                rows(cpix, POISON_PIX), rows(cscale, POISON_PIX),
                                                rows(comp[:, 2], POISON_F), n, planes))
        assert res.peak_residual[m] == np.abs(res.residual[m][mask]).max()
        # unit-sum kernels, components at least h_max inside: the model's flux is the components'
        tol = (2 * 19 * 19 + 2) * K.U * float(np.abs(comp[:, 2]).sum())
        assert abs(float(res.model[m].astype(LD).sum() - comp[:, 2].astype(LD).sum())) <= tol
        assert np.all((comp[:, 0] >= 9) & (comp[:, 0] < ni - 9) & (comp[:, 1] >= 9) & (comp[:, 1] < nj - 9))
    assert len({s for c in res.components for s in c[:, 3]}) > 1           # more than one scale is used
    assert res.image.shape == res.model.shape == res.residual.shape == (M,) + SHAPE


def test_without_scales_the_result_is_todays(eng, example):
    """scales=None: the CleanResult equals, bit for bit, K11 + K12 + K13 composed by hand as
    `_clean_images` composed them before it knew of scales."""
    import torch
    from rajepy_amd import engine as E
    jm, freqs, u, v, w = example
    shape, niter = (15, 21), 40
    res = jm.clean_image_ff(u, v, freqs, weights=w, shape=shape, niter=niter, threshold_jy=1e-6, beam=(0.3, 0.2, 10.))
    im, V, u_d, v_d, fr = jm._model_vis(u, v, freqs, None)
    dirty = im._dirty_images(V, u_d, v_d, fr, w, shape, None, False, device=True)
    psf = im._dirty_images(im._unit_vis(2, int(V.shape[1])), u_d, v_d, fr, w, (29, 41), None, False, device=True)
    model = torch.zeros_like(dirty)
    cpix, cflux, ncomp, peak = eng.clean(dirty, 15, 21, psf, 29, 41, niter, 0.1, 1e-6, model=model)
    cell = im._image_grid(shape, None)[2]
    image = eng.restore(cpix, cflux, ncomp, [E.beam_quadratic(0.3, 0.2, 10., cell)] * 2, 15, 21, add=dirty)
    assert res.image.tobytes() == image.cpu().numpy().tobytes()
    assert res.residual.tobytes() == dirty.cpu().numpy().tobytes()
    assert res.model.tobytes() == model.cpu().numpy().tobytes()
    assert res.peak_residual.tobytes() == peak.cpu().numpy().tobytes()
    hp, hf, hn = cpix.cpu().numpy(), cflux.cpu().numpy(), ncomp.cpu().numpy()
    for m in range(2):
        n = int(hn[m])
        assert res.components[m].shape == (n, 3)
        assert np.array_equal(res.components[m], np.stack([hp[m, :n] // 21, hp[m, :n] % 21, hf[m, :n]], axis=1))
