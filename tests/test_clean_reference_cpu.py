"""Pins tests/clean_ref.py -- the long-double Hogbom CLEAN and the follow-the-device checker that
tests/test_gpu_clean.py holds rjp_clean (K12) and rjp_restore (K13) to -- before anything runs on a
GPU: the reference against hand-worked cases; the checker against a float64 emulation (inside the
bound) and four planted mistakes (outside); the host code (`beam_quadratic`, `fit_beam`, the
Python argument paths), the ABI, the workspace query and the tile rule as host arithmetic."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import clean_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def delta_beam(px, pz):
    b = np.zeros((px, pz))
    b[(px - 1) // 2, (pz - 1) // 2] = 1.0
    return b


# ---- the reference against hand-worked cases ------------------------------------------------------
def test_one_point_source_gain_one_full_beam():
    rng = np.random.default_rng(1)
    nx, nz = 5, 7
    B = K.random_beam(rng, 2 * nx - 1, 2 * nz - 1)
    D = K.random_image(rng, nx, nz, B, noise=0.0, sources=[(3, 2, 0.5)])      # a power of two: D = S B exactly
    cpix, cflux, R = K.hogbom(D, B, None, 0.0, 1.0, 1)
    assert list(cpix) == [3 * nz + 2] and float(cflux[0]) == 0.5
    assert np.abs(R).max() == 0


def test_two_pixels_by_hand():
    # D = (1, 0.5), beam (0.5, 1, 0.5), gain 0.5: picks 0 (f = 0.5) -> R = (0.5, 0.25);
    # 0 again (f = 0.25) -> (0.25, 0.125); all exact in binary
    D = np.array([[1.0, 0.5]])
    B = np.array([[0.5, 1.0, 0.5]])
    cpix, cflux, R = K.hogbom(D, B, None, 0.0, 0.5, 2)
    assert list(cpix) == [0, 0] and [float(f) for f in cflux] == [0.5, 0.25]
    assert np.array_equal(R.astype(float), [[0.25, 0.125]])
    # a negative peak is a peak: gain 1 on (-1, 0.5) with the same beam -> f = -1, R = (0, 1)
    cpix, cflux, R = K.hogbom(np.array([[-1.0, 0.5]]), B, None, 0.0, 1.0, 1)
    assert list(cpix) == [0] and float(cflux[0]) == -1.0 and np.array_equal(R.astype(float), [[0.0, 1.0]])


def test_threshold_stops_midway_and_mask_excludes_the_peak():
    D = np.array([[1.0, 0.5]])
    B = np.array([[0.5, 1.0, 0.5]])
    cpix, cflux, R = K.hogbom(D, B, None, 0.3, 0.5, 10)      # peaks 1, 0.5, 0.25 <= 0.3: two picks
    assert len(cpix) == 2 and float(np.abs(R).max()) == 0.25
    cpix, _, _ = K.hogbom(D, B, None, 0.5, 0.5, 10)           # |R| <= thresh stops: 0.5 is not > 0.5
    assert len(cpix) == 1
    cpix, cflux, R = K.hogbom(D, B, np.array([[0, 1]]), 0.0, 1.0, 1)
    assert list(cpix) == [1] and float(cflux[0]) == 0.5 and np.array_equal(R.astype(float), [[0.75, 0.0]])
    assert len(K.hogbom(D, B, np.zeros((1, 2)), 0.0, 1.0, 5)[0]) == 0


def test_corner_component_clips_the_window():
    B = np.arange(1.0, 10.0).reshape(3, 3) / 5.0
    B[1, 1] = 1.0
    D = np.zeros((3, 4))
    D[2, 3] = 2.0
    cpix, cflux, R = K.hogbom(D, B, None, 0.0, 0.5, 1)
    assert list(cpix) == [11] and float(cflux[0]) == 1.0
    want = D.copy()
    want[1:3, 2:4] -= B[0:2, 0:2]                # only the beam's upper left quarter lies inside
    assert np.array_equal(R.astype(float), want)
    im, bm = K.window(3, 4, 3, 3, 0, 0)
    assert im == (slice(0, 2), slice(0, 2)) and bm == (slice(1, 3), slice(1, 3))


# ---- the checks themselves -----------------------------------------------------------------------
CASES = [(33, 47, 0.1), (33, 47, 1.0), (65, 130, 0.1)]


def make(nx, nz, seed, psf=None):
    rng = np.random.default_rng(seed)
    full = K.random_beam(rng, 2 * nx - 1, 2 * nz - 1)
    D = K.random_image(rng, nx, nz, full)
    if psf is None:
        return D, full
    cx, cz = nx - 1, nz - 1
    hx, hz = psf[0] // 2, psf[1] // 2
    return D, np.ascontiguousarray(full[cx - hx:cx + hx + 1, cz - hz:cz + hz + 1])


def run_follow(D, B, mask, thresh, gain, n_iter, **switches):
    cpix, cflux, R = K.hogbom(D, B, mask, thresh, gain, n_iter, dtype=np.float64, **switches)
    n = len(cpix)
    full_p = np.full(n_iter, -7, dtype=np.int64)
    full_f = np.full(n_iter, np.nan)
    full_p[:n], full_f[:n] = cpix, cflux
    model = np.zeros(D.size)
    for p, f in zip(cpix, cflux):
        model[p] += f
    ok = K.candidates(R, mask)
    peak = float(np.abs(R[ok]).max()) if ok.any() else 0.0
    return K.follow(D, B, mask, thresh, gain, n_iter, full_p, full_f, n, R, peak=peak, model=model,
                    poison_pix=-7, poison_flux=np.nan, roundings=2), (full_p, full_f, n, R)


@pytest.mark.parametrize("nx,nz,gain", CASES)
def test_float64_emulation_passes_inside_the_bound(nx, nz, gain):
    D, B = make(nx, nz, 100 * nx + nz)
    n_iter = 120
    worst, (cp, cf, n, R) = run_follow(D, B, None, 0.0, gain, n_iter)
    assert n == n_iter and worst < 1.0
    assert K.conservation(D, B, cp, cf, n, R, roundings=2) <= 1.0
    # the long-double reference picks the same pixels on these inputs (near-ties have measure 0)
    rp, _, RL = K.hogbom(D, B, None, 0.0, gain, n_iter)
    assert np.array_equal(rp, cp[:n]) and float(np.abs(RL - R).max()) < 1e-14
    # a box mask, a mid-way threshold, a windowed beam
    mask = np.zeros(D.shape, dtype=bool)
    mask[nx // 4:nx, 0:nz // 2] = True
    w2, (_, _, n2, _) = run_follow(D, B, mask, 0.5 * np.abs(D[mask]).max(), gain, n_iter)
    assert w2 < 1.0 and n2 < n_iter
    D3, B3 = make(nx, nz, 100 * nx + nz, psf=(31, 31))
    assert run_follow(D3, B3, None, 0.0, gain, 60)[0] < 1.0
    print("%d x %d gain %g: worst error / bound %.3f (full), %.3f (mask + threshold)" % (nx, nz, gain, worst, w2))


def test_four_planted_mistakes_fall_outside():
    nx, nz = 33, 47
    D, B = make(nx, nz, 4242)
    with pytest.raises(AssertionError):          # a beam centre of n / 2 rounded up, not (n - 1) / 2
        run_follow(D, B, None, 0.0, 0.1, 20, centre=(B.shape[0] // 2 + 1, B.shape[1] // 2 + 1))
    with pytest.raises(AssertionError, match="flux"):          # a forgotten gain
        run_follow(D, B, None, 0.0, 0.1, 20, use_gain=False)
    Dn = -D                                      # the strongest pixel negative: arg-max of R misses it
    with pytest.raises(AssertionError, match="not a maximum"):
        run_follow(Dn if Dn.ravel()[np.abs(Dn).argmax()] < 0 else D, B, None, 0.0, 0.1, 20, use_abs=False)
    T = np.zeros((4, 5))
    T[0, 3] = T[2, 1] = 1.0                      # an exact tie
    with pytest.raises(AssertionError, match="lowest index"):
        run_follow(T, delta_beam(7, 9), None, 0.0, 0.5, 1, tie_low=False)


def test_follow_rule_holds_on_an_exact_tie():
    T = np.zeros((4, 5))
    T[0, 3] = T[2, 1] = 1.0
    T[3, 4] = -1.0
    for B in (delta_beam(7, 9), K.random_beam(np.random.default_rng(3), 7, 9)):
        worst, (cp, cf, n, R) = run_follow(T, B, None, 0.0, 0.5, 12)
        assert n == 12 and cp[0] == 3 and worst <= 1.0


# ---- host code ---------------------------------------------------------------------------------------
def test_beam_quadratic_by_hand():
    from rajepy_amd import engine as E
    cell = np.radians(0.1 / 3600.)               # 0.1 arcsec cells
    k = 4 * np.log(2.)
    A, B, Cq = E.beam_quadratic(1.0, 0.5, 0.0, cell)        # bpa = 0: the major axis lies along z
    assert np.allclose([A, B, Cq], [k / 25., 0.0, k / 100.], rtol=1e-13, atol=1e-18)
    A, B, Cq = E.beam_quadratic(1.0, 0.5, 90.0, cell)       # towards East: along x
    assert np.allclose([A, Cq], [k / 100., k / 25.], rtol=1e-13) and abs(B) < 1e-17
    # bpa = 45 deg: the major axis points to (dx, dz) = (-1, 1) / sqrt 2 (East is decreasing ix)
    A, B, Cq = E.beam_quadratic(1.0, 0.5, 45.0, cell)
    q = lambda dx, dz: A * dx * dx + 2 * B * dx * dz + Cq * dz * dz
    assert np.isclose(q(-1, 1), 2 * k / 100., rtol=1e-13) and np.isclose(q(1, 1), 2 * k / 25., rtol=1e-13)
    assert np.isclose(np.exp(-q(-5 / np.sqrt(2), 5 / np.sqrt(2))), 0.5, rtol=1e-13)   # half at FWHM / 2
    for beam in ((1.0, 0.5, 0.0), (0.8, 0.3, 37.0), (0.8, 0.3, -80.0), (2.0, 1.9, 90.0)):
        assert np.allclose(E.beam_from_quadratic(*E.beam_quadratic(*beam, cell), cell), beam, rtol=1e-9)


def test_fit_beam_recovers_an_exact_gaussian():
    from rajepy_amd import engine as E
    for abc in ((0.05, 0.0, 0.02), (0.03, 0.012, 0.04), (0.2, -0.1, 0.11)):
        d = np.arange(-16, 17, dtype=float)
        dx, dz = d[:, None], d[None, :]
        patch = np.exp(-(abc[0] * dx * dx + 2 * abc[1] * dx * dz + abc[2] * dz * dz))
        assert np.allclose(E.fit_beam(patch), abc, rtol=1e-9, atol=1e-12)
        assert np.allclose(E.fit_beam(3.0 * patch), abc, rtol=1e-9, atol=1e-12)   # the scale drops out
        far = patch.copy()
        far[0, 0] = far[32, 32] = 0.9            # a far sidelobe above half is not the main lobe
        assert np.allclose(E.fit_beam(far), abc, rtol=1e-9, atol=1e-12)
    with pytest.raises(ValueError, match="too few"):
        E.fit_beam(delta_beam(9, 9))
    with pytest.raises(ValueError, match="odd"):
        E.fit_beam(np.ones((4, 5)))


def test_restore_reference_against_plain_numpy():
    nx, nz = 9, 11
    abc = (0.3, 0.1, 0.2)
    cpix, cflux = np.array([0, 5 * nz + 4, nx * nz - 1]), np.array([1.0, -0.5, 2.0])
    out, bound = K.restore_ref(cpix, cflux, 3, abc, nx, nz)
    want = np.zeros((nx, nz))
    for p, f in zip(cpix, cflux):
        for ix in range(nx):
            for iz in range(nz):
                dx, dz = ix - p // nz, iz - p % nz
                want[ix, iz] += f * np.exp(-(abc[0] * dx * dx + 2 * abc[1] * dx * dz + abc[2] * dz * dz))
    assert np.allclose(out.astype(float), want, rtol=1e-13, atol=1e-16)
    assert np.all(bound < 1e-12 * 3.5) and np.all(bound >= 0)
    add = np.arange(nx * nz, dtype=float)
    assert np.allclose((K.restore_ref(cpix, cflux, 3, abc, nx, nz, add)[0] - out).astype(float).ravel(), add)
    assert np.all(K.restore_ref(cpix, cflux, 0, abc, nx, nz)[0] == 0)
    # a beam so narrow that the neighbours underflow: the component's own pixel and nothing else
    out, _ = K.restore_ref(cpix, cflux, 3, (800.0, 0.0, 800.0), nx, nz)
    assert np.count_nonzero(out) == 3 and float(out[5, 4]) == -0.5


# ---- the ABI, the workspace, the tile rule ----------------------------------------------------------
def test_header_symbols_and_argtypes():
    from rajepy_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    assert int(re.search(r"#define RJP_VERSION (\d+)", hdr).group(1)) == _lib.RJP_VERSION == 117
    assert "size_t rjp_clean_workspace(int32_t n_maps, int32_t nx, int32_t nz);" in hdr
    decl = re.search(r"int64_t rjp_clean\((.*?)\);", hdr, re.S).group(1)
    names = [re.search(r"(\w+)$", p.strip()).group(1) for p in decl.split(",")]
    assert names == ["ctx", "d_res", "n_maps", "nx", "nz", "d_psf", "n_psf", "px", "pz", "d_mask",
                     "h_thresh", "gain", "n_iter", "d_cpix", "d_cflux", "d_ncomp", "d_model",
                     "d_peak", "d_work", "work_bytes", "stream"]
    decl = re.search(r"int64_t rjp_restore\((.*?)\);", hdr, re.S).group(1)
    names = [re.search(r"(\w+)$", p.strip()).group(1) for p in decl.split(",")]
    assert names == ["ctx", "d_cpix", "d_cflux", "d_ncomp", "n_maps", "comp_stride", "h_beam",
                     "d_add", "nx", "nz", "d_out", "stream"]
    i32, dp, vp = C.c_int32, C.POINTER(C.c_double), C.c_void_p
    assert _lib.SIGNATURES["rjp_clean_workspace"] == (C.c_size_t, [i32] * 3)
    res, args = _lib.SIGNATURES["rjp_clean"]
    assert res is C.c_int64
    assert args == [vp, vp, i32, i32, i32, vp, i32, i32, i32, vp, dp, C.c_double, i32, vp, vp, vp,
                    vp, vp, vp, C.c_size_t, vp]
    res, args = _lib.SIGNATURES["rjp_restore"]
    assert res is C.c_int64 and args == [vp, vp, vp, vp, i32, i32, dp, vp, i32, i32, vp, vp]
    lib = _lib.load()
    for name in ("rjp_clean_workspace", "rjp_clean", "rjp_restore"):
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert set(re.findall(r"typedef struct (rjp_\w+) \{", hdr)) == {"rjp_fields", "rjp_bursts",
                                                                    "rjp_line", "rjp_geometry"}
    mk = open(os.path.join(ROOT, "rajepy_amd", "csrc", "Makefile")).read()
    assert "$(OBJDIR)/clean.o" in mk


def test_tile_rule_and_workspace_query():
    from rajepy_amd import _lib
    t = K.tiling
    assert t(1, 1, 1) == dict(tiles=1, workgroups=1)
    assert t(1, 32, 32) == dict(tiles=1, workgroups=1) and t(1, 32, 33)["tiles"] == 2
    assert t(3, 67, 131) == dict(tiles=9, workgroups=27)
    assert t(1, 501, 501) == dict(tiles=246, workgroups=246)          # the reference's imaging case
    assert t(64, 256, 256) == dict(tiles=64, workgroups=4096)         # a cube
    assert t(1, 600, 600)["tiles"] == 352 > K.REDUCE_PASS             # two passes of the reduction
    ws = _lib.load().rjp_clean_workspace
    for args in ((1, 1, 1), (1, 5, 3), (3, 67, 131), (1, 501, 501), (64, 256, 256), (1, 600, 600),
                 (7, 130, 65)):
        assert ws(*args) == K.workspace_bytes(*args) > 0 and ws(*args) % 16 == 0, args
    assert ws(1, 1, 1) == 32 and ws(3, 67, 131) == 27 * 24 + 8       # rounded up to 16
    for i in range(3):
        for bad in (0, -1):
            a = [3, 67, 131]
            a[i] = bad
            assert ws(*a) == 0
    assert ws(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) % 16 == 0


def test_python_argument_paths():
    """What RTEngine.clean / restore and Imager._clean_mask refuse before any device call."""
    from rajepy_amd import classes, imaging
    m = imaging.Imager._clean_mask
    assert m(None, None, 4, 5) is None
    box = m(None, (1, 2, 0, 3), 4, 5)
    assert box.shape == (4, 5) and box.sum() == 8 and box[1:3, 0:4].all()
    arr = m(None, np.eye(4, 5), 4, 5)
    assert arr.dtype == bool and arr.sum() == 4
    for bad in ((2, 1, 0, 3), (0, 4, 0, 3), (0, 1, -1, 3), np.ones((5, 4))):
        with pytest.raises(ValueError):
            m(None, bad, 4, 5)
    assert classes.CleanResult._fields == ("image", "residual", "model", "components", "beam",
                                           "peak_residual")
    import inspect
    sig = inspect.signature(classes.JetModel.clean_image_ff)
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["niter"], d["gain"], d["threshold_jy"]) == (500, 0.1, 0.0)         # tclean's
    assert d["mask"] is None and d["beam"] is None and d["psf_shape"] is None and d["mfs"] is False
    rr = inspect.signature(classes.JetModel.clean_image_rrl).parameters
    assert set(sig.parameters) - {"self"} <= set(rr) and "rrl" in rr and "contsub" in rr
    assert "device" in inspect.signature(imaging.Imager._dirty_images).parameters
