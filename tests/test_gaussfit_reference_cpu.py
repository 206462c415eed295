"""tests/gaussfit_ref.py -- the reference that follows rjp_gaussfit's trace on the GPU
(tests/test_gpu_gaussfit.py) -- pinned on the CPU first: hand-worked cases, the Jacobian against
Richardson-extrapolated central differences, a float64 NumPy emulation of the device's arithmetic
(inside the bounds), planted mistakes (outside), then the host helpers (`gauss_results`,
`gauss_start`), the ABI and check_gaussfit from a plain C++ program."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from rajepy_amd import _lib
from rajepy_amd import engine as E
from tests import gaussfit_ref as K

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -7.5
LAM0, XTOL = 1e-3, 1e-12


def gauss(nx, nz, th, dtype=np.float64):
    ix, iz = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    return K.model(th, ix.ravel(), iz.ravel(), dtype, with_jac=False)[0].reshape(nx, nz)


def whole(nx, nz):
    return (0, nx - 1, 0, nz - 1)


def peak_start(img, abc):
    p = np.unravel_index(np.argmax(np.abs(img)), img.shape)
    return np.array([img[p], p[0], p[1], *abc])


def noisy_case(seed=11, level=0.01, nx=67, nz=131):
    truth = np.array([1.3, 33.3, 64.8, 0.0049, 0.0015, 0.0021])
    rng = np.random.default_rng(seed)
    img = gauss(nx, nz, truth) + level * rng.standard_normal((nx, nz))
    return img, peak_start(img, (0.003, 0.0, 0.003)), truth


# ---- hand-worked -----------------------------------------------------------------------------------
def test_a_start_at_the_fixed_point_stops_after_one_trial():
    """A Gaussian sampled exactly: one pixel of 1.5 and a form so narrow that every other pixel's
    exponent (-800) lies below -700, an exact 0.  chi^2 = 0 at the start: accepted, status 1."""
    img = np.zeros((5, 3))
    img[2, 1] = 1.5
    th0 = [1.5, 2.0, 1.0, 800.0, 0.0, 800.0]
    out = K.emulate(img, whole(5, 3), None, th0, LAM0, XTOL, 7, poison=POISON)
    assert out["status"] == 1 and out["niter"] == 1 and out["chi2"] == 0.0 and out["npix"] == 15
    assert np.array_equal(out["theta"], th0)
    assert np.array_equal(out["trace"][0], [0.0, LAM0, 1.0] + th0) and np.all(out["trace"][1:] == POISON)
    # N by hand: only the centre pixel has a non-zero Jacobian, (1, 0, 0, 0, 0, 0)
    assert np.array_equal(out["cov"], [1.0] + [0.0] * 20)
    assert K.follow(img, whole(5, 3), None, th0, LAM0, XTOL, 7, out, POISON) == 0.0


def test_two_pixels_by_hand():
    """A 1 x 2 image (0.5, 2), S = 2, centre on pixel 1, A = C = ln 2: G = (1, 2), r = (-0.5, 0);
    the Jacobian of pixel 0 (dx = 0, dz = -1): (0.5, 0, 2 C dz G, 0, 0, -G dz^2) =
    (0.5, 0, -2 ln 2, 0, 0, -1); of pixel 1: (1, 0, 0, 0, 0, 0)."""
    ln2 = np.log(LD(2))
    th = [2.0, 0.0, 1.0, float(ln2), 0.0, float(ln2)]
    pix = K.counting(np.array([[0.5, 2.0]]), (0, 0, 0, 1), None)
    s = K.Sums(th, pix, 2)
    tol = 8 * np.finfo(LD).eps
    assert s.n == 2 and abs(s.chi2 - LD(0.25)) <= tol + 2e-16      # (ln 2 in float64: 2e-17 off)
    J0 = np.array([0.5, 0, -2 * ln2, 0, 0, -1], dtype=LD)
    J1 = np.array([1, 0, 0, 0, 0, 0], dtype=LD)
    N = np.outer(J0, J0) + np.outer(J1, J1)
    assert np.max(np.abs(K.unpack(s.N, 6) - N)) <= 1e-15
    assert np.max(np.abs(s.g - J0 * LD(-0.5))) <= 1e-15
    assert s.bchi > 0 and np.all(s.bN > 0) and np.all(s.bg > 0)
    # fewer than 6 counting pixels: degenerate, nothing but the status
    out = K.emulate(np.array([[0.5, 2.0]]), (0, 0, 0, 1), None, th, LAM0, XTOL, 5, poison=POISON)
    assert out["status"] == 3 and out["theta"] is None and np.all(out["trace"] == POISON)
    # the tile rule and the workspace
    assert K.tiling(3, 15) == {"tiles": 1, "workgroups": 3}
    assert K.tiling(1, 67 * 131) == {"tiles": 9, "workgroups": 9}
    assert K.tiling(2, 360000) == {"tiles": 352, "workgroups": 704}
    assert K.workspace_bytes(2, 360000) == (704 * 29 + 2 * 48) * 16
    assert K.depth(15) == 85 and K.depth(360000) == 86
    assert [K.tri(i, j) for i, j in K.TRI] == list(range(21))


def test_jacobian_against_richardson_differences():
    th = np.array([-1.3, 3.3, 4.8, 0.21, 0.06, 0.13], dtype=LD)
    ix, iz = (a.ravel() for a in np.meshgrid(np.arange(7), np.arange(9), indexing="ij"))
    _, J = K.model(th, ix, iz, LD)
    for k in range(6):
        def diff(h):
            lo, hi = th.copy(), th.copy()
            lo[k] -= h
            hi[k] += h
            return (K.model(hi, ix, iz, LD, with_jac=False)[0]
                    - K.model(lo, ix, iz, LD, with_jac=False)[0]) / (2 * h)
        h = LD(1e-3) * max(abs(th[k]), LD(0.1))
        rich = (4 * diff(h / 2) - diff(h)) / 3                      # O(h^4)
        assert np.max(np.abs(rich - J[k])) <= 1e-10 * np.max(np.abs(J[k])), k


# ---- the emulation inside the bounds, the mistakes outside -----------------------------------------
@pytest.mark.parametrize("case", ["5x3", "noise-free", "negative, box, mask, NaN", "noisy"])
def test_float64_emulation_stays_inside_the_bounds(case):
    box, mask = None, None
    if case == "5x3":
        truth = np.array([1.0, 2.2, 1.1, 0.30, 0.05, 0.50])
        img = gauss(5, 3, truth)
        th0 = peak_start(img, (0.4, 0.0, 0.4))
    elif case == "noisy":
        img, th0, truth = noisy_case()
    else:
        truth = np.array([1.3, 33.3, 64.8, 0.0049, 0.0015, 0.0021])
        if case != "noise-free":
            truth[0] = -0.7
            box = (8, 60, 20, 120)
            mask = np.ones((67, 131), dtype=bool)
            mask[::7, ::5] = False
        img = gauss(67, 131, truth)
        if case != "noise-free":
            img[20:23, 40:47] = np.nan
        th0 = peak_start(np.nan_to_num(img), (0.003, 0.0, 0.003))
    box = box or whole(*img.shape)
    out = K.emulate(img, box, mask, th0, LAM0, XTOL, 60, poison=POISON)
    worst = K.follow(img, box, mask, th0, LAM0, XTOL, 60, out, POISON)
    assert worst <= 1.0 and out["status"] == 1
    if case != "noisy":
        assert out["niter"] <= 20
        assert np.max(np.abs(out["theta"] - truth) / K.scales(truth).astype(np.float64)) <= 1e-9
    # an exhausted fit is status 0, and the reference follows it too
    short = K.emulate(img, box, mask, th0, LAM0, XTOL, 3, poison=POISON)
    assert short["status"] == 0 and short["niter"] == 3
    assert K.follow(img, box, mask, th0, LAM0, XTOL, 3, short, POISON) <= 1.0


@pytest.mark.parametrize("mistake", ["centre", "b_factor", "lam_identity", "accept_le"])
def test_planted_mistakes_are_outside_the_bounds(mistake):
    """A centre off by half a pixel (chi^2 of the first trial), no factor 2 on the B derivative and
    lambda I for lambda diag N (the first step's backward error), and an accept on <= (a trial
    with the bits of chi^2_cur, which the strict rule rejects; it needs the noisy image, whose fit
    ends in such ties)."""
    img, th0, _ = noisy_case()
    out = K.emulate(img, whole(*img.shape), None, th0, LAM0, XTOL, 60, poison=POISON, mistake=mistake)
    assert out["status"] != 3
    with pytest.raises(AssertionError):
        K.follow(img, whole(*img.shape), None, th0, LAM0, XTOL, 60, out, POISON)


def test_tampered_outputs_are_caught():
    img, th0, _ = noisy_case()
    box = whole(*img.shape)
    good = K.emulate(img, box, None, th0, LAM0, XTOL, 60, poison=POISON)
    K.follow(img, box, None, th0, LAM0, XTOL, 60, good, POISON)

    def tampered(**change):
        bad = dict(good, trace=good["trace"].copy(), cov=good["cov"].copy())
        for k, f in change.items():
            bad[k] = f(bad[k])
        with pytest.raises(AssertionError):
            K.follow(img, box, None, th0, LAM0, XTOL, 60, bad, POISON)

    def edit(i, j, v):
        def f(a):
            a[i, j] = v if not callable(v) else v(a[i, j])
            return a
        return f
    tampered(trace=edit(3, 1, lambda x: 2 * x))                   # a lambda off the sequence
    tampered(trace=edit(good["niter"], 0, 1.0))                   # a row beyond d_niter written
    tampered(trace=edit(2, 2, 0.0))                               # a clearly better trial rejected
    tampered(trace=edit(1, 0, lambda x: x * (1 + 1e-9)))          # chi^2 outside its bound
    tampered(npix=lambda n: n - 1)
    tampered(cov=lambda c: c * (1 + 1e-9))
    tampered(status=lambda s: 0)
    tampered(theta=lambda t: t * (1 + 1e-15))
    tampered(chi2=lambda c: np.nextafter(c, 1.0))


# ---- gauss_results, gauss_start --------------------------------------------------------------------
CELL = np.radians(0.05 / 3600.)


def _sigma(q):
    return np.linalg.inv(2 * np.array([[q[0], q[1]], [q[1], q[2]]]))


def test_gauss_results_sizes_and_flux():
    beam = E.beam_quadratic(0.30, 0.20, 30., CELL)
    src = E.beam_quadratic(0.50, 0.25, -20., CELL)
    q = np.linalg.inv(2 * (_sigma(beam) + _sigma(src)))
    conv = [q[0, 0], q[0, 1], q[1, 1]]
    eye = K.unpack(np.zeros(21), 6)
    cov = [1.0 if i == j else 0.0 for i, j in K.TRI]
    r, p = E.gauss_results([[1.5, 30.2, 40.7] + conv, [1.5, 30.2, 40.7] + list(beam)], [cov, cov],
                           [0.0, 0.0], [100, 100], beam, CELL, shape=(64, 80), status=[1, 1])
    # a known convolved size deconvolves to the known source
    d = r["deconvolved"]
    assert not r["point_source"] and abs(d["maj_as"] - 0.5) <= 1e-12 and abs(d["min_as"] - 0.25) <= 1e-12
    assert abs(d["pa_deg"] + 20.) <= 1e-10
    # a beam-sized fit is a point source, its flux the peak
    assert p["point_source"] and p["deconvolved"] is None and abs(p["I"]["val"] - 1.5) <= 1e-15
    assert abs(p["maj_as"] - 0.30) <= 1e-12 and abs(p["min_as"] - 0.20) <= 1e-12 and abs(p["pa_deg"] - 30.) <= 1e-9
    assert r["I"]["unit"] == "Jy" and r["Ierr"] == {"val": None, "unit": "Jy"} and r["status"] == 1
    # East = decreasing ix, North = +z, from the centre (31.5, 39.5)
    assert abs(r["east_as"] - (-(30.2 - 31.5) * 0.05)) <= 1e-12 and abs(r["north_as"] - (40.7 - 39.5) * 0.05) <= 1e-12
    # I equals the pixel sum over the beam area, on a grid fine against both Gaussians
    fb = np.array(beam) / 16.
    fq = np.array(conv) / 16.                                      # cells 4 times smaller
    img = gauss(512, 512, [1.5, 255.3, 256.1] + list(fq))
    omega = np.pi / np.sqrt(fb[0] * fb[2] - fb[1] ** 2)
    fine = E.gauss_results([[1.5, 255.3, 256.1] + list(fq)], [cov], [0.0], [1], fb, CELL / 4)[0]
    assert abs(fine["I"]["val"] - img.sum() / omega) <= 1e-12 * fine["I"]["val"]
    assert abs(fine["I"]["val"] - r["I"]["val"]) <= 1e-12 * r["I"]["val"]
    # not positive definite / not finite: NaN, no sizes
    bad = E.gauss_results([[1.0, 2.0, 3.0, 0.1, 0.2, 0.1], [np.nan] * 6], [cov, cov], [np.nan] * 2,
                          [-1, -1], beam, CELL, rms=0.1)
    assert all(np.isnan(b["I"]["val"]) and b["deconvolved"] is None and b["Ierr"]["val"] is None for b in bad)
    assert eye.shape == (6, 6)


def test_gauss_results_errors_by_hand():
    """The covariance rms^2 Omega_b (J^T J)^-1 with a diagonal J^T J = diag(n_i): sigma_i =
    rms sqrt(Omega_b / n_i); Ierr by first order with dI/dS = I / S, dI/dA = -I C / (2 det),
    dI/dB = I B / det, dI/dC = -I A / (2 det)."""
    beam = (0.02, 0.004, 0.03)
    A, B, C = 0.011, -0.002, 0.017
    S, rms = 2.5, 0.01
    n = np.array([400., 90., 70., 5e6, 7e6, 3e6])
    cov = [n[i] if i == j else 0.0 for i, j in K.TRI]
    r = E.gauss_results([[S, 10., 12., A, B, C]], [cov], [1.0], [500], beam, CELL, rms=rms)[0]
    omega = np.pi / np.sqrt(0.02 * 0.03 - 0.004 ** 2)
    sd = rms * np.sqrt(omega / n)
    assert abs(r["peak_err"] - sd[0]) <= 1e-15 and abs(r["x0_err"] - sd[1]) <= 1e-15
    assert abs(r["z0_err"] - sd[2]) <= 1e-15 and np.allclose(r["abc_err"], sd[3:], rtol=1e-13, atol=0)
    det = A * C - B * B
    flux = S * np.sqrt((0.02 * 0.03 - 0.004 ** 2) / det)
    grad = np.array([flux / S, -flux * C / (2 * det), flux * B / det, -flux * A / (2 * det)])
    want = np.sqrt(np.sum((grad * sd[[0, 3, 4, 5]]) ** 2))
    assert abs(r["I"]["val"] - flux) <= 1e-15 * flux and abs(r["Ierr"]["val"] - want) <= 1e-13 * want
    # the first-order gradient against a central difference of I itself
    for k, g in zip((3, 4, 5), grad[1:]):
        th = np.array([S, 10., 12., A, B, C])
        h = 1e-6 * th[k]
        lo, hi = th.copy(), th.copy()
        lo[k] -= h
        hi[k] += h
        f = lambda t: E.gauss_results([t], [cov], [1.0], [500], beam, CELL)[0]["I"]["val"]
        assert abs((f(hi) - f(lo)) / (2 * h) - g) <= 1e-6 * abs(g)


def test_gauss_start_on_host_tensors():
    import torch
    img = torch.zeros(3, 5, 7, dtype=torch.float64)
    img[0, 2, 3], img[0, 0, 0], img[0, 4, 6] = -4.0, 5.0, float("nan")
    img[1, 1, 1], img[1, 3, 2] = 9.0, 2.0
    img[2] = float("nan")
    mask = np.ones((5, 7), dtype=bool)
    mask[1, 1] = False
    beam = [(0.1, 0.0, 0.2), (0.3, 0.01, 0.4), (0.5, 0.0, 0.6)]
    th = E.gauss_start(img, 5, 7, beam, box=(1, 4, 1, 6), mask=mask).numpy()
    assert th.shape == (3, 6) and np.array_equal(th[:, 3:], np.array(beam))
    assert list(th[0, :3]) == [-4.0, 2.0, 3.0]          # the box leaves (0, 0) out; NaN is skipped
    assert list(th[1, :3]) == [2.0, 3.0, 2.0]           # the mask leaves (1, 1) out
    assert np.isnan(th[2, 0])                           # no counting pixel: a start gaussfit refuses
    one = E.gauss_start(img[:1], 5, 7, beam[0]).numpy()
    assert list(one[0]) == [5.0, 0.0, 0.0, 0.1, 0.0, 0.2]
    with pytest.raises(ValueError):
        E.gauss_start(img, 5, 7, beam[:2])


# ---- the ABI ---------------------------------------------------------------------------------------
def test_abi_signatures_and_the_workspace_query():
    res, args = _lib.SIGNATURES["rjp_gaussfit"]
    P, i32, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    assert res is ctypes.c_int64
    assert args == [P, P, i32, i32, i32, ctypes.POINTER(i32), P, P, dbl, dbl, i32, P, P, P, P, P, P, P,
                    ctypes.c_size_t, P]
    assert _lib.SIGNATURES["rjp_gaussfit_workspace"] == (ctypes.c_size_t, [i32, i32])
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    assert "int64_t rjp_gaussfit(rjp_ctx* ctx, const double* d_img, int32_t n_maps" in hdr
    assert "size_t rjp_gaussfit_workspace(int32_t n_maps, int32_t box_pixels);" in hdr
    lib = _lib.load()
    for n_maps, nb in ((1, 1), (3, 15), (1, 1024), (1, 1025), (64, 65536), (2, 360000), (7, 2 ** 31 - 1)):
        assert lib.rjp_gaussfit_workspace(n_maps, nb) == K.workspace_bytes(n_maps, nb), (n_maps, nb)
    assert lib.rjp_gaussfit_workspace(0, 15) == 0 and lib.rjp_gaussfit_workspace(1, 0) == 0
    assert lib.rjp_gaussfit_workspace(-1, 15) == 0 and lib.rjp_gaussfit_workspace(1, -5) == 0
    # a NULL context is refused before anything else
    assert lib.rjp_gaussfit(None, None, 1, 1, 1, None, None, None, 1e-3, 1e-12, 1, None, None, None,
                            None, None, None, None, 0, None) == _lib.RJP_ERR_ARG


def test_check_gaussfit_from_plain_cpp(tmp_path):
    """check_gaussfit compiled into a stand-alone program by plain g++
    (tests/rjp_args_gaussfit_cases.cpp): every refusal, status and message, in the order the check
    makes them -- the messages tests/test_gpu_gaussfit.py sees from the library."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "rjp_args_gaussfit_cases"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rajepy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rjp_args_gaussfit_cases.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        case, status, msg = line.split("\t")
        got[case] = (int(status), msg)
    want = {"nulls": ["NULL d_img", "NULL h_box", "NULL d_theta", "NULL d_chi2", "NULL d_cov", "NULL d_npix",
                      "NULL d_niter", "NULL d_status", "NULL beats sizes"],
            "sizes": ["n_maps 0", "nx 0", "nz -1", "sizes beat the box"],
            "npix": ["nx nz 2^31", "npix beats the box"],
            "box": ["i0 < 0", "i1 = nx", "i1 < i0", "j0 < 0", "j1 = nz", "j1 < j0", "box beats lambda0"],
            "tol": ["lambda0 0", "lambda0 inf", "lambda0 nan", "xtol -1", "xtol inf", "xtol nan",
                    "lambda0 beats n_iter"],
            "iter": ["n_iter 0"]}
    seen = set()
    for key, cases in want.items():
        for case in cases:
            assert got[case] == (_lib.RJP_ERR_ARG, K.MSG[key]), case
            seen.add(case)
    valid = {c for c in got if c.startswith("valid")}
    assert len(valid) == 3 and all(got[c] == (0, "") for c in valid)
    assert seen | valid == set(got)


def test_clean_result_carries_imfit_beside_its_six_fields():
    from rajepy_amd import classes
    r = classes.CleanResult(1, 2, 3, 4, 5, 6, imfit=[{"I": 1}])
    assert len(r) == 6 and tuple(r) == (1, 2, 3, 4, 5, 6) and r.imfit == [{"I": 1}]
    assert classes.CleanResult(1, 2, 3, 4, 5, 6).imfit is None
    moved = r._replace(image=9)
    assert moved.image == 9 and moved.imfit is r.imfit
    assert r._replace(imfit=None).imfit is None and r._replace(imfit=None).image == 1
    assert classes.CleanResult._make(range(6)).imfit is None


def test_the_step_test_keeps_a_zero_peak():
    """s_0 = max(|S|, 1e-300): a zero peak with a zero step passes, with any step it does not."""
    s = K.scales([0.0, 1.0, 1.0, 0.1, 0.0, 0.2])
    assert float(s[0]) == 1e-300 and float(s[3]) == float(s[5]) and abs(float(s[3]) - 0.3) < 1e-16
    assert float(K.scales([-2.5, 0, 0, 1, 0, 1])[0]) == 2.5
