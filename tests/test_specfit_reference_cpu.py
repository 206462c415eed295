"""tests/specfit_ref.py -- the long-double reference of K21 (rjp_cube_moments, rjp_specfit) that
tests/test_gpu_specfit.py applies on the device -- pinned without a GPU: hand-worked cases,
Richardson differences of the Jacobian, the float64 emulations on EVERY GPU case's inputs (inside
the bounds, converging where the GPU test demands convergence, every path of the iteration
reached), planted mistakes (outside the bounds), the argument checks from plain C++, the ABI
table, the host helpers by hand and the Python paths on a recording engine."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from rajepy_amd import _lib
from rajepy_amd import engine as E
from rajepy_amd import spectra
from tests import specfit_cases as C
from tests import specfit_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = K.LD
P_F, P_I, P_T = 7.25, -77, -7.5
PATHS = {}


def emulate(case, n_iter=C.N_ITER, theta0=None, mistake=None):
    th0 = case["theta0"] if theta0 is None else theta0
    out = K.emulate(case["Y"], case["x"], case["w"], case["x_ref"], th0, case["free"], C.LAM0, C.XTOL,
                    n_iter, case["live"], poison=P_T, mistake=mistake)
    d3 = out["status"] == 3
    out["chi2"] = np.where(d3, P_F, out["chi2"])
    out["cov"][d3] = P_F
    out["nchan"], out["niter"] = np.where(d3, P_I, out["nchan"]), np.where(d3, P_I, out["niter"])
    if mistake is None:
        for k, v in out["paths"].items():
            PATHS[k] = PATHS.get(k, 0) + v
    return out


def follow(case, out, n_iter=C.N_ITER, theta0=None):
    th0 = case["theta0"] if theta0 is None else theta0
    return K.follow_all(case["Y"], case["x"], case["w"], case["x_ref"], th0, case["free"], C.LAM0,
                        C.XTOL, n_iter, out, P_T, P_F, P_I, case["live"])


# ---- hand-worked cases --------------------------------------------------------------------------
def test_three_channels_of_a_known_gaussian_by_hand():
    """theta = (2, 0, 1, 0, 0) at x = (-1, 0, 1) against y = (1, 1, 1): E = (e^-1/2, 1, e^-1/2)."""
    h = np.exp(LD(-0.5))
    s = K.Sums([[2.0, 0.0, 1.0, 0.0, 0.0]], [[1.0, 1.0, 1.0]], [-1.0, 0.0, 1.0], None, 0.0)
    r = np.array([1 - 2 * h, LD(-1), 1 - 2 * h])
    J = np.array([[h, 1, h], [-2 * h, 0, 2 * h], [2 * h, 0, 2 * h], [1, 1, 1], [-1, 0, 1]], dtype=LD)
    assert abs(s.chi2[0] - np.sum(r * r)) < 1e-18
    assert np.max(np.abs(s.N[0] - J @ J.T)) < 1e-18 and np.max(np.abs(s.g[0] - J @ r)) < 1e-18
    assert s.count[0] == 3 and 0 < s.bchi[0] < 1e-13 and np.all(s.bN[0] >= 0)
    # weights (1, 0, 4): the middle channel does not count; a NaN channel neither
    s = K.Sums([[2.0, 0.0, 1.0, 0.0, 0.0]], [[1.0, np.nan, 1.0]], [-1.0, 0.0, 1.0], [1.0, 3.0, 4.0], 0.0)
    assert s.count[0] == 2 and abs(s.chi2[0] - 5 * (1 - 2 * h) ** 2) < 1e-18
    # a held baseline: the identity's rows
    s = K.Sums([[2.0, 0.0, 1.0, 0.0, 0.0]], [[1.0, 1.0, 1.0]], [-1.0, 0.0, 1.0], None, 0.0, [1, 1, 1, 0, 0])
    assert np.array_equal(s.N[0][3:], np.eye(5)[3:]) and np.all(s.g[0][3:] == 0) and np.all(s.bN[0][3:] == 0)
    # the baseline in the model: b0 + b1 (x - x_ref)
    m = K.model([0.0, 0.0, 1.0, 0.5, 0.25], [-1.0, 0.0, 1.0], 1.0)[0]
    assert np.array_equal(m[0], np.array([0.0, 0.25, 0.5], dtype=LD))


def test_a_top_hat_in_closed_form():
    """y = 3 on channels 4 .. 10 of x = 0 .. 15 (dx = 0.5): m0 = 3 * 7 * 0.5, m1 = 7, m2^2 = (7^2 - 1)
    / 12; the peak is channel 4 (the lowest of the tie)."""
    y = np.zeros(16)
    y[4:11] = 3.0
    m = K.moments(y, np.arange(16.0), np.full(16, 0.5), 5.0, clip=1.0)
    assert m["m0"] == 10.5 and m["m1"] == 7.0 and abs(m["m2"] - np.sqrt(LD(4))) < 1e-18
    assert (m["peak"], m["ipeak"], m["count"]) == (3.0, 4, 7)
    # the float64 emulation agrees inside the bounds, the reference with itself exactly
    e = K.moments(y, np.arange(16.0), np.full(16, 0.5), 5.0, 1.0, True, np.float64)
    assert K.check_moments(y, np.arange(16.0), np.full(16, 0.5), 5.0, 1.0, True, e) <= 1.0


def test_a_finely_sampled_gaussian_recovers_its_parameters():
    """A = 1.7, x0 = 0.3, s = 2.5 on 4001 channels of width 0.01 over +- 8 s: m0 -> A s sqrt(2 pi),
    m1 -> x0, m2 -> s; the trapezoidal sum of a Gaussian over +- 8 s is exact to its tails, e^-32."""
    x = 0.3 + np.linspace(-20.0, 20.0, 4001)
    y = K.model([1.7, 0.3, 2.5, 0, 0], x, 0.0)[0][0].astype(np.float64)
    m = K.moments(y, x, np.full(x.size, 0.01), 0.0)
    assert abs(m["m0"] / (1.7 * 2.5 * np.sqrt(2 * np.pi)) - 1) < 1e-13
    assert abs(m["m1"] - 0.3) < 1e-13 and abs(m["m2"] / 2.5 - 1) < 1e-13
    assert m["ipeak"] == 2000


def test_special_cases_of_the_moments():
    case = C.moment_special()
    got = [K.moments(case["Y"][p], case["x"], case["dx"], case["x_ref"], case["clip"], bool(case["live"][p]))
           for p in range(7)]
    assert (got[0]["ipeak"], got[0]["count"], got[0]["peak"]) == (1, 6, 2.0)
    assert got[1]["count"] == 3 and got[1]["ipeak"] == 3             # 0.5 counts, nextafter(0.5, 0) does not
    for p, n in ((2, 2), (3, 0), (5, 0), (6, 0)):
        g = got[p]
        assert g["m0"] == 0 and not np.signbit(g["m0"]) and np.isnan(g["m1"]) and np.isnan(g["m2"])
        assert np.isnan(g["peak"]) and g["ipeak"] == -1 and g["count"] == n
    assert got[4]["m0"] == 1 and got[4]["m1"] == 1 and np.isnan(got[4]["m2"]) and got[4]["ipeak"] == 2


def test_jacobian_against_richardson_differences():
    rng = np.random.default_rng(5)
    x = np.linspace(-20.0, 25.0, 23)
    for th in ([1.3, 2.0, 4.0, 0.2, 0.01], [1.3, 2.0, 4.0, -0.6, 11.0, 2.5, 0.2, -0.01]):
        th = np.array(th, dtype=LD)
        J = K.model(th, x, 1.5)[1][0]
        for i in range(th.size):
            def f(h):
                a, b = th.copy(), th.copy()
                a[i] += h
                b[i] -= h
                return (K.model(a, x, 1.5)[0][0] - K.model(b, x, 1.5)[0][0]) / (2 * h)
            h = LD(1e-3) * max(abs(th[i]), LD(1))
            rich = (4 * f(h / 2) - f(h)) / 3
            assert np.max(np.abs(rich - J[i])) <= 1e-11 * max(1.0, float(np.max(np.abs(J[i])))), i
    assert rng is not None


# ---- the emulation on every GPU case -------------------------------------------------------------
@pytest.mark.parametrize("n_comp,bl,n_chan", C.SIZED)
def test_emulation_on_the_sized_cases(n_comp, bl, n_chan):
    case = C.sized(n_comp, bl, n_chan)
    out = emulate(case)
    assert follow(case, out) <= 1.0
    assert np.all(out["status"] != 3) and np.all(out["nchan"] == np.sum(
        (case["w"] if case["w"] is not None else np.ones(n_chan)) > 0))
    if C.must_converge(case):
        assert np.all(out["status"] == 1) and C.scaled_error(out["theta"], case["truth"]) <= 1e-9


@pytest.mark.parametrize("name", ["bad 1", "bad 2", "starts", "narrow", "flat held", "flat free", "held"])
def test_emulation_on_the_other_cases(name):
    case = {"bad 1": lambda: C.bad_data(1), "bad 2": lambda: C.bad_data(2), "starts": C.degenerate_starts,
            "narrow": C.narrow, "flat held": lambda: C.flat(False), "flat free": lambda: C.flat(True),
            "held": C.held}[name]()
    out = emulate(case)
    assert follow(case, out) <= 1.0
    if "degenerate" in case:
        deg = np.zeros(out["status"].size, dtype=bool)
        deg[case["degenerate"]] = True
        assert np.array_equal(out["status"] == 3, deg)
        assert np.all(out["status"][~deg] == 1)
        assert C.scaled_error(out["theta"][~deg], case["truth"][~deg]) <= 1e-9
    if name.startswith("flat"):
        assert out["status"][4] == 2 and out["status"][3] == 1
    if name == "held":
        assert np.all(out["status"] == 1) and C.scaled_error(out["theta"], case["truth"]) <= 1e-9
        assert np.array_equal(out["theta"][:, [1, 4]], case["theta0"][:, [1, 4]])


def test_emulation_exhausted_and_continued():
    case = C.sized(1, True, 64)
    first = emulate(case, 3)
    assert follow(case, first, 3) <= 1.0 and np.all(first["status"] == 0) and np.all(first["niter"] == 3)
    second = emulate(case, theta0=first["theta"])
    assert follow(case, second, theta0=first["theta"]) <= 1.0
    assert np.all(second["status"] == 1) and C.scaled_error(second["theta"], case["truth"]) <= 1e-9


def test_emulation_fits_the_big_stack_from_the_moments():
    """The non-vacuity of the GPU test's 1e-9 on 130 x 65 sightlines: the float64 emulation, started
    from the emulated moments, converges on EVERY pixel."""
    case = C.big()
    th0 = C.start_from_moments(case["Y"], case["x"], case["x_ref"])
    out = emulate(case, theta0=th0)
    assert np.all(out["status"] == 1), np.bincount(out["status"])
    assert C.scaled_error(out["theta"], case["truth"]) <= 1e-9
    pick = np.arange(0, out["status"].size, 97)         # a sample of the pixels, followed
    sub = dict(case, Y=case["Y"][pick])
    assert follow(sub, {k: v[pick] for k, v in out.items() if k != "paths"}, theta0=th0[pick]) <= 1.0


def test_every_path_of_the_iteration_is_reached():
    """(after the emulations above, in file order) accept, reject, pivot reject, stalled, converged,
    exhausted, degenerate: each taken by at least one pixel of the GPU cases."""
    if not PATHS:
        for f in (lambda: C.flat(True), lambda: C.bad_data(1), lambda: C.sized(1, False, 4)):
            emulate(f())
    assert all(PATHS.get(k, 0) > 0 for k in ("accept", "reject", "pivot", "stalled", "converged",
                                             "exhausted", "degenerate")), PATHS


@pytest.mark.parametrize("n_pix,n_chan", C.MOMENT_SIZES + [(7, 6)])
def test_emulated_moments_inside_the_bounds(n_pix, n_chan):
    case = C.moment_special() if (n_pix, n_chan) == (7, 6) else C.moment_case(n_pix, n_chan)
    worst = 0.0
    for p in range(n_pix):
        e = K.moments(case["Y"][p], case["x"], case["dx"], case["x_ref"], case["clip"],
                      bool(case["live"][p]), np.float64)
        worst = max(worst, K.check_moments(case["Y"][p], case["x"], case["dx"], case["x_ref"],
                                           case["clip"], bool(case["live"][p]), e))
    assert worst <= 1.0


# ---- planted mistakes ----------------------------------------------------------------------------
@pytest.mark.parametrize("mistake", ["s2", "no_weight", "uncounted"])
def test_planted_mistakes_of_the_fit_are_outside_the_bounds(mistake):
    case = C.sized(2, True, 64)                         # per-channel weights, an eighth of them zero
    assert case["w"] is not None and np.any(case["w"] == 0)
    assert follow(case, emulate(case)) <= 1.0
    with pytest.raises(AssertionError):
        follow(case, emulate(case, mistake=mistake))


@pytest.mark.parametrize("mistake", ["no_dx_m1", "var_xref", "peak_abs"])
def test_planted_mistakes_of_the_moments_are_outside_the_bounds(mistake):
    rng = np.random.default_rng(3)
    x = C.axis("nonuniform", 64, rng)
    dx = C.channel_widths(x)
    y = C.analytic(np.array([[1.2, 4.0, 5.0, 0, 0]]), x, 0.0)[0] - \
        (2.5 if mistake == "peak_abs" else 0.3) * np.exp(-0.5 * ((x + 15) / (0.5 if mistake == "peak_abs" else 1.5)) ** 2)
    args = (y, x, dx, float(x[40]), 0.0, True)
    assert K.check_moments(*args, K.moments(*args, np.float64)) <= 1.0
    with pytest.raises(AssertionError):
        K.check_moments(*args, K.moments(*args, np.float64, mistake=mistake))


def test_tampered_outputs_are_caught():
    case = C.sized(1, True, 64)
    good = emulate(case)
    for key, p, val in (("chi2", 3, None), ("theta", 5, None), ("niter", 7, 2), ("status", 9, 0),
                        ("nchan", 11, 63)):
        bad = {k: np.array(v, copy=True) for k, v in good.items() if k != "paths"}
        if val is None:
            bad[key][p] = bad[key][p] * (1 + 1e-9)
        else:
            bad[key][p] = val
        with pytest.raises(AssertionError):
            follow(case, bad)
    bad = {k: np.array(v, copy=True) for k, v in good.items() if k != "paths"}
    bad["trace"][2, good["niter"][2]] = 0.0             # a row beyond d_niter written
    with pytest.raises(AssertionError):
        follow(case, bad)


# ---- the argument checks and the ABI ------------------------------------------------------------------
def test_checks_from_plain_cpp(tmp_path):
    """check_cube_moments and check_specfit compiled into a stand-alone program by plain g++
    (tests/rjp_args_specfit_cases.cpp): every refusal, status and message, in the order the checks
    make them -- the messages tests/test_gpu_specfit.py sees from the library."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "rjp_args_specfit_cases"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rajepy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rjp_args_specfit_cases.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        case, status, msg = line.split("\t")
        got[case] = (int(status), msg)
    want_m = {"nulls": ["NULL d_cube", "NULL h_x", "NULL h_dx", "NULL d_mom", "NULL beats sizes"],
              "sizes": ["n_pix 0", "n_chan 0", "n_chan -2", "sizes beat the limit"],
              "chan": ["n_chan 4097", "the limit beats x"],
              "x": ["x nan", "x -inf", "x beats dx"],
              "dx": ["dx negative", "dx inf", "dx nan", "dx beats x_ref"],
              "xref": ["x_ref nan", "x_ref inf", "x_ref beats clip"],
              "clip": ["clip negative", "clip inf", "clip nan", "clip beats the workgroups"],
              "wgs": ["2^31 workgroups"]}
    want_f = {"nulls": ["NULL d_cube", "NULL h_x", "NULL d_theta", "NULL d_chi2", "NULL d_cov", "NULL d_nchan",
                        "NULL d_niter", "NULL d_status", "NULL beats sizes"],
              "sizes": ["n_pix 0", "n_pix -3", "n_chan 0", "sizes beat the limit and n_comp"],
              "chan": ["n_chan 4097", "the limit beats n_comp"],
              "comp": ["n_comp 0", "n_comp 3", "n_comp beats x"],
              "x": ["x nan", "x inf", "x beats x_ref"],
              "xref": ["x_ref nan", "x_ref beats w"],
              "w": ["w negative", "w inf", "w nan", "w beats free"],
              "free": ["no free parameter", "no free parameter among the first five", "free beats lambda0"],
              "tol": ["lambda0 0", "lambda0 inf", "lambda0 nan", "xtol -1", "xtol inf", "xtol nan",
                      "lambda0 beats n_iter"],
              "iter": ["n_iter 0", "n_iter beats the workgroups"],
              "wgs": ["2^31 workgroups"]}
    seen = set()
    for pre, want, msg in (("m ", want_m, K.MSG_M), ("f ", want_f, K.MSG_F)):
        for key, cases in want.items():
            for case in cases:
                assert got[pre + case] == (_lib.RJP_ERR_ARG, msg[key]), pre + case
                seen.add(pre + case)
    valid = {c for c in got if c[2:].startswith("valid")}
    assert len(valid) == 7 and all(got[c] == (0, "") for c in valid)
    assert seen | valid == set(got)


def test_abi_signatures():
    P, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    DP, U8 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8)
    assert _lib.SIGNATURES["rjp_cube_moments"] == (i64, [P, P, i64, i32, DP, DP, dbl, dbl, P, P, P, P, P])
    assert _lib.SIGNATURES["rjp_specfit"] == (i64, [P, P, i64, i32, DP, dbl, DP, P, i32, U8, P, dbl, dbl,
                                                    i32, P, P, P, P, P, P, P])
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    assert "int64_t rjp_cube_moments(rjp_ctx* ctx, const double* d_cube, int64_t n_pix, int32_t n_chan," in hdr
    assert "int64_t rjp_specfit(rjp_ctx* ctx, const double* d_cube, int64_t n_pix, int32_t n_chan," in hdr
    assert "#define RJP_SPECFIT_MAX_CHAN 4096" in hdr and "#define RJP_SPECFIT_MAX_COMP 2" in hdr
    assert "#define RJP_VERSION 117" in hdr                            # symbols added, none changed
    assert spectra.SPECFIT_MAX_COMP == K.MAX_COMP == 2 and spectra.SPECFIT_MAX_CHAN == K.MAX_CHAN == 4096
    assert E.SPECFIT_MAX_CHAN == 4096 and E.specfit_results is spectra.specfit_results
    lib = _lib.load()
    # a NULL context is refused before anything else
    assert lib.rjp_cube_moments(None, None, 1, 1, None, None, 0.0, 0.0, None, None, None, None,
                                None) == _lib.RJP_ERR_ARG
    assert lib.rjp_specfit(None, None, 1, 1, None, 0.0, None, None, 1, None, None, 1e-3, 1e-10, 1, None,
                           None, None, None, None, None, None) == _lib.RJP_ERR_ARG


# ---- the host helpers by hand --------------------------------------------------------------------------
def test_velocity_axis_by_hand():
    nu0 = 2.0e10
    v, dv = E.velocity_axis([nu0 * (1 - 1e-4), nu0, nu0 * (1 + 2e-4), nu0 * (1 + 3e-4)], nu0)
    c = 299792.458
    assert np.allclose(v, [1e-4 * c, 0.0, -2e-4 * c, -3e-4 * c], rtol=1e-11, atol=1e-9)
    assert np.allclose(dv, [1e-4 * c, 1.5e-4 * c, 1.5e-4 * c, 1e-4 * c], rtol=1e-10)
    v1, dv1 = E.velocity_axis(nu0 * (1 + 1e-4), nu0)
    assert v1.shape == (1,) and dv1[0] == 0.0
    from rajepy_amd.maths import rrls
    assert abs(rrls.rrl_nu_0("H", 66, 1) / 22.364e9 - 1) < 1e-3        # H66a near 22.36 GHz


def test_specfit_start_by_hand():
    x = np.array([0.0, 1.0, 3.0, 6.0])
    mom = torch.tensor([[1.0, 2.0, 3.0, 0.0], [1.0, 1.0, 1.0, np.nan], [0.8, np.nan, 0.0, np.nan],
                        [2.5, 1.5, 0.7, np.nan]], dtype=torch.float64)
    ipeak = torch.tensor([1, 3, 2, -1], dtype=torch.int32)
    th = E.specfit_start(mom, ipeak, x).numpy()
    assert th.shape == (5, 4)
    assert np.array_equal(th[0, :3], [2.5, 1.5, 0.7]) and np.array_equal(th[1, :3], [1.0, 6.0, 3.0])
    # m2 NaN at channel 3: twice (6 - 3) / 1; m2 = 0 at channel 2: twice (6 - 1) / 2
    assert np.array_equal(th[2, :3], [0.8, 6.0, 5.0])
    assert np.all(np.isnan(th[:3, 3])) and np.all(th[3:] == 0)
    with pytest.raises(ValueError):
        E.specfit_start(mom, ipeak, x, n_comp=2)


def test_specfit_results_errors_by_hand():
    """Pixel 0: A and s free with N_ff = [[4, 1], [1, 2]] (inverse [[2, -1], [-1, 4]] / 7), chi^2 = 6
    over 5 channels: reduced chi^2 = 2.  Pixel 1: status 3.  theta = (3, 1.5, 2, 0.25, 0)."""
    free = [1, 0, 1, 0, 0]
    N = np.eye(5)
    N[0, 0], N[0, 2], N[2, 0], N[2, 2] = 4.0, 1.0, 1.0, 2.0
    cov = torch.tensor(np.stack([K.pack(N), np.full(15, np.nan)], axis=1))
    theta = torch.tensor([[3.0, 9.0], [1.5, 9.0], [2.0, 9.0], [0.25, 9.0], [0.0, 9.0]], dtype=torch.float64)
    chi2 = torch.tensor([6.0, np.nan], dtype=torch.float64)
    nchan, status = torch.tensor([5, -1], dtype=torch.int32), torch.tensor([1, 3], dtype=torch.int32)
    r = E.specfit_results(theta, cov, chi2, nchan, status, free)
    g = lambda k: float(r[k][0][0]) if isinstance(r[k], list) else float(r[k][0])
    vA, vs, cAs = 2 * 2.0 / 7, 2 * 4.0 / 7, 2 * -1.0 / 7
    assert g("peak") == 3.0 and g("centre") == 1.5 and g("sigma") == 2.0 and g("b0") == 0.25
    assert abs(g("fwhm") - 2.0 * np.sqrt(8 * np.log(2))) < 1e-15
    assert abs(g("integral") - 6.0 * np.sqrt(2 * np.pi)) < 1e-14
    assert abs(g("reduced_chi2") - 2.0) < 1e-15 and g("chi2") == 6.0
    assert abs(g("e_peak") - np.sqrt(vA)) < 1e-14 and abs(g("e_sigma") - np.sqrt(vs)) < 1e-14
    assert g("e_centre") == 0.0 and g("e_b0") == 0.0 and g("e_b1") == 0.0
    assert abs(g("e_fwhm") - np.sqrt(8 * np.log(2) * vs)) < 1e-14
    want = np.sqrt(2 * np.pi * (4.0 * vA + 9.0 * vs + 2 * 3.0 * 2.0 * cAs))
    assert abs(g("e_integral") - want) < 1e-13
    for k, v in r.items():
        if k in ("nchan", "status"):
            continue
        t = v[0] if isinstance(v, list) else v
        assert np.isnan(float(t[1])), k
    assert r["status"].tolist() == [1, 3]
    # the formal errors: without the scale
    r = E.specfit_results(theta, cov, chi2, nchan, status, free, scale_errors=False)
    assert abs(float(r["e_peak"][0][0]) - np.sqrt(2.0 / 7)) < 1e-14
    with pytest.raises(ValueError):
        E.specfit_results(theta, cov, chi2, nchan, status, [0] * 5)


# ---- the Python paths on a recording engine ------------------------------------------------------------
class _NoHost(torch.Tensor):
    """A tensor that must stay where it is."""

    def cpu(self, *a, **k):
        raise AssertionError("the cube must not be copied to the host")

    numpy = tolist = __array__ = cpu


class _RecordingEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def cube_moments(self, cube, x, dx, x_ref, clip=0., mask=None):
        assert isinstance(cube, _NoHost)
        F, n = cube.shape[0], cube.numel() // cube.shape[0]
        self.calls.append(dict(kind="moments", F=F, n=n, x=np.array(x), dx=np.array(dx), x_ref=x_ref,
                               clip=clip, mask=mask))
        mom = torch.stack([torch.full((n,), v, dtype=torch.float64) for v in (2.0, 1.0, 0.5, 3.0)])
        return mom, torch.full((n,), F // 2, dtype=torch.int32), torch.full((n,), F, dtype=torch.int32)

    def specfit(self, cube, x, theta, x_ref, weights=None, free=None, n_comp=1, lambda0=1e-3, xtol=1e-10,
                n_iter=40, mask=None, trace=False):
        assert isinstance(cube, _NoHost) and not trace
        n = cube.numel() // cube.shape[0]
        P = 3 * n_comp + 2
        self.calls.append(dict(kind="specfit", n=n, x=np.array(x), theta=theta.clone(), x_ref=x_ref,
                               weights=weights, free=free, n_comp=n_comp, n_iter=n_iter, mask=mask))
        return dict(theta=theta.reshape(P, n).clone(), chi2=torch.ones(n, dtype=torch.float64),
                    cov=torch.from_numpy(np.tile(K.pack(np.eye(P))[:, None], (1, n))),
                    nchan=torch.full((n,), cube.shape[0], dtype=torch.int32),
                    niter=torch.ones(n, dtype=torch.int32), status=torch.ones(n, dtype=torch.int32))


def _model(nx, nz):
    from rajepy_amd import classes
    J = classes.JetModel

    class Model:
        moments, specfit, moments_rrl, specfit_rrl = J.moments, J.specfit, J.moments_rrl, J.specfit_rrl
        _rrl_velocity_axis = J._rrl_velocity_axis

        def _flux_maps(self, freqs, rrl=None, contsub=True, formal=False):
            self.asked.append(dict(rrl=rrl, contsub=contsub, formal=formal, F=len(freqs)))
            return torch.arange(len(freqs) * nx * nz, dtype=torch.float64).reshape(len(freqs), -1) \
                .as_subclass(_NoHost)

    m = Model()
    m.engine, m.nx, m.nz, m.asked = _RecordingEngine(), nx, nz, []
    return m


def test_model_methods_make_one_call_each_and_copy_nothing():
    from rajepy_amd.maths import rrls
    m = _model(3, 4)
    nu0 = rrls.rrl_nu_0("H", 66, 1)
    freqs = nu0 * (1 + np.array([-2e-4, -1e-4, 0.0, 1e-4, 3e-4]))
    v, dv = E.velocity_axis(freqs, nu0)
    out = m.moments_rrl("H66a", freqs, formal=True, clip_jy=1e-6)
    (c,) = m.engine.calls
    assert c["kind"] == "moments" and (c["F"], c["n"]) == (5, 12) and c["clip"] == 1e-6
    assert np.array_equal(c["x"], v) and np.array_equal(c["dx"], dv) and c["x_ref"] == v[2]
    assert m.asked == [dict(rrl="H66a", contsub=True, formal=True, F=5)]
    assert set(out) == {"m0", "m1", "m2", "peak", "ipeak", "count"} and out["m1"].shape == (3, 4)
    # specfit_rrl: the moments for the start, then ONE fit; contsub=True holds the baseline
    m.engine.calls.clear()
    res = m.specfit_rrl("H66a", freqs, n_iter=17)
    kinds = [c["kind"] for c in m.engine.calls]
    assert kinds == ["moments", "specfit"]
    c = m.engine.calls[1]
    assert list(c["free"]) == [1, 1, 1, 0, 0] and c["n_iter"] == 17 and c["n_comp"] == 1
    assert np.array_equal(c["x"], v) and c["x_ref"] == v[2] and c["weights"] is None
    assert c["theta"].shape == (5, 12) and torch.all(c["theta"][0] == 3.0) and torch.all(c["theta"][1] == v[2])
    assert torch.all(c["theta"][2] == 0.5) and torch.all(c["theta"][3:] == 0)
    assert res["fwhm"][0].shape == (3, 4) and res["status"].shape == (3, 4) and res["niter"].shape == (3, 4)
    assert float(res["e_b0"][0, 0]) == 0.0
    # contsub=False: the baseline is free; a caller's pattern is kept; two components need a start
    m.engine.calls.clear()
    m.specfit_rrl("H66a", freqs, contsub=False, weights=np.arange(1., 6.))
    assert m.engine.calls[1]["free"] is None and list(m.engine.calls[1]["weights"]) == [1, 2, 3, 4, 5]
    m.engine.calls.clear()
    m.specfit_rrl("H66a", freqs, free=[1, 0, 1, 1, 0], theta0=[1., 0., 2., 0., 0.])
    (c,) = m.engine.calls
    assert list(c["free"]) == [1, 0, 1, 1, 0] and c["theta"].shape == (5, 12) and torch.all(c["theta"][2] == 2.0)
    with pytest.raises(ValueError):
        m.specfit_rrl("H66a", freqs, comps=2)
    # any cube: a device tensor goes through as it is
    m.engine.calls.clear()
    cube = torch.ones(5, 2, 3, dtype=torch.float64).as_subclass(_NoHost)
    res = m.specfit(cube, v, comps=2, theta0=[1., 0., 2., .5, 9., 1., 0., 0.], mask=np.ones((2, 3)))
    (c,) = m.engine.calls
    assert c["n_comp"] == 2 and c["n"] == 6 and c["free"] is None and len(res["peak"]) == 2
    out = m.moments(cube, v, clip=0.1)
    assert m.engine.calls[-1]["kind"] == "moments" and np.array_equal(m.engine.calls[-1]["dx"], dv)
    assert out["m0"].shape == (2, 3)


def test_public_surface_new_names_only():
    from rajepy_amd import classes
    J, sig = classes.JetModel, lambda f: list(inspect.signature(f).parameters)
    assert sig(E.RTEngine.cube_moments) == ["self", "cube", "x", "dx", "x_ref", "clip", "mask"]
    assert sig(E.RTEngine.specfit) == ["self", "cube", "x", "theta", "x_ref", "weights", "free", "n_comp",
                                       "lambda0", "xtol", "n_iter", "mask", "trace"]
    p = inspect.signature(E.RTEngine.specfit).parameters
    assert [p[k].default for k in ("n_comp", "lambda0", "xtol", "n_iter", "trace")] == [1, 1e-3, 1e-10, 40, False]
    assert sig(E.velocity_axis) == ["freqs", "nu0"]
    assert sig(E.specfit_start) == ["mom", "ipeak", "x", "n_comp"]
    assert sig(E.specfit_results) == ["theta", "cov", "chi2", "nchan", "status", "free", "scale_errors"]
    assert sig(J.moments_rrl) == ["self", "rrl", "freq", "contsub", "formal", "clip_jy"]
    assert sig(J.specfit_rrl) == ["self", "rrl", "freq", "contsub", "formal", "weights", "comps", "theta0",
                                  "free", "n_iter"]
    assert sig(J.moments)[:3] == ["self", "cube", "x"] and sig(J.specfit)[:3] == ["self", "cube", "x"]
    # the pinned parameter lists are as they were
    assert sig(J.clean_image_rrl)[:8] == ["self", "rrl", "u_m", "v_m", "freq", "weights", "shape", "cell_as"]
    assert sig(J.observe_rrl)[:6] == ["self", "rrl", "antennalist", "freq", "t_obs_s", "t_int_s"]
    assert sig(J.dirty_image_ff)[:5] == ["self", "u_m", "v_m", "freq", "weights"]
    assert sig(classes.Pipeline.execute) == ["self", "simobserve", "verbose", "dryrun", "resume", "clobber"] \
        or sig(classes.Pipeline.execute)[:6] == ["self", "simobserve", "verbose", "dryrun", "resume", "clobber"]
    for name in ("clean_image_ff", "clean_image_rrl", "observe_ff", "observe_rrl", "dirty_image_ff"):
        src = inspect.getsource(getattr(J, name))
        assert "specfit" not in src and "moments" not in src
    assert "specfit" not in inspect.getsource(classes.Pipeline.execute)
