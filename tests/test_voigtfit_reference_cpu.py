"""K24 without a device: what tests/test_gpu_voigtfit.py relies on is pinned here first.

The restatement of the device's w(z) (tests/voigtfit_ref.py: w_dev) against mpmath on the census
grid of tools/voigt_w_design.py and its cap; the reference on hand-worked cases; the Jacobian by
Richardson differences; a float64 emulation of the kernel on every GPU case's inputs -- inside the
reference's bounds, converging where the GPU test demands it, every path of the rule reached;
planted mistakes, outside; check_voigtfit from plain C++; the ABI table; `voigt_start` and
`voigt_results` by hand; the Python paths on a recording engine; the public surface.

The module prints the worst measured / bound shares and the noise-free recovery error of the
emulation on the big stack (tests/voigtfit_cases.py: BIG_RECOVERY), which the GPU test asserts at
ten times."""
import ctypes
import inspect
import os
import shutil
import subprocess

import mpmath as mp
import numpy as np
import pytest
import torch

from rajepy_amd import _lib
from rajepy_amd import engine as E
from rajepy_amd import spectra
from tests import voigtfit_cases as C
from tests import voigtfit_ref as R
from tools import voigt_w_design as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_case(case, mistake=None, n_iter=C.N_ITER, pixels=None, stats=None):
    """emulate and follow the case's `follow` pixels -> list of results"""
    out = []
    for p in (case["follow"] if pixels is None else pixels):
        live = case["live"] is None or bool(case["live"][p])
        kw = dict(n_comp=case["n_comp"], w=case["w"], free=case["free"], lambda0=C.LAM0,
                  xtol=case.get("xtol", C.XTOL), n_iter=n_iter)
        res = R.emulate(case["Y"][p], case["x"], case["x_ref"], case["theta0"][p], mistake=mistake,
                        **kw) if live else dict(status=3)
        if live:
            R.follow(res, case["Y"][p], case["x"], case["x_ref"], case["theta0"][p], stats=stats, **kw)
        out.append(res)
    return out


# Every GPU case by name -> (its maker, n_iter).  `run_named` emulates and follows a case ONCE per
# session and keeps the results with the case's own counts, so that every test below stands alone
# (alone, under -k, in any order) and the suite still pays for each case once.
CASES = {"sized %d %d %d %d" % (a[0], int(a[1]), a[2], a[3]): ((lambda a=a: C.sized(*a)), C.N_ITER) for a in C.SIZED}
CASES.update({"ratios": (C.ratios, C.N_ITER), "held g": (lambda: C.held()[0], C.N_ITER),
              "held s": (lambda: C.held()[1], C.N_ITER), "bad": (C.bad_data, C.N_ITER),
              "starts": (C.degenerate_starts, C.N_ITER), "negative g": (C.negative_g_trial, C.N_ITER),
              "narrow": (C.narrow, C.N_ITER), "flat held": (lambda: C.flat(False), C.N_ITER),
              "flat free": (lambda: C.flat(True), C.N_ITER),
              "exhausted": (lambda: C.sized(1, True, 64, 65), 3)})
_DONE = {}


def run_named(name):
    """-> (case, results of its `follow` pixels, its stats)"""
    if name not in _DONE:
        maker, n_iter = CASES[name]
        case, st = maker(), {}
        _DONE[name] = (case, run_case(case, n_iter=n_iter, stats=st), st)
    return _DONE[name]


# ---- w(z) ----------------------------------------------------------------------------------------------
def test_w_restatement_against_mpmath_on_the_census_grid():
    """Every a of the census, every special point (nodes, half-nodes, lattice switches, path
    boundaries, each -+ 1 ulp) and every 12th of the smooth points at 30 digits -- or, with
    RJP_FULL_CENSUS=1 in the environment, all 36350 points at 50 digits as the tool runs them (about
    a minute; worst 9.83e-16): the worst error against the modulus is inside the stated kVoigtWEps /
    2, the stated value is at most 1e-12, and every path is reached."""
    full = os.environ.get("RJP_FULL_CENSUS", "") == "1"
    per_path, per_a, n = D.census(dps=50, thin=1) if full else D.census(dps=30, thin=12)
    print("\nw(z): %d points, worst per path: %s" % (n, ", ".join("%s %.2e" % kv for kv in per_path.items())))
    assert n == 36350 if full else n >= 6000
    assert all(v > 0 for v in per_path.values()), per_path
    assert max(per_path.values()) <= R.EPS_W / 2, per_path
    assert R.EPS_W <= 1e-12
    assert set(per_a) >= {repr(float(a)) for a in (0.0, 1e-300, 1e-12, 1e-6, 1e-3, 0.03, 0.5, 1.0, 10.0, 1e3, 1e6)}


def test_header_states_what_the_restatement_uses():
    src = open(os.path.join(ROOT, "rajepy_amd", "csrc", "voigt_w.h")).read()
    assert "constexpr double kVoigtWEps = %.1e;" % R.EPS_W in src
    rows = [ln.split("X(")[1].split(")")[0].split(",") for ln in src.splitlines() if ln.startswith("  X(")]
    assert len(rows) == 14
    for n, r in enumerate(rows):
        t2i, ei, t2m, em = (float(v) for v in r)
        assert t2i == ((n + 1) / 2.) ** 2 and t2m == ((n + 0.5) / 2.) ** 2
        assert ei == R._EI[n] and em == R._EM[n]
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    assert "|w_dev - w| <= %.1e |w|" % R.EPS_W in hdr


W_U = np.array([0.0, 0.3, 2.0, 5.5, 7.5, 11.9, 12.0, 30.0, -1.25, -500.0])
W_A = (0.0, 1e-3, 0.7, 6.5, 12.0, 40.0)


def test_reference_far_field_against_mpmath():
    """The long-double continued fraction that `w_exact_ld` takes from |z| = 12 on (the GPU reference
    depends on it), against mpmath at 40 digits: 2e-19 of |w|."""
    hit = 0
    for a in W_A:
        K, L = R.w_exact_ld(W_U.astype(R.LD), a)
        with mp.workdps(40):
            for i in range(W_U.size):
                if W_U[i] * W_U[i] + a * a >= 144:
                    z = mp.mpc(float(W_U[i]), a)
                    ex = mp.exp(-z * z) * mp.erfc(mp.mpc(0, -1) * z)
                    got = mp.mpc(R._mpf(K[i]), R._mpf(L[i]))
                    assert abs(got - ex) <= 2e-19 * abs(ex), (W_U[i], a)
                    hit += 1
    assert hit >= 20


def test_w_against_scipy_as_a_cross_check_of_the_mpmath_route():
    wofz = pytest.importorskip("scipy.special").wofz
    for a in W_A:
        K, L = R.w_exact_ld(W_U.astype(R.LD), a)
        w = wofz(W_U + 1j * a)
        assert np.all(np.hypot(K.astype(float) - w.real, L.astype(float) - w.imag) <= 1e-13 * np.abs(w))


# ---- the model by hand ---------------------------------------------------------------------------------
def test_g_zero_is_the_gaussian():
    x = np.linspace(-80, 80, 41)
    F, x0, s = 7.0, 3.0, 11.0
    y = R.profile([F, x0, s, 0.0, 0.0, 0.0], x, 0.0, 1).astype(float)
    want = F / (s * np.sqrt(2 * np.pi)) * np.exp(-(x - x0) ** 2 / (2 * s * s))
    assert np.all(np.abs(y - want) <= 4e-16 * want.max())
    K, _ = R.w_dev((x - x0) / (np.sqrt(2) * s), 0.0)
    assert np.all(np.abs(F * K / (s * np.sqrt(2 * np.pi)) - want) <= 4e-15 * want.max())


def test_small_s_is_the_lorentzian():
    x = np.linspace(-80, 80, 41) + 0.37
    F, g, s = 7.0, 6.0, 1e-6
    y = R.profile([F, 0.0, s, g, 0.0, 0.0], x, 0.0, 1).astype(float)
    want = F * g / (np.pi * (x * x + g * g))
    # the first correction is of relative order 3 s^2 / g^2 = 1e-13
    assert np.all(np.abs(y - want) <= 1e-12 * want)


def test_the_integral_is_F():
    x = np.linspace(-4000, 4000, 8001)
    y = R.profile([5.0, 1.0, 3.0, 2.0, 0.0, 0.0], x, 0.0, 1).astype(float)
    # the Lorentz tails beyond +-X = 4000 hold 2 g / (pi X) of F (and g s^2 / X^3 less: 1e-9)
    got = float(np.sum(y) * (x[1] - x[0]))
    assert abs(got - 5.0 * (1 - 2 * 2.0 / (np.pi * 4000))) < 1e-6


def test_jacobian_by_richardson_differences():
    x = np.array([-35.0, -3.0, 1.0, 2.5, 18.0, 140.0])
    for th in (np.array([5.0, 1.0, 3.0, 2.0, 0.1, 1e-3]), np.array([5.0, 1.0, 8.0, 0.0, 0.0, 0.0]),
               np.array([2.0, -4.0, 0.5, 30.0, 0.0, 0.0])):
        _, J, _, _ = R._ref_channel(th.astype(R.LD), x.astype(R.LD), R.LD(0.5), 1)
        for i in range(6):
            if th[3] == 0.0 and i == 3:
                continue                                    # one-sided at g = 0: not differenced
            h = 1e-3 * max(abs(th[i]), 1.0)
            d = []
            for hh in (h, h / 2):
                tp, tm = th.astype(R.LD), th.astype(R.LD)
                tp[i] += hh
                tm[i] -= hh
                d.append((R.profile(tp, x, 0.5, 1) - R.profile(tm, x, 0.5, 1)) / (2 * R.LD(hh)))
            rich = ((4 * d[1] - d[0]) / 3).astype(float)
            row = J[i].astype(float)
            assert np.all(np.abs(rich - row) <= 1e-9 * np.abs(row).max()), (i, rich, row)


# ---- the emulation on the GPU cases' inputs --------------------------------------------------------------
@pytest.mark.parametrize("n_comp,bl,n_chan,n_pix", C.SIZED)
def test_emulation_inside_the_bounds_sized(n_comp, bl, n_chan, n_pix):
    case, res, _ = run_named("sized %d %d %d %d" % (n_comp, int(bl), n_chan, n_pix))
    if C.must_converge(case):
        # what the GPU test demands of EVERY pixel: converged, at the truth
        for p in range(n_pix):
            r = R.emulate(case["Y"][p], case["x"], case["x_ref"], case["theta0"][p], n_comp, w=case["w"],
                          free=case["free"], lambda0=C.LAM0, xtol=case["xtol"], n_iter=C.N_ITER)
            assert r["status"] == 1, p
            assert C.scaled_error(r["theta"][None], case["truth"][p][None], n_comp) <= 1e-8, p


def test_emulation_on_the_other_cases_reaches_every_path_of_the_rule():
    seen = set()
    ratios, res, _ = run_named("ratios")
    assert all(r["status"] == 1 for r in res)
    err = max(C.scaled_error(r["theta"][None], ratios["truth"][p][None]) for p, r in enumerate(res))
    print("\ng / s from 0 to 20: trials %s, worst |theta - truth| / scale %.2e"
          % ([r["niter"] for r in res], err))
    assert err <= 1e-8 and max(r["niter"] for r in res) <= 12
    traces = list(res)
    for name in ("held g", "held s"):
        case, res, _ = run_named(name)
        assert all(r["status"] == 1 for r in res)
        fixed = [i for i, f in enumerate(case["free"]) if not f]
        for p, r in zip(case["follow"], res):
            assert np.array_equal(r["theta"][fixed], case["theta0"][p][fixed])
            assert C.scaled_error(r["theta"][None], case["truth"][p][None]) <= 1e-8
    bad, res, _ = run_named("bad")
    assert [r["status"] == 3 for r in res] == [p in bad["degenerate"] for p in range(6)]
    _, res, _ = run_named("starts")
    assert [r["status"] for r in res][:5] == [3] * 5 and res[5]["status"] == 1
    _, res, _ = run_named("negative g")
    for r in res:
        tr = r["trace"]
        rejected_negative = (tr[:, 6] < 0) & (tr[:, 2] == 0)
        assert rejected_negative.any(), "no trial with g < 0 was proposed and rejected"
        assert not ((tr[:, 6] < 0) & (tr[:, 2] == 1)).any()
        seen.add("infeasible")
        assert r["status"] in (0, 1) and r["theta"][3] >= 0
    _, res, _ = run_named("narrow")
    print("the line narrower than a channel: status %s, trials %s" % ([r["status"] for r in res],
                                                                      [r["niter"] for r in res]))
    for name in ("flat held", "flat free"):
        _, res, _ = run_named(name)
        assert res[2]["status"] == 1
        seen.update({0: "exhausted", 1: "converged", 2: "stalled"}[r["status"]] for r in res)
        traces += res
    _, first, _ = run_named("exhausted")
    assert all(r["status"] == 0 and r["niter"] == 3 for r in first)
    seen.add("exhausted")
    for r in traces:
        tr = r["trace"]
        if (tr[1:, 2] == 0).any():
            seen.add("reject")
        if (tr[1:, 2] == 1).any():
            seen.add("accept")
    assert {"infeasible", "exhausted", "converged", "accept", "reject"} <= seen, seen


def test_at_most_one_percent_of_the_decisions_go_unjudged():
    """The condition of the trace-following test, over every case of CASES (each emulated and followed
    once per session, here if no test above has done it)."""
    tot = dict(chi=0.0, step=0.0, cov=0.0, decisions=0, unjudged=0)
    for name in CASES:
        st = run_named(name)[2]
        for k in ("chi", "step", "cov"):
            tot[k] = max(tot[k], st.get(k, 0.0))
        for k in ("decisions", "unjudged"):
            tot[k] += st.get(k, 0)
    print("\nworst measured / bound: chi2 %.3f, step %.3f, cov %.3f; %d of %d decisions unjudged"
          % (tot["chi"], tot["step"], tot["cov"], tot["unjudged"], tot["decisions"]))
    assert tot["decisions"] >= 300, tot
    assert tot["unjudged"] <= 0.01 * tot["decisions"], tot


def test_recovery_of_the_big_stack_by_the_emulation():
    """Every 13th of the 130 x 65 noise-free sightlines with g / s in [0.05, 20], from `start_one`:
    all converge; the worst recovery error is what tests/voigtfit_cases.py records as BIG_RECOVERY
    (the GPU test asserts ten times that on every sightline)."""
    case = C.big_stack()
    pick = np.arange(0, case["Y"].shape[0], 13)
    th0 = C.start_one(case["Y"][pick], case["x"])
    worst, iters = 0.0, 0
    for k, p in enumerate(pick):
        r = R.emulate(case["Y"][p], case["x"], 0.0, th0[k], 1, free=case["free"])
        assert r["status"] == 1, (p, r["status"], case["truth"][p])
        worst = max(worst, C.scaled_error(r["theta"][None], case["truth"][p][None]))
        iters = max(iters, r["niter"])
    print("\nbig stack: %d sightlines, up to %d trials, worst |theta - truth| / scale %.3e (recorded %.1e)"
          % (pick.size, iters, worst, C.BIG_RECOVERY))
    assert worst <= C.BIG_RECOVERY


@pytest.mark.parametrize("mistake", ["a_gs", "L_sign", "dropK", "fwhm", "accept_neg_g", "drop_weight"])
def test_planted_mistakes_fall_outside_the_bounds(mistake):
    """a = g / s for g / (sqrt(2) s); L's sign flipped in Rw; the K term dropped from d/ds; the FWHM
    taken for the HWHM; a trial with g < 0 accepted; a dropped weight."""
    if mistake == "accept_neg_g":
        case, pixels = C.negative_g_trial(), [0, 1]
    elif mistake == "drop_weight":
        case, pixels = C.sized(1, True, 64, 65), [0]
        assert case["w"] is not None
    else:
        case, pixels = C.ratios(), [1]
    with pytest.raises(AssertionError):
        run_case(case, mistake=mistake, pixels=pixels, stats={})


# ---- the C side ----------------------------------------------------------------------------------------
def test_check_voigtfit_from_plain_cpp(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "rjp_args_voigtfit_cases"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rajepy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rjp_args_voigtfit_cases.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        case, status, msg = line.split("\t")
        got[case] = (int(status), msg)
    want = {
        "rjp_voigtfit: NULL cube, axis, parameters or outputs":
            ["NULL d_cube", "NULL h_x", "NULL d_theta", "NULL d_chi2", "NULL d_cov", "NULL d_nchan",
             "NULL d_niter", "NULL d_status", "NULL beats sizes"],
        "rjp_voigtfit: n_pix and n_chan must be positive":
            ["n_pix 0", "n_pix -3", "n_chan 0", "sizes beat the limit and n_comp"],
        "rjp_voigtfit: n_chan exceeds RJP_SPECFIT_MAX_CHAN (4096)": ["n_chan 4097", "the limit beats n_comp"],
        "rjp_voigtfit: n_comp must lie in 1 .. RJP_VOIGTFIT_MAX_COMP (2)": ["n_comp 0", "n_comp 3", "n_comp beats x"],
        "rjp_voigtfit: non-finite h_x": ["x nan", "x inf", "x beats x_ref"],
        "rjp_voigtfit: non-finite x_ref": ["x_ref nan", "x_ref -inf", "x_ref beats w"],
        "rjp_voigtfit: negative or non-finite h_w": ["w negative", "w inf", "w nan", "w beats free"],
        "rjp_voigtfit: no free parameter":
            ["no free parameter", "no free parameter among the first six", "free beats lambda0"],
        "rjp_voigtfit: lambda0 and xtol must be finite and positive":
            ["lambda0 0", "lambda0 inf", "lambda0 nan", "xtol -1", "xtol inf", "xtol nan", "lambda0 beats n_iter"],
        "rjp_voigtfit: n_iter < 1": ["n_iter 0", "n_iter beats the workgroups"],
        "rjp_voigtfit: more than 2^31 - 1 workgroups": ["2^31 workgroups"],
    }
    seen = set()
    for msg, cases in want.items():
        for c in cases:
            assert got[c] == (_lib.RJP_ERR_ARG, msg), (c, got[c])
            seen.add(c)
    valid = [c for c in got if c not in seen]
    assert len(valid) == 6 and all(c.startswith("valid") and got[c] == (0, "") for c in valid), valid


def test_abi_signatures():
    P, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    DP, U8 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8)
    assert _lib.SIGNATURES["rjp_voigtfit"] == (i64, [P, P, i64, i32, DP, dbl, DP, P, i32, U8, P, dbl, dbl,
                                                     i32, P, P, P, P, P, P, P])
    assert _lib.SIGNATURES["rjp_voigtfit"] == _lib.SIGNATURES["rjp_specfit"]
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    assert "int64_t rjp_voigtfit(rjp_ctx* ctx, const double* d_cube, int64_t n_pix, int32_t n_chan," in hdr
    assert "#define RJP_VOIGTFIT_MAX_COMP 2" in hdr
    assert "#define RJP_VERSION 117" in hdr                            # symbols added, none changed
    assert spectra.VOIGTFIT_MAX_COMP == E.VOIGTFIT_MAX_COMP == 2
    assert E.voigt_results is spectra.voigt_results and E.voigt_start is spectra.voigt_start
    lib = _lib.load()
    assert lib.rjp_voigtfit(None, None, 1, 1, None, 0.0, None, None, 1, None, None, 1e-3, 1e-10, 1, None,
                            None, None, None, None, None, None) == _lib.RJP_ERR_ARG


# ---- the host helpers by hand --------------------------------------------------------------------------
def test_voigt_start_by_hand():
    x = np.array([0.0, 1.0, 2.0, 4.0, 6.0, 7.0])
    Y = np.array([[0.0, 2.2, 4.0, 2.5, 2.1, 0.0],           # half the peak = 2: channels 1 .. 4 -> hw = 2.5
                  [0.0, 0.0, 0.0, 0.0, 3.0, 0.0],           # one channel: hw = its spacing, (7 - 4) / 2
                  [np.nan] * 6])
    cube = torch.tensor(Y.T.copy())
    mom = torch.tensor([[9.0, 5.0, 0.0], [0.0] * 3, [0.0] * 3, [4.0, 3.0, np.nan]], dtype=torch.float64)
    ipeak = torch.tensor([2, 4, -1], dtype=torch.int32)
    th = E.voigt_start(cube, mom, ipeak, x).numpy()
    assert th.shape == (6, 3)
    assert np.array_equal(th[0, :2], [9.0, 5.0]) and np.array_equal(th[1, :2], [2.0, 6.0])
    assert np.allclose(th[2, :2], [2.5 / 1.1774 / 1.5, 1.5 / 1.1774 / 1.5], rtol=1e-15)
    assert np.array_equal(th[3, :2], [1.25, 0.75])
    assert np.all(np.isnan(th[:4, 2])) and np.all(th[4:] == 0)
    # the host restatement the cases use says the same on a real profile
    case = C.ratios()
    dx = spectra.channel_widths(case["x"])
    Yt = torch.tensor(case["Y"].T.copy())
    momr = torch.stack([(Yt * torch.tensor(dx)[:, None]).sum(0), torch.zeros(8, dtype=torch.float64),
                        torch.zeros(8, dtype=torch.float64), Yt.max(0).values])
    got = E.voigt_start(Yt, momr, Yt.argmax(0).to(torch.int32), case["x"]).numpy().T
    assert np.allclose(got, case["theta0"], rtol=1e-13, atol=0)


def test_erfcx_and_the_width_formula():
    a = np.array([0.0, 1e-3, 0.5, 2.0, 4.999, 5.0, 7.0, 30.0, 1e3])
    got = spectra._erfcx(torch.tensor(a)).numpy()
    want = np.array([float(mp.exp(mp.mpf(v) ** 2) * mp.erfc(mp.mpf(v))) for v in a])
    assert np.all(np.abs(got - want) <= 2e-14 * want), (got - want) / want
    # Olivero and Longbothum against a half-maximum found by bisection on the exact profile: 0.02 %
    for s, g in ((10.0, 0.0), (10.0, 1.0), (10.0, 10.0), (3.0, 30.0), (1.0, 200.0)):
        th = np.array([1.0, 0.0, s, g, 0.0, 0.0])
        prof = lambda v: float(R.profile(th, np.array([v]), 0.0, 1)[0])
        half, lo, hi = 0.5 * prof(0.0), 0.0, 10 * (s + g)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if prof(mid) > half else (lo, mid)
        fG, fL = s * np.sqrt(8 * np.log(2)), 2 * g
        assert abs(0.5346 * fL + np.sqrt(0.2166 * fL * fL + fG * fG) - 2 * lo) <= 2.5e-4 * 2 * lo


def test_voigt_results_by_hand():
    """Pixel 0: F and g free with N_ff = [[4, 1], [1, 2]] (inverse [[2, -1], [-1, 4]] / 7), chi^2 = 6
    over 5 channels: reduced chi^2 = 2.  Pixel 1: status 3.  theta = (3, 1.5, 2, 1, 0.25, 0)."""
    free = [1, 0, 0, 1, 0, 0]
    N = np.eye(6)
    N[0, 0], N[0, 3], N[3, 0], N[3, 3] = 4.0, 1.0, 1.0, 2.0
    pack = np.array([N[i, j] for i, j in R.tri(6)])
    cov = torch.tensor(np.stack([pack, np.full(21, np.nan)], axis=1))
    theta = torch.tensor([[3.0, 9.0], [1.5, 9.0], [2.0, 9.0], [1.0, 9.0], [0.25, 9.0], [0.0, 9.0]],
                         dtype=torch.float64)
    chi2 = torch.tensor([6.0, np.nan], dtype=torch.float64)
    nchan, status = torch.tensor([5, -1], dtype=torch.int32), torch.tensor([1, 3], dtype=torch.int32)
    r = E.voigt_results(theta, cov, chi2, nchan, status, free)
    g = lambda k: float(r[k][0][0]) if isinstance(r[k], list) else float(r[k][0])
    vF, vg, cFg = 2 * 2.0 / 7, 2 * 4.0 / 7, 2 * -1.0 / 7
    assert g("integral") == 3.0 and g("centre") == 1.5 and g("sigma") == 2.0 and g("hwhm_l") == 1.0
    assert g("fwhm_l") == 2.0 and abs(g("fwhm_g") - 2.0 * np.sqrt(8 * np.log(2))) < 1e-15
    assert g("b0") == 0.25 and abs(g("reduced_chi2") - 2.0) < 1e-15 and g("chi2") == 6.0
    a = 1.0 / (np.sqrt(2) * 2.0)
    ex = float(mp.exp(mp.mpf(a) ** 2) * mp.erfc(mp.mpf(a)))
    norm = 1 / (2.0 * np.sqrt(2 * np.pi))
    assert abs(g("peak") - 3.0 * ex * norm) < 1e-15
    assert abs(g("peak") - float(R.profile([3.0, 1.5, 2.0, 1.0, 0, 0], np.array([1.5]), 0.0, 1)[0])) < 1e-15
    fG = 2.0 * np.sqrt(8 * np.log(2))
    root = np.sqrt(0.2166 * 4.0 + fG * fG)
    assert abs(g("fwhm") - (0.5346 * 2.0 + root)) < 1e-14
    assert abs(g("e_integral") - np.sqrt(vF)) < 1e-14 and abs(g("e_hwhm_l") - np.sqrt(vg)) < 1e-14
    assert abs(g("e_fwhm_l") - 2 * np.sqrt(vg)) < 1e-14
    assert g("e_centre") == 0.0 and g("e_sigma") == 0.0 and g("e_fwhm_g") == 0.0 and g("e_b0") == 0.0
    dfdg = 2 * (0.5346 + 0.2166 * 2.0 / root)
    assert abs(g("e_fwhm") - dfdg * np.sqrt(vg)) < 1e-13
    dpF = ex * norm
    dpg = 3.0 * norm * (2 * a * ex - 2 / np.sqrt(np.pi)) / (np.sqrt(2) * 2.0)
    assert abs(g("e_peak") - np.sqrt(dpF * dpF * vF + dpg * dpg * vg + 2 * dpF * dpg * cFg)) < 1e-13
    for k, v in r.items():
        if k in ("nchan", "status"):
            continue
        t = v[0] if isinstance(v, list) else v
        assert np.isnan(float(t[1])), k
    r = E.voigt_results(theta, cov, chi2, nchan, status, free, scale_errors=False)
    assert abs(float(r["e_integral"][0][0]) - np.sqrt(2.0 / 7)) < 1e-14
    with pytest.raises(ValueError):
        E.voigt_results(theta, cov, chi2, nchan, status, [0] * 6)


def test_voigt_results_propagation_with_s_free():
    """F, s and g free with a full 3 x 3 N_ff: e_peak and e_fwhm against gradients taken here by
    central differences of the peak (through mpmath's erfcx) and of the width formula -- the d/ds terms
    of the propagation count (no scaling: the formal errors)."""
    free = [1, 0, 1, 1, 0, 0]
    Nff = np.array([[4.0, 1.0, -0.5], [1.0, 3.0, 0.8], [-0.5, 0.8, 2.0]])
    N = np.eye(6)
    idx = [0, 2, 3]
    for a_, i in enumerate(idx):
        for b_, j in enumerate(idx):
            N[i, j] = Nff[a_, b_]
    cov = torch.tensor(np.array([N[i, j] for i, j in R.tri(6)])[:, None])
    th = np.array([3.0, 1.5, 2.0, 1.3, 0.0, 0.0])
    r = E.voigt_results(torch.tensor(th[:, None]), cov, torch.tensor([6.0], dtype=torch.float64),
                        torch.tensor([9], dtype=torch.int32), torch.tensor([1], dtype=torch.int32), free,
                        scale_errors=False)
    Cff = np.linalg.inv(Nff)

    def peak(F, s, g):
        a = mp.mpf(g) / (mp.sqrt(2) * s)
        return float(F * mp.exp(a * a) * mp.erfc(a) / (s * mp.sqrt(2 * mp.pi)))

    def fwhm(F, s, g):
        fG, fL = s * np.sqrt(8 * np.log(2)), 2 * g
        return 0.5346 * fL + np.sqrt(0.2166 * fL * fL + fG * fG)

    for key, fn in (("peak", peak), ("fwhm", fwhm)):
        grad = []
        with mp.workdps(30):
            for k in range(3):
                h = 1e-5
                up, dn = [th[0], th[2], th[3]], [th[0], th[2], th[3]]
                up[k] += h
                dn[k] -= h
                grad.append((fn(*up) - fn(*dn)) / (2 * h))
        grad = np.array(grad)
        assert abs(grad[1]) > 0.1 * np.abs(grad).max(), (key, grad)       # the d/ds term matters
        want = np.sqrt(grad @ Cff @ grad)
        got = float(r["e_" + key][0][0])
        assert abs(got - want) <= 1e-8 * want, (key, got, want)
        # and the sign of the d/ds term: flipped, the result would differ by far more than 1e-8
        flip = grad * np.array([1.0, -1.0, 1.0])
        assert abs(np.sqrt(flip @ Cff @ flip) - want) > 1e-3 * want
    assert abs(float(r["e_sigma"][0][0]) - np.sqrt(Cff[1, 1])) < 1e-14
    assert abs(float(r["e_fwhm_g"][0][0]) - np.sqrt(8 * np.log(2) * Cff[1, 1])) < 1e-14


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
        self.calls.append(dict(kind="moments", F=F, n=n, x=np.array(x), dx=np.array(dx), x_ref=x_ref))
        mom = torch.stack([torch.full((n,), v, dtype=torch.float64) for v in (2.0, 1.0, 0.5, 3.0)])
        return mom, torch.full((n,), F // 2, dtype=torch.int32), torch.full((n,), F, dtype=torch.int32)

    def voigtfit(self, cube, x, theta, x_ref, weights=None, free=None, n_comp=1, lambda0=1e-3, xtol=1e-10,
                 n_iter=40, mask=None, trace=False):
        assert isinstance(cube, _NoHost) and not trace
        n = cube.numel() // cube.shape[0]
        P = 4 * n_comp + 2
        self.calls.append(dict(kind="voigtfit", n=n, x=np.array(x), theta=theta.clone(), x_ref=x_ref,
                               weights=weights, free=free, n_comp=n_comp, n_iter=n_iter, mask=mask))
        pack = np.array([1.0 if i == j else 0.0 for i, j in R.tri(P)])
        return dict(theta=theta.reshape(P, n).clone(), chi2=torch.ones(n, dtype=torch.float64),
                    cov=torch.from_numpy(np.tile(pack[:, None], (1, n))),
                    nchan=torch.full((n,), cube.shape[0], dtype=torch.int32),
                    niter=torch.ones(n, dtype=torch.int32), status=torch.ones(n, dtype=torch.int32))


def _model(nx, nz):
    from rajepy_amd import classes
    J = classes.JetModel

    class Model:
        voigtfit, voigtfit_rrl = J.voigtfit, J.voigtfit_rrl
        _rrl_velocity_axis = J._rrl_velocity_axis

        def _cube(self, F):
            return (1.0 + torch.arange(F * nx * nz, dtype=torch.float64).reshape(F, -1)).as_subclass(_NoHost)

        def _flux_maps(self, freqs, rrl=None, contsub=True, formal=False):
            self.asked.append(dict(what="flux", rrl=rrl, contsub=contsub, formal=formal, F=len(freqs)))
            return self._cube(len(freqs))

        def _rrl_tau_device(self, rrl, freqs):
            self.asked.append(dict(what="tau", rrl=rrl, F=len(freqs)))
            return self._cube(len(freqs))

    m = Model()
    m.engine, m.nx, m.nz, m.asked = _RecordingEngine(), nx, nz, []
    return m


def test_model_methods_make_one_call_each_and_copy_nothing():
    from rajepy_amd.maths import rrls
    m = _model(3, 4)
    nu0 = rrls.rrl_nu_0("H", 66, 1)
    freqs = nu0 * (1 + np.array([-2e-4, -1e-4, 0.0, 1e-4, 3e-4]))
    v, dv = E.velocity_axis(freqs, nu0)
    res = m.voigtfit_rrl("H66a", freqs, quantity="tau", n_iter=17)
    assert m.asked == [dict(what="tau", rrl="H66a", F=5)]              # no flux is requested
    assert [c["kind"] for c in m.engine.calls] == ["moments", "voigtfit"]
    c = m.engine.calls[1]
    assert list(c["free"]) == [1, 1, 1, 1, 0, 0] and c["n_iter"] == 17 and c["n_comp"] == 1
    assert np.array_equal(c["x"], v) and c["x_ref"] == v[2] and c["weights"] is None
    assert c["theta"].shape == (6, 12) and torch.all(c["theta"][0] == 2.0) and torch.all(c["theta"][1] == v[2])
    assert torch.all(c["theta"][4:] == 0) and torch.all(c["theta"][2] > 0) and torch.all(c["theta"][3] > 0)
    assert res["fwhm"][0].shape == (3, 4) and res["status"].shape == (3, 4) and res["niter"].shape == (3, 4)
    assert float(res["e_b0"][0, 0]) == 0.0
    m.asked.clear()
    m.engine.calls.clear()
    m.voigtfit_rrl("H66a", freqs, formal=True)
    assert m.asked == [dict(what="flux", rrl="H66a", contsub=True, formal=True, F=5)]
    assert list(m.engine.calls[1]["free"]) == [1, 1, 1, 1, 0, 0]
    m.engine.calls.clear()
    m.voigtfit_rrl("H66a", freqs, contsub=False, weights=np.arange(1., 6.))
    assert m.engine.calls[1]["free"] is None and list(m.engine.calls[1]["weights"]) == [1, 2, 3, 4, 5]
    m.engine.calls.clear()
    m.voigtfit_rrl("H66a", freqs, free=[1, 0, 1, 0, 1, 0], theta0=[1., 0., 2., 0., 0., 0.])
    (c,) = m.engine.calls
    assert list(c["free"]) == [1, 0, 1, 0, 1, 0] and c["theta"].shape == (6, 12)
    with pytest.raises(ValueError):
        m.voigtfit_rrl("H66a", freqs, comps=2)
    with pytest.raises(ValueError):
        m.voigtfit_rrl("H66a", freqs, quantity="brightness")
    m.engine.calls.clear()
    cube = torch.ones(5, 2, 3, dtype=torch.float64).as_subclass(_NoHost)
    res = m.voigtfit(cube, v, comps=2, theta0=[1., 0., 2., .5, 9., 1., 3., 0., 0., 0.], mask=np.ones((2, 3)))
    (c,) = m.engine.calls
    assert c["n_comp"] == 2 and c["n"] == 6 and c["free"] is None and len(res["peak"]) == 2


def test_public_surface_new_names_only():
    from rajepy_amd import classes
    J, sig = classes.JetModel, lambda f: list(inspect.signature(f).parameters)
    assert sig(E.RTEngine.voigtfit) == sig(E.RTEngine.specfit)
    p = inspect.signature(E.RTEngine.voigtfit).parameters
    assert [p[k].default for k in ("weights", "free", "n_comp", "lambda0", "xtol", "n_iter", "mask", "trace")] \
        == [None, None, 1, 1e-3, 1e-10, 40, None, False]
    assert sig(E.voigt_start) == ["cube", "mom", "ipeak", "x"]
    assert sig(E.voigt_results) == ["theta", "cov", "chi2", "nchan", "status", "free", "scale_errors"]
    assert sig(J.voigtfit)[:3] == ["self", "cube", "x"]
    assert sig(J.voigtfit_rrl)[:6] == ["self", "rrl", "freq", "quantity", "contsub", "formal"]
    q = inspect.signature(J.voigtfit_rrl).parameters
    assert (q["quantity"].default, q["contsub"].default, q["formal"].default) == ("flux", True, False)
    # the pinned parameter lists of K21 are as they were
    assert sig(E.specfit_start) == ["mom", "ipeak", "x", "n_comp"]
    assert sig(J.specfit_rrl) == ["self", "rrl", "freq", "contsub", "formal", "weights", "comps", "theta0",
                                  "free", "n_iter"]
    assert "voigt" not in inspect.getsource(classes.Pipeline.execute)
