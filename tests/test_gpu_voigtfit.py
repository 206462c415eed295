"""rjp_voigtfit (K24, voigtfit.hip: one Levenberg-Marquardt fit of Voigt profiles plus a baseline per
sightline of a line cube) through the C-ABI, RTEngine and JetModel, against tests/voigtfit_ref.py --
a long-double reference with a 30-digit w(z) that FOLLOWS the device's trace (every bound derived in
its docstring, proportional to kVoigtWEps, none measured) -- on the inputs of
tests/voigtfit_cases.py, which tests/test_voigtfit_reference_cpu.py pins first to a float64
emulation (inside the bounds, converging where convergence is asked here) and to planted mistakes
(outside).

Every raw call runs with guard bands around every buffer, poisoned outputs and the cube 8 bytes off
a 16-byte boundary.  The module prints the worst measured / bound shares."""
import copy
import ctypes

import numpy as np
import pytest

from tests import gpu_util as U
from tests import voigtfit_cases as C
from tests import voigtfit_ref as R

pytestmark = pytest.mark.gpu
YEAR = 31557600.0
STATS = {}
P_F, P_I, P_T = 7.25, -77, float("nan")   # poison of the float outputs, the int outputs, the trace
GUARD = 33                                # elements of guard band on either side (odd: the payload of
                                          # a float64 buffer then starts 8 bytes off a 16-byte line)
KEYS = ("theta", "chi2", "cov", "nchan", "niter", "status", "trace")


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()
    if STATS:
        print("\nworst measured / bound: chi2 %.3f, step %.3f, cov %.3f; %d of %d decisions unjudged"
              % (STATS["chi"], STATS["step"], STATS["cov"], STATS["unjudged"], STATS["decisions"]))


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
            want = np.full(band.shape, self.fill, dtype=h.dtype)
            assert np.array_equal(band, want, equal_nan=h.dtype.kind == "f"), "a guard band was written"
        return h[self.g:self.g + self.n].copy()


def dbl(a):
    return (ctypes.c_double * len(a))(*[float(x) for x in a])


def workgroups(n):
    return (n + 63) // 64


def run_fit(eng, case, n_iter=C.N_ITER, theta0=None, want_trace=True, guard=GUARD):
    """One raw rjp_voigtfit call on a case, every buffer between guard bands -> dict of host arrays
    with the pixel axis first (theta [n, P], chi2, cov [n, T], nchan, niter, status, trace [n, n_iter,
    3 + P])."""
    import torch
    n, Cn = case["Y"].shape
    th0 = np.asarray(case["theta0"] if theta0 is None else theta0, dtype=np.float64)
    th0 = np.broadcast_to(th0, (n, th0.shape[-1]))
    P = th0.shape[1]
    nc, T = (P - 2) // 4, P * (P + 1) // 2
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    cube = np.ascontiguousarray(np.asarray(case["Y"], dtype=np.float64).T)          # [C][n_pix]
    cb = Band(eng, cube.size, f64, -1e300, guard).set(cube)
    mask = Band(eng, n, u8, 0xA5, guard).set(case["live"]) if case["live"] is not None else None
    theta = Band(eng, P * n, f64, P_F, guard).set(np.ascontiguousarray(th0.T))
    chi2, cov = Band(eng, n, f64, P_F, guard), Band(eng, T * n, f64, P_F, guard)
    nchan, niter, status = (Band(eng, n, i32, P_I, guard) for _ in range(3))
    trace = Band(eng, n * n_iter * (3 + P), f64, P_T, guard)
    free = (ctypes.c_uint8 * P)(*[int(x) for x in case["free"]]) if case["free"] is not None else None
    ret = eng.lib.rjp_voigtfit(eng.ctx, cb.ptr, n, Cn, dbl(case["x"]), case["x_ref"],
                               dbl(case["w"]) if case["w"] is not None else None,
                               mask.ptr if mask else None, nc, free, theta.ptr, C.LAM0,
                               case.get("xtol", C.XTOL), n_iter, chi2.ptr, cov.ptr, nchan.ptr, niter.ptr,
                               status.ptr, trace.ptr if want_trace else None, eng._stream())
    eng.synchronize()
    assert ret == workgroups(n), (ret, eng.lib.rjp_last_error(eng.ctx))
    assert cb.get().tobytes() == cube.tobytes(), "the cube was written"
    if mask:
        mask.get()
    return dict(theta=np.ascontiguousarray(theta.get().reshape(P, n).T), chi2=chi2.get(),
                cov=np.ascontiguousarray(cov.get().reshape(T, n).T), nchan=nchan.get(), niter=niter.get(),
                status=status.get(), trace=trace.get().reshape(n, n_iter, 3 + P))


def follow(case, out, pixels=None, n_iter=C.N_ITER, theta0=None, poisoned=True):
    """The reference follows the device's trace of the case's `follow` pixels.  A degenerate pixel
    (status 3) must have left everything but its status as the caller poisoned it."""
    P = out["theta"].shape[1]
    th0 = np.broadcast_to(np.asarray(case["theta0"] if theta0 is None else theta0, dtype=np.float64),
                          out["theta"].shape)
    for p in (case["follow"] if pixels is None else pixels):
        live = case["live"] is None or bool(case["live"][p])
        st = int(out["status"][p])
        if st == 3:
            if poisoned:
                assert np.array_equal(out["theta"][p], th0[p], equal_nan=True)
                assert out["chi2"][p] == P_F and np.all(out["cov"][p] == P_F)
                assert out["nchan"][p] == P_I and out["niter"][p] == P_I
            assert np.isnan(out["trace"][p]).all()
            res = dict(status=3)
        else:
            k = int(out["niter"][p])
            res = dict(theta=out["theta"][p], chi2=out["chi2"][p], cov=R.unpack(out["cov"][p], P),
                       nchan=int(out["nchan"][p]), niter=k, status=st, trace=out["trace"][p][:k])
        if not live:
            assert st == 3
            continue
        R.follow(res, case["Y"][p], case["x"], case["x_ref"], th0[p], n_comp=case["n_comp"], w=case["w"],
                 free=case["free"], lambda0=C.LAM0, xtol=case.get("xtol", C.XTOL), n_iter=n_iter,
                 trace_tail=None if st == 3 else out["trace"][p][int(out["niter"][p]):], stats=STATS)


def same_bits(a, b, keys=KEYS):
    for k in keys:
        x, y = a[k], b[k]
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), \
            "a repeated call changed " + k


# ---- 1: the raw cases ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_comp,bl,n_chan,n_pix", C.SIZED)
def test_sizes_against_the_reference(eng, n_comp, bl, n_chan, n_pix):
    """One and two components, the baseline held and free, P_free (an exactly determined fit) to 257
    channels, 1 to 257 pixels, the three kinds of axis, weights none / per channel / with zeros,
    noise-free and noisy in turn.  Noise-free data on at least 33 channels must be fitted to 1e-8 of
    the scales (the emulation does: test_voigtfit_reference_cpu)."""
    case = C.sized(n_comp, bl, n_chan, n_pix)
    out = run_fit(eng, case)
    follow(case, out)
    assert np.all(out["status"] != 3)
    same_bits(out, run_fit(eng, case))
    same_bits(out, run_fit(eng, case, guard=GUARD + 1))                   # every buffer 8 bytes further on
    if C.must_converge(case):
        err = C.scaled_error(out["theta"], case["truth"], n_comp)
        print("%d comp%s, %d x %d: trials up to %d, worst |theta - truth| / scale %.2e"
              % (n_comp, " + baseline" if bl else "", n_pix, n_chan, out["niter"].max(), err))
        assert np.all(out["status"] == 1) and err <= 1e-8, (np.bincount(out["status"]), err)
        c = run_fit(eng, case, want_trace=False)                          # d_trace = NULL
        assert np.isnan(c["trace"]).all()
        same_bits(out, c, KEYS[:-1])


def test_ratios_from_zero_to_twenty(eng):
    """g / s from exactly 0 to 20, from `voigt_start`'s start: converged within 12 trials to 1e-8 of
    the scales, the trace followed."""
    case = C.ratios()
    out = run_fit(eng, case)
    follow(case, out)
    err = C.scaled_error(out["theta"], case["truth"])
    print("g / s 0 to 20: trials %s, worst |theta - truth| / scale %.2e" % (out["niter"].tolist(), err))
    assert np.all(out["status"] == 1) and out["niter"].max() <= 12 and err <= 1e-8


def test_held_parameters(eng):
    """g held at 0 (a Gaussian fit in area form) and s held at the thermal width: the held parameter
    keeps its bits, its rows of d_cov are the identity's."""
    for case in C.held():
        out = run_fit(eng, case)
        follow(case, out)
        fixed = [i for i, f in enumerate(case["free"]) if not f]
        assert np.all(out["status"] == 1)
        assert np.array_equal(out["theta"][:, fixed], case["theta0"][:, fixed])
        assert C.scaled_error(out["theta"], case["truth"]) <= 1e-8
        N = R.unpack(out["cov"][0], 6)
        for i in fixed:
            assert np.array_equal(N[i], np.eye(6)[i])


@pytest.mark.parametrize("name", ["bad", "starts", "negative g", "narrow", "flat held", "flat free"])
def test_other_cases_against_the_reference(eng, name):
    """NaN / inf channels, an all-NaN, a starved and a masked pixel; starts with s <= 0, g < 0, NaN or
    inf; a trial with g < 0 (rejected); the line narrower than a channel; flat spectra."""
    case = {"bad": C.bad_data, "starts": C.degenerate_starts, "negative g": C.negative_g_trial,
            "narrow": C.narrow, "flat held": lambda: C.flat(False), "flat free": lambda: C.flat(True)}[name]()
    out = run_fit(eng, case)
    follow(case, out)
    same_bits(out, run_fit(eng, case))
    if "degenerate" in case:
        deg = np.zeros(out["status"].size, dtype=bool)
        deg[case["degenerate"]] = True
        assert np.array_equal(out["status"] == 3, deg) and np.all(out["status"][~deg] == 1)
        assert C.scaled_error(out["theta"][~deg], case["truth"][~deg]) <= 1e-8
        # the sound pixels are fitted as if the degenerate ones were not there
        keep = np.nonzero(~deg)[0]
        alone = run_fit(eng, dict(case, Y=case["Y"][keep], theta0=case["theta0"][keep],
                                  live=None if case["live"] is None else case["live"][keep]))
        same_bits({k: out[k][keep] for k in KEYS}, alone)
    if name == "negative g":
        tr = out["trace"]
        for p in range(2):
            rows = tr[p][:out["niter"][p]]
            assert ((rows[:, 6] < 0) & (rows[:, 2] == 0)).any() and not ((rows[:, 6] < 0) & (rows[:, 2] == 1)).any()
        assert np.all(out["theta"][:, 3] >= 0)
    if name.startswith("flat"):
        assert out["status"][2] == 1


def test_exhausted_and_continued(eng):
    case = C.sized(1, True, 64, 65)
    first = run_fit(eng, case, 3)
    follow(case, first, n_iter=3)
    assert np.all(first["status"] == 0) and np.all(first["niter"] == 3)
    second = run_fit(eng, case, theta0=first["theta"])
    follow(case, second, theta0=first["theta"])
    assert np.all(second["status"] == 1) and C.scaled_error(second["theta"], case["truth"]) <= 1e-8


@pytest.mark.parametrize("n_comp,bl", [(1, False), (2, True)])
def test_placement_independence(eng, n_comp, bl):
    """The spectra of a case placed alone (n_pix = 1), across the wave tail and in the last workgroup
    of stacks of 65, 130 and 257 pixels among other spectra and a degenerate neighbour, and permuted:
    the same bits in every output."""
    case = C.sized(n_comp, bl, 34, 70)
    rng = np.random.default_rng(9)
    n = case["Y"].shape[0]
    base = run_fit(eng, case)
    perm = rng.permutation(n)
    out = run_fit(eng, dict(case, Y=case["Y"][perm], theta0=case["theta0"][perm]))
    same_bits({k: base[k][perm] for k in KEYS}, out)
    for p, total, at in ((0, 1, 0), (1, 65, 64), (2, 130, 63), (3, 257, 256), (4, 257, 128)):
        idx = rng.integers(0, n, total)
        idx[at] = p
        th0 = case["theta0"][idx].copy()
        if total > 1:
            th0[(at + 1) % total, 2] = -1.0                                # a degenerate neighbour
        out = run_fit(eng, dict(case, Y=case["Y"][idx], theta0=th0))
        same_bits({k: base[k][p:p + 1] for k in KEYS}, {k: out[k][at:at + 1] for k in KEYS})


def test_the_big_stack_from_voigt_start(eng):
    """130 x 65 noise-free sightlines with random g / s in [0.05, 20]: rjp_cube_moments, `voigt_start`
    on the device, rjp_voigtfit -- every pixel converged, the recovery error within ten times what
    the float64 emulation measures on these inputs (tests/voigtfit_cases.py: BIG_RECOVERY); then
    RTEngine.voigtfit on the same buffers: the same bits."""
    import torch
    from rajepy_amd import engine as E
    from rajepy_amd import spectra
    case = C.big_stack()
    n = case["Y"].shape[0]
    cube = torch.from_numpy(np.ascontiguousarray(case["Y"].T)).to(eng.device)
    mom, ipeak, count = eng.cube_moments(cube, case["x"], spectra.channel_widths(case["x"]), 0.0)
    th0 = E.voigt_start(cube, mom, ipeak, case["x"]).cpu().numpy().T
    pick = np.arange(0, n, 13)
    assert np.allclose(th0[pick], C.start_one(case["Y"][pick], case["x"]), rtol=1e-12, atol=0)
    out = run_fit(eng, dict(case, theta0=th0))
    err = C.scaled_error(out["theta"], case["truth"])
    print("big stack: trials up to %d, worst |theta - truth| / scale %.3e (the emulation's: %.1e)"
          % (out["niter"].max(), err, C.BIG_RECOVERY))
    assert np.all(out["status"] == 1), np.bincount(out["status"])
    assert err <= 10 * C.BIG_RECOVERY, err
    follow(dict(case, theta0=th0), out, pixels=[0, n // 2, n - 1])
    fit = eng.voigtfit(cube, case["x"], torch.from_numpy(np.ascontiguousarray(th0.T)), 0.0,
                       free=case["free"], trace=True)
    assert eng.last_specfit_workgroups == workgroups(n)
    assert fit["theta"].cpu().numpy().T.tobytes() == out["theta"].tobytes()
    assert fit["cov"].cpu().numpy().T.tobytes() == out["cov"].tobytes()
    assert np.array_equal(fit["trace"].cpu().numpy(), out["trace"], equal_nan=True)
    for k in ("chi2", "nchan", "niter", "status"):
        assert fit[k].cpu().numpy().tobytes() == out[k].tobytes(), k


def test_every_refusal_with_its_message(eng):
    import torch
    from rajepy_amd import _lib
    ARG = _lib.RJP_ERR_ARG
    nan, inf = float("nan"), float("inf")
    n, Cn, P = 5, 4, 10
    f64, i32 = torch.float64, torch.int32
    bufs = dict(cube=torch.ones(Cn * n, dtype=f64, device=eng.device),
                theta=torch.full((P * n,), 1.5, dtype=f64, device=eng.device),
                chi2=torch.full((n,), P_F, dtype=f64, device=eng.device),
                cov=torch.full((55 * n,), P_F, dtype=f64, device=eng.device),
                i1=torch.full((n,), P_I, dtype=i32, device=eng.device),
                i2=torch.full((n,), P_I, dtype=i32, device=eng.device),
                i3=torch.full((n,), P_I, dtype=i32, device=eng.device),
                trace=torch.full((n * 2 * (3 + P),), 3.5, dtype=f64, device=eng.device))
    before = {k: t.clone() for k, t in bufs.items()}
    ptr = {k: t.data_ptr() for k, t in bufs.items()}
    many = 64 * (2 ** 31 - 1) + 1

    def fit(a):
        free = (ctypes.c_uint8 * len(a["free"]))(*a["free"]) if a["free"] is not None else None
        return eng.lib.rjp_voigtfit(eng.ctx if a.get("ctx", True) else None, a["cube"], a["n"], a["c"],
                                    dbl(a["x"]) if a["x"] else None, a["x_ref"], dbl(a["w"]) if a["w"] else None,
                                    None, a["nc"], free, a["theta"], a["lam"], a["xtol"], a["n_iter"], a["chi2"],
                                    a["cov"], a["nchan"], a["niter"], a["status"], ptr["trace"], eng._stream())

    gf = dict(cube=ptr["cube"], n=n, c=Cn, x=[3., 1., 2., 0.], x_ref=1.0, w=[1., 0., 2., 1.], nc=2,
              free=[1] * 10, theta=ptr["theta"], lam=1e-3, xtol=1e-10, n_iter=2, chi2=ptr["chi2"],
              cov=ptr["cov"], nchan=ptr["i1"], niter=ptr["i2"], status=ptr["i3"])
    m = dict(nulls="rjp_voigtfit: NULL cube, axis, parameters or outputs",
             sizes="rjp_voigtfit: n_pix and n_chan must be positive",
             chan="rjp_voigtfit: n_chan exceeds RJP_SPECFIT_MAX_CHAN (4096)",
             comp="rjp_voigtfit: n_comp must lie in 1 .. RJP_VOIGTFIT_MAX_COMP (2)",
             x="rjp_voigtfit: non-finite h_x", xref="rjp_voigtfit: non-finite x_ref",
             w="rjp_voigtfit: negative or non-finite h_w", free="rjp_voigtfit: no free parameter",
             tol="rjp_voigtfit: lambda0 and xtol must be finite and positive", iter="rjp_voigtfit: n_iter < 1",
             wgs="rjp_voigtfit: more than 2^31 - 1 workgroups")
    for what, change, msg in [
            ("NULL d_cube", dict(cube=None), m["nulls"]), ("NULL h_x", dict(x=None), m["nulls"]),
            ("NULL d_theta", dict(theta=None), m["nulls"]), ("NULL d_chi2", dict(chi2=None), m["nulls"]),
            ("NULL d_cov", dict(cov=None), m["nulls"]), ("NULL d_nchan", dict(nchan=None), m["nulls"]),
            ("NULL d_niter", dict(niter=None), m["nulls"]), ("NULL d_status", dict(status=None), m["nulls"]),
            ("n_pix 0", dict(n=0), m["sizes"]), ("n_chan -1", dict(c=-1), m["sizes"]),
            ("n_chan 4097", dict(c=4097, x=[1.] * 4097, w=None), m["chan"]),
            ("n_comp 0", dict(nc=0), m["comp"]), ("n_comp 3", dict(nc=3), m["comp"]),
            ("x inf", dict(x=[3., inf, 2., 0.]), m["x"]), ("x_ref inf", dict(x_ref=inf), m["xref"]),
            ("w negative", dict(w=[1., -1., 2., 1.]), m["w"]), ("w nan", dict(w=[1., nan, 2., 1.]), m["w"]),
            ("no free parameter", dict(free=[0] * 10), m["free"]),
            ("lambda0 0", dict(lam=0.0), m["tol"]), ("lambda0 nan", dict(lam=nan), m["tol"]),
            ("xtol -1", dict(xtol=-1.0), m["tol"]), ("xtol inf", dict(xtol=inf), m["tol"]),
            ("n_iter 0", dict(n_iter=0), m["iter"]), ("2^31 workgroups", dict(n=many), m["wgs"]),
            ("NULL beats sizes", dict(cube=None, n=0), m["nulls"]),
            ("sizes beat n_comp", dict(n=0, nc=3), m["sizes"]),
            ("n_comp beats x", dict(nc=3, x=[nan] * 4), m["comp"]),
            ("x beats the weights", dict(x=[nan] * 4, w=[-1.] * 4), m["x"]),
            ("w beats free", dict(w=[-1.] * 4, free=[0] * 10), m["w"]),
            ("free beats lambda0", dict(free=[0] * 10, lam=0.0), m["free"]),
            ("lambda0 beats n_iter", dict(lam=0.0, n_iter=0), m["tol"]),
            ("n_iter beats the workgroups", dict(n_iter=0, n=many), m["iter"])]:
        assert fit(dict(gf, **change)) == ARG, what
        assert eng.lib.rjp_last_error(eng.ctx).decode() == msg, what
    assert fit(dict(gf, ctx=False)) == ARG
    eng.synchronize()
    for k, t in bufs.items():
        assert torch.equal(t, before[k]), "a refusal wrote " + k
    assert fit(dict(gf, w=None, free=None)) == 1                          # the optional pointers may be NULL
    eng.synchronize()


# ---- 2: the widths the model put in --------------------------------------------------------------------
def test_recovers_the_widths_the_model_put_into_a_cell(eng):
    """8 x 1 x 16 cells (n_y = 1: a sightline is one cell, its tau(nu) one exact Voigt profile) with
    log-uniform T (3e3 .. 3e4 K: s from 5 to 16 km/s) and log-uniform n_e (Lorentz HWHM from 1.6 to 50
    km/s), so that g / s spans 0.1 to 10, and a line-of-sight velocity per cell.  rjp_rrl_scan over 64
    channels spanning +-8 max(s, g) of the widest cell; every channel plane divided on the device by
    the cell's 1 - exp(-h nu_c / k T) (kappa_l carries it per channel: a tilt of 1e-3 across the
    band that is no part of a Voigt); `voigtfit` on the velocity axis from `voigt_start`.  Asserted,
    per cell: s against deltanu_g / sqrt(8 ln 2), g against deltanu_l / 2 and x0 against the Doppler
    shift, all from oracle.rt_oracle in km/s, within the first-order effect of K3's stated accuracy
    on the fit, 2 |N^-1 J^T W| (K3_RTOL_WAVE |y|), evaluated by the reference at the solution (the
    factor 2 covers the second order), plus the noise-free recovery error the emulation measures
    (tests/voigtfit_cases.py: BIG_RECOVERY, of the scales)."""
    import torch
    from oracle import rt_oracle as orc
    from rajepy_amd import _lib
    from rajepy_amd import engine as E
    from rajepy_amd.maths import rrls
    from tests import k3_voigt_ref as K3
    lc = rrls.line_constants("H66a")
    el, nn, dn = rrls.rrl_parser("H66a")
    shape = (8, 1, 16)
    rng = np.random.default_rng(2450)
    c_kms = K3.C_LIGHT / 1e3
    temp = np.exp(rng.uniform(np.log(3e3), np.log(3e4), shape))
    g_kms = np.exp(rng.uniform(np.log(1.6), np.log(50.0), shape))
    temp[0, 0, :2], g_kms[0, 0, :2] = [3e4, 3e3], [1.4, 55.0]              # the two ends: g / s 0.09 and 10.8
    ne = 2.0 * g_kms / c_kms * lc["nu_rest"] / lc["kL"]                     # deltanu_l = kL n_e = 2 g
    vy = rng.uniform(-30.0, 40.0, shape)
    one = np.ones(shape)
    z = np.arange(one.size).reshape(shape) % shape[-1]
    g = dict(nd=ne / K3.XI, xi=K3.XI * one, temp=temp, ff=one.copy(), areas=one.copy(), ts=np.zeros(shape),
             vy=vy, rr=np.where(z < shape[-1] // 2, -1.0, 1.0))
    fields = eng.upload_fields(g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"], g["rr"] < 0,
                               vy=g["vy"], csize_au=K3.CSIZE_AU, dtype=8)
    rd = lambda t: t.cpu().numpy().astype(np.float64).reshape(-1)
    nd_d, xi_d, T_d, vy_d = np.abs(rd(fields.nd)), rd(fields.xi), rd(fields.temp), rd(fields.vy)
    # what the model put in, from the oracle, in km/s on the radio velocity axis about nu_rest
    nu0 = lc["nu_rest"] * (1.0 - vy_d * 1e3 / K3.C_LIGHT)
    to_kms = c_kms / lc["nu_rest"]
    s_true = orc.deltanu_g(nu0, T_d, el) / np.sqrt(8.0 * np.log(2.0)) * to_kms
    g_true = orc.deltanu_l(nd_d * xi_d, nn, dn) / 2.0 * to_kms
    x0_true = c_kms * (1.0 - nu0 / lc["nu_rest"])
    ratio = g_true / s_true
    assert ratio.min() <= 0.1 and ratio.max() >= 10.0, (ratio.min(), ratio.max())
    half = 8.0 * max(s_true.max(), g_true.max())
    F = 64
    freqs = lc["nu_rest"] * (1.0 - np.linspace(-half, half, F) / c_kms)
    v, dv = E.velocity_axis(freqs, lc["nu_rest"])
    tau = eng.rrl_scan(fields, None, 0.0, _lib.Line(**lc), list(freqs))   # [F, 128]
    stim = -torch.expm1(-lc["h_over_k"] * torch.from_numpy(freqs).to(eng.device)[:, None] / fields.temp.reshape(1, -1))
    cube = (tau / stim).contiguous()
    x_ref = float(v[F // 2])
    mom, ipeak, _ = eng.cube_moments(cube, v, dv, x_ref)
    free = [1, 1, 1, 1, 0, 0]
    fit = eng.voigtfit(cube, v, E.voigt_start(cube, mom, ipeak, v), x_ref, free=free)
    eng.synchronize()
    status, th = fit["status"].cpu().numpy(), fit["theta"].cpu().numpy().T
    assert np.all(status == 1), np.bincount(status)
    Y = cube.cpu().numpy().T
    worst = 0.0
    for p in range(th.shape[0]):
        bound = 2.0 * R.first_order_shift(th[p], Y[p], v, x_ref, 1, free, U.K3_RTOL_WAVE * np.abs(Y[p]))
        bound = bound + C.BIG_RECOVERY * R.scales(th[p], 1)
        err = np.abs(th[p, 1:4] - [x0_true[p], s_true[p], g_true[p]])
        worst = max(worst, float(np.max(err / bound[1:4])))
        assert np.all(err <= bound[1:4]), (p, ratio[p], err, bound[1:4])
    rel_s, rel_g = np.abs(th[:, 2] / s_true - 1), np.abs(th[:, 3] / g_true - 1)
    print("widths of %d cells, g / s %.3f .. %.2f: worst |s / s_true - 1| %.2e, |g / g_true - 1| %.2e, "
          "|x0 - v_los| %.2e km/s; worst error / bound %.3f; trials up to %d"
          % (th.shape[0], ratio.min(), ratio.max(), rel_s.max(), rel_g.max(),
             np.abs(th[:, 1] - x0_true).max(), worst, int(fit["niter"].max())))


# ---- 3: the example model ------------------------------------------------------------------------------
def _params(tag):
    p = copy.deepcopy(U.load_golden(tag)[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


N_LINE = 48                            # K21's setup: 48 channels 12.3 km/s apart, -282 to 294 km/s
# sum_pixels F against sum_pixels m0 over the converged sightlines of the tau cube.  m0 is the channel
# sum over -282 .. 294 km/s, F the integral over the whole axis: the Lorentz wings beyond the band
# hold about 2 g / (pi X) of a line, and the sightlines that carry the sum (near the base, Lorentz
# HWHM of several hundred km/s) keep most of their area outside it.  The float64 emulation
# (tests/voigtfit_ref.py) fed the device's tau cube gives |sum F - sum m0| / sum m0 = 0.810 on the 338
# sightlines it converges on; twice that is asserted.  A loose check by construction: it catches a
# wrong normalisation of F (sqrt(2 pi), a factor 2), not a percent.
WING_TOL = 2 * 0.810


def test_voigt_fits_of_the_example_model_s_line(eng, tmp_path_factory):
    """`voigtfit_rrl(quantity="tau")` and `quantity="flux"` of the golden example model on K21's 48
    channels: on either cube the trace followed, status 3 exactly on the cube's empty sightlines, the
    same bits as RTEngine.voigtfit on the same cube; the median Doppler and Lorentz widths printed beside
    K21's Gaussian FWHM and the thermal width (multi-cell sightlines with velocity structure are not
    one Voigt: no width is asserted); sum F against sum m0; the reduced chi^2 below the Gaussian
    fit's on every converged sightline of the tau cube."""
    import torch
    from rajepy_amd import classes, logger
    from rajepy_amd import engine as E
    from rajepy_amd.maths import rrls
    log = logger.Log(str(tmp_path_factory.mktemp("voigtfit") / "model.log"), verbose=False)
    jm = classes.JetModel(_params("cfg1_example"), log=log, engine=eng)
    jm.time = 1.0 * YEAR
    rrl = U.load_golden("cfg1_example")[1]["rrl"]
    nu0 = rrls.rrl_nu_0(*rrls.rrl_parser(rrl))
    freqs = nu0 * (1.0 - np.linspace(-282.0, 294.0, N_LINE) * 1e3 / 299792458.0)
    v, dv = E.velocity_axis(freqs, nu0)
    x_ref = float(v[N_LINE // 2])
    free = [1, 1, 1, 1, 0, 0]

    def through_the_engine(cube, res):
        """`voigtfit_rrl`'s maps against RTEngine.voigtfit with a trace on the same cube: the same
        bits, status 3 exactly on the cube's own empty sightlines, six live traces followed."""
        Y = np.ascontiguousarray(cube.cpu().numpy().T)
        m_d, ip_d, _ = eng.cube_moments(cube, v, dv, x_ref)
        th0 = E.voigt_start(cube, m_d, ip_d, v)
        fit = eng.voigtfit(cube, v, th0, x_ref, free=free, trace=True)
        status = fit["status"].cpu().numpy()
        assert np.array_equal(res["status"].cpu().numpy().reshape(-1), status)
        assert np.array_equal(res["niter"].cpu().numpy().reshape(-1), fit["niter"].cpu().numpy())
        live = status != 3
        for key, row in (("integral", 0), ("centre", 1), ("sigma", 2), ("hwhm_l", 3)):
            a, b = res[key][0].cpu().numpy().reshape(-1), fit["theta"][row].cpu().numpy()
            assert a[live].tobytes() == b[live].tobytes() and np.all(np.isnan(a[~live])), key
        a, b = res["chi2"].cpu().numpy().reshape(-1), fit["chi2"].cpu().numpy()
        assert a[live].tobytes() == b[live].tobytes()
        empty = ~np.any(np.isfinite(Y) & (Y != 0.0), axis=1)
        assert np.array_equal(status == 3, empty), (int((status == 3).sum()), int(empty.sum()))
        assert 0 < empty.sum() < Y.shape[0]
        out = dict(theta=fit["theta"].cpu().numpy().T, chi2=fit["chi2"].cpu().numpy(),
                   cov=fit["cov"].cpu().numpy().T, nchan=fit["nchan"].cpu().numpy(),
                   niter=fit["niter"].cpu().numpy(), status=status, trace=fit["trace"].cpu().numpy())
        pick = np.nonzero(live)[0]
        pick = pick[::max(1, pick.size // 6)][:6]
        case = dict(Y=Y, x=v, x_ref=x_ref, w=None, live=None, free=free, theta0=th0.cpu().numpy().T, n_comp=1)
        follow(case, out, pixels=list(pick), poisoned=False)
        return out, status, live, m_d

    res = jm.voigtfit_rrl(rrl, freqs, quantity="tau")
    tau = jm._rrl_tau_device(rrl, freqs).reshape(N_LINE, -1)
    out, status, live, m_d = through_the_engine(tau, res)
    n = status.size
    conv = status == 1
    # K21's Gaussian fit of the same cube, the same baseline held
    gm, gip, _ = eng.cube_moments(tau, v, dv, x_ref)
    gfit = eng.specfit(tau, v, E.specfit_start(gm, gip, v), x_ref, free=[1, 1, 1, 0, 0])
    gres = E.specfit_results(gfit["theta"], gfit["cov"], gfit["chi2"], gfit["nchan"], gfit["status"],
                             [1, 1, 1, 0, 0])
    gconv = gfit["status"].cpu().numpy() == 1
    red_v = res["reduced_chi2"].cpu().numpy().reshape(-1)
    red_g = gres["reduced_chi2"].cpu().numpy()
    el = rrls.rrl_parser(rrl)[0]
    thermal = rrls.deltanu_g(nu0, jm.params["properties"]["T_0"], el) / nu0 * 299792.458
    fg = res["fwhm_g"][0].cpu().numpy().reshape(-1)
    fl = res["fwhm_l"][0].cpu().numpy().reshape(-1)
    ft = res["fwhm"][0].cpu().numpy().reshape(-1)
    print("line %s, tau cube: %d of %d sightlines fitted (status 1: %d, 0: %d, 2: %d); medians over the "
          "converged: fwhm_g %.2f km/s, fwhm_l %.2f km/s, Voigt fwhm %.2f km/s; the Gaussian fit's FWHM %.2f "
          "km/s; thermal FWHM at T_0 %.2f km/s"
          % (rrl, int(live.sum()), n, int(conv.sum()), int((status == 0).sum()), int((status == 2).sum()),
             float(np.median(fg[conv])), float(np.median(fl[conv])), float(np.median(ft[conv])),
             float(np.median(gres["fwhm"][0].cpu().numpy()[gconv])), thermal))
    # on EVERY converged sightline of the tau cube (the Gaussian fit's chi^2 where it stands, converged
    # or not: it has a spectrum there, the same one)
    assert conv.sum() > 0 and np.all(gfit["status"].cpu().numpy()[conv] != 3)
    worse = conv & ~(red_v < red_g)
    print("reduced chi^2: Voigt below Gaussian on %d of %d converged sightlines (the Gaussian fit converged "
          "on %d of them); median ratio %.3e"
          % (int((conv & (red_v < red_g)).sum()), int(conv.sum()), int((conv & gconv).sum()),
             float(np.median(red_v[conv] / red_g[conv]))))
    assert not worse.any(), (int(worse.sum()), red_v[worse][:5], red_g[worse][:5])
    m0 = m_d[0].cpu().numpy()
    sF, sm = float(np.sum(out["theta"][conv, 0])), float(np.sum(m0[conv]))
    print("sum F %.6e, sum m0 %.6e over the converged sightlines: |difference| / sum m0 = %.4f (asserted <= %.3f)"
          % (sF, sm, abs(sF - sm) / sm, WING_TOL))
    assert abs(sF - sm) <= WING_TOL * sm
    # the flux cube through the model, held in the same way: its own empty sightlines, the same bits as
    # RTEngine.voigtfit on the very cube, the trace followed
    resf = jm.voigtfit_rrl(rrl, freqs, quantity="flux")
    flux = jm._flux_maps(freqs, rrl=rrl, contsub=True, formal=False).reshape(N_LINE, -1)
    _, stf, _, _ = through_the_engine(flux, resf)
    ok = stf == 1
    print("flux cube: status 1: %d, 0: %d, 2: %d, 3: %d; medians fwhm_g %.2f, fwhm_l %.2f km/s"
          % (int(ok.sum()), int((stf == 0).sum()), int((stf == 2).sum()), int((stf == 3).sum()),
             float(np.median(resf["fwhm_g"][0].cpu().numpy().reshape(-1)[ok])),
             float(np.median(resf["fwhm_l"][0].cpu().numpy().reshape(-1)[ok]))))
    assert ok.sum() > 0
