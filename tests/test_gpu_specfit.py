"""rjp_cube_moments and rjp_specfit (K21, specfit.hip: moment maps and one Levenberg-Marquardt fit
of Gaussians plus a baseline per sightline of a line cube) through the C-ABI, RTEngine and
JetModel, against tests/specfit_ref.py -- a long-double NumPy reference that judges the moments per
pixel and FOLLOWS the device's trace of every fit (checks (a)-(e) of its docstring, every bound
derived there, none measured), which tests/test_specfit_reference_cpu.py pins to hand-worked cases,
to a float64 emulation on these very inputs (tests/specfit_cases.py: inside the bounds, and
converging where convergence is asked here) and to planted mistakes (outside).

Every raw call runs with guard bands around every buffer and poisoned outputs.  The 1e-9 on the
noise-free fits is a sanity cap, not the accuracy judgement: that is the trace.  The module prints
the worst error / bound per group."""
import copy
import ctypes
import os

import numpy as np
import pytest

from tests import gpu_util as U
from tests import specfit_cases as C
from tests import specfit_ref as K

pytestmark = pytest.mark.gpu
YEAR = 31557600.0
WORST = {}
P_F, P_I, P_T = 7.25, -77, -7.5        # poison of the float outputs, the int outputs, the trace
GUARD = 33                             # elements of guard band on either side (odd: the payload of
                                       # a float64 buffer then starts 8 bytes off a 16-byte line)
LAM0, XTOL, N_ITER = C.LAM0, C.XTOL, C.N_ITER
FIXTURE = os.path.join(U.GOLDEN, "antenna_configs", "vla.a.cfg")
KEYS = ("theta", "chi2", "cov", "nchan", "niter", "status", "trace")
MKEYS = ("m0", "m1", "m2", "peak", "ipeak", "count")


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()
    print("\nworst error / bound per group: " +
          ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    print("worst share per check: " + ", ".join("%s %.3f" % kv for kv in sorted(K.PARTS.items())))


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


def dbl(a):
    return (ctypes.c_double * len(a))(*[float(x) for x in a])


def cube_band(eng, Y, guard):
    import torch
    cube = np.ascontiguousarray(np.asarray(Y, dtype=np.float64).T)          # [C][n_pix]
    return cube, Band(eng, cube.size, torch.float64, -1e300, guard).set(cube)


def run_moments(eng, case, guard=GUARD, ints=True):
    """One raw rjp_cube_moments call on a case, every buffer between guard bands -> dict of host
    arrays [n_pix] (m0, m1, m2, peak, ipeak, count)."""
    import torch
    n, Cn = case["Y"].shape
    cube, cb = cube_band(eng, case["Y"], guard)
    mask = Band(eng, n, torch.uint8, 0xA5, guard).set(case["live"]) if case["live"] is not None else None
    mom = Band(eng, 4 * n, torch.float64, P_F, guard)
    ipeak, count = Band(eng, n, torch.int32, P_I, guard), Band(eng, n, torch.int32, P_I, guard)
    ret = eng.lib.rjp_cube_moments(eng.ctx, cb.ptr, n, Cn, dbl(case["x"]), dbl(case["dx"]), case["x_ref"],
                                   case["clip"], mask.ptr if mask else None, mom.ptr,
                                   ipeak.ptr if ints else None, count.ptr if ints else None, eng._stream())
    eng.synchronize()
    assert ret == K.workgroups(n), (ret, eng.lib.rjp_last_error(eng.ctx))
    assert cb.get().tobytes() == cube.tobytes(), "the cube was written"
    if mask:
        mask.get()
    m = mom.get().reshape(4, n)
    return dict(m0=m[0], m1=m[1], m2=m[2], peak=m[3], ipeak=ipeak.get(), count=count.get())


def judge_moments(kind, case, out):
    for p in range(case["Y"].shape[0]):
        live = True if case["live"] is None else bool(case["live"][p])
        note(kind, K.check_moments(case["Y"][p], case["x"], case["dx"], case["x_ref"], case["clip"], live,
                                   {k: out[k][p] for k in MKEYS}))


def run_fit(eng, case, n_iter=N_ITER, theta0=None, lambda0=LAM0, xtol=XTOL, want_trace=True, guard=GUARD):
    """One raw rjp_specfit call on a case of tests/specfit_cases.py, every buffer between guard
    bands -> dict of host arrays with the pixel axis first (theta [n, P], chi2, cov [n, T], nchan,
    niter, status, trace [n, n_iter, 3 + P], ret)."""
    import torch
    n, Cn = case["Y"].shape
    th0 = np.asarray(case["theta0"] if theta0 is None else theta0, dtype=np.float64)
    th0 = np.broadcast_to(th0, (n, th0.shape[-1]))
    P = th0.shape[1]
    nc, T = (P - 2) // 3, P * (P + 1) // 2
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    cube, cb = cube_band(eng, case["Y"], guard)
    mask = Band(eng, n, u8, 0xA5, guard).set(case["live"]) if case["live"] is not None else None
    theta = Band(eng, P * n, f64, P_F, guard).set(np.ascontiguousarray(th0.T))
    chi2, cov = Band(eng, n, f64, P_F, guard), Band(eng, T * n, f64, P_F, guard)
    nchan, niter, status = (Band(eng, n, i32, P_I, guard) for _ in range(3))
    trace = Band(eng, n * n_iter * (3 + P), f64, P_T, guard)
    free = (ctypes.c_uint8 * P)(*[int(x) for x in case["free"]]) if case["free"] is not None else None
    ret = eng.lib.rjp_specfit(eng.ctx, cb.ptr, n, Cn, dbl(case["x"]), case["x_ref"],
                              dbl(case["w"]) if case["w"] is not None else None,
                              mask.ptr if mask else None, nc, free, theta.ptr, lambda0, xtol, n_iter,
                              chi2.ptr, cov.ptr, nchan.ptr, niter.ptr, status.ptr,
                              trace.ptr if want_trace else None, eng._stream())
    eng.synchronize()
    assert ret == K.workgroups(n), (ret, eng.lib.rjp_last_error(eng.ctx))
    assert cb.get().tobytes() == cube.tobytes(), "the cube was written"
    if mask:
        mask.get()
    return dict(theta=np.ascontiguousarray(theta.get().reshape(P, n).T), chi2=chi2.get(),
                cov=np.ascontiguousarray(cov.get().reshape(T, n).T), nchan=nchan.get(), niter=niter.get(),
                status=status.get(), trace=trace.get().reshape(n, n_iter, 3 + P), ret=ret)


def follow_all(kind, case, out, n_iter=N_ITER, theta0=None, pick=None):
    th0 = np.asarray(case["theta0"] if theta0 is None else theta0, dtype=np.float64)
    th0 = np.broadcast_to(th0, out["theta"].shape)
    Y, live = case["Y"], case["live"]
    if pick is not None:
        Y, th0 = Y[pick], th0[pick]
        live = live[pick] if live is not None else None
        out = {k: out[k][pick] for k in KEYS}
    assert Y.shape[0] <= 600
    note(kind, K.follow_all(Y, case["x"], case["w"], case["x_ref"], th0, case["free"], LAM0, XTOL, n_iter,
                            out, P_T, P_F, P_I, live))


def same_bits(a, b, keys=KEYS):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), "a repeated call changed " + k


# ---- 1: the moments ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pix,n_chan", C.MOMENT_SIZES)
def test_moments_against_the_reference(eng, n_pix, n_chan):
    """1 to 257 pixels (every tail of a wave, five workgroups) of 1 to 257 channels on uniform,
    descending and non-uniform axes, NaN / inf channels, an all-NaN and a masked pixel, a clip; the
    cube 8 bytes off a 16-byte boundary and, with an odd n_pix, every other plane so."""
    case = C.moment_case(n_pix, n_chan)
    out = run_moments(eng, case)
    judge_moments("moments", case, out)
    same_bits(out, run_moments(eng, case), MKEYS)
    same_bits(out, run_moments(eng, case, guard=GUARD + 1), MKEYS)
    no_ints = run_moments(eng, case, ints=False)                          # d_ipeak = d_count = NULL
    same_bits(out, no_ints, MKEYS[:4])
    assert np.all(no_ints["ipeak"] == P_I) and np.all(no_ints["count"] == P_I)


def test_moments_special_cases(eng):
    """+0.0 and the NaN pattern, ipeak = -1, the lowest channel on a tie, clip exactly at a value,
    an exact m0 = 0, s2 / m0 < 0, a masked pixel."""
    case = C.moment_special()
    out = run_moments(eng, case)
    judge_moments("moments", case, out)
    assert list(out["ipeak"]) == [1, 3, -1, -1, 2, -1, -1] and list(out["count"]) == [6, 3, 2, 0, 3, 0, 0]
    for p in (2, 3, 5, 6):
        assert out["m0"][p] == 0.0 and not np.signbit(out["m0"][p])
        assert np.isnan(out["m1"][p]) and np.isnan(out["m2"][p]) and np.isnan(out["peak"][p])
    assert out["peak"][0] == 2.0 and out["peak"][1] == 3.0
    assert out["m0"][4] == 1.0 and out["m1"][4] == 1.0 and np.isnan(out["m2"][4])


# ---- 2: the fit, at the bounds --------------------------------------------------------------------
@pytest.mark.parametrize("n_comp,bl,n_chan", C.SIZED)
def test_sizes_against_the_reference(eng, n_comp, bl, n_chan):
    """One and two components, the baseline held and free, P_free (an exactly determined fit) to 257
    channels, 1 to 257 pixels, the three kinds of axis, weights none / per channel / with zeros,
    noise-free and noisy in turn (tests/specfit_cases.py).  From 64 channels on the noise-free data
    must be fitted to 1e-9 of the scales (the emulation does: test_specfit_reference_cpu)."""
    kind = "%d comp%s" % (n_comp, " + baseline" if bl else "")
    case = C.sized(n_comp, bl, n_chan)
    out = run_fit(eng, case)
    follow_all(kind, case, out)
    assert np.all(out["status"] != 3)
    same_bits(out, run_fit(eng, case))
    if C.must_converge(case):
        err = C.scaled_error(out["theta"], case["truth"])
        print("%s, %d x %d: iterations up to %d, worst |theta - truth| / s %.2e"
              % (kind, case["Y"].shape[0], n_chan, out["niter"].max(), err))
        assert np.all(out["status"] == 1) and err <= 1e-9, (np.bincount(out["status"]), err)
        same_bits(out, run_fit(eng, case, guard=GUARD + 1))               # every buffer 8 bytes further on
        c = run_fit(eng, case, want_trace=False)                          # d_trace = NULL
        assert np.all(c["trace"] == P_T)
        same_bits(out, c, KEYS[:-1])


@pytest.mark.parametrize("name", ["bad 1", "bad 2", "starts", "narrow", "flat held", "flat free", "held"])
def test_other_cases_against_the_reference(eng, name):
    """NaN / inf channels, an all-NaN pixel, too few counted channels, a masked pixel; starts with
    s <= 0 or NaN; a line narrower than a channel; flat spectra (a stall, singular pivots); a mixed
    pattern of held parameters."""
    case = {"bad 1": lambda: C.bad_data(1), "bad 2": lambda: C.bad_data(2), "starts": C.degenerate_starts,
            "narrow": C.narrow, "flat held": lambda: C.flat(False), "flat free": lambda: C.flat(True),
            "held": C.held}[name]()
    out = run_fit(eng, case)
    follow_all(name.split()[0], case, out)
    same_bits(out, run_fit(eng, case))
    if "degenerate" in case:
        deg = np.zeros(out["status"].size, dtype=bool)
        deg[case["degenerate"]] = True
        assert np.array_equal(out["status"] == 3, deg) and np.all(out["status"][~deg] == 1)
        assert C.scaled_error(out["theta"][~deg], case["truth"][~deg]) <= 1e-9
        # n_comp = 1 or 2: the sound pixels are fitted as if the degenerate ones were not there
        keep = np.nonzero(~deg)[0]
        alone = run_fit(eng, dict(case, Y=case["Y"][keep], theta0=case["theta0"][keep],
                                  live=None if case["live"] is None else case["live"][keep]))
        for k in KEYS:
            assert alone[k].tobytes() == out[k][keep].tobytes(), k
    if name.startswith("flat"):
        assert out["status"][4] == 2 and out["status"][3] == 1
    if name == "held":
        assert np.all(out["status"] == 1) and C.scaled_error(out["theta"], case["truth"]) <= 1e-9
        assert np.array_equal(out["theta"][:, [1, 4]], case["theta0"][:, [1, 4]])
        N = K.unpack(out["cov"][0], 5)
        assert np.array_equal(N[1], np.eye(5)[1]) and np.array_equal(N[4], np.eye(5)[4])


def test_exhausted_and_continued(eng):
    case = C.sized(1, True, 64)
    first = run_fit(eng, case, 3)
    follow_all("exhausted", case, first, 3)
    assert np.all(first["status"] == 0) and np.all(first["niter"] == 3)
    second = run_fit(eng, case, theta0=first["theta"])
    follow_all("continued", case, second, theta0=first["theta"])
    assert np.all(second["status"] == 1) and C.scaled_error(second["theta"], case["truth"]) <= 1e-9


def test_the_big_stack_from_the_moments(eng):
    """130 x 65 noise-free sightlines of 40 channels: rjp_cube_moments, `specfit_start` on the
    device, rjp_specfit -- every pixel converged and within 1e-9 of the truth; every 15th pixel
    followed by the reference."""
    import torch
    from rajepy_amd import engine as E
    case = C.big()
    n = case["Y"].shape[0]
    cube = torch.from_numpy(np.ascontiguousarray(case["Y"].T)).to(eng.device)
    mom, ipeak, count = eng.cube_moments(cube, case["x"], C.channel_widths(case["x"]), case["x_ref"])
    assert eng.last_specfit_workgroups == K.workgroups(n) and int(count.min()) == 40
    th0 = E.specfit_start(mom, ipeak, case["x"]).cpu().numpy().T
    out = run_fit(eng, case, theta0=th0)
    err = C.scaled_error(out["theta"], case["truth"])
    print("big stack: iterations up to %d, worst |theta - truth| / s %.2e" % (out["niter"].max(), err))
    assert np.all(out["status"] == 1), np.bincount(out["status"])
    assert err <= 1e-9, err
    follow_all("big", case, out, theta0=th0, pick=np.arange(0, n, 15))
    # RTEngine.specfit on the same buffers: the same bits, pixel planes
    fit = eng.specfit(cube, case["x"], torch.from_numpy(np.ascontiguousarray(th0.T)), case["x_ref"],
                      free=case["free"], trace=True)
    assert fit["theta"].cpu().numpy().T.tobytes() == out["theta"].tobytes()
    assert fit["cov"].cpu().numpy().T.tobytes() == out["cov"].tobytes()
    tr = fit["trace"].cpu().numpy()
    live = np.arange(N_ITER)[None, :] < out["niter"][:, None]
    assert np.array_equal(tr[live], out["trace"][live]) and np.all(np.isnan(tr[~live]))
    for k in ("chi2", "nchan", "niter", "status"):
        assert fit[k].cpu().numpy().tobytes() == out[k].tobytes(), k


# ---- 3: placement independence -----------------------------------------------------------------------
@pytest.mark.parametrize("n_comp,bl", [(1, False), (1, True), (2, True)])
def test_placement_independence(eng, n_comp, bl):
    """The spectra of a case placed alone (n_pix = 1), at the start, across the wave tail and in
    the last workgroup of stacks of 65, 130 and 257 pixels among other spectra, and permuted: the
    same bits in every output of the fit and of the moments."""
    case = C.sized(n_comp, bl, 64)
    rng = np.random.default_rng(9)
    n = case["Y"].shape[0]
    base = run_fit(eng, case)
    mcase = dict(case, dx=C.channel_widths(case["x"]), clip=0.0)
    mbase = run_moments(eng, mcase)
    perm = rng.permutation(n)
    out = run_fit(eng, dict(case, Y=case["Y"][perm], theta0=case["theta0"][perm]))
    for k in KEYS:
        assert out[k].tobytes() == base[k][perm].tobytes(), "a permutation changed " + k
    mout = run_moments(eng, dict(mcase, Y=case["Y"][perm]))
    for k in MKEYS:
        assert mout[k].tobytes() == mbase[k][perm].tobytes(), "a permutation changed " + k
    for p, total, at in ((0, 1, 0), (1, 65, 64), (2, 130, 63), (3, 257, 256), (4, 257, 128)):
        p = p % n
        idx = rng.integers(0, n, total)
        idx[at] = p
        th0 = case["theta0"][idx].copy()
        if total > 1:
            th0[(at + 1) % total, 2] = -1.0                                # a degenerate neighbour
        out = run_fit(eng, dict(case, Y=case["Y"][idx], theta0=th0))
        for k in KEYS:
            assert out[k][at].tobytes() == base[k][p].tobytes(), (k, total, at)
        mout = run_moments(eng, dict(mcase, Y=case["Y"][idx]))
        for k in MKEYS:
            assert mout[k][at].tobytes() == mbase[k][p].tobytes(), (k, total, at)


# ---- 4: refusals ---------------------------------------------------------------------------------------
def test_every_refusal_with_its_message(eng):
    import torch
    from rajepy_amd import _lib
    ARG = _lib.RJP_ERR_ARG
    nan, inf = float("nan"), float("inf")
    n, Cn, P = 5, 4, 8
    f64, i32 = torch.float64, torch.int32
    bufs = dict(cube=torch.ones(Cn * n, dtype=f64, device=eng.device),
                theta=torch.full((P * n,), 1.5, dtype=f64, device=eng.device),
                mom=torch.full((4 * n,), P_F, dtype=f64, device=eng.device),
                chi2=torch.full((n,), P_F, dtype=f64, device=eng.device),
                cov=torch.full((36 * n,), P_F, dtype=f64, device=eng.device),
                i1=torch.full((n,), P_I, dtype=i32, device=eng.device),
                i2=torch.full((n,), P_I, dtype=i32, device=eng.device),
                i3=torch.full((n,), P_I, dtype=i32, device=eng.device),
                trace=torch.full((n * 2 * (3 + P),), P_T, dtype=f64, device=eng.device))
    before = {k: t.clone() for k, t in bufs.items()}
    ptr = {k: t.data_ptr() for k, t in bufs.items()}
    many = 64 * (2 ** 31 - 1) + 1

    def mom(a):
        return eng.lib.rjp_cube_moments(eng.ctx if a.get("ctx", True) else None, a["cube"], a["n"], a["c"],
                                        dbl(a["x"]) if a["x"] else None, dbl(a["dx"]) if a["dx"] else None,
                                        a["x_ref"], a["clip"], None, a["mom"], ptr["i1"], ptr["i2"],
                                        eng._stream())

    gm = dict(cube=ptr["cube"], n=n, c=Cn, x=[3., 1., 2., 0.], dx=[1., 0., 2., 1.], x_ref=1.0, clip=0.0,
              mom=ptr["mom"])
    m = K.MSG_M
    for what, change, msg in [
            ("NULL d_cube", dict(cube=None), m["nulls"]), ("NULL h_x", dict(x=None), m["nulls"]),
            ("NULL h_dx", dict(dx=None), m["nulls"]), ("NULL d_mom", dict(mom=None), m["nulls"]),
            ("n_pix 0", dict(n=0), m["sizes"]), ("n_chan 0", dict(c=0), m["sizes"]),
            ("n_chan 4097", dict(c=4097, x=[1.] * 4097, dx=[1.] * 4097), m["chan"]),
            ("x nan", dict(x=[3., nan, 2., 0.]), m["x"]), ("dx negative", dict(dx=[1., -1., 2., 1.]), m["dx"]),
            ("dx inf", dict(dx=[1., inf, 2., 1.]), m["dx"]), ("x_ref nan", dict(x_ref=nan), m["xref"]),
            ("clip negative", dict(clip=-1.0), m["clip"]), ("clip nan", dict(clip=nan), m["clip"]),
            ("2^31 workgroups", dict(n=many), m["wgs"]),
            ("NULL beats sizes", dict(cube=None, n=0), m["nulls"]),
            ("x beats dx", dict(x=[nan] * 4, dx=[-1.] * 4), m["x"]),
            ("clip beats the workgroups", dict(clip=-1.0, n=many), m["clip"])]:
        assert mom(dict(gm, **change)) == ARG, what
        assert eng.lib.rjp_last_error(eng.ctx).decode() == msg, what
    assert mom(dict(gm, ctx=False)) == ARG

    def fit(a):
        free = (ctypes.c_uint8 * len(a["free"]))(*a["free"]) if a["free"] is not None else None
        return eng.lib.rjp_specfit(eng.ctx if a.get("ctx", True) else None, a["cube"], a["n"], a["c"],
                                   dbl(a["x"]) if a["x"] else None, a["x_ref"], dbl(a["w"]) if a["w"] else None,
                                   None, a["nc"], free, a["theta"], a["lam"], a["xtol"], a["n_iter"], a["chi2"],
                                   a["cov"], a["nchan"], a["niter"], a["status"], ptr["trace"], eng._stream())

    gf = dict(cube=ptr["cube"], n=n, c=Cn, x=[3., 1., 2., 0.], x_ref=1.0, w=[1., 0., 2., 1.], nc=2,
              free=[1] * 8, theta=ptr["theta"], lam=1e-3, xtol=1e-10, n_iter=2, chi2=ptr["chi2"],
              cov=ptr["cov"], nchan=ptr["i1"], niter=ptr["i2"], status=ptr["i3"])
    m = K.MSG_F
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
            ("no free parameter", dict(free=[0] * 8), m["free"]),
            ("lambda0 0", dict(lam=0.0), m["tol"]), ("lambda0 nan", dict(lam=nan), m["tol"]),
            ("xtol -1", dict(xtol=-1.0), m["tol"]), ("xtol inf", dict(xtol=inf), m["tol"]),
            ("n_iter 0", dict(n_iter=0), m["iter"]), ("2^31 workgroups", dict(n=many), m["wgs"]),
            ("NULL beats sizes", dict(cube=None, n=0), m["nulls"]),
            ("sizes beat n_comp", dict(n=0, nc=3), m["sizes"]),
            ("n_comp beats x", dict(nc=3, x=[nan] * 4), m["comp"]),
            ("x beats the weights", dict(x=[nan] * 4, w=[-1.] * 4), m["x"]),
            ("w beats free", dict(w=[-1.] * 4, free=[0] * 8), m["w"]),
            ("free beats lambda0", dict(free=[0] * 8, lam=0.0), m["free"]),
            ("lambda0 beats n_iter", dict(lam=0.0, n_iter=0), m["tol"]),
            ("n_iter beats the workgroups", dict(n_iter=0, n=many), m["iter"])]:
        assert fit(dict(gf, **change)) == ARG, what
        assert eng.lib.rjp_last_error(eng.ctx).decode() == msg, what
    assert fit(dict(gf, ctx=False)) == ARG
    eng.synchronize()
    for k, t in bufs.items():
        assert torch.equal(t, before[k]), "a refusal wrote " + k
    # the optional pointers may be NULL
    assert fit(dict(gf, w=None, free=None)) == 1 and mom(gm) == 1
    eng.synchronize()


# ---- 5: the model level ---------------------------------------------------------------------------
def _params(tag):
    p = copy.deepcopy(U.load_golden(tag)[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


_MODELS = {}
N_LINE = 48                            # channels of the model-level cube, 12.3 km/s apart


def model(eng, tmp_path_factory):
    from rajepy_amd import classes, logger
    if "jm" not in _MODELS:
        log = logger.Log(str(tmp_path_factory.mktemp("specfit") / "model.log"), verbose=False)
        _MODELS["jm"] = classes.JetModel(_params("cfg1_example"), log=log, engine=eng)
        _MODELS["jm"].time = 1.0 * YEAR
    return _MODELS["jm"]


def line_freqs(rrl, n=N_LINE):
    from rajepy_amd.maths import rrls
    nu0 = rrls.rrl_nu_0(*rrls.rrl_parser(rrl))
    return nu0, nu0 * (1.0 - np.linspace(-282.0, 294.0, n) * 1e3 / 299792458.0)


def test_moments_and_fits_of_the_example_model_s_line(eng, tmp_path_factory):
    """The golden example model and its line on 48 channels 12.3 km/s apart (-282 to 294 km/s: the
    line's pressure-broadened wings are hundreds of km/s wide near the base): `moments_rrl` against the
    long-double reference on the model's own `flux_rrl` cube read back; sum_pixels m0 against sum_c
    dx_c flux_rrl(...).sum() at the summed bound; `specfit_rrl` against `RTEngine.specfit` with a
    trace on the same cube (same bits), the trace followed; status 3 exactly on the sightlines whose
    spectrum is all zero or NaN.  The fitted FWHM beside the thermal width is printed, not asserted."""
    import torch
    from rajepy_amd import engine as E
    from rajepy_amd.maths import rrls
    jm = model(eng, tmp_path_factory)
    rrl = U.load_golden("cfg1_example")[1]["rrl"]
    nu0, freqs = line_freqs(rrl)
    v, dv = E.velocity_axis(freqs, nu0)
    flux = np.asarray(jm.flux_rrl(rrl, freqs), dtype=np.float64)          # (F, nx, nz), read back
    Y = np.ascontiguousarray(flux.reshape(N_LINE, -1).T)
    n = Y.shape[0]
    mom = jm.moments_rrl(rrl, freqs)
    got = {k: mom[k].cpu().numpy().reshape(-1) for k in MKEYS}
    case = dict(Y=Y, x=v, dx=dv, x_ref=float(v[N_LINE // 2]), clip=0.0, live=None)
    judge_moments("model moments", case, got)
    LD, u = K.LD, K.LD(K.U53)
    fin = np.isfinite(Y)
    Yl = np.where(fin, Y, 0.0).astype(LD)
    total = np.sum(Yl.sum(axis=0) * dv.astype(LD))
    bound = np.sum(LD(1.01) * fin.sum(axis=1) * u * (np.abs(Yl) @ dv.astype(LD))) + n * u * abs(total)
    m0sum = np.sum(got["m0"].astype(LD))
    print("sum of m0 %.9e Jy km/s, sum_c dx_c sum_p flux %.9e, difference %.2e, bound %.2e"
          % (float(m0sum), float(total), float(abs(m0sum - total)), float(bound)))
    assert abs(m0sum - total) <= bound
    # the fit: through the model, and through the engine with a trace on the same cube
    res = jm.specfit_rrl(rrl, freqs)
    cube = torch.from_numpy(np.ascontiguousarray(flux.reshape(N_LINE, -1))).to(eng.device)
    m_d, ip_d, _ = eng.cube_moments(cube, v, dv, case["x_ref"])
    th0 = E.specfit_start(m_d, ip_d, v)
    free = C.free_flags(1, False)
    fit = eng.specfit(cube, v, th0, case["x_ref"], free=free, trace=True)
    status = fit["status"].cpu().numpy()
    assert np.array_equal(res["status"].cpu().numpy().reshape(-1), status)
    live = status != 3
    for key, row in (("peak", 0), ("centre", 1), ("sigma", 2)):
        a, b = res[key][0].cpu().numpy().reshape(-1), fit["theta"][row].cpu().numpy()
        assert a[live].tobytes() == b[live].tobytes() and np.all(np.isnan(a[~live])), key
    empty = ~np.any(fin & (Y != 0.0), axis=1)
    assert np.array_equal(status == 3, empty), (int((status == 3).sum()), int(empty.sum()))
    assert 0 < empty.sum() < n
    out = dict(theta=fit["theta"].cpu().numpy().T, chi2=fit["chi2"].cpu().numpy(),
               cov=fit["cov"].cpu().numpy().T, nchan=fit["nchan"].cpu().numpy(),
               niter=fit["niter"].cpu().numpy(), status=status, trace=fit["trace"].cpu().numpy())
    pick = np.nonzero(live)[0]
    pick = pick[::max(1, pick.size // 300)][:600]
    # (RTEngine fills with NaN and -1 where this module's raw calls poison)
    nanp = dict(out, trace=np.where(np.isnan(out["trace"]), P_T, out["trace"]))
    fcase = dict(Y=Y, x=v, w=None, x_ref=case["x_ref"], theta0=th0.cpu().numpy().T, free=free, live=None)
    follow_all("model fit", fcase, {k: nanp[k] for k in KEYS}, pick=pick)
    # the widths: printed beside the thermal width, not asserted (a Voigt profile with velocity
    # structure: no number for the comparison is derivable)
    el, nn, dn = rrls.rrl_parser(rrl)
    thermal = rrls.deltanu_g(nu0, jm.params["properties"]["T_0"], el) / nu0 * 299792.458
    fwhm = res["fwhm"][0].cpu().numpy().reshape(-1)
    conv = status == 1
    print("line %s: %d of %d sightlines fitted (status 1: %d, 0: %d, 2: %d), fitted FWHM median %.2f km/s, "
          "10-90 %% %.2f-%.2f km/s; thermal FWHM at T_0 = %.0f K: %.2f km/s; m2 median %.2f km/s"
          % (rrl, int(live.sum()), n, int(conv.sum()), int((status == 0).sum()), int((status == 2).sum()),
             float(np.median(fwhm[conv])), float(np.percentile(fwhm[conv], 10)),
             float(np.percentile(fwhm[conv], 90)), jm.params["properties"]["T_0"], thermal,
             float(np.nanmedian(got["m2"]))))


def test_specfit_of_a_cleaned_line_cube(eng, tmp_path_factory):
    """The chain connects: `clean_image_rrl` of 12 channels with the 27-antenna fixture, then
    `moments` and `specfit` on its `.image` (a device tensor or a host array: whatever the result
    holds) inside a mask of the bright pixels -> finite results there, NaN and status 3 outside."""
    import torch
    from rajepy_amd import engine as E
    jm = model(eng, tmp_path_factory)
    rrl = U.load_golden("cfg1_example")[1]["rrl"]
    nu0, freqs = line_freqs(rrl, 12)
    v, dv = E.velocity_axis(freqs, nu0)
    tr = jm.uv_tracks(FIXTURE, 1200., 60., min_el_deg=20.)
    cell_as = E.observation_grid(tr.max_baseline_m, float(nu0), 1.0)[0]
    res = jm.clean_image_rrl(rrl, tr.u_m, tr.v_m, freqs, shape=(48, 40), cell_as=cell_as, niter=100)
    img = res.image
    host = img.cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
    assert host.shape == (12, 48, 40)
    peak = host.max(axis=0)
    mask = peak >= 0.3 * peak.max()
    assert 3 <= mask.sum() < mask.size
    mom = jm.moments(img, v, dv, mask=mask)
    assert mom["m0"].shape == (48, 40)
    m0 = mom["m0"].cpu().numpy()
    assert np.all(np.isfinite(m0)) and np.all(m0[~mask] == 0.0) and np.all(mom["ipeak"].cpu().numpy()[~mask] == -1)
    fit = jm.specfit(img, v, mask=mask, free=[1, 1, 1, 1, 0])
    st = fit["status"].cpu().numpy()
    assert np.all(st[~mask] == 3) and np.all(st[mask] != 3)
    for k in ("peak", "centre", "sigma", "fwhm", "integral"):
        a = fit[k][0].cpu().numpy()
        assert np.all(np.isfinite(a[mask])) and np.all(np.isnan(a[~mask])), k
    assert np.all(fit["sigma"][0].cpu().numpy()[mask] > 0)
    print("cleaned cube: %d masked-in pixels, status %s, FWHM %.2f-%.2f km/s"
          % (int(mask.sum()), np.bincount(st[mask], minlength=3).tolist(),
             float(np.nanmin(fit["fwhm"][0].cpu().numpy())), float(np.nanmax(fit["fwhm"][0].cpu().numpy()))))
