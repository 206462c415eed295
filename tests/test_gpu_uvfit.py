"""rjp_uvfit (K20, uvfit.hip: Levenberg-Marquardt fits of point / Gaussian components to
visibilities) through the C-ABI, RTEngine.uvfit and JetModel.uvmodelfit*, against
tests/uvfit_ref.py -- a long-double NumPy reference that FOLLOWS the device's trace (checks (a)-(e)
of its docstring, every bound derived there, none measured), which
tests/test_uvfit_reference_cpu.py pins to hand-worked cases, to a float64 emulation on these very
inputs (tests/uvfit_cases.py: inside the bounds, and converging where convergence is asked here) and
to planted mistakes (outside).

Every raw call runs with guard bands around every buffer and the workspace.  The 1e-9 on the
noise-free fits is a sanity cap, not the accuracy judgement: that is the trace.  The module prints
the worst error / bound per group."""
import copy
import ctypes
import os

import numpy as np
import pytest

from tests import gpu_util as U
from tests import uvfit_cases as C
from tests import uvfit_ref as K
from tests import vis_ref as R

pytestmark = pytest.mark.gpu
YEAR = 31557600.0
WORST = {}
P_F, P_I, P_T = 7.25, -77, -7.5        # poison of the float outputs, the int outputs, the trace
GUARD = 33                             # elements of guard band on either side (odd: the payload of
                                       # a float64 buffer then starts 8 bytes off a 16-byte line)
LAM0, XTOL, N_ITER = C.LAM0, C.XTOL, C.N_ITER
FIXTURE = os.path.join(U.GOLDEN, "antenna_configs", "vla.a.cfg")


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


def run_fit(eng, case, n_iter=N_ITER, theta0=None, lambda0=LAM0, xtol=XTOL, want_trace=True, guard=GUARD):
    """One raw rjp_uvfit call on a case of tests/uvfit_cases.py, every buffer between guard bands
    -> dict of host arrays (theta, chi2, cov, nvis, niter, status, trace, work, ret)."""
    import torch
    V = np.ascontiguousarray(case["V"], dtype=np.complex128)
    M, Kn = V.shape
    th0 = np.asarray(case["theta0"] if theta0 is None else theta0, dtype=np.float64)
    P = th0.shape[-1]
    nc, T = P // 6, P * (P + 1) // 2
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    vis = Band(eng, M * Kn * 2, f64, -1e300, guard).set(V.view(np.float64))
    u, v = Band(eng, Kn, f64, -1e300, guard).set(case["u"]), Band(eng, Kn, f64, -1e300, guard).set(case["v"])
    w, w_maps = None, 1
    if case["w"] is not None:
        w_maps = 1 if np.ndim(case["w"]) == 1 else M
        w = Band(eng, w_maps * Kn, f64, -1e300, guard).set(case["w"])
    theta = Band(eng, M * P, f64, P_F).set(np.broadcast_to(th0, (M, P)))
    chi2, cov = Band(eng, M, f64, P_F), Band(eng, M * T, f64, P_F)
    nvis, niter, status = (Band(eng, M, i32, P_I) for _ in range(3))
    trace = Band(eng, M * n_iter * (3 + P), f64, P_T)
    wb = eng.lib.rjp_uvfit_workspace(M, Kn, nc)
    assert wb == K.workspace_bytes(M, Kn, nc)
    work = Band(eng, wb, u8, 0xA5, 64)
    free = (ctypes.c_uint8 * P)(*[int(x) for x in case["free"]]) if case["free"] is not None else None
    dbl = lambda a: (ctypes.c_double * len(a))(*[float(x) for x in a])
    ret = eng.lib.rjp_uvfit(eng.ctx, vis.ptr, M, Kn, dbl(case["su"]), dbl(case["sv"]), u.ptr, v.ptr,
                            w.ptr if w else None, w_maps, nc, free, theta.ptr, lambda0, xtol, n_iter,
                            chi2.ptr, cov.ptr, nvis.ptr, niter.ptr, status.ptr,
                            trace.ptr if want_trace else None, work.ptr, wb, eng._stream())
    eng.synchronize()
    assert ret == K.tiling(M, Kn)["workgroups"], (ret, eng.lib.rjp_last_error(eng.ctx))
    assert vis.get().tobytes() == V.tobytes(), "the visibilities were written"
    for band in (u, v, w):
        if band:
            band.get()
    return dict(theta=theta.get().reshape(M, P), chi2=chi2.get(), cov=cov.get().reshape(M, T),
                nvis=nvis.get(), niter=niter.get(), status=status.get(),
                trace=trace.get().reshape(M, n_iter, 3 + P), work=work.get(), ret=ret)


KEYS = ("theta", "chi2", "cov", "nvis", "niter", "status", "trace")


def one(out, m):
    return {k: out[k][m] for k in KEYS}


def untouched(out, m, theta0):
    """Map m ended degenerate: status 3 and nothing else written."""
    assert out["status"][m] == 3
    assert np.array_equal(out["theta"][m], np.broadcast_to(theta0, out["theta"].shape)[m], equal_nan=True)
    assert out["chi2"][m] == P_F and np.all(out["cov"][m] == P_F)
    assert out["nvis"][m] == P_I and out["niter"][m] == P_I and np.all(out["trace"][m] == P_T)


def follow_all(kind, case, out, n_iter=N_ITER, theta0=None, lambda0=LAM0, xtol=XTOL):
    case = dict(case, theta0=np.broadcast_to(case["theta0"] if theta0 is None else theta0,
                                             out["theta"].shape))
    for m in range(out["theta"].shape[0]):
        if out["status"][m] == 3:
            untouched(out, m, case["theta0"])
        else:
            data, n, th0, free = C.per_map(case, m)
            note(kind, K.follow(data, n, th0, free, lambda0, xtol, n_iter, one(out, m), P_T))


def same_bits(a, b, keys=KEYS + ("work",)):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), "a repeated call changed " + k


def scaled_error(theta, truth):
    sc = np.stack([K.scales(t) for t in np.atleast_2d(truth)]).astype(np.float64)
    return float(np.max(np.abs(np.atleast_2d(theta) - np.atleast_2d(truth)) / sc))


# ---- 1: the sizes, at the bounds ------------------------------------------------------------------
@pytest.mark.parametrize("n_comp,n_vis", [(1, n) for n in C.N_VIS] + [(2, n) for n in C.N_VIS_TWO])
def test_sizes_against_the_reference(eng, n_comp, n_vis):
    """1 to 262145 visibilities: status 3 below n_free / 2 counting visibilities (1, 2 with one
    component, 5 with two), the thread tail, the tile tail, several tiles and, at 262145 (257
    tiles), the second reduction pass; 1 to 3 maps with their own scales, signs included; weights
    none, shared and per map in turn.  From 255 visibilities on the noise-free analytic data must be
    fitted to 1e-9 of the scales within 40 trials (the emulation does: test_uvfit_reference_cpu)."""
    kind = "%d comp" % n_comp
    case = C.sized(n_vis, n_comp)
    big = n_vis > 100000
    n_iter = (4 if n_comp == 1 else 3) if big else N_ITER     # (the reference sums 262145 terms per row)
    out = run_fit(eng, case, n_iter)
    follow_all(kind, case, out, n_iter)
    if 2 * n_vis < 6 * n_comp:
        assert np.all(out["status"] == 3)
        return
    assert np.all(out["status"] != 3) and np.all(out["nvis"] == n_vis)
    if big:
        assert K.tiling(1, n_vis)["tiles"] == 257 > K.REDUCE_PASS
        assert out["status"][0] == 0 and out["niter"][0] == n_iter
        long = run_fit(eng, case, N_ITER, want_trace=False)
        assert long["status"][0] == 1 and scaled_error(long["theta"], case["truth"]) <= 1e-9
        return
    if n_vis >= 255:
        err = scaled_error(out["theta"], case["truth"])
        print("%s, %d visibilities: iterations %s, worst |theta - truth| / s %.2e" % (kind, n_vis, out["niter"], err))
        assert np.all(out["status"] == 1) and err <= 1e-9, (out["status"], err)
        same_bits(out, run_fit(eng, case, n_iter))
        b = run_fit(eng, case, n_iter, guard=GUARD + 1)                  # every buffer 8 bytes further on
        same_bits(out, b, KEYS)
        c = run_fit(eng, case, n_iter, want_trace=False)                 # d_trace = NULL
        assert np.all(c["trace"] == P_T)
        same_bits(out, c, ("theta", "chi2", "cov", "nvis", "niter", "status"))


@pytest.mark.parametrize("n_comp", [1, 2])
def test_flagged_visibilities_and_an_all_flagged_map(eng, n_comp):
    case = C.flagged(n_comp)
    out = run_fit(eng, case)
    follow_all("flagged", case, out)
    assert list(out["status"]) == [1, 3, 1]
    live = [C.per_map(case, m)[0][0].size for m in (0, 2)]
    assert [out["nvis"][0], out["nvis"][2]] == live and live[0] < live[1] < 1500 * 0.85
    assert scaled_error(out["theta"][[0, 2]], case["truth"][[0, 2]]) <= 1e-9
    # the live maps are fitted as if alone
    alone = dict(case, V=case["V"][2:], su=case["su"][2:], sv=case["sv"][2:], w=case["w"][2:],
                 theta0=case["theta0"][2:], truth=case["truth"][2:])
    a = run_fit(eng, alone)
    for k in KEYS:
        assert a[k][0].tobytes() == out[k][2].tobytes(), k


@pytest.mark.parametrize("level,n_comp,n_vis", [(0.02, 1, 2049), (0.01, 2, 1025)])
def test_noisy_data_are_judged_by_the_trace(eng, level, n_comp, n_vis):
    case = C.sized(n_vis, n_comp, noise=level)
    out = run_fit(eng, case)
    follow_all("noisy", case, out)
    print("noisy %d comp: iterations %s, status %s" % (n_comp, out["niter"], out["status"]))
    assert np.all(out["status"] == 1)
    assert scaled_error(out["theta"], case["truth"]) <= 0.05


# ---- 2: fixed parameters, behaviour per map --------------------------------------------------------
@pytest.mark.parametrize("which", ["point+gauss", "held"])
def test_fixed_parameters_keep_their_start(eng, which):
    case = C.fixed(which)
    out = run_fit(eng, case)
    follow_all("fixed", case, out)
    fr = case["free"] != 0
    assert out["status"][0] == 1 and scaled_error(out["theta"], case["truth"]) <= 1e-9
    assert np.array_equal(out["theta"][0][~fr], case["theta0"][0][~fr])
    assert np.all(out["trace"][0, :out["niter"][0], 3:][:, ~fr] == case["theta0"][0][~fr])
    # d_cov: the identity's rows for the fixed parameters
    N = K.unpack(out["cov"][0], fr.size)
    for i in np.nonzero(~fr)[0]:
        want = np.zeros(fr.size)
        want[i] = 1.0
        assert np.array_equal(N[i], want)


def test_start_outside_the_cone_fixed_point_and_the_rest_of_the_stack(eng):
    """Map 0 sits at its fixed point (a point source of 1.5 at the phase centre against V = 1.5:
    phase 0, envelope 1, chi^2 an exact 0) and ends after one trial; map 1 starts outside the PSD
    cone, map 3 from a NaN: status 3, nothing written; map 2 runs on and is fitted as if alone."""
    case = C.stack()
    V, th0, truth = case["V"], case["theta0"].copy(), case["truth"][2]
    out = run_fit(eng, case)
    follow_all("per map", case, out)
    assert list(out["status"]) == [1, 3, 1, 3]
    assert out["niter"][0] == 1 and out["chi2"][0] == 0.0 and np.array_equal(out["theta"][0], th0[0])
    assert out["niter"][2] > 1 and scaled_error(out["theta"][2], truth) <= 1e-9
    alone = run_fit(eng, dict(case, V=V[2:3], su=case["su"][:1], sv=case["sv"][:1], theta0=th0[2:3]))
    for k in KEYS:
        assert out[k][2].tobytes() == alone[k][0].tobytes(), k
    # a negative size alone is outside the cone as well; a zero one (a point) is inside
    th0[1, 3:] = [-1e-3, 0.0, 1.0]
    assert run_fit(eng, dict(case, theta0=th0))["status"][1] == 3
    th0[1, 3:] = 0.0
    assert run_fit(eng, dict(case, theta0=th0))["status"][1] != 3


@pytest.mark.parametrize("n_comp", [1, 2])
def test_exhausted_and_continued(eng, n_comp):
    case = C.sized(1025, n_comp)
    first = run_fit(eng, case, 3)
    follow_all("exhausted", case, first, 3)
    assert np.all(first["status"] == 0) and np.all(first["niter"] == 3)
    second = run_fit(eng, case, N_ITER, theta0=first["theta"])
    follow_all("continued", case, second, N_ITER, theta0=first["theta"])
    long = run_fit(eng, case, N_ITER)
    assert np.all(second["status"] == 1) and np.all(long["status"] == 1)
    assert scaled_error(second["theta"], long["theta"]) <= 1e-9
    assert scaled_error(second["theta"], case["truth"]) <= 1e-9


def test_engine_uvfit(eng):
    import torch
    case = C.fixed("point+gauss")
    raw = run_fit(eng, case, 30)
    V = torch.from_numpy(case["V"]).to(eng.device)
    fit = eng.uvfit(V, case["su"], case["sv"], case["u"], case["v"], case["theta0"], free=case["free"],
                    n_iter=30, lambda0=LAM0, xtol=XTOL, trace=True)
    assert eng.last_uvfit_tiles == raw["ret"] == 1
    assert fit["status"].dtype == torch.int32 and fit["trace"].shape == (1, 30, 15)
    for k in ("theta", "chi2", "cov", "nvis", "niter", "status"):
        assert fit[k].cpu().numpy().tobytes() == raw[k].tobytes(), k
    n = raw["niter"][0]
    tr = fit["trace"].cpu().numpy()
    assert tr[0, :n].tobytes() == raw["trace"][0, :n].tobytes() and np.all(np.isnan(tr[0, n:]))
    # shared and per-map weights, float64 [M, K, 2] visibilities, one start for all maps
    three = C.sized(257, 1)
    w = np.random.default_rng(2).lognormal(0.0, 0.3, (3, 257))
    Vr = torch.view_as_real(torch.from_numpy(three["V"]).to(eng.device)).contiguous()
    for ww in (None, w[0], w):
        a = eng.uvfit(Vr, three["su"], three["sv"], three["u"], three["v"], three["theta0"], weights=ww)
        b = run_fit(eng, dict(three, w=ww), 60)
        assert "trace" not in a and a["theta"].cpu().numpy().tobytes() == b["theta"].tobytes()
    for bad in (dict(n_iter=0), dict(lambda0=0.0), dict(xtol=float("nan")), dict(free=np.zeros(6)),
                dict(free=np.ones(5)), dict(weights=np.ones(5))):
        with pytest.raises(ValueError):
            eng.uvfit(Vr, three["su"], three["sv"], three["u"], three["v"], three["theta0"], **bad)
    with pytest.raises(ValueError):
        eng.uvfit(Vr, three["su"], three["sv"], three["u"], three["v"], np.zeros((3, 18)))
    with pytest.raises(ValueError):
        eng.uvfit(Vr, three["su"], three["sv"], three["u"][:-1], three["v"], three["theta0"])


# ---- 3: refusals ----------------------------------------------------------------------------------
def test_refusals_leave_poisoned_outputs_untouched(eng):
    import torch
    from rajepy_amd import _lib
    M, Kn, n_iter, P = 2, 7, 4, 12
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    full = lambda n, v, dt: torch.full((n,), v, dtype=dt, device=eng.device)
    wb = eng.lib.rjp_uvfit_workspace(M, Kn, 2)
    bufs = dict(vis=full(M * Kn * 2, 7.0, f64), u=full(Kn, 0.1, f64), v=full(Kn, 0.1, f64),
                w=full(M * Kn, 1.0, f64), theta=full(M * P, 0.5, f64), chi2=full(M, P_F, f64),
                cov=full(M * 78, P_F, f64), nvis=full(M, P_I, i32), niter=full(M, P_I, i32),
                status=full(M, P_I, i32), trace=full(M * n_iter * (3 + P), P_T, f64),
                work=full(wb, 0xA5, u8))
    before = {k: t.clone() for k, t in bufs.items()}
    good = dict(bufs, n_maps=M, n_vis=Kn, su=(1.0, -1.0), sv=(1.0, 1.0), w_maps=M, n_comp=2,
                free=None, lam=1e-3, xtol=1e-10, n_iter=n_iter, nbytes=wb, ctx=True)
    ptr = lambda t: t.data_ptr() if t is not None else None
    dbl = lambda a: (ctypes.c_double * len(a))(*a) if a is not None else None

    def fit(a):
        free = (ctypes.c_uint8 * len(a["free"]))(*a["free"]) if a["free"] is not None else None
        return eng.lib.rjp_uvfit(eng.ctx if a["ctx"] else None, ptr(a["vis"]), a["n_maps"], a["n_vis"],
                                 dbl(a["su"]), dbl(a["sv"]), ptr(a["u"]), ptr(a["v"]), ptr(a["w"]),
                                 a["w_maps"], a["n_comp"], free, ptr(a["theta"]), a["lam"], a["xtol"],
                                 a["n_iter"], ptr(a["chi2"]), ptr(a["cov"]), ptr(a["nvis"]),
                                 ptr(a["niter"]), ptr(a["status"]), ptr(a["trace"]), ptr(a["work"]),
                                 a["nbytes"], eng._stream())

    ARG, WS = _lib.RJP_ERR_ARG, _lib.RJP_ERR_WORKSPACE
    inf, nan = float("inf"), float("nan")
    m = K.MSG
    cases = [("NULL " + k, {k: None}, ARG, m["nulls"])
             for k in ("vis", "su", "sv", "u", "v", "theta", "chi2", "cov", "nvis", "niter", "status")]
    cases += [("n_maps 0", dict(n_maps=0), ARG, m["sizes"]), ("n_vis 0", dict(n_vis=0), ARG, m["sizes"]),
              ("n_vis -1", dict(n_vis=-1), ARG, m["sizes"]),
              ("n_comp 0", dict(n_comp=0), ARG, m["comp"]), ("n_comp 3", dict(n_comp=3), ARG, m["comp"]),
              ("w_maps 0", dict(w_maps=0), ARG, m["wmaps"]), ("w_maps 3", dict(w_maps=3), ARG, m["wmaps"]),
              ("su nan", dict(su=(1.0, nan)), ARG, m["scale"]), ("sv inf", dict(sv=(inf, 1.0)), ARG, m["scale"]),
              ("no free parameter", dict(free=[0] * 12), ARG, m["free"]),
              ("lambda0 0", dict(lam=0.0), ARG, m["tol"]), ("lambda0 inf", dict(lam=inf), ARG, m["tol"]),
              ("lambda0 nan", dict(lam=nan), ARG, m["tol"]), ("xtol -1", dict(xtol=-1.0), ARG, m["tol"]),
              ("xtol nan", dict(xtol=nan), ARG, m["tol"]), ("xtol inf", dict(xtol=inf), ARG, m["tol"]),
              ("n_iter 0", dict(n_iter=0), ARG, m["iter"]),
              ("short workspace", dict(nbytes=wb - 1), WS, m["short"]),
              ("NULL workspace", dict(work=None), WS, m["short"]),
              # which one wins: the order of check_uvfit, the workspace last
              ("NULL beats sizes", dict(vis=None, n_vis=0), ARG, m["nulls"]),
              ("sizes beat n_comp", dict(n_maps=0, n_comp=3), ARG, m["sizes"]),
              ("n_comp beats w_maps", dict(n_comp=3, w_maps=5), ARG, m["comp"]),
              ("w_maps beats the scales", dict(w_maps=5, su=(nan, 1.0)), ARG, m["wmaps"]),
              ("scales beat free", dict(su=(nan, 1.0), free=[0] * 12), ARG, m["scale"]),
              ("free beats lambda0", dict(free=[0] * 12, lam=0.0), ARG, m["free"]),
              ("lambda0 beats n_iter", dict(lam=0.0, n_iter=0), ARG, m["tol"]),
              ("n_iter beats the workspace", dict(n_iter=0, nbytes=0), ARG, m["iter"])]
    for what, change, code, msg in cases:
        assert fit(dict(good, **change)) == code, what
        assert eng.lib.rjp_last_error(eng.ctx).decode() == msg, what
    # more than 2^31 - 1 workgroups: 1025 maps of 2^31 - 1 visibilities (2^21 tiles each); nothing on
    # the device is dereferenced before the refusal, so the small buffers do
    many = dict(n_maps=1025, n_vis=2 ** 31 - 1, su=(1.0,) * 1025, sv=(1.0,) * 1025, w_maps=1)
    for what, change, msg in (("1025 x 2^21 workgroups", many, m["wgs"]),
                              ("workgroups beat the workspace", dict(many, nbytes=0, work=None), m["wgs"]),
                              ("n_iter beats the workgroups", dict(many, n_iter=0), m["iter"])):
        assert fit(dict(good, **change)) == ARG, what
        assert eng.lib.rjp_last_error(eng.ctx).decode() == msg, what
    assert fit(dict(good, ctx=False)) == ARG
    eng.synchronize()
    for k, t in bufs.items():
        assert torch.equal(t, before[k]), "a refusal wrote " + k
    assert eng.lib.rjp_uvfit_workspace(0, 15, 1) == 0 and eng.lib.rjp_uvfit_workspace(2, 0, 1) == 0
    assert eng.lib.rjp_uvfit_workspace(2, 15, 0) == 0 and eng.lib.rjp_uvfit_workspace(2, 15, 3) == 0
    # optional pointers may be NULL; w_maps is not looked at without weights
    assert fit(dict(good, w=None, w_maps=9, trace=None, free=None)) == 2
    eng.synchronize()


# ---- 4: the chain ---------------------------------------------------------------------------------
def test_rendered_gaussian_through_rjp_vis_is_fitted_back(eng):
    """K14's G = S exp(-(A dx^2 + 2 B dx dz + C dz^2)) rendered on 41 x 37 pixels, transformed by
    rjp_vis at 600 points of at most 0.25 cycles per cell, and fitted in the uv plane: Sigma =
    (2 Q)^-1, F = S pi / sqrt(det Q), the offset from the map centre -- to 1e-8 of the scales (the
    pixel sum differs from the continuous transform by aliasing alone, 6e-10 in a NumPy prototype
    on this input)."""
    import torch
    from tests import gaussfit_ref as G
    nx, nz, A, B, Cq = 41, 37, 0.05, 0.01, 0.08
    ix, iz = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    img = G.model([1.0, 21.3, 17.2, A, B, Cq], ix.ravel(), iz.ravel(), np.float64, with_jac=False)[0]
    rng = np.random.default_rng(41)
    a, b = R.random_points(rng, 600, 0.25)
    V = eng.vis(torch.from_numpy(img[None]).to(eng.device), nx, nz, [1.0], [1.0], a, b)
    det = A * Cq - B * B
    truth = np.array([np.pi / np.sqrt(det), 21.3 - (nx - 1) / 2, 17.2 - (nz - 1) / 2,
                      Cq / (2 * det), -B / (2 * det), A / (2 * det)])
    case = dict(V=V.cpu().numpy(), u=a, v=b, su=[1.0], sv=[1.0], w=None, free=None,
                theta0=C.off(truth)[None], truth=truth[None])
    out = run_fit(eng, case)
    follow_all("chain", case, out)
    err = scaled_error(out["theta"], truth)
    print("rendered Gaussian: iterations %s, worst |theta - truth| / s %.2e" % (out["niter"], err))
    assert out["status"][0] == 1 and err <= 1e-8, err


def test_two_moving_components_as_one_stack(eng):
    """Two analytic components that move linearly over 5 epochs, seen in 2 channels (scales 1 and
    0.8): one stack of 10 maps, one call; the fitted positions recover the motion to 1e-9 cells."""
    case = C.moving()
    out = run_fit(eng, case)
    follow_all("chain", case, out)
    assert out["ret"] == 10 and np.all(out["status"] == 1)
    fit = out["theta"].reshape(5, 2, 12)
    for c, (vx, vz) in enumerate(((0.3, -0.2), (-0.5, 0.45))):
        pos = fit[:, :, 6 * c + 1:6 * c + 3]
        motion = (pos[1:] - pos[:-1])
        assert np.max(np.abs(motion - np.array([vx, vz]))) <= 1e-9, motion
    assert scaled_error(out["theta"], case["truth"]) <= 1e-9


# ---- 5: the model level ---------------------------------------------------------------------------
def _params(tag):
    p = copy.deepcopy(U.load_golden(tag)[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


_MODELS = {}
T_OBS, T_INT, MIN_EL = 1200., 60., 20.


def model(eng, tmp_path_factory):
    from rajepy_amd import classes, logger
    if "jm" not in _MODELS:
        log = logger.Log(str(tmp_path_factory.mktemp("uvfit") / "model.log"), verbose=False)
        _MODELS["jm"] = classes.JetModel(_params("cfg1_example"), log=log, engine=eng)
        _MODELS["jm"].time = 1.0 * YEAR
    return _MODELS["jm"]


def two_start(jm, one_fit, cell):
    """A two-component start from the one-component fit: its halves, a quarter of the major axis
    either side of the centre along it."""
    from rajepy_amd import engine as E
    f = one_fit
    d = 0.25 * f["maj_as"]
    s, c = np.sin(np.radians(f["pa_deg"])), np.cos(np.radians(f["pa_deg"]))
    comp = lambda sg: E.uvfit_theta(0.5 * f["I"]["val"], f["east_as"] + sg * d * s, f["north_as"] + sg * d * c,
                                    0.6 * f["maj_as"], max(f["min_as"], 0.2 * f["maj_as"]), f["pa_deg"], cell)
    return np.concatenate([comp(+1), comp(-1)])


def test_uvmodelfit_on_the_example_model(eng, tmp_path_factory):
    """The golden example model with the 27-antenna fixture (20 integrations, 7020 visibilities):
    `uvmodelfit_ff` against `uvmodelfit` on `visibilities_ff`'s output, bit for bit; the noisy
    visibilities of `observe_ff` with weights 1 / sigma^2: the reduced chi^2 of the two-component
    fit; the one-component flux against the zero-spacing flux and against K14's."""
    from rajepy_amd import engine as E
    jm = model(eng, tmp_path_factory)
    freqs = np.array([4.9e9, 5.1e9])
    tr = jm.uv_tracks(FIXTURE, T_OBS, T_INT, min_el_deg=MIN_EL)
    cell_as = E.observation_grid(tr.max_baseline_m, 5e9, 1.0)[0]
    cell = np.radians(cell_as / 3600.)
    assert tr.u_m.numel() == 7020
    a = jm.uvmodelfit_ff(tr.u_m, tr.v_m, freqs, cell_as=cell_as)
    V = jm.visibilities_ff(tr.u_m, tr.v_m, freqs)
    b = jm.uvmodelfit(V, tr.u_m, tr.v_m, freqs, cell_as=cell_as)
    assert len(a) == len(b) == 2 and all(len(x) == 1 for x in a)
    for f in range(2):
        assert a[f][0]["status"] in (0, 1) and a[f][0]["nvis"] == 7020
        for k in ("theta",):
            assert a[f][0][k].tobytes() == b[f][0][k].tobytes(), (f, k)
        for k in ("chi2", "east_as", "north_as", "maj_as", "min_as", "pa_deg"):
            assert np.array([a[f][0][k]]).tobytes() == np.array([b[f][0][k]]).tobytes(), (f, k)
        assert a[f][0]["I"]["val"] == b[f][0]["I"]["val"] and a[f][0]["Ierr"] == b[f][0]["Ierr"]
    # the one-component flux: the zero spacing, and K14's integrated flux of the restored image
    zero = jm.flux_vs_time([jm.time], freqs)[0]
    res = jm.clean_image_ff(tr.u_m, tr.v_m, freqs, shape=(48, 40), cell_as=cell_as, niter=300,
                            threshold_jy=0.0, imfit=True)
    for f in range(2):
        I = a[f][0]["I"]["val"]
        d0, d14 = abs(I - zero[f]) / zero[f], abs(I - res.imfit[f]["I"]["val"]) / zero[f]
        print("channel %d: uv-plane I %.6e Jy, zero spacing %.6e Jy (relative difference %.3e), imfit I %.6e "
              "Jy (relative difference %.3e); reduced chi^2 of the noise-free one-component fit %.3e; size "
              "%.4f x %.4f arcsec at %.1f deg" % (f, I, zero[f], d0, res.imfit[f]["I"]["val"], d14,
                                                 a[f][0]["reduced_chi2"], a[f][0]["maj_as"],
                                                 a[f][0]["min_as"], a[f][0]["pa_deg"]))
        # MEASURED model misfits, asserted at twice the measured value: the jet
        # is not one Gaussian, so neither number is a rounding bound
        assert d0 <= MISFIT_ZERO_SPACING, (f, d0)
        assert d14 <= MISFIT_IMFIT, (f, d14)
    # noisy data with thermal weights: two components
    peak = float(zero.max())
    sigma = np.array([0.1, 0.05]) * peak
    obs = jm.observe_ff(tr, freqs, T_OBS, T_INT, sigma_jy=sigma, seed=11,
                        shape=(48, 40), cell_as=cell_as, niter=10)
    w = np.repeat(1.0 / sigma[:, None] ** 2, 7020, axis=1)
    start = np.stack([two_start(jm, a[f][0], cell) for f in range(2)])
    two = jm.uvmodelfit(obs.vis, tr.u_m, tr.v_m, freqs, weights=w, cell_as=cell_as, comps=2, theta0=start)
    one_ = jm.uvmodelfit(obs.vis, tr.u_m, tr.v_m, freqs, weights=w, cell_as=cell_as)
    for f in range(2):
        red, red1 = two[f][0]["reduced_chi2"], one_[f][0]["reduced_chi2"]
        margin = 5.0 / np.sqrt(2 * 7020)
        print("channel %d: reduced chi^2 two components %.5f, one component %.5f (|. - 1| allowed %.5f), status %d, "
              "Ierr %s" % (f, red, red1, margin, two[f][0]["status"], [c["Ierr"]["val"] for c in two[f]]))
        assert two[f][0]["nvis"] == 7020 and len(two[f]) == 2
        assert abs(red - 1.0) <= margin, (f, red)
        assert all(c["Ierr"]["val"] is not None and c["Ierr"]["val"] > 0 for c in two[f])


# twice the largest relative difference measured on the device (see the test above and DESIGN)
MISFIT_ZERO_SPACING = 3.8e-3       # measured 1.63e-3 and 1.89e-3 (4.9, 5.1 GHz)
MISFIT_IMFIT = 2.7e-3              # measured 1.08e-3 and 1.31e-3


def test_uvmodelfit_vs_time_and_mfs(eng, tmp_path_factory):
    """`uvmodelfit_vs_time` gives, epoch by epoch, what `uvmodelfit_ff` gives at that model time
    (same bits: one call per chunk of the same visibilities); `mfs` fits one model to both
    channels."""
    from rajepy_amd import engine as E
    jm = model(eng, tmp_path_factory)
    freqs = np.array([4.9e9, 5.1e9])
    tr = jm.uv_tracks(FIXTURE, T_OBS, T_INT, min_el_deg=MIN_EL)
    cell_as = E.observation_grid(tr.max_baseline_m, 5e9, 1.0)[0]
    times = [0.8 * YEAR, 1.0 * YEAR, 1.3 * YEAR]
    sweep = jm.uvmodelfit_vs_time(times, tr.u_m, tr.v_m, freqs, cell_as=cell_as)
    assert len(sweep) == 3 and all(len(e) == 2 and len(e[0]) == 1 for e in sweep)
    # From a given start, the same bits as `uvmodelfit` of the sweep's own visibilities, epoch by
    # epoch: a map's fit does not depend on the stack it is in.  (The default start does, in its
    # last bits: `uvfit_start` sums with torch reductions, whose order follows the stack's shape.)
    V = jm.visibilities_vs_time(times, tr.u_m, tr.v_m, freqs)
    start = np.array([[sweep[e][f][0]["theta"] for f in range(2)] for e in range(3)]) * 1.05
    given = jm.uvmodelfit_vs_time(times, tr.u_m, tr.v_m, freqs, cell_as=cell_as, theta0=start)
    old = jm.time
    try:
        for e, t in enumerate(times):
            want = jm.uvmodelfit(V[e], tr.u_m, tr.v_m, freqs, cell_as=cell_as, theta0=start[e])
            # ... and what `uvmodelfit_ff` finds at that model time (the maps of a sweep and of the
            # model's own time agree to rounding, not to the bit)
            jm.time = t
            at = jm.uvmodelfit_ff(tr.u_m, tr.v_m, freqs, cell_as=cell_as)
            for f in range(2):
                assert given[e][f][0]["theta"].tobytes() == want[f][0]["theta"].tobytes(), (e, f)
                assert scaled_error(given[e][f][0]["theta"], sweep[e][f][0]["theta"]) <= 1e-7, (e, f)
                assert scaled_error(sweep[e][f][0]["theta"], at[f][0]["theta"]) <= 1e-7, (e, f)
    finally:
        jm.time = old
    flux = np.array([[sweep[e][f][0]["I"]["val"] for f in range(2)] for e in range(3)])
    assert np.all(flux > 0) and np.ptp(flux[:, 0]) > 0, "the epochs differ"
    old_bytes = jm.VIS_STACK_BYTES
    try:
        jm.VIS_STACK_BYTES = 2 * jm.nx * jm.nz * 8                       # chunks of one epoch
        chunked = jm.uvmodelfit_vs_time(times, tr.u_m, tr.v_m, freqs, cell_as=cell_as, theta0=start)
    finally:
        jm.VIS_STACK_BYTES = old_bytes
    for e in range(3):
        for f in range(2):
            assert chunked[e][f][0]["theta"].tobytes() == given[e][f][0]["theta"].tobytes()
    mfs = jm.uvmodelfit_ff(tr.u_m, tr.v_m, freqs, cell_as=cell_as, mfs=True)
    assert len(mfs) == 1 and mfs[0][0]["nvis"] == 2 * 7020 and mfs[0][0]["status"] in (0, 1)
    lo, hi = sorted(x[0]["I"]["val"] for x in jm.uvmodelfit_ff(tr.u_m, tr.v_m, freqs, cell_as=cell_as))
    assert lo <= mfs[0][0]["I"]["val"] <= hi
    # a point component: sizes held at 0
    pt = jm.uvmodelfit_ff(tr.u_m, tr.v_m, freqs, cell_as=cell_as, comptype="P")
    assert all(p[0]["point_source"] and p[0]["maj_as"] == 0.0 and p[0]["maj_err_as"] is None for p in pt)
    with pytest.raises(ValueError):
        jm.uvmodelfit_ff(tr.u_m, tr.v_m, freqs, comps=2)               # no start for two components
    with pytest.raises(ValueError):
        jm.uvmodelfit_ff(tr.u_m, tr.v_m, freqs, comps=3, theta0=np.zeros(18))
