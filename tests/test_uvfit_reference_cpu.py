"""tests/uvfit_ref.py -- the reference that follows rjp_uvfit's trace on the GPU
(tests/test_gpu_uvfit.py) -- pinned on the CPU first: hand-worked cases, the Jacobian against
Richardson-extrapolated central differences, the identity with K14's parametrisation against a
long-double direct Fourier sum, a float64 NumPy emulation of the device's arithmetic on every GPU
case's inputs (inside the bounds, and converging where the GPU test demands it), planted mistakes
(outside), then the host helpers, the ABI, check_uvfit from a plain C++ program and the Python
paths on a recording engine."""
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
from rajepy_amd import imaging
from tests import gaussfit_ref as G
from tests import uvfit_cases as C
from tests import uvfit_ref as K
from tests import vis_ref as R

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -7.5
LAM0, XTOL, N_ITER = C.LAM0, C.XTOL, C.N_ITER
PI = K.PI_LD


def emulate(case, m, n_iter=N_ITER, xtol=XTOL, **kw):
    data, n, th0, free = C.per_map(case, m)
    return (data, n, th0, free), K.emulate(data, n, th0, free, LAM0, xtol, n_iter, poison=POISON, **kw)


def follow(args, out, n_iter=N_ITER, xtol=XTOL):
    data, n, th0, free = args
    return K.follow(data, n, th0, free, LAM0, xtol, n_iter, out, POISON)


# ---- hand-worked -----------------------------------------------------------------------------------
def test_a_point_source_at_the_phase_centre_by_hand():
    """V = F for all k, a point of flux F at the centre: the phasor is 1, the envelope 1, chi^2 = 0;
    the Jacobian columns are dF (1, 0), dx (0, -2 pi a F), dz (0, -2 pi b F), dsxx (-2 pi^2 a^2 F, 0),
    dsxz (-4 pi^2 a b F, 0), dszz (-2 pi^2 b^2 F, 0): N in closed form, real and imaginary columns
    orthogonal."""
    F = 1.5
    rng = np.random.default_rng(1)
    a, b, w = rng.uniform(-0.2, 0.2, 9), rng.uniform(-0.2, 0.2, 9), rng.lognormal(0, 0.4, 9)
    th = [F, 0.0, 0.0, 0.0, 0.0, 0.0]
    data = K.counting(np.full(9, F + 0j), a, b, w)
    s = K.Sums(th, data, 9)
    al, bl, wl = a.astype(LD), b.astype(LD), w.astype(LD)
    re = np.stack([np.ones(9, dtype=LD), 0 * al, 0 * al, -2 * PI * PI * al * al * F,
                   -4 * PI * PI * al * bl * F, -2 * PI * PI * bl * bl * F])
    im = np.stack([0 * al, -2 * PI * al * F, -2 * PI * bl * F, 0 * al, 0 * al, 0 * al])
    N = (re * wl) @ re.T + (im * wl) @ im.T
    assert s.n == 9 and s.chi2 == 0 and np.all(s.g == 0)
    assert np.max(np.abs(K.unpack(s.N, 6) - N)) <= 1e-17 * np.max(np.abs(N))
    assert N[0, 0] == wl.sum() and N[0, 1] == 0 and N[1, 3] == 0
    assert s.bchi > 0 and np.all(s.bN > 0) and np.all(s.bg > 0)
    # the fit ends after one trial with an exact 0, and the reference follows it
    out = K.emulate(data, 9, th, None, LAM0, XTOL, 7, poison=POISON)
    assert out["status"] == 1 and out["niter"] == 1 and out["chi2"] == 0.0 and out["nvis"] == 9
    assert np.array_equal(out["trace"][0], [0.0, LAM0, 1.0] + th) and np.all(out["trace"][1:] == POISON)
    assert K.follow(data, 9, th, None, LAM0, XTOL, 7, out, POISON) <= 1.0
    # a residual d in the real part: g_F = sum w d
    s2 = K.Sums(th, K.counting(np.full(9, F + 0.25 + 0j), a, b, w), 9)
    assert abs(s2.g[0] - LD(0.25) * wl.sum()) <= 1e-17 and abs(s2.chi2 - LD(0.0625) * wl.sum()) <= 1e-17


def test_one_visibility_at_the_origin():
    """(u, v) = (0, 0): M = sum F whatever the positions and sizes, only the dF columns are not zero;
    one visibility is fewer than n_free / 2: degenerate, nothing but the status."""
    th = [1.25, 3.0, -2.0, 4.0, 1.0, 2.0, 0.5, -1.0, 6.0, 0.0, 0.0, 0.0]
    data = K.counting(np.array([2.0 + 0.5j]), np.zeros(1), np.zeros(1), np.array([4.0]))
    M, J, _ = K.model(th, data[1], data[2], LD)
    assert M[0, 0] == LD(1.75) and M[1, 0] == 0
    assert J[0, 0, 0] == 1 and J[6, 0, 0] == 1 and np.count_nonzero(J) == 2
    s = K.Sums(th, data, 1)
    assert s.chi2 == 4 * (LD(0.25) ** 2 + LD(0.5) ** 2)
    assert s.g[0] == 4 * LD(0.25) and s.g[6] == s.g[0]
    for free, n in ((None, 12), ([1] + [0] * 11, 1), ([1, 1, 1] + [0] * 9, 3)):
        out = K.emulate(data, 1, th, free, LAM0, XTOL, 5, poison=POISON)
        assert (out["status"] == 3) == (2 * 1 < n), n
        if out["status"] == 3:
            assert out["theta"] is None and np.all(out["trace"] == POISON)
    # the tile rule, the workspace and the depth of the sums
    assert K.sizes(1) == (6, 21, 29, 48) and K.sizes(2) == (12, 78, 92, 120)
    assert K.tiling(3, 1024) == {"tiles": 1, "workgroups": 3}
    assert K.tiling(2, 262145) == {"tiles": 257, "workgroups": 514}
    assert K.workspace_bytes(2, 262145, 2) == (514 * 92 + 2 * 120) * 16
    assert K.depth(1024) == 89 and K.depth(262145) == 90


def test_jacobian_against_richardson_differences():
    th = np.array([-1.3, 3.3, -4.8, 2.1, 0.6, 1.3, 0.7, -2.2, 1.9, 0.0, 0.0, 0.0], dtype=LD)
    rng = np.random.default_rng(4)
    a, b = rng.uniform(-0.25, 0.25, 40), rng.uniform(-0.25, 0.25, 40)
    _, J, _ = K.model(th, a, b, LD)
    for k in range(12):
        def diff(h):
            lo, hi = th.copy(), th.copy()
            lo[k] -= h
            hi[k] += h
            return (K.model(hi, a, b, LD, with_jac=False)[0] - K.model(lo, a, b, LD, with_jac=False)[0]) / (2 * h)
        h = LD(1e-3) * max(abs(th[k]), LD(0.1))
        rich = (4 * diff(h / 2) - diff(h)) / 3                      # O(h^4)
        assert np.max(np.abs(rich - J[k])) <= 1e-9 * np.max(np.abs(J[k])), k


def test_identity_with_the_image_plane_gaussian():
    """K14's S exp(-(A dx^2 + 2 B dx dz + C dz^2)) rendered on 41 x 37 pixels and summed directly
    (tests/vis_ref.py, long double) is this model with Sigma = (2 Q)^-1, F = S pi / sqrt(det Q) and
    the offset from the map centre, up to the aliasing of the pixel sum (far below 1e-9 here)."""
    nx, nz, A, B, Cq = 41, 37, 0.05, 0.01, 0.08
    ix, iz = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    img = G.model([1.0, 21.3, 17.2, A, B, Cq], ix.ravel(), iz.ravel(), np.float64, with_jac=False)[0]
    a, b = R.random_points(np.random.default_rng(41), 60, 0.25)
    direct = R.vis_ref(img.reshape(nx, nz), a, b)
    det = A * Cq - B * B
    th = [np.pi / np.sqrt(det), 21.3 - (nx - 1) / 2, 17.2 - (nz - 1) / 2, Cq / (2 * det), -B / (2 * det),
          A / (2 * det)]
    M = K.model(th, a, b, LD, with_jac=False)[0]
    assert np.max(np.abs(direct.real - M[0])) <= 1e-9 * th[0]
    assert np.max(np.abs(direct.imag - M[1])) <= 1e-9 * th[0]


# ---- the emulation inside the bounds and converging, the mistakes outside --------------------------
def _check(case, n_iter=N_ITER, converge=True):
    for m in range(case["V"].shape[0]):
        args, out = emulate(case, m, n_iter)
        if out["status"] == 3:
            assert 2 * args[0][0].size < (12 if case["theta0"].shape[-1] == 12 and case["free"] is None
                                          else 6) or not K.psd(args[2])
            continue
        assert follow(args, out, n_iter) <= 1.0
        if converge:
            err = np.max(np.abs(out["theta"] - case["truth"][m]) / K.scales(case["truth"][m]).astype(np.float64))
            assert out["status"] == 1 and out["niter"] <= N_ITER and err <= 1e-9, (m, out["status"], err)


@pytest.mark.parametrize("n_comp,n_vis", [(1, n) for n in C.N_VIS] + [(2, n) for n in C.N_VIS_TWO])
def test_emulation_on_the_sized_cases(n_comp, n_vis):
    """Inside the bounds on every input of test_gpu_uvfit's size cases, and -- non-vacuity -- it
    reaches the 1e-9 within 40 trials that the GPU test demands from 255 visibilities on."""
    big = n_vis > 100000
    case = C.sized(n_vis, n_comp)
    _check(case, (4 if n_comp == 1 else 3) if big else N_ITER, converge=255 <= n_vis and not big)
    if big:
        _, out = emulate(case, 0)
        err = np.max(np.abs(out["theta"] - case["truth"][0]) / K.scales(case["truth"][0]).astype(np.float64))
        assert out["status"] == 1 and err <= 1e-9


@pytest.mark.parametrize("name", ["flagged 1", "flagged 2", "point+gauss", "held", "noisy 1", "noisy 2"])
def test_emulation_on_the_other_cases(name):
    case = {"flagged 1": lambda: C.flagged(1), "flagged 2": lambda: C.flagged(2),
            "point+gauss": lambda: C.fixed("point+gauss"), "held": lambda: C.fixed("held"),
            "noisy 1": lambda: C.sized(2049, 1, noise=0.02), "noisy 2": lambda: C.sized(1025, 2, noise=0.01)}[name]()
    _check(case, converge=not name.startswith("noisy"))
    if name.startswith("noisy"):
        for m in range(case["V"].shape[0]):
            out = emulate(case, m)[1]
            err = np.max(np.abs(out["theta"] - case["truth"][m]) / K.scales(case["truth"][m]).astype(np.float64))
            assert out["status"] == 1 and err <= 0.05
    # an exhausted fit is status 0, and the reference follows it too
    args, short = emulate(case, 0, 3)
    assert short["status"] == 0 and short["niter"] == 3 and follow(args, short, 3) <= 1.0


def test_emulation_on_the_stack_and_the_moving_components():
    case = C.stack()
    status = []
    for m in range(4):
        args, out = emulate(case, m)
        status.append(out["status"])
        if out["status"] != 3:
            assert follow(args, out) <= 1.0
    assert status == [1, 3, 1, 3]
    _check(C.moving())


def _mistake_case(mistake):
    if mistake == "fixed_moves":
        return C.fixed("held")
    if mistake == "accept_le":
        return C.sized(2049, 1, noise=0.02)
    case = C.sized(1025, 2, noise=0.01)
    return dict(case, w=np.random.default_rng(9).lognormal(0.0, 0.5, 1025))


@pytest.mark.parametrize("mistake", ["phase_sign", "env_4pi2", "xz_factor", "no_weight", "lam_identity",
                                     "accept_le", "fixed_moves"])
def test_planted_mistakes_are_outside_the_bounds(mistake):
    """The opposite phase sign, 4 pi^2 for 2 pi^2 and a dropped weight (chi^2 of the first trial), a
    missing factor 2 on the sxz derivative and lambda I for lambda diag N (the first step's backward
    error), an accept on <= (a trial with the bits of chi^2_cur, which the strict rule rejects: it
    needs a fit that goes on into such ties, noisy data and an xtol of 1e-13) and a fixed parameter
    that moves."""
    case = _mistake_case(mistake)
    xtol = 1e-13 if mistake == "accept_le" else XTOL
    args, out = emulate(case, 0, xtol=xtol, mistake=mistake)
    assert out["status"] != 3
    with pytest.raises(AssertionError):
        follow(args, out, xtol=xtol)
    # the same case without the mistake is followed
    args, good = emulate(case, 0, xtol=xtol)
    assert follow(args, good, xtol=xtol) <= 1.0


def test_tampered_outputs_are_caught():
    case = C.sized(1025, 2, noise=0.01)
    args, good = emulate(case, 0)
    follow(args, good)

    def tampered(**change):
        bad = dict(good, trace=good["trace"].copy(), cov=good["cov"].copy())
        for k, f in change.items():
            bad[k] = f(bad[k])
        with pytest.raises(AssertionError):
            follow(args, bad)

    def edit(i, j, v):
        def f(a):
            a[i, j] = v if not callable(v) else v(a[i, j])
            return a
        return f
    tampered(trace=edit(3, 1, lambda x: 2 * x))                   # a lambda off the sequence
    tampered(trace=edit(good["niter"], 0, 1.0))                   # a row beyond d_niter written
    tampered(trace=edit(2, 2, 0.0))                               # a clearly better trial rejected
    tampered(trace=edit(1, 0, lambda x: x * (1 + 1e-9)))          # chi^2 outside its bound
    tampered(nvis=lambda n: n - 1)
    tampered(cov=lambda c: c * (1 + 1e-9))
    tampered(status=lambda s: 0)
    tampered(theta=lambda t: t * (1 + 1e-15))
    tampered(chi2=lambda c: np.nextafter(c, 1.0))


def test_the_step_scale():
    s = K.scales([0.0, 1.0, 1.0, 0.1, 0.0, 0.2, -2.5, 0, 0, 3.0, 1.0, 4.0])
    assert float(s[0]) == 1e-300 and float(s[3]) == float(s[4]) == float(s[5]) == 1.0
    assert float(s[6]) == 2.5 and float(s[9]) == float(s[11]) == 7.0 and float(s[7]) == 1.0
    assert K.psd([1, 0, 0, 0, 0, 0]) and K.psd([1, 0, 0, 1, 1, 1]) and not K.psd([1, 0, 0, 1, 1.01, 1])
    assert not K.psd([1, 0, 0, -1e-9, 0, 1]) and not K.psd([1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 2, 1])


# ---- the host helpers ------------------------------------------------------------------------------
CELL = np.radians(0.05 / 3600.)


def test_uvfit_theta_round_trips_and_conventions():
    th = E.uvfit_theta(2.0, 0.1, -0.2, 0.5, 0.25, 30., CELL)
    assert th[0] == 2.0 and abs(th[1] + 2.0) <= 1e-12 and abs(th[2] + 4.0) <= 1e-12     # East = -x
    back = E.uvfit_components(th, CELL)
    assert np.allclose(back, (2.0, 0.1, -0.2, 0.5, 0.25, 30.), rtol=0, atol=1e-11)
    # Sigma = (2 Q)^-1 of beam_quadratic's form: the same ellipse in both planes
    A, B, Cq = E.beam_quadratic(0.5, 0.25, 30., CELL)
    sig = np.linalg.inv(2 * np.array([[A, B], [B, Cq]]))
    assert np.allclose([th[3], th[4], th[5]], [sig[0, 0], sig[0, 1], sig[1, 1]], rtol=1e-12, atol=0)
    # pa = 0: the major axis along z (North); pa = 90: along -x (East)
    n = E.uvfit_theta(1.0, 0, 0, 0.4, 0.1, 0., CELL)
    e = E.uvfit_theta(1.0, 0, 0, 0.4, 0.1, 90., CELL)
    assert n[5] > n[3] and abs(n[4]) <= 1e-15 and e[3] > e[5]
    for pa in (-89., -20., 0., 45., 90.):
        assert abs(E.uvfit_components(E.uvfit_theta(1, 0, 0, 0.3, 0.2, pa, CELL), CELL)[5] - pa) <= 1e-9
    p = E.uvfit_theta(3.0, 0.05, 0.05, 0., 0., 0., CELL)
    assert list(p[3:]) == [0., 0., 0.] and E.uvfit_components(p, CELL)[3:] == (0., 0., 0.)
    with pytest.raises(ValueError):
        E.uvfit_theta(1, 0, 0, -1., 0., 0., CELL)
    with pytest.raises(ValueError):
        E.uvfit_components([1, 0, 0, 1.0, 2.0, 1.0], CELL)
    # from an imfit result: the deconvolved size, or a point
    fit = {"I": {"val": 1.5, "unit": "Jy"}, "east_as": 0.1, "north_as": -0.2, "point_source": False,
           "deconvolved": {"maj_as": 0.5, "min_as": 0.25, "pa_deg": 30.}}
    assert np.allclose(E.uvfit_theta_from_imfit(fit, CELL), E.uvfit_theta(1.5, 0.1, -0.2, 0.5, 0.25, 30., CELL))
    pt = dict(fit, deconvolved=None, point_source=True)
    assert list(E.uvfit_theta_from_imfit(pt, CELL)[3:]) == [0., 0., 0.]
    with pytest.raises(ValueError):
        E.uvfit_theta_from_imfit({"I": {"val": 1.0}}, CELL)


def test_uvfit_results_errors_by_hand():
    """C = N^-1 over the free parameters of a hand-made N; reduced chi^2 = chi^2 / (2 nvis - n_free)
    and the sqrt(reduced chi^2) scaling; a fixed parameter has the error 0."""
    th = E.uvfit_theta(2.0, 0.1, -0.2, 0.5, 0.25, 30., CELL)
    n = np.array([400., 90., 70., 5e2, 7e2, 3e2])
    N = np.diag(n)
    N[0, 3] = N[3, 0] = 100.
    cov = K.pack(N)
    cell_as = 0.05
    r = E.uvfit_results([th], [cov], [30.0], [13], None, CELL, status=[1], scale_errors=False)[0][0]
    Cm = np.linalg.inv(N)
    assert abs(r["Ierr"]["val"] - np.sqrt(Cm[0, 0])) <= 1e-15 and r["I"] == {"val": 2.0, "unit": "Jy"}
    assert abs(r["east_err_as"] - np.sqrt(Cm[1, 1]) * cell_as) <= 1e-15
    assert abs(r["north_err_as"] - np.sqrt(Cm[2, 2]) * cell_as) <= 1e-15
    assert np.allclose(r["sigma_err"], np.sqrt(np.diag(Cm)[3:]), rtol=1e-13, atol=0)
    assert r["reduced_chi2"] == 30.0 / (26 - 6) and r["nvis"] == 13 and r["status"] == 1 and r["chi2"] == 30.0
    assert abs(r["east_as"] - 0.1) <= 1e-12 and abs(r["maj_as"] - 0.5) <= 1e-11 and not r["point_source"]
    # first-order errors of the axes against a central difference of uvfit_components
    for name, k in (("maj_err_as", 3), ("min_err_as", 4), ("pa_err_deg", 5)):
        g = np.zeros(3)
        for j in range(3):
            h = 1e-6 * max(abs(th[3 + j]), 1.0)
            lo, hi = th.copy(), th.copy()
            lo[3 + j] -= h
            hi[3 + j] += h
            g[j] = (E.uvfit_components(hi, CELL)[k] - E.uvfit_components(lo, CELL)[k]) / (2 * h)
        want = np.sqrt(g @ Cm[3:, 3:] @ g)
        assert abs(r[name] - want) <= 1e-6 * want, name
    # scaled by sqrt(reduced chi^2)
    s = E.uvfit_results([th], [cov], [30.0], [13], None, CELL)[0][0]
    assert abs(s["Ierr"]["val"] - np.sqrt(1.5) * r["Ierr"]["val"]) <= 1e-15
    # fixed sizes (a point): identity rows, the inverse over the free block alone, no size errors
    free = [1, 1, 1, 0, 0, 0]
    Nf = np.eye(6)
    Nf[:3, :3] = [[4., 1., 0.], [1., 9., 0.], [0., 0., 16.]]
    pt = np.array([2.0, 1.0, 1.0, 0., 0., 0.])
    f = E.uvfit_results([pt], [K.pack(Nf)], [8.0], [5], free, CELL, scale_errors=False)[0][0]
    Cf = np.linalg.inv(Nf[:3, :3])
    assert abs(f["Ierr"]["val"] - np.sqrt(Cf[0, 0])) <= 1e-15 and f["sigma_err"] == (0., 0., 0.)
    assert f["point_source"] and f["maj_err_as"] is None and f["reduced_chi2"] == 8.0 / 7
    # two components; no degree of freedom; a map that was not fitted
    two = E.uvfit_results([np.r_[th, pt]], [K.pack(np.eye(12))], [1.0], [6], None, CELL)[0]
    assert len(two) == 2 and np.isnan(two[0]["reduced_chi2"]) and two[0]["Ierr"]["val"] is None
    bad = E.uvfit_results([[np.nan] * 6], [[np.nan] * 21], [np.nan], [-1], None, CELL, status=[3])[0][0]
    assert np.isnan(bad["I"]["val"]) and bad["Ierr"]["val"] is None and bad["status"] == 3
    with pytest.raises(ValueError):
        E.uvfit_results([th], [cov], [1.0], [9], [1, 1], CELL)


def test_uvfit_start_on_host_tensors():
    rng = np.random.default_rng(6)
    u, v = rng.uniform(-0.2, 0.2, 400), rng.uniform(-0.2, 0.2, 400)
    u[0] = v[0] = 0.0
    truth = np.array([[1.3, 0.4, -0.3, 4.0, 0.0, 4.0], [0.6, 0.0, 0.0, 0.0, 0.0, 0.0]])
    su, sv = np.array([1.0, -0.9]), np.array([1.0, 1.1])
    V = np.stack([C.analytic(truth[m], su[m] * u, sv[m] * v) for m in range(2)])
    V = np.concatenate([V, np.full((1, 400), np.nan + 0j)])
    th = E.uvfit_start(torch.from_numpy(V), np.r_[su, 1.0], np.r_[sv, 1.0], torch.from_numpy(u),
                       torch.from_numpy(v)).numpy()
    assert th.shape == (3, 6) and np.all(th[:, [1, 2, 4]] == 0) and np.all(th[:, 3] == th[:, 5])
    # a circular Gaussian at (almost) the phase centre: |V| falls off as the straight line assumes
    assert abs(th[0, 0] - 1.3) <= 1e-9 and abs(th[0, 3] - 4.0) <= 1e-8
    assert abs(th[1, 0] - 0.6) <= 1e-12 and abs(th[1, 3]) <= 1e-9   # a point: no fall-off, size 0
    assert np.isnan(th[2, 0])                                       # no counting visibility
    # the start is good enough for the emulation to converge from
    data = K.counting(V[0], su[0] * u, sv[0] * v, None)
    out = K.emulate(data, 400, th[0], None, LAM0, XTOL, N_ITER)
    assert out["status"] == 1 and np.max(np.abs(out["theta"] - truth[0])) <= 1e-9
    # weights: a zero weight takes a visibility -- here a wild one at the origin -- out
    w = np.ones(400)
    w[0] = 0.0
    V[0, 0] = 100.0
    args = (np.r_[su, 1.0], np.r_[sv, 1.0], torch.from_numpy(u), torch.from_numpy(v))
    Vr = torch.view_as_real(torch.from_numpy(V)).contiguous()
    assert abs(E.uvfit_start(Vr, *args).numpy()[0, 0] - 1.3) > 0.1
    assert abs(E.uvfit_start(Vr, *args, torch.from_numpy(w)).numpy()[0, 0] - 1.3) <= 1e-9


# ---- the ABI ---------------------------------------------------------------------------------------
def test_abi_signatures_and_the_workspace_query():
    res, args = _lib.SIGNATURES["rjp_uvfit"]
    P, i32, dbl, DP = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.POINTER(ctypes.c_double)
    assert res is ctypes.c_int64
    assert args == [P, P, i32, i32, DP, DP, P, P, P, i32, i32, ctypes.POINTER(ctypes.c_uint8), P, dbl, dbl,
                    i32, P, P, P, P, P, P, P, ctypes.c_size_t, P]
    assert _lib.SIGNATURES["rjp_uvfit_workspace"] == (ctypes.c_size_t, [i32, i32, i32])
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    assert "int64_t rjp_uvfit(rjp_ctx* ctx, const double* d_vis, int32_t n_maps, int32_t n_vis," in hdr
    assert "size_t rjp_uvfit_workspace(int32_t n_maps, int32_t n_vis, int32_t n_comp);" in hdr
    assert "#define RJP_UVFIT_MAX_COMP 2" in hdr and "#define RJP_VERSION 117" in hdr
    assert imaging.UVFIT_MAX_COMP == K.MAX_COMP == 2
    lib = _lib.load()
    for n_maps, nv in ((1, 1), (3, 15), (1, 1024), (1, 1025), (64, 65536), (2, 262145), (7, 2 ** 31 - 1)):
        for nc in (1, 2):
            assert lib.rjp_uvfit_workspace(n_maps, nv, nc) == K.workspace_bytes(n_maps, nv, nc), (n_maps, nv, nc)
    for bad in ((0, 15, 1), (1, 0, 1), (-1, 15, 1), (1, -5, 2), (1, 15, 0), (1, 15, 3)):
        assert lib.rjp_uvfit_workspace(*bad) == 0, bad
    # a NULL context is refused before anything else
    assert lib.rjp_uvfit(None, None, 1, 1, None, None, None, None, None, 1, 1, None, None, 1e-3, 1e-10, 1,
                         None, None, None, None, None, None, None, 0, None) == _lib.RJP_ERR_ARG


def test_check_uvfit_from_plain_cpp(tmp_path):
    """check_uvfit compiled into a stand-alone program by plain g++ (tests/rjp_args_uvfit_cases.cpp):
    every refusal, status and message, in the order the check makes them -- the messages
    tests/test_gpu_uvfit.py sees from the library."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "rjp_args_uvfit_cases"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rajepy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rjp_args_uvfit_cases.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        case, status, msg = line.split("\t")
        got[case] = (int(status), msg)
    want = {"nulls": ["NULL d_vis", "NULL h_su", "NULL h_sv", "NULL d_u", "NULL d_v", "NULL d_theta",
                      "NULL d_chi2", "NULL d_cov", "NULL d_nvis", "NULL d_niter", "NULL d_status",
                      "NULL beats sizes"],
            "sizes": ["n_maps 0", "n_vis 0", "n_vis -1", "sizes beat n_comp"],
            "comp": ["n_comp 0", "n_comp 3", "n_comp beats w_maps"],
            "wmaps": ["w_maps 0", "w_maps 3", "w_maps beats the scales"],
            "scale": ["su nan", "sv inf", "scales beat free"],
            "free": ["no free parameter", "no free parameter among the first six", "free beats lambda0"],
            "tol": ["lambda0 0", "lambda0 inf", "lambda0 nan", "xtol -1", "xtol inf", "xtol nan",
                    "lambda0 beats n_iter"],
            "iter": ["n_iter 0", "n_iter beats the workgroups"],
            "wgs": ["1025 x 2^21 workgroups"]}
    seen = set()
    for key, cases in want.items():
        for case in cases:
            assert got[case] == (_lib.RJP_ERR_ARG, K.MSG[key]), case
            seen.add(case)
    valid = {c for c in got if c.startswith("valid")}
    assert len(valid) == 4 and all(got[c] == (0, "") for c in valid)
    assert seen | valid == set(got)


# ---- the Python paths on a recording engine -----------------------------------------------------------
class _NoHost(torch.Tensor):
    """A tensor that must stay where it is."""

    def cpu(self, *a, **k):
        raise AssertionError("visibilities must not be copied to the host")

    numpy = tolist = __array__ = cpu


class _Maps:
    """A stack of maps that is never looked into."""

    def __init__(self, n_maps, npix):
        self.shape = (n_maps, npix)

    def reshape(self, *shape):
        assert shape[0] == self.shape[0]
        return self


class _RecordingEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls, self.to_host = [], False

    def _device_f64(self, values):
        if isinstance(values, torch.Tensor):
            return values.reshape(-1)
        return torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64).reshape(-1))

    def vis(self, maps, nx, nz, su, sv, u, v):
        self.calls.append(dict(kind="vis", n_maps=maps.shape[0]))
        M, Kn = maps.shape[0], u.numel()
        V = torch.complex(torch.arange(M * Kn, dtype=torch.float64).reshape(M, Kn) + 1000.0 * len(self.calls),
                          torch.ones(M, Kn, dtype=torch.float64))
        return V if self.to_host else V.as_subclass(_NoHost)

    def ff_formal_sweep(self, fields, bursts, epochs_s, gff_mode, ctau, csrc, want_maps=False, want_totals=True):
        self.calls.append(dict(kind="sweep", epochs=list(epochs_s)))
        return _Maps(len(epochs_s) * len(ctau), fields.npix), None

    def uvfit(self, vis, su, sv, u, v, theta0, weights=None, free=None, n_iter=60, lambda0=1e-3, xtol=1e-10,
              trace=False):
        assert isinstance(vis, _NoHost) and not trace
        M, Kn = vis.shape
        th = torch.as_tensor(theta0, dtype=torch.float64)
        th = th.reshape(1, -1).expand(M, -1) if th.dim() == 1 else th
        P = th.shape[1]
        self.calls.append(dict(kind="uvfit", M=M, K=Kn, su=np.array(su), sv=np.array(sv), u=u, v=v,
                               theta0=th.clone(), weights=weights, free=free, n_iter=n_iter,
                               first=complex(torch.Tensor(torch.view_as_real(vis))[0, 0, 0], 1.0)))
        return dict(theta=th.clone(), chi2=torch.ones(M, dtype=torch.float64),
                    cov=torch.from_numpy(np.tile(K.pack(np.eye(P)), (M, 1))),
                    nvis=torch.full((M,), Kn, dtype=torch.int32), niter=torch.ones(M, dtype=torch.int32),
                    status=torch.ones(M, dtype=torch.int32))


class _Fields:
    def __init__(self, npix):
        self.npix = npix


def _model(nx, nz):
    from rajepy_amd import classes
    J = classes.JetModel

    class Model:
        SCAN_CACHE_EPOCHS = J.SCAN_CACHE_EPOCHS
        VIS_STACK_BYTES = J.VIS_STACK_BYTES
        _vis_scales, _vis_chunk, _channel_coeffs = J._vis_scales, J._vis_chunk, J._channel_coeffs
        _imager = J._imager
        visibilities_vs_time = J.visibilities_vs_time
        uvmodelfit, uvmodelfit_vs_time = J.uvmodelfit, J.uvmodelfit_vs_time

    m = Model()
    m.engine, m.nx, m.nz, m.csize = _RecordingEngine(), nx, nz, 0.5
    m.params = {"target": {"dist": 120.}, "properties": {"T_0": 1e4}}
    m.gff_mode, m._dtype = E.RJP_GFF_POWERLAW, _lib.RJP_F64
    m.device_fields = _Fields(nx * nz)
    m._rjp_bursts = lambda: None
    return m


def test_uvmodelfit_vs_time_is_one_uvfit_call_per_chunk():
    nx = nz = 2048                                      # 32 MiB per map: 3 channels -> 10 epochs per GiB
    m = _model(nx, nz)
    times = np.arange(23, dtype=np.float64) * 0.1 * 31557600.0
    freqs = np.array([5e9, 2e10, 4e10])
    u, v = np.array([0., 100., -3e3, 2e4]), np.array([0., -50., 1e3, 1e4])
    th0 = np.arange(23 * 3 * 6, dtype=np.float64).reshape(23, 3, 6) * 1e-3
    th0[..., 3:] = [2.0, 0.1, 3.0]
    w = np.arange(1., 13.).reshape(3, 4)
    out = m.uvmodelfit_vs_time(times, u, v, freqs, formal=True, theta0=th0, weights=w, cell_as=0.01,
                               free=[1, 1, 1, 0, 1, 1], n_iter=17)
    calls = m.engine.calls
    assert [c["kind"] for c in calls] == ["sweep", "vis", "uvfit"] * 3
    fits = [c for c in calls if c["kind"] == "uvfit"]
    assert [c["M"] for c in fits] == [30, 30, 9] and all(c["K"] == 4 and c["n_iter"] == 17 for c in fits)
    su, sv = E.image_scales(freqs, np.radians(0.01 / 3600.))
    for c, (e0, n) in zip(fits, ((0, 10), (10, 10), (20, 3))):
        assert np.array_equal(c["su"], np.tile(su, n)) and np.array_equal(c["sv"], np.tile(sv, n))
        assert np.array_equal(c["theta0"].numpy(), th0[e0:e0 + n].reshape(n * 3, 6))
        assert np.array_equal(c["weights"].numpy().reshape(n, 3, 4), np.broadcast_to(w, (n, 3, 4)))
        assert list(c["free"]) == [True, True, True, False, True, True]
        assert c["u"].tolist() == list(u) and c["v"].tolist() == list(v)
    # results indexed [E][F][component], in the order of the epochs
    assert len(out) == 23 and all(len(e) == 3 and len(e[0]) == 1 for e in out)
    assert out[0][0][0]["theta"][0] == th0[0, 0, 0] and out[22][2][0]["theta"][1] == th0[22, 2, 1]
    assert out[11][1][0]["nvis"] == 4 and out[11][1][0]["status"] == 1
    # no epochs: no call; two components without a start: refused before any call
    m2 = _model(4, 4)
    assert m2.uvmodelfit_vs_time([], u, v, freqs, formal=True) == [] and m2.engine.calls == []
    with pytest.raises(ValueError):
        m2.uvmodelfit_vs_time(times, u, v, freqs, formal=True, comps=2)
    assert m2.engine.calls == []
    # the existing sweep makes no fit
    m2.engine.to_host = True
    m2.visibilities_vs_time(times[:2], u, v, freqs, formal=True)
    assert [c["kind"] for c in m2.engine.calls] == ["sweep", "vis"]


def test_uvmodelfit_mfs_concatenates_the_channels():
    m = _model(8, 8)
    freqs = np.array([5e9, 2e10])
    u, v = np.array([0., 100., -3e3]), np.array([0., -50., 1e3])
    V = torch.complex(torch.arange(6, dtype=torch.float64).reshape(2, 3), torch.ones(2, 3, dtype=torch.float64))
    V = V.as_subclass(_NoHost)
    th0 = [1.0, 0.0, 0.0, 2.0, 0.0, 2.0]
    res = m.uvmodelfit(V, u, v, freqs, weights=[1., 2., 3.], cell_as=0.01, theta0=th0, mfs=True)
    (c,) = m.engine.calls
    su, sv = E.image_scales(freqs, np.radians(0.01 / 3600.))
    assert c["kind"] == "uvfit" and (c["M"], c["K"]) == (1, 6) and list(c["su"]) == list(c["sv"]) == [1.0]
    assert np.array_equal(c["u"].numpy(), np.outer(su, u).reshape(-1))
    assert np.array_equal(c["v"].numpy(), np.outer(sv, v).reshape(-1))
    assert c["weights"].tolist() == [1., 2., 3., 1., 2., 3.] and c["free"] is None
    assert len(res) == 1 and len(res[0]) == 1 and res[0][0]["nvis"] == 6
    # per channel without mfs: one call for both channels; a point component: sizes held at 0
    m.engine.calls.clear()
    res = m.uvmodelfit(V, u, v, freqs, cell_as=0.01, theta0=th0, comptype="P", free=[1, 0, 1, 1, 1, 1])
    (c,) = m.engine.calls
    assert (c["M"], c["K"]) == (2, 3) and np.array_equal(c["su"], su) and c["weights"] is None
    assert list(c["free"]) == [True, False, True, False, False, False]
    assert c["theta0"][:, 3:].abs().max() == 0 and len(res) == 2 and res[0][0]["point_source"]
    for bad in (dict(comps=3), dict(comps=2, theta0=None), dict(comptype="X"), dict(free=[0] * 6),
                dict(free=[1] * 5), dict(weights=[1., 2.])):
        with pytest.raises(ValueError):
            m.uvmodelfit(V, u, v, freqs, **dict(dict(cell_as=0.01, theta0=th0), **bad))
    with pytest.raises(ValueError):
        m.uvmodelfit(V, u[:2], v[:2], freqs, theta0=th0)


def test_public_surface_new_methods_only():
    from rajepy_amd import classes
    J = classes.JetModel
    assert list(inspect.signature(E.RTEngine.uvfit).parameters) == [
        "self", "vis", "su", "sv", "u", "v", "theta0", "weights", "free", "n_iter", "lambda0", "xtol", "trace"]
    p = inspect.signature(E.RTEngine.uvfit).parameters
    assert (p["n_iter"].default, p["lambda0"].default, p["xtol"].default, p["trace"].default) == (60, 1e-3, 1e-10, False)
    assert list(inspect.signature(J.uvmodelfit).parameters) == [
        "self", "vis", "u_m", "v_m", "freq", "weights", "cell_as", "comps", "comptype", "theta0", "free", "mfs",
        "n_iter"]
    assert list(inspect.signature(J.uvmodelfit_ff).parameters)[:5] == ["self", "u_m", "v_m", "freq", "formal"]
    assert list(inspect.signature(J.uvmodelfit_vs_time).parameters)[:6] == [
        "self", "times_s", "u_m", "v_m", "freq", "formal"]
    assert list(inspect.signature(E.uvfit_theta).parameters) == [
        "flux", "east_as", "north_as", "maj_as", "min_as", "pa_deg", "cell_rad"]
    assert list(inspect.signature(E.uvfit_results).parameters) == [
        "theta", "cov", "chi2", "nvis", "free", "cell_rad", "status", "scale_errors"]
    assert list(inspect.signature(E.uvfit_start).parameters) == ["vis", "su", "sv", "u", "v", "weights"]
    for name in ("clean_image_ff", "observe_ff", "dirty_image_ff", "visibilities_vs_time"):
        assert "uvfit" not in inspect.getsource(getattr(J, name))
