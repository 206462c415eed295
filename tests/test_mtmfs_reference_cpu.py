"""tests/mtmfs_ref.py -- the long-double reference that judges rjp_mtmfs (K19) in
tests/test_gpu_mtmfs.py -- held to hand-worked cases, to a float64 emulation of the device's chains on
every GPU case's inputs (inside the bounds) and to planted mistakes (outside); the host helpers
`taylor_weights` and `taylor_hessian_inverse`; check_mtmfs from plain C++; the ABI; and the public
surface (`nterms`, `reffreq_hz`, `alpha_cut_jy`, `CleanResult.taylor`) on a recording engine.  No GPU."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from rajepy_amd import _lib, imaging
from tests import clean_ref as C
from tests import mtmfs_cases as MC
from tests import mtmfs_ref as K
from tests import test_msclean_reference_cpu as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
POISON_PIX, POISON_F = -77, 7.25
NU0 = 5e9


# ---- the host helpers ---------------------------------------------------------------------------------
def test_taylor_weights():
    f = np.array([3e9, 4e9, 5e9, 4.4e9])
    tw = imaging.taylor_weights(f, 4e9, 4)
    w = (f - 4e9) / 4e9
    assert tw.shape == (4, 4) and np.all(tw[0] == 1.0) and np.array_equal(tw[1], w)
    assert np.array_equal(tw[2], w * w) and np.array_equal(tw[3], w * w * w)
    assert list(tw[:, 0]) == [1.0, -0.25, 0.0625, -0.015625] and not tw[1:, 1].any()
    assert imaging.taylor_weights(5e9, 5e9, 1).shape == (1, 1)
    from rajepy_amd import engine as E
    assert E.taylor_weights is imaging.taylor_weights
    assert E.taylor_hessian_inverse is imaging.taylor_hessian_inverse
    for bad in (lambda: imaging.taylor_weights(f, 0.0, 2), lambda: imaging.taylor_weights(f, np.nan, 2),
                lambda: imaging.taylor_weights(f, 4e9, 0), lambda: imaging.taylor_weights([1e9, np.inf], 4e9, 2)):
        with pytest.raises(ValueError):
            bad()


def test_hessian_inverse_by_hand_and_the_narrow_band_refusal():
    """w = (-1/4, 0, 1/4): the moments are m_0 = 1, m_2 = 2 (1/16) / 3 = 1/24, m_4 = 2 (1/256) / 3 = 1/384,
    the odd ones 0.  Two terms: H = diag(1, 1/24), Hinv = diag(1, 24).  Three terms: H = [[1, 0, m_2],
    [0, m_2, 0], [m_2, 0, m_4]]; the (0, 2) block has determinant m_4 - m_2^2 = 1/384 - 1/576 = 1/1152, so
    Hinv_00 = 1152 m_4 = 3, Hinv_02 = -1152 m_2 = -48, Hinv_22 = 1152, Hinv_11 = 24."""
    tw = imaging.taylor_weights([3e9, 4e9, 5e9], 4e9, 5)
    c = tw.mean(axis=1)
    assert np.allclose(c, [1, 0, 1 / 24, 0, 1 / 384], rtol=1e-15, atol=0)
    H, Hinv = imaging.taylor_hessian_inverse(c[:3])
    assert np.array_equal(H, [[1.0, 0.0], [0.0, c[2]]]) and np.allclose(Hinv, [[1, 0], [0, 24]], rtol=1e-15)
    H, Hinv = imaging.taylor_hessian_inverse(c)
    assert np.array_equal(H, [[1, 0, c[2]], [0, c[2], 0], [c[2], 0, c[4]]])
    assert np.allclose(Hinv, [[3, 0, -48], [0, 24, 0], [-48, 0, 1152]], rtol=1e-12, atol=1e-12)
    assert np.array_equal(Hinv, Hinv.T)
    H, Hinv = imaging.taylor_hessian_inverse([2.0])
    assert H.shape == (1, 1) and Hinv[0, 0] == 0.5
    # a band of 2e-7 of the frequency: m_2 = 2e-14 / 3, the condition number 1.5e14 > 1e10
    narrow = imaging.taylor_weights(NU0 * (1 + np.array([-1e-7, 0.0, 1e-7])), NU0, 3).mean(axis=1)
    with pytest.raises(ValueError, match="too narrow for nterms = 2"):
        imaging.taylor_hessian_inverse(narrow)
    assert imaging.TAYLOR_COND_MAX == 1e10
    # one frequency, two terms: H = [[1, 0], [0, 0]]; two frequencies, three terms: singular
    with pytest.raises(ValueError, match="positive definite"):
        imaging.taylor_hessian_inverse([1.0, 0.0, 0.0])
    with pytest.raises(ValueError):
        imaging.taylor_hessian_inverse(imaging.taylor_weights([4e9, 6e9], 5e9, 5).mean(axis=1))
    for bad in ([1.0, 0.0], [], [1.0, np.nan, 1.0]):
        with pytest.raises(ValueError):
            imaging.taylor_hessian_inverse(bad)


# ---- hand-worked: one source with a spectrum linear in w ---------------------------------------------------
def linear_source(tw_fn, nx=9, nz=7, at=(5, 2), coef=(0.75, -0.5), seed=3):
    """One on-grid source I(nu) = I_0 + I_1 w seen channel by channel through the channels' own beams,
    imaged into Taylor planes with the weights `tw_fn(freqs, nu_0, n)` -> (R0, B, H, Hinv)."""
    rng = np.random.default_rng(seed)
    w = K.BAND_W
    freqs = NU0 * (1.0 + w)
    px, pz = 2 * nx - 1, 2 * nz - 1
    cb = K.channel_beams(rng, px, pz, w)
    tw = tw_fn(freqs, NU0, 3)
    B, H, Hinv = K.spectral_beams(rng, 2, px, pz, w, tw=tw, channels=cb)
    flux = coef[0] + coef[1] * w                                  # the TRUE spectrum, in the true w
    R0 = np.zeros((2, nx, nz))
    im, bm = C.window(nx, nz, px, pz, at[0], at[1])
    for t in range(2):
        for f in range(len(w)):
            R0[t][im] += tw[t, f] * flux[f] * cb[f][bm] / len(w)
    return R0, B, H, Hinv


def test_one_source_linear_in_w_by_hand():
    """gain = 1, n_t = 2: R_t = I_0 B_t + I_1 B_{t+1} shifted to the source, so at the source R = H (I_0, I_1)
    and one iteration returns (I_0, I_1) and empties both planes.  The planes are sums of 8 float64
    products (9 u each), Hinv is a float64 inverse (cond u): the coefficients are within
    16 cond(H) u (|I_0| + |I_1|), and so is what is left of the planes (|B| <= 1)."""
    I = (0.75, -0.5)
    R0, B, H, Hinv = linear_source(imaging.taylor_weights, coef=I)
    cpix, ccoef, R = K.mtmfs(R0, B, Hinv, None, 0.0, 1.0, 1)
    tol = 16 * np.linalg.cond(H) * K.U * (abs(I[0]) + abs(I[1]))
    assert list(cpix) == [5 * 7 + 2]
    assert abs(float(ccoef[0, 0]) - I[0]) <= tol and abs(float(ccoef[0, 1]) - I[1]) <= tol
    assert float(np.abs(R).max()) <= 2 * tol and tol < 1e-12
    # the same through `follow`, as the device would be judged
    res = R.astype(np.float64)
    K.follow(R0, B, Hinv, None, 0.0, 1.0, 1, cpix, ccoef.astype(np.float64), 1, res, roundings=2)
    # w = nu / nu_0 in taylor_weights: a consistent expansion about nu = 0, whose term 0 is the flux
    # extrapolated to zero frequency, I_0 - I_1 -- not the flux at the reference frequency
    wrong = lambda f, nu0, n: K.band_weights(np.asarray(f) / nu0, n)
    R0w, Bw, Hw, Hinvw = linear_source(wrong, coef=I)
    _, cw, _ = K.mtmfs(R0w, Bw, Hinvw, None, 0.0, 1.0, 1)
    assert abs(float(cw[0, 0]) - I[0]) > 1e6 * tol
    assert np.allclose(Hinvw @ R0w[:, 5, 2], [I[0] - I[1], I[1]], rtol=0, atol=1e-9)     # at the source itself


def test_one_term_reproduces_clean_ref():
    rng = np.random.default_rng(11)
    nx, nz, px, pz = 13, 9, 25, 17
    B = C.random_beam(rng, px, pz)
    D = C.random_image(rng, nx, nz, B)
    D[3, 3] = np.nan
    mask = MC.box(nx, nz)
    for dtype in (LD, np.float64):
        a = C.hogbom(D, B, mask, 1e-3, 0.2, 40, dtype=dtype)
        b = K.mtmfs(D[None], B[None], [[1.0]], mask, 1e-3, 0.2, 40, dtype=dtype)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1][:, 0]) and len(a[0]) > 5
        assert np.array_equal(a[2], b[2][0], equal_nan=True)
    assert K.workspace_bytes(3, 1, 67, 131) == C.workspace_bytes(3, 67, 131)      # one term: K12's


# ---- the emulation on every GPU case's inputs; non-vacuity ------------------------------------------------
def emulate(case, m, **switches):
    """The float64 emulation of map m of a case -> what `follow` takes (rows padded with poison)."""
    R0 = case["R0"][m]
    B = case["B"][m if case["B"].shape[0] > 1 else 0]
    n_iter, n_t = case["n_iter"], case["n_t"]
    cpix, ccoef, R = K.mtmfs(R0, B, case["hinv"][m], case["mask"], case["thresh"][m], case["gain"], n_iter,
                             dtype=np.float64, **switches)
    n = len(cpix)
    rows_p = np.concatenate([cpix, np.full(n_iter - n, POISON_PIX)])
    rows_c = np.concatenate([ccoef.astype(np.float64), np.full((n_iter - n, n_t), POISON_F)])
    return R0, B, rows_p, rows_c, n, R.astype(np.float64)


def judge(case, m, out, roundings=2):
    R0, B, rows_p, rows_c, n, res = out
    worst = K.follow(R0, B, case["hinv"][m], case["mask"], case["thresh"][m], case["gain"], case["n_iter"],
                     rows_p, rows_c, n, res, poison_pix=POISON_PIX, poison_coef=POISON_F, roundings=roundings)
    worst["identity"] = K.conservation(R0, B, rows_p, rows_c, n, res, roundings=roundings)
    return worst


@pytest.mark.parametrize("name", MC.NAMES)
def test_float64_emulation_inside_the_bounds_and_non_vacuity(name):
    case = MC.build(name)
    M, n_t, nx, nz = case["R0"].shape
    for m in range(M):
        out = emulate(case, m)
        worst = judge(case, m, out)
        assert all(v <= 1.0 for v in worst.values()), worst
        # the reference alone (long double, free-running) finds something to do in every live map
        cpix, ccoef, _ = K.mtmfs(case["R0"][m], case["B"][m if case["B"].shape[0] > 1 else 0], case["hinv"][m],
                                 case["mask"], case["thresh"][m], case["gain"], case["n_iter"])
        if not case["live"][m]:
            assert len(cpix) == 0 and out[4] == 0
            continue
        assert len(cpix) >= 3, (name, m, len(cpix))
        if nx * nz > K.TILE:
            assert (cpix >= K.TILE).any(), "no component outside tile 0"
    if name == "67x131 full":
        assert emulate(case, 0)[4] < case["n_iter"] == emulate(case, 1)[4]     # map 0 stops early, map 1 runs on
    if name == "31x33 odd npix":
        assert (nx * nz) % 2 == 1 and np.isnan(case["R0"][0, 1]).sum() == 1 and not np.isnan(case["R0"][0, 0]).any()


def crossing():
    """`two sources with crossing spectra`: A = (1.0, -1.0) and B = (0.95, +0.95) on 31 x 33 with two
    terms and the band's first moment 0.1: R_0 is larger at B (1.045 against 0.9), a_0 at A."""
    rng = np.random.default_rng(77)
    nx, nz = 31, 33
    B, H, Hinv = K.spectral_beams(rng, 2, 2 * nx - 1, 2 * nz - 1)
    R0 = K.taylor_planes(rng, nx, nz, B, 2, sources=[(8, 20, [1.0, -1.0]), (21, 6, [0.95, 0.95])])
    return dict(R0=R0[None], B=B[None], hinv=Hinv[None], mask=None, thresh=np.zeros(1), gain=0.1, n_iter=10,
                n_t=2)


def test_planted_mistakes_fall_outside():
    case = crossing()
    assert all(v <= 1.0 for v in judge(case, 0, emulate(case, 0)).values())
    assert abs(case["R0"][0, 0, 21, 6]) > abs(case["R0"][0, 0, 8, 20])            # |R_0| prefers the other source
    first = emulate(case, 0)[2][0]
    assert first == 8 * 33 + 20 and emulate(case, 0, pick_r0=True)[2][0] == 21 * 33 + 6
    for switch in ("beam_abs_diff", "pick_r0", "update_q0_only", "gain_twice", "hinv_row0"):
        with pytest.raises(AssertionError):
            judge(case, 0, emulate(case, 0, **{switch: True}))
    # ... and on a three-term GPU case, where B_{|t-q|} and B_{t+q} differ in more places
    case3 = MC.build("31x33 nt3")
    for switch in ("beam_abs_diff", "update_q0_only", "gain_twice", "hinv_row0"):
        with pytest.raises(AssertionError):
            judge(case3, 0, emulate(case3, 0, **{switch: True}))
    # the follow rule's own teeth: a coefficient off by 1e-9, a tie given to the higher pixel
    R0, B, rows_p, rows_c, n, res = emulate(case, 0)
    bent = rows_c.copy()
    bent[2, 1] *= 1 + 1e-9
    with pytest.raises(AssertionError, match="coefficient 1 of component 2"):
        judge(case, 0, (R0, B, rows_p, bent, n, res))
    tied = MC.build("5x3 nt1")
    R0, B, rows_p, rows_c, n, res = emulate(tied, 0)
    if rows_p[0] == 0:                                            # pixel 0 ties with the last pixel
        swapped = rows_p.copy()
        swapped[0] = 14
        with pytest.raises(AssertionError):
            judge(tied, 0, (R0, B, swapped, rows_c, n, res))


# ---- the ABI ---------------------------------------------------------------------------------------------
def test_abi_signatures_and_header():
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    P, i32, dbl, DP = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.POINTER(ctypes.c_double)
    decl = re.search(r"int64_t rjp_mtmfs\((.*?)\);", hdr, re.S).group(1)
    names = [re.search(r"(\w+)$", p.strip()).group(1) for p in decl.split(",")]
    assert names == ["ctx", "d_res", "n_maps", "n_t", "nx", "nz", "d_spsf", "n_psf", "px", "pz", "h_hinv", "d_mask",
                     "h_thresh", "gain", "n_iter", "d_cpix", "d_ccoef", "d_ncomp", "d_model", "d_peak", "d_work",
                     "work_bytes", "stream"]
    assert "size_t rjp_mtmfs_workspace(int32_t n_maps, int32_t n_t, int32_t nx, int32_t nz);" in hdr
    assert "#define RJP_MTMFS_MAX_NT 4" in hdr and "#define RJP_VERSION 117 " in hdr and _lib.RJP_VERSION == 117
    for text in ("casa/tasks.py:243-246", "a_q = Hinv[q][0] R_0[p]", "fma(Hinv[q][t], R_t[p], a_q)",
                 "c_q = gain a_q(p*) (one product)", "fma(-c_q, B_{t+q}[x - p* + centre], r)",
                 "n_t roundings per update", "Slots at and beyond d_ncomp[m] are not written",
                 "continues the same clean", "rjp_clean's bit for bit", "2 x (8 n_t + 4) bytes per map and tile"):
        assert text in hdr, text
    assert _lib.SIGNATURES["rjp_mtmfs_workspace"] == (ctypes.c_size_t, [i32] * 4)
    res, args = _lib.SIGNATURES["rjp_mtmfs"]
    assert res is ctypes.c_int64
    assert args == [P, P, i32, i32, i32, i32, P, i32, i32, i32, DP, P, DP, dbl, i32, P, P, P, P, P, P,
                    ctypes.c_size_t, P]
    lib = _lib.load()
    assert lib.rjp_version() == 117
    for name in ("rjp_mtmfs_workspace", "rjp_mtmfs"):
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    mk = open(os.path.join(ROOT, "rajepy_amd", "csrc", "Makefile")).read()
    assert "$(OBJDIR)/mtmfs.o" in mk
    assert lib.rjp_mtmfs(None, None, 1, 1, 1, 1, None, 1, 1, 1, None, None, None, 0.1, 1, None, None, None,
                         None, None, None, 0, None) == _lib.RJP_ERR_ARG          # a NULL context, before all else
    ws = lib.rjp_mtmfs_workspace
    for a in ((1, 1, 1, 1), (1, 2, 5, 3), (3, 3, 67, 131), (1, 4, 501, 501), (2, 2, 600, 600), (7, 4, 130, 65)):
        assert ws(*a) == K.workspace_bytes(*a) > 0 and ws(*a) % 16 == 0, a
    assert K.workspace_bytes(1, 2, 67, 131) == 368 > 9 * 2 * 20          # (360, rounded up to 16)
    assert K.workgroups(3, 67, 131) == 27
    for i in range(4):
        for bad in (0, -1):
            a = [3, 2, 67, 131]
            a[i] = bad
            assert ws(*a) == 0
    assert ws(1, 5, 5, 3) == 0                                                  # beyond RJP_MTMFS_MAX_NT
    big = 2 ** 31 - 1
    assert ws(big, 4, big, big) == 0 and ws(big, 1, 46340, 46340) % 16 == 0      # the size overflows / it does not


def test_checks_from_plain_cpp(tmp_path):
    """check_mtmfs compiled into a stand-alone program by plain g++ (tests/rjp_args_mtmfs_cases.cpp): every
    refusal, status and message, in the order the checks make them -- the messages tests/test_gpu_mtmfs.py
    sees from the library."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "rjp_args_mtmfs_cases"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rajepy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rjp_args_mtmfs_cases.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        case, status, msg = line.split("\t")
        got[case] = (int(status), msg)
    want = {"null": ["NULL d_res", "NULL d_spsf", "NULL h_hinv", "NULL h_thresh", "NULL d_cpix", "NULL d_ccoef",
                     "NULL d_ncomp", "NULL beats sizes"],
            "sizes": ["n_maps 0", "n_t 0", "n_t -1", "nx 0", "nz -1", "px 0", "pz 0", "sizes beat n_t"],
            "nt": ["n_t 5", "n_t 2^31 - 1", "n_t beats even"],
            "even": ["px even", "pz even", "even beats n_psf"],
            "npsf": ["n_psf 0", "n_psf 3", "n_psf beats gain"],
            "npix": ["nx nz 2^31"],
            "gain": ["gain 0", "gain 1.5", "gain nan", "gain beats n_iter"],
            "niter": ["n_iter 0", "n_iter beats thresh"],
            "thresh": ["thresh negative", "thresh inf", "thresh beats hinv"],
            "hinv": ["hinv nan", "hinv inf in the last map", "hinv -inf off the diagonal"]}
    seen = set()
    for key, cases in want.items():
        for case in cases:
            assert got[case] == (_lib.RJP_ERR_ARG, K.MSG[key]), case
            seen.add(case)
    valid = {c for c in got if "valid" in c}
    assert len(valid) == 4 and all(got[c] == (0, "") for c in valid)
    assert seen | valid == set(got)


# ---- the Python paths on a recording engine ----------------------------------------------------------
class _Recording(MS._RecordingEngine):
    """vis_adjoint returns the smooth beam-like image of the grid times the sum of the visibilities'
    real parts (so the Taylor-weighted images differ by the band's moments); mtmfs records what it is
    given and finds nothing."""

    def vis_adjoint(self, vis, nx, nz, su, sv, u, v, w=None):
        self.calls.append(dict(kind="adjoint", nx=nx, nz=nz, vis=vis.clone()))
        img = torch.from_numpy(self.beam(nx, nz).reshape(-1))
        return (vis.real.sum(dim=1)[:, None] * img[None, :]).contiguous()

    def mtmfs(self, res, n_t, nx, nz, spsf, px, pz, hinv, n_iter, gain, thresh, mask=None, model=None):
        M = res.shape[0]
        self.calls.append(dict(kind="mtmfs", res=res.clone(), n_t=n_t, nx=nx, nz=nz, spsf=spsf.clone(), px=px,
                               pz=pz, hinv=np.array(hinv), n_iter=n_iter, gain=gain, thresh=thresh, mask=mask))
        assert res.is_contiguous() and spsf.is_contiguous() and model.shape == res.shape and not model.any()
        assert tuple(res.shape) == (M, n_t, nx * nz) and tuple(spsf.shape) == (M, 2 * n_t - 1, px * pz)
        return (torch.zeros(M, n_iter, dtype=torch.int32), torch.zeros(M, n_iter, n_t, dtype=torch.float64),
                torch.zeros(M, dtype=torch.int32), torch.full((M,), 0.125, dtype=torch.float64))


def _model(nx, nz):
    m = MS._model(nx, nz)
    m._engine = _Recording()
    return m


FREQS = np.array([4e9, 4.5e9, 5.25e9, 6e9])
KW = dict(shape=(15, 13), beam=(0.1, 0.1, 0.), niter=2)


def test_one_term_is_the_path_as_it_was():
    m = _model(6, 4)
    res = m.clean_image_ff(MS.U_M, MS.V_M, FREQS, mfs=True, nterms=1, **KW)
    assert MS.kinds(m) == ["adjoint", "adjoint", "clean", "restore"] and res.taylor is None
    m2 = _model(6, 4)
    res2 = m2.clean_image_ff(MS.U_M, MS.V_M, FREQS, mfs=True, **KW)
    assert MS.kinds(m2) == MS.kinds(m) and res2.image.tobytes() == res.image.tobytes()
    m3 = _model(6, 4)                                    # without a given beam: the patch goes to fit_beam as before
    m3.clean_image_ff(MS.U_M, MS.V_M, FREQS, shape=(15, 13), niter=2)
    assert MS.kinds(m3) == ["adjoint", "adjoint", "clean", "restore"]


def test_two_terms_on_the_recording_engine():
    ni, nj, pi_, pj = 15, 13, 11, 9
    m = _model(6, 4)
    res = m.clean_image_ff(MS.U_M, MS.V_M, FREQS, mfs=True, nterms=2, shape=(ni, nj), psf_shape=(pi_, pj),
                           beam=(0.1, 0.1, 0.), niter=3, gain=0.2, threshold_jy=0.25, mask=(0, 12, 2, 12))
    # R_0 and B_0 as ever, then B_1, B_2 (on the beam grid) and R_1 (on the image's), then K19 and a restore per term
    assert MS.kinds(m) == ["adjoint"] * 5 + ["mtmfs", "restore", "restore"]
    adj = [(c["nx"], c["nz"]) for c in m.engine.calls[:5]]
    assert adj == [(ni, nj), (pi_, pj), (pi_, pj), (pi_, pj), (ni, nj)]
    c = m.engine.calls[5]
    assert (c["n_t"], c["nx"], c["nz"], c["px"], c["pz"]) == (2, ni, nj, pi_, pj)
    assert (c["n_iter"], c["gain"], c["thresh"]) == (3, 0.2, 0.25)
    nu0 = 5e9                                                    # the mid-point of the lowest and highest channel
    tw = imaging.taylor_weights(FREQS, nu0, 3)
    # unit visibilities of 4 baselines and 4 channels over the sum of the weights: the beam times the moments
    mom = [float(np.repeat(tw[q], 4).sum()) / 16 for q in range(3)]
    beam = _Recording.beam(pi_, pj).reshape(-1)
    for q in range(3):
        assert np.allclose(c["spsf"][0, q].numpy(), mom[q] * beam, rtol=1e-14, atol=1e-18), q
    # the visibilities handed to K11 for term q are V times w_f^q, channel by channel
    V1 = m.engine.calls[2]["vis"].reshape(4, 4)
    assert np.array_equal(V1.real.numpy(), np.repeat(tw[1][:, None], 4, axis=1))
    assert m.engine.calls[1]["vis"].real.numpy().tolist() == [[1.0] * 16]
    H, Hinv = imaging.taylor_hessian_inverse(c["spsf"][0, :, (pi_ // 2) * pj + pj // 2].numpy())
    assert c["hinv"].shape == (1, 2, 2) and np.array_equal(c["hinv"][0], Hinv)
    want = np.zeros((ni, nj), dtype=bool)
    want[0:13, 2:13] = True
    assert np.array_equal(np.asarray(c["mask"]).reshape(ni, nj), want)
    # the result: tt0 is the image, R_0 the residual, the rows (ix, iz, c_0, c_1), the peak K19's
    assert res.image.shape == res.residual.shape == res.model.shape == (1, ni, nj)
    assert res.components[0].shape == (0, 4) and res.peak_residual[0] == 0.125
    t = res.taylor
    assert isinstance(t, list) and len(t) == 1 and set(t[0]) == {
        "tt", "residual_tt", "model_tt", "alpha", "beta", "alpha_cut_jy", "reffreq_hz", "hessian", "hinv"}
    t = t[0]
    assert t["tt"].shape == t["residual_tt"].shape == t["model_tt"].shape == (2, ni, nj)
    assert t["beta"] is None and t["reffreq_hz"] == nu0 and np.array_equal(t["hessian"], H)
    assert np.array_equal(t["hinv"], Hinv) and np.array_equal(res.residual[0], t["residual_tt"][0])
    assert np.array_equal(res.image[0], t["tt"][0])
    # no component: tt_t is term t of the principal solution of the planes, sum_q Hinv[t][q] R_q
    R = c["res"][0].numpy().reshape(2, ni, nj)
    for k in range(2):
        assert np.allclose(t["tt"][k], Hinv[k, 0] * R[0] + Hinv[k, 1] * R[1], rtol=1e-13, atol=1e-16)
    # alpha: tt1 / tt0 above the cut (0.1 of the largest tt0), NaN exactly below
    cut = 0.1 * t["tt"][0].max()
    assert t["alpha_cut_jy"] == cut
    hi = t["tt"][0] > cut
    assert hi.any() and (~hi).any() and np.array_equal(np.isnan(t["alpha"]), ~hi)
    assert np.array_equal(t["alpha"][hi], (t["tt"][1] / t["tt"][0])[hi])
    # reffreq_hz and alpha_cut_jy given; three terms: beta
    m3 = _model(6, 4)
    r3 = m3.clean_image_ff(MS.U_M, MS.V_M, FREQS, mfs=True, nterms=3, reffreq_hz=4.8e9, alpha_cut_jy=-1.0, **KW)
    assert MS.kinds(m3) == ["adjoint"] * 8 + ["mtmfs"] + ["restore"] * 3
    t3 = r3.taylor[0]
    assert t3["reffreq_hz"] == 4.8e9 and t3["alpha_cut_jy"] == -1.0 and t3["tt"].shape == (3, 15, 13)
    ok = t3["tt"][0] > -1.0
    a = t3["tt"][1] / t3["tt"][0]
    assert np.array_equal(t3["alpha"][ok], a[ok])
    assert np.array_equal(t3["beta"][ok], (t3["tt"][2] / t3["tt"][0] - a * (a - 1.) / 2.)[ok])
    # Imager._clean_images takes the keywords by name
    m4 = _model(6, 4)
    r4 = m4._imager._clean_images(torch.ones(4, 4, dtype=torch.complex128), torch.from_numpy(MS.U_M),
                                  torch.from_numpy(MS.V_M), FREQS, None, (15, 13), None, True, 2, 0.1, 0.0, None,
                                  (0.1, 0.1, 0.), None, nterms=2)
    assert r4.taylor is not None and r4.major is None and r4.imfit is None


def test_the_refusals():
    m = _model(6, 4)
    bads = [dict(nterms=2),                                      # without mfs
            dict(nterms=2, mfs=True, scales=[0, 3]),
            dict(nterms=2, mfs=True, major_cycles=1),
            dict(nterms=5, mfs=True), dict(nterms=0, mfs=True), dict(nterms=1.5, mfs=True),
            dict(nterms="two", mfs=True),
            dict(nterms=2, mfs=True, reffreq_hz=-1.0), dict(nterms=2, mfs=True, alpha_cut_jy=np.nan)]
    for bad in bads:
        with pytest.raises(ValueError):
            m.clean_image_ff(MS.U_M, MS.V_M, FREQS, **dict(KW, **bad))
    assert "mtmfs" not in MS.kinds(m)
    # fewer distinct frequencies than terms
    with pytest.raises(ValueError, match="distinct frequencies"):
        m.clean_image_ff(MS.U_M, MS.V_M, np.array([5e9, 5e9, 6e9]), mfs=True, nterms=3, **KW)
    # a band too narrow for the terms: the Hessian's refusal reaches the caller
    with pytest.raises(ValueError, match="too narrow"):
        m.clean_image_ff(MS.U_M, MS.V_M, 5e9 * (1 + np.array([-1e-7, 0, 1e-7])), mfs=True, nterms=2, **KW)
    # nterms = 1 takes none of the checks: scales and major cycles go on as before
    m.clean_image_ff(MS.U_M, MS.V_M, FREQS[:1], scales=[0, 3], nterms=1, **KW)


def test_public_surface():
    from rajepy_amd import classes, engine as E
    J = classes.JetModel
    new = ["nterms", "reffreq_hz", "alpha_cut_jy"]
    tail = ["major_cycles", "cyclefactor", "cycleniter", "min_psf_fraction", "max_psf_fraction"]
    for fn in (J.clean_image_ff, J.clean_image_rrl, J.observe_ff, J.observe_rrl, imaging.Imager._clean_images,
               imaging.Imager._observe):
        p = inspect.signature(fn).parameters
        names = list(p)
        i = names.index("scale_bias")
        assert names[i + 1:] == new + tail, fn.__qualname__
        assert p["nterms"].default == 1 and p["reffreq_hz"].default is None and p["alpha_cut_jy"].default is None
    p = inspect.signature(E.RTEngine.mtmfs).parameters
    assert list(p) == ["self", "res", "n_t", "nx", "nz", "spsf", "px", "pz", "hinv", "n_iter", "gain", "thresh",
                       "mask", "model"]
    assert p["mask"].default is None and p["model"].default is None
    assert "nterms" not in inspect.signature(classes.Pipeline.execute).parameters
    # CleanResult.taylor: an attribute beside the six fields, like imfit and major
    R = imaging.CleanResult
    six = dict(image=1, residual=2, model=3, components=4, beam=5, peak_residual=6)
    r = R(**six)
    assert r.taylor is None and R.taylor is None and len(r) == 6 and R._fields == tuple(six)
    r = R(1, 2, 3, 4, 5, 6, taylor=[{"tt": 0}], imfit=["f"])
    assert r.taylor == [{"tt": 0}] and r.imfit == ["f"] and r.major is None and tuple(r) == (1, 2, 3, 4, 5, 6)
    r2 = r._replace(image=9)
    assert r2.taylor == [{"tt": 0}] and r2.imfit == ["f"] and r2.image == 9
    r3 = r._replace(taylor=None, major=["m"])
    assert r3.taylor is None and r3.major == ["m"] and r3.imfit == ["f"]
    assert R._make(range(6)).taylor is None
    a, b, c, d, e, f = r                                          # code that unpacks the six keeps working
