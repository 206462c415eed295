"""Pins tests/msclean_ref.py -- the long-double convolution and the follow-the-device multi-scale
CLEAN that tests/test_gpu_msclean.py holds rjp_convolve2d and rjp_msclean (K17) to -- before anything
runs on a GPU: the reference against hand-worked cases and against clean_ref for one scale; the scale
kernels; a float64 emulation of both kernels (inside the bounds) and five planted mistakes (outside);
then the ABI, the workspace query and the tile rules as host arithmetic, check_convolve2d /
check_msclean from a plain C++ program, and the Python paths on a recording engine."""
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
from tests import msclean_ref as K

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against hand-worked cases --------------------------------------------------------
def test_convolution_by_hand():
    out, scale = K.conv(np.array([[3.0]]), np.array([[-2.0]]), add=np.array([[0.5]]))   # 1 x 1
    assert float(out[0, 0]) == -5.5 and float(scale[0, 0]) == 6.5
    # a 3 x 3 asymmetric kernel on a delta at (1, 2) of 4 x 5: a CONVOLUTION puts ker[a, b] at
    # (1 + a - 1, 2 + b - 1), so the kernel appears unflipped around the source, clipped at the edge
    ker = np.arange(1.0, 10.0).reshape(3, 3)
    src = np.zeros((4, 5))
    src[1, 2] = 2.0
    out, _ = K.conv(src, ker)
    want = np.zeros((4, 5))
    want[0:3, 1:4] = 2.0 * ker
    assert np.array_equal(out.astype(float), want)
    src = np.zeros((4, 5))
    src[0, 4] = 1.0                                        # a corner: only ker[1:, :2] lies inside
    want = np.zeros((4, 5))
    want[0:2, 3:5] = ker[1:, :2]
    assert np.array_equal(K.conv(src, ker)[0].astype(float), want)
    # the correlation is the other thing on an asymmetric kernel
    assert not np.array_equal(K.conv(src, ker, flip=False)[0].astype(float), want)
    # a kernel larger than the image; zero outside; NaN by IEEE: 0 NaN = NaN wherever the kernel reaches
    img = np.arange(15.0).reshape(5, 3)
    assert float(K.conv(img, np.ones((9, 9)))[0][2, 1]) == img.sum()
    img[4, 0] = np.nan
    k3 = np.zeros((3, 3))
    k3[1, 1] = 1.0
    o = K.conv(img, k3)[0].astype(float)
    assert np.isnan(o[3:, :2]).all() and np.isfinite(o[:3]).all() and np.isfinite(o[:, 2]).all()


def test_two_scales_on_5_by_3_by_hand():
    # planes: R_0 = delta plane, R_1; X_00 = delta beam (centre 1), X_01 = 0.5 at the centre,
    # X_11 = 2 at the centre; weights (1, 0.5); gain 0.5.  All numbers exact in binary.
    n_s, nx, nz = 2, 5, 3
    X = np.zeros((3, 3, 3))
    X[K.tri(0, 0, 2), 1, 1], X[K.tri(0, 1, 2), 1, 1], X[K.tri(1, 1, 2), 1, 1] = 1.0, 0.5, 2.0
    X[K.tri(0, 1, 2), 1, 2] = 0.25                         # one off-centre value of the cross beam
    R0 = np.zeros((2, nx, nz))
    R0[0, 2, 1], R0[1, 2, 1], R0[1, 4, 0] = 1.0, 4.0, -1.0
    # scores: plane 0: 1; plane 1: 0.5 * 4 = 2 -> (k, p) = (1, 7), f = 0.5 * 4 / 2 = 1
    cpix, cscale, cflux, R = K.msclean(R0, X, [1.0, 0.5], None, 0.0, 0.5, 1)
    assert list(cpix) == [7] and list(cscale) == [1] and float(cflux[0]) == 1.0
    want = R0.copy()
    want[1, 2, 1] -= 2.0                                   # X_11
    want[0, 2, 1] -= 0.5                                   # X[1][0] is the plane of X[0][1], not transposed
    want[0, 2, 2] -= 0.25
    assert np.array_equal(R.astype(float), want)
    # next: plane 0: max(0.5, 0.25) = 0.5; plane 1: 0.5 * 2 = 1 -> (1, 7) again, f = 0.5
    cpix, cscale, cflux, R = K.msclean(R0, X, [1.0, 0.5], None, 0.0, 0.5, 2)
    assert list(cpix) == [7, 7] and list(cscale) == [1, 1] and float(cflux[1]) == 0.5
    # a tie of the scores goes to the lower scale: weights (1, 0.25) make both 1
    cpix, cscale, cflux, _ = K.msclean(R0, X, [1.0, 0.25], None, 0.0, 0.5, 1)
    assert (list(cpix), list(cscale), float(cflux[0])) == ([7], [0], 0.5)
    # weight 0: the plane is updated, never picked; the threshold is on the score
    cpix, cscale, _, R = K.msclean(R0, X, [0.0, 0.5], None, 0.0, 0.5, 1)
    assert list(cscale) == [1] and float(R[0, 2, 1]) == 0.5
    assert len(K.msclean(R0, X, [1.0, 0.5], None, 2.0, 0.5, 5)[0]) == 0      # 2 is not > 2
    assert len(K.msclean(R0, X, [1.0, 0.5], None, 1.9, 0.5, 5)[0]) == 1
    # a zero X_kk(centre) of a plane with weight > 0: finished from the start
    X0 = X.copy()
    X0[K.tri(1, 1, 2), 1, 1] = 0.0
    assert len(K.msclean(R0, X0, [1.0, 0.5], None, 0.0, 0.5, 5)[0]) == 0
    assert len(K.msclean(R0, X0, [1.0, 0.0], None, 0.0, 0.5, 5)[0]) == 5
    assert K.tri(0, 0, 3) == 0 and K.tri(0, 2, 3) == 2 and K.tri(1, 1, 3) == 3 and K.tri(2, 1, 3) == 4 \
        and K.tri(2, 2, 3) == 5


def test_one_scale_reproduces_clean_ref():
    rng = np.random.default_rng(5)
    nx, nz = 17, 23
    B = C.random_beam(rng, 2 * nx - 1, 2 * nz - 1)
    D = C.random_image(rng, nx, nz, B)
    mask = np.zeros((nx, nz), dtype=bool)
    mask[2:15, 3:20] = True
    for m in (None, mask):
        p1, f1, R1 = C.hogbom(D, B, m, 0.01, 0.1, 40)
        p2, k2, f2, R2 = K.msclean(D[None], B[None], [1.0], m, 0.01, 0.1, 40)
        assert np.array_equal(p1, p2) and not k2.any()
        assert np.array_equal(f1, f2) and np.array_equal(R1, R2[0])       # (a division by 1.0 is exact)


def test_scale_kernel_and_biases():
    assert np.array_equal(imaging.scale_kernel(0), [[1.0]]) and np.array_equal(imaging.scale_kernel(-3), [[1.0]])
    for s in (0.5, 1.0, 2.5, 4, 10):
        k = imaging.scale_kernel(s)
        h = int(np.ceil(s)) - 1
        assert k.shape == (2 * h + 1, 2 * h + 1) and abs(k.sum() - 1.0) < 1e-15 and k.dtype == np.float64
        assert np.array_equal(k, k.T) and np.array_equal(k, k[::-1]) and np.array_equal(k, k[:, ::-1])
        d = np.arange(-h, h + 1)
        r2 = d[:, None] ** 2 + d[None, :] ** 2
        assert np.all(k[r2 >= s * s] == 0) and np.all(k[r2 < s * s] > 0) and k[h, h] == k.max()
        para = np.where(r2 < s * s, 1 - r2 / s ** 2, 0.0)
        assert np.allclose(k, para / para.sum(), rtol=1e-15, atol=0)
    assert np.array_equal(imaging.scale_kernel(4)[3], imaging.scale_kernel(4)[:, 3])
    assert np.allclose(imaging.scale_biases([0, 4, 10]), [1.0, 0.76, 0.4], rtol=1e-15)
    assert np.array_equal(imaging.scale_biases([7]), [1.0]) and np.array_equal(imaging.scale_biases([0]), [1.0])
    with pytest.raises(ValueError):
        imaging.scale_kernel(np.inf)
    from rajepy_amd import engine as E
    assert E.scale_kernel is imaging.scale_kernel and E.scale_biases is imaging.scale_biases


# ---- the checks themselves: a float64 emulation inside, planted mistakes outside -------------------------
def test_float64_convolution_inside_the_bound_and_a_correlation_outside():
    rng = np.random.default_rng(11)
    for (nx, nz), (kx, kz) in (((5, 3), (9, 9)), ((33, 47), (3, 5)), ((20, 31), (15, 15))):
        img = rng.standard_normal((nx, nz))
        ker = rng.standard_normal((kx, kz))
        add = rng.standard_normal((nx, nz))
        got = K.conv(img, ker, add, dtype=np.float64)[0]
        worst = K.check_conv(got, img, ker, add, roundings=2)
        assert worst < 1.0
        with pytest.raises(AssertionError, match="convolution"):           # planted: a correlation
            K.check_conv(K.conv(img, ker, add, dtype=np.float64, flip=False)[0], img, ker, add, roundings=2)
        with pytest.raises(AssertionError, match="convolution"):           # planted: `add` forgotten
            K.check_conv(K.conv(img, ker, None, dtype=np.float64)[0], img, ker, add, roundings=2)
    img[3, 4] = np.nan
    img[10, 2] = np.inf
    got = K.conv(img, ker, add, dtype=np.float64)[0]
    assert K.check_conv(got, img, ker, add, roundings=2) < 1.0
    bad = got.copy()
    bad[np.isnan(bad)] = 0.0
    with pytest.raises(AssertionError, match="NaN pattern"):
        K.check_conv(bad, img, ker, add, roundings=2)


def run_follow(R0, X, weight, mask, thresh, gain, n_iter, **switches):
    cpix, cscale, cflux, R = K.msclean(R0, X, weight, mask, thresh, gain, n_iter, dtype=np.float64, **switches)
    n = len(cpix)
    fp, fk, ff = np.full(n_iter, -7, dtype=np.int64), np.full(n_iter, -7, dtype=np.int64), np.full(n_iter, np.nan)
    fp[:n], fk[:n], ff[:n] = cpix, cscale, cflux
    model = np.zeros(R0.shape).reshape(R0.shape[0], -1)
    for p, k, f in zip(cpix, cscale, cflux):
        model[k, p] += f
    ok = K._cands(R, weight, mask)
    peak = float((np.asarray(weight)[:, None, None] * np.abs(R))[ok].max()) if ok.any() else 0.0
    worst = K.follow(R0, X, weight, mask, thresh, gain, n_iter, fp, fk, ff, n, R, peak=peak, model=model,
                     poison_pix=-7, poison_flux=np.nan, roundings=2)
    return worst, (fp, fk, ff, n, R)


@pytest.mark.parametrize("nx,nz,scales,gain", [(33, 47, (0, 2.5), 0.1), (33, 47, (0, 2.5, 4), 0.3),
                                               (40, 25, (0, 3), 1.0)])
def test_float64_emulation_passes_inside_the_bound(nx, nz, scales, gain):
    rng = np.random.default_rng(100 * nx + nz)
    R0, X, w = K.scale_problem(rng, nx, nz, scales)
    n_iter = 60
    worst, (fp, fk, ff, n, R) = run_follow(R0, X, w, None, 0.0, gain, n_iter)
    assert n == n_iter and worst < 1.0 and len(set(fk[:n])) > 1           # more than one scale is picked
    assert K.conservation(R0, X, fp, fk, ff, n, R, roundings=2) <= 1.0
    rp, rk, _, RL = K.msclean(R0, X, w, None, 0.0, gain, n_iter)
    assert np.array_equal(rp, fp[:n]) and np.array_equal(rk, fk[:n]) and float(np.abs(RL - R).max()) < 1e-13
    mask = np.zeros((nx, nz), dtype=bool)
    mask[nx // 4:nx - 4, 4:nz // 2 + 4] = True
    w0 = w.copy()
    w0[1] = 0.0                                                             # a plane that is never picked
    top = float((w0[:, None, None] * np.abs(R0))[:, mask].max())
    w2, (_, fk2, _, n2, _) = run_follow(R0, X, w0, mask, 0.4 * top, gain, n_iter)
    assert w2 < 1.0 and 0 < n2 < n_iter and not (fk2[:n2] == 1).any()
    R3, X3, w3 = K.scale_problem(rng, nx, nz, scales, psf=(21, 17))
    assert run_follow(R3, X3, w3, None, 0.0, gain, 40)[0] < 1.0
    print("%d x %d %r gain %g: worst error / bound %.3f, %.3f (mask, threshold, a zero weight)"
          % (nx, nz, scales, gain, worst, w2))


def test_planted_mistakes_fall_outside():
    rng = np.random.default_rng(77)
    nx, nz = 33, 47
    R0, X, w = K.scale_problem(rng, nx, nz, (0, 2.5, 4))
    # the cross beams of a random (u, v) coverage are point symmetric, so a transposed plane is the
    # same plane: break the symmetry of the off-diagonal planes, as a beam with w-terms would
    Xa = X.copy()
    for t in (K.tri(0, 1, 3), K.tri(0, 2, 3), K.tri(1, 2, 3)):
        Xa[t] *= (1.0 + 0.5 * np.linspace(-1, 1, X.shape[2]))[None, :]
    assert run_follow(R0, Xa, w, None, 0.0, 0.2, 30)[0] < 1.0
    with pytest.raises(AssertionError):          # X[l][k] taken from a transposed plane
        run_follow(R0, Xa, w, None, 0.0, 0.2, 30, transpose_lower=True)
    with pytest.raises(AssertionError, match="flux"):          # f without the division
        run_follow(R0, X, 2 * w, None, 0.0, 0.2, 30, divide=False)
    with pytest.raises(AssertionError):          # only the picked plane updated
        run_follow(R0, X, w, None, 0.0, 0.2, 30, update_all=False)
    # the tie broken towards the higher scale: two planes with the same untouched value, weights 1
    T = np.zeros((2, 4, 5))
    T[0, 2, 1] = T[1, 0, 3] = 1.0
    Xd = np.zeros((3, 7, 9))
    Xd[:, 3, 4] = 1.0
    assert run_follow(T, Xd, [1.0, 1.0], None, 0.0, 0.5, 1)[1][1][0] == 0
    with pytest.raises(AssertionError, match="lower scale"):
        run_follow(T, Xd, [1.0, 1.0], None, 0.0, 0.5, 1, tie_low_scale=False)


# ---- the ABI, the workspace query, the tile rules ---------------------------------------------------------
def test_abi_signatures_and_header():
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    P, i32, dbl, DP = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.POINTER(ctypes.c_double)

    def names(fn):
        decl = re.search(r"int64_t %s\((.*?)\);" % fn, hdr, re.S).group(1)
        return [re.search(r"(\w+)$", p.strip()).group(1) for p in decl.split(",")]

    assert names("rjp_convolve2d") == ["ctx", "d_in", "n_maps", "nx", "nz", "d_ker", "n_ker", "kx", "kz",
                                       "d_add", "d_out", "stream"]
    assert names("rjp_msclean") == ["ctx", "d_res", "n_maps", "n_s", "nx", "nz", "d_xpsf", "n_psf", "px", "pz",
                                    "h_weight", "d_mask", "h_thresh", "gain", "n_iter", "d_cpix", "d_cscale",
                                    "d_cflux", "d_ncomp", "d_model", "d_peak", "d_work", "work_bytes", "stream"]
    assert "size_t rjp_msclean_workspace(int32_t n_maps, int32_t n_s, int32_t nx, int32_t nz);" in hdr
    assert "#define RJP_CONV_MAX_K 255" in hdr and "#define RJP_CONV_TILE_X 16" in hdr \
        and "#define RJP_CONV_TILE_Z 64" in hdr and "casa/tasks.py:243-244" in hdr
    assert _lib.SIGNATURES["rjp_convolve2d"] == (ctypes.c_int64, [P, P, i32, i32, i32, P, i32, i32, i32, P, P, P])
    assert _lib.SIGNATURES["rjp_msclean_workspace"] == (ctypes.c_size_t, [i32] * 4)
    res, args = _lib.SIGNATURES["rjp_msclean"]
    assert res is ctypes.c_int64
    assert args == [P, P, i32, i32, i32, i32, P, i32, i32, i32, DP, P, DP, dbl, i32, P, P, P, P, P, P, P,
                    ctypes.c_size_t, P]
    lib = _lib.load()
    for name in ("rjp_convolve2d", "rjp_msclean_workspace", "rjp_msclean"):
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    mk = open(os.path.join(ROOT, "rajepy_amd", "csrc", "Makefile")).read()
    assert "$(OBJDIR)/convolve.o" in mk and "$(OBJDIR)/msclean.o" in mk and "clean_common.h" in mk
    # a NULL context is refused before anything else
    assert lib.rjp_convolve2d(None, None, 1, 1, 1, None, 1, 1, 1, None, None, None) == _lib.RJP_ERR_ARG
    assert lib.rjp_msclean(None, None, 1, 1, 1, 1, None, 1, 1, 1, None, None, None, 0.1, 1, None, None, None,
                           None, None, None, None, 0, None) == _lib.RJP_ERR_ARG


def test_tile_rules_and_workspace_query():
    assert K.conv_workgroups(1, 1, 1) == 1 and K.conv_workgroups(1, 16, 64) == 1
    assert K.conv_workgroups(1, 17, 64) == 2 and K.conv_workgroups(1, 16, 65) == 2
    assert K.conv_workgroups(3, 67, 131) == 3 * 5 * 3 and K.conv_workgroups(2, 130, 65) == 2 * 9 * 2
    # the LDS budget: tile plus halo plus the chunk's kernel rows, at every odd kernel width
    for kz in range(1, K.CONV_MAX_K + 1, 2):
        ka = K.conv_chunk_rows(K.CONV_MAX_K, kz)
        w = 64 + kz - 1
        assert ka >= 1 and (16 + ka - 1) * w + ka * kz <= K.CONV_LDS
        assert ka == K.CONV_MAX_K or (16 + ka) * w + (ka + 1) * kz > K.CONV_LDS
    assert K.conv_chunk_rows(129, 129) == 16 and K.conv_chunk_rows(3, 5) == 3 and K.conv_chunk_rows(255, 255) == 5
    assert K.CONV_LDS * 8 * 2 <= 160 * 1024                                 # two workgroups per CU
    ws = _lib.load().rjp_msclean_workspace
    for a in ((1, 1, 1, 1), (1, 2, 5, 3), (3, 3, 67, 131), (1, 3, 501, 501), (2, 2, 600, 600), (7, 4, 130, 65)):
        assert ws(*a) == K.ms_workspace_bytes(*a) > 0 and ws(*a) % 16 == 0, a
    assert ws(1, 1, 67, 131) == C.workspace_bytes(1, 67, 131)             # one scale: K12's
    assert K.ms_workgroups(1, 2, 600, 600) == 704 > 2 * K.REDUCE_PASS       # three passes of the reduction
    for i in range(4):
        for bad in (0, -1):
            a = [3, 2, 67, 131]
            a[i] = bad
            assert ws(*a) == 0
    big = 2 ** 31 - 1
    assert ws(big, big, big, big) == 0                                      # the size overflows
    assert ws(big, 1, big, big) % 16 == 0


def test_checks_from_plain_cpp(tmp_path):
    """check_convolve2d and check_msclean compiled into a stand-alone program by plain g++
    (tests/rjp_args_msclean_cases.cpp): every refusal, status and message, in the order the checks
    make them -- the messages tests/test_gpu_msclean.py sees from the library."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "rjp_args_msclean_cases"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rajepy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rjp_args_msclean_cases.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        case, status, msg = line.split("\t")
        got[case] = (int(status), msg)
    want = {"conv_null": ["conv NULL d_in", "conv NULL d_ker", "conv NULL d_out", "conv NULL beats sizes"],
            "conv_sizes": ["conv n_maps 0", "conv nx 0", "conv nz -1", "conv kx 0", "conv kz -3",
                           "conv sizes beat even"],
            "conv_even": ["conv kx even", "conv kz even", "conv even beats max"],
            "conv_max": ["conv kx 257", "conv kz 257", "conv max beats n_ker"],
            "conv_nker": ["conv n_ker 0", "conv n_ker 3", "conv n_ker beats the image size"],
            "conv_npix": ["conv nx nz 2^31"],
            "conv_wgs": ["conv workgroups"],
            "null": ["NULL d_res", "NULL d_xpsf", "NULL h_weight", "NULL h_thresh", "NULL d_cpix",
                     "NULL d_cscale", "NULL d_cflux", "NULL d_ncomp", "NULL beats sizes"],
            "sizes": ["n_maps 0", "n_s 0", "nx 0", "nz -1", "px 0", "pz 0", "sizes beat even"],
            "even": ["px even", "pz even", "even beats n_psf"],
            "npsf": ["n_psf 0", "n_psf 3", "n_psf beats gain"],
            "npix": ["nx nz 2^31"],
            "gain": ["gain 0", "gain 1.5", "gain nan", "gain beats n_iter"],
            "niter": ["n_iter 0", "n_iter beats thresh"],
            "thresh": ["thresh negative", "thresh inf", "thresh beats weight"],
            "weight": ["weight negative", "weight inf", "weight nan"]}
    seen = set()
    for key, cases in want.items():
        for case in cases:
            assert got[case] == (_lib.RJP_ERR_ARG, K.MSG[key]), case
            seen.add(case)
    valid = {c for c in got if "valid" in c}
    assert len(valid) == 6 and all(got[c] == (0, "") for c in valid)
    assert seen | valid == set(got)


# ---- the Python paths on a recording engine ----------------------------------------------------------
class _RecordingEngine:
    """vis_adjoint returns a smooth positive beam-like image of the grid it is asked for;
    convolve2d is a real float64 convolution; msclean records what it is given and finds nothing."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def _device_f64(self, values):
        if isinstance(values, torch.Tensor):
            return values
        return torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64).reshape(-1))

    def vis(self, maps, nx, nz, su, sv, u, v):
        M, K_ = len(su), u.numel()
        return torch.complex(torch.ones(M, K_, dtype=torch.float64), torch.zeros(M, K_, dtype=torch.float64))

    @staticmethod
    def beam(nx, nz):
        x = np.arange(nx)[:, None] - (nx - 1) / 2
        z = np.arange(nz)[None, :] - (nz - 1) / 2
        return np.exp(-(x * x + z * z) / 18.0) * (1 + 0.01 * x)

    def vis_adjoint(self, vis, nx, nz, su, sv, u, v, w=None):
        M, K_ = vis.shape
        self.calls.append(dict(kind="adjoint", nx=nx, nz=nz))
        img = torch.from_numpy(self.beam(nx, nz).reshape(-1))
        return (K_ * (1.0 + torch.arange(M, dtype=torch.float64))[:, None] * img[None, :]).contiguous()

    def clean(self, res, nx, nz, psf, px, pz, n_iter, gain, thresh, mask=None, model=None):
        M = res.shape[0]
        self.calls.append(dict(kind="clean", px=px, pz=pz))
        return (torch.zeros(M, n_iter, dtype=torch.int32), torch.zeros(M, n_iter, dtype=torch.float64),
                torch.zeros(M, dtype=torch.int32), torch.zeros(M, dtype=torch.float64))

    def convolve2d(self, inp, nx, nz, ker, kx, kz, add=None):
        assert inp.is_contiguous() and ker.is_contiguous() and ker.numel() == kx * kz
        self.calls.append(dict(kind="conv", nx=nx, nz=nz, kx=kx, kz=kz, add=add is not None))
        x = inp.numpy().reshape(-1, nx, nz)
        a = add.numpy().reshape(-1, nx, nz) if add is not None else [None] * len(x)
        k = ker.numpy().reshape(kx, kz)
        return torch.from_numpy(np.stack([K.conv(x[m], k, a[m], dtype=np.float64)[0] for m in range(len(x))])
                                .reshape(len(x), nx * nz))

    def msclean(self, res, n_s, nx, nz, xpsf, px, pz, weight, n_iter, gain, thresh, mask=None, model=None):
        M = res.shape[0]
        self.calls.append(dict(kind="msclean", res=res.clone(), n_s=n_s, nx=nx, nz=nz, xpsf=xpsf.clone(), px=px,
                               pz=pz, weight=np.array(weight), n_iter=n_iter, gain=gain, thresh=thresh,
                               mask=mask.clone(), model=model))
        assert res.is_contiguous() and xpsf.is_contiguous() and model.shape == res.shape and not model.any()
        return (torch.zeros(M, n_iter, dtype=torch.int32), torch.zeros(M, n_iter, dtype=torch.int32),
                torch.zeros(M, n_iter, dtype=torch.float64), torch.zeros(M, dtype=torch.int32),
                torch.zeros(M, dtype=torch.float64))

    def restore(self, cpix, cflux, ncomp, abc, nx, nz, add=None):
        self.calls.append(dict(kind="restore", add=add is not None))
        return add.clone() if add is not None else torch.zeros(cpix.shape[0], nx * nz, dtype=torch.float64)


def _model(nx, nz):
    from rajepy_amd import classes

    class Model(classes.JetModel):
        """A JetModel that holds only what its imaging front reads (see test_uvweight_reference_cpu)."""

        def __init__(self):
            self._engine, self._nx, self._nz, self._csize = _RecordingEngine(), nx, nz, 0.5
            self._params = {"target": {"dist": 120.}}

    m = Model()
    m._ff_products = lambda freqs, flux=False, device=False, formal=False: torch.zeros(len(freqs), nx * nz)
    return m


U_M, V_M = np.array([0., 100., -3e3, 2e4]), np.array([0., -50., 1e3, 1e4])
FREQS = np.array([5e9, 2e10])


def kinds(m):
    return [c["kind"] for c in m.engine.calls]


def test_without_scales_nothing_new_is_called():
    m = _model(6, 4)
    res = m.clean_image_ff(U_M, V_M, FREQS, shape=(15, 13), beam=(0.1, 0.1, 0.), niter=2)
    assert kinds(m) == ["adjoint", "adjoint", "clean", "restore"]
    assert (m.engine.calls[1]["nx"], m.engine.calls[1]["nz"]) == (29, 25)
    assert all(c.shape == (0, 3) for c in res.components)


def test_planes_weights_mask_and_the_enlarged_beam_grid():
    ni, nj, pi_, pj = 15, 13, 11, 9
    m = _model(6, 4)
    res = m.clean_image_ff(U_M, V_M, FREQS, shape=(ni, nj), beam=(0.1, 0.1, 0.), niter=3, psf_shape=(pi_, pj),
                           scales=[4, 2.5, 4], mask=(0, 12, 2, 12), threshold_jy=0.25)
    call = [c for c in m.engine.calls if c["kind"] == "msclean"]
    assert len(call) == 1 and "clean" not in kinds(m)
    c = call[0]
    # plane 0 is ALWAYS the delta scale, here with weight 0 (0 is not among the scales); 2.5 and 4 follow
    hmax = 3
    assert c["n_s"] == 3 and (c["nx"], c["nz"], c["px"], c["pz"]) == (ni, nj, pi_, pj)
    assert (c["n_iter"], c["gain"], c["thresh"]) == (3, 0.1, 0.25)
    # the beam was made on a grid 4 h_max larger in each direction, the image on its own
    adj = [x for x in m.engine.calls if x["kind"] == "adjoint"]
    assert [(a["nx"], a["nz"]) for a in adj] == [(ni, nj), (pi_ + 4 * hmax, pj + 4 * hmax)]
    kers = [imaging.scale_kernel(s) for s in (0, 2.5, 4)]
    big = _RecordingEngine.beam(pi_ + 4 * hmax, pj + 4 * hmax)     # map 0, over the sum of the 4 weights
    g = 2 * hmax
    for k in range(3):
        for l in range(k, 3):
            want = K.conv64(K.conv64(big, kers[k]), kers[l])[g:g + pi_, g:g + pj]
            got = c["xpsf"][0, K.tri(k, l, 3)].numpy().reshape(pi_, pj)
            assert np.allclose(got, want, rtol=1e-13, atol=1e-16), (k, l)
    # ... which is NOT the convolution of the cropped beam: that one is truncated at the window's edge
    trunc = K.conv64(big[g:g + pi_, g:g + pj], kers[2])
    assert abs(trunc[0, 0] - c["xpsf"][0, K.tri(0, 2, 3)].numpy().reshape(pi_, pj)[0, 0]) > 1e-3 * abs(trunc[0, 0])
    # the planes: R_l = m_l * D, plane 0 the dirty image itself
    D = c["res"][0, 0].numpy().reshape(ni, nj)
    assert np.array_equal(D, _RecordingEngine.beam(ni, nj))
    for l in (1, 2):
        assert np.allclose(c["res"][0, l].numpy().reshape(ni, nj), K.conv64(D, kers[l]), rtol=1e-13)
    # the weights: bias_k / X_kk(centre), 0 for the delta plane
    bias = imaging.scale_biases([0, 2.5, 4])
    centre = (pi_ // 2) * pj + pj // 2
    for mm in range(2):
        xkk = [float(c["xpsf"][mm, K.tri(k, k, 3), centre]) for k in range(3)]
        assert c["weight"].shape == (2, 3) and c["weight"][mm, 0] == 0.0
        assert np.allclose(c["weight"][mm, 1:], bias[1:] / np.array(xkk[1:]), rtol=1e-15)
    # the mask: the box, minus everything nearer than h_max to the border
    want = np.zeros((ni, nj), dtype=bool)
    want[0:13, 2:13] = True
    want[:hmax], want[ni - hmax:], want[:, :hmax], want[:, nj - hmax:] = False, False, False, False
    assert np.array_equal(c["mask"].numpy().reshape(ni, nj), want) and want.sum() == 9 * 7
    # the result: rows of four columns, the raw plane as the residual, its masked max as the peak
    assert all(x.shape == (0, 4) for x in res.components) and res.image.shape == (2, ni, nj)
    assert np.array_equal(res.residual[0], D) and res.peak_residual[0] == np.abs(D[want]).max()
    assert type(res).__name__ == "CleanResult" and res._fields == ("image", "residual", "model", "components",
                                                                   "beam", "peak_residual")
    # model and image: one restore per plane; the scales' convolutions chained through `add`
    tail = m.engine.calls[m.engine.calls.index(c) + 1:]
    assert [x["kind"] for x in tail] == ["restore", "conv", "restore", "conv", "conv", "restore", "conv"]
    assert all(x["add"] for x in tail if x["kind"] == "conv") and tail[0]["add"] and not tail[2]["add"]


def test_delta_among_the_scales_a_bias_list_and_the_refusals():
    m = _model(6, 4)
    m.clean_image_ff(U_M, V_M, FREQS[:1], shape=(15, 13), beam=(0.1, 0.1, 0.), niter=2, scales=[0, 3])
    c = [x for x in m.engine.calls if x["kind"] == "msclean"][0]
    assert c["n_s"] == 2 and c["weight"][0, 0] == 1.0 / float(c["xpsf"][0, 0, (29 // 2) * 25 + 25 // 2])
    assert c["mask"].numpy().reshape(15, 13)[2:13, 2:11].all() and c["mask"].sum() == 11 * 9
    m.clean_image_ff(U_M, V_M, FREQS[:1], shape=(15, 13), beam=(0.1, 0.1, 0.), niter=2, scales=[0, 3],
                     scale_bias=[0.5, 2.0])
    c2 = [x for x in m.engine.calls if x["kind"] == "msclean"][1]
    assert np.allclose(c2["weight"], c["weight"] * [0.5, 2.0 / 0.4], rtol=1e-15)
    m.clean_image_ff(U_M, V_M, FREQS[:1], shape=(5, 5), beam=(0.1, 0.1, 0.), niter=2, scales=[0])
    c3 = [x for x in m.engine.calls if x["kind"] == "msclean"][2]
    assert c3["n_s"] == 1 and c3["mask"].all() and "conv" not in kinds(m)[-3:]
    for bad in (dict(scales=[]), dict(scales=[np.nan]), dict(scales=[0, 3], scale_bias=[1.0]),
                dict(scales=[0, 3], scale_bias=[1.0, -1.0]), dict(scales=[3], scale_bias=[1.0, 0.0]),
                dict(scales=[0, 8]),                             # h_max = 7: nothing left of 15 x 13
                dict(scales=[0, 4], mask=(0, 2, 0, 12))):        # the box lies inside the border strip
        with pytest.raises(ValueError):
            m.clean_image_ff(U_M, V_M, FREQS[:1], shape=(15, 13), beam=(0.1, 0.1, 0.), niter=2, **bad)


def test_chunks_count_the_planes_and_the_cross_beams():
    m = _model(6, 4)
    m.VIS_STACK_BYTES = (15 * 13 * (2 * 2 + 1) + 3 * 11 * 9) * 8          # one channel's planes and cross beams
    m.clean_image_ff(U_M, V_M, FREQS, shape=(15, 13), beam=(0.1, 0.1, 0.), niter=2, psf_shape=(11, 9),
                     scales=[0, 3])
    assert kinds(m).count("msclean") == 2
    m2 = _model(6, 4)
    m2.VIS_STACK_BYTES = 2 * (15 * 13 * (2 * 2 + 1) + 3 * 11 * 9) * 8
    m2.clean_image_ff(U_M, V_M, FREQS, shape=(15, 13), beam=(0.1, 0.1, 0.), niter=2, psf_shape=(11, 9),
                      scales=[0, 3])
    assert kinds(m2).count("msclean") == 1


def test_public_surface():
    from rajepy_amd import classes, engine as E
    J = classes.JetModel
    ff = inspect.signature(J.clean_image_ff).parameters
    for name in ("clean_image_ff", "clean_image_rrl", "observe_ff", "observe_rrl"):
        p = inspect.signature(getattr(J, name)).parameters
        assert p["scales"].default is None and p["scale_bias"].default is None, name
        assert set(ff) - {"self", "u_m", "v_m"} <= set(p), name
    p = inspect.signature(E.RTEngine.convolve2d).parameters
    assert list(p) == ["self", "inp", "nx", "nz", "ker", "kx", "kz", "add"] and p["add"].default is None
    p = inspect.signature(E.RTEngine.msclean).parameters
    assert list(p) == ["self", "res", "n_s", "nx", "nz", "xpsf", "px", "pz", "weight", "n_iter", "gain", "thresh",
                       "mask", "model"]
    p = inspect.signature(imaging.Imager._clean_images).parameters
    assert p["scales"].default is None and p["scale_bias"].default is None
    assert "scales" not in inspect.signature(classes.Pipeline.execute).parameters
