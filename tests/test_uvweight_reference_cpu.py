"""tests/uvweight_ref.py -- the reference rjp_uv_weights (K15) is held to on the GPU
(tests/test_gpu_uvweight.py) -- pinned on the CPU first: hand-worked cases, the fixed point against
a long-double density, a float64 emulation of the device's arithmetic (inside the bound), planted
mistakes (outside), then check_uv_weights from a plain C++ program, the ABI, the workspace query
and the Python paths on a recording engine."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from rajepy_amd import _lib
from tests import uvweight_ref as K

LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def both(su, sv, u, v, w, nx, nz, mode, robust=0.5, **planted):
    d = K.integer_density(su, sv, u, v, w, nx, nz, **planted)
    return d, K.weights(d, w, mode, robust)


# ---- hand-worked cases ---------------------------------------------------------------------------
def test_one_visibility():
    # 5 x 3 cells (hx = 2, hz = 1): a = 0.3 -> rint(1.5) = 2, b = -0.2 -> rint(-0.6) = -1
    d, r = both([1.0], [1.0], [0.3], [-0.2], [3.0], 5, 3, K.UNIFORM)
    W = d["W"][0].reshape(5, 3)
    assert W[2 + 2, 1 - 1] == 3.0 and W[2 - 2, 1 + 1] == 3.0 and W.sum() == 6.0
    assert d["sum_w"] == [3.0] and d["counted"] == [1] and d["outside"] == [0]
    assert d["s"] == 62 - 2 - 1                              # 3 < 2^2, 2 n_vis = 2^1
    assert float(r["wout"][0][0]) == 1.0                     # uniform: w / W
    d, r = both([1.0], [1.0], [0.3], [-0.2], [3.0], 5, 3, K.BRIGGS, robust=0.0)
    f2 = 25.0 * 6.0 / 18.0                                   # (5)^2 (2 sum w) / (3^2 + 3^2)
    assert abs(float(r["f2"][0]) - f2) < 1e-15
    assert abs(float(r["wout"][0][0]) - 3.0 / (1.0 + f2 * 3.0)) < 1e-15


def test_two_visibilities_in_mirror_cells_and_the_origin_doubled():
    u, v, w = [0.25, -0.25, 0.0], [0.125, -0.125, 0.0], [1.0, 2.0, 5.0]
    d, r = both([1.0], [1.0], u, v, w, 16, 8, K.UNIFORM)
    W = d["W"][0].reshape(17, 9)
    assert W[8 + 4, 4 + 1] == 3.0 and W[8 - 4, 4 - 1] == 3.0          # both see both
    assert W[8, 4] == 10.0                                            # the origin counts twice
    assert W.sum() == 2 * 8.0 and d["sum_w"] == [8.0]
    assert [float(x) for x in r["wout"][0]] == [1.0 / 3.0, 2.0 / 3.0, 0.5]
    # (u, v) -> (-u, -v) on any of them changes nothing
    d2, r2 = both([1.0], [1.0], [-0.25, -0.25, -0.0], [-0.125, -0.125, 0.0], w, 16, 8, K.UNIFORM)
    assert d2["Q"] == d["Q"] and np.array_equal(r2["wout"][0], r["wout"][0])


def test_rint_is_to_nearest_even_and_the_range_is_symmetric():
    # 16 cells: products 0.5, 1.5, 2.5, -0.5 -> 0, 2, 2, -0; hx = 8: 8 counts, 8.5 -> 8, 9 does not
    u = np.array([0.5, 1.5, 2.5, -0.5, 8.0, 8.5, 9.0, -9.0]) / 16
    idx, inside = K.cells(1.0, 1.0, u, np.zeros(8), 16, 1)
    assert list(idx) == [8, 10, 10, 8, 16, 16, -1, -1] and list(inside) == [True] * 6 + [False] * 2
    # 5 cells: hx = 2 (integer division), 1 x 1: only the origin
    assert list(K.cells(1.0, 1.0, np.array([0.41, 0.5, -0.5, 0.51]), np.zeros(4), 5, 1)[0]) == [4, 4, 0, -1]
    assert list(K.cells(1.0, 1.0, np.array([0.5, -0.5, 0.51, 1.5]), np.zeros(4), 1, 1)[0]) == [0, 0, -1, -1]
    assert K.n_cells(1, 1) == 1 and K.n_cells(5, 3) == 15 and K.n_cells(16, 8) == 153
    # a product that overflows is out of range, not flagged
    d = K.integer_density([1e300], [1.0], [1e300, 0.0], [0.0, 0.0], None, 4, 4)
    assert d["counted"] == [1] and d["outside"] == [1]


def test_flags_and_the_empty_scale():
    nan, inf = np.nan, np.inf
    u = [0.1, nan, 0.1, 0.1, 0.1, 0.1, -inf]
    v = [0.1, 0.1, inf, 0.1, 0.1, 0.1, 0.1]
    w = [2.0, 1.0, 1.0, nan, inf, -1.0, 1.0]
    d, r = both([1.0], [1.0], u, v, w, 8, 8, K.BRIGGS)
    assert d["counted"] == [1] and d["outside"] == [0] and d["w_max"] == 2.0
    assert [float(x) for x in r["wout"][0][1:]] == [0.0] * 6 and float(r["wout"][0][0]) > 0
    # w_max = 0: s = 0 and all zeros; nothing counted: the same
    d, r = both([1.0], [1.0], [0.1, 0.2], [0.1, 0.2], [0.0, -0.0], 8, 8, K.BRIGGS)
    assert d["s"] == 0 and d["counted"] == [2] and not d["W"][0].any() and float(r["f2"][0]) == 0
    assert not np.any(r["wout"][0])
    d, r = both([1.0], [1.0], [0.9], [0.9], None, 8, 8, K.UNIFORM)
    assert d["s"] == 0 and d["counted"] == [0] and d["outside"] == [1] and not np.any(r["wout"][0])


def test_the_shift_keeps_the_total_below_2_62():
    for w_max, n in ((1.0, 1), (0.75, 3), (2.0 ** 20, 5000), (2.0 ** -20 * 0.6, 4), (1e-310, 2), (1e300, 7)):
        s = K.shift(w_max, n)
        e = int(np.frexp(w_max)[1])
        assert w_max < 2.0 ** e if e < 1024 else True
        L = 62 - e - s
        assert 2 ** L >= 2 * n and (L == 0 or 2 ** (L - 1) < 2 * n)
        q = int(np.rint(np.ldexp(w_max, s)))
        assert 2 * n * q <= 2 ** 62
    assert K.shift(0.0, 5) == 0


def test_distinct_cells_with_equal_weights_give_equal_weights():
    # 12 visibilities in 12 cells of 16 x 8, no two of them mirrors, none at the origin
    gu, gv = np.array([1, 2, 3, 4, 5, 6, 7, 8, -1, -2, -3, -4]), np.array([1, 2, 3, 4, -1, -2, -3, -4, 2, 3, 4, 1])
    u, v = gu / 16.0, gv / 8.0
    for mode in (K.UNIFORM, K.BRIGGS):
        d, r = both([1.0], [1.0], u, v, None, 16, 8, mode)
        assert sorted(set(d["W"][0])) == [0.0, 1.0] and d["W"][0].sum() == 24
        assert len(set(float(x) for x in r["wout"][0])) == 1
        assert K.noise_factor(r["wout"][0], np.ones(12)) == 1.0


def clustered(n=1000, seed=5):
    """Half of the weight in one pair of cells, the rest spread over 16 x 8 cells."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-0.45, 0.45, n), rng.uniform(-0.45, 0.45, n)
    u[: n // 2], v[: n // 2] = 3 / 16.0, -2 / 8.0
    return u, v, np.ones(n)


def test_robust_2_is_natural_and_minus_2_is_uniform():
    u, v, w = clustered()
    d, nat = both([1.0], [1.0], u, v, w, 16, 8, K.BRIGGS, robust=2.0)
    ratio = np.asarray(nat["wout"][0] / w, dtype=np.float64)
    assert ratio.max() <= 1.0 and ratio.min() >= 0.98                 # within 2 % of natural
    d, uni = both([1.0], [1.0], u, v, w, 16, 8, K.UNIFORM)
    d, neg = both([1.0], [1.0], u, v, w, 16, 8, K.BRIGGS, robust=-2.0)
    ratio = np.asarray(neg["wout"][0] * neg["f2"][0] / uni["wout"][0], dtype=np.float64)
    assert ratio.max() <= 1.0 and ratio.min() >= 0.95                 # within 5 % of uniform
    # the thermal noise only grows away from natural weighting
    nf = [K.noise_factor(x["wout"][0], w) for x in (nat, neg, uni)]
    assert 1.0 <= nf[0] < 1.001 and nf[0] < nf[1] <= nf[2] * (1 + 1e-12) and nf[2] > 1.5
    rng = np.random.default_rng(3)
    w2 = np.ldexp(rng.uniform(0.5, 1, 1000), rng.integers(-5, 6, 1000))
    d, r = both([1.0], [1.0], u, v, w2, 16, 8, K.BRIGGS, robust=0.5)
    assert K.noise_factor(r["wout"][0], w2) >= 1.0


# ---- the fixed point against the unquantised long-double density -----------------------------------
def big_case():
    """1000 points, 16 x 8 cells, weights over 2^+-20, planted half-integer products and edges."""
    return K.case(16, 8, 1000, 2, seed=17, ties=True)


def test_fixed_point_against_the_long_double_density():
    su, sv, u, v, w = big_case()
    d = K.integer_density(su, sv, u, v, w, 16, 8)
    ref = K.longdouble_density(su, sv, u, v, w, 16, 8)
    assert 0 < min(d["counted"]) and max(d["outside"]) > 0 and min(d["counted"]) < 1000
    for m in range(2):
        W, n_c = K.as_ld(d["Q"][m], d["s"]), d["n_c"][m]
        assert n_c.sum() == 2 * d["counted"][m]
        bound = n_c * LD(2.0) ** (-d["s"] - 1) + n_c * LD(2.0) ** -63 * np.abs(ref[m])
        assert np.all(np.abs(W - ref[m]) <= bound)
        assert np.all((W == 0) == (n_c == 0))
        # sum_c W = 2 sum_k w, exactly
        assert sum(d["Q"][m]) == 2 * d["sum_q"][m]
        assert np.array_equal(d["W"][m], d["W"][m][::-1])              # Hermitian
    # a permutation permutes, nothing else changes
    p = np.random.default_rng(1).permutation(1000)
    d2 = K.integer_density(su, sv, u[p], v[p], w[p], 16, 8)
    assert d2["Q"] == d["Q"] and d2["sum_q"] == d["sum_q"] and d2["s"] == d["s"]


# ---- the emulation inside, the planted mistakes outside --------------------------------------------
@pytest.mark.parametrize("mode, robust", [(K.UNIFORM, 0.0), (K.BRIGGS, 0.5), (K.BRIGGS, -2.0), (K.BRIGGS, 2.0)])
def test_a_float64_emulation_falls_inside_the_bound(mode, robust):
    su, sv, u, v, w = big_case()
    d, r = both(su, sv, u, v, w, 16, 8, mode, robust)
    got, f2, sw2 = K.emulate(d, w, mode, robust)
    for m in range(2):
        assert K.worst_ratio(got[m], r["wout"][m], r["b_wout"][m]) <= 1.0
        assert K.worst_ratio([sw2[m]], [r["sum_w2"][m]], r["b_sum_w2"][m]) <= 1.0
        if mode == K.BRIGGS:
            assert K.worst_ratio([f2[m]], [r["f2"][m]], r["b_f2"][m]) <= 1.0
            assert K.worst_ratio(got[m], r["wout"][m], r["b_wout"][m]) > 0


def moved(a, b):
    """The largest change of a weight relative to itself."""
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    live = a != 0
    return float((np.abs(b[live] - a[live]) / np.abs(a[live])).max())


@pytest.mark.parametrize("planted, mode, robust", [
    (dict(mirror=False), K.UNIFORM, 0.5),
    (dict(origin_twice=False), K.UNIFORM, 0.5),
    (dict(rounding="half_up"), K.UNIFORM, 0.5),
    (dict(rounding="trunc"), K.UNIFORM, 0.5),
    (dict(double_sum_w=False), K.BRIGGS, -2.0),
])
def test_planted_mistakes_fall_outside(planted, mode, robust):
    su, sv, u, v, w = big_case()
    d, r = both(su, sv, u, v, w, 16, 8, mode, robust)
    if "double_sum_w" in planted:
        got = K.emulate(d, w, mode, robust, **planted)[0]
    else:
        dm = K.integer_density(su, sv, u, v, w, 16, 8, **planted)
        got = K.emulate(dm, w, mode, robust)[0]
        # (a mistaken cell rule may drop or add visibilities: compare where both count)
        got = [np.where(d["idx"][m] >= 0, got[m], 0.0) for m in range(2)]
    m = 0                                                # the map with the planted products
    both_count = (np.asarray(r["wout"][m]) != 0) & (got[m] != 0)
    assert moved(np.where(both_count, r["wout"][m], 0), np.where(both_count, got[m], 0)) > 0.4
    assert np.max(np.abs(got[m][both_count].astype(LD) - r["wout"][m][both_count]) /
                  r["wout"][m][both_count]) > 1e6 * r["b_wout"][m]


# ---- check_uv_weights from plain C++, the ABI, the workspace query ------------------------------------
def test_check_uv_weights_from_plain_cpp(tmp_path):
    """check_uv_weights compiled into a stand-alone program by plain g++
    (tests/rjp_args_uvweight_cases.cpp): every refusal, status and message, in the order the check
    makes them -- the messages tests/test_gpu_uvweight.py sees from the library."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "rjp_args_uvweight_cases"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rajepy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rjp_args_uvweight_cases.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        case, status, msg = line.split("\t")
        got[case] = (int(status), msg)
    want = {"null": ["NULL h_su", "NULL h_sv", "NULL d_u", "NULL d_v", "NULL d_wout", "NULL beats sizes"],
            "sizes": ["n_maps 0", "n_vis 0", "nx 0", "nz -1", "sizes beat the scale"],
            "scale": ["su inf", "sv nan", "scale beats the mode"],
            "mode": ["mode 0", "mode 3", "mode beats robust"],
            "robust": ["robust 2.5", "robust below -2", "robust nan", "robust inf"]}
    seen = set()
    for key, cases in want.items():
        for case in cases:
            assert got[case] == (_lib.RJP_ERR_ARG, K.MSG[key]), case
            seen.add(case)
    valid = {c for c in got if c.startswith("valid")}
    assert len(valid) == 4 and all(got[c] == (0, "") for c in valid)
    assert seen | valid == set(got)


def test_abi_signatures_and_the_workspace_query():
    res, args = _lib.SIGNATURES["rjp_uv_weights"]
    P, i32, dbl, DP = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.POINTER(ctypes.c_double)
    assert res is ctypes.c_int64                          # not an `int`: the workgroups of the scatter
    assert args == [P, i32, i32, DP, DP, P, P, P, i32, i32, i32, dbl, P, P, P, P, ctypes.c_size_t, P]
    assert _lib.SIGNATURES["rjp_uv_weights_workspace"] == (ctypes.c_size_t, [i32] * 4)
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    assert "int64_t rjp_uv_weights(rjp_ctx* ctx, int32_t n_maps, int32_t n_vis, const double* h_su" in hdr
    assert "size_t rjp_uv_weights_workspace(int32_t n_maps, int32_t nx, int32_t nz, int32_t n_vis);" in hdr
    assert "classes.py:2775-2776" in hdr and _lib.RJP_VERSION == 117
    lib = _lib.load()
    ws = lib.rjp_uv_weights_workspace
    for a in ((1, 1, 1, 1), (3, 5, 3, 63), (1, 16, 8, 1000), (2, 67, 131, 5000), (1, 501, 501, 1263600),
              (64, 256, 256, 65536), (1, 46339, 46339, 7)):
        assert ws(*a) == K.workspace_bytes(*a) > 0, a
    # 46341^2 cells are more than 2^31 - 1: the call refuses such a grid and the query has no size for it
    assert K.n_cells(46339, 46339) <= 2 ** 31 - 1 < K.n_cells(46340, 46340)
    assert ws(1, 46340, 46340, 7) == K.workspace_bytes(1, 46340, 46340, 7) == 0
    assert ws(1, 2 ** 31 - 1, 2 ** 31 - 1, 1) == 0
    assert ws(1, 1, 1, 1) == 256 + 32 + 8 + 8
    for i in range(4):
        for bad in (0, -1):
            a = [3, 67, 131, 100]
            a[i] = bad
            assert ws(*a) == 0
    assert K.workgroups(3, 257) == 6 and K.workgroups(64, 65536) == 16384
    # a NULL context is refused before anything else
    assert lib.rjp_uv_weights(None, 1, 1, None, None, None, None, None, 1, 1, 2, 0.5, None, None, None,
                              None, 0, None) == _lib.RJP_ERR_ARG


# ---- the Python paths on a recording engine ----------------------------------------------------------
class _RecordingEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def _device_f64(self, values):
        if isinstance(values, torch.Tensor):
            return values
        return torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64).reshape(-1))

    def vis(self, maps, nx, nz, su, sv, u, v):
        self.calls.append(dict(kind="vis"))
        M, K_ = len(su), u.numel()
        return torch.complex(torch.arange(1, M * K_ + 1, dtype=torch.float64).reshape(M, K_),
                             torch.ones(M, K_, dtype=torch.float64))

    def uv_weights(self, u, v, su, sv, nx, nz, w=None, mode="briggs", robust=0.5, want_density=False):
        M, K_ = len(su), u.numel()
        n = len([c for c in self.calls if c["kind"] == "weights"])
        self.calls.append(dict(kind="weights", u=u.clone(), v=v.clone(), su=np.array(su), sv=np.array(sv),
                               nx=nx, nz=nz, w=None if w is None else w.clone(), mode=mode, robust=robust))
        # weight k of map m of call n: (n + 1) (m + 1) / (k + 1)
        out = (n + 1.0) * torch.arange(1, M + 1, dtype=torch.float64)[:, None] / \
            torch.arange(1, K_ + 1, dtype=torch.float64)[None, :]
        self.last_uv_weight_stats = torch.zeros(M, 6, dtype=torch.float64)
        return out

    def vis_adjoint(self, vis, nx, nz, su, sv, u, v, w=None):
        assert vis.dtype == torch.complex128 and vis.is_contiguous()
        M = vis.shape[0]
        self.calls.append(dict(kind="adjoint", vis=vis.clone(), nx=nx, nz=nz, su=np.array(su), u=u.clone(),
                               w=None if w is None else w.clone()))
        n = len([c for c in self.calls if c["kind"] == "adjoint"])
        return (100.0 * n + torch.arange(M, dtype=torch.float64))[:, None].expand(M, nx * nz).clone()

    def clean(self, res, nx, nz, psf, px, pz, n_iter, gain, thresh, mask=None, model=None):
        M = res.shape[0]
        self.calls.append(dict(kind="clean", px=px, pz=pz))
        return (torch.zeros(M, n_iter, dtype=torch.int32), torch.zeros(M, n_iter, dtype=torch.float64),
                torch.zeros(M, dtype=torch.int32), torch.zeros(M, dtype=torch.float64))

    def restore(self, cpix, cflux, ncomp, abc, nx, nz, add=None):
        return add.clone()


def _model(nx, nz):
    from rajepy_amd import classes

    class Model(classes.JetModel):
        """A JetModel that holds only what its imaging front reads: the engine, the grid and the
        distance; the `imaging.Imager` it hands over to is the real one."""

        def __init__(self):
            self._engine, self._nx, self._nz, self._csize = _RecordingEngine(), nx, nz, 0.5
            self._params = {"target": {"dist": 120.}}

    m = Model()
    m._ff_products = lambda freqs, flux=False, device=False, formal=False: torch.zeros(len(freqs), nx * nz)
    m._rrl_flux = lambda line, freqs, lte, contsub, formal=False, device=False: torch.zeros(len(freqs), nx * nz)
    return m


U_M, V_M = np.array([0., 100., -3e3, 2e4]), np.array([0., -50., 1e3, 1e4])
FREQS = np.array([5e9, 2e10, 4e10])
W4 = np.array([1.0, 2.0, 0.5, 4.0])


def kinds(m):
    return [c["kind"] for c in m.engine.calls]


def test_no_weighting_makes_no_weights_call():
    from rajepy_amd import classes
    for weighting in (None, "natural"):
        m = _model(6, 4)
        m.dirty_image_rrl("H66a", U_M, V_M, FREQS, weights=W4, weighting=weighting)
        m.dirty_beam(U_M, V_M, FREQS, weighting=weighting)
        m.dirty_image_ff(U_M, V_M, FREQS, weights=classes.Weighting(weighting, weights=W4))
        m.clean_image_ff(U_M, V_M, FREQS, weights=W4, shape=(5, 5), beam=(0.1, 0.1, 0.), niter=2,
                         weighting=weighting)
        assert "weights" not in kinds(m)
        adj = [c for c in m.engine.calls if c["kind"] == "adjoint"]
        assert adj[0]["w"].tolist() == list(W4) and adj[1]["w"] is None and adj[2]["w"].tolist() == list(W4)
    with pytest.raises(ValueError):
        m.dirty_beam(U_M, V_M, FREQS, weighting="superuniform")
    with pytest.raises(ValueError):
        m.dirty_image_ff(U_M, V_M, FREQS, weights=classes.Weighting("superuniform"))


def test_one_weights_call_per_chunk_multiplied_into_the_visibilities():
    from rajepy_amd import classes, engine as E
    m = _model(6, 4)
    out = m.dirty_image_ff(U_M, V_M, FREQS, weights=classes.Weighting("briggs", -1.0, W4), shape=(9, 7),
                           cell_as=0.01)
    assert kinds(m) == ["vis", "weights", "adjoint"] and out.shape == (3, 9, 7)
    wc, adj = m.engine.calls[1], m.engine.calls[2]
    iu, iv = E.image_scales(FREQS, np.radians(0.01 / 3600.))
    assert (wc["nx"], wc["nz"], wc["mode"], wc["robust"]) == (9, 7, "briggs", -1.0)
    assert np.array_equal(wc["su"], iu) and np.array_equal(wc["sv"], iv) and wc["w"].tolist() == list(W4)
    assert wc["u"].tolist() == list(U_M) and adj["w"] is None
    iw = np.arange(1, 4)[:, None] / np.arange(1., 5.)[None, :]
    V = np.arange(1., 13.).reshape(3, 4)
    assert np.array_equal(adj["vis"].real.numpy(), V * iw) and np.array_equal(adj["vis"].imag.numpy(), iw)
    for f in range(3):
        assert np.all(out[f] == (100.0 + f) / torch.tensor(iw[f]).sum().item())   # its own sum of w'
    # chunks: the [F, K] weights stay under VIS_STACK_BYTES too
    m2 = _model(6, 4)
    m2.VIS_STACK_BYTES = 2 * 4 * 8
    m2.dirty_beam(U_M, V_M, FREQS, shape=(2, 1), weighting="uniform")
    assert kinds(m2) == ["weights", "adjoint", "weights", "adjoint"]
    assert [len(c["su"]) for c in m2.engine.calls] == [2, 2, 1, 1]
    assert m2.engine.calls[0]["mode"] == "uniform" and m2.engine.calls[0]["w"] is None


def test_mfs_has_one_density_over_all_points():
    from rajepy_amd import engine as E
    m = _model(6, 4)
    out = m.dirty_image_rrl("H66a", U_M, V_M, FREQS, weights=W4, shape=(9, 7), mfs=True, weighting="uniform")
    assert kinds(m) == ["vis", "weights", "adjoint"] and out.shape == (1, 9, 7)
    wc, adj = m.engine.calls[1], m.engine.calls[2]
    su, sv = E.vis_scales(FREQS, 0.5, 120.)
    assert list(wc["su"]) == [1.0] and list(wc["sv"]) == [1.0] and (wc["nx"], wc["nz"]) == (9, 7)
    assert np.array_equal(wc["u"].numpy().reshape(3, 4), su[:, None] * U_M[None, :])
    assert np.array_equal(wc["v"].numpy().reshape(3, 4), sv[:, None] * V_M[None, :])
    assert np.array_equal(wc["w"].numpy(), np.tile(W4, 3))
    assert torch.equal(adj["u"], wc["u"]) and adj["w"] is None and adj["vis"].shape == (1, 12)
    iw = 1.0 / np.arange(1., 13.)
    assert np.array_equal(adj["vis"].real.numpy()[0], np.arange(1., 13.) * iw)
    assert np.all(out == 100.0 / torch.tensor(iw).sum().item())


def test_clean_weighs_on_the_image_grid_once_per_chunk_for_image_and_beam():
    m = _model(6, 4)
    res = m.clean_image_ff(U_M, V_M, FREQS, weights=W4, shape=(5, 5), cell_as=0.01, beam=(0.1, 0.1, 0.),
                           niter=2, weighting="briggs", robust=0.0)
    assert kinds(m) == ["vis", "weights", "adjoint", "adjoint", "clean"] and res.image.shape == (3, 5, 5)
    wc, img, psf = m.engine.calls[1:4]
    assert (wc["nx"], wc["nz"]) == (5, 5) and (img["nx"], img["nz"]) == (5, 5) and (psf["nx"], psf["nz"]) == (9, 9)
    iw = np.arange(1, 4)[:, None] / np.arange(1., 5.)[None, :]
    assert np.array_equal(psf["vis"].real.numpy(), iw) and not psf["vis"].imag.any()     # the same weights
    assert np.array_equal(img["vis"].imag.numpy(), iw) and img["w"] is None and psf["w"] is None
    # chunks of channels: one weights call each; mfs: one call for everything
    m2 = _model(6, 4)
    m2.VIS_STACK_BYTES = (3 * 5 * 5 + 9 * 9) * 8             # one channel's images and beam
    m2.clean_image_ff(U_M, V_M, FREQS, shape=(5, 5), beam=(0.1, 0.1, 0.), niter=2, weighting="uniform")
    assert kinds(m2)[1:] == ["weights", "adjoint", "adjoint", "clean"] * 3
    m3 = _model(6, 4)
    m3.clean_image_ff(U_M, V_M, FREQS, shape=(5, 5), beam=(0.1, 0.1, 0.), niter=2, weighting="uniform", mfs=True)
    assert kinds(m3) == ["vis", "weights", "adjoint", "adjoint", "clean"]
    assert (m3.engine.calls[1]["nx"], m3.engine.calls[3]["nx"]) == (5, 9) and len(m3.engine.calls[1]["su"]) == 1


def test_imaging_weights_returns_the_rows_and_the_statistics():
    m = _model(6, 4)
    iw, st = m.imaging_weights(U_M, V_M, FREQS, weights=W4, shape=(9, 7), cell_as=0.01)
    assert kinds(m) == ["weights"] and iw.shape == (3, 4)
    want = np.arange(1, 4)[:, None] / np.arange(1., 5.)[None, :]
    assert np.array_equal(iw, want) and st["noise_factor"].shape == (3,)
    nf = np.sqrt((want ** 2 / W4).sum(axis=1) * W4.sum()) / want.sum(axis=1)
    assert np.allclose(st["noise_factor"], nf, rtol=1e-14) and np.all(st["noise_factor"] >= 1)
    assert set(st) == {"sum_w", "sum_w2", "f2", "counted", "out_of_range", "shift", "sum_wout", "noise_factor"}
    iw, st = m.imaging_weights(U_M, V_M, FREQS, weights=W4, shape=(9, 7), mfs=True, weighting="uniform")
    assert iw.shape == (3, 4) and st["noise_factor"].shape == (1,) and m.engine.calls[-1]["mode"] == "uniform"
    n = len(m.engine.calls)
    ub = U_M.copy()
    ub[1] = np.nan
    iw, st = m.imaging_weights(ub, V_M, FREQS, weights=W4, weighting="natural")
    assert len(m.engine.calls) == n and np.array_equal(iw, np.tile([1.0, 0.0, 0.5, 4.0], (3, 1)))
    assert np.all(st["noise_factor"] == 1) and np.all(st["sum_w"] == 5.5) and np.all(st["counted"] == 3)


def test_public_surface():
    from rajepy_amd import classes, engine as E
    J = classes.JetModel
    p = inspect.signature(E.RTEngine.uv_weights).parameters
    assert list(p) == ["self", "u", "v", "su", "sv", "nx", "nz", "w", "mode", "robust", "want_density"]
    assert [p[k].default for k in list(p)[7:]] == [None, "briggs", 0.5, False]
    for name in ("dirty_image_rrl", "dirty_beam", "clean_image_ff", "clean_image_rrl"):
        p = inspect.signature(getattr(J, name)).parameters
        assert p["weighting"].default is None and p["robust"].default == 0.5, name
    p = inspect.signature(J.imaging_weights).parameters
    assert list(p) == ["self", "u_m", "v_m", "freq", "weights", "shape", "cell_as", "weighting", "robust", "mfs"]
    assert (p["weighting"].default, p["robust"].default, p["mfs"].default) == ("briggs", 0.5, False)
    assert classes.Weighting() == ("briggs", 0.5, None)
    assert E.RTEngine.UV_WEIGHT_MODES == {"uniform": 1, "briggs": 2}
