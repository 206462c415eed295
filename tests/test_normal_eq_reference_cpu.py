"""tests/normal_eq_ref.py -- the long-double reference that tests/test_gpu_normal_eq.py holds K23
(rjp_normal_eq) to -- pinned on the CPU: hand-worked cases (one sample; two samples of opposite
phase; a zero weight beside a NaN datum), a float64 emulation on every GPU case's inputs (inside
the derived bound), five planted mistakes (outside), check_normal_eq from plain C++, the ABI table,
`lm_minimise` against tests/lm_ref.py on a toy sum of Gaussians with every status reached,
`RTEngine.normal_eq` and both `fit_ejections_*` paths on a recording engine, and
`set_ejection_event` against `add_ejection_event`.  No GPU."""
import copy
import ctypes
import inspect
import os
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from rajepy_amd import _lib, classes, inference, logger
from rajepy_amd import engine as E
from tests import gpu_util as U
from tests import lm_ref
from tests import normal_eq_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YEAR = 31557600.0


# ---- by hand -------------------------------------------------------------------------------------------
def test_one_sample_by_hand():
    """y = 3 + 4i, m = 1 + i: r = 2 + 3i, w = 2.  J_0 = 1 - i, J_1 = 2i.  chi2 = 2 x 13; g_0 = 2 Re((1 + i)(2 +
    3i)) = 2 (2 - 3); g_1 = 2 Re(-2i (2 + 3i)) = 2 x 6; N_00 = 2 x 2, N_01 = 2 Re((1 + i) 2i) = -4, N_11 = 8."""
    case = dict(data=np.array([[3 + 4j]]), model=np.array([[1 + 1j]]), dmodel=np.array([[[1 - 1j], [2j]]]),
                sel=[0, 1], w=np.array([2.0]), n_part=2)
    ref = K.reference(case)
    assert ref["count"] == 1 and float(ref["chi2"]) == 26.0
    assert ref["g"].astype(float).tolist() == [-2.0, 12.0] and ref["N"].astype(float).tolist() == [4.0, -4.0, 8.0]
    # the selection permutes the outputs
    ref = K.reference(dict(case, sel=[1, 0]))
    assert ref["g"].astype(float).tolist() == [12.0, -2.0] and ref["N"].astype(float).tolist() == [8.0, -4.0, 4.0]


def test_two_samples_of_opposite_phase_by_hand():
    """J = (1, -1), r = (1, 1): g = 1 - 1 = 0, N = 2, chi2 = 2; as real samples and as complex ones turned by i."""
    for n_part, ph in ((1, 1.0), (2, 1j)):
        case = dict(data=np.array([[2.0, 2.0]]) * ph, model=np.array([[1.0, 1.0]]) * ph,
                    dmodel=np.array([[[1.0, -1.0]]]) * ph, sel=[0], w=None, n_part=n_part)
        ref = K.reference(case)
        assert (ref["count"], float(ref["chi2"]), float(ref["g"][0]), float(ref["N"][0])) == (2, 2.0, 0.0, 2.0)


def test_a_zero_weight_beside_a_nan_datum_by_hand():
    """w = (0, 1, 1), y = (5, NaN, 2), m = (0, 0, 1), J = (7, 7, 3): the third sample alone counts."""
    case = dict(data=np.array([[5.0, np.nan, 2.0]]), model=np.array([[0.0, 0.0, 1.0]]),
                dmodel=np.array([[[7.0, 7.0, 3.0]]]), sel=[0], w=np.array([0.0, 1.0, 1.0]), n_part=1)
    ref = K.reference(case)
    assert (ref["count"], float(ref["chi2"]), float(ref["g"][0]), float(ref["N"][0])) == (1, 1.0, 3.0, 9.0)
    # ... whatever the model or the derivative of the other two hold
    case["model"][0, :2] = np.nan
    case["dmodel"][0, 0, :2] = np.inf
    ref = K.reference(case)
    assert (ref["count"], float(ref["chi2"]), float(ref["g"][0]), float(ref["N"][0])) == (1, 1.0, 3.0, 9.0)
    assert K.workgroups(1, 512) == 1 and K.workgroups(3, 171) == 2 and K.workspace_bytes(2, 512, 3) == 2 * 11 * 8


# ---- the emulation on the GPU cases, and the planted mistakes ------------------------------------------
@pytest.mark.parametrize("n_rows,n_vis,n_part,n_sel,n_par,wkind", K.SIZED)
def test_emulation_on_the_sized_cases(n_rows, n_vis, n_part, n_sel, n_par, wkind):
    case = K.sized(n_rows, n_vis, n_part, n_sel, n_par, wkind)
    ref = K.reference(case)
    got = K.emulate(case)
    assert K.judge(got, ref, n_part) <= 1.0
    assert np.all(np.isfinite(got["N"])) and np.all(np.isfinite(got["g"]))
    if n_rows * n_vis > 1:
        assert 0 < ref["count"] < n_rows * n_vis, "the GPU case would be vacuous"
    if n_rows >= 3:
        assert not K.counting(case["data"], case["w"], n_part)[1].any()        # a row with nothing counting


def test_emulation_on_the_nan_plane():
    case, j = K.nan_plane()
    ref, got = K.reference(case), K.emulate(case)
    tg, tN = K.touches(len(case["sel"]), j)
    assert np.array_equal(np.isnan(ref["g"]), tg) and np.array_equal(np.isnan(ref["N"]), tN) and tN.sum() == 5
    assert K.judge(got, ref, 2) <= 1.0
    got["g"][j] = 0.0                                           # a NaN on one side alone is a failure
    assert K.judge(got, ref, 2) == float("inf")


@pytest.mark.parametrize("mistake", ["no_conj", "w_squared", "drop_imag", "ignore_sel", "add_noncounting"])
def test_planted_mistakes_land_outside(mistake):
    case = K.sized(3, 513, 2, 5, 8, "rows")
    dead = ~K.counting(case["data"], case["w"], 2)
    assert dead.any() and not np.array_equal(case["sel"], np.arange(5))
    # finite derivatives where nothing counts, so that adding them is a wrong number, not a NaN
    case["dmodel"][np.broadcast_to(dead[:, None, :], case["dmodel"].shape)] = 1.0 + 1.0j
    ref = K.reference(case)
    assert K.judge(K.emulate(case), ref, 2) <= 1.0
    assert K.judge(K.emulate(case, mistake), ref, 2) > 1e3


# ---- the argument checks and the ABI ------------------------------------------------------------------
def test_checks_from_plain_cpp(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "rjp_args_normal_eq_cases"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rajepy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rjp_args_normal_eq_cases.cpp"), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        case, status, msg = line.split("\t")
        got[case] = (int(status), msg)
    want = {"null": ["NULL d_data", "NULL d_model", "NULL d_out", "NULL d_count", "NULL beats sizes"],
            "count": ["n_rows 0", "n_vis -1", "sizes beat n_part"],
            "part": ["n_part 0", "n_part 3", "n_part beats n_sel"],
            "nsel": ["n_sel -1", "n_sel 49", "n_sel beats the NULLs"],
            "needs": ["NULL d_dmodel", "NULL h_sel", "the NULLs beat n_par"],
            "npar": ["n_par 2", "n_par beats the indices"],
            "range": ["index -1", "index n_par", "range beats repeat"],
            "repeat": ["repeat", "repeat beats w_rows"],
            "wrows": ["w_rows 0", "w_rows 2", "w_rows beats the workgroups"],
            "wgs": ["2^31 workgroups", "2^60 samples"]}
    seen = set()
    for key, cases in want.items():
        for case in cases:
            assert got[case] == (_lib.RJP_ERR_ARG, K.MSG[key]), case
            seen.add(case)
    valid = {c for c in got if c.startswith("valid")}
    assert len(valid) == 6 and all(got[c] == (0, "") for c in valid)
    assert seen | valid == set(got)


def test_abi_signatures():
    P, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    IP = ctypes.POINTER(ctypes.c_int32)
    assert _lib.SIGNATURES["rjp_normal_eq_workspace"] == (ctypes.c_size_t, [i64, i32, i32])
    assert _lib.SIGNATURES["rjp_normal_eq"] == (i64, [P, P, P, P, i64, i32, i32, i32, IP, i32, P, i64, P, P, P,
                                                      ctypes.c_size_t, P])
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    assert "int64_t rjp_normal_eq(rjp_ctx* ctx, const double* d_data, const double* d_model," in hdr
    assert "size_t rjp_normal_eq_workspace(int64_t n_rows, int32_t n_vis, int32_t n_sel);" in hdr
    assert "#define RJP_NORMAL_EQ_MAX_SEL 48" in hdr and "#define RJP_VERSION 117" in hdr   # symbols added, none changed
    assert inference.NORMAL_EQ_MAX_SEL == K.MAX_SEL == E.NORMAL_EQ_MAX_SEL == 48
    assert E.lm_minimise is inference.lm_minimise and E.BurstFit is inference.BurstFit
    assert classes.EjectionFit is inference.EjectionFit
    lib = _lib.load()
    assert lib.rjp_normal_eq(None, None, None, None, 1, 1, 2, 0, None, 0, None, 1, None, None, None, 0,
                             None) == _lib.RJP_ERR_ARG
    for args in ((1, 1, 0), (3, 171, 3), (5, 1573, 48)):
        assert lib.rjp_normal_eq_workspace(*args) == K.workspace_bytes(*args)
    assert lib.rjp_normal_eq_workspace(0, 1, 0) == 0 and lib.rjp_normal_eq_workspace(1, 1, 49) == 0
    assert lib.rjp_normal_eq_workspace(2 ** 40, 2 ** 20, 0) == 0
    assert lib.rjp_normal_eq_workspace((2 ** 31 - 1) * 512, 1, 0) == (2 ** 31 - 1) * 16


# ---- lm_minimise on a toy problem -----------------------------------------------------------------------
X = np.linspace(-4.0, 6.0, 81)
TRUTH = np.array([2.0, -0.5, 0.8, 1.2, 2.5, 1.1])          # two Gaussians: amplitude, centre, width


def toy_model(th):
    y = np.zeros_like(X)
    J = np.zeros((X.size, th.size))
    for c in range(th.size // 3):
        a, x0, s = th[3 * c:3 * c + 3]
        e = np.exp(-0.5 * ((X - x0) / s) ** 2)
        y += a * e
        J[:, 3 * c] = e
        J[:, 3 * c + 1] = a * e * (X - x0) / s ** 2
        J[:, 3 * c + 2] = a * e * (X - x0) ** 2 / s ** 3
    return y, J


def toy(data, calls=None):
    def evaluate(th, want_jac):
        if calls is not None:
            calls.append(bool(want_jac))
        y, J = toy_model(th)
        r = data - y
        return (float(r @ r), J.T @ r, J.T @ J) if want_jac else (float(r @ r), None, None)
    return evaluate


def toy_feasible(th):
    return bool(np.all(th[2::3] > 0))


def follow(rows, free, lambda0):
    """Every row of a trace against the rule restated with tests/lm_ref.py: the accept decisions, the
    lambda sequence, and every trial = the current point + the damped Cholesky step."""
    cur, chi_cur, lam, N, g = None, np.inf, lambda0, None, None
    for i, row in enumerate(rows):
        if i:
            while True:
                delta, ok = lm_ref.cholesky_solve(lm_ref.damped(N, lam), g)
                if ok:
                    break
                lam *= 10.0
            assert row["lam"] == lam
            assert np.allclose(row["theta"], cur + delta, rtol=1e-12, atol=1e-300)
            assert np.array_equal(row["theta"][~free], cur[~free])
        acc = toy_feasible(row["theta"]) and np.isfinite(row["chi2"]) and row["chi2"] < chi_cur
        assert row["accepted"] == acc
        if acc:
            cur, chi_cur, N, g = row["theta"], row["chi2"], row["N"], row["g"]
            for k in np.nonzero(~free)[0]:
                assert g[k] == 0 and N[k, k] == 1 and not N[k, np.arange(N.shape[0]) != k].any()
            lam = max(lam / 10.0, lm_ref.LAM_MIN) if i else lam
        else:
            lam *= 10.0
    return cur, chi_cur, lam


def test_lm_minimise_follows_the_rule_and_reaches_every_status():
    data = toy_model(TRUTH)[0]
    start = TRUTH * np.array([1.1, 1.3, 0.9, 0.9, 1.05, 1.1])
    free = np.array([True, True, True, True, False, True])
    calls = []
    res = E.lm_minimise(toy(data, calls), start, free, toy_feasible, lambda th: np.abs(th) + 1.0, n_iter=60,
                        lambda0=1e-3, xtol=1e-10, trace=True)
    assert res.status == 1 and res.niter == len(res.trace) < 60
    cur, chi_cur, _ = follow(res.trace, free, 1e-3)
    assert np.array_equal(cur, res.theta) and chi_cur == res.chi2
    assert res.theta[4] == start[4]                                        # a held parameter keeps its bits
    truth = TRUTH.copy()
    assert np.max(np.abs(res.theta - truth)[free]) < 0.15                  # (the held centre is 5 % off)
    chis = [r["chi2"] for r in res.trace if r["accepted"]]
    assert all(b < a for a, b in zip(chis, chis[1:]))
    # derivatives: at the start, and once more per accepted trial -- never for a rejected one
    n_acc = sum(r["accepted"] for r in res.trace)
    assert calls[0] is True and sum(calls) == n_acc and len(calls) == len(res.trace) + n_acc - 1
    # all free from a near start: the truth to rounding, status 1
    res = E.lm_minimise(toy(data), TRUTH * 1.02, None, toy_feasible, None, 40, 1e-3, 1e-9, True)
    assert res.status == 1 and np.max(np.abs(res.theta - TRUTH)) < 1e-7
    follow(res.trace, np.ones(6, dtype=bool), 1e-3)
    # a start that is the truth: chi2 = 0 exactly -> status 1 after one trial
    res = E.lm_minimise(toy(data), TRUTH, None, toy_feasible)
    assert res.status == 1 and res.niter == 1 and res.chi2 == 0.0
    # status 0: the trials run out
    res = E.lm_minimise(toy(data), start, None, toy_feasible, n_iter=3, trace=True)
    assert res.status == 0 and res.niter == 3 and len(res.trace) == 3
    # status 2: a chi2 that never falls again
    seq = iter([5.0] + [6.0] * 100)
    res = E.lm_minimise(lambda th, j: (next(seq), np.ones(2), np.eye(2)), np.zeros(2), n_iter=100, xtol=1e-300,
                        trace=True)
    assert res.status == 2 and res.lam > 1e12 and not any(r["accepted"] for r in res.trace[1:])
    # (lambda = 1e-3 x 10^k after k rejections: above 1e12 at k = 16, the 17th trial)
    assert res.niter == 17 and [r["lam"] for r in res.trace[1:4]] == [1e-3, 1e-2, 1e-1]
    # ... and a matrix whose pivots fail whatever lambda: status 2 at the first solve
    res = E.lm_minimise(lambda th, j: (5.0, np.ones(2), -np.eye(2)), np.zeros(2))
    assert res.status == 2 and res.niter == 1
    # status 3: an infeasible or non-finite start, or a first chi2 that is not finite; nothing evaluated or kept
    calls = []
    bad = TRUTH.copy()
    bad[2] = -1.0
    res = E.lm_minimise(toy(data, calls), bad, None, toy_feasible)
    assert res.status == 3 and res.niter == 0 and calls == [] and res.N is None
    bad[2] = np.nan
    assert E.lm_minimise(toy(data), bad).status == 3
    assert E.lm_minimise(lambda th, j: (np.inf, np.ones(2), np.eye(2)), np.zeros(2)).status == 3
    # an infeasible trial is rejected without an evaluation
    calls = []
    big = lambda th, j: (calls.append(j), (float((th[0] - 5) ** 2), np.array([5 - th[0]]), np.array([[1e-4]])))[1]
    res = E.lm_minimise(big, np.array([0.0]), None, lambda th: th[0] < 100.0, n_iter=4, trace=True)
    assert res.trace[1]["theta"][0] > 100.0 and not res.trace[1]["accepted"] and np.isnan(res.trace[1]["chi2"])
    assert calls == [True] and res.trace[2]["lam"] == 1e-2
    with pytest.raises(ValueError):
        E.lm_minimise(toy(data), TRUTH, n_iter=0)
    with pytest.raises(ValueError):
        E.lm_minimise(toy(data), TRUTH, free=[True])


def test_cholesky_solve_against_lm_ref():
    rng = np.random.default_rng(5)
    A = rng.standard_normal((7, 7))
    N, g = A @ A.T + 0.1 * np.eye(7), rng.standard_normal(7)
    for lam in (1e-12, 1e-3, 10.0):
        M = lm_ref.damped(N, lam)
        want, ok = lm_ref.cholesky_solve(M, g)
        got, ok2 = inference.cholesky_solve(N + np.diag(lam * np.diag(N)), g)
        assert ok and ok2 and np.allclose(got, want, rtol=1e-12, atol=0)
    assert not inference.cholesky_solve(-N, g)[1]
    assert np.array_equal(inference.unpack_triangle(lm_ref.pack(N), 7), lm_ref.unpack(lm_ref.pack(N), 7))


# ---- RTEngine.normal_eq on a recording library --------------------------------------------------------
class _Engine(E.RTEngine):
    """RTEngine.normal_eq without a device: the library call is recorded."""

    def __init__(self):
        self.device = torch.device("cpu")
        self._work, self.calls, self.ctx = None, [], None
        self.lib = types.SimpleNamespace(rjp_normal_eq_workspace=K.workspace_bytes)

    def _call_tiles(self, name, *args):
        self.calls.append((name, args))
        return 7


def test_engine_normal_eq_hands_over_what_it_was_given():
    eng = _Engine()
    case = K.sized(3, 40, 2, 3, 6, "rows")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    chi2, g, N, count = eng.normal_eq(t(case["data"]), t(case["model"]), t(case["dmodel"]), case["sel"], t(case["w"]))
    (name, a), = eng.calls
    assert name == "rjp_normal_eq" and a[3:7] == (3, 40, 2, 6) and a[8] == 3 and a[10] == 3
    assert [a[7][i] for i in range(3)] == case["sel"].tolist() and a[14] >= K.workspace_bytes(3, 40, 3)
    assert chi2.dim() == 0 and tuple(g.shape) == (3,) and tuple(N.shape) == (6,) and count.dtype == torch.int64
    assert eng.last_normal_eq_workgroups == 7
    # real samples, shared weights, no planes and no derivative stack
    eng.calls.clear()
    _, g, N, _ = eng.normal_eq(t(case["data"].real), t(case["model"].real), None, [], t(case["w"][0]))
    (name, a), = eng.calls
    assert a[2] is None and a[3:7] == (3, 40, 1, 0) and a[8] == 0 and a[10] == 1 and g.numel() == 0 == N.numel()
    # float64 [..., 2] stacks are complex samples
    eng.normal_eq(torch.view_as_real(t(case["data"])), torch.view_as_real(t(case["model"])),
                  torch.view_as_real(t(case["dmodel"])), [5], None)
    assert eng.calls[-1][1][5] == 2 and eng.calls[-1][1][9] is None
    for bad in (dict(sel=[0, 0]), dict(sel=[6]), dict(sel=list(range(49))), dict(w=t(case["w"][0, :7])),
                dict(model=t(case["model"][:2])), dict(dmodel=t(case["dmodel"].real)), dict(dmodel=None)):
        kw = dict(data=t(case["data"]), model=t(case["model"]), dmodel=t(case["dmodel"]), sel=[1], w=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            eng.normal_eq(kw["data"], kw["model"], kw["dmodel"], kw["sel"], kw["w"])


# ---- both fit paths on a recording engine --------------------------------------------------------------
class _NoHost(torch.Tensor):
    """A tensor that must stay where it is."""

    def cpu(self, *a, **k):
        raise AssertionError("maps, visibilities and derivatives must not be copied to the host")

    numpy = tolist = __array__ = cpu


def _nohost(*shape, complex_=False):
    return torch.ones(*shape, dtype=torch.complex128 if complex_ else torch.float64).as_subclass(_NoHost)


class _Recorder:
    """The engine calls of a fit, recorded; `normal_eq` answers from a script: chi2 of evaluation i is
    `script[i]` (a call without planes starts a new evaluation, a call with planes repeats the current
    one -- or starts the first), split evenly over the chunks; g and N are fixed random numbers."""
    device = torch.device("cpu")
    NPIX = 6

    def __init__(self, script, chunks=1):
        self.calls, self.script, self.chunks, self.at, self.seen = [], script, chunks, -1, 0
        rng = np.random.default_rng(11)
        A = rng.standard_normal((48, 48))
        # (N so large that every step is far below an ulp of its parameter: the script alone decides)
        self.N_raw, self.g_raw = 1e40 * (A @ A.T + np.eye(48)), rng.standard_normal(48)

    def _device_f64(self, values):
        if not isinstance(values, torch.Tensor):
            values = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64))
        return values.to(torch.float64).reshape(-1).contiguous()

    def _bursts(self, b):
        return [[(b.t0[j][i], b.amp_rel[j][i], b.inv2s2[j][i]) for i in range(b.n[j])] for j in range(2)]

    def ff_grad(self, fields, bursts, epochs_s, gff_mode, tavg=None, ctau=None, cflux=None, want_maps=False):
        self.calls.append(dict(kind="ff_grad", E=len(epochs_s), bursts=self._bursts(bursts)))
        n_par = 3 * (bursts.n[0] + bursts.n[1])
        return None, None, _nohost(len(epochs_s), len(ctau)), _nohost(len(epochs_s), len(ctau), n_par)

    def ff_formal_grad(self, fields, bursts, epochs_s, gff_mode, ctau, csrc, want_maps=False):
        self.calls.append(dict(kind="ff_formal_grad", E=len(epochs_s), maps=want_maps, bursts=self._bursts(bursts)))
        n_par, Ee, F = 3 * (bursts.n[0] + bursts.n[1]), len(epochs_s), len(ctau)
        return _nohost(Ee, F), _nohost(Ee, F, n_par), _nohost(Ee, F, n_par, self.NPIX) if want_maps else None

    def ff_formal_sweep(self, fields, bursts, epochs_s, gff_mode, ctau, csrc, want_maps=False, want_totals=True):
        self.calls.append(dict(kind="ff_formal_sweep", E=len(epochs_s), maps=want_maps))
        Ee, F = len(epochs_s), len(ctau)
        return (_nohost(Ee, F, self.NPIX) if want_maps else None), (_nohost(Ee, F) if want_totals else None)

    def ff_scan(self, fields, bursts, epochs_s, gff_mode, want_em=True, out=None, want_tavg=True):
        self.calls.append(dict(kind="ff_scan", E=len(epochs_s), em=want_em))
        return _nohost(len(epochs_s), self.NPIX), None, None

    def ff_maps(self, sumA, tavg, ctau, cflux, want_tau=True, want_flux=True, want_ftot=True, out=None):
        self.calls.append(dict(kind="ff_maps", flux=want_flux, tau=want_tau))
        return None, None, _nohost(sumA.shape[0], len(ctau))

    def vis(self, maps, nx, nz, su, sv, u, v):
        assert isinstance(maps, _NoHost)
        M = maps.numel() // self.NPIX
        self.calls.append(dict(kind="vis", M=M, K=int(u.numel()), su=np.array(su), u=u.clone()))
        return _nohost(M, int(u.numel()), complex_=True)

    def normal_eq(self, data, model, dmodel, sel, weights=None):
        assert isinstance(model, _NoHost) and (dmodel is None or isinstance(dmodel, _NoHost))
        sel = np.asarray(sel, dtype=np.int64)
        if self.seen % self.chunks == 0 and (sel.size == 0 or self.at < 0):
            self.at += 1
        self.seen += 1
        self.calls.append(dict(kind="normal_eq", sel=sel.copy(), rows=int(data.shape[0]), n_vis=int(data.shape[1]),
                               dshape=None if dmodel is None else tuple(dmodel.shape), w=weights,
                               complex_=data.dtype == torch.complex128))
        N = self.N_raw[np.ix_(sel, sel)] / self.chunks
        return (torch.tensor(self.script[self.at] / self.chunks, dtype=torch.float64),
                torch.from_numpy(self.g_raw[sel] / self.chunks),
                torch.from_numpy(N[np.triu_indices(sel.size)].copy()), torch.tensor(5, dtype=torch.int64))


def tilted_model(tmp_path, engine):
    p = copy.deepcopy(U.load_golden("tilted")[2])
    for k in ("mod_r_0",):
        p["geometry"].pop(k, None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    jm = classes.JetModel(p, log=logger.Log(str(tmp_path / "m.log"), verbose=False), engine=engine)
    jm._dev = types.SimpleNamespace(a0=1, a0_mode=jm.gff_mode, ts=1)       # never built: no device
    jm._tavg = torch.ones(3)
    jm._nx, jm._nz = 2, 3                                                  # (maps of 6 pixels)
    return jm


RB_TIE = [[("1", n), ("2", n)] for n in ("t_0", "peak_jml", "half_life")]
SCRIPT = [10.0, 5.0, 7.0, 4.0, 4.5, 3.0, 2.0, 1.0]


def expected_fit_space(jm, rec, sel_planes):
    """T^T D N D T and T^T D g by hand for the tilted model: planes 0-2 ejection '1' (red), 3-5 '2', 6-8 '3'."""
    chain = []
    for k, ej in jm.ejections.items():
        chain += list(classes.ejection_chain_rule(ej["t_0"], ej["peak_jml"], ej["half_life"], jm.ss_jml(ej["which"]))[1])
    chain = np.array(chain)
    n = 9
    N, g = np.zeros((n, n)), np.zeros(n)
    N[np.ix_(sel_planes, sel_planes)] = rec.N_raw[np.ix_(sel_planes, sel_planes)]
    g[sel_planes] = rec.g_raw[sel_planes]
    N, g = N * np.outer(chain, chain), g * chain
    T = np.zeros((9, 6))
    ej = list(jm.ejections.values())
    for c in range(3):
        name = inference.PARAM_NAMES[c]
        T[c, c], T[3 + c, c], T[6 + c, 3 + c] = 1.0, ej[1][name] / ej[0][name], 1.0
    return T.T @ N @ T, T.T @ g, T


def test_fit_ejections_flux_on_a_recording_engine(tmp_path):
    for formal in (False, True):
        rec = _Recorder(SCRIPT)
        jm = tilted_model(tmp_path, rec)
        before = copy.deepcopy(jm.ejections), copy.deepcopy(jm._bursts), jm._version
        times, freq = np.array([0.5, 1.0, 1.5, 2.0]) * YEAR, [5e9, 1.5e9]
        R = jm.fit_ejections_flux(times, freq, np.ones((4, 2)), sigma=0.5, formal=formal, tie=RB_TIE,
                                  free={"1": ["t_0", "peak_jml", "half_life"], "2": ["t_0", "peak_jml", "half_life"],
                                        "3": ["t_0", "peak_jml"]}, n_iter=6, xtol=1e-300, trace=True)
        # trials: the start (derivatives), 5 accepted, 7 rejected, 4 accepted, 4.5 rejected, 3 accepted
        assert [r["accepted"] for r in R.trace] == [True, True, False, True, False, True] and R.status == 0
        assert R.chi2 == 3.0 and R.niter == 6 and R.ndata == 5 and np.isnan(R.reduced_chi2)     # (5 data, 5 free)
        jac = "ff_formal_grad" if formal else "ff_grad"
        trial = ["ff_formal_sweep"] if formal else ["ff_scan", "ff_maps"]
        kinds = [c["kind"] for c in rec.calls]
        one_jac, one_trial = [jac, "normal_eq"], trial + ["normal_eq"]
        assert kinds == one_jac + (one_trial + one_jac) + one_trial + (one_trial + one_jac) + one_trial + \
            (one_trial + one_jac)                      # a rejected trial requests no derivatives
        ne = [c for c in rec.calls if c["kind"] == "normal_eq"]
        assert all(c["rows"] == 8 and c["n_vis"] == 1 and not c["complex_"] for c in ne)
        assert all(c["dshape"] in (None, (8, 9, 1)) for c in ne)
        assert all(torch.equal(c["w"], torch.full((8, 1), 4.0, dtype=torch.float64)) for c in ne)
        with_planes = [c for c in ne if c["sel"].size]
        assert all(c["sel"].tolist() == list(range(8)) for c in with_planes) and len(with_planes) == 4
        assert all(c["dshape"] is None for c in ne if not c["sel"].size)
        if not formal:
            assert all(c["em"] is False for c in rec.calls if c["kind"] == "ff_scan")
            assert all(not c["flux"] and not c["tau"] for c in rec.calls if c["kind"] == "ff_maps")
        # the first row: T^T (D N D) T with the identity's row for the held half_life of ejection 3
        N_fit, g_fit, T = expected_fit_space(jm, rec, list(range(8)))
        row = R.trace[0]
        assert np.allclose(row["N"][:5, :5], N_fit[:5, :5], rtol=1e-13, atol=0)
        assert np.allclose(row["g"][:5], g_fit[:5], rtol=1e-13, atol=0)
        assert row["g"][5] == 0 and row["N"][5, 5] == 1 and not row["N"][5, :5].any() and not row["N"][:5, 5].any()
        # the bursts of the start are the model's own, bit for bit; the model is untouched
        first = [c for c in rec.calls if c["kind"] == jac][0]["bursts"]
        want = [[(t0, a, 1.0 / (2.0 * s ** 2.0)) for t0, a, s in jm._bursts[j]] for j in "RB"]
        assert first == want
        assert (jm.ejections, jm._bursts, jm._version) == before
        # ties and holds in the result
        th = R.theta
        assert th[0, 0] == th[1, 0] and th[0, 2] == th[1, 2]
        assert th[1, 1] / th[0, 1] == pytest.approx(jm.ss_jml("B") / jm.ss_jml("R"), rel=1e-15)
        assert th[2, 2] == jm.ejections["3"]["half_life"] and R.ejections["3"]["e_half_life"] == 0.0
        assert set(R.ejections["1"]) == {"t_0", "peak_jml", "half_life", "which", "e_t_0", "e_peak_jml", "e_half_life"}
        assert R.cov.shape == (5, 5)


def test_fit_ejections_vis_on_a_recording_engine(tmp_path):
    rec = _Recorder([100.0 / (1 + i) for i in range(40)], chunks=2)
    jm = tilted_model(tmp_path, rec)
    times, freq, Kv = np.array([0.5, 1.0, 1.5, 2.0]) * YEAR, [5e9, 1.5e9], 7
    jm.VIS_STACK_BYTES = 2 * (2 * 9) * 6 * 8              # two epochs of derivative maps per chunk
    vis = torch.ones(4, 2, Kv, dtype=torch.complex128).as_subclass(_NoHost)
    u = np.linspace(10.0, 70.0, Kv)
    R = jm.fit_ejections_vis(times, u, -u, freq, vis, weights=np.full(Kv, 2.0), tie=RB_TIE, n_iter=3,
                             xtol=1e-300, trace=True)
    assert R.status == 0 and R.niter == 3 and R.ndata == 2 * (5 + 5)
    kinds = [c["kind"] for c in rec.calls]
    jac_chunk = ["ff_formal_sweep", "vis", "ff_formal_grad", "vis", "normal_eq"]
    trial_chunk = ["ff_formal_sweep", "vis", "normal_eq"]
    # The model visibilities of a chunk are kept under the key of the kernel parameters: an accepted trial's
    # derivative evaluation reuses its own V.  The recorder's steps are below an ulp of every parameter, so
    # here the key never changes after the start and every later evaluation finds its V (the device tests,
    # whose parameters move, recover the truth through the same code).
    again_chunk = ["ff_formal_grad", "vis", "normal_eq"]
    assert kinds == 2 * jac_chunk + 2 * (2 * ["normal_eq"] + 2 * again_chunk)  # one normal_eq per chunk
    assert trial_chunk[-1] == "normal_eq"
    assert all(c["E"] == 2 and c["maps"] for c in rec.calls if c["kind"] in ("ff_formal_sweep", "ff_formal_grad"))
    ne = [c for c in rec.calls if c["kind"] == "normal_eq"]
    assert all(c["rows"] == 4 and c["n_vis"] == Kv and c["complex_"] and c["w"].numel() == Kv for c in ne)
    assert ne[0]["dshape"] == (4, 9, Kv) and ne[0]["sel"].tolist() == list(range(9)) and ne[2]["dshape"] is None
    assert ne[2]["sel"].size == 0                                   # a trial requests no derivative maps
    vs = [c for c in rec.calls if c["kind"] == "vis"]
    assert [c["M"] for c in vs[:4]] == [4, 36, 4, 36] and all(c["K"] == Kv for c in vs)
    su = classes.vis_scales(np.array(freq), jm.csize, jm.params["target"]["dist"])[0]
    assert np.array_equal(vs[0]["su"], np.tile(su, 2)) and np.array_equal(vs[1]["su"], np.tile(np.repeat(su, 9), 2))
    N_fit, g_fit, _ = expected_fit_space(jm, rec, list(range(9)))
    assert np.allclose(R.trace[0]["N"], N_fit, rtol=1e-13, atol=0) and np.allclose(R.trace[0]["g"], g_fit, rtol=1e-13)
    assert R.trace[0]["chi2"] == 100.0
    # a coverage per epoch: one vis call per epoch (and per kind of map), still one normal_eq per chunk
    rec.calls.clear()
    uu = np.stack([u + e for e in range(4)])
    w = np.ones((4, Kv))
    w[1, 3:] = 0.0
    jm.fit_ejections_vis(times, uu, -uu, freq, vis, weights=w, tie=RB_TIE, n_iter=1)
    kinds = [c["kind"] for c in rec.calls]
    assert kinds == 2 * ["ff_formal_sweep", "vis", "vis", "ff_formal_grad", "vis", "vis", "normal_eq"]
    vs = [c for c in rec.calls if c["kind"] == "vis"]
    assert [float(c["u"][0]) for c in vs] == [10.0, 11.0, 10.0, 11.0, 12.0, 13.0, 12.0, 13.0]
    assert [c["M"] for c in vs[:4]] == [2, 2, 18, 18]
    ne = [c for c in rec.calls if c["kind"] == "normal_eq"]
    assert ne[0]["w"].numel() == 4 * Kv and ne[0]["w"].reshape(2, 2, Kv)[1, :, 3:].sum() == 0
    # refusals
    with pytest.raises(ValueError):
        jm.fit_ejections_vis(times, u, -u[:3], freq, vis)
    jm32 = tilted_model(tmp_path, rec)
    jm32._dtype = _lib.RJP_F32
    for call in (lambda: jm32.fit_ejections_vis(times, u, -u, freq, vis),
                 lambda: jm32.fit_ejections_flux(times, freq, np.ones((4, 2))),
                 lambda: jm32.fit_ejections_flux(times, freq, np.ones((4, 2)), formal=True)):
        with pytest.raises(ValueError, match="f64 storage"):
            call()
    none = tilted_model(tmp_path, rec)
    none._ejections, none._bursts = {}, {"R": [], "B": []}
    with pytest.raises(ValueError, match="no ejections"):
        none.fit_ejections_flux(times, freq, np.ones((4, 2)))


def test_an_infeasible_start_and_update(tmp_path):
    rec = _Recorder(SCRIPT)
    jm = tilted_model(tmp_path, rec)
    times, freq = np.array([0.5, 1.0]) * YEAR, [5e9]
    R = jm.fit_ejections_flux(times, freq, np.ones((2, 1)), theta0={"3": {"half_life": -1.0}}, update=True)
    assert R.status == 3 and R.ejections is None and R.cov is None and rec.calls == [] and np.isnan(R.chi2)
    # update=True writes the result back through set_ejection_event
    v0 = jm._version
    R = jm.fit_ejections_flux(times, freq, np.ones((2, 1)), tie=RB_TIE, free=np.arange(9).reshape(3, 3) != 8,
                              n_iter=2, xtol=1e-300, update=True)
    assert R.status == 0 and jm._version > v0
    for i, k in enumerate(jm.ejections):
        assert [jm.ejections[k][n] for n in inference.PARAM_NAMES] == R.theta[i].tolist()
    # too few data for the free parameters: status 3 (5 counting samples, 6 fit parameters)
    rec = _Recorder(SCRIPT)
    jm = tilted_model(tmp_path, rec)
    R = jm.fit_ejections_flux(times, freq, np.ones((2, 1)), tie=RB_TIE, n_iter=2, xtol=1e-300)
    assert R.status == 3 and R.ejections is None
    with pytest.raises(ValueError):
        jm.fit_ejections_flux(times, freq, np.ones((2, 1)), tie=[[("1", "t_0"), ("2", "t_0")], [("2", "t_0"), ("3", "t_0")]])
    with pytest.raises(ValueError):
        jm.fit_ejections_flux(times, freq, np.ones((3, 1)))


def test_layout_free_and_tie(tmp_path):
    """A `free` dict restricts the ejections it names and leaves the others free; a tie keeps the start's ratio."""
    bf = inference.BurstFit(tilted_model(tmp_path, None))
    lay = bf.layout({"3": ["t_0", "peak_jml"], "1": []}, None, None)
    assert lay["free_phys"].reshape(3, 3).tolist() == [[False] * 3, [True] * 3, [True, True, False]]
    assert bf.layout({"2": "half_life"}, None, None)["free_phys"].reshape(3, 3)[1].tolist() == [False, False, True]
    assert bf.layout(None, None, None)["free_phys"].all() and bf.layout({}, None, None)["free_phys"].all()
    mask = np.arange(9).reshape(3, 3) % 2 == 0
    assert np.array_equal(bf.layout(mask, None, None)["free_phys"].reshape(3, 3), mask)
    lay = bf.layout({"1": ["t_0", "peak_jml"]}, RB_TIE, None)              # a group is free iff all members are
    assert lay["free_fit"].tolist() == [True, True, False, True, True, True] and lay["T"].shape == (9, 6)
    p0 = lay["phys0"]
    assert lay["ratio"].tolist() == [1, 1, 1, 1, p0[1, 1] / p0[0, 1], 1, 1, 1, 1]
    assert np.array_equal(bf.physical(lay, lay["theta0"]), p0)
    with pytest.raises(ValueError):
        bf.layout(None, [[("1", "t_0")]], None)
    with pytest.raises(ValueError):
        bf.layout({"4": ["t_0"]}, None, None)


def test_set_ejection_event_against_add_ejection_event(tmp_path):
    """Changing an event in place leaves the model as if it had been built with the new values."""
    a = tilted_model(tmp_path, None)
    b = tilted_model(tmp_path, None)
    b._ejections, b._bursts = {}, {"R": [], "B": []}
    new = {"1": (0.31 * YEAR, 2.1e15, 0.22 * YEAR), "2": None, "3": (0.7 * YEAR, 3.1e15, 0.33 * YEAR)}
    for k, ej in a.ejections.items():
        t0, pk, hl = new[k] or (ej["t_0"], ej["peak_jml"], ej["half_life"])
        b.add_ejection_event(t0, pk, hl, ej["which"])
    a._scan_cache["x"], a._tavg, v0 = 1, 2, a._version
    a.set_ejection_event("1", *new["1"])
    assert a._version == v0 + 1 and not a._scan_cache and a._tavg is None          # what add_ejection_event invalidates
    a.set_ejection_event(3, t_0=new["3"][0])
    a.set_ejection_event("3", peak_jml=new["3"][1], half_life=new["3"][2])
    assert a.ejections == b.ejections and a._bursts == b._bursts
    assert list(a.ejections) == ["1", "2", "3"]
    with pytest.raises(KeyError):
        a.set_ejection_event("4", t_0=1.0)


def test_public_surface_new_names_only():
    J, sig = classes.JetModel, lambda f: list(inspect.signature(f).parameters)
    common = ["free", "tie", "theta0", "n_iter", "lambda0", "xtol", "update", "trace"]
    assert sig(J.fit_ejections_flux) == ["self", "times_s", "freq", "flux", "sigma", "formal"] + common
    assert sig(J.fit_ejections_vis) == ["self", "times_s", "u_m", "v_m", "freq", "vis", "weights"] + common
    p = inspect.signature(J.fit_ejections_vis).parameters
    assert [p[k].default for k in common] == [None, None, None, 30, 1e-3, 1e-8, False, False]
    assert sig(J.set_ejection_event) == ["self", "key", "t_0", "peak_jml", "half_life"]
    assert sig(E.RTEngine.normal_eq) == ["self", "data", "model", "dmodel", "sel", "weights"]
    assert sig(E.lm_minimise) == ["evaluate", "theta0", "free", "feasible", "scales", "n_iter", "lambda0", "xtol",
                                  "trace"]
    assert classes.EjectionFit._fields == ("ejections", "theta", "cov", "chi2", "reduced_chi2", "ndata", "status",
                                           "niter", "trace")
    for name in ("flux_vs_time_jac", "visibilities_vs_time_jac", "flux_vs_time", "add_ejection_event"):
        assert "BurstFit" not in inspect.getsource(getattr(J, name))
    assert "fit_ejections" not in inspect.getsource(classes.Pipeline.execute)
