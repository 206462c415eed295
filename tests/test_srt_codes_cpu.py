"""Launch-time codes of the packed state (srt_codes_kernel in ff_lt.hip, the residual stream of
ff_scan_hybrid_kernel in ff_scan_tab.hip), restated in NumPy next to tests/test_srt_residual_cpu.py.

With the codes a table-residual bin streams 6 bytes per cell: a 32-bit code of the launch time and
the 16-bit weight.  The code is c = min(floor((ts - ts_lo) S), 2^32 - 1), S = 2^32 / (ts_hi - ts_lo);
the scan takes w_q = A - c B for the lookup's w = (t - ts - lo) inv_h, with q = (ts_hi - ts_lo) 2^-32,
B = q inv_h, A = (t - ts_lo - lo) inv_h - B / 2 (the middle of the code's interval), and calls a cell
AMBIGUOUS when f = w_q - floor(w_q) has |f - 1/2| > 1/2 - mg, mg = 2 B + rho, rho = 2^-48 Tm inv_h,
Tm = |t| + max(|ts_lo|, |ts_hi|) + |lo|, or when its code is saturated.  An ambiguous cell is re-read
from the layout's cells and evaluated exactly.  The derivation (ff_scan_tab.hip, "the margin"):
the code stands for launch times within (1/2 + 2^-18) q of the middle, both evaluations together
round by <= 10 x 2^-53 Tm inv_h < rho, so |w - w_q| < mg and a cell that is not ambiguous has
floor(w) = floor(w_q): the same table piece after the same clamp.  xi = 2 (w - floor w) - 1 then
moves by 2 |w - w_q| <= (1 + 2^-17) B + 2 rho, plus one f32 rounding (<= 2^-25) on either side.

The device evaluates w_q with one fused multiply-add; NumPy rounds c B first, one more unit of
2^-53 Tm inv_h against the 32 that rho grants, so every bound here holds for both.

No GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import gpu_util as U
from tests import test_srt_residual_cpu as R
from tests import test_srt_truncation_cpu as S

YEAR = S.YEAR
SAT = 2 ** 32 - 1
N_UNIFORM = 4_000_000


# ---- the restatement ---------------------------------------------------------------------------
def encode(ts, ts_range):
    """srt_codes_kernel: f64 as written, then the clamp and the conversion."""
    lo_t, hi_t = ts_range
    span = hi_t - lo_t
    scale = 4294967296.0 / span if span > 0.0 else 0.0
    v = np.floor((np.asarray(ts, dtype=np.float64) - lo_t) * scale)
    return np.minimum(np.maximum(v, 0.0), 4294967295.0).astype(np.uint64)


def code_params(t, ts_range, lo, inv_h):
    """The host side of the scan: (A, B, mg, rho, q)."""
    lo_t, hi_t = ts_range
    q = np.ldexp(hi_t - lo_t, -32)
    B = q * inv_h
    A = (t - lo_t - lo) * inv_h - 0.5 * B
    Tm = abs(t) + max(abs(lo_t), abs(hi_t)) + abs(lo)
    rho = np.ldexp(Tm * inv_h, -48)
    return A, B, 2.0 * B + rho, rho, q


def coded_lookup(c, A, B, mg, ni):
    """-> (piece, xi in f32, ambiguous) from the code, as the residual stream takes them."""
    hm = 0.5 - mg if mg < 0.5 else -1.0
    wv = A - c.astype(np.float64) * B
    f = wv - np.floor(wv)
    amb = (np.abs(f - 0.5) > hm) | (c == SAT)
    w = np.minimum(np.maximum(wv, 0.0), np.nextafter(float(ni), 0.0))
    kf = np.floor(w)
    return kf.astype(np.int64), (2.0 * (w - kf) - 1.0).astype(np.float32), amb


def exact_lookup(ts, t, lo, inv_h, ni):
    """-> (piece, xi in f32) of the 10-byte path (R.err_eval's own index arithmetic)."""
    w = np.minimum(np.maximum((t - ts - lo) * inv_h, 0.0), np.nextafter(float(ni), 0.0))
    kf = np.floor(w)
    return kf.astype(np.int64), (2.0 * (w - kf) - 1.0).astype(np.float32)


def fallback_share(t, ts_range, lo, inv_h):
    """Expected share of launch times spread evenly over the range that fall back: 2 mg of every
    unit of w (the test runs on the unclamped w_q), plus the saturated code's 2^-32."""
    return 2.0 * code_params(t, ts_range, lo, inv_h)[2] + 2.0 ** -32


def launch_times(t, ts_range, ni, lo, inv_h, rng, n_uniform=N_UNIFORM):
    """(uniform draw, adversarial points): every piece boundary inside the range with its f64
    neighbours and +-q/2, +-q, +-3q/2, +-2q, +-5q/2 beside it (the margin is 2 q: both of its edges
    are probed), the ends of the range with their neighbours, and times whose w clamps at either
    end of the table."""
    lo_t, hi_t = ts_range
    q = np.ldexp(hi_t - lo_t, -32)
    uni = rng.uniform(lo_t, hi_t, n_uniform)
    tb = t - lo - np.arange(-2, ni + 3) / inv_h                  # w = k, two pieces past either end
    pts = [tb, np.nextafter(tb, -np.inf), np.nextafter(tb, np.inf)]
    for m in (0.5, 1.0, 1.5, 2.0, 2.5):
        pts += [tb - m * q, tb + m * q]
    ends = np.array([lo_t, hi_t])
    pts += [ends, np.nextafter(ends, np.inf)[:1], np.nextafter(ends, -np.inf)[1:],
            lo_t + q * np.array([0.5, 1.0, 1.5]), hi_t - q * np.array([0.5, 1.0, 1.5])]
    pts += [t - lo + np.array([0.5, 1.0, 10.0]) / inv_h,         # w < 0
            t - lo - (ni + np.array([0.5, 1.0, 10.0])) / inv_h]  # w > ni
    adv = np.concatenate(pts)
    return uni, adv[(adv >= lo_t) & (adv <= hi_t)]


def narrow_bursts(ts_range, t):
    """The example's bursts with a weak narrow one in both jets, as narrow as the 320 pieces that
    chi table + error table may take allow (tests/test_gpu_srt_residual.py uses 0.35: too many)."""
    ex = U.example_burst_lists()
    sg = min(s for lst in ex for _, _, s in lst)
    for f in np.arange(0.60, 0.35, -0.005):
        bursts = tuple(list(lst) + [(0.5 * YEAR, 0.5, f * sg)] for lst in ex)
        ni = S.chi_table(bursts, ts_range, t)[0]
        if 300 <= ni <= 320:
            return bursts
        assert ni < 300, (f, ni)
    raise AssertionError("no width gives 300 .. 320 pieces")


CASES = {
    "example 0.3 yr": (U.example_burst_lists, S.TS_RANGE, 0.3),
    "example 1.0 yr": (U.example_burst_lists, S.TS_RANGE, 1.0),
    "example 1.7 yr": (U.example_burst_lists, S.TS_RANGE, 1.7),
    "example 2.2 yr": (U.example_burst_lists, S.TS_RANGE, 2.2),
    "narrow 1.0 yr": (None, S.TS_RANGE, 1.0),
    "range 0.7 .. 4.1 yr, 1.6 yr": (U.example_burst_lists, (0.7 * YEAR, 4.1 * YEAR), 1.6),
}


# ---- tests ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_codes_decide_the_piece_or_fall_back(case):
    make, ts_range, years = CASES[case]
    t = years * YEAR
    bursts = make() if make else narrow_bursts(ts_range, t)
    ni, lo, inv_h, tabs, errs = R.err_table(bursts, ts_range, t)
    if make is None:
        assert 300 <= ni <= 320, ni
    A, B, mg, rho, q = code_params(t, ts_range, lo, inv_h)
    rng = np.random.default_rng(20261021)
    uni, adv = launch_times(t, ts_range, ni, lo, inv_h, rng)
    dxi_bound = (1.0 + 2.0 ** -17) * B + 2.0 * rho + 2.0 ** -24
    worst = 0.0
    for name, ts in (("uniform", uni), ("adversarial", adv)):
        c = encode(ts, ts_range)
        kq, xq, amb = coded_lookup(c, A, B, mg, ni)
        ke, xe = exact_lookup(ts, t, lo, inv_h, ni)
        ok = ~amb
        # outside the fallback the piece is the exact lookup's, for every input
        assert np.array_equal(kq[ok], ke[ok]), (case, name, ts[ok][kq[ok] != ke[ok]][:5])
        dxi = np.abs(xq[ok].astype(np.float64) - xe[ok].astype(np.float64))
        if dxi.size:
            worst = max(worst, float(dxi.max()))
            assert dxi.max() <= dxi_bound, (case, name, dxi.max(), dxi_bound)
        # and the fallback does fire beside a boundary: an exact w within 1.4 B of an integer puts
        # w_q within (1.4 + 1/2 + 2^-18) B + rho < mg of it
        wu = (t - ts - lo) * inv_h
        near = np.abs(wu - np.rint(wu)) <= 1.4 * B
        assert amb[near].all(), (case, name)
        if name == "adversarial":
            assert near.sum() >= 7 * min(ni, 10), (case, int(near.sum()))
        print("%s, %s: %d of %d fall back (%.3g)" % (case, name, int(amb.sum()), ts.size,
                                                      amb.mean()))
        if name == "uniform":
            share = fallback_share(t, ts_range, lo, inv_h)
            assert amb.mean() <= 10.0 * share, (case, amb.mean(), share)
            print("%s: derived share %.3g, pieces %d, B %.3g, mg %.3g" % (case, share, ni, B, mg))
    # Markov: |E~'| <= 8^2 max |E~| on a piece, so E~ moves by <= 64 max |E~| |d xi|; relative to F
    xs = np.linspace(-1.0, 1.0, 257)
    rel = 0.0
    for lst, tab, err in zip(bursts, tabs, errs):
        e = np.polynomial.polynomial.polyval(xs, err.astype(np.float64).T)       # [ni, 257]
        d = lo + (np.arange(ni)[:, None] + 0.5 * (xs[None, :] + 1.0)) / inv_h
        F = U.chi_exact(lst, d) ** 2
        rel = max(rel, float((np.abs(e).max(axis=1) / F.min(axis=1)).max()))
    moved = 64.0 * rel * dxi_bound
    print("%s: worst |d xi| %.3g (<= %.3g), max |E~| / F %.3g, E~ moves by <= %.3g F"
          % (case, worst, dxi_bound, rel, moved))
    assert moved < 1e-17, (case, rel, dxi_bound)


@pytest.mark.parametrize("ts_range", [S.TS_RANGE, (0.7 * YEAR, 4.1 * YEAR), (-3.0e7, 1.0e6)])
def test_the_code_is_monotone_and_saturates(ts_range):
    lo_t, hi_t = ts_range
    q = np.ldexp(hi_t - lo_t, -32)
    rng = np.random.default_rng(7)
    ts = np.sort(np.concatenate([rng.uniform(lo_t, hi_t, 1_000_000), [lo_t, hi_t],
                                 lo_t + q * np.arange(0.0, 8.0, 0.25),
                                 hi_t - q * np.arange(0.0, 8.0, 0.25)]))
    c = encode(ts, ts_range)
    assert np.all(np.diff(c.astype(np.int64)) >= 0)
    assert c[0] == 0 and encode([lo_t], ts_range)[0] == 0
    assert encode([hi_t], ts_range)[0] == SAT
    assert np.all(encode(hi_t + q * np.array([1.0, 1e3, 1e12]), ts_range) == SAT)
    assert np.all(encode(lo_t - q * np.array([1.0, 1e3, 1e12]), ts_range) == 0)
    # the decoding interval: c - 2^-18 <= u < c + 1 + 2^-18 below the saturated code
    u = (ts.astype(np.longdouble) - np.longdouble(lo_t)) / np.longdouble(q)
    below = c < SAT
    cl = c.astype(np.longdouble)
    assert np.all(u[below] >= cl[below] - 2.0 ** -18) and np.all(u[below] < cl[below] + 1 + 2.0 ** -18)
    assert np.all(u[~below] >= SAT - 2.0 ** -18)
    # a saturated code never decides a cell
    assert coded_lookup(np.array([SAT], dtype=np.uint64), 10.5, 1e-8, 1e-7, 100)[2][0]
    # an empty range: every cell codes 0
    assert np.all(encode([lo_t, lo_t], (lo_t, lo_t)) == 0)


def test_a_margin_of_half_or_more_sends_every_cell_back():
    c = np.arange(0, 1000, dtype=np.uint64)
    assert coded_lookup(c, 17.3, 1e-3, 0.5, 40)[2].all()
    assert coded_lookup(c, 17.3, 1e-3, 0.75, 40)[2].all()


# ---- the argument check of rjp_srt_codes from plain C++ ------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESSAGES = {
    "fields": "fields is NULL",
    "storage": "launch-time-bucketed layout: needs RJP_F64 fields with d_a0 and d_ts",
    "dims": "launch-time-bucketed layout: grid dimensions must be positive",
    "K": "launch-time-bucketed layout: 1 <= K <= 32",
    "range": "launch-time-bucketed layout: fields.ts_lo / ts_hi (rjp_field_range) required",
    "null": "rjp_srt_codes: NULL argument",
    "align": "rjp_srt_codes: d_cells and d_pc must be 16-byte aligned",
}


def test_check_srt_codes_from_plain_cpp(tmp_path):
    """check_srt_codes compiled into a stand-alone program by plain g++
    (tests/rjp_args_srt_codes_cases.cpp): every refusal, status and message, in the order the check
    refuses; the messages are the ones tests/test_gpu_srt_codes.py pins on the library."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "rjp_args_srt_codes_cases"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rajepy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rjp_args_srt_codes_cases.cpp"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        case, status, msg = line.split("\t")
        got[case] = (int(status), msg)
    want = {"fields": ["NULL fields", "fields beat K"],
            "storage": ["f32", "no a0", "no ts", "storage beats dimensions"],
            "dims": ["n_y 0", "dimensions beat K"],
            "K": ["K 0", "K 33", "K beats the range"],
            "range": ["no range", "range nan", "range inf", "range reversed", "the range beats NULL"],
            "null": ["NULL d_start", "NULL d_rowbase", "NULL d_cells", "NULL d_pc",
                     "NULL beats alignment"],
            "align": ["d_pc + 4", "d_pc + 8", "d_cells + 8"]}
    seen = set()
    for key, cases in want.items():
        for case in cases:
            assert got[case] == (-1, MESSAGES[key]), case
            seen.add(case)
    valid = {c for c in got if c.startswith("valid")}
    assert len(valid) == 5 and all(got[c] == (0, "") for c in valid)
    assert seen | valid == set(got)
