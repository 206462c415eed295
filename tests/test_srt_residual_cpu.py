"""Table-residual bins of the hybrid single-epoch scan (ff_scan_tab.hip, ff_lt.hip), restated in
NumPy next to tests/test_srt_truncation_cpu.py.

A launch-time bin whose Chebyshev interpolant p matches the exact chi^2 (check (a)) but not the LDS
table's chi^2 (check (b)) differs from the table by the table's own interpolation error
E_i(xi) = T_i(xi)^2 - F, a smooth function of the piece i and the piece coordinate xi alone.
srt_err_kernel fits E per piece by a polynomial of degree 8 from 12 Chebyshev nodes (f64), stores
the 9 monomial coefficients in f32, and srt_coef_kernel accepts such a bin as a RESIDUAL bin when
(b') |p + E~ - T^2| <= kSrtMomTol T^2 holds at the same 4 N points, E~ evaluated by the scan's f32
Horner chain at the scan's own (piece, xi).  The scan then sums
    sum |a0| T^2 = sum_n W_n M_n + sum_cells |a0| E~(ts)
and the second term -- at most ~2.2e-13 of the bin's sum -- needs |a0| to 2^-9 only: the packed
state keeps the launch time (8 B) and a 16-bit weight (8 exponent and 8 mantissa bits: a weight is
never negative, so the sign bit of bfloat16 goes to the mantissa), 10 bytes per cell instead of 16.

No GPU: everything here is NumPy; the exact chi^2 of check (a) is evaluated in long double."""
import numpy as np
import pytest

from tests import gpu_util as U
from tests import test_srt_truncation_cpu as S

YEAR, TOL, TAIL_FRAC, K, N, TS_RANGE = S.YEAR, S.TOL, S.TAIL_FRAC, S.K, S.N, S.TS_RANGE
ERR_NODES, ERR_DEG = 12, 8                 # kErrNodes, kErrNC - 1
W_RELERR = 2.0 ** -9                       # the packed weight's rounding
F32_MIN_NORMAL = 2.0 ** -126
# row n: the monomial coefficients of T_n (kErrCheb in ff_scan_tab.hip)
CHEB_TO_MONOMIAL = np.array([np.pad(np.polynomial.chebyshev.cheb2poly([0.0] * n + [1.0]),
                                    (0, ERR_DEG - n)) for n in range(ERR_DEG + 1)])


# ---- the per-call error table (srt_err_kernel) -------------------------------------------------
def err_table(bursts, ts_range, t):
    """Per jet [ni, 9] f32 monomial coefficients of E_i(xi) = T_i(xi)^2 - F on every table piece."""
    ni, lo, inv_h, tabs = S.chi_table(bursts, ts_range, t)
    m = np.arange(ERR_NODES)
    xs = np.cos(np.pi * (m + 0.5) / ERR_NODES)
    Tn = np.cos(np.pi * np.outer(np.arange(ERR_DEG + 1), 2 * m + 1) / (2 * ERR_NODES))  # [n, m]
    out = []
    for lst, tab in zip(bursts, tabs):
        tl = lo + (np.arange(ni)[:, None] + 0.5 * (xs[None, :] + 1.0)) / inv_h
        F = U.chi_exact(lst, tl) ** 2
        v = np.repeat(tab[:, 7:8], ERR_NODES, axis=1)
        for n in range(6, -1, -1):
            v = v * xs[None, :] + tab[:, n:n + 1]
        c = (2.0 / ERR_NODES) * ((v * v - F) @ Tn.T)          # Chebyshev coefficients, [ni, 9]
        c[:, 0] *= 0.5
        out.append((c @ CHEB_TO_MONOMIAL).astype(np.float32))
    return ni, lo, inv_h, tabs, out


def err_eval(err, ni, lo, inv_h, d):
    """E~ at the time since launch d, as the scan evaluates it: the lookup's piece and xi in f64,
    xi rounded to f32, Horner in f32."""
    w = np.minimum(np.maximum((d - lo) * inv_h, 0.0), np.nextafter(float(ni), 0.0))
    kf = np.floor(w)
    xi = (2.0 * (w - kf) - 1.0).astype(np.float32)
    c = err[kf.astype(int)]
    v = c[:, ERR_DEG].copy()
    for n in range(ERR_DEG - 1, -1, -1):
        v = (v * xi + c[:, n]).astype(np.float32)
    return v.astype(np.float64)


def verdicts(bursts, t, K=K, N=N, ts_range=TS_RANGE):
    """Per jet {bin: (kind, m, err)} over the bins of the support: kind 'b' = accepted by (a) and
    (b) as before, 'res' = passes (a), fails (b), passes (b'), 'read' = neither; m by the device's
    count rule with (b') in place of (b) on a residual bin; err = the realised (b) / (b') error of
    the m coefficients."""
    ni, lo, inv_h, tabs, errs = err_table(bursts, ts_range, t)
    plan = U.srt_plan_host([0] * (2 * K), ts_range, K, bursts, t)
    lo_t, hi_t = ts_range
    h = (hi_t - lo_t) / K
    nodes = np.cos(np.pi * (np.arange(N) + 0.5) / N)
    Tm = np.polynomial.chebyshev.chebvander(nodes, N - 1)
    x = -1.0 + 2.0 * np.arange(4 * N) / (4 * N - 1)
    out = []
    for j in range(2):
        res = {}
        for b in range(plan["b0"][j], plan["b1"][j]):
            ts_of = lambda xx: lo_t + (b + 0.5 * (xx + 1.0)) * h
            W = (2.0 / N) * (Tm.T @ U.chi_exact(bursts[j], t - ts_of(nodes)) ** 2)
            W[0] *= 0.5
            F = (S.chi_exact_ld(bursts[j], t - ts_of(x).astype(np.longdouble)) ** 2).astype(np.float64)
            T = S.table_chi(tabs[j], ni, lo, inv_h, t - ts_of(x)) ** 2
            Et = err_eval(errs[j], ni, lo, inv_h, t - ts_of(x))

            def check(m, resid):
                p = np.polynomial.chebyshev.chebval(x, W[:m])
                ea = np.max(np.abs(p - F) / F)
                eb = np.max(np.abs(p + (Et if resid else 0.0) - T) / T)
                return ea, eb
            ea, eb = check(N, False)
            if ea > TOL:
                res[b] = ("read", 0, ea)
                continue
            resid = eb > TOL
            if resid and check(N, True)[1] > TOL:
                res[b] = ("read", 0, check(N, True)[1])
                continue
            lim = TAIL_FRAC * TOL * F.min()
            m, tail = N, 0.0
            while m > 1 and tail + abs(W[m - 1]) <= lim:
                tail += abs(W[m - 1])
                m -= 1
            if m < N and max(check(m, resid)) > TOL:
                m = N
            res[b] = ("res" if resid else "b", m, check(m, resid)[1])
        out.append(res)
    return out


# ---- the packed weight (srt_pack_kernel) ---------------------------------------------------------
def pack_weight(w):
    """(16-bit code, out-of-range flag) of non-negative f64 weights: 8 exponent bits (f32's bias) and
    8 mantissa bits, round to nearest even straight from the f64 bits; a finite non-zero weight
    whose code would leave the normal range raises the flag (and is stored as zero)."""
    b = np.asarray(w, dtype=np.float64).view(np.uint64)
    r = b + np.uint64((1 << 43) - 1) + ((b >> np.uint64(44)) & np.uint64(1))
    top = (r >> np.uint64(44)).astype(np.int64)
    e = (top >> 8) - 896
    man = top & 255
    ok = (e >= 1) & (e <= 254)
    code = np.where(ok, (e << 8) | man, 0).astype(np.uint16)
    flag = ~ok & (b != 0)
    return code, flag


def unpack_weight(code):
    return (code.astype(np.uint32) << np.uint32(15)).view(np.float32).astype(np.float64)


# ---- tests -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("years", [0.3, 1.0, 1.7, 2.2])
def test_every_bin_rejected_by_b_alone_passes_b_prime(years):
    bursts = U.example_burst_lists()
    res = verdicts(bursts, years * YEAR)
    old = S.coefficient_counts(bursts, years * YEAR)
    worst = 0.0
    for j in range(2):
        kinds = [k for k, _, _ in res[j].values()]
        # rule (a) accepts every support bin of the example, so nothing is left to the cells
        assert "read" not in kinds, (years, j, res[j])
        n_b = kinds.count("b")
        # (b) itself is untouched: the same bins, with the same counts, as the truncation module's
        assert n_b == len(old[j][1]), (years, j)
        if years in S.EXAMPLE:
            assert n_b == S.EXAMPLE[years][0][j]
        assert {r[0]: r[1] for r in old[j][1]} == {b: m for b, (k, m, _) in res[j].items() if k == "b"}
        for b, (k, m, e) in res[j].items():
            assert e <= TOL, (years, j, b, k, m, e)
            if k == "res":
                worst = max(worst, e)
        print("%.1f yr, jet %d: %d by (b), %d residual, m of the residual bins %s"
              % (years, j, n_b, kinds.count("res"), [m for k, m, _ in res[j].values() if k == "res"]))
    assert any(k == "res" for j in range(2) for k, _, _ in res[j].values())
    print("%.1f yr: worst (b') error of a residual bin %.2e (kSrtMomTol %.0e)" % (years, worst, TOL))


def test_a_burst_too_narrow_for_a_is_not_made_residual():
    h = (TS_RANGE[1] - TS_RANGE[0]) / K
    bursts = [(0.5 * YEAR, 4.0, 0.12 * h)], [(0.5 * YEAR, 2.0, 0.12 * h)]
    res = verdicts(bursts, 1.0 * YEAR)
    failed_a = 0
    for j in range(2):
        for b, (k, m, e) in res[j].items():
            ts_of = lambda xx: TS_RANGE[0] + (b + 0.5 * (xx + 1.0)) * h
            ok_a = U.srt_bin_passes(bursts[j], TS_RANGE, K, N, b, 1.0 * YEAR, TOL)
            if not ok_a:
                failed_a += 1
                assert k == "read", (j, b, k)
    assert failed_a > 0


def test_packed_weight_rounds_to_two_to_the_minus_nine():
    rng = np.random.default_rng(5)
    w = np.concatenate([10.0 ** rng.uniform(-37.9, 38.4, 200000),
                        np.ldexp(1.0 + rng.integers(0, 512, 4096) / 512.0, rng.integers(-126, 127, 4096)),
                        [1.0, 1.0 + 2.0 ** -9, 1.0 + 3 * 2.0 ** -9, 2.0 - 2.0 ** -10, F32_MIN_NORMAL]])
    code, flag = pack_weight(w)
    assert not flag.any()
    back = unpack_weight(code)
    assert np.max(np.abs(back - w) / w) <= W_RELERR
    # ties go to the even mantissa, and a carry moves into the exponent
    assert unpack_weight(pack_weight(np.array([1.0 + 2.0 ** -9]))[0])[0] == 1.0
    assert unpack_weight(pack_weight(np.array([1.0 + 3 * 2.0 ** -9]))[0])[0] == 1.0 + 2.0 ** -7
    assert unpack_weight(pack_weight(np.array([2.0 - 2.0 ** -10]))[0])[0] == 2.0
    assert pack_weight(np.array([0.0]))[0][0] == 0 and not pack_weight(np.array([0.0]))[1][0]


def test_range_flag_fires_just_outside_the_normal_f32_range_only():
    inside = np.array([F32_MIN_NORMAL, 1.2e-38, 1.0, 3.0e38, np.ldexp(2.0 - 2.0 ** -8, 127)])
    outside = np.array([1.17e-38, 1.0e-38, 5e-324, 3.5e38, 1e39, 1e300])
    assert not pack_weight(inside)[1].any()
    assert pack_weight(outside)[1].all()
    assert (pack_weight(outside)[0] == 0).all()
