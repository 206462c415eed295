"""The coefficient-count rule of srt_coef_kernel (ff_scan_tab.hip), restated in NumPy: a launch-time
bin whose degree-(N - 1) Chebyshev interpolant of chi^2 passes checks (a) (against the exact chi^2)
and (b) (against the LDS table's chi^2) at kSrtMomTol keeps the first m coefficients, m the smallest
count whose dropped tail sum_{n >= m} |W_n| is <= kSrtTailFrac kSrtMomTol F_min; the truncated
interpolant must pass (a) and (b) again, else m = N.  For the reference example's bursts at
0.3 / 1.0 / 1.7 yr (K = 32, N = 20, launch times over [0, 5] yr) every accepted bin's truncated
interpolant passes both checks and obeys the tail bound, and the moment planes read are well below
the N - 1 per bin read without the rule (printed).  A burst just wide enough for its bins to pass
keeps all N coefficients on some of them: the fallback the GPU test then runs.

No GPU: the table (chi_table_plan, chi_table_kernel, the lookup) and the checks are f64 NumPy, the
exact chi^2 of check (a) is evaluated in long double."""
import math

import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U

YEAR = orc.YEAR
TOL = U.SRT_MOM_TOL            # kSrtMomTol
TAIL_FRAC = 0.25               # kSrtTailFrac
K, N = 32, 20
TS_RANGE = (0.0, 5.0 * YEAR)


def chi_table(bursts, ts_range, t):
    """chi_table_plan + chi_table_kernel: (ni, lo, inv_h, [per jet: [ni, 8] monomial coefficients])."""
    lo_t, hi_t = ts_range
    s_lo, s_hi, B = math.inf, -math.inf, 0.0
    for lst in bursts:
        if len(lst):
            a, b = U._support(lst)
            s_lo, s_hi = min(s_lo, a), max(s_hi, b)
        B = max(B, sum(amp * 105.0 / sg ** 8 for _, amp, sg in lst))
    lo, hi = max(s_lo, t - hi_t), min(s_hi, t - lo_t)
    ni = max(1, int(math.ceil((hi - lo) / (2.0 * (U.CHI_TOL * 5160960.0 / B) ** (1.0 / 8.0)))))
    assert ni <= U.CHI_MAX_NI
    inv_h = ni / (hi - lo)
    xs = -np.cos(np.pi * (np.arange(8) + 0.5) / 8)
    vinv = np.linalg.inv(np.vander(xs, 8, increasing=True))
    tabs = []
    for lst in bursts:
        tl = lo + (np.arange(ni)[:, None] + 0.5 * (xs[None, :] + 1.0)) / inv_h
        tabs.append(U.chi_exact(lst, tl) @ vinv.T)
    return ni, lo, inv_h, tabs


def table_chi(tab, ni, lo, inv_h, d):
    """The scans' lookup of chi at the time since launch d."""
    w = np.minimum(np.maximum((d - lo) * inv_h, 0.0), np.nextafter(float(ni), 0.0))
    kf = np.floor(w)
    xi = 2.0 * (w - kf) - 1.0
    c = tab[kf.astype(int)]
    v = c[:, 7]
    for n in range(6, -1, -1):
        v = v * xi + c[:, n]
    return v


def chi_exact_ld(lst, d):
    d = np.asarray(d, dtype=np.longdouble)
    chi = np.ones_like(d)
    for t0, amp, sg in lst:
        chi = chi + np.longdouble(amp) * np.exp(-(d - np.longdouble(t0)) ** 2 /
                                                (2 * np.longdouble(sg) ** 2))
    return chi


def coefficient_counts(bursts, t, K=K, N=N, ts_range=TS_RANGE):
    """Per jet a list of (bin, m, tail, F_min, err_a, err_b) for the bins of the support that pass
    (a) and (b) with all N coefficients, plus the number of bins in the support; m by the device's
    rule, tail = sum_{n >= m} |W_n|, err_a / err_b of the interpolant of m coefficients."""
    ni, lo, inv_h, tabs = chi_table(bursts, ts_range, t)
    plan = U.srt_plan_host([0] * (2 * K), ts_range, K, bursts, t)
    lo_t, hi_t = ts_range
    h = (hi_t - lo_t) / K
    nodes = np.cos(np.pi * (np.arange(N) + 0.5) / N)
    Tm = np.polynomial.chebyshev.chebvander(nodes, N - 1)
    x = -1.0 + 2.0 * np.arange(4 * N) / (4 * N - 1)
    out = []
    for j in range(2):
        rows = []
        for b in range(plan["b0"][j], plan["b1"][j]):
            ts_of = lambda xx: lo_t + (b + 0.5 * (xx + 1.0)) * h
            W = (2.0 / N) * (Tm.T @ U.chi_exact(bursts[j], t - ts_of(nodes)) ** 2)
            W[0] *= 0.5
            F = (chi_exact_ld(bursts[j], t - ts_of(x).astype(np.longdouble)) ** 2).astype(np.float64)
            T = table_chi(tabs[j], ni, lo, inv_h, t - ts_of(x)) ** 2

            def errs(m):
                p = np.polynomial.chebyshev.chebval(x, W[:m])
                return np.max(np.abs(p - F) / F), np.max(np.abs(p - T) / T)
            if max(errs(N)) > TOL:
                continue                                   # read cell by cell, today and afterwards
            lim = TAIL_FRAC * TOL * F.min()
            m, tail = N, 0.0
            while m > 1 and tail + abs(W[m - 1]) <= lim:
                tail += abs(W[m - 1])
                m -= 1
            if m < N and max(errs(m)) > TOL:
                m, tail = N, 0.0
            rows.append((b, m, tail, F.min()) + errs(m))
        out.append((plan["b1"][j] - plan["b0"][j], rows))
    return out


# (accepted bins red / blue, planes read without the rule): the acceptance counts of the device at
# 1.0 yr are the 13 / 18 of DESIGN.md section 3
EXAMPLE = {0.3: ((12, 18), (228, 342)), 1.0: ((13, 18), (247, 342)), 1.7: ((17, 22), (323, 418))}


@pytest.mark.parametrize("years", sorted(EXAMPLE))
def test_truncated_interpolant_passes_and_obeys_the_bound(years):
    bursts = U.example_burst_lists()
    res = coefficient_counts(bursts, years * YEAR)
    accepted, planes_all = EXAMPLE[years]
    for j, (n_support, rows) in enumerate(res):
        assert len(rows) == accepted[j], (years, j, len(rows), n_support)
        assert (N - 1) * len(rows) == planes_all[j]
        for b, m, tail, fmin, ea, eb in rows:
            assert 1 <= m <= N
            assert ea <= TOL and eb <= TOL, (years, j, b, m, ea, eb)
            assert tail <= TAIL_FRAC * TOL * fmin, (years, j, b, m, tail)
        planes = sum(m - 1 for _, m, *_ in rows)
        # the rule is worth having only if it drops a good part of the planes: more than a third
        assert planes < 2 * planes_all[j] / 3, (years, j, planes)
        print("%.1f yr, jet %d: %d of %d bins accepted, moment planes read %d of %d, m = %s"
              % (years, j, len(rows), n_support, planes, planes_all[j], [r[1] for r in rows]))


def just_wide_enough_bursts():
    """One burst per jet whose width is near the narrowest for which bins of the layout pass with
    N = 20 coefficients: on the bins of its flanks the last coefficients are still above the tail
    bound, so nothing can be dropped."""
    h = (TS_RANGE[1] - TS_RANGE[0]) / K
    return [(0.5 * YEAR, 4.0, 0.40 * h)], [(0.5 * YEAR, 2.0, 0.42 * h)]


def test_a_burst_just_wide_enough_keeps_all_coefficients():
    bursts = just_wide_enough_bursts()
    res = coefficient_counts(bursts, 1.0 * YEAR)
    full = 0
    for j, (n_support, rows) in enumerate(res):
        assert len(rows) > 0, j
        for b, m, tail, fmin, ea, eb in rows:
            assert ea <= TOL and eb <= TOL and tail <= TAIL_FRAC * TOL * fmin
        full += sum(1 for r in rows if r[1] == N)
        print("jet %d: %d of %d bins accepted, m = %s" % (j, len(rows), n_support,
                                                          [r[1] for r in rows]))
    assert full > 0
