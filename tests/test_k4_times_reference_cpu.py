"""K4's launch times against tests/golden/k4_times.npz (50 digits, tests/golden/make_k4_times_golden.py),
without a GPU:

  * the fixture belongs to the committed case table (hash) and, where mpmath imports, recomputes;
  * the oracle's own float64 formula (scipy's hyp2f1) deviates from it by a recorded amount per family
    -- the baseline the device bound of tests/test_gpu_k4_reference.py is judged against;
  * `JetModel._host_launch_times`, the fallback of a refused model, holds the bound on the exactly
    degenerate case;
  * a float64 NumPy restatement of the device's evaluation (fields.hip: hyp_series, hyp_flow_factor,
    and its host half hyp_plan, which picks the switch point between the two series and refuses what neither
    can hold) meets the bound on every case it does not refuse, and refuses only what may be refused.

The bound on a launch time is the project's own: |got - ref| <= 1e-10 |ref| + 1e-3 s.
"""
import importlib.util
import json
import math
import os

import numpy as np
import pytest

from oracle import rt_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "k4_times.npz")
RTOL, ATOL = 1e-10, 1e-3

# ---- restatement of fields.hip: hyp_plan (host) and hyp_series / hyp_flow_factor (device) ---------
HYP_MAX_TERMS = 400                    # kHypMaxTerms: no series may need more
HYP_CONN_TERMS = 100                   # kHypConnTerms: ... and the connection series not more than this
HYP_STOP = 1e-17                       # a term below this share of the sum ends a series
HYP_SWITCHES = (1.0, 1.25, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 16.0, 64.0, math.inf)      # kHypSwitch
HYP_MAX_LOSS = 4096.0                  # kHypMaxLoss: digits the connection formula may cancel
HYP_PROBES = (1.0, 1.5, 2.0, 4.0, 16.0)


def _generator():
    spec = importlib.util.spec_from_file_location(
        "make_k4_times_golden", os.path.join(HERE, "golden", "make_k4_times_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()


def load_fixture():
    assert os.path.exists(FIXTURE), "tests/golden/k4_times.npz is missing: run its generator"
    z = np.load(FIXTURE)
    cases = json.loads(str(z["cases"]))
    return z, cases


def hyp_series(a, beta, s):
    """sum_k (a)_k / (beta + 1)_k s^k as the device sums it, on arrays of s: a series ends at the
    first term below HYP_STOP of the sum once the denominators beta + 1 + k are positive and the term
    ratio is below 1 (before that the terms of the connection series fall and rise again: for large b
    and A near 1 they come back to order one around k = (b - a)(1 + 1/A)).
    -> (sum, largest |term| including the leading 1, terms taken; HYP_MAX_TERMS + 1 = did not end)."""
    s = np.asarray(s, dtype=np.float64)
    term, total, big = np.ones_like(s), np.ones_like(s), np.ones_like(s)
    taken = np.full(s.shape, HYP_MAX_TERMS + 1)
    done = np.zeros(s.shape, dtype=bool)
    for k in range(HYP_MAX_TERMS):
        ratio = (a + k) / (beta + 1.0 + k) * s
        new = term * ratio
        term = np.where(done, term, new)
        total = np.where(done, total, total + term)
        big = np.maximum(big, np.abs(term))
        end = ~done & (np.abs(term) <= HYP_STOP * np.abs(total)) & \
            (beta + 1.0 + k > 0.0) & (np.abs(ratio) < 1.0)
        taken[end] = k + 1
        done = done | end
        if done.all():
            break
    return total, big, taken


def _gamma_ratio(b, amb, a):
    """Gamma(b + 1) Gamma(a - b) / Gamma(a), through lgamma where a factor leaves the f64 range."""
    try:
        v = math.gamma(b + 1.) * math.gamma(amb) / math.gamma(a)
        if math.isfinite(v) and v != 0.0:
            return v
    except (OverflowError, ValueError):
        pass
    sgn = lambda x: 1.0 if x > 0 or math.floor(x) % 2 == 0 else -1.0
    lg = math.lgamma(b + 1.) + math.lgamma(amb) - math.lgamma(a)
    return sgn(b + 1.) * sgn(amb) * sgn(a) * math.exp(lg)


def hyp_plan(a, b):
    """-> dict(k1, k2, a_switch) or None (refused).  The Pfaff series serves A <= a_switch, the 1/z
    connection formula A > a_switch; a_switch is the smallest of HYP_SWITCHES at which the connection
    formula loses at most HYP_MAX_LOSS to cancellation and ends within HYP_CONN_TERMS (probed at a few
    A >= a_switch) while the Pfaff series at a_switch ends within HYP_MAX_TERMS."""
    amb = a - b
    nonpos_int = lambda v, tol: v < 0.5 and abs(v - round(v)) < tol
    if nonpos_int(amb, 1e-9) or nonpos_int(b, 1e-6) or nonpos_int(b + 1., 1e-6) or b == a:
        return None
    k1 = b / (b - a)
    k2 = 0.0 if (a <= 0.0 and a == round(a)) else _gamma_ratio(b, amb, a)
    if not (math.isfinite(k1) and math.isfinite(k2)):
        return None
    for sw in HYP_SWITCHES:
        s_max = sw / (1.0 + sw) if math.isfinite(sw) else 1.0
        if hyp_series(a, b, np.array([s_max]))[2][0] > HYP_MAX_TERMS:
            break                                  # a larger switch needs still more terms
        if not math.isfinite(sw):                  # large b: the Pfaff series alone, for every A
            return dict(k1=k1, k2=k2, a_switch=sw)
        A = sw * np.array(HYP_PROBES)
        sa = (A / (1.0 + A)) ** a
        ser, big, conv = hyp_series(a, amb, 1.0 / (1.0 + A))
        t2 = k2 * A ** amb
        tot = sa * k1 * ser + t2
        with np.errstate(all="ignore"):
            loss = np.maximum(np.abs(sa * k1) * big, np.abs(t2)) / np.abs(tot)
        if np.all(conv <= HYP_CONN_TERMS) and np.all(loss <= HYP_MAX_LOSS):
            return dict(k1=k1, k2=k2, a_switch=sw)
    return None


def hyp_flow_factor(a, b, plan, A):
    """A^a 2F1(a, b; b + 1; -A) for A > 0 as the device evaluates it."""
    s = A / (1.0 + A)
    sa = s ** a
    low = A <= plan["a_switch"]
    out = np.empty_like(A)
    out[low] = sa[low] * hyp_series(a, b, s[low])[0]
    hi = ~low
    out[hi] = sa[hi] * plan["k1"] * hyp_series(a, a - b, 1.0 / (1.0 + A[hi]))[0] + \
        plan["k2"] * A[hi] ** (a - b)
    return out


def device_launch_times(params, rc, ww):
    """fields.hip:flow_time_antiderivative / build_fields_kernel (ts_mode 1 and 2) in NumPy [s], or
    None where rjp_build_fields refuses."""
    g, t, pl = params["geometry"], params["target"], params["power_laws"]
    au = orc.AU
    mr0, r0, v0 = g["mod_r_0"] * au, g["r_0"] * au, params["properties"]["v_0"] * 1e3
    eps, q_v, a = g["epsilon"], pl["q_v"], pl["q^d_v"]
    b = (1. - q_v + eps * a) / eps
    const = mr0 ** q_v / (v0 * (1. - q_v + eps * a))
    if a == 0.0:
        rad = rc * au + g["mod_r_0"] * au - g["r_0"] * au
        base = const * (r0 + mr0 - r0) ** (1. - q_v)
        return (const * rad ** (1. - q_v) - base) / orc.YEAR * orc.YEAR
    plan = hyp_plan(a, b)
    if plan is None:
        return None

    def anti(r_m, w_m):
        rad = r_m + mr0 - r0
        lead = const * rad ** (1. - q_v)
        A = (t["R_1"] * au * (g["w_0"] * au) * rad ** eps) / \
            (w_m * mr0 ** eps * (t["R_2"] * au - t["R_1"] * au))
        return lead * hyp_flow_factor(a, b, plan, A)

    w_m = ww * au
    return (anti(rc * au, w_m) - anti(np.full_like(w_m, r0), w_m)) / orc.YEAR * orc.YEAR


def within(got, ref, scale=1.0):
    return np.abs(got - ref) <= scale * (RTOL * np.abs(ref) + ATOL)


def rel_err(got, ref):
    """Worst |got - ref| / max(|ref|, 1e7 s): relative to the launch time, but to no less than the
    time at which the bound's absolute term equals its relative one."""
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), ATOL / RTOL)))


# ---- the tests -----------------------------------------------------------------------------------
def test_fixture_belongs_to_the_case_table():
    z, cases = load_fixture()
    assert str(z["table_hash"]) == GEN.table_hash(), \
        "tests/golden/k4_times.npz is older than the case table: run make_k4_times_golden.py"
    assert [c["name"] for c in cases] == [c["name"] for c in GEN.CASES]
    assert os.path.getsize(FIXTURE) < 256 * 1024
    for c in GEN.CASES:
        n = z[c["name"] + "/idx"].size
        assert 0 < n <= GEN.MAX_CELLS
        assert np.isfinite(z[c["name"] + "/ts"]).all()
        if "crossover" in c["tags"]:
            A = z[c["name"] + "/A"]
            for lo, hi in ((0.0, 1.0), (1.0, 1.5), (1.5, 10.0)):
                assert ((A > lo) & (A <= hi)).sum() >= 20, (c["name"], lo, hi)


@pytest.mark.parametrize("case", GEN.CASES, ids=lambda c: c["name"])
def test_fixture_recomputes(case):
    """10 cells per case again at 50 digits: equal to 1 ulp (the geometry is float64 NumPy)."""
    pytest.importorskip("mpmath")
    z, _ = load_fixture()
    jet, rc, ww, mask, A, a, b = GEN.case_geometry(case)
    idx = z[case["name"] + "/idx"]
    assert mask[idx].all()
    sel = np.linspace(0, idx.size - 1, 10).astype(int)
    ts = GEN.ref_times(rc[idx[sel]], ww[idx[sel]], jet.params)
    ref = z[case["name"] + "/ts"][sel]
    assert np.all(np.abs(ts - ref) <= np.spacing(np.abs(ref))), (ts, ref)
    np.testing.assert_array_equal(A[idx], z[case["name"] + "/A"])


# The oracle (scipy.special.hyp2f1 in float64) against the fixture, per family: (upper bound on
# rel_err over the sampled cells where scipy is finite, sampled cells where it is NOT finite).
# Measured with scipy 1.15.3: typical 3.4e-14, large_b 2.5e-15 (31 cells of
# big_b150 NaN), huge_b 4.7e-16 (34 cells NaN), near_degenerate 2.3e-10 (d = 5e-7; 1.0e-10 at 2e-6,
# 3.3e-11 at 1e-5), degenerate 5.6e-16, a_integer 7.1e-15, closed_form 1.8e-15.  So scipy itself
# misses the 1e-10 bound on the near-degenerate family and returns NaN for b >= 150 at A >= 2.5.
ORACLE_DEVIATION = {
    "typical": (2e-13, 0), "large_b": (2e-14, 40), "huge_b": (2e-14, 40),
    "near_degenerate": (1e-9, 0), "degenerate": (1e-14, 0), "a_integer": (5e-14, 0),
    "closed_form": (2e-14, 0),
}


def oracle_deviation():
    z, cases = load_fixture()
    worst = {}
    for c in cases:
        ref, f64 = z[c["name"] + "/ts"], z[c["name"] + "/ts_f64"]
        ok = np.isfinite(f64)
        dev, bad = worst.get(c["family"], (0.0, 0))
        worst[c["family"]] = (max(dev, rel_err(f64[ok], ref[ok])), max(bad, int((~ok).sum())))
    return worst


def test_oracle_deviation_per_family():
    worst = oracle_deviation()
    print("oracle (scipy) deviation from the 50-digit fixture (rel_err, non-finite cells):", worst)
    assert set(worst) == set(ORACLE_DEVIATION)
    for fam, (bound, n_bad) in ORACLE_DEVIATION.items():
        assert worst[fam][0] <= bound and worst[fam][1] <= n_bad, (fam, worst[fam])


def test_host_fallback_on_the_degenerate_case():
    """q_v = 0, eps = 1/2: a - b = -2, refused by the device; JetModel._host_launch_times."""
    from rajepy_amd.classes import JetModel
    z, _ = load_fixture()
    case = next(c for c in GEN.CASES if c["name"] == "degenerate")
    assert hyp_plan(1.0, 3.0) is None
    from rajepy_amd import logger
    p = GEN.case_params(case)
    p["ejection"] = {k: np.array(v) for k, v in p["ejection"].items()}
    model = JetModel(p, log=logger.Log(os.devnull, verbose=False))      # no device is touched
    ts = model._host_launch_times().ravel()
    idx, ref = z["degenerate/idx"], z["degenerate/ts"]
    assert within(ts[idx], ref).all(), rel_err(ts[idx], ref)


def test_restated_rule_holds_the_bound():
    """The switch rule, the term cap and the refusals, on the CPU first."""
    z, _ = load_fixture()
    refused, report = [], {}
    for c in GEN.CASES:
        jet, rc, ww, mask, A, a, b = GEN.case_geometry(c)
        idx, ref = z[c["name"] + "/idx"], z[c["name"] + "/ts"]
        with np.errstate(all="ignore"):
            got = device_launch_times(jet.params, rc[idx], ww[idx])
        if got is None:
            refused.append(c["name"])
            assert "may_refuse" in c["tags"] or c["family"] == "degenerate", c["name"]
            continue
        with np.errstate(all="ignore"):             # finite on the whole jet mask, not only the sample
            assert np.isfinite(device_launch_times(jet.params, rc[mask], ww[mask])).all(), c["name"]
        report[c["family"]] = max(report.get(c["family"], 0.0), rel_err(got, ref))
        assert within(got, ref).all(), (c["name"], rel_err(got, ref))
    print("restated device rule, worst relative error per family:", report, "refused:", refused)
    assert len(refused) <= 9 + 1                   # the exactly degenerate case on top


def test_plan_keeps_the_old_switch_where_it_was_right():
    """Typical b: the connection formula is sound from A = 1 on; the plan leaves it there."""
    assert hyp_plan(-0.4, (1. + 0.1 - 0.6 * 0.4) / 0.6)["a_switch"] == 1.0
    assert hyp_plan(1.3, 13.0)["a_switch"] > 1.0
    huge = hyp_plan(1.5, 179.68181818181816)          # Gamma(b + 1) overflows: through lgamma
    assert math.isfinite(huge["k2"]) and huge["a_switch"] == math.inf
