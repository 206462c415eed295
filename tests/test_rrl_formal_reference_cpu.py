"""The NumPy reference of the RRL formal solution (tests/rrl_formal_ref.py), pinned on the two golden
models through the oracle before tests/test_gpu_rrl_formal.py holds the kernel to it: the
recurrence equals the difference of the two chains, and on the isothermal model the reference's
own product B(T_avg) e^-tau_ff (1 - e^-tau_rrl).

Below that, the long-double reference and its per-pixel bound (tests/rrl_formal_ld_ref.py) on the
hand-made inputs the GPU tests run: the derivative formulas against finite differences, the walk
against a 50-digit mpmath evaluation of the two chains, the rounding term against the float64
recurrence, and the errors the bound must catch where rrl_formal_ref.within does not.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U
from tests import rrl_formal_ld_ref as L
from tests import rrl_formal_ref as R


def _oracle_case(tag):
    from rajepy_amd import engine as E
    z, meta, p, g, jet = U.golden_dense(tag)
    jet.time = float(z["years"][0]) * orc.YEAR
    rf = np.asarray(z["rrl_freqs"], dtype=np.float64)
    with np.errstate(all="ignore"):
        c = jet.optical_depth_ff(rf, collapse=False)
        l = jet.optical_depth_rrl(meta["rrl"], rf, collapse=False)
    csrc, hnu_k = E.rrl_channel_coeffs(rf, jet.csize, p["target"]["dist"])
    return z, jet, c, l, csrc, hnu_k


@pytest.mark.parametrize("tag", ["cfg1_example", "tilted"])
def test_recurrence_equals_the_chain_difference_and_the_isothermal_product(tag):
    z, jet, c, l, csrc, hnu_k = _oracle_case(tag)
    rec = R.np_rrl_formal(c, l, jet.temperature, hnu_k, csrc)
    chains = R.np_rrl_formal_chains(c, l, jet.temperature, hnu_k, csrc)
    assert np.array_equal(np.isnan(rec), np.isnan(chains))
    top = np.nanmax(np.abs(rec), axis=(1, 2))[:, None, None]
    assert np.nanmax(np.abs(rec - chains) / top) <= 1e-10
    gold = z["flux_rrl_contsub"]
    assert np.array_equal(np.isnan(rec), np.isnan(gold))
    line = np.isfinite(gold) & (gold != 0.0)
    assert line.sum() > 100
    rel = np.abs(rec[line] / gold[line] - 1.0)
    if tag == "cfg1_example":
        # T is constant along every sightline: the sum telescopes to the reference's product
        assert rel.max() <= 1e-11, rel.max()
        assert R.within(rec, gold, 1e-11) <= 1.0
    else:
        # q_T = -0.05, q^d_T = -0.1: the isothermal product mis-weights the cells
        assert np.mean(rel > 1e-3) >= 0.5, np.mean(rel > 1e-3)
        assert rel.max() < 0.1


def test_two_cells_closed_form():
    """Cold in front of hot, both with line and continuum opacity: the recurrence against the
    closed form of two cells; negative when the hot cell behind is thick in the continuum."""
    c = np.array([0.3, 40.0]).reshape(1, 1, 2, 1)
    l = np.array([0.2, 0.5]).reshape(1, 1, 2, 1)
    temp = np.array([5e3, 2e4]).reshape(1, 2, 1)
    hk = np.array([1.07])
    B = 1.0 / np.expm1(hk[0] / temp.ravel())
    c1, c2, l1, l2 = 0.3, 40.0, 0.2, 0.5
    tot = B[0] * -np.expm1(-(c1 + l1)) + B[1] * -np.expm1(-(c2 + l2)) * np.exp(-(c1 + l1))
    cont = B[0] * -np.expm1(-c1) + B[1] * -np.expm1(-c2) * np.exp(-c1)
    got = R.np_rrl_formal(c, l, temp, hk, [1.0])[0, 0, 0]
    assert got == pytest.approx(tot - cont, rel=1e-12)
    assert got < 0.0
    mirror = R.np_rrl_formal(c[:, :, ::-1], l[:, :, ::-1], temp[:, ::-1], hk, [1.0])[0, 0, 0]
    assert mirror > 0.0


def test_pipeline_execute_accepts_formal_rrl(tmp_path):
    """`formal_rrl` is a keyword of Pipeline.execute (default False); formal=True alone still
    refuses a run table with an RRL run, formal=True with formal_rrl=True does not."""
    from rajepy_amd import classes, logger
    from tests.test_host_logic import example_params, pline_params
    par = inspect.signature(classes.Pipeline.execute).parameters
    assert par["formal_rrl"].default is False
    dcy = str(tmp_path / "out")
    os.makedirs(dcy)
    log = logger.Log(os.path.join(dcy, "model.log"), verbose=False)
    jm = classes.JetModel(example_params(), log=log)
    pl = classes.Pipeline(jm, pline_params(dcy), log=log)
    assert any(r.obs_type != "continuum" for r in pl.runs)
    with pytest.raises(ValueError):
        pl.execute(simobserve=False, verbose=False, dryrun=True, formal=True)
    for kw in ({"formal_rrl": True}, {"formal": True, "formal_rrl": True}):
        pl.execute(simobserve=False, verbose=False, dryrun=True, resume=False, **kw)
    assert par["formal"].default is False


# ---- the long-double reference and its bound (tests/rrl_formal_ld_ref.py) ----------------------------
needs_ld = pytest.mark.skipif(not L.HAVE_LD, reason=L.LD_REASON)
LD = L.LD
CPU_NCHAN = 5                # the per-lane layout's bound (1e-9); 21 where a test says so
_REFS = {}


def _line():
    from rajepy_amd.maths import rrls
    return rrls.line_constants("H66a")


def _ref(name, nchan=CPU_NCHAN, band=None):
    """(case, reference) of an input on the fields an f64 upload holds: computed once, never changed."""
    key = (name, nchan, band)
    if key not in _REFS:
        cs = L.case(name, _line(), nchan, band=band)
        _REFS[key] = (cs, L.reference_of(cs, L.host_dev(cs), _line()))
    return _REFS[key]


def test_planck_bounds_are_the_ones_the_code_states():
    """EPS_B and the two criteria of tests/rrl_formal_ld_ref.py are read off band_needs_exp
    (rrl_voigt.h) and the per-lane criterion of rrl_formal.hip: the sources still say so."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rajepy_amd",
                        "csrc")
    voigt = open(os.path.join(csrc, "rrl_voigt.h")).read()
    formal = open(os.path.join(csrc, "rrl_formal.hip")).read()
    m = re.search(r"bool band_needs_exp\(.*?return !\(0\.5 \* \(a \* dnu_max\) \* \(a \* dnu_max\) < "
                  r"([0-9.e+-]+) \* \(1\.0 - E0\)\);", voigt, re.S)
    assert m and float(m.group(1)) == L.CRIT_WAVE == L.EPS_B_WAVE
    m = re.search(r"!\(ad \* ad \* ad < ([0-9.e+-]+) \* \(1\.0 - cl\.E0\)\)", formal)
    assert m and float(m.group(1)) == L.CRIT_LANE == 6.0 * L.EPS_B_LANE
    assert L.E_EXP * L.U0 >= 4e-15           # one_minus_exp_neg's stated relative error (rjp_device.h)


@needs_ld
@pytest.mark.parametrize("name", L.INPUTS)
def test_derivative_formulas_against_finite_differences(name):
    """dI/dl_i, dI/dc_i and dI/dB_i of a whole row of cells at a time (sightlines are independent)
    against central differences of the long-double walk, relative step 1e-6.  The step's own error
    is h^2 / 6 of the third logarithmic derivative, <= 1e-12 * 50^2 of the summands' magnitudes; the
    bar is 1e-5 of them (B enters linearly: 1e-9)."""
    cs, r = _ref(name)
    q = r["q"]
    c, l, B = q["c"], q["l"], q["B"]
    s = L.sensitivities(c, l, B)
    h = LD(1e-6)
    ny = c.shape[2]
    for row in (0, 7, 8, 31, 36, ny - 1):
        for key, an, scale, bar in (("l", l * s["dIdl"], l * s["scale_l"], 1e-5),
                                    ("c", c * s["dIdc"], c * s["scale_c"], 1e-5),
                                    ("B", B * s["E"], B * np.abs(s["E"]), 1e-9)):
            up = {"c": c.copy(), "l": l.copy(), "B": B.copy()}
            dn = {"c": c.copy(), "l": l.copy(), "B": B.copy()}
            up[key][:, :, row] *= 1 + h
            dn[key][:, :, row] *= 1 - h
            fd = (L.walk(up["c"], up["l"], up["B"]) - L.walk(dn["c"], dn["l"], dn["B"])) / (2 * h)
            err = np.abs(fd - an[:, :, row])
            # the walk's own roundings, seen through the division by 2 h
            floor = np.sum(s["mag"], axis=2) * (80 * c.shape[2] * 2.0 ** -63 / 2e-6)
            assert np.all(err <= bar * scale[:, :, row] + floor), (name, key, row, float(np.max(err)))


def _mp_chains(c, l, temp, hk, cs):
    """I_tot - I_cont of one sightline and channel at 50 digits."""
    import mpmath as mp
    mp.mp.dps = 50
    big = lambda v: mp.mpf(float(v)) + mp.mpf(float(v - LD(float(v))))      # a long double, exactly
    tot = cont = mp.mpf(0)
    tt = tc = mp.mpf(0)
    for ci, li, tk in zip(c, l, temp):
        if ci == 0 and li == 0:
            continue
        ci, li = big(ci), big(li)
        Bp = 1 / mp.expm1(mp.mpf(float(hk)) / mp.mpf(float(tk)))
        tot += Bp * -mp.expm1(-(ci + li)) * mp.exp(-tt)
        cont += Bp * -mp.expm1(-ci) * mp.exp(-tc)
        tt += ci + li
        tc += ci
    return mp.mpf(float(cs)) * (tot - cont)


@needs_ld
def test_walk_against_a_50_digit_evaluation_of_the_two_chains():
    """Twelve sightlines, the thick ones among them (front cells of c = 1 ... 30, their mirror,
    tau_C = 100 and 600, per-cell l of 50, bursts, continuum-only and dead cells), at the centre and
    the first channel: the long-double recurrence against mpmath's I_tot - I_cont.  The walk's error
    is the bound's rounding term with 2^-64 for 2^-53."""
    import mpmath as mp
    picks = [("thick", 0, z) for z in range(5)] + [("thick", 1, 4), ("thick", 0, 10),
                                                   ("thick", 1, 13), ("thickline", 0, 0),
                                                   ("thickline", 1, 8), ("spread", 0, 0),
                                                   ("mixed", 0, 1)]
    assert len(picks) == 12
    for name, x, z in picks:
        cs, r = _ref(name)
        q, temp = r["q"], L.host_dev(cs)["temp"]
        for f in (0, CPU_NCHAN // 2):
            want = _mp_chains(q["c"][f, x, :, z], q["l"][f, x, :, z], temp[x, :, z], cs["hnu_k"][f],
                              cs["csrc"][f])
            got = r["ref_ld"][f, x, z]
            err = abs(mp.mpf(float(got)) + mp.mpf(float(got - LD(float(got)))) - want)
            allowed = r["terms"][3][f, x, z] * 2.0 ** -11
            assert err <= allowed, (name, x, z, f, float(err), allowed, float(want))


@needs_ld
@pytest.mark.parametrize("name", L.INPUTS)
def test_float64_recurrence_stays_inside_the_rounding_term(name):
    """rrl_formal_ref.np_rrl_formal (float64, exp(-c), NumPy's libm) on the float64-rounded per-cell
    depths against the long-double walk of the same values: inside the rounding term ALONE (every
    eps = 0), which checks rho against an independent implementation.  And the long-double walk
    against the long-double chains where tau_C <= 20, to 2^-64 times the roundings of I_tot."""
    cs, r = _ref(name)
    q = r["q"]
    c64, l64 = q["c"].astype(np.float64), q["l"].astype(np.float64)
    q64 = dict(q, c=c64.astype(LD), l=l64.astype(LD))
    temp = L.host_dev(cs)["temp"]
    got = R.np_rrl_formal(c64, l64, temp, cs["hnu_k"], cs["csrc"])
    cs_ld = cs["csrc"].astype(LD)[:, None, None]
    ref = np.where(q["hot"][None], cs_ld * L.walk(q64["c"], q64["l"], q64["B"]), LD("nan"))
    rounding = L.bound_terms(q64, cs["csrc"])[3]
    share, _, at = L.judge(got, dict(ref_ld=ref, bound=rounding, terms=[rounding] * 4), name)
    print(name, "float64 recurrence: %.3f of the rounding term at %r" % (share, at))
    assert share <= 1.0, (name, share, at)
    diff, size = L.chains(q["c"], q["l"], q["B"])
    thin = np.sum(q["c"], axis=2) <= 20
    assert thin.any()
    n = q["c"].shape[2]
    assert np.all(np.abs(L.walk(q["c"], q["l"], q["B"]) - diff)[thin] <=
                  (80 * n * 2.0 ** -63 * size + r["terms"][3] * 2.0 ** -11 /
                   np.abs(cs["csrc"])[:, None, None])[thin])


def _walk64(c, l, B, e_c_by_subtraction=False, reset_d=0, drop_ud=False):
    """The float64 recurrence with the errors the bound must catch."""
    I = np.zeros(c.shape[:2] + c.shape[3:])
    D, Th = np.zeros_like(I), np.ones_like(I)
    for iy in range(c.shape[2]):
        ci, li, Bi = c[:, :, iy], l[:, :, iy], B[:, :, iy]
        if reset_d and iy and iy % reset_d == 0:
            D = np.zeros_like(I)
        e_c = 1.0 - (-np.expm1(-ci)) if e_c_by_subtraction else np.exp(-ci)
        om_l = -np.expm1(-li)
        u = -np.expm1(-ci) + e_c * om_l
        I = I + Bi * (e_c * om_l * Th - (0.0 if drop_ud else u * D))
        D = e_c * (D + (Th - D) * om_l)
        Th = Th * e_c
    return I


def _f64(r, cs):
    q = r["q"]
    return (q["c"].astype(np.float64), q["l"].astype(np.float64), q["B"].astype(np.float64),
            cs["csrc"][:, None, None])


@needs_ld
@pytest.mark.parametrize("nchan", [5, 21])
def test_e_c_by_subtraction_exceeds_the_bound_behind_a_thick_front_cell(nchan):
    """e_c = 1 - (1 - e^-c) carries e^c 2^-53 of relative error.  Behind a front cell of c = 30 the
    pixel B e^-c (1 - e^-l) inherits all of it (1.7e-4): outside the bound on either layout's Voigt
    budget, and at c = 20 (2e-8) outside the per-lane layout's 1e-9.  rrl_formal_ref.within passes
    both: the bright pixels of the channel set its scale."""
    cs, r = _ref("thick", nchan)
    c, l, B, csrc = _f64(r, cs)
    bad = np.where(r["q"]["hot"][None], csrc * _walk64(c, l, B, e_c_by_subtraction=True), np.nan)
    good = np.where(r["q"]["hot"][None], csrc * _walk64(c, l, B), np.nan)
    assert L.judge(good, r)[0] <= 1.0
    share = np.abs(bad - r["ref"]) / r["bound"]
    print("thick front cells, e_c by subtraction, %d channels: error / bound at c = 1 ... 30:" % nchan,
          [float(share[:, 0, z].max()) for z in range(5)])
    for z in (4, 9):
        assert share[:, 0, z].max() > 1.0, (z, share[:, 0, z].max())
    if nchan <= 16:
        assert max(share[:, 0, 3].max(), share[:, 0, 8].max()) > 1.0
    assert R.within(bad, r["ref"], U.k3_rtol(nchan)) <= 1.0


MUTANTS = ["reset D at rows 8 k", "reset D at rows 16 k", "reset D at rows 32 k", "drop u D",
           "l off by 1e-6", "first-order B on 0.7-1.3"]


@needs_ld
@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("nchan", [5, 21])
def test_mutants_on_faint_sightlines_exceed_the_bound_and_pass_within(mutant, nchan):
    """Each error applied to the faint sightlines alone (pixels at most 1e-4 of their channel's
    brightest): every one of those pixels' sightlines leaves the bound on some channel, and
    rrl_formal_ref.within still passes the map."""
    wide = mutant.startswith("first-order")
    cs, r = _ref("wide" if wide else "faint", nchan)
    c, l, B, csrc = _f64(r, cs)
    faint = cs["faint"]
    top = np.nanmax(np.abs(r["ref"]), axis=(1, 2))[:, None]
    assert np.all(np.abs(r["ref"][:, faint]) <= 1e-4 * top)
    good = csrc * _walk64(c, l, B)
    if mutant.startswith("reset D"):
        bad = _walk64(c, l, B, reset_d=int(mutant.split()[-2]))
    elif mutant == "drop u D":
        bad = _walk64(c, l, B, drop_ud=True)
    elif mutant == "l off by 1e-6":
        bad = _walk64(c, l * (1.0 + 1e-6), B)
    else:
        line, temp = _line(), L.host_dev(cs)["temp"]
        nu_ref = 0.5 * (cs["nu"].min() + cs["nu"].max())
        x0 = line["h_over_k"] * nu_ref / temp
        dh = (cs["hnu_k"] - line["h_over_k"] * nu_ref)[:, None, None, None]
        B1 = temp * np.exp(-x0) / (temp * -np.expm1(-x0) + dh)
        bad = _walk64(c, l, np.where(B != 0.0, B1, 0.0))
    out = np.where(faint[None], csrc * bad, good)
    assert L.judge(good, r)[0] <= 1.0
    share = np.abs(out - r["ref"]) / r["bound"]
    worst = share[:, faint].max(axis=0)
    print(mutant, nchan, "channels: error / bound on the faint sightlines %.3g ... %.3g"
          % (worst.min(), worst.max()))
    assert np.all(worst > 1.0), worst
    assert np.all(share[:, ~faint] <= 1.0)
    assert R.within(out, r["ref"], U.k3_rtol(nchan)) <= 1.0
