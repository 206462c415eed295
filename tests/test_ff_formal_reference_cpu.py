"""The long-double reference of the free-free formal solution and its per-pixel bound
(tests/ff_formal_ref.py), pinned before tests/test_gpu_ff_formal_ld.py holds K5 to them: the walk
against a 50-digit mpmath evaluation, the isothermal closed form, test_gpu_formal_rt.np_formal,
ff_formal_grad_ref.walk and the oracle on `tilted`; dI/dc_i against Richardson differences; a float64
restatement of formal_update inside the bound on every input the GPU tests run; planted mistakes
outside it (two of them INSIDE the flat rtol = 1e-11 the older tests use); and the bound itself no
wider than 1e-11 |ref| except where the module says why.  No GPU."""
import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import f32_ref as F
from tests import ff_formal_grad_ref as G
from tests import ff_formal_ref as R
from tests import gpu_util as U

pytestmark = pytest.mark.skipif(not R.HAVE_LD, reason=R.LD_REASON)
LD = R.LD
NCHAN = 17
_REFS = {}


def _ref(name, bursts=True, mode=0, ny=R.NY, nz=R.NZ, nchan=NCHAN):
    """(case, (a0, ts, temp), reference) on what the tau layout of an f64 upload holds: computed once,
    never changed."""
    key = (name, bursts, mode, ny, nz, nchan)
    if key not in _REFS:
        cs = R.case(name, nchan, ny=ny, nz=nz, mode=mode, bursts=bursts)
        arrays = R.host_arrays(cs)
        _REFS[key] = (cs, arrays, R.reference_of(cs, arrays))
    return _REFS[key]


def _emulated(cs, arrays, mistake=None, where=None, skip=None):
    b, _ = R.b_tau(arrays[0], arrays[1], cs["bursts"], cs["t"], T=np.float64, skip=skip)
    return R.emulate(b, arrays[2], cs["ctau"], cs["csrc"], mistake, where)


def _inside_rtol(got, ref, rtol=1e-11):
    """The older tests' bar: identical NaN / zero patterns and a flat relative tolerance -- on the
    pixels above 1e-300: below, no float64 result carries 1e-11 (the correct emulation does not)."""
    if not (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got == 0, ref == 0)):
        return False
    ok = np.isfinite(ref) & (np.abs(ref) > 1e-300)
    return bool(np.all(np.abs(got - ref)[ok] <= rtol * np.abs(ref)[ok]))


def _exact(v):
    """A long double as an mpmath number, exactly."""
    import mpmath as mp
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(v - LD(hi)))


# ---- the walk --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.INPUTS)
def test_walk_against_a_50_digit_evaluation(name):
    """Four sightlines of every input (for "thick": the front cells of dtau = 30 and 1e4, their
    mirrors, tau = 100 and 600) on three channels: the long-double sum against mpmath on the same
    c_i and T_i.  The walk's own error is the emission and csrc terms with 2^-64 for 2^-53; the summed
    depth in the exponent adds tau k 2^-64 <= 0.37 k 2^-64 to the term of cell k: 2^-9 of those terms
    (and the floor) is the bar."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    cs, arrays, r = _ref(name)
    picks = {"thick": [(0, 4), (0, 8), (1, 4), (1, 8), (0, 10), (1, 14)],
             "thin": [(0, 0), (0, 1), (1, 2), (0, 3), (1, 9)],
             "mixed": [(0, 3), (1, 5), (0, 0), (1, 11)]}.get(name, [(0, 0), (1, 1), (0, 8), (1, 16)])
    for x, z in picks:
        for f in (0, NCHAN // 2, NCHAN - 1):
            tot, front = mp.mpf(0), mp.mpf(0)
            for ci, ti in zip(r["c"][f, x, :, z], r["T"][f, x, :, z]):
                ci = _exact(ci)
                tot += _exact(ti) * -mp.expm1(-ci) * mp.exp(-front)
                front += ci
            want = mp.mpf(float(cs["csrc"][f])) * tot
            got = r["ref_ld"][f, x, z]
            if np.isnan(got):
                assert not np.any(arrays[2][x, :, z] > 0)
                continue
            allowed = 2.0 ** -9 * (r["terms"][1] + r["terms"][3] + r["terms"][4])[f, x, z]
            assert abs(_exact(got) - want) <= allowed, (name, x, z, f, float(want))


def test_isothermal_sightlines_give_the_closed_form():
    """T constant along the sightline: the sum telescopes to T (1 - e^-tau), thin, thick and with
    dead cells between."""
    rng = np.random.default_rng(5)
    c = (10.0 ** rng.uniform(-9, 1.5, (3, 2, 40, 9))).astype(LD)
    c[:, :, ::5] = 0
    temp = np.broadcast_to(10.0 ** rng.uniform(2.5, 4.5, (2, 1, 9)), (2, 40, 9)).copy()
    r = R.reference(c, np.full((2, 40, 9), R.U0), temp, [1.0, 2.0, 0.5])
    want = np.array([1.0, 2.0, 0.5], dtype=LD)[:, None, None] * temp[:, 0].astype(LD)[None] * \
        -np.expm1(-np.sum(c, axis=2))
    assert np.all(np.abs(r["ref_ld"] - want) <= 2.0 ** -9 * (r["terms"][1] + r["terms"][4]))


@pytest.mark.parametrize("name", R.INPUTS)
def test_reference_agrees_with_np_formal_and_the_gradient_reference(name):
    """test_gpu_formal_rt.np_formal (float64 cumsum, exp(-front)) on the float64-rounded c at its own
    1e-11 where the depth in front stays below 1e4 2^-53 / 1e-11, and ff_formal_grad_ref.walk(...)["I"]
    (long double, a running sum in the exponent) at 2^-9 of the rounding terms."""
    from tests.test_gpu_formal_rt import np_formal
    cs, arrays, r = _ref(name)
    a0, ts, temp = arrays
    c64 = np.where(r["c"] == 0, np.nan, r["c"]).astype(np.float64)
    old = np_formal(c64, np.where(np.isnan(temp), 0.0, temp), cs["csrc"])
    ref = r["ref"]
    assert np.array_equal(np.isnan(old), np.isnan(ref))
    ok = np.isfinite(ref) & (np.abs(ref) > 1e-300)
    assert np.all(np.abs(old - ref)[ok] <= 1e-11 * np.abs(ref)[ok])
    g = G.walk(a0, ts, temp, cs["bursts"] if cs["bursts"] is not None else ([], []), cs["t"],
               cs["ctau"], cs["csrc"])["I"]
    assert np.array_equal(np.isnan(g), np.isnan(ref))
    fin = ~np.isnan(ref)
    allowed = 2.0 ** -9 * (r["terms"][1] + r["terms"][3] + r["terms"][4])
    assert np.all(np.abs(g - r["ref_ld"])[fin] <= allowed[fin])


def _tilted():
    from rajepy_amd import engine as E
    z, meta, p, g, jet = U.golden_dense("tilted")
    freqs = np.asarray(z["freqs"], dtype=np.float64)
    assert p["power_laws"]["q_T"] != 0.
    ctau, cflux = E.ff_channel_coeffs(freqs, jet.csize, p["target"]["dist"], E.RJP_GFF_POWERLAW, None)
    return z, g, jet, freqs, ctau, cflux


def test_reference_agrees_with_the_oracle_on_tilted():
    """tests/golden/tilted at two golden epochs: the reference on the host restatement of the tau
    field against np_formal on the oracle's per-cell optical depths, at np_formal's 1e-11."""
    from tests.test_gpu_formal_rt import np_formal
    z, g, jet, freqs, ctau, cflux = _tilted()
    a0 = U.golden_a0(g, -0.05)
    for yr in z["years"][1:]:
        jet.time = float(yr) * orc.YEAR
        r = R.reference_tau(a0, g["ts"], g["temp"], F.burst_lists_of(jet), jet.time, ctau, cflux)
        with np.errstate(all="ignore"):
            want = np_formal(jet.optical_depth_ff(freqs, collapse=False), jet.temperature, cflux)
        assert np.array_equal(np.isnan(want), np.isnan(r["ref"]))
        assert np.array_equal(want == 0, r["ref"] == 0)
        ok = np.isfinite(want) & (want != 0)
        assert ok.sum() > 100
        assert np.all(np.abs(r["ref"] - want)[ok] <= 1e-11 * np.abs(want)[ok])


# ---- the sensitivities -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.INPUTS)
def test_sensitivities_against_richardson_differences(name):
    """dI/dc_i of a whole row of cells at a time (sightlines are independent) against Richardson's
    (4 D(h/2) - D(h)) / 3 of central differences with the step h c / (1 + c), h = 1e-3: its own error is
    h^4 / 30 of the fifth derivative, of the size of Theta e^-c (T + R) like every other; the bar is 1e-9
    of that, plus the walk's own roundings seen through the division by the step."""
    cs, arrays, r = _ref(name)
    c, T, s = r["c"], r["T"], r["s"]
    ny = c.shape[2]
    total = np.sum(s["t"], axis=2)
    sharp = 0
    for row in sorted({0, 1, 15, 16, 31, 32, ny - 1}):
        d = LD(1e-3) * c[:, :, row] / (1 + c[:, :, row])

        def diff(step):
            up, dn = c.copy(), c.copy()
            up[:, :, row] += step
            dn[:, :, row] -= step
            return (R.walk(up, T) - R.walk(dn, T)) / np.where(step > 0, 2 * step, 1)

        fd = (4 * diff(d / 2) - diff(d)) / 3
        live = d > 0
        err = np.abs(fd - s["dIdc"][:, :, row])
        floor = 8 * (ny + 2) * 2.0 ** -63 * total / np.where(live, d, 1)
        assert np.all(err[live] <= (1e-9 * s["scale"][:, :, row] + floor)[live]), (name, row)
        sharp += int(np.sum((1e-9 * s["scale"][:, :, row] > floor) & live))
    assert sharp >= 50, (name, sharp)       # (the bar is the formula's, not the floor's)


# ---- the float64 restatement of the kernel's update ----------------------------------------------------------
@pytest.mark.parametrize("bursts", [True, False])
@pytest.mark.parametrize("name", R.INPUTS)
def test_float64_emulation_stays_inside_the_bound(name, bursts):
    """formal_update with om = -expm1 in float64 on every input of the GPU tests: both Gaunt modes,
    the small grids, with and without bursts."""
    worst = 0.0
    for mode, ny, nz in [(0, R.NY, R.NZ), (1, R.NY, R.NZ)] + [(0, ny, R.NZ) for ny in R.NYS] + \
            [(0, R.NY, nz) for nz in R.NZS]:
        cs, arrays, r = _ref(name, bursts, mode, ny, nz)
        share, top, at = R.judge(_emulated(cs, arrays), r, name)
        assert share <= 1.0, (name, bursts, mode, ny, nz, share, top, at)
        worst = max(worst, share)
    print("float64 emulation, %s, %s bursts: worst share of the bound %.3g"
          % (name, "with" if bursts else "without", worst))


def _thin_where(cs):
    """The sightlines of "thin" with dtau = 1e-6 ... 1e-4."""
    w = np.zeros((R.NX, R.NZ), dtype=bool)
    w[:, len(R.THIN):] = True
    return w


# mistake: (input, with bursts, also inside rtol = 1e-11)
PLANTED = {"exp64": ("thin", False, True), "clamp30": ("thick", False, True),
           "float-dtau": ("spread", True, False), "far-end": ("coldfront", True, False),
           "theta-first": ("thick", True, False), "slab-reset": ("spread", True, False),
           "dead-T": ("mixed", True, False), "ninth-burst": ("spread", True, False)}


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_planted_mistakes_leave_the_bound(mistake):
    """Every planted mistake (ff_formal_ref.emulate) fails `judge` on its named input, the correct
    emulation passes it; "exp64" (on the sightlines of dtau = 1e-6 ... 1e-4) and "clamp30" (front and
    back cells of dtau >= 37) stay inside a flat rtol = 1e-11 on every pixel of that input: the new
    bar is the tighter one."""
    name, bursts, quiet = PLANTED[mistake]
    cs, arrays, r = _ref(name, bursts)
    assert R.judge(_emulated(cs, arrays), r)[0] <= 1.0
    where = _thin_where(cs) if mistake == "exp64" else None
    bad = _emulated(cs, arrays, None if mistake == "ninth-burst" else mistake, where,
                    skip=8 if mistake == "ninth-burst" else None)
    if mistake in ("dead-T", "theta-first"):
        # a NaN where the reference has none; a pixel behind dtau >= 37 that is 0 and must not be
        pattern = np.isnan if mistake == "dead-T" else (lambda a: a == 0)
        assert pattern(bad).sum() > pattern(r["ref"]).sum()
        with pytest.raises(AssertionError):
            R.judge(bad, r)
        return
    share, top, at = R.judge(bad, r)
    rel = np.nanmax(np.abs(bad - r["ref"]) / np.where(r["ref"] != 0, np.abs(r["ref"]), np.inf))
    print("%s on %s: %.3g bounds at (f, x, z) = %r (%s), %.3g of the pixel at worst"
          % (mistake, name, share, tuple(int(i) for i in at), top, rel))
    assert share > 1.0, (mistake, share)
    assert _inside_rtol(bad, r["ref"]) == quiet, (mistake, rel)
    assert len(PLANTED) >= 6 and sum(q for _, _, q in PLANTED.values()) >= 2


# ---- the bound is no wider than the bar it replaces -------------------------------------------------------------
# where bound > 1e-11 |ref|: the sightlines of dtau = 1e-320, whose pixels (~1e-315) are a few hundred
# units of 2^-1074 -- no float64 result carries 1e-11 there; the floor dominates.  No pixel needs the
# attenuation term for this: the cold front's costs 3.7e-13 of its pixel.
WIDER = {"thin": {(0, 0): "subnormal floor", (1, 0): "subnormal floor"}}


@pytest.mark.parametrize("bursts", [True, False])
@pytest.mark.parametrize("name", R.INPUTS)
def test_bound_is_at_most_1e_11_of_the_pixel(name, bursts):
    """bound <= 1e-11 |ref| on every finite non-zero pixel of every input except the listed ones,
    where the named term dominates the bound."""
    for mode in (0, 1):
        cs, arrays, r = _ref(name, bursts, mode)
        ref, bound = r["ref"], r["bound"]
        ok = np.isfinite(ref) & (ref != 0)
        assert ok.sum() >= ref.size // 2
        wide = ok & (bound > 1e-11 * np.abs(ref))
        listed = WIDER.get(name, {})
        for f, x, z in np.argwhere(wide):
            assert (x, z) in listed and R.dominant(r, (f, x, z)) == listed[x, z], (name, f, x, z)
        if not bursts:
            # without bursts only roundings are left: (E + 2 + n_y) 2^-53 and the cold front's 38 u T_max
            rest = ok & ~wide
            assert np.all(bound[rest] <= 4e-13 * np.abs(ref)[rest])
