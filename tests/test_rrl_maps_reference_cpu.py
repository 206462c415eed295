"""The long-double reference of the recombination-line map stage (tests/rrl_maps_ref.py) before
tests/test_gpu_rrl_maps.py holds rjp_rrl_maps to it: the reference against 50 digits, a float64
emulation of the kernel inside the bound on the very inputs the GPU tests use (the inputs are
feasible), and each planted mistake pushed over the bound by a named input set.  No GPU."""
import numpy as np
import pytest

from tests import rrl_maps_ref as R

CASES = [("tails-%dx%d-%s" % (P, F, "total" if ff else "contsub"), (P, F, ff))
         for P, F in R.TAIL_SHAPES for ff in (False, True)]


def _case(name):
    return R.radio_case() if name == "radio" else R.tail_case(*dict(CASES)[name])


# ---- the reference against 50 digits -----------------------------------------------------------
def _mpf(mp, v):
    """A long double as an mpf, exactly."""
    if not np.isfinite(v):
        return mp.mpf(float(v))
    m, e = np.frexp(v)
    return mp.mpf(int(np.ldexp(m, 64))) * mp.mpf(2) ** (int(e) - 64)


def test_long_double_reference_against_50_digits():
    """A few hundred points: every planted edge value of the tail sets (P = 63: all of them, over
    two channels, with the continuum) and a sample of the radio band.  Allowed: the long double's
    own roundings, (8 + kappa(x)) of its epsilons on the line, one more on the sum, and its
    smallest subnormal."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 50
    eps = mp.mpf(2) ** -63
    tiny = mp.mpf(2) ** -16445
    c = R.tail_case(63, 2, True)
    r = R.radio_case()
    sets = [(c, range(63)), (r, range(0, 4097, 41))]
    n = 0
    for case, pixels in sets:
        ref = R.flux_ref(*R.args_of(case))
        F = ref.shape[0]
        for f in range(F):
            for p in pixels:
                T = case["tavg"][p]
                cont = None if case["flux_ff"] is None else case["flux_ff"][f, p]
                if np.isnan(T) or (cont is not None and np.isnan(cont)):
                    assert np.isnan(ref[f, p])
                    continue
                x = mp.mpf(float(case["hnu_k"][f])) / mp.mpf(float(T))
                t_l, t_c = float(case["tau_rrl"][f, p]), float(case["tau_ff"][f, p])
                om = mp.mpf(1) if np.isinf(t_l) else -mp.expm1(-mp.mpf(t_l))
                line = mp.mpf(float(case["cflux"][f])) / mp.expm1(x) * mp.exp(-mp.mpf(t_c)) * om
                want = line if cont is None else line + mp.mpf(float(cont))
                kappa = x / (1 - mp.exp(-x))
                allow = eps * abs(line) * (8 + kappa) + eps * abs(want) + tiny
                assert abs(_mpf(mp, ref[f, p]) - want) <= allow, (f, p)
                n += 1
    assert n >= 300
    # the edge values were among the points
    for name, _, v in R.PLANTS:
        assert R.pixel_of(name, v, 63) is not None


def test_worst_ratio_rules():
    ref = np.array([[1.0, np.nan, 0.0]])
    b = np.array([[1e-15, np.nan, 0.0]])
    assert R.worst_ratio(np.array([[1.0 + 4e-16, np.nan, 0.0]]), ref, b) < 1.0
    assert R.worst_ratio(np.array([[1.0, 0.0, 0.0]]), ref, b) == np.inf       # NaN lost
    assert R.worst_ratio(np.array([[np.nan, np.nan, 0.0]]), ref, b) == np.inf  # NaN gained
    assert R.worst_ratio(np.array([[1.0, np.nan, 5e-324]]), ref, b) == np.inf  # bound 0: equal
    assert R.n_additions(1) == 21 and R.n_additions(256 * 256) == 21
    assert R.n_additions(256 * 257 + 1) == 22
    assert abs(R.C0 - 44.03) < 0.01


# ---- the inputs are what the issue asks for -----------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in CASES])
def test_tail_inputs_hold_their_planted_values(name):
    P, F, ff = dict(CASES)[name]
    c = R.tail_case(P, F, ff)
    ref = R.flux_ref(*R.args_of(c))
    line = R.flux_ref(c["tau_rrl"], c["tau_ff"], c["tavg"], None, c["cflux"], c["hnu_k"])
    assert np.all(c["cflux"][1:] >= 2 * c["cflux"][:-1]) and len(set(c["hnu_k"])) == F
    # the channel's largest value sits in the last pixel
    assert np.all(ref[:, P - 1] == np.nanmax(ref, axis=1))
    px = lambda n, v: R.pixel_of(n, v, P)
    if P >= 63:
        assert all(px(n, v) is not None for n, _, v in R.PLANTS)
        assert np.all(line[:, px("tau_rrl", 0.0)] == 0) and not np.signbit(
            line[:, px("tau_rrl", 0.0)]).any()
        assert np.all(line[:, px("tau_rrl", 1e-300)] > 0)
        assert np.all(line[:, px("tau_ff", 1e4)].astype(np.float64) == 0)
        sub = line[:, px("tau_ff", 745.0)].astype(np.float64)
        assert np.all((sub >= 0) & (sub < 2.0 ** -1022))
        assert np.isnan(ref[:, px("tavg", np.nan)]).all()
        assert np.isnan(ref).sum() == (2 * F if ff else F)
        if ff:
            assert np.isnan(ref[:, px("flux_ff", np.nan)]).all()
            assert np.isfinite(line[:, px("flux_ff", np.nan)]).all()
    else:
        assert P == 1 and np.isfinite(ref).all()


def test_radio_inputs_cover_the_band():
    c = R.radio_case()
    x = c["hnu_k"][:, None] / c["tavg"][None, :]
    assert 2e-6 < x.min() < 3e-6 and 4e-4 < x.max() < 5e-4
    assert c["tau_rrl"].min() < 1e-5 and c["tau_rrl"].max() > 20
    assert c["tau_ff"].min() < 1e-5 and c["tau_ff"].max() > 20


# ---- a correct kernel fits ------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in CASES] + ["radio"])
def test_float64_emulation_stays_inside_the_bound(name):
    c = _case(name)
    flux, ftot = R.emulate(c)
    rf, rt = R.ratios(flux, ftot, c)
    print("%s: emulation / bound: flux %.3f, ftot %.3f" % (name, rf, rt))
    assert rf <= 1.0 and rt <= 1.0
    px = None if name == "radio" else R.pixel_of("tau_rrl", 0.0, flux.shape[1])
    if px is not None and c["flux_ff"] is None:
        assert np.all(flux[:, px] == 0) and not np.signbit(flux[:, px]).any()     # +0.0


# ---- planted mistakes ----------------------------------------------------------------------------
# mistake -> (the input set that catches it, "flux" or "ftot": where it shows)
CAUGHT_BY = {
    "exp(x) - 1": ("radio", "flux"),
    "1 - exp(-tau_rrl)": ("tails-63x2-contsub", "flux"),        # thin columns, tau_rrl = 1e-300
    "neighbour channel": ("tails-63x2-contsub", "flux"),
    "channel 0": ("tails-257x3-contsub", "flux"),
    "tavg at f * P + p": ("tails-256x2-contsub", "flux"),
    "last partial workgroup left out": ("tails-257x3-total", "ftot"),   # the largest value at P - 1
    "NaN into ftot": ("tails-255x17-contsub", "ftot"),          # the tavg = NaN pixel
    "NaN continuum counted as its line": ("tails-4097x5-total", "ftot"),  # the NaN in flux_ff
    "continuum left out": ("tails-64x1-total", "flux"),
    "continuum twice": ("tails-1x1-total", "flux"),
    "exp(+tau_ff)": ("tails-65793x2-contsub", "flux"),
}


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_planted_mistake_is_caught(mistake):
    name, where = CAUGHT_BY[mistake]
    c = _case(name)
    rf, rt = R.ratios(*R.emulate(c, mistake), c)
    print("%s on %s: flux %.3g, ftot %.3g of the bound" % (mistake, name, rf, rt))
    assert (rf if where == "flux" else rt) > 1.0
    if where == "ftot":
        assert rf <= 1.0                    # only the total shows it
    # and the very same set passes without the mistake
    rf0, rt0 = R.ratios(*R.emulate(c), c)
    assert rf0 <= 1.0 and rt0 <= 1.0


def test_present_kernel_formula_loses_digits_in_the_radio_band():
    """exp(x) - 1 against the bound over the radio band: thousands of times over, on nearly every
    pixel (the figures of the issue: 4.5e-11 worst, 9200 times over, 99.7 % of the pixels)."""
    c = R.radio_case()
    flux, _ = R.emulate(c, "exp(x) - 1")
    ref, bound = R.flux_ref(*R.args_of(c)), R.flux_bound(*R.args_of(c))
    ratio = np.abs(flux - ref) / bound
    rel = np.abs(flux - ref) / np.abs(ref)
    print("exp(x) - 1: worst %.3g of the bound, relative %.3g, %.1f %% of the pixels over it"
          % (ratio.max(), rel.max(), 100 * np.mean(ratio > 1)))
    assert ratio.max() > 1e3 and np.mean(ratio > 1) > 0.9
