"""tests/ff_maps_ref.py on the CPU, before any kernel is held to it: the long-double reference
against mpmath at 50 digits, the restated one_minus_exp_neg against 50 digits over every octave it
sees, the float64 emulation of K2's four launch shapes inside the bounds on every case of
tests/test_gpu_ff_maps.py (the cases are feasible), every planted mistake outside them (the
cases can tell), and the restated launch rule against shapes worked by hand."""
import mpmath
import numpy as np
import pytest

from tests import ff_maps_ref as M

mpmath.mp.dps = 50
LD_EPS = 2.0 ** -63                      # one rounding to nearest of the x87 long double


def _mp(x):
    return mpmath.mpf(float(x))


def _rel(got, want):
    return abs((mpmath.mpf(got) - want) / want) if want != 0 else abs(mpmath.mpf(got))


def _mp_ld(x):
    """A long double as an mpf, exactly: its mantissa as two doubles, its exponent beside it (a
    long double reaches far below the smallest double)."""
    m, ex = np.frexp(M.LD(x))
    hi = float(m)
    return mpmath.ldexp(mpmath.mpf(hi) + mpmath.mpf(float(m - M.LD(hi))), int(ex))


# ---- the reference ------------------------------------------------------------------------------
def test_reference_against_50_digits_on_the_named_inputs():
    """tau, flux and totals of the planted case (every plant of ff_maps_ref.PLANTS present):
    each voxel within a few long-double roundings of 50 digits, NaN and inf where they belong."""
    c = M.make_case(129, 2, 3)
    assert len(c["pix"]) == len(M.PLANTS)
    worst_t = worst_f = worst_s = 0.0
    for e in range(2):
        tau = M.tau_ref(c["ctau"], c["A"][e])
        flux = M.flux_ref(c["ctau"], c["cflux"], c["A"][e], c["tavg"])
        tot = M.ftot_ref(flux)
        for f in range(3):
            s = mpmath.mpf(0)
            for p in range(129):
                a, ta = c["A"][e, p], c["tavg"][p]
                if a != a:
                    assert np.isnan(tau[f, p]) and np.isnan(flux[f, p])
                    continue
                if np.isinf(a):
                    assert tau[f, p] == np.inf
                    want = _mp(c["cflux"][f]) * _mp(ta)
                else:
                    t = _mp(c["ctau"][f]) * _mp(a)
                    worst_t = max(worst_t, float(_rel(_mp_ld(tau[f, p]), t)))
                    want = _mp(c["cflux"][f]) * _mp(ta) * -mpmath.expm1(-t) if ta == ta else None
                if ta != ta:
                    assert np.isnan(flux[f, p])
                    continue
                if want < mpmath.mpf(2) ** -16000:         # below the long double's normal range
                    assert float(flux[f, p]) == 0.0 or abs(_mp_ld(flux[f, p]) - want) < 1e-4900
                else:
                    worst_f = max(worst_f, float(_rel(_mp_ld(flux[f, p]), want)))
                s += want
            worst_s = max(worst_s, float(_rel(_mp_ld(tot[f]), s)))
    print("reference against 50 digits: tau %.2e, flux %.2e, totals %.2e (long-double rounding "
          "%.2e)" % (worst_t, worst_f, worst_s, LD_EPS))
    assert worst_t <= LD_EPS                     # one product
    assert worst_f <= 6 * LD_EPS                 # tau, expm1l (1 ulp), two products
    assert worst_s <= 6 * LD_EPS                 # the sum itself adds nothing to its terms' error
    px = M.pixel_of(c, "A", 0.0)
    assert np.all(M.tau_ref(c["ctau"], c["A"][0])[:, px] == 0)
    assert np.all(M.flux_ref(c["ctau"], c["cflux"], c["A"][0], c["tavg"])[:, px] == 0)


def _om_grid():
    rng = np.random.default_rng(20251101)
    t = [np.exp(rng.uniform(np.log(1e-320), np.log(900.0), 6000)),
         np.exp(rng.uniform(np.log(1e-3), np.log(40.0), 6000)),     # where 1 - e^-t is neither t nor 1
         np.array([0.0, 1e-320, 1e-300, 1e-17, 1e-8, 799.9, 800.0, 800.1, 900.0])]
    for k in range(1, 1156):                      # every k the reduction can take: 800 log2 e = 1154.2
        edge = (k - 0.5) * M.LN2
        t.append(np.array([np.nextafter(edge, 0.0), edge, np.nextafter(edge, np.inf)]))
    return np.concatenate(t)


def test_restated_one_minus_exp_neg_against_50_digits():
    """The 4e-15 rjp_device.h states for one_minus_exp_neg, which the flux bound budgets: the
    restatement (FMAs as one rounding, and as two) over tau from 1e-320 to 900 with every k
    boundary of the reduction and its neighbours.  Above 800 the argument is clamped: 1 either
    way at 16 digits."""
    t = _om_grid()
    want = [-mpmath.expm1(-_mp(x)) for x in t]
    worst = {}
    for name, fma in (("one rounding", M.fma_dekker), ("two roundings", M.fma_two_roundings)):
        got = M.one_minus_exp_neg(t, fma=fma)
        rel = np.array([float(_rel(g, w)) for g, w in zip(got, want)])
        i = int(np.argmax(rel))
        worst[name] = rel[i]
        print("one_minus_exp_neg restated, FMA as %s: worst relative error %.3e at tau = %.17g"
              % (name, rel[i], t[i]))
    zero = M.one_minus_exp_neg(np.array([0.0]))[0]
    assert zero == 0.0 and not np.signbit(zero)                     # +0.0 at 0
    assert worst["one rounding"] <= 4e-15
    assert worst["two roundings"] <= 4e-15
    assert M.one_minus_exp_neg(np.array([np.inf]))[0] == 1.0
    assert M.one_minus_exp_neg(np.array([np.nan]))[0] == 1.0        # what K2 has to test for itself


# ---- the GPU cases are feasible -------------------------------------------------------------------
@pytest.mark.parametrize("k", M.GPU_CASES, ids=M.case_id)
def test_emulation_of_every_gpu_case_is_inside_the_bounds(k):
    c = M.make_case(k.npix, k.E, k.F)
    L = M.case_launch(k)
    tau, flux, ftot = M.emulate(c, L)
    r = M.judge(c, L, tau, flux, ftot)
    print("%s %s: emulation / bound %s" % (M.case_id(k), L, r))
    assert all(v <= 1.0 for v in r.values()), r
    assert np.isfinite(ftot).all()


def test_gpu_cases_reach_what_they_are_there_for():
    """Every kernel, both lane widths of each, the tails the issue names."""
    seen = set()
    for k in M.GPU_CASES:
        L = M.case_launch(k)
        seen.add((L.kernel, L.kp, L.vec))
        if k.misaligned:
            assert k.npix % 2 == 0 and L.vec == 1
    assert seen == {(kn, kp, v) for kn, kp in (("small", 1), ("acc", 1), ("acc", 4), ("ftot", 4))
                    for v in (1, 2)}
    ids = {M.case_id(k): M.case_launch(k) for k in M.GPU_CASES}
    assert ids["16384x1x100-all"].fchunk == 2 and ids["16385x1x100-all"].fchunk == 4
    assert ids["131074x1x17-ftot"].nparts == 260 > M.BLOCK
    # every plant sits in some small-kernel case, in every register-accumulator case and in the
    # larger totals-only ones
    for k in M.GPU_CASES:
        if k.npix > len(M.PLANTS):
            assert len(M.make_case(k.npix, k.E, k.F)["pix"]) == len(M.PLANTS)
    tiny = set()
    for k in M.GPU_CASES:
        if k.npix <= 3:
            tiny |= set(M.make_case(k.npix, k.E, k.F)["pix"])
    assert len(tiny) >= 12                       # the tiny maps between them plant half the values


# ---- the cases can tell ----------------------------------------------------------------------------
KP4 = M.Launch("acc", 2, 4, 2, 8, 16)            # the launch of (2050, 8, 1018), on fewer channels
KP1 = M.Launch("acc", 2, 1, 3, 12, 16)           # the launch of (1030, 6, 906)
PLANTED = [   # mistake, (npix, E, F), launch (None: what launch_rule says), what it must break
    ("float64 exp", (129, 1, 3), None, "flux"),
    ("LN2_LO dropped", (129, 1, 3), None, "flux"),
    ("NaN sum gives 1", (129, 1, 3), None, "flux"),
    ("NaN sum gives 1", (2050, 1, 17), "ftot", "ftot"),
    ("NaN sum gives 1", (2050, 1, 17), KP4, "ftot"),
    ("NaN pixel poisons the total", (129, 1, 3), None, "ftot"),
    ("NaN pixel poisons the total", (2050, 1, 17), "ftot", "ftot"),
    ("last pixel group dropped", (2050, 1, 17), KP4, "ftot"),
    ("last pixel group dropped", (2050, 1, 17), "ftot", "ftot"),
    ("dead lane counted", (2050, 1, 17), KP4, "ftot"),
    ("dead lane counted", (2050, 1, 17), "ftot", "ftot"),
    ("dead lane counted", (129, 1, 3), None, "ftot"),
    ("ragged channel slice", (1030, 2, 26), KP1, "ftot"),
    ("hoisted zeroing in a cube kernel", (129, 1, 3), None, "flux"),
]


def _launch_of(shape, launch):
    if launch == "ftot":
        return M.launch_rule(*shape, want_tau=False, want_flux=False)
    return launch or M.launch_rule(*shape)


@pytest.mark.parametrize("mistake,shape,launch,breaks", PLANTED,
                         ids=["%s-%s" % (m, l if isinstance(l, str) else ("kp%d" % l.kp if l else "small"))
                              for m, _, l, _ in PLANTED])
def test_planted_mistake_is_outside_the_bound(mistake, shape, launch, breaks):
    c = M.make_case(*shape)
    L = _launch_of(shape, launch)
    good = M.judge(c, L, *M.emulate(c, L))
    bad = M.judge(c, L, *M.emulate(c, L, mistake))
    print("%s on %s, %s: emulation / bound %s, with the mistake %s" % (mistake, shape, L, good, bad))
    assert all(v <= 1.0 for v in good.values())
    assert bad[breaks] > 1.0


def test_every_mistake_is_planted_somewhere():
    assert {m for m, _, _, _ in PLANTED} == set(M.MISTAKES)


def test_a_mistake_the_old_tolerances_let_through():
    """1 - exp(-tau) through float64 exp on optical depths between 3e-3 and 1e-2: the flux is off by
    up to 1.1e-16 / tau, inside the rtol = 1e-13 (flux) and 1e-12 (totals) that
    test_k2_per_lane_flux_accumulators_every_launch_shape and tests/test_gpu_k2_order.py hold K2
    to against float64 NumPy, and outside the bound."""
    c = M.make_case(1022, 1, 3, tau_range=(3e-3, 1e-2))
    L = M.launch_rule(1022, 1, 3)
    tau, flux, ftot = M.emulate(c, L, "float64 exp")
    want_tau = c["ctau"][None, :, None] * c["A"][:, None, :]
    want_flux = c["cflux"][None, :, None] * (c["tavg"][None, None, :] * -np.expm1(-want_tau))
    np.testing.assert_allclose(tau, want_tau, rtol=1e-14)
    np.testing.assert_allclose(flux, want_flux, rtol=1e-13)
    np.testing.assert_allclose(ftot, np.nansum(want_flux, axis=2), rtol=1e-12)
    bad = M.judge(c, L, tau, flux, ftot)
    good = M.judge(c, L, *M.emulate(c, L))
    print("float64 exp, tau in [3e-3, 1e-2]: passes rtol = 1e-13 / 1e-12; error / bound %s "
          "(without the mistake %s)" % (bad, good))
    assert bad["flux"] > 1.0 and all(v <= 1.0 for v in good.values())


def test_zeroing_a_nan_sum_in_the_totals_kernel_is_no_mistake():
    """ff_ftot_kernel may zero a NaN A beside the weight of its pixel: 1 - e^-0 is 0, the term is
    the same zero, the totals are the same bits.  (Carried into a kernel that writes the cubes the
    same zeroing IS a mistake: 'hoisted zeroing in a cube kernel' above.)"""
    c = M.make_case(2050, 3, 17)
    L = M.launch_rule(2050, 3, 17, want_tau=False, want_flux=False)
    a = M.emulate(c, L)[2]
    b = M.emulate(c, L, M.HARMLESS)[2]
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- the launch rule --------------------------------------------------------------------------------
HAND = [   # (npix, E, F), keywords -> (kernel, VEC, KP, blocks, nparts, fchunk), worked by hand
    ((1, 1, 1), {}, ("small", 1, 1, 1, 4, 1)),
    ((2, 1, 1), {}, ("small", 2, 1, 1, 4, 1)),
    ((2, 1, 1), dict(aligned=False), ("small", 1, 1, 1, 4, 1)),
    # 511 lanes, 2 workgroups, 2 * 3 * fsplit < 2048 until fsplit = 32 >= 17 channels
    ((1022, 3, 17), {}, ("small", 2, 1, 2, 8, 1)),
    ((1022, 3, 17), dict(want_ftot=False), ("small", 2, 1, 2, 0, 1)),
    ((1022, 3, 17), dict(aligned=False), ("small", 1, 1, 4, 16, 1)),
    # 8192 lanes, 32 workgroups, fsplit 64, ceil(100 / 64) = 2
    ((16384, 1, 100), {}, ("small", 2, 1, 32, 128, 2)),
    # 16385 scalar lanes, 65 workgroups, 65 * 32 = 2080 >= 2048, ceil(100 / 32) = 4
    ((16385, 1, 100), {}, ("small", 1, 1, 65, 260, 4)),
    # 515 lanes: 3 workgroups x 6 epochs x 57 slices = 1026 >= 1024; one group of four: 342
    ((1030, 6, 906), {}, ("acc", 2, 1, 3, 12, 16)),
    ((1030, 6, 906), dict(want_ftot=False), ("acc", 2, 1, 3, 0, 16)),
    ((1031, 6, 906), {}, ("acc", 1, 1, 5, 20, 16)),
    # 1025 lanes: 2 x 8 x 64 = 1024
    ((2050, 8, 1018), {}, ("acc", 2, 4, 2, 8, 16)),
    ((1025, 8, 1018), {}, ("acc", 1, 4, 2, 8, 16)),
    # one slice fewer: 2 x 8 x 63 = 1008 < 1024, 5 x 8 x 63 >= 1024
    ((2050, 8, 1008), {}, ("acc", 2, 1, 5, 20, 16)),
    # the two shapes of tests/test_gpu_k2_order.py: 32638 lanes, 32 x 2 x 16 = 1024
    ((65276, 2, 250), {}, ("acc", 2, 4, 32, 128, 16)),
    ((65277, 2, 250), {}, ("acc", 1, 4, 64, 256, 16)),
    ((65276, 1, 250), {}, ("acc", 2, 1, 128, 512, 16)),          # one epoch: 512 < 1024 <= 2048
    # totals only: 65537 lanes / 1024 -> 65 workgroups, 260 partials
    ((131074, 1, 17), dict(want_tau=False, want_flux=False), ("ftot", 2, 4, 65, 260, 16)),
    ((2047, 3, 33), dict(want_tau=False, want_flux=False), ("ftot", 1, 4, 2, 8, 16)),
    ((2050, 1, 17), dict(want_tau=False, want_flux=False, aligned=False), ("ftot", 1, 4, 3, 12, 16)),
    # one cube is enough to leave the totals-only kernel
    ((2050, 1, 17), dict(want_tau=False), ("small", 2, 1, 5, 20, 1)),
]


@pytest.mark.parametrize("shape,kw,want", HAND, ids=[str(s) + str(sorted(k)) for s, k, _ in HAND])
def test_launch_rule_against_hand_worked_shapes(shape, kw, want):
    assert tuple(M.launch_rule(*shape, **kw)) == want


def test_additions_per_launch_shape():
    """D of the header, shape by shape."""
    D = lambda shape, **kw: M.n_additions(M.launch_rule(*shape, **kw), shape[0])
    assert D((1022, 3, 17)) == 19 and D((1030, 6, 906)) == 19
    assert D((2050, 8, 1018)) == 25 and D((1025, 8, 1018)) == 21
    assert D((131074, 1, 17), want_tau=False, want_flux=False) == 26
    assert D((16385, 1, 100)) == 1 + 16 + 2
