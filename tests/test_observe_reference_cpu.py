"""tests/observe_ref.py -- the reference rjp_uv_tracks and rjp_vis_noise (K16) are held to on the GPU
(tests/test_gpu_observe.py) -- checked on the CPU: Philox4x32-10 against its known answers, the
uniforms, a float64 emulation of both kernels inside the bounds and nine planted mistakes outside
them, rigid facts of the tracks, the statistics of the reference's own sample; then the host layer
of rajepy_amd/engine.py (antenna lists, geodesy, the observing plan, the noise levels, the imaging
rule of the pipeline), check_uv_tracks / check_vis_noise from a plain C++ program, and the ABI."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from rajepy_amd import _lib
from rajepy_amd import engine as E
from tests import observe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "antenna_configs", "vla.a.cfg")
LD = np.longdouble


def worst(got, ref, bound):
    ok = np.isfinite(np.asarray(ref, dtype=np.float64)) & (np.broadcast_to(bound, np.shape(ref)) > 0)
    err = np.abs(np.asarray(got)[ok].astype(LD) - np.asarray(ref)[ok]).astype(np.float64)
    return float(np.max(err / np.broadcast_to(bound, np.shape(ref))[ok]))


# ---- Philox and the uniforms ---------------------------------------------------------------------------
def test_philox_known_answers_and_the_vectorisation():
    for counter, key, out in R.KNOWN_ANSWERS:
        assert R.philox_int(counter, key) == out
    rng = np.random.default_rng(1)
    c = rng.integers(0, 2 ** 32, (4, 500), dtype=np.uint64)
    c[:, 0], c[:, 1] = 0, R.MASK
    for key in ((0, 0), (R.MASK, R.MASK), (0x12345678, 0x9abcdef0)):
        x = R.philox_np(c[0], c[1], c[2], c[3], *key)
        for i in range(500):
            assert tuple(int(w[i]) for w in x) == R.philox_int(c[:, i], key)
    # the counter layout: (lo32(k), hi32(k), m, 0), key = (seed low, seed high)
    seed, k, m = (0xa4093822 | (0x299f31d0 << 32)), 0x243f6a88 | (0x85a308d3 << 32), 0x13198a2e
    c0, c1, c2, c3, k0, k1 = R.counter_words(seed, [k], [m])
    assert (int(c0[0]), int(c1[0]), int(c2[0]), int(c3[0]), k0, k1) == \
        (0x243f6a88, 0x85a308d3, 0x13198a2e, 0, 0xa4093822, 0x299f31d0)


def test_uniforms_are_exact_and_strictly_inside_the_unit_interval():
    for hi, lo, n in ((0, 0, 1), (R.MASK, R.MASK, 2 ** 53 - 1), (1, 0xfff, 2 ** 21 + 1), (0, 0x1000, 3)):
        assert R.unit_int(hi, lo) == n
        u = R.unit_ld([hi], [lo])[0]
        assert u == LD(n) * LD(2.0 ** -53) and float(u) == n * 2.0 ** -53      # exact in double too
        assert int(float(u) * 2.0 ** 53) == n and 0.0 < float(u) < 1.0
    assert float(R.unit_ld([0], [0])[0]) == 2.0 ** -53 and float(R.unit_ld([R.MASK], [R.MASK])[0]) == 1 - 2.0 ** -53
    # the planted 53-bit uniform reaches 1 at the all-one words: r = 0 where the contract has 1.5e-8
    bad = R.bad_unit_f64(np.array([R.MASK], dtype=np.uint64), np.array([R.MASK], dtype=np.uint64))[0]
    assert bad == 1.0
    r_ref = float(np.sqrt(LD(-2) * np.log(R.unit_ld([R.MASK], [R.MASK])[0])))
    r_bad = math.sqrt(-2.0 * math.log(bad))
    assert r_bad == 0.0 and abs(r_bad - r_ref) > 1e5 * r_ref * (R.C_N * R.U + R.SINCOS_TRUNC)


# ---- the float64 emulations inside, the planted mistakes outside ---------------------------------------
def _tracks_case():
    xyz, up = R.random_array(12, seed=4)
    gha = 0.299 + np.random.default_rng(5).uniform(-0.3, 0.3, 9) + np.arange(9) - 4
    dec, lat = np.radians(18.0), np.radians(34.0)
    return xyz, up, gha, dec, lat


def test_tracks_emulation_inside_and_planted_mistakes_outside():
    xyz, up, gha, dec, lat = _tracks_case()
    sd, cd = float(np.sin(dec)), float(np.cos(dec))
    ref = R.tracks_ref(xyz, gha, sd, cd)
    emu = R.tracks_ref(xyz, gha, sd, cd, dtype=np.float64)
    for c in "uvw":
        assert worst(emu[c], ref[c], ref["bound"][None, :]) <= 1.0, c
    mistakes = {"hour angle in radians": dict(radians=True), "opposite sign of G": dict(neg_g=True),
                "b = xyz_i - xyz_j": dict(reverse_b=True), "j-major pair order": dict(j_major=True)}
    for name, kw in mistakes.items():
        bad = R.tracks_ref(xyz, gha, sd, cd, dtype=np.float64, **kw)
        assert max(worst(bad[c], ref[c], ref["bound"][None, :]) for c in "uvw") > 1e6, name
    swapped = R.tracks_ref(xyz, gha, float(np.sin(lat)), float(np.cos(lat)), dtype=np.float64)
    assert max(worst(swapped[c], ref[c], ref["bound"][None, :]) for c in "vw") > 1e6, "dec swapped with lat"
    assert worst(swapped["u"], ref["u"], ref["bound"][None, :]) <= 1.0            # (u has no declination)


def test_noise_emulation_inside_and_planted_mistakes_outside():
    rng = np.random.default_rng(8)
    M, K = 3, 300
    V = rng.normal(0, 2, (M, K, 2))
    V[1, 7] = (-0.0, 0.0)
    sigma, s = [0.7, 0.0, 12.0], rng.uniform(0.5, 2.0, K)
    k0, m0 = 2 ** 32 - 100, 2
    ref, bound, copy_ = R.noise_ref(V, sigma, s, R.SEED, k0, m0)
    emu = R.noise_f64(V, sigma, s, R.SEED, k0, m0)
    assert worst(emu, ref, bound) <= 1.0
    assert np.array_equal(emu[1].view(np.int64), V[1].view(np.int64)) and list(copy_) == [False, True, False]
    for name, kw in {"no carry into the second word": dict(carry=False), "m and k swapped": dict(swap=True),
                     "sin / cos swapped": dict(swap_trig=True)}.items():
        bad = R.noise_f64(V, sigma, s, R.SEED, k0, m0, **kw)
        live = [0, 2]
        assert worst(bad[live], ref[live], bound[live]) > 1e6, name
    # without the carry the first 100 visibilities are still right: the mistake shows past 2^32 only
    head = R.noise_f64(V, sigma, s, R.SEED, k0, m0, carry=False)[:, :100]
    assert worst(head[[0, 2]], ref[[0, 2], :100], bound[[0, 2], :100]) <= 1.0
    # NaN and a non-finite scale
    V[0, 3, 0] = np.nan
    s[5] = np.inf
    ref = R.noise_ref(V, sigma, s, R.SEED)[0]
    assert np.isnan(ref[0, 3, 0]) and np.isfinite(ref[0, 3, 1]) and np.isnan(ref[:, 5]).all()


# ---- rigid facts of the tracks ----------------------------------------------------------------------------
def test_rigid_facts_of_the_tracks():
    xyz, up, gha, dec, lat = _tracks_case()
    sd, cd = float(np.sin(dec)), float(np.cos(dec))
    ref = R.tracks_ref(xyz, gha, sd, cd)
    i, j = R.pairs(12)
    b = (xyz[j] - xyz[i]).astype(LD)
    b2 = (b ** 2).sum(axis=1)
    # (sin_dec and cos_dec are float64: the sum of their squares is 1 to within 2 u, not 1e-19)
    assert np.max(np.abs(ref["u"] ** 2 + ref["v"] ** 2 + ref["w"] ** 2 - b2[None, :]) / b2) < 4 * R.U
    # (i, j) <-> (j, i) flips the sign
    rev = R.tracks_ref(xyz[::-1], gha, sd, cd)
    back = {(11 - a, 11 - c): n for n, (a, c) in enumerate(zip(*R.pairs(12)))}
    perm = [back[(c, a)] for a, c in zip(i, j)]
    for c in "uvw":
        assert np.array_equal(rev[c][:, perm], -ref[c])
    # circles at the pole
    g = np.linspace(0, 1, 33)
    pole = R.tracks_ref(xyz, g, 1.0, 0.0)
    rad = np.sqrt(b[:, 0] ** 2 + b[:, 1] ** 2)
    assert np.max(np.abs(np.sqrt(pole["u"] ** 2 + pole["v"] ** 2) - rad[None, :]) / rad) < 1e-17
    assert np.max(np.abs(pole["w"] - b[None, :, 2])) == 0
    # an east-west baseline (bz = 0): an ellipse of axis ratio |sin dec| centred on the origin
    ew = np.array([[6.0e6, 0.0, 1.0e6], [6.0e6 - 300.0, 4000.0, 1.0e6]])
    t = R.tracks_ref(ew, g, sd, cd)
    L2 = LD(300.0) ** 2 + LD(4000.0) ** 2
    assert np.max(np.abs(t["u"][:, 0] ** 2 + (t["v"][:, 0] / LD(sd)) ** 2 - L2)) / L2 < 1e-17
    assert abs(float(t["u"].sum() - t["u"][-1, 0])) < 1e-12 * 4000 * 32            # centred: a full turn sums to 0
    assert abs(float(t["v"].sum() - t["v"][-1, 0])) < 1e-12 * 4000 * 32
    # the elevation of the array centre at transit = 90 deg - |lat - dec|
    cfg = E.read_antenna_config(FIXTURE)
    geo = E.geodetic(cfg.xyz)
    for dec_deg in (-20.0, 18.13, 34.0, 60.0):
        d = np.radians(dec_deg)
        G = 2 * np.pi * (0.0 - geo.lon0_deg / 360.)                              # H = 0
        s_hat = np.array([np.cos(d) * np.cos(G), -np.cos(d) * np.sin(G), np.sin(d)])
        assert abs(np.degrees(np.arcsin(geo.up0 @ s_hat)) - (90. - abs(geo.lat0_deg - dec_deg))) < 1e-9


# ---- statistics of the reference's own sample ----------------------------------------------------------
def test_statistics_of_the_reference_sample_at_the_seed_of_the_gpu_tests():
    """2^20 normals of seed R.SEED = 20240516: maps 0 and 1, 2^18 visibilities, both parts.  Every
    condition is 5 sigma of its estimator under the hypothesis of independent N(0, 1) draws."""
    K = 2 ** 18
    _, g1, g2 = R.normals(R.SEED, np.arange(K)[None, :], np.array([0, 1])[:, None])
    g1, g2 = g1.astype(np.float64), g2.astype(np.float64)
    g = np.concatenate([g1.ravel(), g2.ravel()])
    N = g.size
    assert N == 2 ** 20
    assert abs(g.mean()) <= 5. / np.sqrt(N)
    assert abs(g.var() - 1.) <= 5. * np.sqrt(2. / N)
    n2 = g1.size
    assert abs(np.mean(g1 * g2)) <= 5. / np.sqrt(n2), "re / im"
    assert abs(np.mean(g1[:, :-1] * g1[:, 1:])) <= 5. / np.sqrt(n2 - 2), "lag 1 in k"
    assert abs(np.mean(g1[0] * g1[1])) <= 5. / np.sqrt(K), "between maps"
    assert abs(np.mean(g2[0] * g2[1])) <= 5. / np.sqrt(K), "between maps"
    gs = np.sort(g)
    cdf = 0.5 * (1. + np.array([math.erf(x) for x in gs / np.sqrt(2.)]))
    D = max(np.max(np.arange(1, N + 1) / N - cdf), np.max(cdf - np.arange(N) / N))
    assert D <= 1.95 / np.sqrt(N), D * np.sqrt(N)


def test_image_rms_formula_against_images_of_pure_noise():
    """The mean pixel variance over 200 seeds of a 9 x 9 direct-sum image of pure noise (NumPy, the
    reference's normals) against engine.image_rms, within 5 standard errors (from the scatter of
    the 200 per-seed means)."""
    rng = np.random.default_rng(12)
    K, n = 40, 9
    a, b = rng.uniform(-0.4, 0.4, K), rng.uniform(-0.4, 0.4, K)
    w = rng.uniform(0.2, 3.0, K)
    w[3] = 0.0                                                  # a flagged visibility
    sig = rng.uniform(0.5, 2.0, K)
    x = np.arange(n) - (n - 1) / 2.
    ph = np.exp(2j * np.pi * (a[:, None, None] * x[None, :, None] + b[:, None, None] * x[None, None, :]))
    per_seed = []
    for seed in range(200):
        _, g1, g2 = R.normals(1000 + seed, np.arange(K), np.zeros(K, dtype=np.uint64))
        noise = sig * (g1.astype(np.float64) + 1j * g2.astype(np.float64))
        img = np.real((w * noise)[:, None, None] * ph).sum(axis=0) / w.sum()
        per_seed.append(np.mean(img ** 2))
    per_seed = np.array(per_seed)
    want = E.image_rms(w, sig)
    assert want.shape == (1,) and want[0] == pytest.approx(np.sqrt((w ** 2 * sig ** 2).sum()) / w.sum(), rel=1e-15)
    se = per_seed.std(ddof=1) / np.sqrt(200.)
    assert abs(per_seed.mean() - want[0] ** 2) <= 5. * se, (per_seed.mean(), want[0] ** 2, se)
    assert se < 0.1 * want[0] ** 2, "the test can tell a wrong formula: sigma^2 / K is 30 % off"
    # per map, broadcasting, and a map without weights
    two = E.image_rms(np.stack([w, 2 * w]), np.array([[1.0], [3.0]]))
    assert two[1] == pytest.approx(3 * two[0], rel=1e-15) and np.isnan(E.image_rms(np.zeros(4), 1.0)[0])


# ---- antenna lists, geodesy, the plan, the noise level -------------------------------------------------
def test_read_antenna_config(tmp_path):
    cfg = E.read_antenna_config(FIXTURE)
    names, xyz = R.read_fixture(FIXTURE)
    assert cfg.observatory == "VLA" and cfg.names == names and len(names) == 27
    assert np.array_equal(cfg.xyz, xyz) and np.all(cfg.diameters == 25.0)
    assert cfg.names[0] == "W08" and cfg.xyz[0, 0] == -1601614.061201

    def write(text):
        p = tmp_path / "x.cfg"
        p.write_text(text)
        return str(p)
    head = "# observatory=TEST\n# coordsys=XYZ\n"
    ok = E.read_antenna_config(write(head + "\n1 2 3 12. A1\n4 5 6 12. A2  # trailing words\n"))
    assert ok.names == ["A1", "A2"] and ok.observatory == "TEST"
    for system in ("LOC (local tangent plane)", "UTM"):
        with pytest.raises(ValueError, match="coordsys=" + system.split()[0]):
            E.read_antenna_config(write("# observatory=ALMA\n# coordsys=%s\n1 2 3 12. A1\n4 5 6 12. A2\n" % system))
    for body, what in (("1 2 3 12.\n4 5 6 12. A2\n", "found 4 columns"), ("1 x 3 12. A1\n4 5 6 12. A2\n", "must be numbers"),
                       ("1 2 3 0. A1\n4 5 6 12. A2\n", "non-positive diameter"), ("1 2 inf 12. A1\n4 5 6 12. A2\n", "non-finite"),
                       ("1 2 3 12. A1\n", "fewer than two"), ("1 2 3 12. A1\n4 5 6 12. A1\n", "not unique")):
        with pytest.raises(ValueError, match=what):
            E.read_antenna_config(write(head + body))
    with pytest.raises(ValueError, match="no `# coordsys=`"):
        E.read_antenna_config(write("# observatory=TEST\n1 2 3 12. A1\n4 5 6 12. A2\n"))


def _heikkinen(x, y, z):
    """Geodetic latitude and longitude [deg] by Heikkinen's closed form (1982): no iteration."""
    a, f = 6378137.0, 1. / 298.257223563
    b = a * (1. - f)
    e2, ep2 = f * (2. - f), (a * a - b * b) / (b * b)
    r = math.hypot(x, y)
    F = 54. * b * b * z * z
    G = r * r + (1. - e2) * z * z - e2 * (a * a - b * b)
    c = e2 * e2 * F * r * r / G ** 3
    s = (1. + c + math.sqrt(c * c + 2. * c)) ** (1. / 3.)
    P = F / (3. * (s + 1. / s + 1.) ** 2 * G * G)
    Q = math.sqrt(1. + 2. * e2 * e2 * P)
    r0 = -P * e2 * r / (1. + Q) + math.sqrt(0.5 * a * a * (1. + 1. / Q) - P * (1. - e2) * z * z / (Q * (1. + Q)) -
                                             0.5 * P * r * r)
    V = math.sqrt((r - e2 * r0) ** 2 + (1. - e2) * z * z)
    z0 = b * b * z / (a * V)
    return math.degrees(math.atan((z + ep2 * z0) / r)), math.degrees(math.atan2(y, x))


def test_geodetic_against_a_closed_form():
    """The mean position of the fixture lies at 34.076648 N, 107.618358 W (Heikkinen's closed form,
    which `geodetic`'s fixed-point iteration does not share): inside the Very Large Array, whose
    nominal site is 34.0787 N, 107.6184 W.  Every antenna to 1e-6 deg (1e-9 in fact)."""
    cfg = E.read_antenna_config(FIXTURE)
    geo = E.geodetic(cfg.xyz)
    lat0, lon0 = _heikkinen(*cfg.xyz.mean(axis=0))
    assert abs(lat0 - 34.076648) < 1e-6 and abs(lon0 + 107.618358) < 1e-6
    assert abs(geo.lat0_deg - lat0) < 1e-9 and abs(geo.lon0_deg - lon0) < 1e-9
    assert abs(geo.lat0_deg - 34.0787) < 0.01 and abs(geo.lon0_deg + 107.6184) < 0.01
    for p, la, lo, up in zip(cfg.xyz, geo.lat_deg, geo.lon_deg, geo.up):
        want = _heikkinen(*p)
        assert abs(la - want[0]) < 1e-9 and abs(lo - want[1]) < 1e-9
        assert abs(np.linalg.norm(up) - 1.) < 1e-15 and up[2] == pytest.approx(math.sin(math.radians(la)), abs=1e-15)
    # the poles and the equator
    g = E.geodetic([[0., 0., 6356752.314245], [6378137., 0., 0.], [0., -6378137., 0.]])
    assert np.allclose(g.lat_deg, [90., 0., 0.], atol=1e-9) and np.allclose(g.lon_deg[1:], [0., -90.], atol=1e-12)


def test_observing_plan():
    # always up: dec 80 from lat 34 is 24 deg up at lower culmination
    ha, day = E.observing_plan(80., 34., 3600., 60., 20.)
    assert len(ha) == 60 and np.all(day == 0)
    assert np.allclose(ha, (np.arange(60) - 29.5) * 60. / 86164.0905, rtol=0, atol=1e-18)
    assert len(E.observing_plan(80., 34., 86400. * 2, 7200., 20.)[0]) == 24        # two days, no third of length 0
    # split over days: H = arccos((sin 20 - sin 34 sin -20) / (cos 34 cos 20)) = arccos(0.53327 / 0.77904) = 46.80 deg
    H = math.degrees(math.acos((math.sin(math.radians(20)) - math.sin(math.radians(34)) * math.sin(math.radians(-20))) /
                               (math.cos(math.radians(34)) * math.cos(math.radians(-20)))))
    time_up = int(7200. * H / 15.)
    assert time_up == 22464
    ha, day = E.observing_plan(-20., 34., 2.5 * time_up, 600., 20., hourangle_h=-1.5)
    n = time_up // 600
    assert list(np.bincount(day)) == [n, n, (time_up // 2) // 600] and n == 37
    for d in range(3):
        assert np.mean(ha[day == d]) == pytest.approx(-1.5 / 24., abs=1e-15)          # centred on the hour angle
    assert np.max(np.abs(ha[day == 0] + 1.5 / 24.)) * 86164.0905 <= time_up / 2.
    assert np.allclose(np.diff(ha[day == 0]), 600. / 86164.0905, rtol=1e-12)
    # never up: dec -50 culminates 6 deg above the horizon of lat 34
    with pytest.raises(ValueError, match="never reaches"):
        E.observing_plan(-50., 34., 3600., 60., 20.)
    # t_obs < t_int: one integration, at the hour angle
    ha, day = E.observing_plan(18., 34., 30., 60., 20., hourangle_h=2.0)
    assert list(ha) == [2.0 / 24.] and list(day) == [0]
    with pytest.raises(ValueError, match="positive"):
        E.observing_plan(18., 34., 0., 60., 20.)


def test_thermal_sigma():
    # SEFD 420 Jy, 2 MHz, 10 s, two polarisations: 420 / sqrt(2 * 2 * 2e6 * 10) = 46.957 mJy
    assert E.thermal_sigma(420., 2e6, 10.) == pytest.approx(420. / math.sqrt(8e7), rel=1e-15)
    assert E.thermal_sigma(420., 2e6, 10.) == pytest.approx(0.0469574, rel=1e-5)
    assert E.thermal_sigma(420., 2e6, 10., n_pol=1, efficiency=0.5) == pytest.approx(2. * 420. / math.sqrt(4e7), rel=1e-15)
    assert np.allclose(E.thermal_sigma(420., [1e6, 4e6], 10.), [420. / math.sqrt(4e7), 420. / math.sqrt(1.6e8)])
    assert E.thermal_sigma(0., 1e6, 1.) == 0.
    for bad in ((-1., 1e6, 1.), (1., 0., 1.), (1., 1e6, -2.), (float("nan"), 1e6, 1.)):
        with pytest.raises(ValueError):
            E.thermal_sigma(*bad)


def test_the_imaging_rule_on_hand_worked_numbers():
    """29979.2458 m at 10 GHz are 10^6 wavelengths: a beam of 1e-6 rad = 0.206264806 arcsec, a cell
    of 0.051566 arcsec; a model 10 arcsec across needs ceil(20 / 0.051566) = 388 cells -> 500; one
    20 arcsec across ceil(40 / 0.051566) = 776."""
    assert E.observation_grid(29979.2458, 1e10, 10.) == (0.051566, 500)
    assert E.observation_grid(29979.2458, 1e10, 20.) == (0.051566, 776)
    assert E.observation_grid(29979.2458, 2e10, 20.) == (0.025783, 1552)
    with pytest.raises(ValueError, match="rounds to 0"):
        E.observation_grid(1e9, 1e12, 1.)


def test_the_file_name_rule(tmp_path):
    for name in ("VLA.A.cfg", "alma_9.CFG", "MeerKAT.cfg", "vla.b.txt", "sma.0.cfg", "sma.cfg"):
        (tmp_path / name).write_text("")
    d = str(tmp_path)
    find = lambda t, c: os.path.basename(E.antenna_config_path(d, t, c) or "") or None
    assert find("vla", "a") == "VLA.A.cfg" and find("VLA", "A") == "VLA.A.cfg"
    assert find("ALMA", "9") == "alma_9.CFG"
    assert find("meerkat", "0") == "MeerKAT.cfg" and find("meerkat", "1") is None
    assert find("SMA", "0") == "sma.0.cfg"                       # the full name first
    assert find("vla", "b") is None and find("atca", "6a") is None
    assert E.antenna_config_path(str(tmp_path / "missing"), "vla", "a") is None
    assert os.path.basename(E.antenna_config_path(os.path.dirname(FIXTURE), "VLA", "A")) == "vla.a.cfg"


# ---- the argument checks from plain C++, the ABI --------------------------------------------------------
def test_check_uv_tracks_and_check_vis_noise_from_plain_cpp(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "rjp_args_observe_cases"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rajepy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rjp_args_observe_cases.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        case, status, msg = line.split("\t")
        got[case] = (int(status), msg)
    want_t = {"null": ["NULL h_xyz", "NULL h_gha", "NULL d_u", "NULL d_v", "NULL beats n_ant"],
              "n_ant": ["n_ant 1", "n_ant -3", "n_ant beats n_t"], "n_t": ["n_t 0", "n_t beats xyz"],
              "xyz": ["xyz nan", "xyz inf", "xyz beats the declination"],
              "dec": ["sin_dec nan", "cos_dec inf", "non-finite beats the circle"],
              "unit": ["off the circle", "zero vector"], "size": ["2^32 outputs", "3 x 715827883 outputs"]}
    want_n = {"null": ["NULL d_vis", "NULL h_sigma", "NULL d_out", "NULL beats sizes"],
              "sizes": ["n_maps 0", "n_vis -1", "sizes beat sigma"],
              "sigma": ["sigma negative", "sigma nan", "sigma inf", "sigma beats k0"],
              "k0": ["k0 -1", "k0 + n_vis 2^63", "k0 beats m0"], "m0": ["m0 -1", "m0 + n_maps 2^31"]}
    seen = set()
    for prefix, want, msgs in (("tracks ", want_t, R.TRACKS_MESSAGES), ("noise ", want_n, R.NOISE_MESSAGES)):
        for key, cases in want.items():
            for case in cases:
                assert got[prefix + case] == (_lib.RJP_ERR_ARG, msgs[key]), case
                seen.add(prefix + case)
    valid = {c for c in got if " valid" in c}
    assert len(valid) == 8 and all(got[c] == (0, "") for c in valid)
    assert seen | valid == set(got)


def test_abi_prototypes():
    P, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    DP = ctypes.POINTER(ctypes.c_double)
    res, args = _lib.SIGNATURES["rjp_uv_tracks"]
    assert res is i64 and args == [P, DP, i32, DP, i32, dbl, dbl, DP, dbl, P, P, P, P]
    res, args = _lib.SIGNATURES["rjp_vis_noise"]
    assert res is i64 and args == [P, P, i32, i32, DP, P, ctypes.c_uint64, i64, i32, P, P]
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    assert "int64_t rjp_uv_tracks(rjp_ctx* ctx, const double* h_xyz, int32_t n_ant, const double* h_gha," in hdr
    assert "int64_t rjp_vis_noise(rjp_ctx* ctx, const double* d_vis, int32_t n_maps, int32_t n_vis," in hdr
    for words in ("counter = (low 32 bits of k0 + k, high 32 bits of k0 + k, m0 + m, 0)", "up_i . s(t) < sin_min_el",
                  "classes.py:2490-2650", "i-major order"):
        assert words in hdr, words
    assert _lib.RJP_VERSION == 117
    lib = _lib.load()
    # a NULL context is refused before anything else
    assert lib.rjp_uv_tracks(None, None, 0, None, 0, 0., 1., None, 0., None, None, None, None) == _lib.RJP_ERR_ARG
    assert lib.rjp_vis_noise(None, None, 0, 0, None, None, 0, 0, 0, None, None) == _lib.RJP_ERR_ARG


def test_execute_and_main_take_the_new_keywords():
    import inspect
    from rajepy_amd import classes, main
    p = inspect.signature(classes.Pipeline.execute).parameters
    assert list(p)[-3:] == ["antenna_configs", "sefd_jy", "seed"]
    assert p["antenna_configs"].default is None and p["sefd_jy"].default is None and p["seed"].default == 0
    q = inspect.signature(classes.JetModel.observe_ff).parameters
    assert list(q)[1:5] == ["antennalist", "freq", "t_obs_s", "t_int_s"]
    assert [q[k].default for k in ("sigma_jy", "sefd_jy", "chanwidth_hz", "seed", "nsigma")] == [None, None, None, 0, 0.]
    assert set(inspect.signature(classes.JetModel.clean_image_ff).parameters) - {"u_m", "v_m"} <= set(q)
    assert list(inspect.signature(classes.JetModel.uv_tracks).parameters)[1:] == \
        ["antennalist", "t_obs_s", "t_int_s", "min_el_deg", "hourangle_h"]
    assert classes.UVTracks._fields == ("u_m", "v_m", "w_m", "ha_h", "day", "ant1", "ant2", "max_baseline_m")
    assert classes.Observation._fields == ("tracks", "vis_clean", "vis", "sigma", "image_rms", "clean")
    with pytest.raises(SystemExit):
        main.main(["--help"])
