"""What tests/test_gpu_k3_evaluations.py stands on, checked without a device:

* scipy.special.wofz -- the Re w of tests/k3_voigt_ref.line_term_ref -- against the 40-digit fixture
  tests/golden/k3_voigt.npz, and the fixture against its own generator;
* line_term_ref, summed along y, against the oracle's optical_depth_rrl on two golden models;
* k3_voigt_ref.path_codes on hand-made cells: every path code and both states of the exp flag;
* tools/voigt_design.py, run: the worst error of every Voigt path it restates is within the figure
  the accuracy budget at the head of rajepy_amd/csrc/rrl_scan.hip states for it;
* the GPU cases themselves, built on the host: the reference drops fewer than 1 % of a case's
  evaluations, and every path code is reached by at least 1000 of them.
"""
import importlib.util
import os
import re

import numpy as np
import pytest
from scipy.special import wofz

from tests import gpu_util as U
from tests import k3_voigt_ref as R
from rajepy_amd.maths import rrls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = rrls.line_constants("H66a")


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the fixture ----------------------------------------------------------------------------------
def test_wofz_agrees_with_the_40_digit_fixture_everywhere():
    """1e-12 relative at every point of the fixture: line_term_ref may take Re w from wofz over the
    whole domain of the GPU tests (y from 1e-10 to 1e3, x from 0 to 1e4, on and beside the lattice
    nodes).  Measured: 2.5e-14."""
    x, y, rew = R.load_fixture()
    assert x.size * y.size <= 6000 and rew.shape == (y.size, x.size)
    assert os.path.getsize(R.GOLDEN) <= os.path.getsize(os.path.join(U.GOLDEN, "k4_times.npz"))
    assert np.isfinite(rew).all() and (rew > 0).all()
    got = wofz(x[None, :] + 1j * y[:, None]).real
    rel = np.abs(got - rew) / rew
    print("wofz against the fixture: worst %.2e" % rel.max())
    assert rel.max() <= 1e-12


def test_fixture_comes_out_of_its_generator():
    """The committed axes are the generator's, and a sample of its points (every 23rd, which walks
    through all rows and columns) comes out of mpmath bit for bit."""
    pytest.importorskip("mpmath")
    gen = _load(os.path.join(U.GOLDEN, "make_k3_voigt_golden.py"), "make_k3_voigt_golden")
    x, y, rew = R.load_fixture()
    gx, gy = gen.grid()
    assert np.array_equal(gx, x) and np.array_equal(gy, y)
    for k in range(0, rew.size, 23):
        iy, ix = divmod(k, x.size)
        assert gen.rew_mp(x[ix], y[iy]) == rew[iy, ix], (x[ix], y[iy])
    # the set the issue asks for
    for t in (0.03, 1.0, 1.3, np.pi / 0.675, np.pi / 0.6, 8.0):
        assert np.any(np.isclose(y, t * 0.995)) and np.any(np.isclose(y, t * 1.005))
    assert y.min() == 1e-10 and np.isclose(y.max(), 1e3)
    for h in (0.6, 0.675):
        for n in (0, 1, 5, 11):
            for d in (0.0, 0.25 * h, 1e-6):
                assert np.any(np.isclose(x, n * h + d, rtol=0, atol=1e-12))
    for v in (8.0, 14.0, 16.0, 40.0, 1e3, 1e4):
        assert v in x


# ---- line_term_ref against the oracle -----------------------------------------------------------------
@pytest.mark.parametrize("tag", ["cfg1_example", "tilted"])
def test_line_term_ref_summed_along_y_is_the_oracles_optical_depth(tag):
    """nansum over y of line_term_ref = OracleJet.optical_depth_rrl on the golden model's fields and
    channels, to 1e-12 of the map value plus what the oracle's own float64 x costs it (`tol` with
    bound 1e-12, summed over the sightline's terms: the oracle forms nu - nu0 in float64)."""
    z, meta, p, g, jet = U.golden_dense(tag)
    from oracle import rt_oracle as orc
    jet.time = float(z["years"][0]) * orc.YEAR
    rrl = meta["rrl"]
    nus = np.asarray(z["rrl_freqs"], dtype=np.float64)
    nus = nus[np.unique(np.linspace(0, nus.size - 1, 7).astype(int))]     # (seconds, not half a minute)
    line = rrls.line_constants(rrl)
    # (only the cells inside the jet go through the longdouble reference: x87 arithmetic on the NaN
    # of the cells outside is slow, and nansum drops them anyway)
    nd = np.where(g["rr"] < 0, -1.0, 1.0) * jet.number_density
    live = np.isfinite(nd) & np.isfinite(g["temp"])
    fields = dict(nd=nd[live], xi=g["xi"][live], temp=g["temp"][live],
                  pf=(g["ff"] / g["areas"])[live], vy=g["vy"][live], csize_au=jet.csize)
    ref = R.line_term_ref(fields, line, nus)
    with np.errstate(all="ignore"):
        want = jet.optical_depth_rrl(rrl, nus)
        dead = jet.optical_depth_rrl(rrl, nus, collapse=False)[:, ~live]
    assert not np.any(np.isfinite(dead) & (dead != 0))       # nothing outside `live` counts
    t = R.tol(1e-12, ref["x"], ref["y"], ref["rew"], ref["imw"], ref["nu0_is2"])
    term = np.zeros((nus.size,) + nd.shape)
    allow = np.zeros((nus.size,) + nd.shape)
    term[:, live] = np.where(np.isfinite(ref["term"]), ref["term"], 0.0)
    allow[:, live] = np.where(np.isfinite(ref["term"]), t * ref["term"], 0.0)
    got, allowed = term.sum(axis=2), allow.sum(axis=2)
    assert np.array_equal(got == 0, want == 0)
    ok = want != 0
    assert ok.any()
    err = np.abs(got - want)
    print("%s: worst |sum - oracle| / oracle = %.2e, worst error / allowed = %.3f"
          % (tag, (err[ok] / want[ok]).max(), (err[ok] / allowed[ok]).max()))
    assert np.all(err[ok] <= allowed[ok])


# ---- path_codes ------------------------------------------------------------------------------------
def _cells(y, temp=1e4):
    g = R.host_fields(np.asarray(y, dtype=np.float64).reshape(1, 1, -1), temp, LINE)
    return R.cell_consts(R.as_device_fields(g), LINE)


def test_lane_fold_and_layouts():
    assert [R.lanes_per_block(n) for n in (1, 16, 17, 64, 128, 129, 256, 300)] == \
        [16, 16, 64, 64, 64, 256, 256, 256]
    runs = R.wave_runs(256)
    assert len(runs) == 4
    assert list(runs[0][0][:3]) == [0, 1, 2] and list(runs[0][1][:3]) == [255, 254, 253]
    assert list(runs[3][0][[0, -1]]) == [96, 127] and list(runs[3][1][[0, -1]]) == [159, 128]
    runs = R.wave_runs(129)                        # one block, 129 live lanes: the third wave holds one
    assert [(e.size, o.size) for e, o in runs] == [(32, 32), (32, 32), (1, 0)]
    assert runs[2][0][0] == 64
    runs = R.wave_runs(65)                         # two blocks of the 64-lane layout
    assert [(e.size, o.size) for e, o in runs] == [(32, 32), (1, 0)] and runs[1][0][0] == 64
    for n in (17, 64, 65, 128, 129, 256, 300, 513):
        seen = np.concatenate([np.concatenate(r) for r in R.wave_runs(n)])
        assert sorted(seen) == list(range(n))


def test_path_codes_on_hand_made_cells_reach_every_code():
    nu_c, sig2 = R.line_centre(LINE, 1e4)
    ys = np.array([1e-3, 0.5, 2.0, 5.0, 9.0])      # centred | pole | lite pole | no pole term | y > 8
    cells = _cells(ys)
    code = lambda kind, n=256: R.path_codes(cells, R.wave_channels(kind, n, nu_c, sig2), n)[:, 0, 0, :]
    c = code("core")                               # waves at |x| in 0-1.5, 1.5-3, 3-4.5, 4.5-6
    w0, w3 = 0, 96                                 # a channel of the first wave, one of the fourth
    assert list(c[w0]) == [R.CENTRED, R.PLAIN_POLE, R.PLAIN_POLE_LITE, R.PLAIN, R.FAR_A]
    # the pole-term cut: cq ~ 21 - ln y ...: at 4.5 <= |x| the y = 2 cell needs no pole term
    assert list(c[w3]) == [R.CENTRED, R.PLAIN_POLE, R.PLAIN, R.PLAIN, R.FAR_A]
    c = code("switch")                             # 8.001-8.16 | 7.84-7.999 | 14.001-14.28 | 13.72-13.999
    assert list(c[0]) == [R.FAR_A] * 5 and list(c[32]) == [R.CENTRED, R.PLAIN, R.FAR_A, R.FAR_A, R.FAR_A]
    assert list(c[64]) == [R.FAR_B] * 5 and list(c[96]) == [R.FAR_A] * 3 + [R.FAR_B] * 2
    c = code("outlier")
    # (a band out to |x| = 2e6 is too wide for the first-order stimulated-emission factor: flag set)
    assert np.all(c & R.EXP_FLAG) and not np.any(code("core") & R.EXP_FLAG)
    c = c & 7
    assert list(c[w0]) == [R.GENERIC] * 4 + [R.FAR_A] and list(c[w3]) == list(code("core")[w3])
    # the 64-lane layout decides per block of 64 channels, the 16-lane layout has no codes
    c = code("core", 128)
    assert list(c[0]) == [R.CENTRED, R.PLAIN_POLE, R.PLAIN_POLE_LITE, R.PLAIN, R.FAR_A]
    assert list(c[64]) == [R.CENTRED, R.PLAIN_POLE, R.PLAIN_POLE_LITE, R.PLAIN, R.FAR_A]
    assert np.all(R.path_codes(cells, R.x_channels(R.X16, nu_c, sig2), 16) == R.GENERIC)
    # irregular cells: an infinite density runs the generic code, a NaN or empty one is skipped
    g = R.host_fields(np.full((1, 1, 3), 0.5), 1e4, LINE)
    g["nd"][0, 0, 0], g["nd"][0, 0, 1], g["xi"][0, 0, 2] = np.inf, np.nan, 0.0
    bad = R.cell_consts(R.as_device_fields(g), LINE)
    c = R.path_codes(bad, R.wave_channels("core", 256, nu_c, sig2), 256)[0, 0, 0]
    assert list(c) == [R.GENERIC, R.SKIP, R.SKIP]


def test_path_codes_exp_flag_at_its_threshold():
    """The band-expansion case: the quotient of band_needs_exp is 0.9 / 1.1 for the 300 K cells (the
    half-width is about 23.7 MHz at 1.0), far below 1 for the 1e4 K cells."""
    y, temp = R.band_cells()
    cells = R.cell_consts(R.as_device_fields(R.host_fields(y, temp, LINE)), LINE)
    cold = temp == R.BAND_TEMPS[0]
    nu_c, _ = R.line_centre(LINE, R.BAND_TEMPS[0])
    assert 23.0e6 < R.band_halfwidth(LINE, 300.0, nu_c, 1.0) < 24.5e6
    for ratio, want in ((0.9, False), (1.1, True)):
        nu, dnu = R.band_channels(LINE, ratio)
        _, quot = R.band_needs_exp(cells["a"], 0.5 * (nu.min() + nu.max()), 0.5 * (nu.max() - nu.min()))
        assert np.allclose(quot[cold], ratio, rtol=1e-6) and np.all(quot[~cold] < 0.05)
        c = R.path_codes(cells, nu, 256)
        assert np.all(((c[:, cold] & R.EXP_FLAG) != 0) == want)
        assert not np.any(c[:, ~cold] & R.EXP_FLAG)
        assert np.all((c & 7) != R.SKIP)


# ---- the design figures --------------------------------------------------------------------------------
# path -> the figure of the accuracy budget at the head of rrl_scan.hip, as written there
DESIGN = {"plain": "3.5e-9", "far6": "4.1e-9", "far4": "1.2e-9", "plain_skip": "1.5e-9",
          "centred": "7.2e-10", "centred_skip": "2.9e-9", "generic_core": "1.3e-11",
          "generic_far": "3e-10"}


def test_design_tool_figures_are_within_the_header_of_rrl_scan():
    """tools/voigt_design.py restates every path in NumPy with the kernel's constants and operation
    structure; its worst errors against wofz must not exceed what the header of rrl_scan.hip states,
    and the header must state these figures."""
    src = open(os.path.join(ROOT, "rajepy_amd", "csrc", "rrl_scan.hip")).read()
    head = src[:src.index('#include "rrl_voigt.h"')]
    for pat in (r"\(3\.5e-9,", r"\(4\.1e-9 / 1\.2e-9\)", r"<= 1\.5e-9 on the plain lattice",
                r"<= 2\.9e-9 on the centred one", r"\(7\.2e-10 with its pole term\)", r"core 1\.3e-11",
                r"continued fraction 3e-10"):
        assert re.search(pat, head), pat
    tool = _load(os.path.join(ROOT, "tools", "voigt_design.py"), "voigt_design")
    m = tool.measure()
    assert set(m) == set(DESIGN)
    for name, fig in DESIGN.items():
        print("%-13s %.3e at x = %.6g, y = %.6g   (header: %s)"
              % (name, m[name][0], m[name][1][0], m[name][1][1], fig))
    for name, fig in DESIGN.items():
        assert m[name][0] <= float(fig), (name, m[name], fig)
    # every wave-uniform path is inside the bound the GPU tests hold it to, the generic code inside its own
    assert max(m[k][0] for k in ("plain", "plain_skip", "far6", "far4", "centred",
                                 "centred_skip")) < U.K3_RTOL_WAVE
    assert max(m["generic_core"][0], m["generic_far"][0]) < U.K3_RTOL_LANE
    # the tool's constants are the kernel's
    hdr = open(os.path.join(ROOT, "rajepy_amd", "csrc", "rrl_voigt.h")).read()
    assert "constexpr double kHW = %r;" % tool.H in hdr and "constexpr int kNPairW = %d;" % tool.NPAIR in hdr
    assert "constexpr double kPoleLiteY = %r;" % tool.POLE_LITE_Y in hdr
    assert "constexpr double kH = %r;" % tool.H_GEN in hdr and "constexpr int kNPair = %d;" % tool.NPAIR_GEN in hdr
    assert (R.H_WAVE, R.POLE_LITE_Y, R.CEN_YMAX) == (tool.H, tool.POLE_LITE_Y, tool.CEN_YMAX)


# ---- the GPU cases, on the host ------------------------------------------------------------------------
@pytest.mark.parametrize("temp", R.WAVE_TEMPS)
def test_wave_cases_drop_under_one_percent_and_reach_every_path(temp):
    """Per temperature (one GPU test each): the reference keeps more than 99 % of every case's
    evaluations, and over the test's cases every path code 1-7 holds at least 1000 evaluations."""
    nu_c, sig2 = R.line_centre(LINE, temp)
    g = R.host_fields(R.wave_cells_y(), temp, LINE)
    g["nd"][3, 0, 17] = np.inf                     # the cell with an infinite field
    fields = R.as_device_fields(g)
    cells = R.cell_consts(fields, LINE)
    count = np.zeros(8, dtype=np.int64)
    for kind in R.WAVE_KINDS:
        for nchan in R.WAVE_NCHAN:
            nu = R.wave_channels(kind, nchan, nu_c, sig2)
            term = R.line_term_ref(fields, LINE, nu)["term"]
            keep = np.isfinite(term) & (term != 0)
            assert (~keep).sum() < 0.01 * keep.size, (kind, nchan)
            codes = R.path_codes(cells, nu, nchan)
            count += np.bincount((codes & 7)[keep], minlength=8)
    print("evaluations per path code at %g K: %r" % (temp, count.tolist()))
    assert np.all(count[1:] >= 1000), count


def test_lane_and_band_cases_drop_under_one_percent():
    for temp in (1e3, 2e4):
        nu_c, sig2 = R.line_centre(LINE, temp)
        y = R.lane_cells_y()
        assert np.all((y.ravel()[0::2] < R.CEN_YMAX) & (y.ravel()[1::2] > 1.0))
        fields = R.as_device_fields(R.host_fields(y, temp, LINE))
        for xs in (R.X1, R.X5, R.X16, R.X40):
            term = R.line_term_ref(fields, LINE, R.x_channels(xs, nu_c, sig2))["term"]
            assert np.all(np.isfinite(term) & (term > 0))
    y, temp = R.band_cells()
    fields = R.as_device_fields(R.host_fields(y, temp, LINE))
    for ratio in (0.9, 1.1):
        term = R.line_term_ref(fields, LINE, R.band_channels(LINE, ratio)[0])["term"]
        assert np.all(np.isfinite(term) & (term > 0))
