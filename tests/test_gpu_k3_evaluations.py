"""K3 (rjp_rrl_scan, rjp_rrl_cells) held to the reference ONE EVALUATION AT A TIME.

Every grid here has n_y = 1 (except the tile-map test): a "sightline sum" is then the single term
kappa_L * path of one cell and one channel, and the reference is tests/k3_voigt_ref.line_term_ref of
that cell -- longdouble arithmetic around scipy.special.wofz, itself held to a 40-digit fixture by
tests/test_k3_voigt_reference_cpu.py.  The allowed error of a term is k3_voigt_ref.tol: the bound
the project states for the code under test (gpu_util.K3_RTOL_WAVE = 1e-8 for the wave-uniform paths,
K3_RTOL_LANE = 1e-9 for the per-lane code) plus the derived conditioning of Re w in x.  The inputs of
the reference are read back from the device tensors of the uploaded fields, so neither packing nor
f32 rounding is under test.

Which of the seven Faddeeva paths of rrl_voigt.h an evaluation takes is restated on the host
(k3_voigt_ref.path_codes); the tests assert that every path is reached by >= 1000 evaluations and
print the worst relative error per path (DESIGN.md section 3 quotes the table).  Measured on an
MI355X: 4.05e-9 (6-term series), 1.14e-9 (4-term series), 3.43e-9 / 2.43e-9 / 3.00e-9 (plain lattice
without / with / with the lite pole term), 2.67e-9 (centred lattice, where its pole term is cut),
1.5e-11 (generic code), 1.1e-10 (per-lane code in its far field).
"""
import copy

import numpy as np
import pytest

from tests import gpu_util as U
from tests import k3_voigt_ref as R

pytestmark = pytest.mark.gpu
YEAR = 31536000.0
WORST_WAVE, WORST_LANE = {}, {}


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def line():
    from rajepy_amd import _lib
    from rajepy_amd.maths import rrls
    lc = rrls.line_constants("H66a")
    return lc, _lib.Line(**lc)


def _upload(eng, g, dtype=8):
    return eng.upload_fields(g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"], g["rr"] < 0,
                             vy=g["vy"], csize_au=R.CSIZE_AU, dtype=dtype)


def _read_back(fields, shape, bursts=None):
    """The reference's inputs: the device tensors of the uploaded fields, as float64."""
    rd = lambda t: t.cpu().numpy().astype(np.float64).reshape(shape)
    d = dict(nd=rd(fields.nd), xi=rd(fields.xi), temp=rd(fields.temp), pf=rd(fields.pf),
             vy=rd(fields.vy), ts=rd(fields.ts), csize_au=fields.csize_au)
    if bursts is not None:
        d["bursts"] = bursts
    return d


def _bursts(with_bursts):
    """(host lists, rjp_bursts, epoch): the example's bursts seen 40 years on (chi = 1), or none."""
    if not with_bursts:
        return None, None, 0.0
    from rajepy_amd.engine import make_bursts
    lists = U.example_burst_lists()
    return lists, make_bursts(*lists), 40.0 * YEAR


def _scan(eng, fields, dev_bursts, t, line_dev, nu, shape):
    tau = eng.rrl_scan(fields, dev_bursts, t, line_dev, list(nu))
    eng.synchronize()
    return tau.cpu().numpy().reshape((len(nu),) + shape)          # n_y = 1: [F, nx, 1, nz]


# ---- wave-uniform paths: the 256- and the 64-lane layout -------------------------------------------
@pytest.mark.parametrize("temp,with_bursts", [(1e3, False), (1e4, False), (2e4, False), (1e4, True)])
def test_wave_paths_one_evaluation_at_a_time(eng, line, temp, with_bursts):
    """512 cells whose Voigt y runs over the fixture's y set (1e-10 .. 1e3 and +-0.5 % around every y
    threshold of the paths), one of them with an infinite density; channel lists of 256, 64, 65, 128
    and 129 channels whose waves sit on the core (|x| <= 6, both wings), just inside and outside
    |x| = 8 and 14, across 8, 14 and 16, in the wings up to |x| = 1e3, and beside one channel at
    |x| = 2e6 (generic code).  Every evaluation against line_term_ref at K3_RTOL_WAVE."""
    lc, line_dev = line
    shape = R.WAVE_SHAPE
    nu_c, sig2 = R.line_centre(lc, temp)
    g = R.host_fields(R.wave_cells_y(), temp, lc,
                      ts=np.random.default_rng(5).uniform(0.0, 5.0 * YEAR, shape))
    g["nd"][3, 0, 17] = np.inf
    lists, dev_bursts, t = _bursts(with_bursts)
    fields = _upload(eng, g)
    dev = _read_back(fields, shape, lists)
    cells = R.cell_consts(dev, lc, t)
    mine, count = {}, np.zeros(8, dtype=np.int64)
    for kind in R.WAVE_KINDS:
        for nchan in R.WAVE_NCHAN:
            nu = R.wave_channels(kind, nchan, nu_c, sig2)
            got = _scan(eng, fields, dev_bursts, t, line_dev, nu, shape)
            ref = R.line_term_ref(dev, lc, nu, t)
            codes = R.path_codes(cells, nu, nchan)
            with np.errstate(all="ignore"):
                relp = np.abs(got - ref["term"]) / ref["term"]
            keepp = np.isfinite(ref["term"]) & (ref["term"] != 0)
            R.worst_by_path(relp, keepp, codes, mine)               # (printed even if it fails below)
            print("%-8s %3d channels: worst %.2e" % (kind, nchan, np.max(relp[keepp])))
            rel, keep = R.check_terms(got, ref, U.K3_RTOL_WAVE)
            count += np.bincount((codes & 7)[keep], minlength=8)
    print("T = %g K%s\n%s" % (temp, ", bursts long past" if with_bursts else "", R.path_table(mine)))
    for c, (w, n) in mine.items():
        w0, n0 = WORST_WAVE.get(c, (0.0, 0))
        WORST_WAVE[c] = (max(w, w0), n + n0)
    print("all cases so far\n" + R.path_table(WORST_WAVE))
    assert np.all(count[1:] >= 1000), count.tolist()


# ---- the per-lane code ---------------------------------------------------------------------------------
@pytest.mark.parametrize("temp", [1e3, 2e4])
def test_per_lane_code_one_evaluation_at_a_time(eng, line, temp):
    """The 16-lane layout (1, 5 and 16 channels) and rjp_rrl_cells (40 channels) on cells that
    alternate between y < 0.03 and y > 1: one wave holds lanes that are far-field and lanes that are
    not, lanes on the shifted lattice and lanes on the plain one.  At K3_RTOL_LANE."""
    lc, line_dev = line
    shape = R.WAVE_SHAPE
    nu_c, sig2 = R.line_centre(lc, temp)
    fields = _upload(eng, R.host_fields(R.lane_cells_y(), temp, lc))
    dev = _read_back(fields, shape)
    for xs in (R.X1, R.X5, R.X16):
        nu = R.x_channels(xs, nu_c, sig2)
        got = _scan(eng, fields, None, 0.0, line_dev, nu, shape)
        ref = R.line_term_ref(dev, lc, nu)
        rel, keep = R.check_terms(got, ref, U.K3_RTOL_LANE)
        assert keep.all()
        R.worst_by_path(rel, keep, np.full(rel.shape, R.GENERIC), WORST_LANE)
        print("rrl_scan, %2d channels: worst %.2e" % (len(xs), rel.max()))
    nu = R.x_channels(R.X40, nu_c, sig2)
    out = eng.rrl_cells(fields, None, 0.0, line_dev, list(nu))
    eng.synchronize()
    got = out.cpu().numpy().reshape((len(nu),) + shape)
    rel, keep = R.check_terms(got, R.line_term_ref(dev, lc, nu), U.K3_RTOL_LANE)
    assert keep.all()
    R.worst_by_path(rel, keep, np.full(rel.shape, R.GENERIC), WORST_LANE)
    print("rrl_cells, 40 channels: worst %.2e" % rel.max())
    print("per-lane code so far\n" + R.path_table(WORST_LANE))


# ---- f32 storage -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchan,kind", [(16, None), (64, "core"), (256, "switch"), (256, "core")])
def test_f32_storage_one_evaluation_at_a_time(eng, line, nchan, kind):
    """One case of each layout on fields stored in f32: the reference reads the f32 values back, so
    the bounds are those of f64 storage."""
    lc, line_dev = line
    shape, temp = R.WAVE_SHAPE, 1e4
    nu_c, sig2 = R.line_centre(lc, temp)
    fields = _upload(eng, R.host_fields(R.wave_cells_y(), temp, lc), dtype=4)
    assert fields.nd.element_size() == 4
    dev = _read_back(fields, shape)
    nu = R.x_channels(R.X16, nu_c, sig2) if kind is None else R.wave_channels(kind, nchan, nu_c, sig2)
    got = _scan(eng, fields, None, 0.0, line_dev, nu, shape)
    rel, keep = R.check_terms(got, R.line_term_ref(dev, lc, nu), U.k3_rtol(nchan))
    assert keep.all()
    print("f32 storage, %d channels (%s): worst %.2e" % (nchan, kind, rel.max()))


# ---- the first-order stimulated-emission factor at its threshold ---------------------------------------
def test_band_expansion_on_either_side_of_its_threshold(eng, line):
    """300 K and 1e4 K cells in one grid, 256 channels whose half-width puts the quotient of
    band_needs_exp at 0.9 (first-order factor, dropped term up to 1.8e-9 at the band edges) and at
    1.1 (exp() per lane) for the 300 K cells."""
    lc, line_dev = line
    shape = R.WAVE_SHAPE
    y, temp = R.band_cells()
    fields = _upload(eng, R.host_fields(y, temp, lc))
    dev = _read_back(fields, shape)
    cells = R.cell_consts(dev, lc)
    cold = dev["temp"] == R.BAND_TEMPS[0]
    assert cold.sum() == cold.size // 2
    for ratio, want in ((0.9, False), (1.1, True)):
        nu, dnu = R.band_channels(lc, ratio)
        codes = R.path_codes(cells, nu, 256)
        assert np.all(((codes[:, cold] & R.EXP_FLAG) != 0) == want)
        assert not np.any(codes[:, ~cold] & R.EXP_FLAG)
        got = _scan(eng, fields, None, 0.0, line_dev, nu, shape)
        ref = R.line_term_ref(dev, lc, nu)
        rel, keep = R.check_terms(got, ref, U.K3_RTOL_WAVE)
        assert keep.all()
        edge = [0, 127, 128, 255]                    # both band edges and the centre
        print("half-width %.4f MHz (quotient %.1f, flag %s): worst at the edges and the centre %s, "
              "over the band %.2e" % (dnu / 1e6, ratio, "set" if want else "clear",
                                      ["%.2e" % rel[i][cold[...]].max() for i in edge],
                                      rel[:, cold].max()))


# ---- the XCD tile map on whole maps ------------------------------------------------------------------
@pytest.mark.parametrize("nchan", [256, 40])
@pytest.mark.parametrize("shape", [(9, 3, 24), (5, 2, 52), (1, 2, 130)])
def test_tile_map_on_whole_maps(eng, line, shape, nchan):
    """Workgroup counts that are no multiple of 8 (27 / 18, 35 / 20 and 17 / 9 for the 256- / 64-lane
    kernels) with a ragged last tile in z: the remapped workgroups and the identity tail together
    must cover every tile exactly once.  Random cells, every pixel against the oracle."""
    from oracle import rt_oracle as orc
    from rajepy_amd.maths import rrls
    lc, line_dev = line
    zt = 8 if nchan > 128 else 16
    wgs = shape[0] * -(-shape[2] // zt)
    assert wgs % 8 != 0 and wgs > 8
    g = U.synth_host(shape, 20251018 + shape[2], 1)
    p = copy.deepcopy(U.load_golden("cfg1_example")[2])
    p["ejection"] = U.example_bursts_params()
    p["grid"].update(n_x=shape[0], n_y=shape[1], n_z=shape[2])
    jet = orc.OracleJet.from_fields(p, g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"],
                                    g["rr"], g["vy"])
    jet.time = 1.0 * YEAR
    fields = eng.upload_fields(g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"],
                               g["rr"] < 0, vy=g["vy"], csize_au=jet.csize, dtype=8)
    nu = orc.chan_freqs(rrls.rrl_nu_0("H", 66, 1), nchan * 1e5, 1e5)
    assert len(nu) == nchan
    tau = eng.rrl_scan(fields, U.bursts_from_oracle(jet), jet.time, line_dev, list(nu))
    eng.synchronize()
    ref = jet.optical_depth_rrl("H66a", np.asarray(nu))
    assert np.isfinite(ref).all() and (ref > 0).all()
    got = tau.cpu().numpy().reshape(ref.shape)
    print("%r, %d channels, %d workgroups: worst %.2e" % (shape, nchan, wgs,
                                                        np.max(np.abs(got - ref) / ref)))
    np.testing.assert_allclose(got, ref, rtol=U.k3_rtol(nchan), atol=0)
