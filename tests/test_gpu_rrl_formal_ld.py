"""K6 (rjp_rrl_formal) held to the long-double reference of tests/rrl_formal_ld_ref.py PIXEL BY PIXEL:
|got - ref| <= bound[f, p], the derived absolute bound of that module (Voigt, continuum, Planck
expansion, roundings), on hand-made grids of 2 x 70 x 17 cells (70 rows cross the slabs of 8, 16 and
32 rows mid-sightline; 17 sightlines are a full tile and a one-wide one at ZT = 16, four tiles and a
one-wide one at ZT = 4), of one row, and of 8 rows whose first three are empty, for channel counts
that cover the three lane layouts, their full and one-lane blocks and a second channel block.  The
reference's inputs are read back from the device tensors of the uploaded fields.

This supplements rrl_formal_ref.within (asserted here too), whose absolute term is normalised to
the channel's brightest pixel.  Every input also asserts that occupied y-ranges change no bit and
that `add=` adds exactly its argument.  Every test prints its worst error as a share of the bound
and the term of the bound that dominates there (quotes them).

Measured on an MI355X (table in DESIGN.md section 3, K6): worst share 0.25 (per-cell l up to 50, 257
channels), 0.05 ... 0.2 elsewhere on the wave-uniform layouts, <= 0.03 on the per-lane layout; the
Voigt term dominates the bound at every worst pixel.  With e_c = 1 - (1 - e^-c) in the kernel the
pixel behind a front cell of c = 30 was off by 6e4 ... 6e5 times its bound on every channel count."""
import numpy as np
import pytest

from tests import f32_ref as F
from tests import gpu_util as U
from tests import rrl_formal_ld_ref as L
from tests import rrl_formal_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not L.HAVE_LD, reason=L.LD_REASON)]


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


def _upload(eng, cs, dtype):
    g = cs["g"]
    return eng.upload_fields(g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"], g["rr"] < 0,
                             vy=g["vy"], csize_au=L.CSIZE, dtype=dtype)


def _maps(eng, line_dev, cs, fields):
    """-> (the map, the map with occupied y-ranges, the map with `add`, add), host [F, nx, nz]."""
    import torch
    from rajepy_amd.engine import make_bursts
    bursts = make_bursts(*cs["bursts"]) if cs["bursts"] is not None else None
    nx, _, nz = fields.shape
    nchan = len(cs["nu"])
    host = lambda t: t.cpu().numpy().reshape(nchan, nx, nz)
    call = lambda add=None: host(eng.rrl_formal(fields, bursts, cs["t"], cs["mode"], line_dev,
                                                cs["nu"], cs["ctau"], cs["csrc"], cs["hnu_k"],
                                                add=add))
    got = call()
    scale = float(np.nanmax(np.abs(got))) if np.isfinite(got).any() else 1.0
    add = np.random.default_rng(nchan).uniform(-scale, scale, got.shape)
    add[:, ::2, ::3] *= 1e-7
    added = call(torch.from_numpy(add.reshape(nchan, -1)).to(eng.device))
    assert fields.ylo is None
    eng.compute_y_bounds(fields)
    assert fields.ylo is not None
    return got, call(), added, add


def _hold(eng, line, cs, dtype=8, what="", dev_of=None):
    """Upload, run, judge per pixel; the identities; -> worst share of the bound."""
    lc, line_dev = line
    fields = _upload(eng, cs, dtype)
    dev = F.device_fields(fields)
    r = L.reference_of(cs, dev if dev_of is None else dev_of(dev), lc)
    got, bounded, added, add = _maps(eng, line_dev, cs, fields)
    share, top, at = L.judge(got, r, what)
    old = R.within(got, r["ref"], U.k3_rtol(len(cs["nu"])))
    print("\nLDREF %s: worst error %.3g of the bound at (f, x, z) = %r, where %s dominates it; "
          "%.3g of rrl_formal_ref.within" % (what, share, tuple(int(i) for i in at), top, old))
    # occupied y-ranges change no bit
    assert np.array_equal(got, bounded, equal_nan=True), what
    # add: one more rounding, or none where the compiler fuses csrc I + add
    want = got + add
    assert np.array_equal(np.isnan(added), np.isnan(got)), what
    ok = ~np.isnan(got)
    assert np.all(np.abs(added - want)[ok] <= 2.0 ** -53 * (np.abs(got) + np.abs(want))[ok]), what
    assert share <= 1.0, (what, share, at, top)
    assert old <= 1.0, (what, old)
    return share, r, got


@pytest.mark.parametrize("nchan", L.NCHANS)
@pytest.mark.parametrize("name", L.INPUTS)
def test_every_pixel_inside_its_bound(eng, line, name, nchan):
    """The inputs of rrl_formal_ld_ref.case on 2 x 70 x 17 cells, f64 storage: (a) "spread", 300 K to
    3e4 K inside every sightline with 11 bursts in each jet; (b) "thick", one front cell of c = 1, 5,
    10, 20, 30 at the line centre in front of thin gas, the mirror order, and 70 cells that sum to
    tau_C = 100 and 600; (c) "thickline", per-cell l up to 50 with cold gas in front of hot gas
    (negative pixels, pixels near zero); (d) "faint", every other sightline of a tile at 1e-6 of its
    neighbours; (e) "mixed", live, continuum-only and dead cells interleaved, a NaN sightline, a zero
    one and a channel of line-only cells (ctau = 0: the fields admit no such cell, every factor of b
    is one of C); (f) the bands at 0.9 and 1.1 of band_needs_exp's threshold for the 300 K cells and
    0.7 ... 1.3 of the rest frequency (+-1e-3 is the band of the others)."""
    lc, _ = line
    cs = L.case(name, lc, nchan)
    _, r, got = _hold(eng, line, cs, what="%s, %d channels, f64" % (name, nchan))
    ref = r["ref"]
    if name == "spread":
        assert min(len(b) for b in cs["bursts"]) > 8 and np.ptp(cs["g"]["rr"]) > 0
        T = cs["g"]["temp"]
        assert np.all(T.min(axis=1) == 300.0) and np.all(T.max(axis=1) == 3e4)
    if name == "thickline":
        assert np.any(ref < 0) and np.any(got < 0)
    if name == "mixed":
        assert np.isnan(ref[:, 0, 3]).all() and np.all(ref[:, 1, 5] == 0.0)
    if name == "thick" and nchan % 2:
        top = np.nanmax(np.abs(ref[nchan // 2]))
        assert abs(ref[nchan // 2, 0, 4]) < 1e-10 * top        # the pixel behind c = 30


@pytest.mark.parametrize("nchan", L.NCHANS)
def test_temperature_spread_on_f32_storage(eng, line, nchan):
    """Input (a) on float fields: the reference reads the stored floats back, so the rounding of the
    fields is not under test and the bound is the f64 one."""
    lc, _ = line
    _hold(eng, line, L.case("spread", lc, nchan), dtype=4,
          what="spread, %d channels, f32" % nchan)


@pytest.mark.parametrize("nchan", L.NCHANS)
@pytest.mark.parametrize("ny", [1, 8])
def test_one_row_and_a_range_that_starts_mid_slab(eng, line, ny, nchan):
    """n_y = 1, and n_y = 8 with rows 0-2 empty: with occupied y-ranges the walk starts at row 3 of
    the only slab (_hold runs the kernel without and with them)."""
    lc, _ = line
    _hold(eng, line, L.case("spread", lc, nchan, ny=ny),
          what="spread, n_y = %d, %d channels, f64" % (ny, nchan))


@pytest.mark.parametrize("nchan", [16, 65, 257])
def test_tau_c_above_800_stays_finite(eng, line, nchan):
    """Input (b) with the 70-cell sightlines at tau_C = 150 and 900: Theta_C underflows to 0 on the
    way (e^-745 is the smallest double).  Finite everywhere, no NaN; the values against the
    reference of the cells in front of row 44 (tau_C = 566 there: what lies behind adds less than
    e^-560 of a front cell's term)."""
    lc, _ = line
    cs = L.case("thick", lc, nchan)
    cs["g"]["ff"][:, :, 10:16] *= 1.5
    tau_c = cs["ctau"].max() * np.nansum(
        (cs["g"]["nd"] * cs["g"]["xi"]) ** 2 * cs["g"]["ff"] * cs["g"]["temp"] ** -1.5, axis=1)
    assert tau_c[:, 13:16].min() > 800.0 and tau_c[:, 13:16].max() < 1000.0

    def front(dev):
        dev = dict(dev, pf=dev["pf"].copy())
        dev["pf"][:, 44:, 13:16] = 0.0
        return dev

    _, r, got = _hold(eng, line, cs, what="thick with tau_C = 900, %d channels, f64" % nchan,
                      dev_of=front)
    assert np.all(np.isfinite(got))
    assert float(np.sum(r["q"]["c"], axis=2)[:, :, 13:16].max()) < 600.0
