"""The epoch-sweep kernels against an independent long-double reference at EVERY epoch and pixel, at
bounds derived per path in tests/sweep_ref.py (pinned without a GPU by
tests/test_epoch_sweep_reference_cpu.py): the epoch tiles of ff_scan_kernels.h -- direct evaluation,
the two- and the three-operation uniform-spacing recurrences at 4 / 8 / 16 / 32 epochs, the LDS-DMA
tile kernel -- K1m (ff_moments.hip), K1m-LT (ff_lt.hip), the cached contraction, and the light
curves K2 makes of their sums.

Every test reads the device's own arrays back for the reference, asserts the path through
last_scan_path() / last_scan_tiles() (the latter against the host restatement of ff_scan_plan),
compares zero / NaN / inf patterns exactly and every finite value at the derived ABSOLUTE bound, and
prints the worst measured / bound ratio per path."""
import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import f32_ref as F
from tests import gpu_util as U
from tests import sweep_ref as R

pytestmark = pytest.mark.gpu
YEAR = orc.YEAR
MODE = 0                                  # RJP_GFF_SCALAR
PATHS = {R.DIRECT: "direct", R.TWO_OP: "two-op", R.THREE_OP: "three-op"}


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    e.cache_moments = False
    yield e
    e.close()


# ---- models ----------------------------------------------------------------------------------------
def _host(shape, seed, jets):
    """gpu_util.synth_host with a temperature spread; `jets`: "halves" = the generator's (red where
    i_z < n_z / 2: on these small maps every wave straddles the plane and runs the three-operation
    recurrence), "rows" = a jet per x-row, "red" / "blue" = one jet everywhere (waves inside one jet:
    the two-operation recurrence), "cells" = a jet per CELL."""
    g = U.synth_host(shape, seed, 1)
    if jets == "rows":
        g["rr"] = np.where((np.arange(shape[0]) % 2 == 0)[:, None, None], -1.0, 1.0) * np.ones(shape)
    elif jets == "cells":
        g["rr"] = np.where(np.random.default_rng(seed).random(shape) < 0.45, -1.0, 1.0)
    elif jets != "halves":
        g["rr"] = np.full(shape, -1.0 if jets == "red" else 1.0)
    return g


def _upload(eng, g, layout):
    """Host fields -> device fields on the layout the scans are to take: "tau" (a0, ts[, em0]),
    "cmp" (em0, temp, ts) or "wide" (the five fields)."""
    eng.use_compact = layout != "wide"
    try:
        f = eng.upload_fields(g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"],
                              g["rr"] < 0, csize_au=0.5, dtype=8)
    finally:
        eng.use_compact = True
    if layout == "tau":
        eng.tau_layout(f, MODE)
        assert f.a0 is not None
    assert (f.em0 is None) == (layout == "wide")
    return f


def _weights(f, layout):
    """The device's own arrays: -> (a0, em0, ts, r_tau, r_em) -- signed weights of the optical-depth
    sums and of the emission measure [n_x, n_y, n_z], launch times, and the rounding terms r of
    sweep_ref's bound (on the compact / wide layouts the weights are formed on the device:
    f32_ref.tau_rtol / em_rtol)."""
    shape = f.shape
    ny = shape[1]
    rd = lambda t: t.cpu().numpy().reshape(shape)
    ts = rd(f.ts)
    if layout == "tau":
        return rd(f.a0), rd(f.em0), ts, (ny + 4) * R.EPS, (ny + 4) * R.EPS
    dev = F.device_fields(f)
    lay = "compact" if layout == "cmp" else "wide"
    return F.a0_of(dev, MODE, lay), F.em0_of(dev, lay), ts, F.tau_rtol(ny), F.em_rtol(ny)


def _report(what, worst):
    print("%s: worst measured / bound %s" % (what, ", ".join(
        "%s %.3f" % (k, v) for k, v in sorted(worst.items())) or "-"))


def _run_tiles(eng, f, layout, wts, bursts, epochs, want_em, mixed, worst, what):
    """One sweep on the epoch tiles: the path, the tiles against the host plan, every (epoch, pixel)
    of the sums (and EM maps) against the reference at the derived bound."""
    from rajepy_amd import engine as E
    a0, em0, ts, r_tau, r_em = wts
    nx, ny, nz = f.shape
    eng.use_moments = False
    try:
        sumA, em, _ = eng.ff_scan(f, E.make_bursts(*bursts), epochs, MODE, want_em=want_em,
                                  want_tavg=False)
    finally:
        eng.use_moments = True
    assert eng.last_scan_path()[0] == "tiles", what
    dev_tiles = eng.last_scan_tiles()
    tiles = R.tile_plan_host(epochs, bursts, 8, layout, want_em, nz, True)
    assert [(e0, et, un, vec) for e0, et, un, _, vec in dev_tiles] == tiles, (what, dev_tiles, tiles)
    assert all(1 <= ns <= ny for _, _, _, ns, _ in dev_tiles)
    if layout == "wide":
        assert all(et <= 8 for _, et, _, _ in tiles)
    eng.synchronize()
    maps = [(sumA, a0, 1.0, r_tau, "sums")]
    if want_em:
        maps.append((em, em0, F.em_scale(f.csize_au), r_em, "EM"))
    for got, w0, scale, rr, name in maps:
        got = got.cpu().numpy().reshape(len(epochs), nx, nz)
        ref = R.ref_sweep(w0, ts, bursts, epochs, threads=1) * scale
        B, path = R.tile_bound(w0 * scale, ts, bursts, epochs, tiles, ref, rr, mixed)
        for code, label in PATHS.items():
            sel = path == code
            if sel.any():
                worst[label] = max(worst.get(label, 0.0), R.ratio(got, ref, B, sel))
        R.within(got, ref, B, (what, name))
    return tiles


def _epoch_lists():
    return [("u4", R.uniform_epochs(4)), ("u8", R.uniform_epochs(8)), ("u16", R.uniform_epochs(16)),
            ("u32", R.uniform_epochs(32)), ("u45", R.uniform_epochs(45)),
            ("u23", R.uniform_epochs(23)), ("irr17", R.irregular_epochs())]


# ---- the epoch tiles, f64 storage ------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tau", "cmp", "wide"])
@pytest.mark.parametrize("shape,jets", [((3, 37, 16), "halves"), ((3, 37, 16), "blue"),
                                        ((3, 37, 15), "halves"), ((3, 37, 15), "red"),
                                        ((2, 200, 64), "rows")])
def test_tiles_with_the_example_bursts(eng, layout, shape, jets):
    """Burst set (a) on every epoch list -- uniform 4 / 8 / 16 / 32, 45 = 32 + 8 + 4 + 1,
    23 = 16 + 4 + 2 + 1, 17 irregular -- with and without EM maps (the 32-epoch tile with EM is a
    kernel of its own).  Long tiles exist on the tau and compact layouts only; wide falls back to
    tiles of <= 8 epochs.  (2, 200, 64) with a jet per x-row: the 16- and 32-epoch tiles run one
    sightline per lane, a wave is one row and takes the two-operation path; its 8- and 4-epoch tiles
    hold two rows per wave and take the three-operation one."""
    g = _host(shape, 4300 + shape[2], jets)
    f = _upload(eng, g, layout)
    wts = _weights(f, layout)
    worst = {}
    for name, ep in _epoch_lists():
        for want_em in (False, True):
            tiles = _run_tiles(eng, f, layout, wts, U.example_burst_lists(), ep, want_em, None,
                               worst, (layout, shape, jets, name, want_em))
            if name.startswith("u") and layout != "wide":
                want = {"u4": [4], "u8": [8], "u16": [16], "u32": [32], "u45": [32, 8, 4, 1],
                        "u23": [16, 4, 2, 1]}[name]
                assert [et for _, et, _, _ in tiles] == want
                assert all(un == (et >= 4) for _, et, un, _ in tiles)
            if name == "irr17":
                assert all(un == 0 for _, _, un, _ in tiles)
    _report("tiles, example bursts, %s %s %s" % (layout, shape, jets), worst)
    assert "direct" in worst and ("two-op" in worst or "three-op" in worst)
    if jets in ("red", "blue"):
        assert "three-op" not in worst
    if jets == "halves":
        assert "two-op" not in worst


@pytest.mark.parametrize("jets", ["blue", "halves"])
@pytest.mark.parametrize("layout,et", [(lay, et) for lay in ("tau", "cmp", "wide")
                                       for et in (4, 8, 16, 32) if lay != "wide" or et <= 8])
def test_tiles_at_the_28_sigma_limit(eng, layout, jets, et):
    """Burst sets (b) and (c): one narrow burst per jet whose sigma puts the tile's half-span at
    27.9 sigma -- the recurrence must be on, and it is the only place where the anchor's magnitude and
    the kDead cut matter -- and at 28.1 sigma: that tile size is refused.  Two planted cells peak at
    the tile's first and at its last epoch, as far from the anchor as a live cell gets.  (The wide
    layout has no long tiles: ET = 4 and 8 only.)"""
    shape = (3, 37, 16)
    worst = {}
    for rs in (27.9, 28.1):
        ep, bursts, t0 = R.narrow_case(et, rs)
        g = _host(shape, 4400 + et, jets)
        g["ts"] = 0.2 * g["ts"]                       # launch times the narrow burst reaches
        g["ts"][0, 5, 0] = ep[0] - t0                 # peaks at the first epoch ...
        g["ts"][0, 6, 0] = ep[-1] - t0                # ... and at the last
        g["ts"][2, 7, 15] = ep[0] - t0
        g["ts"][2, 8, 15] = ep[-1] - t0
        f = _upload(eng, g, layout)
        wts = _weights(f, layout)
        for want_em in (False, True):
            tiles = _run_tiles(eng, f, layout, wts, bursts, ep, want_em, None, worst,
                               (layout, jets, et, rs, want_em))
            if rs < 28.0:
                assert tiles == [(0, et, 1, 2 if et < 16 else 1)]
            else:
                assert all(t_et < et or un == 0 for _, t_et, un, _ in tiles)
                if et <= 8:
                    assert tiles == [(0, et, 0, 2)]
        # the planted cells are seen: the burst at its peak, squared, in the pixel's sum
        ref = R.ref_sweep(wts[0], wts[2], bursts, ep, threads=1)
        amp = bursts[0][0][1] if g["rr"][0, 5, 0] < 0 else bursts[1][0][1]
        assert ref[0, 0, 0] >= abs(wts[0][0, 5, 0]) * (1 + amp) ** 2 * (1 - 1e-9)
        assert ref[-1, 0, 0] >= abs(wts[0][0, 6, 0]) * (1 + amp) ** 2 * (1 - 1e-9)
    _report("tiles at 27.9 / 28.1 sigma, ET %d, %s %s" % (et, layout, jets), worst)
    assert ("two-op" if jets == "blue" else "three-op") in worst
    if et <= 8:
        assert "direct" in worst


@pytest.mark.parametrize("layout", ["tau", "cmp"])
@pytest.mark.parametrize("name,jets", [("eleven+three", "red"), ("eleven+three", "blue"),
                                       ("eleven+three", "halves"), ("dip", "blue"),
                                       ("dip", "halves"), ("red-only", "red"),
                                       ("red-only", "halves")])
def test_tiles_overflow_dips_and_the_burstless_jet(eng, layout, name, jets):
    """(d) 11 bursts in one jet and 3 in the other: more than eight per jet inside a recurrence (the
    parameter prefetch clamps, the overflow loop forms 2 k2 dt itself; straddling waves read q from
    the overflow table).  (e) a dip of amplitude -0.9 beside a positive burst: chi passes near 0, the
    bound is absolute.  (f) bursts in the red jet only, NaN launch times in both jets: the burst-less
    jet keeps its cells."""
    shape = (3, 37, 16)
    g = _host(shape, 4500, jets)
    if name == "red-only":
        m = np.random.default_rng(45).random(shape) < 0.06
        g["ts"] = np.where(m, np.nan, g["ts"])
        assert np.isnan(g["ts"][g["rr"] < 0]).any()
        assert jets == "red" or np.isnan(g["ts"][g["rr"] > 0]).any()
    f = _upload(eng, g, layout)
    wts = _weights(f, layout)
    bursts = R.tile_burst_sets()[name]
    worst = {}
    for ename, ep in (("u32", R.uniform_epochs(32)), ("u8", R.uniform_epochs(8)),
                      ("u45", R.uniform_epochs(45)), ("irr17", R.irregular_epochs())):
        for want_em in (False, True):
            tiles = _run_tiles(eng, f, layout, wts, bursts, ep, want_em, None, worst,
                               (layout, name, jets, ename, want_em))
            if ename == "u32":
                assert tiles == [(0, 32, 1, 1)]
    if name == "dip":
        # the dip is felt: some cell's chi comes within 0.2 of zero at some epoch of the sweep
        red = np.signbit(wts[0])
        with np.errstate(all="ignore"):
            low = min(float(np.nanmin(U.chi_exact(bursts[0 if r else 1], t - wts[2][red == r])))
                      for t in R.uniform_epochs(45) for r in (True, False) if (red == r).any())
        assert low < 0.2, low
    _report("tiles, %s, %s %s" % (name, layout, jets), worst)


@pytest.mark.parametrize("layout", ["tau", "cmp", "wide"])
def test_tiles_with_both_jets_on_every_sightline(eng, layout):
    """(g) the jet flag changes along y (a real, inclined jet), built as
    test_gpu_lt.py::test_mixed_jet_sightlines_on_every_sweep_path builds it: every wave straddles the
    red / blue plane and takes the three-operation path, at ET = 4, 8, 16, 32."""
    worst = {}
    for shape in ((3, 37, 16), (3, 37, 15)):
        g = _host(shape, 4600, "cells")
        f = _upload(eng, g, layout)
        wts = _weights(f, layout)
        assert np.signbit(wts[0]).any(axis=1).all() and (~np.signbit(wts[0])).any(axis=1).all()
        for et in (4, 8, 16, 32):
            for want_em in (False, True):
                tiles = _run_tiles(eng, f, layout, wts, U.example_burst_lists(), R.uniform_epochs(et),
                                   want_em, True, worst, (layout, shape, et, want_em))
                if layout != "wide":
                    assert [t[1] for t in tiles] == [et]
    _report("tiles, a jet per cell, %s" % layout, worst)
    assert set(worst) == {"three-op"}


# ---- K1m -------------------------------------------------------------------------------------------------
def _run_moments(eng, f, wts, bursts, epochs, want_em, want_path, shapes, what):
    """One sweep on a moment path: path and shape against the host restatement, sums (and EM maps)
    against the reference at the moment bound.  -> worst measured / bound."""
    from rajepy_amd import engine as E
    a0, em0, ts, _, _ = wts
    nx, ny, nz = f.shape
    sumA, em, _ = eng.ff_scan(f, E.make_bursts(*bursts), epochs, MODE, want_em=want_em,
                              want_tavg=False)
    path = eng.last_scan_path()[0]
    assert path == want_path, (what, path)
    assert eng.last_scan_tiles() == []
    K, N = eng.last_moment_shape
    rng = f.ts_range
    assert rng == (float(np.nanmin(ts)), float(np.nanmax(ts)))
    if shapes is not None:
        tab = R.mom_tables_host(bursts, epochs, rng, shapes)
        assert tab is not None and (tab["K"], tab["N"]) == (K, N), (what, (K, N), tab and tab["tried"])
        W = tab["W"]
    else:
        W, err = R.mom_table(bursts, epochs, rng, K, N)
        assert err <= R.MOM_TOL, (what, err)
    eng.synchronize()
    worst = 0.0
    maps = [(sumA, a0, 1.0, "sums")]
    if want_em:
        maps.append((em, em0, F.em_scale(f.csize_au), "EM"))
    for got, w0, scale, name in maps:
        got = got.cpu().numpy().reshape(len(epochs), nx, nz)
        ref = R.ref_sweep(w0, ts, bursts, epochs) * scale
        B, _ = R.moment_bound(w0, ts, bursts, epochs, rng, K, N, W, ref, scale)
        worst = max(worst, R.ratio(got, ref, B))
        R.within(got, ref, B, (what, name))
    return worst, (K, N)


@pytest.fixture()
def forced(eng):
    """`force_moments`: the library's cost model keeps the epoch tiles on grids this small."""
    eng.force_moments, eng.use_moments = True, True
    yield eng
    eng.force_moments = False


@pytest.mark.parametrize("scale,shape_kn", [(1.0, (53, 12)), (2.5, (80, 8)), (0.8, (39, 16))])
def test_moments_on_19_tiles_of_sightlines(forced, scale, shape_kn):
    """(19, 96, 16): 304 sightlines = 19 tiles of moments_kernel -- the XCD map moves 16 of them and
    leaves 3 on the identity -- at the three (bins, order) shapes, 12 / 32 / 33 / 100 uniform and 17
    irregular epochs (one to four contraction passes, the split contraction and its sum kernel), EM
    maps through the second pass."""
    eng = forced
    shape = (19, 96, 16)
    f = _upload(eng, _host(shape, 4700, "halves"), "tau")
    wts = _weights(f, "tau")
    bursts = R.scaled_example(scale)
    worst = {}
    for name, ep, want_em in (("u12", R.uniform_epochs(12), False), ("u32", R.uniform_epochs(32), False),
                              ("u33", R.uniform_epochs(33), True), ("u100", R.uniform_epochs(100), False),
                              ("irr17", R.irregular_epochs(), True)):
        worst[name], kn = _run_moments(eng, f, wts, bursts, ep, want_em, "moments", R.MOM_SHAPES,
                                       (shape, scale, name))
        assert kn == shape_kn
    _report("K1m %s x%.1f" % (shape_kn, scale), worst)


def test_moments_ragged_tile_y_bounds_and_special_cells(forced):
    """(5, 90, 23): odd n_z, 8 tiles with 3 live lanes in the last, occupied y-ranges attached, NaN /
    zero cells in every field, T = 0 cells (an infinite weight: the sightline comes out +inf, as the
    reference's sum does) and NaN launch times."""
    eng = forced
    shape = (5, 90, 23)
    g = _host(shape, 4800, "halves")
    rng = np.random.default_rng(48)
    for k, vals in (("nd", [np.nan, 0.0]), ("xi", [np.nan]), ("temp", [np.nan]),
                    ("ff", [np.nan, 0.0]), ("ts", [np.nan])):
        m = rng.random(shape) < 0.08
        g[k] = np.where(m, rng.choice(vals, size=shape), g[k])
    g["nd"][:, :7, :] = np.nan
    g["nd"][:, -9:, :] = np.nan
    for c in ((1, 20, 3), (4, 33, 22)):                         # T = 0: T^-1.5 = inf
        g["nd"][c], g["xi"][c], g["ff"][c], g["ts"][c], g["temp"][c] = 3e6, 0.3, 1.0, 2.0 * YEAR, 0.0
    f = _upload(eng, g, "tau")
    eng.compute_y_bounds(f)
    wts = _weights(f, "tau")
    assert np.isinf(wts[0]).sum() >= 1 and np.isnan(wts[0]).any() and (wts[0] == 0).any()
    worst = {}
    for name, ep, want_em in (("u33", R.uniform_epochs(33), True), ("irr17", R.irregular_epochs(), False)):
        worst[name], kn = _run_moments(eng, f, wts, U.example_burst_lists(), ep, want_em, "moments",
                                       R.MOM_SHAPES, (shape, name))
        assert kn == (53, 12)
    # ... and bursts in one jet only: the other jet's NaN launch times do not drop its cells
    worst["red-only"], _ = _run_moments(eng, f, wts, U.example_burst_lists(only="R"),
                                        R.uniform_epochs(12), False, "moments", R.MOM_SHAPES,
                                        (shape, "red-only"))
    _report("K1m (5, 90, 23) with y-bounds and special cells", worst)


def test_moments_unsplit_contraction(forced):
    """(512, 16, 512): 262144 sightlines = 4096 waves, the size from which the contraction runs
    unsplit (moments_eval_kernel<false>), 12 epochs."""
    from rajepy_amd import engine as E
    eng = forced
    shape = (512, 16, 512)
    assert (shape[0] * shape[2] + 63) // 64 >= 4096                 # mom_eval_split: one chunk
    f = eng.synth_fields(shape, 4900, 1, 8, csize_au=0.5, wide=False, tau_mode=MODE)
    wts = _weights(f, "tau")
    worst, kn = _run_moments(eng, f, wts, U.example_burst_lists(), R.uniform_epochs(12), False,
                             "moments", R.MOM_SHAPES, shape)
    _report("K1m %s, unsplit contraction" % (kn,), {"u12": worst})


def test_cached_moments_with_other_epochs_and_bursts(forced):
    """The cached contraction against the REFERENCE (test_gpu_moments.py compares it with the
    uncached sweep): the first sweep fills the caller-kept maps, the second -- other epochs, other
    burst parameters -- is the contraction alone."""
    eng = forced
    shape = (4, 180, 48)
    f = _upload(eng, _host(shape, 5000, "halves"), "tau")
    wts = _weights(f, "tau")
    eng.cache_moments = True
    try:
        w1, kn = _run_moments(eng, f, wts, U.example_burst_lists(), R.uniform_epochs(32), False,
                              "moments", R.MOM_SHAPES, (shape, "fill"))
        assert kn == (53, 12) and (f.mom_cache["K"], f.mom_cache["N"]) == kn
        other = ([(0.6 * YEAR, 3.0, 0.2 * YEAR), (2.2 * YEAR, 6.0, 0.5 * YEAR)],
                 [(1.1 * YEAR, 2.0, 0.4 * YEAR)])
        ep2 = (np.linspace(0.2, 4.4, 17) * YEAR).tolist()
        w2, kn2 = _run_moments(eng, f, wts, other, ep2, False, "cached", None, (shape, "cached"))
        assert kn2 == kn
        w3, _ = _run_moments(eng, f, wts, U.example_burst_lists(), R.irregular_epochs(), False,
                             "cached", None, (shape, "cached, irregular"))
    finally:
        eng.cache_moments = False
        f.mom_cache = None
    _report("cached contraction %s" % (kn,), {"fill": w1, "other epochs + bursts": w2, "irregular": w3})


# ---- K1m-LT ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,scale", [(1, 10.0), (20, 1.0), (32, 1.0)])
def test_lt_moments_on_300_sightlines(forced, K, scale):
    """(3, 96, 100): 300 sightlines = 5 groups of 64 -- row shares over several waves plus
    lt_reduce_kernel -- with 1, 20 and 32 launch-time bins (one bin holds only bursts ten times as
    broad as the example's), 12 and 32 epochs."""
    eng = forced
    shape = (3, 96, 100)
    f = _upload(eng, _host(shape, 5100, "halves"), "tau")
    eng.build_lt(f, K)
    wts = _weights(f, "tau")
    worst = {}
    for name, ep in (("u12", R.uniform_epochs(12)), ("u32", R.uniform_epochs(32)),
                     ("irr17", R.irregular_epochs())):
        worst[name], kn = _run_moments(eng, f, wts, R.scaled_example(scale), ep, False, "lt",
                                       R.lt_shapes(K), (shape, K, name))
        assert kn[0] == K
    _report("K1m-LT K = %d, order %d" % kn, worst)


def test_lt_moments_one_wave_per_group(forced):
    """(256, 32, 256) = 1024 groups of 64 sightlines: one wave per group, 12 and 32 epochs."""
    eng = forced
    shape = (256, 32, 256)
    f = eng.synth_fields(shape, 5200, 1, 8, csize_au=0.5, wide=False, tau_mode=MODE)
    eng.build_lt(f, 20)
    wts = _weights(f, "tau")
    worst = {}
    for name, ep in (("u12", R.uniform_epochs(12)), ("u32", R.uniform_epochs(32))):
        worst[name], kn = _run_moments(eng, f, wts, U.example_burst_lists(), ep, False, "lt",
                                       R.lt_shapes(20), (shape, name))
    f.lt = None
    _report("K1m-LT %s, one wave per group" % (kn,), worst)


# ---- light curves ------------------------------------------------------------------------------------------
def _lc_check(got, sums_ref, bound, tavg, ctau, cflux, what):
    want, _ = R.light_curves(sums_ref, tavg, ctau, cflux)
    BF = R.light_curve_bound(sums_ref, bound, tavg, ctau, cflux)
    assert got.shape == want.shape and (want > 0).all()
    frac = float(np.max(np.abs(got - want) / BF))
    print("%s: worst measured / bound %.3f (worst relative difference %.3g, bound %.3g)"
          % (what, frac, float(np.max(np.abs(got - want) / want)), float(np.max(BF / want))))
    assert frac <= 1.0, (what, frac)


def test_light_curves_without_cubes(eng):
    """rjp_ff_maps with neither cube (ff_ftot_kernel) on the sums of a 33-epoch sweep, against
    long-double totals of the map formulas on the reference sums: the tau bound carried through
    1 - e^-tau plus (P + 4) 2^-53 (sweep_ref.light_curve_bound)."""
    from rajepy_amd import engine as E
    shape = (2, 200, 64)
    g = _host(shape, 5300, "rows")
    g["temp"][0, :, 5] = np.nan                                     # an empty sightline: T_avg NaN
    g["nd"][0, :, 5] = np.nan
    f = _upload(eng, g, "tau")
    wts = _weights(f, "tau")
    a0, _, ts, r_tau, _ = wts
    bursts, ep = U.example_burst_lists(), R.uniform_epochs(33)
    eng.use_moments = False
    try:
        sumA, _, _ = eng.ff_scan(f, E.make_bursts(*bursts), ep, MODE, want_em=False, want_tavg=False)
    finally:
        eng.use_moments = True
    assert eng.last_scan_path()[0] == "tiles"
    tiles = [(e0, et, un, vec) for e0, et, un, _, vec in eng.last_scan_tiles()]
    assert tiles == R.tile_plan_host(ep, bursts, nz=shape[2]) and [t[1] for t in tiles] == [32, 1]
    tavg = eng.tavg(f)
    freqs = np.array([1e9, 5e9, 5e10])
    ctau, cflux = E.ff_channel_coeffs(freqs, 0.5, 120., MODE, [5.0, 4.5, 4.0])
    tau, flux, ftot = eng.ff_maps(sumA, tavg, ctau, cflux, want_tau=False, want_flux=False)
    assert tau is None and flux is None
    eng.synchronize()
    tavg_h = tavg.cpu().numpy()
    assert np.isnan(tavg_h).sum() == 1
    ref = R.ref_sweep(a0, ts, bursts, ep, threads=1)
    B, _ = R.tile_bound(a0, ts, bursts, ep, tiles, ref, r_tau)
    _lc_check(ftot.cpu().numpy(), ref, B, tavg_h, ctau, cflux, "rjp_ff_maps totals, 33 epochs")


def test_jetmodel_flux_vs_time(eng, tmp_path):
    """JetModel.flux_vs_time on the example jet (K4-built fields, both lobes, occupied y-ranges)
    against the same reference built from the model's own a0 / ts / T_avg."""
    from rajepy_amd import classes, logger
    from tests.test_host_logic import example_params
    jm = classes.JetModel(example_params(), log=logger.Log(str(tmp_path / "a.log"), verbose=False),
                          engine=eng)
    freqs = np.array([1e9, 5e9, 5e10])
    times = np.linspace(0., 3., 13) * YEAR
    lc = jm.flux_vs_time(times, freqs)
    assert eng.last_scan_path()[0] == "tiles"
    tiles = [(e0, et, un, vec) for e0, et, un, _, vec in eng.last_scan_tiles()]
    dev = jm.device_fields
    shape = (jm.nx, jm.ny, jm.nz)
    a0 = dev.a0.cpu().numpy().reshape(shape)
    ts = dev.ts.cpu().numpy().reshape(shape)
    tavg = jm._model_tavg().cpu().numpy()
    bursts = (jm._bursts["R"], jm._bursts["B"])
    assert tiles == R.tile_plan_host(times, bursts, nz=jm.nz)
    _, (ctau, cflux) = jm._channel_coeffs(freqs)
    ref = R.ref_sweep(a0, ts, bursts, times)
    # (whether a wave straddles the lobes depends on the geometry: the three-operation figure
    # bounds both recurrences)
    B, _ = R.tile_bound(a0, ts, bursts, times, tiles, ref, (jm.ny + 4) * R.EPS, mixed=True)
    _lc_check(np.asarray(lc), ref, B, tavg, ctau, cflux, "JetModel.flux_vs_time, 13 epochs")


# ---- the diagnostic entry point ----------------------------------------------------------------------------
def test_last_scan_tiles_refusals_and_other_paths(forced):
    """rjp_last_scan_tiles: no tiles on a context before any scan; NULL outputs and a `cap` too small
    are refused (the count is still reported); moment, cached, layout and table scans report none."""
    import ctypes as C
    from rajepy_amd import _lib, engine as E
    from rajepy_amd.engine import RTEngine
    fresh = RTEngine(0)
    try:
        assert fresh.last_scan_tiles() == []
        n = C.c_int32(-1)
        assert fresh.lib.rjp_last_scan_tiles(fresh.ctx, C.byref(n), None, 0) == 0 and n.value == 0
    finally:
        fresh.close()
    eng = forced
    lib = eng.lib
    f = _upload(eng, _host((3, 37, 16), 5400, "halves"), "tau")
    bursts = E.make_bursts(*U.example_burst_lists())
    ep = R.uniform_epochs(45)
    eng.use_moments = False
    eng.ff_scan(f, bursts, ep, MODE, want_em=False, want_tavg=False)
    eng.use_moments = True
    tiles = eng.last_scan_tiles()
    assert [t[1] for t in tiles] == [32, 8, 4, 1]
    n = C.c_int32(-1)
    buf = (C.c_int32 * 20)(*([-7] * 20))
    assert lib.rjp_last_scan_tiles(None, C.byref(n), buf, 4) == _lib.RJP_ERR_ARG
    assert lib.rjp_last_scan_tiles(eng.ctx, None, buf, 4) == _lib.RJP_ERR_ARG
    assert lib.rjp_last_scan_tiles(eng.ctx, C.byref(n), None, 4) == _lib.RJP_ERR_ARG
    assert lib.rjp_last_scan_tiles(eng.ctx, C.byref(n), buf, -1) == _lib.RJP_ERR_ARG
    assert n.value == -1 and list(buf) == [-7] * 20
    assert lib.rjp_last_scan_tiles(eng.ctx, C.byref(n), buf, 3) == _lib.RJP_ERR_ARG     # cap too small
    assert n.value == 4 and list(buf) == [-7] * 20
    assert lib.rjp_last_scan_tiles(eng.ctx, C.byref(n), buf, 4) == 0
    assert [tuple(buf[5 * k:5 * k + 5]) for k in range(4)] == tiles
    # a moment scan, a cached one, the launch-time-ordered layout, the single-epoch table: no tiles
    eng.ff_scan(f, bursts, R.uniform_epochs(32), MODE, want_em=False, want_tavg=False)
    assert eng.last_scan_path()[0] == "moments" and eng.last_scan_tiles() == []
    eng.cache_moments = True
    try:
        eng.ff_scan(f, bursts, R.uniform_epochs(32), MODE, want_em=False, want_tavg=False)
        eng.ff_scan(f, bursts, R.uniform_epochs(32), MODE, want_em=False, want_tavg=False)
        assert eng.last_scan_path()[0] == "cached" and eng.last_scan_tiles() == []
    finally:
        eng.cache_moments = False
        f.mom_cache = None
    eng.build_lt(f, 20)
    eng.ff_scan(f, bursts, R.uniform_epochs(32), MODE, want_em=False, want_tavg=False)
    assert eng.last_scan_path()[0] == "lt" and eng.last_scan_tiles() == []
    f.lt = None
    # ... and a tile scan after them reports its tiles again
    eng.ff_scan(f, bursts, R.uniform_epochs(8), MODE, want_em=False, want_tavg=False)
    assert eng.last_scan_path()[0] == "tiles"
    assert [t[:3] for t in eng.last_scan_tiles()] == [(0, 8, 1)]
    big = eng.synth_fields((64, 72, 512), 5401, 0, 8, csize_au=0.5, wide=False, tau_mode=MODE)
    eng.ff_scan(big, bursts, [1.0 * YEAR], MODE, want_em=False, want_tavg=False)
    assert eng.last_scan_path()[0] == "table" and eng.last_scan_tiles() == []
    eng.synchronize()
