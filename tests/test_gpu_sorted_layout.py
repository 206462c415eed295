"""Single-epoch scans on the launch-time-bucketed layout of (a0, ts) (include/rjprt.h
`rjp_fields.d_srt_cells`; ff_lt.hip builds it, ff_scan_tab.hip reads it): against the grid-order
table scan of the same fields at epochs with none, part or all of the cells inside the bursts'
support, with both jets in one sightline, NaN / zero / infinite cells and occupied y-ranges;
rjp_ff_step equal to rjp_ff_scan + rjp_ff_maps bit for bit; in-place edits detach the layout; the
memory refusal; sampled sightlines of the cfg4-sized map against the oracle."""
import copy

import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
SEED = 20240507
SHAPE = (128, 256, 256)            # 32768 sightlines: the smallest map the table path takes


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    e.cache_moments = False
    yield e
    e.close()


def _example_bursts(only=None):
    """The reference example's four bursts (files/example-model-params.py:51-54); `only` = "R" or
    "B" keeps the bursts of that jet alone."""
    from rajepy_amd import engine as E
    p = U.example_bursts_params()
    red, blue = [], []
    for t0, hl, chi, which in zip(p["t_0"], p["hl"], p["chi"], p["which"]):
        sig = hl * orc.YEAR * 2. / (2. * np.sqrt(2. * np.log(2.)))
        for jet, lst in (("R", red), ("B", blue)):
            if jet in str(which) and (only is None or only == jet):
                lst.append((t0 * orc.YEAR, chi - 1., sig))
    return E.make_bursts(red, blue)


def _scan(eng, fields, bursts, years, sorted_=True):
    eng.use_sorted = sorted_
    try:
        a = eng.ff_scan(fields, bursts, [years * orc.YEAR], fields.a0_mode, want_em=False,
                        want_tavg=False)[0].clone()
    finally:
        eng.use_sorted = True
    path, layout = eng.last_scan_path()[0], eng.last_scan_layout()
    return a, path, layout


def _agree(got, ref, rtol):
    import torch
    torch.cuda.synchronize()
    assert torch.equal(got == 0, ref == 0)
    assert torch.equal(torch.isnan(got), torch.isnan(ref))
    assert torch.equal(torch.isinf(got), torch.isinf(ref))
    ok = torch.isfinite(ref) & (ref != 0)
    rel = ((got - ref).abs()[ok] / ref[ok]).max().item() if ok.any() else 0.0
    assert rel <= rtol, rel
    return rel


@pytest.mark.parametrize("temp_mode", [0, 1])
def test_sorted_layout_vs_grid_order_across_epochs(eng, temp_mode):
    from rajepy_amd import engine as E
    mode = E.RJP_GFF_SCALAR if temp_mode == 0 else E.RJP_GFF_POWERLAW
    fields = eng.synth_fields(SHAPE, SEED, temp_mode, 8, csize_au=0.5, tau_mode=mode)
    assert fields.srt is not None and fields.srt["K"] == 32
    assert fields.srt["rows"] * 64 >= fields.ncells
    bursts = _example_bursts()
    rels = {}
    # partial support (1.0, 0.3 yr), none of the cells (-30, 40 yr: chi == 1 everywhere)
    for years in (1.0, 0.3, -30.0, 40.0):
        got, path, layout = _scan(eng, fields, bursts, years)
        assert (path, layout) == ("table", "sorted"), years
        ref, path_r, layout_r = _scan(eng, fields, bursts, years, sorted_=False)
        assert (path_r, layout_r) == ("table", "grid")
        rels[years] = _agree(got, ref, 1e-13)
    print("max relative difference sorted vs grid order:", rels)
    # at 2.6 yr ~95 % of the cells lie in the support, and with a burst wide enough to cover
    # every launch time all of them: more than 90 % of the layout would be read, so the scan keeps
    # the grid order
    assert _scan(eng, fields, bursts, 2.6)[1:] == ("table", "grid")
    wide = E.make_bursts([(1.0 * orc.YEAR, 2.0, 3.0 * orc.YEAR)], [(1.0 * orc.YEAR, 2.0, 3.0 * orc.YEAR)])
    got, path, layout = _scan(eng, fields, wide, 1.0)
    assert (path, layout) == ("table", "grid")


def test_sorted_layout_both_jets_nan_zero_inf_and_y_ranges(eng):
    """Both jets in one sightline (sign flips along y), NaN / zero / infinite weights, NaN launch
    times -- dropped when their jet has bursts, chi = 1 when it has none (bursts in one jet only:
    the grid-order scan reads the unmasked copy of the launch times, the layout its aux sums)."""
    import torch
    from rajepy_amd import engine as E
    fields = eng.synth_fields(SHAPE, SEED + 1, 1, 8, csize_au=0.5, tau_mode=E.RJP_GFF_SCALAR)
    g = torch.Generator(device=eng.device)
    g.manual_seed(11)
    n = fields.ncells
    r = lambda: torch.rand(n, device=eng.device, generator=g)
    flip = r() < 0.3
    fields.a0[flip] = -fields.a0[flip]
    fields.a0[r() < 0.02] = float("nan")
    fields.a0[r() < 0.02] = 0.0
    fields.ts[r() < 0.02] = float("nan")
    # a few sightlines get an infinite weight (one with a finite, one with a NaN launch time)
    nx, ny, nz = fields.shape
    for (x, y, z, t_nan) in ((3, 10, 5, False), (7, 20, 200, True), (100, 0, 255, False)):
        c = (x * ny + y) * nz + z
        fields.a0[c] = float("inf") * (1 if z >= nz // 2 else -1)
        if t_nan:
            fields.ts[c] = float("nan")
    # an all-NaN sightline and an all-zero one: exact zeros
    for x, z, v in ((5, 7, float("nan")), (6, 9, 0.0)):
        fields.a0[(x * ny + torch.arange(ny, device=eng.device)) * nz + z] = v
    assert eng.build_sorted(fields) is not None
    for only in (None, "R", "B"):
        bursts = _example_bursts(only)
        for years in (1.0, 0.3):
            got, path, layout = _scan(eng, fields, bursts, years)
            assert (path, layout) == ("table", "sorted"), (only, years)
            ref = _scan(eng, fields, bursts, years, sorted_=False)[0]
            _agree(got, ref, 1e-13)
            assert got[0, 5 * nz + 7].item() == 0.0 and got[0, 6 * nz + 9].item() == 0.0
            assert np.isinf(got[0, 3 * nz + 5].item()) and np.isinf(got[0, 100 * nz + 255].item())
    # occupied y-ranges (from the producer): the same maps, and the grid-order scan's same bits
    bursts = _example_bursts()
    free, path, layout = _scan(eng, fields, bursts, 1.0, sorted_=False)
    assert (path, layout) == ("table", "grid")
    eng.compute_y_bounds(fields)
    got, path, layout = _scan(eng, fields, bursts, 1.0)
    assert layout == "sorted"
    ref, path, layout = _scan(eng, fields, bursts, 1.0, sorted_=False)
    assert (path, layout) == ("table", "grid")
    _agree(got, ref, 1e-13)
    assert torch.equal(ref.view(torch.int64), free.view(torch.int64))


def test_ff_step_is_scan_plus_maps_on_the_sorted_layout(eng):
    import torch
    from rajepy_amd import engine as E
    from rajepy_amd.maths import physics as ph
    mode = E.RJP_GFF_SCALAR
    fields = eng.synth_fields(SHAPE, SEED + 2, 0, 8, csize_au=0.5, tau_mode=mode, wide=False,
                              with_em0=False)
    assert fields.srt is not None
    bursts = _example_bursts()
    nu = np.array([1e9, 5e9, 2e10])
    ctau, cflux = E.ff_channel_coeffs(nu, 0.5, 120., mode, [ph.gff(f, 1e4) for f in nu])
    tavg = eng.tavg(fields)
    P, F = fields.npix, len(nu)
    ep = [1.0 * orc.YEAR]
    out = (eng._f64(1, P), None, eng._f64(1, F, P), eng._f64(1, F, P), eng._f64(1, F))
    eng.ff_step(fields, bursts, ep, mode, tavg, ctau, cflux, out)
    assert eng.last_scan_path()[0] == "table" and eng.last_scan_layout() == "sorted"
    sumA = eng.ff_scan(fields, bursts, ep, mode, want_em=False, want_tavg=False)[0]
    assert eng.last_scan_layout() == "sorted"
    tau, flux, ftot = eng.ff_maps(sumA, tavg, ctau, cflux)
    eng.synchronize()
    assert torch.equal(out[0], sumA)
    assert torch.equal(out[2], tau) and torch.equal(out[3], flux) and torch.equal(out[4], ftot)


def test_in_place_edits_detach_the_layout_and_memory_refusal(eng):
    from rajepy_amd import engine as E
    fields = eng.synth_fields(SHAPE, SEED + 3, 0, 8, csize_au=0.5, tau_mode=E.RJP_GFF_SCALAR,
                              wide=False, with_em0=False)
    bursts = _example_bursts()
    assert _scan(eng, fields, bursts, 1.0)[2] == "sorted"
    fields.ts[17] = fields.ts[17] * 0.5                 # same pointer, new version
    got, path, layout = _scan(eng, fields, bursts, 1.0)
    assert (path, layout) == ("table", "grid")
    assert eng.build_sorted(fields) is not None
    assert _scan(eng, fields, bursts, 1.0)[2] == "sorted"
    fields.a0[3] = 2.0 * fields.a0[3]
    assert _scan(eng, fields, bursts, 1.0)[2] == "grid"
    # a rebuilt a0 drops the layout with the other derived state
    assert eng.build_sorted(fields) is not None
    eng._drop_derived_state(fields)
    assert fields.srt is None
    # refusal: the layout would leave less than the required share of HBM free
    eng.srt_min_free = 1.0
    try:
        assert eng.build_sorted(fields) is None and fields.srt is None
        f2 = eng.synth_fields(SHAPE, SEED + 3, 0, 8, csize_au=0.5, tau_mode=E.RJP_GFF_SCALAR,
                              wide=False, with_em0=False)
        assert f2.srt is None
        assert _scan(eng, f2, bursts, 1.0)[1:] == ("table", "grid")
    finally:
        eng.srt_min_free = 0.2
    # A/B switch
    eng.use_sorted = False
    try:
        f3 = eng.synth_fields(SHAPE, SEED + 3, 0, 8, csize_au=0.5, tau_mode=E.RJP_GFF_SCALAR,
                              wide=False, with_em0=False)
        assert f3.srt is None
    finally:
        eng.use_sorted = True


def test_sorted_layout_at_cfg4_size_vs_oracle(eng):
    """512 x 4096 x 512 (the bench's map) on the sorted layout: sampled sightlines against the
    oracle at 1e-10, the whole map against the grid-order scan, at the bench's epoch and at 0.3 yr."""
    from rajepy_amd import engine as E
    from rajepy_amd.maths import physics as ph
    shape = (512, 4096, 512)
    mode = E.RJP_GFF_SCALAR
    fields = eng.synth_fields(shape, SEED, 0, 8, csize_au=0.5, tau_mode=mode, wide=False,
                              with_em0=False)
    assert fields.srt is not None
    nx, ny, nz = shape
    rng = np.random.default_rng(7)
    pix = [(int(rng.integers(nx)), int(rng.integers(nz))) for _ in range(12)]
    pix += [(0, 0), (nx - 1, nz - 1), (17, nz // 2 - 1), (17, nz // 2)]
    idx = [x * nz + z for (x, z) in pix]
    cells = np.array([(x * ny + y) * nz + z for (x, z) in pix for y in range(ny)], dtype=np.uint64)
    g = U.synth_host((len(pix), ny, 1), SEED, 0, cells=cells, nz_full=nz)
    p = copy.deepcopy(U.load_golden("cfg1_example")[2])
    p["ejection"] = U.example_bursts_params()
    p["power_laws"]["q_T"] = 0.
    p["grid"].update(n_x=len(pix), n_y=ny, n_z=1)
    jet = orc.OracleJet.from_fields(p, g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"],
                                    g["rr"], g["vy"])
    bursts = U.bursts_from_oracle(jet)
    ctau, _ = E.ff_channel_coeffs([5e9], 0.5, 120., mode, [ph.gff(5e9, 1e4)])
    for years in (1.0, 0.3):
        got, path, layout = _scan(eng, fields, bursts, years)
        assert (path, layout) == ("table", "sorted")
        ref = _scan(eng, fields, bursts, years, sorted_=False)[0]
        ms = []
        for flag in (True, False):
            eng.use_sorted = flag
            ms.append(eng.time_ff_scan(fields, bursts, [years * orc.YEAR], mode, reps=10,
                                       want_em=False, want_tavg=False))
        eng.use_sorted = True
        print("cfg4, %.1f yr: max relative difference sorted vs grid order %.3g; scan %.3f ms "
              "sorted, %.3f ms grid order" % (years, _agree(got, ref, 1e-13), ms[0], ms[1]))
        jet.time = years * orc.YEAR
        np.testing.assert_allclose(ctau[0] * got.cpu().numpy()[0, idx],
                                   jet.optical_depth_ff(5e9)[:, 0], rtol=1e-10)
