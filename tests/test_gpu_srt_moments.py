"""Single-epoch scans that contract the launch-time bins where chi^2 is smooth from the bucketed
layout's Chebyshev moments (include/rjprt.h `rjp_fields.d_srt_mom`; ff_lt.hip builds them,
ff_scan_tab.hip contracts them): the moments against a host f64 restatement; the hybrid scan
against the moment-free sorted scan and the grid order at 1.0 and 0.3 yr, with NaN / zero /
infinite cells and both jets in one sightline; the bin counters (contracted bins at the bench
epoch, none for a burst too narrow for any bin); in-place edits never reach stale moments; the
memory refusal of the moments alone; sampled cfg4 sightlines against the oracle."""
import copy

import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
SEED = 20240611
SHAPE = (128, 2048, 256)           # 32768 sightlines of 2048 cells: ~64 cells per bin and lane


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


def _scan(eng, fields, bursts, years, sorted_=True, moments=True):
    eng.use_sorted, eng.use_srt_moments = sorted_, moments
    try:
        a = eng.ff_scan(fields, bursts, [years * orc.YEAR], fields.a0_mode, want_em=False,
                        want_tavg=False)[0].clone()
    finally:
        eng.use_sorted = eng.use_srt_moments = True
    return a, eng.last_scan_layout(), eng.last_srt_bins()


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


def _three_ways(eng, fields, bursts, years):
    """hybrid vs moment-free sorted vs grid order: patterns equal, <= 1e-13 relative."""
    got, lay, bins = _scan(eng, fields, bursts, years)
    assert lay == "sorted", years
    plain, lay_p, bins_p = _scan(eng, fields, bursts, years, moments=False)
    assert lay_p == "sorted" and bins_p == (0, 0)
    grid, lay_g, _ = _scan(eng, fields, bursts, years, sorted_=False)
    assert lay_g == "grid"
    return got, bins, _agree(got, plain, 1e-13), _agree(got, grid, 1e-13)


def test_moments_vs_host_restatement(eng):
    from rajepy_amd import engine as E
    fields = eng.synth_fields((64, 512, 512), SEED, 0, 8, csize_au=0.5,
                              tau_mode=E.RJP_GFF_SCALAR, wide=False, with_em0=False)
    srt = fields.srt
    assert srt is not None and srt["mom"] is not None and srt["N"] == eng.srt_N
    K, N, P = srt["K"], srt["N"], fields.npix
    lo, hi = fields.ts_range
    inv_h = K / (hi - lo)
    start = srt["start"].cpu().numpy().reshape(2 * K + 1, P)
    cum = srt["cum"].cpu().numpy().reshape(2 * K + 1, P)
    rowbase = srt["rowbase"].cpu().numpy()
    mom = srt["mom"].view(2 * K, N - 1, P)
    rng = np.random.default_rng(3)
    for p in [0, 63, 64, P - 1] + [int(v) for v in rng.integers(P, size=6)]:
        g, lane = divmod(p, 64)
        n_cells = int(start[2 * K, p])
        rows = srt["cells"].view(-1, 64, 2)[int(rowbase[g]):int(rowbase[g]) + n_cells, lane]
        a, t = rows[:, 0].cpu().numpy(), rows[:, 1].cpu().numpy()
        got = mom[:, :, p].cpu().numpy()
        for q in range(2 * K):
            s0, s1 = int(start[q, p]), int(start[q + 1, p])
            w = (t[s0:s1] - lo) * inv_h
            k = np.clip(np.floor(w), 0, K - 1)
            assert np.all(k == q % K)
            x = 2.0 * (w - k) - 1.0
            T = np.polynomial.chebyshev.chebvander(x, N - 1)        # [cells, N]
            ref = a[s0:s1] @ T[:, 1:]
            scale = a[s0:s1].sum()
            # (M_0, the prefix-sum step: exact to rounding of the sightline's total)
            assert abs(scale - (cum[q + 1, p] - cum[q, p])) <= 1e-13 * cum[2 * K, p]
            assert np.all(np.abs(got[q] - ref) <= 1e-13 * scale), (p, q)


@pytest.mark.parametrize("temp_mode", [0, 1])
def test_hybrid_vs_sorted_vs_grid_order(eng, temp_mode):
    from rajepy_amd import engine as E
    mode = E.RJP_GFF_SCALAR if temp_mode == 0 else E.RJP_GFF_POWERLAW
    fields = eng.synth_fields(SHAPE, SEED, temp_mode, 8, csize_au=0.5, tau_mode=mode,
                              wide=False, with_em0=False)
    assert fields.srt is not None and fields.srt["mom"] is not None
    bursts = _example_bursts()
    out = {}
    for years in (1.0, 0.3):
        _, bins, rel_p, rel_g = _three_ways(eng, fields, bursts, years)
        out[years] = (bins, rel_p, rel_g)
        assert bins[0] > 0, (years, bins)
    print("hybrid: (contracted, read) bins, rel. difference vs sorted, vs grid order:", out)


def test_hybrid_both_jets_nan_zero_inf(eng):
    """Both jets in one sightline (sign flips along y), NaN / zero / infinite weights, NaN launch
    times, bursts in both jets or one only."""
    import torch
    from rajepy_amd import engine as E
    fields = eng.synth_fields(SHAPE, SEED + 1, 1, 8, csize_au=0.5, tau_mode=E.RJP_GFF_SCALAR,
                              wide=False, with_em0=False)
    g = torch.Generator(device=eng.device)
    g.manual_seed(12)
    n = fields.ncells
    r = lambda: torch.rand(n, device=eng.device, generator=g)
    nx, ny, nz = fields.shape
    # a quarter of the sightlines get cells of both jets (the groups of the others stay single-jet)
    col = torch.arange(n, device=eng.device) % nz
    flip = (r() < 0.3) & (col < nz // 4)
    fields.a0[flip] = -fields.a0[flip]
    fields.a0[r() < 0.02] = float("nan")
    fields.a0[r() < 0.02] = 0.0
    fields.ts[r() < 0.02] = float("nan")
    for (x, y, z, t_nan) in ((3, 10, 5, False), (7, 20, 200, True), (100, 0, 255, False)):
        c = (x * ny + y) * nz + z
        fields.a0[c] = float("inf") * (1 if z >= nz // 2 else -1)
        if t_nan:
            fields.ts[c] = float("nan")
    for x, z, v in ((5, 7, float("nan")), (6, 9, 0.0)):
        fields.a0[(x * ny + torch.arange(ny, device=eng.device)) * nz + z] = v
    assert eng.build_sorted(fields) is not None and fields.srt["mom"] is not None
    for only in (None, "R", "B"):
        bursts = _example_bursts(only)
        for years in (1.0, 0.3):
            got, bins, _, _ = _three_ways(eng, fields, bursts, years)
            assert bins[0] > 0, (only, years, bins)
            assert got[0, 5 * nz + 7].item() == 0.0 and got[0, 6 * nz + 9].item() == 0.0
            assert np.isinf(got[0, 3 * nz + 5].item()) and np.isinf(got[0, 100 * nz + 255].item())


def test_narrow_burst_contracts_nothing(eng):
    """A burst far narrower than a bin, its whole support inside one bin of each jet: no
    interpolant of degree N - 1 passes, that bin is read, and the maps are the moment-free scan's
    bit for bit."""
    import torch
    from rajepy_amd import engine as E
    fields = eng.synth_fields(SHAPE, SEED + 2, 0, 8, csize_au=0.5, tau_mode=E.RJP_GFF_SCALAR,
                              wide=False, with_em0=False)
    yr = orc.YEAR
    lo, hi = fields.ts_range
    h = (hi - lo) / fields.srt["K"]
    # both peaks launched at the centre of bin 12 (+-9 sigma of support: 0.45 bins; one short
    # table for both jets)
    t0 = 1.0 * yr - (lo + 12.5 * h)
    narrow = E.make_bursts([(t0, 5.0, h / 40)], [(t0, 3.0, h / 40)])
    got, lay, bins = _scan(eng, fields, narrow, 1.0)
    assert lay == "sorted" and bins[0] == 0 and bins[1] > 0, bins
    plain = _scan(eng, fields, narrow, 1.0, moments=False)[0]
    torch.cuda.synchronize()
    assert torch.equal(got, plain)
    _agree(got, _scan(eng, fields, narrow, 1.0, sorted_=False)[0], 1e-13)


def test_stale_moments_never_used_and_memory_refusal(eng):
    import torch
    from rajepy_amd import engine as E
    fields = eng.synth_fields(SHAPE, SEED + 3, 0, 8, csize_au=0.5, tau_mode=E.RJP_GFF_SCALAR,
                              wide=False, with_em0=False)
    bursts = _example_bursts()
    assert _scan(eng, fields, bursts, 1.0)[2][0] > 0
    # an in-place edit: neither the layout nor its moments are attached any more ...
    fields.a0[:: 7] = 3.0 * fields.a0[:: 7]
    got, lay, bins = _scan(eng, fields, bursts, 1.0)
    assert lay == "grid" and bins == (0, 0)
    ref = _scan(eng, fields, bursts, 1.0, sorted_=False)[0]
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    # ... until they are rebuilt from the edited fields
    assert eng.build_sorted(fields)["mom"] is not None
    got, lay, bins = _scan(eng, fields, bursts, 1.0)
    assert lay == "sorted" and bins[0] > 0
    _agree(got, ref, 1e-13)
    fields.ts[5] = fields.ts[5] * 0.5
    assert _scan(eng, fields, bursts, 1.0)[1] == "grid"
    # refusal of the moments alone: the layout fits the srt_min_free rule, its moments do not
    srt = eng.build_sorted(fields)
    need, mom_bytes = srt["bytes"], srt["mom_bytes"]
    assert mom_bytes == 2 * srt["K"] * (srt["N"] - 1) * fields.npix * 8
    fields.srt = srt = None
    free, hbm = torch.cuda.mem_get_info(eng.device)
    free += torch.cuda.memory_reserved(eng.device) - torch.cuda.memory_allocated(eng.device)
    eng.srt_min_free = (free - need - mom_bytes / 2) / hbm
    try:
        srt = eng.build_sorted(fields)
    finally:
        eng.srt_min_free = 0.2
    assert srt is not None and srt["mom"] is None and srt["N"] == 0 and srt["mom_bytes"] == 0
    got, lay, bins = _scan(eng, fields, bursts, 1.0)
    assert lay == "sorted" and bins == (0, 0)
    _agree(got, _scan(eng, fields, bursts, 1.0, sorted_=False)[0], 1e-13)
    # the A/B switch: no moments built
    eng.use_srt_moments = False
    try:
        assert eng.build_sorted(fields)["mom"] is None
    finally:
        eng.use_srt_moments = True


def test_hybrid_at_cfg4_size_vs_oracle(eng):
    """512 x 4096 x 512 (the bench's map): sampled sightlines against the oracle at 1e-10, the
    whole map against the moment-free sorted scan and the grid order, at 1.0 and 0.3 yr."""
    from rajepy_amd import engine as E
    from rajepy_amd.maths import physics as ph
    shape = (512, 4096, 512)
    mode = E.RJP_GFF_SCALAR
    fields = eng.synth_fields(shape, SEED, 0, 8, csize_au=0.5, tau_mode=mode, wide=False,
                              with_em0=False)
    assert fields.srt is not None and fields.srt["mom"] is not None
    print("cfg4 moments: N = %d, %.2f GB, built in %.2f ms" % (
        fields.srt["N"], fields.srt["mom_bytes"] / 1e9, fields.srt["mom_build_ms"]))
    nx, ny, nz = shape
    rng = np.random.default_rng(8)
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
        got, bins, rel_p, rel_g = _three_ways(eng, fields, bursts, years)
        assert bins[0] > 0
        print("cfg4, %.1f yr: (contracted, read) %s, rel. difference vs sorted %.3g, vs grid "
              "order %.3g" % (years, bins, rel_p, rel_g))
        jet.time = years * orc.YEAR
        np.testing.assert_allclose(ctau[0] * got.cpu().numpy()[0, idx],
                                   jet.optical_depth_ff(5e9)[:, 0], rtol=1e-10)
