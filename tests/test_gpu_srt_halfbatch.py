"""The cell loop of the bucketed single-epoch scans (ff_scan_sorted_kernel, ff_scan_hybrid_kernel;
ff_scan_tab.hip) streams a wave's window in batches of 8 rows; a lane loads and sums the rows of
its own run only.  This test was written with a variant of that loop whose batches travel as two
halves of 4 (one summed while the other is in flight); the variant did not pay and is not in the
library, the test stays for whatever loop is: a row summed from the wrong
slot of a batch, a load that overtakes its sum, or a row outside a lane's run fetched after all
shows here.

Map: 128 x 320 x 256 (32768 sightlines: the smallest the table path takes), the launch times
written here.  One burst far narrower than a launch-time bin (test_gpu_srt_ragged's): the scans
read bin 12 of both jets cell by cell and contract nothing.  In every group of 64 sightlines the
lanes' runs in that bin have every length from 0 to 17 rows -- shorter than half a batch, between
half a batch and a batch, past two batches -- and start at row offsets 0 .. 7 of the wave's window
(the cells a lane holds in earlier bins: 40 + offset).  The lanes 40 .. 63 of the last group hold no
cell of bin 12 at all (32768 sightlines are whole groups; a second map, 131 x 320 x 254, ends in a
group of 58 sightlines and 6 lanes past the map).  Every cell of the layout outside a lane's own
run is overwritten with NaN, as tests/test_gpu_srt_ragged.py does.

Checks: the hybrid scan and the moment-free scan against tests/gpu_util.ref_single_epoch within
single_epoch_bound(n_y) (derived in tests/test_gpu_single_epoch_reference.py), and, nothing being
contracted, the hybrid scan equal to the moment-free one bit for bit."""
import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
YEAR = orc.YEAR
SEED = 20261021
NY = 320
FULL = (128, NY, 256)
LAST58 = (131, NY, 254)           # 33274 = 519 x 64 + 58
BIN = 12
BEFORE = 40                       # cells of every lane in the bins before BIN, + its offset


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    e.cache_moments = False
    yield e
    e.close()


def run_lengths(P):
    """-> (rows of the lane's run in BIN, its offset in the wave's window), per sightline"""
    p = np.arange(P)
    g, lane = p // 64, p % 64
    length = (5 * lane + g) % 18                   # every length 0 .. 17 in every full group
    offset = (3 * lane + g) % 8                    # every offset 0 .. 7
    last = g == (P - 1) // 64
    length[last & (lane >= 40)] = 0
    return length, offset


def write_launch_times(ts, ts_range, K, rng):
    """[n_x, n_y, n_z] in place: per sightline BEFORE + offset cells in bins 0 .. BIN - 1, `length`
    cells in BIN, the rest in the bins behind it, in random order along y.  The range stays what
    it was: one cell keeps its lower and one its upper end."""
    nx, ny, nz = ts.shape
    P = nx * nz
    lo, hi = ts_range
    h = (hi - lo) / K
    length, offset = run_lengths(P)
    n0 = (BEFORE + offset)[:, None]
    n1 = n0 + length[:, None]
    y = np.arange(ny)[None, :]
    col = np.where(y < n0, lo + rng.uniform(0.02, BIN - 0.05, (P, ny)) * h,
                   np.where(y < n1, lo + (BIN + rng.uniform(0.05, 0.95, (P, ny))) * h,
                            lo + rng.uniform(BIN + 1.05, K - 0.05, (P, ny)) * h))
    col[0, 0], col[0, ny - 1] = lo, hi
    col = rng.permuted(col, axis=1)
    ts[:] = col.reshape(nx, nz, ny).transpose(0, 2, 1)
    return length, offset


class Model:
    def __init__(self, eng, shape, seed):
        import torch
        from rajepy_amd import engine as E
        self.eng, self.shape, self.mode = eng, shape, E.RJP_GFF_SCALAR
        f = eng.synth_fields(shape, seed, 0, 8, csize_au=0.5, tau_mode=self.mode, wide=False,
                             with_em0=False)
        self.K = 32
        self.ts_range = eng.launch_time_range(f)
        ts = f.ts.cpu().numpy().reshape(shape).copy()
        self.length, self.offset = write_launch_times(ts, self.ts_range, self.K,
                                                      np.random.default_rng(seed))
        f.ts.copy_(torch.from_numpy(ts.ravel()).to(eng.device))
        srt = eng.build_sorted(f)
        assert srt is not None and srt["mom"] is not None and srt["K"] == self.K and srt["N"] == 20
        assert eng.launch_time_range(f) == self.ts_range
        self.fields, self.srt = f, srt
        self.a0, self.ts = f.a0.cpu().numpy().reshape(shape), ts
        self.hist = [int(v) for v in srt["hist"]]
        lo, hi = self.ts_range
        h = (hi - lo) / self.K
        t0 = 1.0 * YEAR - (lo + (BIN + 0.5) * h)
        self.bursts = ([(t0, 5.0, h / 40)], [(t0, 3.0, h / 40)])
        self.t = 1.0 * YEAR


def poison_outside_runs(m, plan):
    """(NaN, NaN) into every cell of the layout outside [start(b0), start(b1)) of its lane for
    both jets, the padding rows included; -> the number of cells kept."""
    import torch
    srt, K, P = m.srt, m.K, m.fields.npix
    dev = srt["cells"].device
    cells = srt["cells"].view(-1, 64, 2)
    rowbase = srt["rowbase"].long()
    G = rowbase.numel() - 1
    start = torch.zeros(2 * K + 1, G * 64, dtype=torch.int64, device=dev)
    start[:, :P] = srt["start"].view(2 * K + 1, P).long()
    R = torch.arange(cells.shape[0], device=dev)
    g = torch.bucketize(R, rowbase[1:].contiguous(), right=True).clamp(max=G - 1)
    r = (R - rowbase[g])[:, None]
    p = g[:, None] * 64 + torch.arange(64, device=dev)[None, :]
    keep = torch.zeros_like(p, dtype=torch.bool)
    for j in range(2):
        b0, b1 = plan["b0"][j], plan["b1"][j]
        keep |= (r >= start[j * K + b0][p]) & (r < start[j * K + b1][p])
    cells[~keep] = float("nan")
    return int(keep.sum().item())


def scan(m, moments):
    from rajepy_amd import engine as E
    eng = m.eng
    eng.use_srt_moments = moments
    try:
        a = eng.ff_scan(m.fields, E.make_bursts(*m.bursts), [m.t], m.mode, want_em=False,
                        want_tavg=False)[0].clone()
    finally:
        eng.use_srt_moments = True
    eng.synchronize()
    assert not eng.range_guard()
    assert eng.last_scan_path()[0] == "table" and eng.last_scan_layout() == "sorted"
    return a[0], eng.last_srt_bins()


@pytest.mark.parametrize("shape", [FULL, LAST58], ids=["full", "last58"])
def test_runs_of_every_length_and_offset(eng, shape):
    import torch
    m = Model(eng, shape, SEED + shape[0])
    P = m.fields.npix
    plan = U.srt_plan_host(m.hist, m.ts_range, m.K, m.bursts, m.t)
    assert plan["layout"] == "sorted" and plan["b0"] == [BIN, BIN] and plan["b1"] == [BIN + 1] * 2, plan
    # the layout holds the runs this test means: per lane `length` rows, the first of them
    # BEFORE + offset rows into the lane's column of the group, whichever jet the lane is in
    start = m.srt["start"].cpu().numpy().reshape(2 * m.K + 1, P).astype(np.int64)
    run = (start[BIN + 1] - start[BIN]) + (start[m.K + BIN + 1] - start[m.K + BIN])
    assert np.array_equal(run, m.length)
    red = start[BIN + 1] > start[BIN]
    first = np.where(red, start[BIN], start[m.K + BIN])
    grp = np.arange(P) // 64
    last = (P - 1) // 64
    for g in (0, 1, 17, last // 2, last):
        in_g = grp == g
        if g != last:
            assert set(run[in_g].tolist()) == set(range(18)), g
        else:
            assert (run[in_g][40:] == 0).all() and in_g.sum() == (64 if shape == FULL else 58)
        for jet in (red, ~red):                    # (a wave's window is one jet's)
            sel = in_g & (run > 0) & jet
            if sel.sum() >= 32:
                off = first[sel] - first[sel].min()
                assert set(off.tolist()) == set(range(8)), (g, sorted(set(off.tolist())))
    kept = poison_outside_runs(m, plan)
    assert kept == int(run.sum())
    ref = U.ref_single_epoch(m.a0, m.ts, m.bursts, m.t).ravel()
    hyb, bins = scan(m, True)
    srt, bins_s = scan(m, False)
    assert bins[0] == 0 and bins[1] > 0 and bins_s == (0, 0), (bins, bins_s)
    rel_h = U.against(hyb.cpu().numpy(), ref, U.single_epoch_bound(NY), (shape, "hybrid"))
    rel_s = U.against(srt.cpu().numpy(), ref, U.single_epoch_bound(NY), (shape, "sorted"))
    print("%s: rel. hybrid %.2e sorted %.2e, %d cells kept" % (shape, rel_h, rel_s, kept))
    assert torch.equal(hyb.view(torch.int64), srt.view(torch.int64))
