"""Launch-time codes of the packed state on the device (srt_codes_kernel in ff_lt.hip; the residual
stream of ff_scan_hybrid_kernel with rjp_fields.d_srt_pc attached): a table-residual bin streams a
32-bit code of the launch time and the 16-bit weight, 6 bytes per cell instead of 10, and a cell
whose code cannot decide the table piece is re-read from the layout's cells.  The arithmetic, the
margin and the expected share of such cells are restated in tests/test_srt_codes_cpu.py.

Bounds.  Codes on against codes off, per sightline: 2^-51 relative.  Both runs add the same terms
in the same order; a cell decided from its code moves its term by < 2e-18 of itself
(tests/test_srt_codes_cpu.py), and the residual sum is <= 2.2e-13 of the sightline's, so the two
sums can differ by a last rounding in each of the two additions that follow the residual sum.
Against tests/gpu_util.ref_single_epoch: single_epoch_bound(n_y), as every single-epoch scan.
Fallback cells of launch times drawn evenly into the residual bins: at most ten times the
restatement's share (2 mg per unit of w, 2.4e-7 here) of the cells streamed -- a condition.

The maps are the smallest the table path takes, drawn as tests/test_gpu_srt_residual.py draws them
(its Model and helpers are imported, not changed)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import gpu_util as U
from tests import test_gpu_srt_residual as G
from tests import test_srt_codes_cpu as Cc

pytestmark = pytest.mark.gpu
YEAR, K, N, R = G.YEAR, G.K, G.N, G.R
SEED = 20261021
ONOFF_RTOL = 2.0 ** -51
S320, S480, ODD = G.S320, G.S480, G.ODD
GOLDEN_OFF = os.path.join(U.GOLDEN, "srt_codes_off_s320_1yr.npy")
GOLDEN_SEED = SEED + 21


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    e.cache_moments = False
    yield e
    e.close()


_models = {}


@pytest.fixture(scope="module")
def model(eng):
    def get(shape):
        if shape not in _models:
            _models[shape] = G.Model(eng, shape, SEED + shape[0] + shape[1])
        return _models[shape]
    yield get
    _models.clear()


def scan(m, bursts, t, codes=True):
    """-> (map [P] on the device, (contracted, read), residual bins, fallback cells, the struct
    had the codes attached)"""
    from rajepy_amd import engine as E
    eng = m.eng
    eng.use_srt_codes = codes
    try:
        hb = E.make_bursts(*bursts)
        attached = bool(eng._scan_struct(m.fields, hb, 1).d_srt_pc)
        a = eng.ff_scan(m.fields, hb, [t], m.mode, want_em=False, want_tavg=False)[0].clone()
    finally:
        eng.use_srt_codes = True
    eng.synchronize()
    assert not eng.range_guard()
    assert eng.last_scan_path()[0] == "table" and eng.last_scan_layout() == "sorted"
    return a[0], eng.last_srt_bins(), eng.last_srt_resid(), eng.last_srt_fallbacks(), attached


def bits(a):
    import torch
    return a.view(torch.int64)


def stream_cells(m, bursts, t):
    """Host: the cells of the (group, jet, bin) triples that can be residual (Model.cap's rule) --
    an upper bound on the cells the residual stream reads; -> (cells, per-sightline counts of the
    residual bins [jet][bin] -> [P])."""
    held, longest = m.stats
    cnt = np.diff(m.start.astype(np.int64), axis=0)              # [2 K, P]
    P = cnt.shape[1]
    grp = np.arange(P) // 64
    cells, per = 0, {}
    for j in range(2):
        for b in G.res_bins(bursts, t)[j]:
            taken = held[j] & (longest[j * K + b] * 6 > (N - 1) * 8)
            per[(j, b)] = np.where(taken[grp], cnt[j * K + b], 0)
            cells += int(per[(j, b)].sum())
    return cells, per


def host_fallbacks(m, bursts, t):
    """Host: (the cells the restatement calls ambiguous, all cells) of the (group, jet, bin)
    triples stream_cells() counts, from the model's own arrays."""
    ni, lo, inv_h, _ = R.S.chi_table(bursts, R.TS_RANGE, t)
    A, B, mg, _, _ = Cc.code_params(t, R.TS_RANGE, lo, inv_h)
    held, longest = m.stats
    nx, ny, nz = m.shape
    a0, ts = m.a0, m.ts
    kept = (np.abs(a0) > 0) & np.isfinite(a0) & ~np.isnan(ts)
    lo_t, hi_t = R.TS_RANGE
    binw = np.clip(np.floor((ts - lo_t) * (K / (hi_t - lo_t))), 0, K - 1)
    grp = (np.arange(nx * nz) // 64).reshape(nx, 1, nz)
    red = np.signbit(a0)
    amb = cells = 0
    for j in range(2):
        for b in G.res_bins(bursts, t)[j]:
            taken = held[j] & (longest[j * K + b] * 6 > (N - 1) * 8)
            sel = kept & (red if j == 0 else ~red) & (binw == b) & taken[grp]
            cells += int(sel.sum())
            amb += int(Cc.coded_lookup(Cc.encode(ts[sel], R.TS_RANGE), A, B, mg, ni)[2].sum())
    return amb, cells


# ---- 1, 4: codes on against codes off and the reference; the fallback share of an even draw -----
@pytest.mark.parametrize("years", [1.0, 0.3])
@pytest.mark.parametrize("shape", [S320, S480, ODD], ids=["320", "480", "dead_lanes"])
def test_codes_on_against_codes_off_and_the_reference(model, shape, years):
    m = model(shape)
    assert m.srt["packed"] is not None and m.srt["packed"]["pc"] is not None
    bursts, t = U.example_burst_lists(), years * YEAR
    on, bins_on, res_on, fb_on, att_on = scan(m, bursts, t)
    off, bins_off, res_off, fb_off, att_off = scan(m, bursts, t, codes=False)
    assert att_on and not att_off
    assert bins_on == bins_off and res_on == res_off and res_on > 0, (bins_on, bins_off, res_on, res_off)
    assert fb_off == 0
    a, b = on.cpu().numpy(), off.cpu().numpy()
    rel = U.against(a, b, np.inf, (shape, years, "on / off"))
    print("%s, %.1f yr: codes on / off worst rel. %.3e (<= 2^-51 = %.3e), %d sightlines differ"
          % (shape, years, rel, ONOFF_RTOL, int((a != b).sum())))
    assert rel <= ONOFF_RTOL, (shape, years, rel)
    ny = shape[1]
    rel_ref = U.against(a, m.ref(bursts, t), U.single_epoch_bound(ny), (shape, years, "reference"))
    # the even draw: fallbacks against ten times the derived share of the cells streamed
    ni, lo, inv_h, _ = R.S.chi_table(bursts, R.TS_RANGE, t)
    share = Cc.fallback_share(t, R.TS_RANGE, lo, inv_h)
    cells, _ = stream_cells(m, bursts, t)
    print("%s, %.1f yr: reference %.2e (<= %.2e); residual bins %d, <= %d cells streamed, "
          "%d fell back (derived share %.3g: %.2f expected, cap %.1f)"
          % (shape, years, rel_ref, U.single_epoch_bound(ny), res_on, cells, fb_on, share,
             share * cells, 10 * share * cells))
    assert cells > 1_000_000
    assert fb_on <= 10.0 * share * cells, (fb_on, share, cells)
    # ... and no more than the restatement finds among those cells (an upper bound like `cells`:
    # the device takes a bin as residual on its own verdict)
    assert fb_on <= host_fallbacks(m, bursts, t)[0]


# ---- 2: all launch times equal ---------------------------------------------------------------------
@pytest.mark.parametrize("where", ["inside", "boundary", "one code step beside"])
def test_all_launch_times_equal(eng, where):
    """Every cell the scan reads (but one sightline's, which spans the range) launched at the same
    time in a bin that is residual for the red jet: inside a table piece no cell falls back; on a
    piece boundary of the epoch's table, or one code step beside it, every one does, and the map
    of those sightlines is the 10-byte path's bit for bit."""
    bursts, t = U.example_burst_lists(), 1.0 * YEAR
    ni, lo, inv_h, _ = R.S.chi_table(bursts, R.TS_RANGE, t)
    q = Cc.code_params(t, R.TS_RANGE, lo, inv_h)[4]
    rb = G.res_bins(bursts, t)[0]
    b = rb[len(rb) // 2]
    h = 5.0 * YEAR / K
    k = int(np.floor((t - (b + 0.5) * h - lo) * inv_h))
    ts0 = t - lo - k / inv_h                                     # w = k exactly (to a rounding)
    if where == "inside":
        ts0 -= 0.37 / inv_h
    elif where != "boundary":
        ts0 += q
    assert b * h < ts0 < (b + 1) * h
    m = G.Model(eng, S320, SEED + 5, ts_fn=G._equal_ts(ts0), both_jets=False)
    on, bins_on, res_on, fb_on, _ = scan(m, bursts, t)
    off, bins_off, res_off, _, _ = scan(m, bursts, t, codes=False)
    assert bins_on == bins_off and res_on == res_off and res_on > 0
    # the host's count: what the restatement calls ambiguous among the cells of every (group, jet,
    # bin) the residual stream takes -- all of the cells at ts0, or none of them
    want, cells = host_fallbacks(m, bursts, t)
    n_y = S320[1]
    assert cells > 1_000_000
    print("equal, %s: %d residual bins, %d cells streamed, fallbacks %d (host: %d)"
          % (where, res_on, cells, fb_on, want))
    # (all but the spanning sightline's own cells are at ts0)
    assert (want < 10) if where == "inside" else (cells - n_y <= want <= cells), (where, want, cells)
    assert fb_on == want, (where, fb_on, want)
    others = np.arange(m.fields.npix) != 1                       # ts[0, :, 1] spans the range
    a, c = on.cpu().numpy(), off.cpu().numpy()
    rel = U.against(a, c, ONOFF_RTOL, ("equal", where))
    print("equal, %s: on / off worst rel. %.3e" % (where, rel))
    if where != "inside":
        assert np.array_equal(a[others].view(np.int64), c[others].view(np.int64))
    U.against(a, m.ref(bursts, t), U.single_epoch_bound(S320[1]), ("equal", where, "reference"))


# ---- 3: poison -------------------------------------------------------------------------------------
def test_rows_outside_the_residual_runs_are_never_re_read(eng):
    """NaN in every row of `cells` that no path of this scan may read for its lane -- outside the
    lane's runs of the residual bins and of the bins its group reads cell by cell (a run of at most
    9 rows cannot be contracted: 16 B x 9 <= 8 B x 19), so the contracted bins beside a residual
    run and the padding are all poisoned -- and the saturated code, which always asks for the
    fallback, in every code outside the residual runs: the map does not change by a bit and no
    further cell falls back."""
    import torch
    m = G.Model(eng, S320, SEED + 11)
    bursts, t = U.example_burst_lists(), 1.0 * YEAR
    clean, _, n_clean, fb_clean, att = scan(m, bursts, t)
    assert att and n_clean > 0
    srt, P = m.srt, m.fields.npix
    dev = srt["cells"].device
    rowbase = srt["rowbase"].long()
    Gn = rowbase.numel() - 1
    start = torch.zeros(2 * K + 1, Gn * 64, dtype=torch.int64, device=dev)
    start[:, :P] = srt["start"].view(2 * K + 1, P).long()
    longest = torch.from_numpy(m.stats[1]).to(dev)               # [2 K, G]
    plan = U.srt_plan_host([0] * (2 * K), R.TS_RANGE, K, bursts, t)
    resb = G.res_bins(bursts, t)

    def runs(first_row, n_rows, only_res):
        """[n_rows, 64] bool per absolute row: the row lies in a run the scan may read"""
        Rr = torch.arange(n_rows, device=dev)
        g = torch.bucketize(Rr, first_row.contiguous(), right=True) - 1
        r = (Rr - first_row[g])[:, None]
        p = g[:, None] * 64 + torch.arange(64, device=dev)[None, :]
        keep = torch.zeros_like(p, dtype=torch.bool)
        for j in range(2):
            for b in range(plan["b0"][j], plan["b1"][j]):
                mine = (r >= start[j * K + b][p]) & (r < start[j * K + b + 1][p])
                if b in resb[j]:
                    keep |= mine
                elif not only_res:
                    keep |= mine & (longest[j * K + b][g] <= 9)[:, None]
        return keep
    n_cell_rows = srt["cells"].numel() // 128
    keep_cells = runs(rowbase[:-1], n_cell_rows, False)
    prow = ((rowbase[:-1] + 7) // 8) * 8 + 8 * torch.arange(Gn, device=dev)
    rows = srt["packed"]["rows"]
    keep_codes = runs(prow, rows, True)
    assert 0 < int(keep_cells.sum()) < keep_cells.numel() and 0 < int(keep_codes.sum())
    version = srt["cells"]._version
    srt["cells"].view(n_cell_rows, 64, 2)[~keep_cells] = float("nan")
    assert srt["cells"]._version != version
    srt["packed"]["version"] = srt["cells"]._version            # (the poison is no edit of the model)
    pc = srt["packed"]["pc"].view(rows // 4, 64, 4)
    pc[~keep_codes.view(rows // 4, 4, 64).transpose(1, 2)] = -1  # 0xffffffff
    got, _, n_res, fb, att = scan(m, bursts, t)
    assert att and n_res == n_clean
    assert fb == fb_clean, (fb, fb_clean)
    assert torch.equal(bits(got), bits(clean))


# ---- 5: detaching, refusal of the packed state, the switch -----------------------------------------
def test_cells_edited_in_place_detach_the_codes_with_the_packed_state(eng):
    m = G.Model(eng, S320, SEED + 17)
    bursts, t = U.example_burst_lists(), 1.0 * YEAR
    _, _, n_res, _, att = scan(m, bursts, t)
    assert att and n_res > 0
    m.srt["cells"].mul_(1.0)                     # (the same values: only the version moves)
    _, _, n_res, fb, att = scan(m, bursts, t)
    assert not att and n_res == 0 and fb == 0
    eng._drop_derived_state(m.fields)
    assert m.fields.srt is None


def test_a_refused_packed_state_has_no_codes(eng):
    import torch

    def huge(a0):
        a0[3, 7, 5] = 1e39
    m = G.Model(eng, S320, SEED + 13, a0_edit=huge)
    assert m.srt["packed"] is None
    bursts, t = U.example_burst_lists(), 1.0 * YEAR
    on, _, n_res, fb, att = scan(m, bursts, t)
    off, _, _, _, _ = scan(m, bursts, t, codes=False)
    assert not att and n_res == 0 and fb == 0
    assert torch.equal(bits(on), bits(off))


def test_the_switch_off_runs_the_ten_byte_path_of_a_build_without_the_codes(eng):
    """`use_srt_codes = False` against the map of the same model recorded from a library built with
    -DRJP_SRT_CODES=0 (tests/golden/srt_codes_off_s320_1yr.npy; tools/srt_hybrid_ab.py holds that
    build bit-equal to the parent commit's on the bench's model): bit for bit.  And a model built
    with the switch off carries no codes."""
    m = G.Model(eng, S320, GOLDEN_SEED)
    bursts, t = U.example_burst_lists(), 1.0 * YEAR
    off, _, n_res, fb, att = scan(m, bursts, t, codes=False)
    assert not att and n_res > 0 and fb == 0
    gold = np.load(GOLDEN_OFF)
    assert np.array_equal(off.cpu().numpy().view(np.int64), gold.view(np.int64))
    eng.use_srt_codes = False
    try:
        srt = eng.build_sorted(m.fields)
    finally:
        eng.use_srt_codes = True
    assert srt["packed"] is not None and srt["packed"]["pc"] is None
    again, _, n2, fb2, att2 = scan(m, bursts, t)
    assert not att2 and n2 == n_res and fb2 == 0
    assert np.array_equal(again.cpu().numpy().view(np.int64), gold.view(np.int64))


def test_a_table_too_large_for_residual_bins_is_bit_equal_on_and_off(model):
    import torch
    m = model(S320)
    ex = U.example_burst_lists()
    sg = min(s for lst in ex for _, _, s in lst)
    bursts = tuple(list(lst) + [(0.5 * YEAR, 0.5, 0.35 * sg)] for lst in ex)
    t = 1.0 * YEAR
    ni = U.chi_table_host(m.shape, R.TS_RANGE, bursts, t)
    assert ni is not None and 2 * ni * (80 + 48) > 80 * 1024 and ni <= U.CHI_MAX_NI, ni
    on, bins_on, n_res, fb, att = scan(m, bursts, t)
    off, bins_off, _, _, _ = scan(m, bursts, t, codes=False)
    assert att and n_res == 0 and fb == 0 and bins_on == bins_off
    assert torch.equal(bits(on), bits(off))


# ---- the codes themselves --------------------------------------------------------------------------
def test_codes_are_the_restatement_of_the_layouts_launch_times(model):
    """Every code of the packed state against tests/test_srt_codes_cpu.encode of the same row of
    `cells`; rows past a lane's length and the padding hold 0."""
    import torch
    m = model(ODD)
    srt, P = m.srt, m.fields.npix
    rowbase = srt["rowbase"].cpu().numpy().astype(np.int64)
    Gn = rowbase.size - 1
    cells = srt["cells"].cpu().numpy().reshape(-1, 64, 2)
    rows = srt["packed"]["rows"]
    pc = srt["packed"]["pc"].cpu().numpy().view(np.uint32).reshape(rows // 4, 64, 4)
    pc = pc.transpose(0, 2, 1).reshape(rows, 64)                 # [packed row, lane]
    length = np.zeros(Gn * 64, dtype=np.int64)
    length[:P] = m.start[2 * K]
    want = np.zeros((rows, 64), dtype=np.uint32)
    for g in range(Gn):
        n = int(rowbase[g + 1] - rowbase[g])
        r0 = ((rowbase[g] + 7) // 8) * 8 + 8 * g
        ts = cells[rowbase[g]:rowbase[g] + n, :, 1]
        mine = np.arange(n)[:, None] < length[g * 64:(g + 1) * 64][None, :]
        want[r0:r0 + n] = np.where(mine, Cc.encode(np.where(mine, ts, 0.0), R.TS_RANGE), 0)
    assert np.array_equal(pc, want)
    assert srt["packed"]["pc_bytes"] == rows * 64 * 4 and srt["packed"]["pc_build_ms"] > 0.0
    # every row of the buffer is written: the same codes over a buffer full of ones
    eng = m.eng
    again = torch.full_like(srt["packed"]["pc"], -1)
    fs = m.fields.struct()
    assert eng.lib.rjp_srt_codes(eng.ctx, C.byref(fs), K, srt["start"].data_ptr(),
                                 srt["rowbase"].data_ptr(), srt["cells"].data_ptr(),
                                 again.data_ptr(), eng._stream()) == 1
    eng.synchronize()
    assert torch.equal(again, srt["packed"]["pc"])


# ---- 6: refusals ------------------------------------------------------------------------------------
REFUSALS = {
    "null": "rjp_srt_codes: NULL argument",
    "align": "rjp_srt_codes: d_cells and d_pc must be 16-byte aligned",
    "K": "launch-time-bucketed layout: 1 <= K <= 32",
    "range": "launch-time-bucketed layout: fields.ts_lo / ts_hi (rjp_field_range) required",
    "fields": "fields is NULL",
    "storage": "launch-time-bucketed layout: needs RJP_F64 fields with d_a0 and d_ts",
}


def test_refusals_of_rjp_srt_codes(model):
    from rajepy_amd import _lib
    m = model(S320)
    eng, srt = m.eng, m.srt
    fs = m.fields.struct()
    assert fs.ts_hi > fs.ts_lo
    start, rowbase, cells = (srt[k].data_ptr() for k in ("start", "rowbase", "cells"))
    pc = srt["packed"]["pc"]
    before = pc.clone()

    def call(f=fs, k=K, a=start, b=rowbase, c=cells, d=pc.data_ptr()):
        st = eng.lib.rjp_srt_codes(eng.ctx, C.byref(f) if f is not None else None, k, a, b, c, d,
                                   eng._stream())
        return int(st), (eng.lib.rjp_last_error(eng.ctx) or b"").decode()
    for kw in ({"a": None}, {"b": None}, {"c": None}, {"d": None}):
        assert call(**kw) == (_lib.RJP_ERR_ARG, REFUSALS["null"]), kw
    assert call(d=pc.data_ptr() + 4) == (_lib.RJP_ERR_ARG, REFUSALS["align"])
    assert call(c=cells + 8) == (_lib.RJP_ERR_ARG, REFUSALS["align"])
    assert call(k=0) == (_lib.RJP_ERR_ARG, REFUSALS["K"])
    assert call(k=33) == (_lib.RJP_ERR_ARG, REFUSALS["K"])
    assert call(f=None) == (_lib.RJP_ERR_ARG, REFUSALS["fields"])
    bad = m.fields.struct()
    bad.ts_lo = bad.ts_hi = 0.0
    assert call(f=bad) == (_lib.RJP_ERR_ARG, REFUSALS["range"])
    bad = m.fields.struct()
    bad.ts_hi = float("nan")
    assert call(f=bad) == (_lib.RJP_ERR_ARG, REFUSALS["range"])
    bad = m.fields.struct()
    bad.d_a0 = None
    assert call(f=bad) == (_lib.RJP_ERR_ARG, REFUSALS["storage"])
    # which one wins: K before the range, the fields before the pointers before the alignment
    bad = m.fields.struct()
    bad.ts_lo = bad.ts_hi = 0.0
    assert call(f=bad, k=0)[1] == REFUSALS["K"]
    assert call(k=0, a=None)[1] == REFUSALS["K"]
    assert call(a=None, d=pc.data_ptr() + 4)[1] == REFUSALS["null"]
    eng.synchronize()
    import torch
    assert torch.equal(pc, before)                               # a refused call writes nothing
    assert call()[0] == 1                                        # ... and the valid call rebuilds them
    eng.synchronize()
    assert torch.equal(pc, before)
