"""K25 (regions.hip: rjp_image_stats, rjp_label_regions, rjp_mask_grow) through the raw C-ABI and
RTEngine, against tests/regions_ref.py -- NumPy / scipy.ndimage restatements of the definitions in
include/rjprt.h, which tests/test_regions_reference_cpu.py pins to hand-worked cases, to
emulations of the device's algorithms and to planted mistakes.

Every case of tests/regions_cases.py is held BIT FOR BIT (count, n_nonfinite, min, max, median,
mad, labels, areas, region counts, grown masks); sum and sumsq at the any-order bound derived in
the reference's docstring.  Every raw call runs between guard bands (the image 8 bytes off a
16-byte line), with poisoned outputs and a poisoned workspace; the cap flag must stay 0."""
import numpy as np
import pytest

from tests import regions_cases as RC
from tests import regions_ref as K

pytestmark = pytest.mark.gpu
GUARD = 33                             # odd: a float64 payload starts 8 bytes off a 16-byte line
P_W = 0xA5
WORST = {}


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()
    print("\nworst sum error / bound: " + ", ".join("%s %.3g" % kv for kv in sorted(WORST.items())))


class Band:
    """A device buffer of `n` elements between two guard bands of `guard` poisoned elements."""

    def __init__(self, eng, n, dtype, fill, guard=GUARD):
        import torch
        self.t = torch.full((guard + n + guard,), fill, dtype=dtype, device=eng.device)
        self.n, self.g, self.fill = n, guard, fill
        self.ptr = self.t.data_ptr() + guard * self.t.element_size()

    def set(self, host):
        import torch
        self.t[self.g:self.g + self.n] = torch.from_numpy(np.ascontiguousarray(host).ravel()).to(self.t.device)
        return self

    def get(self):
        h = self.t.cpu().numpy()
        for band in (h[:self.g], h[self.g + self.n:]):
            assert np.array_equal(band, np.full(band.shape, self.fill, dtype=h.dtype)), "a guard band was written"
        return h[self.g:self.g + self.n].copy()


def flag_of(work):
    return int(work.get()[:4].view(np.int32)[0])


# ---- statistics ---------------------------------------------------------------------------------------
def run_stats(eng, case, guard=GUARD, poison=P_W):
    import torch
    img, mask, nx, nz = case["img"], case["mask"], case["nx"], case["nz"]
    M = img.shape[0]
    ib = Band(eng, img.size, torch.float64, -1e300, guard).set(img)
    assert ib.ptr % 16 == 8
    mb = Band(eng, mask.size, torch.uint8, 0x5A, guard).set(mask) if mask is not None else None
    ob = Band(eng, M * 8, torch.float64, 7.25, guard)
    need = eng.lib.rjp_image_stats_workspace(M, nx, nz)
    assert need == K.stats_workspace(M, nx, nz)
    kb = Band(eng, need, torch.uint8, poison, guard * 8)
    ret = eng.lib.rjp_image_stats(eng.ctx, ib.ptr, M, nx, nz, mb.ptr if mb else None,
                                  mask.shape[0] if mask is not None else 0, 1 if case["inside"] else 0,
                                  ob.ptr, kb.ptr, need, eng._stream())
    eng.synchronize()
    assert ret == K.stats_workgroups(M, nx, nz), (ret, eng.lib.rjp_last_error(eng.ctx))
    assert ib.get().tobytes() == img.tobytes(), "the image was written"
    kb.get()
    return ob.get().reshape(M, 8)


def judge_stats(got, case):
    img, mask = case["img"], case["mask"]
    for m in range(img.shape[0]):
        mk = None if mask is None else mask[m if mask.shape[0] > 1 else 0]
        ref = K.image_stats(img[m], mk, case["inside"])
        for i, k in enumerate(("count", "n_nonfinite", "min", "max", "median", "mad")):
            want = np.float64(ref[k])
            assert got[m, i].tobytes() == want.tobytes(), (m, k, got[m, i], want)
        b_sum, b_sq = K.sum_bounds(ref)
        if ref["count"] == 0:
            assert got[m, 6:].tobytes() == np.zeros(2).tobytes()
            continue
        for i, k, b in ((6, "sum", b_sum), (7, "sumsq", b_sq)):
            if ref[k] > np.finfo(np.float64).max:
                assert got[m, i] == np.inf, (m, k)
                continue
            err = abs(float(np.longdouble(got[m, i]) - ref[k]))
            if b > 0:
                WORST[k] = max(WORST.get(k, 0.0), err / b)
            assert err <= b, (m, k, err, b)


STAT_CASES = RC.stat_cases()


@pytest.mark.parametrize("group", range(4))
def test_image_stats_cases_bit_for_bit(eng, group):
    """Every statistics case: the six exact numbers bit for bit, the two sums at the derived bound;
    the same bits on a repeated call with other guard bands and another workspace poison."""
    for name, case in STAT_CASES[group::4]:
        got = run_stats(eng, case)
        try:
            judge_stats(got, case)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
        again = run_stats(eng, case, guard=GUARD + 2, poison=0x00)
        assert again.tobytes() == got.tobytes(), name


# ---- labels -------------------------------------------------------------------------------------------
def run_labels(eng, case, conn, want_area=True, poison=P_W):
    import torch
    mask, M, nx, nz = case["mask"], case["n_maps"], case["nx"], case["nz"]
    n = nx * nz
    mb = Band(eng, mask.size, torch.uint8, 0x5A).set(mask)
    lb = Band(eng, M * n, torch.int32, -77)
    ab = Band(eng, M * n, torch.int32, -78) if want_area else None
    nb = Band(eng, M, torch.int32, -79)
    need = eng.lib.rjp_label_regions_workspace(M, nx, nz)
    assert need == K.label_workspace(M, nx, nz)
    kb = Band(eng, need, torch.uint8, poison, GUARD * 8)
    ret = eng.lib.rjp_label_regions(eng.ctx, mb.ptr, mask.shape[0], M, nx, nz, conn, lb.ptr,
                                    ab.ptr if ab else None, nb.ptr, kb.ptr, need, eng._stream())
    eng.synchronize()
    assert ret == K.region_workgroups(M, nx, nz), (ret, eng.lib.rjp_last_error(eng.ctx))
    assert mb.get().tobytes() == mask.tobytes(), "the mask was written"
    assert flag_of(kb) == 0, "a union-find loop ran into its cap"
    return lb.get().reshape(M, n), ab.get().reshape(M, n) if ab else None, nb.get()


@pytest.mark.parametrize("conn", [1, 2])
def test_label_regions_cases_bit_for_bit(eng, conn):
    for name, case in RC.label_cases():
        lab, area, nreg = run_labels(eng, case, conn)
        mask = case["mask"]
        for m in range(case["n_maps"]):
            rl, ra, rn = K.label_regions(mask[m if mask.shape[0] > 1 else 0], case["nx"], case["nz"], conn)
            assert np.array_equal(lab[m], rl), (name, m, "labels")
            assert np.array_equal(area[m], ra), (name, m, "areas")
            assert int(nreg[m]) == rn, (name, m, nreg[m], rn)
        if name in ("serpentine-130x65", "3maps-67x131", "random0.59-130x65"):
            l2, a2, n2 = run_labels(eng, case, conn, want_area=False, poison=0x00)
            assert a2 is None and np.array_equal(l2, lab) and np.array_equal(n2, nreg), name
    ser = dict(RC.label_cases())["serpentine-130x65"]
    lab, area, nreg = run_labels(eng, ser, conn)
    assert int(nreg[0]) == 1 and int(area[0, 0]) == 4290 and set(np.unique(lab)) == {0, 1}


# ---- growth -------------------------------------------------------------------------------------------
def run_grow(eng, case, n_iter, conn, poison=P_W):
    import torch
    seed, con, M, nx, nz = case["seed"], case["con"], case["n_maps"], case["nx"], case["nz"]
    sb = Band(eng, seed.size, torch.uint8, 0x5A).set(seed)
    cb = Band(eng, con.size, torch.uint8, 0x5B).set(con)
    need = eng.lib.rjp_mask_grow_workspace(M, nx, nz)
    assert need == K.grow_workspace(M, nx, nz)
    kb = Band(eng, need, torch.uint8, poison, GUARD * 8)
    ret = eng.lib.rjp_mask_grow(eng.ctx, sb.ptr, cb.ptr, con.shape[0], M, nx, nz, n_iter, conn, kb.ptr,
                                need, eng._stream())
    eng.synchronize()
    assert ret == K.region_workgroups(M, nx, nz), (ret, eng.lib.rjp_last_error(eng.ctx))
    assert cb.get().tobytes() == con.tobytes(), "the constraint was written"
    assert flag_of(kb) == 0, "a union-find loop ran into its cap"
    return sb.get().reshape(M, nx * nz)


@pytest.mark.parametrize("conn", [1, 2])
@pytest.mark.parametrize("n_iter", RC.GROW_ITERS)
def test_mask_grow_cases_bit_for_bit(eng, n_iter, conn):
    for name, case in RC.grow_cases():
        got = run_grow(eng, case, n_iter, conn)
        seed, con = case["seed"], case["con"]
        if n_iter == 0:
            assert got.tobytes() == seed.tobytes(), (name, "n_iter = 0 must not touch the seed")
            continue
        for m in range(case["n_maps"]):
            want = K.mask_grow(seed[m], con[m if con.shape[0] > 1 else 0], case["nx"], case["nz"], n_iter, conn)
            assert np.array_equal(got[m] != 0, want), (name, m, int((got[m] != 0).sum()), int(want.sum()))
            if n_iter > 0:
                assert set(np.unique(got[m])) <= {0, 1}
        if name.startswith(("corridor", "3maps")):
            assert run_grow(eng, case, n_iter, conn, poison=0x00).tobytes() == got.tobytes(), name


# ---- refusals -----------------------------------------------------------------------------------------
def test_every_refusal_with_its_message_and_untouched_outputs(eng):
    import torch
    M, nx, nz = 2, 20, 70
    n = nx * nz
    img = Band(eng, M * n, torch.float64, 1.5)
    msk = Band(eng, M * n, torch.uint8, 1)
    st = Band(eng, M * 8, torch.float64, 7.25)
    lab = Band(eng, M * n, torch.int32, -77)
    nrg = Band(eng, M, torch.int32, -79)
    work = Band(eng, max(eng.lib.rjp_mask_grow_workspace(M, nx, nz),
                         eng.lib.rjp_image_stats_workspace(M, nx, nz)) + 8, torch.uint8, P_W, guard=40)   # (+ 8: room to misalign)
    assert work.ptr % 8 == 0
    lib, ctx, s = eng.lib, eng.ctx, eng._stream()
    E_ARG, E_WORK = -1, -4

    def stats(**kw):
        a = dict(img=img.ptr, M=M, nx=nx, nz=nz, mask=None, n_mask=0, out=st.ptr, work=work.ptr, wb=work.n)
        a.update(kw)
        return lib.rjp_image_stats(ctx, a["img"], a["M"], a["nx"], a["nz"], a["mask"], a["n_mask"], 1,
                                   a["out"], a["work"], a["wb"], s)

    def label(**kw):
        a = dict(mask=msk.ptr, n_mask=M, M=M, nx=nx, nz=nz, conn=1, lab=lab.ptr, nreg=nrg.ptr,
                 work=work.ptr, wb=work.n)
        a.update(kw)
        return lib.rjp_label_regions(ctx, a["mask"], a["n_mask"], a["M"], a["nx"], a["nz"], a["conn"],
                                     a["lab"], None, a["nreg"], a["work"], a["wb"], s)

    def grow(**kw):
        a = dict(seed=msk.ptr, con=msk.ptr, n_mask=1, M=M, nx=nx, nz=nz, it=3, conn=1, work=work.ptr,
                 wb=work.n)
        a.update(kw)
        return lib.rjp_mask_grow(ctx, a["seed"], a["con"], a["n_mask"], a["M"], a["nx"], a["nz"], a["it"],
                                 a["conn"], a["work"], a["wb"], s)

    table = [
        (stats, dict(img=None), E_ARG, "stats_null"), (stats, dict(out=None), E_ARG, "stats_null"),
        (stats, dict(nx=0), E_ARG, "stats_size"), (stats, dict(M=65536), E_ARG, "stats_maps"),
        (stats, dict(nx=1048561, nz=1), E_ARG, "stats_nx"), (stats, dict(nx=65536, nz=32768), E_ARG, "stats_pix"),
        (stats, dict(mask=msk.ptr, n_mask=3), E_ARG, "stats_nmask"),
        (stats, dict(M=65535, nx=8192, nz=8200), E_ARG, "stats_wgs"),
        (stats, dict(work=None), E_WORK, "stats_work"),
        (stats, dict(wb=lib.rjp_image_stats_workspace(M, nx, nz) - 1), E_WORK, "stats_work"),
        (stats, dict(work=work.ptr + 4, wb=work.n - 4), E_WORK, "stats_align"),
        (label, dict(mask=None), E_ARG, "label_null"), (label, dict(lab=None), E_ARG, "label_null"),
        (label, dict(nreg=None), E_ARG, "label_null"), (label, dict(nz=-3), E_ARG, "label_size"),
        (label, dict(M=65536, n_mask=65536), E_ARG, "label_maps"), (label, dict(nx=1048561, nz=1), E_ARG, "label_nx"),
        (label, dict(nx=65536, nz=32768), E_ARG, "label_pix"), (label, dict(n_mask=3), E_ARG, "label_nmask"),
        (label, dict(conn=0), E_ARG, "label_conn"), (label, dict(conn=3), E_ARG, "label_conn"),
        (label, dict(work=None), E_WORK, "label_work"),
        (label, dict(wb=lib.rjp_label_regions_workspace(M, nx, nz) - 1), E_WORK, "label_work"),
        (label, dict(work=work.ptr + 1, wb=work.n - 1), E_WORK, "label_align"),
        (grow, dict(seed=None), E_ARG, "grow_null"), (grow, dict(con=None), E_ARG, "grow_null"),
        (grow, dict(M=0), E_ARG, "grow_size"), (grow, dict(M=65536), E_ARG, "grow_maps"),
        (grow, dict(nx=1048561, nz=1), E_ARG, "grow_nx"), (grow, dict(nx=65536, nz=32768), E_ARG, "grow_pix"),
        (grow, dict(n_mask=3), E_ARG, "grow_nmask"),
        (grow, dict(conn=5), E_ARG, "grow_conn"), (grow, dict(work=None), E_WORK, "grow_work"),
        (grow, dict(wb=lib.rjp_mask_grow_workspace(M, nx, nz) - 1, it=-1), E_WORK, "grow_work"),
        (grow, dict(work=work.ptr + 2, wb=work.n - 2), E_WORK, "grow_align"),
    ]
    for fn, change, status, key in table:
        got = fn(**change)
        assert got == status, (fn.__name__, change, got)
        assert lib.rjp_last_error(ctx).decode() == K.MESSAGES[key], (fn.__name__, change)
    eng.synchronize()
    for band in (img, msk, st, lab, nrg, work):
        h = band.get()
        assert np.array_equal(h, np.full(h.shape, band.fill, dtype=h.dtype)), "a refused call wrote"
    assert lib.rjp_image_stats(None, img.ptr, M, nx, nz, None, 0, 1, st.ptr, work.ptr, work.n, s) == E_ARG
    for q in (lib.rjp_image_stats_workspace, lib.rjp_label_regions_workspace, lib.rjp_mask_grow_workspace):
        assert q(0, 4, 4) == 0 and q(1, 65536, 32768) == 0 and q(65536, 1, 1) == 0 and q(1, 4, 4) > 0


# ---- the engine's wrappers ----------------------------------------------------------------------------
def test_engine_wrappers(eng):
    import torch
    case = RC.stat_case((23, 89), "nonfinite", "per_map_out", 3)
    img = torch.from_numpy(case["img"]).to(eng.device)
    mask = torch.from_numpy(case["mask"]).to(eng.device)
    st = eng.image_stats(img, 23, 89, mask=mask, inside=False)
    judge_stats(st.cpu().numpy(), case)
    lc = dict(RC.label_cases())["3maps-67x131"]
    lab, area, nreg = eng.label_regions(torch.from_numpy(lc["mask"]).to(eng.device), 67, 131, 2)
    for m in range(3):
        rl, ra, rn = K.label_regions(lc["mask"][m], 67, 131, 2)
        assert np.array_equal(lab[m].cpu().numpy(), rl) and np.array_equal(area[m].cpu().numpy(), ra)
        assert int(nreg[m]) == rn
    gc = dict(RC.grow_cases())["shared-3maps-67x131"]
    seed = torch.from_numpy(gc["seed"]).to(eng.device)
    for n_iter in (0, 11, -1):
        out = eng.mask_grow(seed, torch.from_numpy(gc["con"]).to(eng.device), 67, 131, n_iter, 1)
        assert seed.cpu().numpy().tobytes() == gc["seed"].tobytes(), "mask_grow changed its seed"
        for m in range(3):
            want = K.mask_grow(gc["seed"][m], gc["con"][0], 67, 131, n_iter, 1)
            assert np.array_equal(out[m].cpu().numpy() != 0, want), (n_iter, m)


# ---- end to end: observe_ff with noise, major cycles and the automatic mask ---------------------------------
AM = dict(sidelobe_threshold=0.0, noise_threshold=3.0)      # DESIGN section 3 (K25) says why these two


def test_observe_ff_with_the_automatic_mask(eng, tmp_path_factory):
    """(a) every update equals the reference's automask_step fed that run's residual (restated from
    the component list with the engine's wrappers), (b) the masks only grow, (c) every component lies
    inside its map's final mask and the user's, (d) automask=None is the result as it was, bit for bit,
    (e) at run 1 a region is kept and one is pruned.  Prints the peak residual and the components
    outside the model's support with and without the automatic mask (not asserted)."""
    import torch
    from rajepy_amd import engine as E
    from tests import observe_ref as R
    from tests import test_gpu_observe as O
    jm = O.model(eng, tmp_path_factory)
    freqs = np.array([4.9e9, 5.1e9])
    tr = jm.uv_tracks(O.FIXTURE, O.T_OBS, O.T_INT, min_el_deg=O.MIN_EL)
    cell_as = O.grid_of(jm, tr, 5e9)
    ni, nj = O.SHAPE
    peak = float(np.abs(jm.visibilities_ff([0.], [0.], freqs)).max())
    sigma = np.array([2.0, 1.0]) * peak
    box = (4, 43, 3, 36)
    beam = (4.0 * cell_as, 3.0 * cell_as, 30.)
    kw = dict(shape=O.SHAPE, cell_as=cell_as, niter=60, major_cycles=3, mask=box, beam=beam, sigma_jy=sigma,
              seed=R.SEED)
    base = jm.observe_ff(tr, freqs, O.T_OBS, O.T_INT, **kw)
    none = jm.observe_ff(tr, freqs, O.T_OBS, O.T_INT, automask=None, **kw)
    for name in ("image", "residual", "model", "peak_residual"):                                   # (d)
        assert getattr(none.clean, name).tobytes() == getattr(base.clean, name).tobytes(), name
    assert none.clean.automask is None and base.clean.automask is None
    auto = jm.observe_ff(tr, freqs, O.T_OBS, O.T_INT, automask=AM, **kw)
    am = auto.clean.automask
    assert np.array_equal(auto.vis, base.vis) and len(am) == 2
    # the restatement: the residual at the top of a run is the image of V minus the visibilities of the
    # components found before it
    im = jm._imager
    cell = im._image_grid(O.SHAPE, cell_as)[2]
    su, sv = E.image_scales(freqs, cell)
    V = torch.from_numpy(auto.vis).to(eng.device)
    opts = E.automask_options(AM)
    abc = [E.beam_quadratic(*beam, cell)] * 2
    side = np.array([d["sidelobe"] for d in auto.clean.major])
    um = np.zeros(O.SHAPE, dtype=bool)
    um[box[0]:box[1] + 1, box[2]:box[3] + 1] = True
    comps = auto.clean.components
    n_runs = max(len(a["runs"]) for a in am)
    assert n_runs >= 2 and all(len(a["runs"]) == n_runs for a in am)
    prev = np.zeros((2, ni * nj), dtype=bool)
    for j in range(n_runs):
        start = [a["runs"][j]["start"] for a in am]
        if max(start) == 0:
            Rj = im._dirty_images(V, tr.u_m, tr.v_m, freqs, None, O.SHAPE, cell_as, False, device=True)
        else:
            width = kw["niter"]                  # the chunk's own list width
            cpix = torch.zeros(2, width, dtype=torch.int32, device=eng.device)
            cflux = torch.zeros(2, width, dtype=torch.float64, device=eng.device)
            for m in range(2):
                c = comps[m][:start[m]]
                cpix[m, :start[m]] = torch.from_numpy((c[:, 0] * nj + c[:, 1]).astype(np.int32)).to(eng.device)
                cflux[m, :start[m]] = torch.from_numpy(np.ascontiguousarray(c[:, 2])).to(eng.device)
            count = torch.tensor(start, dtype=torch.int32, device=eng.device)
            Vres = eng.vis_components(cpix, cflux, count, ni, nj, su, sv, tr.u_m, tr.v_m, vis_in=V.contiguous(),
                                      sign=-1)
            Rj = im._dirty_images(Vres, tr.u_m, tr.v_m, freqs, None, O.SHAPE, cell_as, False, device=True)
        want, winfo = K.automask_step(Rj.cpu().numpy(), prev, um, side, abc, opts, ni, nj)
        got, _ = E.automask_step(eng, Rj, torch.from_numpy(prev).to(eng.device), torch.from_numpy(um).to(eng.device),
                                 side, abc, opts, shape=O.SHAPE)
        assert np.array_equal(got.cpu().numpy() != 0, want), ("run", j)                           # (a)
        for m in range(2):
            for k, v in winfo[m].items():
                assert np.float64(am[m]["runs"][j][k]).tobytes() == np.float64(v).tobytes(), (j, m, k)
        assert not (prev & ~want).any()                                                            # (b)
        prev = want
    for m in range(2):
        final = am[m]["mask"]
        assert np.array_equal(final.reshape(-1), prev[m]) and not (final & ~um).any()
        ix, iz = comps[m][:, 0].astype(int), comps[m][:, 1].astype(int)
        assert final[ix, iz].all() and um[ix, iz].all()                                           # (c)
        first = am[m]["runs"][0]
        print("\nmap %d run 1: %s" % (m, {k: first[k] for k in ("sigma", "T", "T_low", "n_regions", "n_kept",
                                                                 "n_seed", "n_mask")}))
    assert all(a["runs"][0]["n_kept"] >= 1 for a in am)                                          # (e)
    assert any(a["runs"][0]["n_regions"] > a["runs"][0]["n_kept"] for a in am)
    support = jm.flux_ff(freqs) > 0 if hasattr(jm, "flux_ff") else None
    for name, res in (("box", base.clean), ("automask", auto.clean)):
        outside = "n/a"
        if support is not None and support.shape[1:] == O.SHAPE:
            outside = [int((~support[m][c[:, 0].astype(int), c[:, 1].astype(int)]).sum())
                       for m, c in enumerate(res.components)]
        print("%s: peak residual %s, components %s, outside the model's support %s"
              % (name, res.peak_residual, [len(c) for c in res.components], outside))


def test_imstat_on_a_line_cube(eng, tmp_path_factory):
    from tests import test_gpu_observe as O
    jm = O.model(eng, tmp_path_factory)
    tr = jm.uv_tracks(O.FIXTURE, O.T_OBS, O.T_INT, min_el_deg=O.MIN_EL)
    from rajepy_amd.maths import rrls
    nu0 = rrls.line_constants("H66a")["nu_rest"]
    freqs = nu0 * (1.0 + np.array([-2e-5, 0.0, 2e-5]))
    cube = jm.clean_image_rrl("H66a", tr.u_m, tr.v_m, freqs, shape=O.SHAPE, cell_as=O.grid_of(jm, tr, nu0),
                              niter=10, beam=(1.0, 1.0, 0.))
    inner = np.zeros(O.SHAPE, dtype=bool)
    inner[10:30, 8:30] = True
    for mask, inside in ((None, True), (inner, True), (inner, False)):
        got = jm.imstat(cube.image, mask=mask, inside=inside)
        assert len(got) == 3
        for f in range(3):
            ref = K.image_stats(cube.image[f], mask, inside)
            assert got[f]["npts"] == int(ref["count"]) > 0
            for a, b in (("min", "min"), ("max", "max"), ("median", "median"), ("medabsdevmed", "mad")):
                assert np.float64(got[f][a]).tobytes() == np.float64(ref[b]).tobytes(), (f, a)
            assert got[f]["sigma_robust"] == 1.4826 * ref["mad"]
            b_sum, _ = K.sum_bounds(ref)
            assert abs(float(np.longdouble(got[f]["sum"]) - ref["sum"])) <= b_sum
