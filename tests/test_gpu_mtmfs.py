"""rjp_mtmfs (K19, mtmfs.hip) through the C-ABI, RTEngine.mtmfs and JetModel.clean_image_ff /
observe_ff(nterms=...), against tests/mtmfs_ref.py: the long-double multi-term MFS CLEAN that FOLLOWS
the device's component list.  tests/test_mtmfs_reference_cpu.py pins the reference to hand-worked
cases, to a float64 emulation on these same inputs (inside the bounds) and to planted mistakes
(outside), and shows that every case finds components, outside tile 0 where there is more than one tile.

The bounds are derived in tests/mtmfs_ref.py, not measured:
    plane t, pixel x:   (updates of x) n_t 2^-53 (|R0_t[x]| + sum_c sum_q |c_q| |B_{t+q}|)      = b_t[x]
    a_q at pixel p:     n_t 2^-53 sum_t |Hinv[q][t]| |R_t[p]| + sum_t |Hinv[q][t]| b_t[p]
The module prints the worst error / bound per rule."""
import copy
import os

import numpy as np
import pytest

from tests import clean_ref as C
from tests import gpu_util as U
from tests import mtmfs_cases as MC
from tests import mtmfs_ref as K
from tests import test_gpu_clean as G

pytestmark = pytest.mark.gpu
YEAR = 31557600.0
LD = np.longdouble
WORST = {}
POISON_PIX, POISON_F = -77, 7.25
GUARD = 33
Band = G.Band
FIXTURE = os.path.join(U.GOLDEN, "antenna_configs", "vla.a.cfg")


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()
    print("\nworst error / bound per rule: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def note(kind, r):
    WORST[kind] = max(WORST.get(kind, 0.0), float(r))
    assert r <= 1.0, (kind, r)


# ---- 1: direct calls -----------------------------------------------------------------------------------
def run_mt(eng, R0, B, hinv, mask, thresh, gain, n_iter, model0=None, want_peak=True, guard=GUARD):
    """One raw rjp_mtmfs call on R0 [M, n_t, nx, nz] with B [n_psf, 2 n_t - 1, px, pz] and hinv
    [M, n_t, n_t], every buffer between guard bands, the workspace of exactly the queried size -> dict of
    host arrays; the returned count is held to the tile rule."""
    import torch
    from rajepy_amd import _lib
    M, n_t, nx, nz = R0.shape
    n_psf, nb, px, pz = B.shape
    assert nb == 2 * n_t - 1
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    res = Band(eng, R0.size, f64, -1e300, guard).set(R0)
    psf = Band(eng, B.size, f64, 1e300, guard).set(B)
    cpix = Band(eng, M * n_iter, i32, POISON_PIX)
    ccoef = Band(eng, M * n_iter * n_t, f64, POISON_F)
    ncomp = Band(eng, M, i32, POISON_PIX)
    model = Band(eng, R0.size, f64, -1e300).set(np.zeros(R0.size) if model0 is None else model0)
    peak = Band(eng, M, f64, POISON_F)
    wb = eng.lib.rjp_mtmfs_workspace(M, n_t, nx, nz)
    assert wb == K.workspace_bytes(M, n_t, nx, nz)
    work = Band(eng, wb, u8, 0xA5, 64)
    dmask = Band(eng, nx * nz, u8, 1, 3).set(np.asarray(mask != 0, dtype=np.uint8)) if mask is not None else None
    h = np.ascontiguousarray(np.broadcast_to(np.asarray(hinv, dtype=np.float64).reshape(-1, n_t, n_t), (M, n_t, n_t)))
    ret = eng.lib.rjp_mtmfs(eng.ctx, res.ptr, M, n_t, nx, nz, psf.ptr, n_psf, px, pz, _lib.dbl_array(h),
                            dmask.ptr if dmask else None, _lib.dbl_array(np.broadcast_to(thresh, (M,))),
                            float(gain), n_iter, cpix.ptr, ccoef.ptr, ncomp.ptr, model.ptr,
                            peak.ptr if want_peak else None, work.ptr, wb, eng._stream())
    eng.synchronize()
    assert ret == K.workgroups(M, nx, nz), (ret, eng.lib.rjp_last_error(eng.ctx))
    assert psf.get().tobytes() == np.ascontiguousarray(B).tobytes()
    if dmask:
        dmask.get()
    return dict(res=res.get().reshape(R0.shape), cpix=cpix.get().reshape(M, n_iter),
                ccoef=ccoef.get().reshape(M, n_iter, n_t), ncomp=ncomp.get(), model=model.get().reshape(R0.shape),
                peak=peak.get(), work=work.get(), ret=ret)


def follow_all(kind, R0, B, hinv, mask, thresh, gain, n_iter, out, model0=None, want_peak=True):
    M, n_t = R0.shape[:2]
    th = np.broadcast_to(thresh, (M,))
    h = np.broadcast_to(np.asarray(hinv, dtype=np.float64).reshape(-1, n_t, n_t), (M, n_t, n_t))
    for m in range(M):
        Bm = B[m if B.shape[0] > 1 else 0]
        w = K.follow(R0[m], Bm, h[m], mask, th[m], gain, n_iter, out["cpix"][m], out["ccoef"][m], out["ncomp"][m],
                     out["res"][m], peak=out["peak"][m] if want_peak else None, model=out["model"][m],
                     model0=None if model0 is None else model0[m], poison_pix=POISON_PIX, poison_coef=POISON_F)
        for rule, r in w.items():
            note(rule, r)
            note(kind + " " + rule, r)
        note("identity", K.conservation(R0[m], Bm, out["cpix"][m], out["ccoef"][m], out["ncomp"][m], out["res"][m]))
    if not want_peak:
        assert np.all(out["peak"] == POISON_F), "d_peak = NULL was written"


KEYS = ("res", "cpix", "ccoef", "ncomp", "model", "peak")


def same_bits(a, b, keys=KEYS + ("work",)):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), "the bits of " + k + " differ"


def run_case(eng, case, **kw):
    return run_mt(eng, case["R0"], case["B"], case["hinv"], case["mask"], case["thresh"], case["gain"],
                  case["n_iter"], **kw)


@pytest.mark.parametrize("name", MC.NAMES)
def test_follow_the_device(eng, name):
    """Every case of tests/mtmfs_cases.py: judged by the reference; the same bits on a repeated call and
    with every base pointer 8 bytes off a 16-byte boundary; d_peak NULL."""
    case = MC.build(name)
    M, n_t, nx, nz = case["R0"].shape
    out = run_case(eng, case)
    follow_all(name, case["R0"], case["B"], case["hinv"], case["mask"], case["thresh"], case["gain"],
               case["n_iter"], out)
    assert np.all(out["ncomp"][case["live"]] >= 3), out["ncomp"]
    same_bits(out, run_case(eng, case))
    same_bits(out, run_case(eng, case, guard=GUARD + 1), KEYS)
    nop = run_case(eng, case, want_peak=False)
    assert np.all(nop["peak"] == POISON_F)
    same_bits(out, nop, ("res", "cpix", "ccoef", "ncomp", "model"))
    if name == "67x131 full":
        # map 0 stops at its threshold while map 1 runs on
        assert 0 < out["ncomp"][0] < case["n_iter"] == out["ncomp"][1] and out["peak"][0] <= case["thresh"][0]
        assert (out["cpix"][:, :3] >= K.TILE).any()
    if name == "31x33 odd npix":
        # the all-NaN map beside live ones: nothing found, nothing touched; the NaN of one plane stays
        assert out["ncomp"][1] == 0 and out["peak"][1] == 0.0 and np.isnan(out["res"][1]).all()
        assert np.all(out["cpix"][1] == POISON_PIX) and not out["model"][1].any()
        assert np.array_equal(np.isnan(out["res"][0]), np.isnan(case["R0"][0]))
        assert out["ncomp"][0] == out["ncomp"][2] == case["n_iter"]


def test_one_pixel_by_hand(eng):
    # one pixel, two terms: B = (1, 0.5, 0.5), H = [[1, .5], [.5, .5]], Hinv = [[2, -2], [-2, 4]]; exact in binary
    B = np.array([1.0, 0.5, 0.5]).reshape(1, 3, 1, 1)
    hinv = np.array([[2.0, -2.0], [-2.0, 4.0]])
    R0 = np.array([1.0, 0.75]).reshape(1, 2, 1, 1)            # = H (0.5, 1.0)
    out = run_mt(eng, R0, B, hinv, None, 0.0, 0.5, 2)
    # a = (0.5, 1.0), c = (0.25, 0.5): R_0 = 1 - .25 - .25 = .5, R_1 = .75 - .125 - .25 = .375; then halves again
    assert list(out["ccoef"][0].ravel()) == [0.25, 0.5, 0.125, 0.25] and list(out["cpix"][0]) == [0, 0]
    assert list(out["res"].ravel()) == [0.25, 0.1875] and out["ncomp"][0] == 2
    assert out["peak"][0] == 0.125 and list(out["model"].ravel()) == [0.375, 0.75]
    follow_all("1 x 1", R0, B, hinv, None, 0.0, 0.5, 2, out)
    one = run_mt(eng, R0, B, hinv, None, 0.0, 1.0, 3)          # gain 1 empties both planes: one component
    assert one["ncomp"][0] == 1 and not one["res"].any() and one["peak"][0] == 0.0
    assert list(one["ccoef"][0, 0]) == [0.5, 1.0] and np.all(one["cpix"][0, 1:] == POISON_PIX)
    stop = run_mt(eng, R0, B, hinv, None, 0.25, 0.5, 5)        # |a_0| = 0.5, 0.25: the second is not > 0.25
    assert stop["ncomp"][0] == 1 and stop["peak"][0] == 0.25
    follow_all("1 x 1", R0, B, hinv, None, 0.25, 0.5, 5, stop)


@pytest.mark.parametrize("nx,nz,px,pz", [(5, 3, 9, 5), (67, 131, 133, 261), (31, 33, 31, 31)])
def test_one_term_equals_rjp_clean_bit_for_bit(eng, nx, nz, px, pz):
    """n_t = 1, Hinv = 1.0, a beam whose centre is exactly 1.0: a_0 = R and c_0 = gain R exactly, so every
    output -- the workspace included -- equals rjp_clean's, with full and windowed beams."""
    for i, (M, n_psf, masked, n_iter, gain, nan) in enumerate(((1, 1, False, 60, 0.1, False),
                                                               (3, 3, True, 37, 0.1, True),
                                                               (3, 1, False, 12, 1.0, False))):
        D, B = G.inputs(37 * nx + px + i, M, n_psf, nx, nz, px, pz, nan=nan, corners=i == 0)
        assert np.all(B[:, (px - 1) // 2, (pz - 1) // 2] == 1.0)
        mask = G.box(nx, nz) if masked else None
        top = np.array([np.abs(D[m][C.candidates(D[m], mask)]).max() for m in range(M)])
        thresh = 0.3 * top if i == 1 else 0.0
        a = G.run_clean(eng, D, B, mask, thresh, gain, n_iter)
        b = run_mt(eng, D[:, None], B[:, None], np.ones((M, 1, 1)), mask, thresh, gain, n_iter)
        for k in ("cpix", "ncomp", "peak", "work"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert a["cflux"].tobytes() == b["ccoef"].tobytes()
        assert a["res"].tobytes() == b["res"].tobytes() and a["model"].tobytes() == b["model"].tobytes()


def test_a_continued_call_equals_one_long_call(eng):
    case = MC.build("130x65 nt4")
    R0, B, hinv, mask, gain = case["R0"], case["B"], case["hinv"], case["mask"], case["gain"]
    n = 20
    first = run_mt(eng, R0, B, hinv, mask, 0.0, gain, n)
    assert np.all(first["ncomp"] == n)
    second = run_mt(eng, first["res"], B, hinv, mask, 0.0, gain, n, model0=first["model"])
    long = run_mt(eng, R0, B, hinv, mask, 0.0, gain, 2 * n)
    joined = dict(second, ncomp=first["ncomp"] + second["ncomp"],
                  **{k: np.concatenate([first[k], second[k]], axis=1) for k in ("cpix", "ccoef")})
    follow_all("continued", R0, B, hinv, mask, 0.0, gain, 2 * n, joined)
    for k in ("cpix", "ccoef"):
        assert joined[k].tobytes() == long[k].tobytes(), k
    assert second["res"].tobytes() == long["res"].tobytes() and second["model"].tobytes() == long["model"].tobytes()
    assert second["peak"].tobytes() == long["peak"].tobytes()


def test_all_zero_mask_touches_nothing(eng):
    case = MC.build("31x33 nt3")
    R0 = case["R0"]
    m0 = np.arange(R0.size, dtype=np.float64)
    out = run_mt(eng, R0, case["B"], case["hinv"], np.zeros((31, 33)), 0.0, 0.1, 9, model0=m0)
    assert np.all(out["ncomp"] == 0) and np.all(out["peak"] == 0.0)
    assert out["res"].tobytes() == R0.tobytes() and np.array_equal(out["model"].ravel(), m0)
    assert np.all(out["cpix"] == POISON_PIX) and np.all(out["ccoef"] == POISON_F)


def test_engine_mtmfs(eng):
    import torch
    case = MC.build("130x65 nt4")
    R0, B, hinv, mask = case["R0"], case["B"], case["hinv"], case["mask"]
    M, n_t, nx, nz = R0.shape
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(eng.device)
    res, model = dev(R0.reshape(M, n_t, -1)), torch.zeros(M, n_t, nx * nz, dtype=torch.float64, device=eng.device)
    cpix, ccoef, ncomp, peak = eng.mtmfs(res, n_t, nx, nz, dev(B), 41, 25, hinv[0], 37, 0.1, 0.0, mask=mask,
                                         model=model)
    assert eng.last_mtmfs_workgroups == K.workgroups(M, nx, nz) == 18
    assert cpix.shape == (M, 37) and ccoef.shape == (M, 37, n_t) and cpix.dtype == ncomp.dtype == torch.int32
    raw = run_mt(eng, R0, B, hinv, mask, 0.0, 0.1, 37)
    for name, t in (("cpix", cpix), ("ccoef", ccoef), ("ncomp", ncomp), ("res", res), ("model", model),
                    ("peak", peak)):
        assert t.cpu().numpy().tobytes() == raw[name].tobytes(), name
    for bad in (lambda: eng.mtmfs(res, n_t, nx, nz, dev(B), 41, 25, hinv[0], 0, 0.1, 0.0),
                lambda: eng.mtmfs(res, 3, nx, nz, dev(B), 41, 25, hinv[0], 5, 0.1, 0.0),
                lambda: eng.mtmfs(res, n_t, nx, nz, dev(B[:, :5]), 41, 25, hinv[0], 5, 0.1, 0.0),
                lambda: eng.mtmfs(res, n_t, nx, nz, dev(B), 41, 25, hinv[0, :3], 5, 0.1, 0.0),
                lambda: eng.mtmfs(res, n_t, nx, nz, dev(B), 41, 25, hinv[0], 5, 0.1, [0.0, 0.0, 0.0]),
                lambda: eng.mtmfs(res, n_t, nx, nz, dev(B), 41, 25, hinv[0], 5, 0.1, 0.0, mask=np.ones(5))):
        with pytest.raises(ValueError):
            bad()


# ---- 2: refusals ---------------------------------------------------------------------------------------
def test_refusals_leave_poisoned_outputs_untouched(eng):
    import torch
    from rajepy_amd import _lib
    M, n_t, nx, nz, px, pz, n_iter = 2, 2, 5, 3, 9, 5, 4
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    full = lambda n, v, dt: torch.full((n,), v, dtype=dt, device=eng.device)
    wb = eng.lib.rjp_mtmfs_workspace(M, n_t, nx, nz)
    bufs = dict(res=full(M * n_t * nx * nz, 7.0, f64), psf=full(M * 3 * px * pz, 0.5, f64),
                mask=full(nx * nz, 1, u8), cpix=full(M * n_iter, POISON_PIX, i32),
                ccoef=full(M * n_iter * n_t, POISON_F, f64), ncomp=full(M, POISON_PIX, i32),
                model=full(M * n_t * nx * nz, 3.0, f64), peak=full(M, POISON_F, f64), work=full(wb, 0xA5, u8))
    before = {k: t.clone() for k, t in bufs.items()}
    hinv = [2.0, -2.0, -2.0, 4.0, 1.0, 0.0, 0.0, 24.0]
    good = dict(bufs, n_maps=M, n_t=n_t, nx=nx, nz=nz, n_psf=M, px=px, pz=pz, hinv=hinv, thresh=[0.0, 0.1],
                gain=0.1, n_iter=n_iter, nbytes=wb, ctx=True)
    ptr = lambda t: t.data_ptr() if t is not None else None
    arr = lambda v: _lib.dbl_array(v) if v is not None else None

    def mt(a):
        return eng.lib.rjp_mtmfs(eng.ctx if a["ctx"] else None, ptr(a["res"]), a["n_maps"], a["n_t"], a["nx"],
                                 a["nz"], ptr(a["psf"]), a["n_psf"], a["px"], a["pz"], arr(a["hinv"]),
                                 ptr(a["mask"]), arr(a["thresh"]), a["gain"], a["n_iter"], ptr(a["cpix"]),
                                 ptr(a["ccoef"]), ptr(a["ncomp"]), ptr(a["model"]), ptr(a["peak"]),
                                 ptr(a["work"]), a["nbytes"], eng._stream())

    ARG, WS = _lib.RJP_ERR_ARG, _lib.RJP_ERR_WORKSPACE
    big = 2 ** 31 - 1
    bad_h = lambda i, v: [v if j == i else x for j, x in enumerate(hinv)]
    cases = [("NULL d_res", dict(res=None), ARG, "null"), ("NULL d_spsf", dict(psf=None), ARG, "null"),
             ("NULL h_hinv", dict(hinv=None), ARG, "null"), ("NULL h_thresh", dict(thresh=None), ARG, "null"),
             ("NULL d_cpix", dict(cpix=None), ARG, "null"), ("NULL d_ccoef", dict(ccoef=None), ARG, "null"),
             ("NULL d_ncomp", dict(ncomp=None), ARG, "null"),
             ("n_maps = 0", dict(n_maps=0), ARG, "sizes"), ("n_t = 0", dict(n_t=0), ARG, "sizes"),
             ("n_t < 0", dict(n_t=-2), ARG, "sizes"), ("nx < 0", dict(nx=-1), ARG, "sizes"),
             ("nz = 0", dict(nz=0), ARG, "sizes"), ("px = 0", dict(px=0), ARG, "sizes"),
             ("pz < 0", dict(pz=-5), ARG, "sizes"),
             ("n_t = 5", dict(n_t=5, hinv=[1.0] * 50), ARG, "nt"), ("n_t = 2^31 - 1", dict(n_t=big), ARG, "nt"),
             ("even px", dict(px=8), ARG, "even"), ("even pz", dict(pz=4), ARG, "even"),
             ("n_psf = 0", dict(n_psf=0), ARG, "npsf"), ("n_psf = 3", dict(n_psf=3), ARG, "npsf"),
             ("too many pixels", dict(nx=big, nz=big), ARG, "npix"),
             ("gain = 0", dict(gain=0.0), ARG, "gain"), ("gain > 1", dict(gain=1.0000001), ARG, "gain"),
             ("NaN gain", dict(gain=np.nan), ARG, "gain"),
             ("n_iter = 0", dict(n_iter=0), ARG, "niter"),
             ("negative threshold", dict(thresh=[0.0, -1e-9]), ARG, "thresh"),
             ("NaN threshold", dict(thresh=[np.nan, 0.0]), ARG, "thresh"),
             ("NaN Hinv", dict(hinv=bad_h(0, np.nan)), ARG, "hinv"),
             ("infinite Hinv in the last map", dict(hinv=bad_h(7, np.inf)), ARG, "hinv"),
             ("-inf Hinv off the diagonal", dict(hinv=bad_h(1, -np.inf)), ARG, "hinv"),
             ("too many workgroups", dict(n_maps=2000, n_psf=1, nx=46340, nz=46340, hinv=[1.0] * 8000,
                                          thresh=[0.0] * 2000), ARG, "wgs"),
             ("a short workspace", dict(nbytes=wb - 1), WS, "work"),
             ("no workspace", dict(work=None), WS, "work")]
    for what, kw, want, key in cases:
        assert mt(dict(good, **kw)) == want, what
        assert eng.lib.rjp_last_error(eng.ctx).decode() == K.MSG[key], what
    assert mt(dict(good, ctx=False)) == ARG
    assert eng.lib.rjp_last_error(None).decode() == "null context"
    eng.synchronize()
    for k, t in bufs.items():
        assert torch.equal(t, before[k]), k + " was touched by a refusal"
    # the context still serves a valid call; NULL mask, model and peak are no refusals
    assert mt(dict(good, mask=None, model=None, peak=None)) == K.workgroups(M, nx, nz) == 2
    eng.synchronize()
    assert not bool((bufs["ncomp"] == POISON_PIX).any()) and torch.equal(bufs["model"], before["model"])
    assert torch.equal(bufs["peak"], before["peak"])


# ---- 3: the golden example model through JetModel -----------------------------------------------------
def _params(tag):
    p = copy.deepcopy(U.load_golden(tag)[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


SHAPE = (48, 40)
FREQS = np.linspace(4e9, 6e9, 8)
T_OBS, T_INT, MIN_EL = 1200., 60., 20.
# The science check (see the test): |sum c_1 / sum c_0 - fitted slope| measured on the first MI355X run was
# 2.060e-3 (components 1.847865 against the fit's 1.845805, 0.11 % of the slope); the assertion allows
# twice that, the factor 2 covering the spread between machines.
ALPHA_MEASURED = 2.060e-3
ALPHA_TOL = 2 * ALPHA_MEASURED


@pytest.fixture(scope="module")
def example(eng, tmp_path_factory):
    from rajepy_amd import classes, engine as E, logger
    log = logger.Log(str(tmp_path_factory.mktemp("mtmfs") / "cfg1.log"), verbose=False)
    jm = classes.JetModel(_params("cfg1_example"), log=log, engine=eng)
    jm.time = 1.0 * YEAR
    tr = jm.uv_tracks(FIXTURE, T_OBS, T_INT, min_el_deg=MIN_EL)
    cell = E.observation_grid(tr.max_baseline_m, 5e9, 1.0)[0]
    return jm, tr, cell


def test_clean_image_ff_with_two_terms_on_the_example_model(eng, example, monkeypatch):
    """clean_image_ff(mfs=True, nterms=2) on the 27-antenna tracks, 8 channels over 4 - 6 GHz: the planes and
    beams handed to K19 (recorded at the call) -- R_0 and B_0 the one-term `mfs` dirty image and beam bit
    for bit -- the result against the chunk restated with the engine's wrappers, the device's list
    followed by the reference, and alpha NaN exactly below the cut."""
    import torch
    from rajepy_amd import engine as E
    jm, tr, cell = example
    seen = {}
    real = eng.mtmfs

    def spy(res, n_t, nx, nz, spsf, px, pz, hinv, n_iter, gain, thresh, mask=None, model=None):
        seen.update(R0=res.cpu().numpy().copy(), B=spsf.cpu().numpy().copy(), hinv=np.array(hinv), n_t=n_t,
                    shape=(nx, nz, px, pz), thresh=thresh, mask=mask)
        return real(res, n_t, nx, nz, spsf, px, pz, hinv, n_iter, gain, thresh, mask=mask, model=model)

    monkeypatch.setattr(eng, "mtmfs", spy)
    ni, nj = SHAPE
    pi_, pj = 2 * ni - 1, 2 * nj - 1
    niter, gain = 150, 0.1
    kw = dict(shape=SHAPE, cell_as=cell, mfs=True, weighting="briggs", robust=0.5)
    # the one-term `mfs` clean first: its dirty image and beam (made with the image grid's weights, as the
    # clean makes them) are what R_0 and B_0 must equal bit for bit
    one = {}
    real_clean = eng.clean

    def spy1(res_, nx, nz, psf, px, pz, n_iter, gain_, thresh_, mask=None, model=None):
        one.update(D=res_.cpu().numpy().copy(), B=psf.cpu().numpy().copy())
        return real_clean(res_, nx, nz, psf, px, pz, n_iter, gain_, thresh_, mask=mask, model=model)

    monkeypatch.setattr(eng, "clean", spy1)
    jm.clean_image_ff(tr.u_m, tr.v_m, FREQS, niter=1, nterms=1, **kw)
    monkeypatch.setattr(eng, "clean", real_clean)
    thresh = 1e-3 * float(np.abs(one["D"]).max())
    res = jm.clean_image_ff(tr.u_m, tr.v_m, FREQS, niter=niter, gain=gain, threshold_jy=thresh, nterms=2, **kw)
    monkeypatch.setattr(eng, "mtmfs", real)
    assert seen["n_t"] == 2 and seen["shape"] == (ni, nj, pi_, pj) and seen["mask"] is None
    R0 = seen["R0"].reshape(2, ni, nj)
    B = seen["B"].reshape(3, pi_, pj)
    assert one["D"].tobytes() == R0[0].tobytes() and one["B"].tobytes() == B[0].tobytes(), \
        "R_0 / B_0 are not the one-term mfs dirty image / beam"
    assert abs(B[0, ni - 1, nj - 1] - 1.0) <= 1e-12
    t = res.taylor[0]
    H, Hinv = E.taylor_hessian_inverse(B[:, ni - 1, nj - 1])
    assert np.array_equal(t["hessian"], H) and np.array_equal(seen["hinv"][0], Hinv) and t["reffreq_hz"] == 5e9
    # the device's list, followed on the planes and beams it was handed
    comp = res.components[0]
    n = len(comp)
    assert comp.shape == (n, 4) and n >= 3
    cpix = (comp[:, 0] * nj + comp[:, 1]).astype(np.int64)
    rows_p = np.concatenate([cpix, np.full(niter - n, POISON_PIX)])
    rows_c = np.concatenate([comp[:, 2:], np.full((niter - n, 2), POISON_F)])
    w = K.follow(R0, B, Hinv, None, thresh, gain, niter, rows_p, rows_c, n, t["residual_tt"],
                 peak=res.peak_residual[0], model=t["model_tt"])
    for rule, r in w.items():
        note("clean_image_ff " + rule, r)
    assert np.array_equal(res.residual[0], t["residual_tt"][0]) and np.array_equal(res.model[0], t["model_tt"][0])
    assert np.array_equal(res.image[0], t["tt"][0])
    # the chunk restated with the engine's wrappers: the same bits
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(eng.device)
    planes, model = dev(seen["R0"]), torch.zeros(1, 2, ni * nj, dtype=torch.float64, device=eng.device)
    cp, cc, nc, pk = eng.mtmfs(planes, 2, ni, nj, dev(seen["B"]), pi_, pj, Hinv, niter, gain, thresh, model=model)
    assert int(nc[0]) == n and np.array_equal(cp.cpu().numpy()[0, :n], cpix)
    assert cc.cpu().numpy()[0, :n].tobytes() == np.ascontiguousarray(comp[:, 2:]).tobytes()
    assert planes.cpu().numpy().tobytes() == t["residual_tt"].tobytes() and float(pk[0]) == res.peak_residual[0]
    abc = [E.beam_quadratic(*res.beam[0], np.radians(cell / 3600.))]
    hd = dev(Hinv)
    for k in range(2):
        ps = hd[k, 0] * planes[:, 0] + hd[k, 1] * planes[:, 1]
        tt = eng.restore(cp, cc[:, :, k].contiguous(), nc, abc, ni, nj, add=ps).cpu().numpy().reshape(ni, nj)
        # (the beam went through (bmaj, bmin, bpa) and back: not the same bits)
        assert np.allclose(tt, t["tt"][k], rtol=1e-9, atol=1e-9 * np.abs(t["tt"][k]).max()), k
    # alpha: NaN exactly below the cut
    cut = 0.1 * t["tt"][0].max()
    assert t["alpha_cut_jy"] == cut and t["beta"] is None
    hi = t["tt"][0] > cut
    assert hi.any() and (~hi).any() and np.array_equal(np.isnan(t["alpha"]), ~hi)
    assert np.array_equal(t["alpha"][hi], (t["tt"][1] / t["tt"][0])[hi])


def test_observe_ff_with_two_terms_runs_through_to_imfit(eng, example):
    jm, tr, cell = example
    peak = float(np.abs(jm.visibilities_ff([0.], [0.], FREQS[:1])).max())
    obs = jm.observe_ff(tr, FREQS, T_OBS, T_INT, sigma_jy=0.5 * peak, seed=5, nsigma=3., shape=SHAPE, cell_as=cell,
                        mfs=True, niter=60, nterms=2, imfit=True, weighting="briggs")
    c = obs.clean
    assert c.taylor is not None and len(c.taylor) == 1 and c.taylor[0]["tt"].shape == (2,) + SHAPE
    assert c.image.shape == (1,) + SHAPE and np.array_equal(c.image[0], c.taylor[0]["tt"][0])
    assert len(c.imfit) == 1 and np.isfinite(c.imfit[0]["peak"]) and c.imfit[0]["Ierr"]["val"] is not None
    n = len(c.components[0])
    assert c.components[0].shape == (n, 4) and (n == 60 or c.peak_residual[0] <= 3. * obs.image_rms[0])


def test_the_spectral_slope_of_the_components(eng, example):
    """The science check.  sum_c c_1 / sum_c c_0 -- the model's spectral slope at the reference frequency --
    against the slope s_1 / s_0 of a weighted two-term least-squares fit in w of the model's own channel
    totals (nansum of the flux_ff maps; the weights are the channels' shares of the imaging weights,
    equal here).  How close the two come is not derivable: Taylor truncation (the spectrum is a power law,
    not a line in w) and the unsampled zero spacing both enter.  Measured on the first GPU run:
    ALPHA_MEASURED = 2.060e-3 in the slope (0.11 % of it); asserted: twice that, the factor 2 covering the
    spread between machines."""
    jm, tr, cell = example
    res = jm.clean_image_ff(tr.u_m, tr.v_m, FREQS, shape=SHAPE, cell_as=cell, mfs=True, nterms=2, niter=300,
                            gain=0.1, threshold_jy=0.0)
    comp = res.components[0]
    got = float(comp[:, 3].sum() / comp[:, 2].sum())
    totals = np.array([np.nansum(m) for m in jm.flux_ff(FREQS)])
    w = (FREQS - 5e9) / 5e9
    A = np.stack([np.ones_like(w), w], axis=1)
    s0, s1 = np.linalg.lstsq(A, totals, rcond=None)[0]
    want = float(s1 / s0)
    dev = abs(got - want)
    print("\nspectral slope: components %.6f, fit %.6f, deviation %.3e (alpha %.4f against %.4f); "
          "sum c_0 %.6e Jy against s_0 %.6e Jy" % (got, want, dev, got, want, comp[:, 2].sum(), s0))
    assert dev <= ALPHA_TOL, (got, want, dev)
