"""rjp_clean (K12, clean.hip: Hogbom CLEAN minor cycles on a stack of images) and rjp_restore (K13:
clean components convolved with the clean beam, plus the residual) through the C-ABI,
RTEngine.clean / restore and JetModel.clean_image_*, against tests/clean_ref.py -- a long-double
NumPy Hogbom that FOLLOWS the device's component list instead of comparing pick sequences, which
tests/test_clean_reference_cpu.py pins to hand-worked cases, to a float64 emulation (inside the
bound) and to four planted mistakes (outside).

The bound is derived in tests/clean_ref.py, not measured: per pixel
    b[q] = (updates of q) x 1 rounding (the update is one fma) x 2^-53 x (|D[q]| + sum_c |f_c| |B|).
The module prints the worst error / bound per group."""
import copy

import numpy as np
import pytest

from tests import clean_ref as K
from tests import gpu_util as U
from tests import vis_ref as R

pytestmark = pytest.mark.gpu
YEAR = 31557600.0
LD = np.longdouble
WORST = {}
POISON_PIX, POISON_F = -77, 7.25
GUARD = 33                             # elements of guard band on either side (odd: the payload of
                                       # a float64 buffer then starts 8 bytes off a 16-byte line)


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()
    print("\nworst error / bound per group: " +
          ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def note(kind, r):
    WORST[kind] = max(WORST.get(kind, 0.0), float(r))
    assert r <= 1.0, (kind, r)


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


def run_clean(eng, D, B, mask, thresh, gain, n_iter, model0=None, want_peak=True, guard=GUARD):
    """One raw rjp_clean call on D [M, nx, nz] with B [n_psf, px, pz], every buffer between guard
    bands -> dict of host arrays (res, cpix, cflux, ncomp, model, peak, work, ret)."""
    import torch
    from rajepy_amd import _lib
    M, nx, nz = D.shape
    n_psf, px, pz = B.shape
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    res = Band(eng, D.size, f64, -1e300, guard).set(D)
    psf = Band(eng, B.size, f64, 1e300, guard).set(B)
    cpix = Band(eng, M * n_iter, i32, POISON_PIX)
    cflux = Band(eng, M * n_iter, f64, POISON_F)
    ncomp = Band(eng, M, i32, POISON_PIX)
    model = Band(eng, D.size, f64, -1e300).set(np.zeros(D.size) if model0 is None else model0)
    peak = Band(eng, M, f64, POISON_F)
    wb = eng.lib.rjp_clean_workspace(M, nx, nz)
    assert wb == K.workspace_bytes(M, nx, nz)
    work = Band(eng, wb, u8, 0xA5, 64)
    dmask = Band(eng, nx * nz, u8, 1, 3).set(np.asarray(mask != 0, dtype=np.uint8)) if mask is not None else None
    ret = eng.lib.rjp_clean(eng.ctx, res.ptr, M, nx, nz, psf.ptr, n_psf, px, pz,
                            dmask.ptr if dmask else None, _lib.dbl_array(np.broadcast_to(thresh, (M,))),
                            float(gain), n_iter, cpix.ptr, cflux.ptr, ncomp.ptr, model.ptr,
                            peak.ptr if want_peak else None, work.ptr, wb, eng._stream())
    eng.synchronize()
    assert ret == K.tiling(M, nx, nz)["workgroups"], (ret, eng.lib.rjp_last_error(eng.ctx))
    psf.get()
    if dmask:
        dmask.get()
    return dict(res=res.get().reshape(D.shape), cpix=cpix.get().reshape(M, n_iter),
                cflux=cflux.get().reshape(M, n_iter), ncomp=ncomp.get(),
                model=model.get().reshape(D.shape), peak=peak.get(), work=work.get(), ret=ret)


def follow_all(kind, D, B, mask, thresh, gain, n_iter, out, model0=None, want_peak=True):
    M = D.shape[0]
    th = np.broadcast_to(thresh, (M,))
    for m in range(M):
        Bm = B[m if B.shape[0] > 1 else 0]
        r = K.follow(D[m], Bm, mask, th[m], gain, n_iter, out["cpix"][m], out["cflux"][m],
                     out["ncomp"][m], out["res"][m], peak=out["peak"][m] if want_peak else None,
                     model=out["model"][m], model0=None if model0 is None else model0[m],
                     poison_pix=POISON_PIX, poison_flux=POISON_F)
        note(kind, r)
        note(kind + " (conservation)", K.conservation(D[m], Bm, out["cpix"][m], out["cflux"][m],
                                                      out["ncomp"][m], out["res"][m]))
    if not want_peak:
        assert np.all(out["peak"] == POISON_F), "d_peak = NULL was written"


def same_bits(a, b):
    for k in ("res", "cpix", "cflux", "ncomp", "model", "peak", "work"):
        assert a[k].tobytes() == b[k].tobytes(), "a repeated call changed " + k


def inputs(seed, M, n_psf, nx, nz, px, pz, nan=False, corners=False):
    """M images of a few point sources convolved with the beam(s) [n_psf, px, pz] (windows of
    random-coverage beams) plus noise at 1e-3 of the peak."""
    rng = np.random.default_rng(seed)
    B = np.stack([K.random_beam(rng, px, pz) for _ in range(n_psf)])
    D = np.empty((M, nx, nz))
    for m in range(M):
        src = None
        if corners:
            src = [(0, 0, 1.0), (nx - 1, nz - 1, -0.9), (nx // 2, nz // 3, 0.6)]
        D[m] = K.random_image(rng, nx, nz, B[m if n_psf > 1 else 0], sources=src)
        if nan:
            D[m].ravel()[rng.choice(nx * nz, max(1, nx * nz // 50), replace=False)] = np.nan
            D[m, nx // 2, nz // 2] = np.inf
    return D, B


def box(nx, nz):
    mask = np.zeros((nx, nz), dtype=bool)
    mask[nx // 5:nx - nx // 6, nz // 4:nz] = True
    return mask


# ---- 1: the shapes, at the bound ------------------------------------------------------------------
def test_one_pixel(eng):
    D, B = np.array([[[0.75]]]), np.array([[[1.0]]])
    out = run_clean(eng, D, B, None, 0.0, 0.5, 37)
    assert out["ncomp"][0] == 37 and np.all(out["cpix"] == 0)
    assert out["cflux"][0, 0] == 0.375 and out["res"][0, 0, 0] == 0.75 * 0.5 ** 37
    follow_all("1 x 1", D, B, None, 0.0, 0.5, 37, out)
    out = run_clean(eng, D, B, None, 0.0, 1.0, 3)             # gain 1 empties it: one component
    assert out["ncomp"][0] == 1 and out["res"][0, 0, 0] == 0.0 and out["peak"][0] == 0.0
    follow_all("1 x 1", D, B, None, 0.0, 1.0, 3, out)


def test_five_by_three(eng):
    for case, (M, n_psf) in enumerate(((1, 1), (3, 1), (3, 3))):
        D, B = inputs(50 + case, M, n_psf, 5, 3, 9, 5, nan=case == 2, corners=case == 1)
        for gain, n_iter in ((0.1, 37), (1.0, 1), (1.0, 300)):
            mask = box(5, 3) if n_iter == 37 else None
            out = run_clean(eng, D, B, mask, 0.0, gain, n_iter)
            follow_all("5 x 3", D, B, mask, 0.0, gain, n_iter, out)


@pytest.mark.parametrize("nx,nz,px,pz", [(67, 131, 133, 261), (67, 131, 31, 31), (130, 65, 259, 129)])
def test_tails_and_tiles_against_the_reference(eng, nx, nz, px, pz):
    """Nine tiles with a tail, full Hogbom and a windowed beam; 1 and 3 maps with 1 and 3 beams; no
    mask and a box; 1, 37 and 300 iterations; gain 0.1 and 1; thresholds of 0, mid-way and above the
    peak; NaN and infinite pixels; sources at (0, 0) and (nx - 1, nz - 1); a repeated call."""
    kind = "%d x %d beam %d x %d" % (nx, nz, px, pz)
    combos = [  # M, n_psf, mask, n_iter, gain, thresh, nan, corners
        (1, 1, False, 300, 0.1, "zero", False, True),
        (3, 3, True, 37, 0.1, "mid", False, True),
        (3, 1, False, 37, 1.0, "zero", True, False),
        (1, 1, True, 1, 1.0, "zero", False, True),
        (3, 3, False, 300, 0.1, "mid", True, False),
        (3, 1, False, 37, 0.1, "above", False, False),
    ]
    for i, (M, n_psf, masked, n_iter, gain, th, nan, corners) in enumerate(combos):
        D, B = inputs(1000 * nx + 10 * px + i, M, n_psf, nx, nz, px, pz, nan=nan, corners=corners)
        mask = box(nx, nz) if masked else None
        top = np.array([np.abs(D[m][K.candidates(D[m], mask)]).max() for m in range(M)])
        thresh = {"zero": 0.0, "mid": 0.5 * top, "above": 1.5 * top}[th]
        out = run_clean(eng, D, B, mask, thresh, gain, n_iter)
        follow_all(kind, D, B, mask, thresh, gain, n_iter, out)
        if th == "above":
            assert np.all(out["ncomp"] == 0) and out["res"].tobytes() == D.tobytes()
            assert np.all(out["model"] == 0) and np.array_equal(out["peak"], top)
        if th == "mid":
            assert np.all(out["ncomp"] > 0) and np.all(out["ncomp"] < n_iter) and np.all(out["peak"] <= thresh)
        if th == "zero" and not nan:
            assert np.all(out["ncomp"] == n_iter)
        if corners and not masked:
            assert out["cpix"][0, 0] in (0, nx * nz - 1)
        if i in (1, 4):
            same_bits(out, run_clean(eng, D, B, mask, thresh, gain, n_iter))
    # the 16-byte path and the 8-byte one (a map base 8 bytes off) give the same bits
    D, B = inputs(77, 2, 1, nx, nz, px, pz)
    a = run_clean(eng, D, B, None, 0.0, 0.1, 37, guard=GUARD)
    b = run_clean(eng, D, B, None, 0.0, 0.1, 37, guard=GUARD + 1)
    for k in ("res", "cpix", "cflux", "ncomp", "model", "peak"):
        assert a[k].tobytes() == b[k].tobytes(), k
    # d_peak = NULL: one launch fewer, nothing else differs
    c = run_clean(eng, D, B, None, 0.0, 0.1, 37, want_peak=False)
    follow_all(kind, D, B, None, 0.0, 0.1, 37, c, want_peak=False)
    assert c["res"].tobytes() == a["res"].tobytes() and c["cflux"].tobytes() == a["cflux"].tobytes()


def test_more_tiles_than_one_reduction_pass(eng):
    nx = nz = 600
    assert K.tiling(1, nx, nz)["tiles"] == 352 > K.REDUCE_PASS
    rng = np.random.default_rng(600)
    B = K.random_beam(rng, 15, 15)[None]
    # the strongest sources in tiles beyond the first pass (pixels past 256 x 1024), and in the last
    src = [(599, 599, 1.0), (450, 17, -0.9), (0, 0, 0.8), (300, 300, 0.7), (437, 0, 0.6)]
    assert 450 * nz + 17 > K.REDUCE_PASS * K.TILE
    D = K.random_image(rng, nx, nz, B[0], sources=src)[None]
    out = run_clean(eng, D, B, None, 0.0, 0.5, 20)
    assert out["ncomp"][0] == 20 and out["cpix"][0, 0] == 599 * nz + 599 and out["cpix"][0, 1] == 450 * nz + 17
    follow_all("600 x 600", D, B, None, 0.0, 0.5, 20, out)


# ---- 2: behaviour ------------------------------------------------------------------------------------
def test_all_zero_mask_touches_nothing(eng):
    D, B = inputs(5, 3, 1, 67, 131, 31, 31)
    m0 = np.arange(D.size, dtype=np.float64)
    out = run_clean(eng, D, B, np.zeros((67, 131)), 0.0, 0.1, 37, model0=m0)
    assert np.all(out["ncomp"] == 0) and np.all(out["peak"] == 0.0)
    assert out["res"].tobytes() == D.tobytes() and np.array_equal(out["model"].ravel(), m0)
    assert np.all(out["cpix"] == POISON_PIX) and np.all(out["cflux"] == POISON_F)


def test_a_continued_call_equals_one_long_call(eng):
    nx, nz = 67, 131
    D, B = inputs(9, 3, 3, nx, nz, 133, 261)
    n1, n2, gain = 37, 63, 0.1
    first = run_clean(eng, D, B, None, 0.0, gain, n1)
    assert np.all(first["ncomp"] == n1)
    second = run_clean(eng, first["res"], B, None, 0.0, gain, n2, model0=first["model"])
    long = run_clean(eng, D, B, None, 0.0, gain, n1 + n2)
    joined = dict(second, cpix=np.concatenate([first["cpix"], second["cpix"]], axis=1),
                  cflux=np.concatenate([first["cflux"], second["cflux"]], axis=1),
                  ncomp=first["ncomp"] + second["ncomp"])
    follow_all("continued", D, B, None, 0.0, gain, n1 + n2, joined)
    follow_all("continued", D, B, None, 0.0, gain, n1 + n2, long)
    # the same arithmetic in the same order: here even the same bits
    assert joined["cpix"].tobytes() == long["cpix"].tobytes()
    assert joined["cflux"].tobytes() == long["cflux"].tobytes()
    assert second["res"].tobytes() == long["res"].tobytes()
    assert second["model"].tobytes() == long["model"].tobytes()


def test_engine_clean_and_restore(eng):
    import torch
    nx, nz = 67, 131
    D, B = inputs(21, 3, 1, nx, nz, 31, 31)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(eng.device)
    res, model = dev(D.reshape(3, -1)), torch.zeros(3, nx * nz, dtype=torch.float64, device=eng.device)
    mask = box(nx, nz)
    cpix, cflux, ncomp, peak = eng.clean(res, nx, nz, dev(B), 31, 31, 37, 0.1, 0.0, mask=mask, model=model)
    assert eng.last_clean_tiles == 27
    assert cpix.shape == (3, 37) and cpix.dtype == torch.int32 and ncomp.dtype == torch.int32
    raw = run_clean(eng, D, B, mask, 0.0, 0.1, 37)
    assert cpix.cpu().numpy().tobytes() == raw["cpix"].tobytes()
    assert cflux.cpu().numpy().tobytes() == raw["cflux"].tobytes()
    assert res.cpu().numpy().tobytes() == raw["res"].tobytes()
    assert model.cpu().numpy().tobytes() == raw["model"].tobytes()
    assert peak.cpu().numpy().tobytes() == raw["peak"].tobytes()
    abc = (0.11, 0.03, 0.07)
    img = eng.restore(cpix, cflux, ncomp, abc, nx, nz, add=res)
    bare = eng.restore(cpix, cflux, ncomp, [abc] * 3, nx, nz)
    assert (bare.cpu().numpy() + res.cpu().numpy()).tobytes() == img.cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        eng.clean(res, nx, nz, dev(B), 31, 31, 0, 0.1, 0.0)
    with pytest.raises(ValueError):
        eng.clean(res[:, :-1].contiguous(), nx, nz, dev(B), 31, 31, 5, 0.1, 0.0)
    with pytest.raises(ValueError):
        eng.clean(res, nx, nz, dev(B[:, :, :-1]), 31, 31, 5, 0.1, 0.0)
    with pytest.raises(ValueError):
        eng.clean(res, nx, nz, dev(B), 31, 31, 5, 0.1, [0.0, 0.0])
    with pytest.raises(ValueError):
        eng.clean(res, nx, nz, dev(B), 31, 31, 5, 0.1, 0.0, mask=np.ones(5))
    with pytest.raises(ValueError):
        eng.restore(cpix, cflux, ncomp, [abc] * 2, nx, nz)
    with pytest.raises(ValueError):
        eng.restore(cpix.to(torch.int64), cflux, ncomp, abc, nx, nz)


# ---- 3: refusals --------------------------------------------------------------------------------------
C_NULLS = "rjp_clean: NULL images, beams, thresholds or component outputs"
C_SIZES = "rjp_clean: n_maps, nx, nz, px and pz must be positive"
C_ODD = "rjp_clean: px and pz must be odd (the beam's centre is a pixel)"
C_NPSF = "rjp_clean: n_psf must be 1 or n_maps"
C_NPIX = "rjp_clean: nx * nz exceeds 2^31 - 1"
C_GAIN = "rjp_clean: gain must lie in (0, 1]"
C_ITER = "rjp_clean: n_iter < 1"
C_THR = "rjp_clean: negative or non-finite threshold"
C_SHORT = "rjp_clean: workspace smaller than rjp_clean_workspace()"
R_NULLS = "rjp_restore: NULL components, beams or output"
R_SIZES = "rjp_restore: n_maps, comp_stride, nx and nz must be positive"
R_NPIX = "rjp_restore: nx * nz exceeds 2^31 - 1"
R_BEAM = "rjp_restore: the beam (A, B, C) must be positive definite"


def test_refusals_leave_poisoned_outputs_untouched(eng):
    import torch
    from rajepy_amd import _lib
    M, nx, nz, px, pz, n_iter = 2, 5, 3, 9, 5, 4
    f64, i32, u8 = torch.float64, torch.int32, torch.uint8
    full = lambda n, v, dt: torch.full((n,), v, dtype=dt, device=eng.device)
    wb = eng.lib.rjp_clean_workspace(M, nx, nz)
    bufs = dict(res=full(M * nx * nz, 7.0, f64), psf=full(M * px * pz, 0.5, f64),
                mask=full(nx * nz, 1, u8), cpix=full(M * n_iter, POISON_PIX, i32),
                cflux=full(M * n_iter, POISON_F, f64), ncomp=full(M, POISON_PIX, i32),
                model=full(M * nx * nz, 3.0, f64), peak=full(M, POISON_F, f64), work=full(wb, 0xA5, u8))
    before = {k: t.clone() for k, t in bufs.items()}
    good = dict(bufs, n_maps=M, nx=nx, nz=nz, n_psf=M, px=px, pz=pz, thresh=[0.0, 0.1], gain=0.1,
                n_iter=n_iter, nbytes=wb, ctx=True)
    ptr = lambda t: t.data_ptr() if t is not None else None

    def clean(a):
        return eng.lib.rjp_clean(eng.ctx if a["ctx"] else None, ptr(a["res"]), a["n_maps"], a["nx"], a["nz"],
                                 ptr(a["psf"]), a["n_psf"], a["px"], a["pz"], ptr(a["mask"]),
                                 _lib.dbl_array(a["thresh"]) if a["thresh"] is not None else None,
                                 a["gain"], a["n_iter"], ptr(a["cpix"]), ptr(a["cflux"]), ptr(a["ncomp"]),
                                 ptr(a["model"]), ptr(a["peak"]), ptr(a["work"]), a["nbytes"], eng._stream())

    ARG, WS = _lib.RJP_ERR_ARG, _lib.RJP_ERR_WORKSPACE
    big = 2 ** 31 - 1
    cases = [("NULL d_res", dict(res=None), ARG, C_NULLS), ("NULL d_psf", dict(psf=None), ARG, C_NULLS),
             ("NULL h_thresh", dict(thresh=None), ARG, C_NULLS), ("NULL d_cpix", dict(cpix=None), ARG, C_NULLS),
             ("NULL d_cflux", dict(cflux=None), ARG, C_NULLS), ("NULL d_ncomp", dict(ncomp=None), ARG, C_NULLS),
             ("n_maps = 0", dict(n_maps=0), ARG, C_SIZES), ("nx < 0", dict(nx=-1), ARG, C_SIZES),
             ("nz = 0", dict(nz=0), ARG, C_SIZES), ("px = 0", dict(px=0), ARG, C_SIZES),
             ("pz < 0", dict(pz=-5), ARG, C_SIZES),
             ("even px", dict(px=8), ARG, C_ODD), ("even pz", dict(pz=4), ARG, C_ODD),
             ("n_psf = 0", dict(n_psf=0), ARG, C_NPSF), ("n_psf = 3", dict(n_psf=3), ARG, C_NPSF),
             ("too many pixels", dict(nx=big, nz=big), ARG, C_NPIX),
             ("gain = 0", dict(gain=0.0), ARG, C_GAIN), ("gain > 1", dict(gain=1.0000001), ARG, C_GAIN),
             ("gain < 0", dict(gain=-0.1), ARG, C_GAIN), ("NaN gain", dict(gain=np.nan), ARG, C_GAIN),
             ("n_iter = 0", dict(n_iter=0), ARG, C_ITER), ("n_iter < 0", dict(n_iter=-3), ARG, C_ITER),
             ("negative threshold", dict(thresh=[0.0, -1e-9]), ARG, C_THR),
             ("NaN threshold", dict(thresh=[np.nan, 0.0]), ARG, C_THR),
             ("infinite threshold", dict(thresh=[0.0, np.inf]), ARG, C_THR),
             ("a short workspace", dict(nbytes=wb - 1), WS, C_SHORT),
             ("no workspace", dict(work=None), WS, C_SHORT)]
    for what, kw, want, msg in cases:
        assert clean(dict(good, **kw)) == want, what
        assert eng.lib.rjp_last_error(eng.ctx).decode() == msg, what
    assert clean(dict(good, ctx=False)) == ARG
    assert eng.lib.rjp_last_error(None).decode() == "null context"

    out = full(M * nx * nz, 7.0, f64)

    def restore(**kw):
        a = dict(cpix=bufs["cpix"], cflux=bufs["cflux"], ncomp=bufs["ncomp"], n_maps=M, stride=n_iter,
                 beam=[0.5, 0.1, 0.4, 0.2, 0.0, 0.3], add=bufs["res"], nx=nx, nz=nz, out=out, ctx=True)
        a.update(kw)
        return eng.lib.rjp_restore(eng.ctx if a["ctx"] else None, ptr(a["cpix"]), ptr(a["cflux"]),
                                   ptr(a["ncomp"]), a["n_maps"], a["stride"],
                                   _lib.dbl_array(a["beam"]) if a["beam"] is not None else None,
                                   ptr(a["add"]), a["nx"], a["nz"], ptr(a["out"]), eng._stream())

    ok = [0.5, 0.1, 0.4]
    rcases = [("NULL d_cpix", dict(cpix=None), R_NULLS), ("NULL d_cflux", dict(cflux=None), R_NULLS),
              ("NULL d_ncomp", dict(ncomp=None), R_NULLS), ("NULL h_beam", dict(beam=None), R_NULLS),
              ("NULL d_out", dict(out=None), R_NULLS),
              ("n_maps = 0", dict(n_maps=0), R_SIZES), ("comp_stride = 0", dict(stride=0), R_SIZES),
              ("nx < 0", dict(nx=-2), R_SIZES), ("nz = 0", dict(nz=0), R_SIZES),
              ("too many pixels", dict(nx=big, nz=big), R_NPIX),
              ("A = 0", dict(beam=ok + [0.0, 0.0, 0.3]), R_BEAM), ("C < 0", dict(beam=ok + [0.2, 0.0, -0.3]), R_BEAM),
              ("A C = B^2", dict(beam=[0.25, 0.5, 1.0] + ok), R_BEAM),
              ("A C < B^2", dict(beam=ok + [0.2, 0.3, 0.3]), R_BEAM),
              ("NaN beam", dict(beam=ok + [0.2, np.nan, 0.3]), R_BEAM),
              ("infinite beam", dict(beam=[np.inf, 0.0, 0.3] + ok), R_BEAM)]
    for what, kw, msg in rcases:
        assert restore(**kw) == ARG, what
        assert eng.lib.rjp_last_error(eng.ctx).decode() == msg, what
    assert restore(ctx=False) == ARG
    eng.synchronize()
    for k, t in bufs.items():
        assert torch.equal(t, before[k]), k + " was touched by a refusal"
    assert bool((out == 7.0).all())
    # the context still serves a valid call of each; NULL mask, model, peak and add are no refusals
    assert clean(dict(good, mask=None, model=None, peak=None)) == K.tiling(M, nx, nz)["workgroups"] == 2
    eng.synchronize()
    assert not bool((bufs["ncomp"] == POISON_PIX).any()) and torch.equal(bufs["model"], before["model"])
    assert restore(add=None) == 2                         # ceil(15 / 256) workgroups x 2 maps
    eng.synchronize()
    assert not bool((out == 7.0).any())


# ---- 4: restore ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nz,S", [(1, 1, 1), (5, 3, 4), (67, 131, 300), (130, 65, 40)])
def test_restore_against_the_long_double_sum(eng, nx, nz, S):
    """Against the long-double sum, per pixel at exp_any's stated error plus the accumulation
    (clean_ref.restore_ref); d_add NULL and given, ncomp = 0 and = the stride, more components than
    one LDS chunk (300 > 256), a beam so narrow that the neighbours underflow."""
    import torch
    rng = np.random.default_rng(nx + nz + S)
    M = 3
    ncomp = np.array([S, 0, max(1, S // 2)], dtype=np.int32)
    cpix = rng.integers(0, nx * nz, (M, S)).astype(np.int32)
    cflux = rng.standard_normal((M, S))
    for m in range(M):                                     # beyond ncomp: poison, never read
        cpix[m, ncomp[m]:] = 2 ** 31 - 1
        cflux[m, ncomp[m]:] = np.nan
    abc = np.array([[0.05, 0.02, 0.08], [0.3, -0.1, 0.2], [900.0, 0.0, 800.0]])
    add = rng.standard_normal((M, nx * nz))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    d = dev(cpix), dev(cflux), dev(ncomp)
    for with_add in (False, True):
        got = eng.restore(*d, abc, nx, nz, add=dev(add) if with_add else None).cpu().numpy()
        for m in range(M):
            ref, bnd = K.restore_ref(cpix[m], cflux[m], ncomp[m], abc[m], nx, nz, add[m] if with_add else None)
            err = np.abs(got[m].reshape(nx, nz).astype(LD) - ref).astype(np.float64)
            assert np.all(err <= bnd), (m, with_add, float((err - bnd).max()))
            if (bnd > 0).any():
                note("restore", float((err[bnd > 0] / bnd[bnd > 0]).max()))
        assert got[1].tobytes() == (add[1] if with_add else np.zeros(nx * nz)).tobytes(), "ncomp = 0"
        if not with_add:
            # the narrow beam: every component adds its flux to its own pixel and exact zeros elsewhere
            want = np.zeros(nx * nz)
            for c in range(ncomp[2]):
                want[cpix[2, c]] += cflux[2, c]
            assert np.array_equal(got[2] != 0, want != 0) and np.allclose(got[2], want, rtol=1e-13, atol=0)
    again = eng.restore(*d, abc, nx, nz, add=dev(add)).cpu().numpy()
    assert again.tobytes() == got.tobytes()


# ---- 5: the chain vis -> vis_adjoint -> clean, and the golden models through JetModel ---------------
def test_three_delta_pixels_come_back(eng):
    """A map with three delta pixels through rjp_vis, rjp_vis_adjoint and rjp_clean: every component
    lies on one of the three pixels, and per source the summed flux F_j misses S_j by at most
    peak_residual / (1 - s), s = the largest sum of |beam| between one source and the others:
    R = sum_j (S_j - F_j) B(. - p_j) exactly, so at source i  |S_i - F_i| <= |R(p_i)| + s max_j |S_j - F_j|
    (plus the direct sums' own rounding, 1e-12 here)."""
    import torch
    nx, nz, Kv = 15, 17, 400
    rng = np.random.default_rng(15)
    u, v = R.random_points(rng, Kv, 0.5)
    src = {(3, 4): 1.0, (10, 12): 0.7, (7, 2): -0.5}
    I = np.zeros((nx, nz))
    for (ix, iz), s in src.items():
        I[ix, iz] = s
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(eng.device)
    V = eng.vis(dev(I.reshape(1, -1)), nx, nz, [1.0], [1.0], u, v)
    dirty = eng.vis_adjoint(V, nx, nz, [1.0], [1.0], u, v) / Kv
    ones = torch.view_as_complex(dev(np.stack([np.ones((1, Kv)), np.zeros((1, Kv))], axis=-1)))
    psf = eng.vis_adjoint(ones, 2 * nx - 1, 2 * nz - 1, [1.0], [1.0], u, v) / Kv
    Bh = psf.cpu().numpy().reshape(2 * nx - 1, 2 * nz - 1)
    assert Bh[nx - 1, nz - 1] == 1.0
    thresh = 1e-4
    cpix, cflux, ncomp, peak = eng.clean(dirty, nx, nz, psf, 2 * nx - 1, 2 * nz - 1, 500, 0.1, thresh)
    n, peak = int(ncomp.cpu()[0]), float(peak.cpu()[0])
    hp, hf = cpix.cpu().numpy()[0, :n], cflux.cpu().numpy()[0, :n]
    assert 0 < n < 500 and peak <= thresh
    assert {(int(p) // nz, int(p) % nz) for p in hp} == set(src)
    pos = list(src)
    s = max(sum(abs(Bh[nx - 1 + a[0] - b[0], nz - 1 + a[1] - b[1]]) for b in pos if b != a) for a in pos)
    assert s < 0.5
    for (ix, iz), want in src.items():
        F = hf[hp == ix * nz + iz].sum()
        assert abs(F - want) <= peak / (1 - s) + 1e-12, ((ix, iz), F, want)


def _params(tag):
    p = copy.deepcopy(U.load_golden(tag)[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


_MODELS = {}
SHAPE = (15, 21)


def model(eng, tag, tmp_path_factory):
    from rajepy_amd import classes, logger
    if tag not in _MODELS:
        log = logger.Log(str(tmp_path_factory.mktemp("clean") / (tag + ".log")), verbose=False)
        _MODELS[tag] = classes.JetModel(_params(tag), log=log, engine=eng)
    return _MODELS[tag]


def baselines(jm, freqs, n=60, amax=0.15, seed=3):
    """Baselines in metres that reach `amax` cycles per model cell at the highest frequency (a beam
    of about four cells, so that its main lobe is resolved); weights over a decade.  Fewer than 64,
    so that rjp_vis_adjoint never splits them over workgroups: a map's dirty image then has the
    same bits whatever the number of maps in the call."""
    su, _ = jm._vis_scales(freqs)
    rng = np.random.default_rng(seed)
    u, v = R.random_points(rng, n, amax / np.abs(su).max())
    return u, v, rng.lognormal(0.0, 0.5, n)


def check_result(kind, res, D, B, niter, thresh, gain, mask=None):
    """A CleanResult against the dirty images D and beams B (host, from dirty_image_* / dirty_beam
    with the same arguments): conservation and the follow rule per map, the stopping rule, the model."""
    M, ni, nj = D.shape
    assert res.image.shape == res.residual.shape == res.model.shape == D.shape
    assert len(res.components) == len(res.beam) == M and res.peak_residual.shape == (M,)
    for m in range(M):
        comp = res.components[m]
        n = len(comp)
        cpix = (comp[:, 0] * nj + comp[:, 1]).astype(np.int64)
        note(kind + " (conservation)", K.conservation(D[m], B[m], cpix, comp[:, 2], n, res.residual[m]))
        rows_p = np.concatenate([cpix, np.full(niter - n, POISON_PIX)])
        rows_f = np.concatenate([comp[:, 2], np.full(niter - n, POISON_F)])
        note(kind, K.follow(D[m], B[m], mask, thresh, gain, niter, rows_p, rows_f, n, res.residual[m],
                            peak=res.peak_residual[m], model=res.model[m]))
        assert res.peak_residual[m] <= thresh or n == niter
        bmaj, bmin, bpa = res.beam[m]
        assert bmaj >= bmin > 0 and -90 < bpa <= 90


def test_clean_image_ff_on_the_example_model(eng, tmp_path_factory):
    import torch
    from rajepy_amd import engine as E
    jm = model(eng, "cfg1_example", tmp_path_factory)
    freqs = np.asarray(U.load_golden("cfg1_example")[0]["freqs"], dtype=np.float64)[:3]
    jm.time = 1.0 * YEAR
    u, v, w = baselines(jm, freqs)
    D = jm.dirty_image_ff(u, v, freqs, weights=w, shape=SHAPE)
    B = jm.dirty_beam(u, v, freqs, weights=w, shape=(2 * SHAPE[0] - 1, 2 * SHAPE[1] - 1))
    thresh = 0.02 * float(np.abs(D).max())
    res = jm.clean_image_ff(u, v, freqs, weights=w, shape=SHAPE, niter=60, threshold_jy=thresh)
    check_result("clean_image_ff", res, D, B, 60, thresh, 0.1)
    assert all(len(c) > 0 for c in res.components)
    # a given beam: image = restore(components) + residual, to the bit
    cell = np.arctan(jm.csize * E.con.au / (jm.params["target"]["dist"] * E.con.parsec))
    beam = res.beam[0]
    giv = jm.clean_image_ff(u, v, freqs, weights=w, shape=SHAPE, niter=60, threshold_jy=thresh, beam=beam)
    assert giv.residual.tobytes() == res.residual.tobytes() and giv.model.tobytes() == res.model.tobytes()
    abc = E.beam_quadratic(*beam, cell)
    for m in range(3):
        comp = giv.components[m]
        S = max(1, len(comp))
        cp = np.zeros((1, S), dtype=np.int32)
        cf = np.zeros((1, S))
        cp[0, :len(comp)] = comp[:, 0] * SHAPE[1] + comp[:, 1]
        cf[0, :len(comp)] = comp[:, 2]
        dev = lambda a: torch.from_numpy(a).to(eng.device)
        bare = eng.restore(dev(cp), dev(cf), dev(np.array([len(comp)], dtype=np.int32)), abc, *SHAPE)
        assert (bare.cpu().numpy().reshape(SHAPE) + giv.residual[m]).tobytes() == giv.image[m].tobytes()
        assert np.allclose(E.beam_quadratic(*giv.beam[m], cell), abc, rtol=1e-9, atol=1e-12)
        # the fitted beam of map 0 is this one: the same image there within the round trip
        if m == 0:
            assert np.abs(res.image[0] - giv.image[0]).max() <= 1e-9 * np.abs(comp[:, 2]).sum()
    # a box mask, a windowed beam, chunks of one map (the stack limit below two maps' buffers)
    mask = (3, 11, 5, 16)
    Bw = jm.dirty_beam(u, v, freqs, weights=w, shape=(9, 11))
    old = jm.VIS_STACK_BYTES
    try:
        jm.VIS_STACK_BYTES = 8 * (3 * SHAPE[0] * SHAPE[1] + 9 * 11)
        box_res = jm.clean_image_ff(u, v, freqs, weights=w, shape=SHAPE, niter=40, gain=0.2,
                                    threshold_jy=thresh, mask=mask, psf_shape=(9, 11))
    finally:
        jm.VIS_STACK_BYTES = old
    mk = np.zeros(SHAPE, dtype=bool)
    mk[3:12, 5:17] = True
    check_result("clean_image_ff (box, window)", box_res, D, Bw, 40, thresh, 0.2, mask=mk)
    for c in box_res.components:
        assert np.all((c[:, 0] >= 3) & (c[:, 0] <= 11) & (c[:, 1] >= 5) & (c[:, 1] <= 16))
    with pytest.raises(ValueError):
        jm.clean_image_ff(u, v, freqs, shape=SHAPE, psf_shape=(8, 11))
    with pytest.raises(ValueError):
        jm.clean_image_ff(u, v, freqs, shape=SHAPE, gain=0.0)


def test_clean_image_mfs_formal_and_one_line(eng, tmp_path_factory):
    jm = model(eng, "cfg1_example", tmp_path_factory)
    z, meta, _ = U.load_golden("cfg1_example")
    freqs = np.asarray(z["freqs"], dtype=np.float64)[:2]
    jm.time = 1.0 * YEAR
    u, v, w = baselines(jm, freqs)
    full = (2 * SHAPE[0] - 1, 2 * SHAPE[1] - 1)
    D = jm.dirty_image_ff(u, v, freqs, weights=w, shape=SHAPE, mfs=True)
    B = jm.dirty_beam(u, v, freqs, weights=w, shape=full, mfs=True)
    res = jm.clean_image_ff(u, v, freqs, weights=w, shape=SHAPE, mfs=True, niter=50)
    assert res.image.shape == (1,) + SHAPE
    check_result("mfs", res, D, B, 50, 0.0, 0.1)
    rf = np.asarray(z["rrl_freqs"], dtype=np.float64)[3:5]
    u, v, w = baselines(jm, rf)
    D = jm.dirty_image_rrl(meta["rrl"], u, v, rf, weights=w, shape=SHAPE, contsub=False)
    B = jm.dirty_beam(u, v, rf, weights=w, shape=full)
    res = jm.clean_image_rrl(meta["rrl"], u, v, rf, weights=w, shape=SHAPE, contsub=False, niter=50)
    check_result("clean_image_rrl", res, D, B, 50, 0.0, 0.1)
    jt = model(eng, "tilted", tmp_path_factory)
    ft = np.asarray(U.load_golden("tilted")[0]["freqs"], dtype=np.float64)
    jt.time = 0.4 * YEAR
    u, v, w = baselines(jt, ft)
    D = jt.dirty_image_ff(u, v, ft, weights=w, shape=SHAPE, formal=True)
    B = jt.dirty_beam(u, v, ft, weights=w, shape=full)
    res = jt.clean_image_ff(u, v, ft, weights=w, shape=SHAPE, formal=True, niter=50)
    check_result("formal", res, D, B, 50, 0.0, 0.1)
    plain = jt.clean_image_ff(u, v, ft, weights=w, shape=SHAPE, niter=50)
    assert np.abs(plain.image - res.image).max() > 0
