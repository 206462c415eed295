"""rjp_vis_adjoint (K11) without a GPU: the long-double reference the GPU tests hold the kernel to
(tests/vis_adjoint_ref.py) against the inverse FFT, hand-worked fringes, the transpose identity with
tests/vis_ref.py and the conjugate pair; its derived bound against a float64 emulation of the
kernel's arithmetic (inside) and four planted mistakes (outside); the flag rule; the ABI the binding
declares, the workspace query and the tiling rule as host arithmetic; `engine.image_scales`; and the
Python paths of JetModel.dirty_image_* / dirty_beam with a recording engine."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import vis_adjoint_ref as A
from tests import vis_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


# ---- the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nz", [(8, 6), (5, 3), (16, 9)])
def test_reference_equals_ifft2_at_on_grid_points(nx, nz):
    """One visibility per FFT bin at a = kx / nx, b = kz / nz, each carrying the phase that moves
    the origin from pixel 0 to the grid centre: the sum is nx nz ifft2, and its real part."""
    rng = np.random.default_rng(nx * 100 + nz)
    Y = rng.normal(size=(nx, nz)) + 1j * rng.normal(size=(nx, nz))
    kx, kz = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    a, b = (kx / nx).ravel(), (kz / nz).ravel()
    shift = np.exp(2j * np.pi * (a * (nx - 1) / 2 + b * (nz - 1) / 2))
    ref = A.vis_adjoint_ref(Y.ravel() * shift, a, b, nx, nz).astype(np.float64)
    want = (np.fft.ifft2(Y) * nx * nz).real
    err = np.abs(ref - want).max() / np.abs(Y).sum()
    print("reference against ifft2: %.2e of sum |Y|" % err)
    assert err < 2e-14


def test_reference_hand_worked_fringes_and_the_conjugate_pair():
    nx, nz = 7, 10
    jx, jz = np.meshgrid(np.arange(nx) - 3.0, np.arange(nz) - 4.5, indexing="ij")
    # one visibility 2.5 e^{0.7 i} with weight 3 at (0.3, -0.2): a cosine fringe
    V, a, b, w = np.array([2.5 * np.exp(0.7j)]), np.array([0.3]), np.array([-0.2]), np.array([3.0])
    want = 7.5 * np.cos(2 * np.pi * (0.3 * jx - 0.2 * jz) + 0.7)
    assert np.abs(A.vis_adjoint_ref(V, a, b, nx, nz, w).astype(np.float64) - want).max() < 7.5e-14
    # two visibilities: the zero spacing (a constant) and a fringe along z alone
    V2, a2, b2 = np.array([4.0, 1.0j]), np.array([0.0, 0.0]), np.array([0.0, 0.125])
    want = 4.0 - np.sin(2 * np.pi * 0.125 * jz)
    assert np.abs(A.vis_adjoint_ref(V2, a2, b2, nx, nz).astype(np.float64) - want).max() < 1e-14
    # a visibility and its conjugate at (-u, -v) give twice one of them, to long-double rounding
    rng = np.random.default_rng(4)
    V, w = A.random_vis(rng, 9, flagged=0.0)
    a, b = R.random_points(rng, 9, 0.5)
    one = A.vis_adjoint_ref(V, a, b, nx, nz, w)
    both = A.vis_adjoint_ref(np.concatenate([V, np.conj(V)]), np.concatenate([a, -a]),
                             np.concatenate([b, -b]), nx, nz, np.concatenate([w, w]))
    assert np.abs((both - 2 * one).astype(np.float64)).max() <= 4e-19 * A.sum_abs(V, a, b, w) * 18
    # the centre pixel of an odd grid sees every phase 0: sum w Re V
    odd = A.vis_adjoint_ref(V, a, b, 7, 9, w)
    assert abs(float(odd[3, 4]) - float((w * V.real).sum())) <= 1e-15 * A.sum_abs(V, a, b, w)


@pytest.mark.parametrize("nx,nz,amax", [(5, 3, 0.5), (9, 14, 0.5), (9, 14, 8.0)])
def test_transpose_identity_with_the_k10_reference(nx, nz, amax):
    """<Y, A I>_w = <A^T (w Y), I>: sum_k w_k Re(conj(Y_k) vis_ref(I)_k) = sum_p I_p ref(Y)_p, to
    long-double rounding (both references sum a few hundred terms of relative error 2^-63)."""
    rng = np.random.default_rng(nx + 31 * nz)
    I = R.random_map(rng, nx, nz)
    I0 = np.where(np.isnan(I), 0.0, I).astype(LD)
    Y, w = A.random_vis(rng, 23, flagged=0.0)
    a, b = R.random_points(rng, 23, amax)
    Vm = R.vis_ref(I, a, b)
    lhs = (w.astype(LD) * (Y.real.astype(LD) * Vm.real + Y.imag.astype(LD) * Vm.imag)).sum()
    rhs = (I0 * A.vis_adjoint_ref(Y, a, b, nx, nz, w)).sum()
    scale = R.sum_abs(I) * A.sum_abs(Y, a, b, w)
    print("transpose identity: %.2e of sum |I| sum |w Y|" % (abs(float(lhs - rhs)) / scale))
    assert abs(float(lhs - rhs)) <= 1e-17 * scale


def test_flag_rule():
    rng = np.random.default_rng(11)
    nx, nz, K = 6, 5, 12
    V, w = A.random_vis(rng, K, flagged=0.0)
    a, b = R.random_points(rng, K, 0.5)
    full = A.vis_adjoint_ref(V, a, b, nx, nz, w)
    keep = np.ones(K, dtype=bool)
    keep[[2, 5, 7, 8, 10]] = False
    want = A.vis_adjoint_ref(V[keep], a[keep], b[keep], nx, nz, w[keep])
    V2, w2, a2, b2 = V.copy(), w.copy(), a.copy(), b.copy()
    V2[2] = complex(np.nan, 1.0)
    V2[5] = complex(1.0, -np.inf)
    w2[7], a2[8], b2[10] = np.inf, np.nan, -np.inf
    assert np.array_equal(A.unflagged(V2, a2, b2, w2), keep)
    got = A.vis_adjoint_ref(V2, a2, b2, nx, nz, w2)
    assert np.abs((got - want).astype(np.float64)).max() <= 4e-18 * A.sum_abs(V, a, b, w)
    assert np.abs((got - full).astype(np.float64)).max() > 1e-3
    assert abs(A.sum_abs(V2, a2, b2, w2) / A.sum_abs(V[keep], a[keep], b[keep], w[keep]) - 1) < 1e-15
    # every visibility flagged: exact zeros, from the reference and from the emulation
    allbad = np.full(K, np.nan)
    assert np.all(A.vis_adjoint_ref(V, allbad, b, nx, nz, w) == 0)
    assert np.all(A.vis_adjoint_emulated(V, a, b, nx, nz, allbad) == 0)
    # w = None means ones
    assert np.array_equal(A.vis_adjoint_ref(V, a, b, nx, nz), A.vis_adjoint_ref(V, a, b, nx, nz, np.ones(K)))


CASES = [(5, 3, 0.5, 12, None), (64, 64, 0.5, 40, 16), (67, 131, 0.5, 12, None),
         (67, 131, 8.0, 12, None)]


@pytest.mark.parametrize("nx,nz,amax,K,kper", CASES)
def test_emulation_inside_the_bound_and_planted_mistakes_outside(nx, nz, amax, K, kper):
    rng = np.random.default_rng(nx * 1000 + nz)
    V, w = A.random_vis(rng, K, flagged=0.0)
    a, b = R.random_points(rng, K, amax)
    a[1], b[1] = 0.37 * amax, -0.41 * amax
    V[1], w[1] = 3.0 - 2.0j, 1.7
    V[3], w[5] = complex(np.nan, 1.0), np.inf             # two flagged visibilities
    ns = 1 if kper is None else -(-K // kper)
    ref, S = A.vis_adjoint_ref(V, a, b, nx, nz, w), A.sum_abs(V, a, b, w)
    bnd = A.bound(V, a, b, nx, nz, w, k_splits=ns, k_per_split=kper)
    assert S > 0 and not A.unflagged(V, a, b, w).all() and bnd < 1e-12
    good = A.worst_ratio(A.vis_adjoint_emulated(V, a, b, nx, nz, w, k_per_split=kper), ref, S, bnd)
    print("%d x %d, |a| <= %g: emulation at %.4f of the bound %.2e" % (nx, nz, amax, good, bnd))
    assert good <= 1.0
    for what, kw in (("centre n / 2", dict(centre_shift=0.5)), ("opposite sign", dict(sign=-1.0)),
                     ("float32 phasor", dict(phasor_dtype=np.float32)),
                     ("a dropped weight", dict(drop_weight=True))):
        r = A.worst_ratio(A.vis_adjoint_emulated(V, a, b, nx, nz, w, k_per_split=kper, **kw), ref, S, bnd)
        assert r > 100.0, (what, r)


def test_bound_terms():
    """The four terms, by hand, at one point: 67 x 131, one visibility at |a| = |b| = 0.5."""
    u = 2.0 ** -53
    want = (2 * np.pi * (0.5 * 33 + 0.5 * 65) * u + 2 * (2.01e-14 + 6 * u) + 6 * u + (2 + 1 + 4) * u)
    got = A.bound([1.0 + 1.0j], [0.5], [-0.5], 67, 131)
    assert abs(got / want - 1) < 1e-12 and 0.7e-13 < got < 1.2e-13
    # term 1 is weighted by |w V|: a strong short baseline beside a weak long one
    two = A.bound([1.0, 1e-3], [0.0, 8.0], [0.0, 8.0], 67, 131)
    assert two < 0.01 * A.bound([1.0], [8.0], [8.0], 67, 131) + 2 * (2.01e-14 + 6 * u) + 30 * u
    # term 4: 2 FMAs per visibility of the longest split, and the combine
    d = A.bound(np.ones(1000), np.zeros(1000), np.zeros(1000), 5, 3, k_splits=16, k_per_split=64) \
        - A.bound(np.ones(1000), np.zeros(1000), np.zeros(1000), 5, 3, k_splits=1, k_per_split=16)
    assert abs(d / u - (2 * 48 + 15)) < 1e-3


# ---- the ABI ------------------------------------------------------------------------------------------
def test_header_version_symbols_and_argtypes():
    from rajepy_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    assert int(re.search(r"#define RJP_VERSION (\d+)", hdr).group(1)) == _lib.RJP_VERSION == 117
    assert "size_t rjp_vis_adjoint_workspace(int32_t n_maps, int32_t nx, int32_t nz, int32_t n_vis);" in hdr
    decl = re.search(r"int64_t rjp_vis_adjoint\((.*?)\);", hdr, re.S).group(1)
    names = [re.search(r"(\w+)$", p.strip()).group(1) for p in decl.split(",")]
    assert names == ["ctx", "d_vis", "n_maps", "n_vis", "h_su", "h_sv", "d_u", "d_v", "d_w", "nx",
                     "nz", "d_img", "d_work", "work_bytes", "stream"]
    doc = hdr[hdr.index("K11"):hdr.index("size_t rjp_vis_adjoint_workspace(")]
    for word in ("2^29", "transpose of rjp_vis", "classes.py:2770-2782", "non-finite", "2^-53"):
        assert word in doc, word
    res, args = _lib.SIGNATURES["rjp_vis_adjoint_workspace"]
    assert res is C.c_size_t and args == [C.c_int32] * 4
    res, args = _lib.SIGNATURES["rjp_vis_adjoint"]
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    assert res is C.c_int64
    assert args == [vp, vp, C.c_int32, C.c_int32, dp, dp, vp, vp, vp, C.c_int32, C.c_int32, vp, vp,
                    C.c_size_t, vp]
    lib = _lib.load()
    assert lib.rjp_version() == 117
    assert lib.rjp_vis_adjoint.argtypes == args and lib.rjp_vis_adjoint.restype is C.c_int64
    assert lib.rjp_vis_adjoint_workspace.restype is C.c_size_t
    # no new struct came with it
    assert set(re.findall(r"typedef struct (rjp_\w+) \{", hdr)) == {"rjp_fields", "rjp_bursts",
                                                                    "rjp_line", "rjp_geometry"}


def test_tiling_rule_by_hand():
    t = A.tiling
    assert t(1, 5, 3, 1) == dict(row_tiles=1, col_tiles=1, k_splits=1, k_per_split=16, workgroups=1)
    assert t(1, 5, 3, 64)["k_splits"] == 1 and t(1, 5, 3, 65) == dict(
        row_tiles=1, col_tiles=1, k_splits=2, k_per_split=48, workgroups=2)
    assert t(3, 130, 65, 257) == dict(row_tiles=2, col_tiles=1, k_splits=5, k_per_split=64, workgroups=30)
    assert t(2, 67, 131, 1000) == dict(row_tiles=1, col_tiles=2, k_splits=16, k_per_split=64, workgroups=64)
    assert t(1, 64, 64, 1000)["row_tiles"] == 1 and t(1, 65, 64, 10)["row_tiles"] == 1
    assert t(1, 129, 129, 10)["row_tiles"] == 2 and t(1, 129, 129, 10)["col_tiles"] == 2
    # the probe's points: the big one has tiles enough, the small one splits 8 ways
    assert t(64, 512, 512, 4096) == dict(row_tiles=4, col_tiles=4, k_splits=1, k_per_split=4096, workgroups=1024)
    assert t(8, 256, 256, 512) == dict(row_tiles=2, col_tiles=2, k_splits=8, k_per_split=64, workgroups=256)
    for args in ((1, 1, 1, 1), (2, 70, 300, 999), (5, 64, 128, 129), (255, 3, 3, 5000), (1, 3, 3, 100000)):
        r = t(*args)
        assert r["k_per_split"] % 16 == 0 and r["k_splits"] * r["k_per_split"] >= args[3]
        assert (r["k_splits"] - 1) * r["k_per_split"] < args[3], "no empty split"
        assert r["k_splits"] == 1 or r["k_per_split"] >= 48


def test_workspace_query():
    from rajepy_amd import _lib
    ws = _lib.load().rjp_vis_adjoint_workspace
    good = (3, 130, 65, 257)
    assert ws(*good) == A.workspace_bytes(*good) == 3 * 5 * 130 * 65 * 8
    for i in range(4):
        for bad in (0, -1):
            a = list(good)
            a[i] = bad
            assert ws(*a) == 0 == A.workspace_bytes(*a), a
    for args in ((1, 1, 1, 1), (1, 5, 3, 64), (1, 5, 3, 65), (2, 67, 131, 1000), (64, 512, 512, 4096),
                 (8, 256, 256, 512), (255, 64, 64, 129), (256, 64, 64, 129), (1, 1, 7, 5000)):
        assert ws(*args) == A.workspace_bytes(*args) > 0, args
    assert ws(64, 512, 512, 4096) == 16                  # the probe's big point needs no partials
    assert ws(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) in (0, 16)   # no overflow into a small size


# ---- the scales ---------------------------------------------------------------------------------------
def test_image_scales_against_vis_scales():
    from rajepy_amd import engine as E
    freqs = np.array([5e9, 4.3e10])
    cell = np.arctan((0.5 * E.con.au) / (120. * E.con.parsec))
    su, sv = E.image_scales(freqs, cell)
    vu, vv = E.vis_scales(freqs, 0.5, 120.)
    assert np.array_equal(su, vu) and np.array_equal(sv, vv)
    # a quarter of that cell: a quarter of the cycles per cell; a scalar frequency gives length 1
    qu, qv = E.image_scales(freqs, cell / 4)
    assert np.allclose(qu, vu / 4, rtol=1e-15) and np.allclose(qv, vv / 4, rtol=1e-15)
    assert E.image_scales(5e9, cell)[0].shape == (1,) and np.all(su < 0) and np.all(sv > 0)
    # 1 arcsecond cells at 5 GHz, 1 km: 16678.205 wavelengths x 4.848137e-6 rad
    assert abs(E.image_scales(5e9, np.radians(1 / 3600.))[1][0] * 1000. - 16678.205 * 4.848137e-6) < 1e-8


# ---- the Python paths -------------------------------------------------------------------------------
class _DeviceMaps:
    """Stands for a stack of maps on the device: it can be reshaped and nothing else."""

    def __init__(self, n_maps, npix):
        self.n_maps, self.npix = n_maps, npix

    def reshape(self, *shape):
        assert shape[0] == self.n_maps and shape[1] in (-1, self.npix), shape
        return self

    def cpu(self):
        raise AssertionError("maps must not be copied to the host")

    numpy = tolist = __array__ = cpu


class _DeviceVis(torch.Tensor):
    """A tensor that stands for visibilities on the device: any route to the host fails."""

    @staticmethod
    def wrap(t):
        return t.as_subclass(_DeviceVis)

    def cpu(self, *a, **k):
        raise AssertionError("visibilities must not be copied to the host")

    numpy = tolist = __array__ = cpu


class _RecordingEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def _device_f64(self, values):
        if isinstance(values, torch.Tensor):
            return values
        return torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64).reshape(-1))

    def vis(self, maps, nx, nz, su, sv, u, v):
        assert isinstance(maps, _DeviceMaps) and isinstance(u, torch.Tensor)
        self.calls.append(dict(kind="vis", nx=nx, nz=nz, su=np.array(su), sv=np.array(sv), u=u, v=v))
        M, K = maps.n_maps, u.numel()
        return _DeviceVis.wrap(torch.complex(torch.arange(M * K, dtype=torch.float64).reshape(M, K),
                                             torch.ones(M, K, dtype=torch.float64)))

    def vis_adjoint(self, vis, nx, nz, su, sv, u, v, w=None):
        assert isinstance(vis, torch.Tensor) and vis.dtype == torch.complex128 and vis.is_contiguous()
        M, K = vis.shape
        assert len(su) == len(sv) == M and u.numel() == v.numel() == K
        self.calls.append(dict(kind="adjoint",
                               vis=torch.view_as_real(vis).as_subclass(torch.Tensor).clone(),
                               nx=nx, nz=nz, su=np.array(su), sv=np.array(sv), u=u.clone(),
                               v=v.clone(), w=None if w is None else w.clone(),
                               device_vis=isinstance(vis, _DeviceVis)))
        n = len([c for c in self.calls if c["kind"] == "adjoint"])
        # image m of call n is the constant 100 n + m
        return (100.0 * n + torch.arange(M, dtype=torch.float64))[:, None].expand(M, nx * nz).clone()


def _model(nx, nz):
    from rajepy_amd import classes

    class Model(classes.JetModel):
        """A JetModel that holds only what its imaging front reads: the engine, the grid and the
        distance; the `imaging.Imager` it hands over to is the real one."""

        def __init__(self):
            self._engine, self._nx, self._nz, self._csize = _RecordingEngine(), nx, nz, 0.5
            self._params = {"target": {"dist": 120.}}

    m = Model()
    m.asked = []

    def ff(freqs, flux=False, device=False, formal=False):
        assert flux and device
        m.asked.append(("ff", formal))
        return _DeviceMaps(len(freqs), nx * nz)

    def rrl(line, freqs, lte, contsub, formal=False, device=False):
        assert device and lte
        m.asked.append(("rrl", line, contsub, formal))
        return _DeviceMaps(len(freqs), nx * nz)
    m._ff_products, m._rrl_flux = ff, rrl
    return m


U_M, V_M = np.array([0., 100., -3e3, 2e4]), np.array([0., -50., 1e3, 1e4])
FREQS = np.array([5e9, 2e10, 4e10])


def test_dirty_image_is_vis_then_one_adjoint_per_chunk_normalised_by_the_weights():
    from rajepy_amd import engine as E
    m = _model(6, 4)
    w = np.array([1.0, 2.0, 0.5, 4.0])
    out = m.dirty_image_ff(U_M, V_M, FREQS, weights=w, formal=True)
    assert out.shape == (3, 6, 4) and out.dtype == np.float64 and m.asked == [("ff", True)]
    kinds = [c["kind"] for c in m.engine.calls]
    assert kinds == ["vis", "adjoint"]
    vis, adj = m.engine.calls
    su, sv = E.vis_scales(FREQS, 0.5, 120.)
    assert np.array_equal(vis["su"], su) and np.array_equal(adj["su"], su) and np.array_equal(adj["sv"], sv)
    assert (adj["nx"], adj["nz"]) == (6, 4) and adj["device_vis"], "the visibilities stay on the device"
    assert adj["u"].tolist() == list(U_M) and adj["v"].tolist() == list(V_M) and adj["w"].tolist() == list(w)
    assert torch.equal(adj["vis"][..., 0], torch.arange(12, dtype=torch.float64).reshape(3, 4))
    for f in range(3):
        assert np.all(out[f] == (100.0 + f) / 7.5)        # / sum w
    # chunks: 2 images of 48 x 32 x 8 bytes fit, the third goes into a second call
    m2 = _model(6, 4)
    m2.VIS_STACK_BYTES = 2 * 48 * 32 * 8
    out = m2.dirty_image_ff(U_M, V_M, FREQS, shape=(48, 32), cell_as=0.001)
    adj = [c for c in m2.engine.calls if c["kind"] == "adjoint"]
    assert [c["vis"].shape[0] for c in adj] == [2, 1] and out.shape == (3, 48, 32)
    iu, iv = E.image_scales(FREQS, np.radians(0.001 / 3600.))
    assert np.array_equal(adj[0]["su"], iu[:2]) and np.array_equal(adj[1]["sv"], iv[2:])
    assert adj[0]["w"] is None and (adj[0]["nx"], adj[0]["nz"]) == (48, 32)
    assert np.all(out[0] == 100.0 / 4) and np.all(out[1] == 101.0 / 4) and np.all(out[2] == 200.0 / 4)
    assert torch.equal(adj[1]["vis"][..., 0], torch.arange(8, 12, dtype=torch.float64).reshape(1, 4))
    # the model's own grid is the vis call's, whatever the image's
    assert (m2.engine.calls[0]["nx"], m2.engine.calls[0]["nz"]) == (6, 4)
    # a flagged baseline leaves the normalisation
    m3 = _model(6, 4)
    ub = U_M.copy()
    ub[2] = np.nan
    out = m3.dirty_image_ff(ub, V_M, FREQS[:1], weights=w)
    assert np.all(out[0] == 100.0 / 7.0)
    with pytest.raises(ValueError):
        m3.dirty_image_ff(U_M, V_M, FREQS, weights=w[:3])
    with pytest.raises(ValueError):
        m3.dirty_image_ff(U_M, V_M, FREQS, shape=(0, 4))
    with pytest.raises(ValueError):
        m3.dirty_image_ff(U_M, V_M, FREQS, cell_as=-1.0)


def test_mfs_is_one_visibility_set_in_cycles_per_cell():
    from rajepy_amd import engine as E
    m = _model(6, 4)
    w = np.array([1.0, 2.0, 0.5, 4.0])
    out = m.dirty_image_ff(U_M, V_M, FREQS, weights=w, shape=(9, 7), mfs=True)
    assert out.shape == (1, 9, 7)
    adj = [c for c in m.engine.calls if c["kind"] == "adjoint"]
    assert len(adj) == 1 and adj[0]["device_vis"]
    c = adj[0]
    su, sv = E.vis_scales(FREQS, 0.5, 120.)
    assert c["vis"].shape == (1, 12, 2) and list(c["su"]) == [1.0] and list(c["sv"]) == [1.0]
    assert np.array_equal(c["u"].numpy().reshape(3, 4), su[:, None] * U_M[None, :])
    assert np.array_equal(c["v"].numpy().reshape(3, 4), sv[:, None] * V_M[None, :])
    assert np.array_equal(c["w"].numpy(), np.tile(w, 3))
    assert torch.equal(c["vis"][0, :, 0], torch.arange(12, dtype=torch.float64))
    assert np.all(out == 100.0 / (3 * 7.5))
    # without weights: / (F K)
    m2 = _model(6, 4)
    assert np.all(m2.dirty_image_ff(U_M, V_M, FREQS, mfs=True) == 100.0 / 12)
    assert m2.engine.calls[-1]["w"] is None


def test_dirty_beam_and_rrl_paths():
    m = _model(6, 4)
    out = m.dirty_beam(U_M, V_M, FREQS[:2], shape=(5, 5))
    assert out.shape == (2, 5, 5) and m.asked == []
    assert [c["kind"] for c in m.engine.calls] == ["adjoint"]
    c = m.engine.calls[0]
    assert bool((c["vis"][..., 0] == 1).all()) and bool((c["vis"][..., 1] == 0).all())
    assert c["vis"].shape == (2, 4, 2) and np.all(out[1] == 101.0 / 4)
    assert m.dirty_beam(U_M, V_M, FREQS, mfs=True).shape == (1, 6, 4)
    out = m.dirty_image_rrl("H66a", U_M, V_M, FREQS, contsub=False, formal=True)
    assert out.shape == (3, 6, 4) and m.asked == [("rrl", "H66a", False, True)]
    assert [c["kind"] for c in m.engine.calls[-2:]] == ["vis", "adjoint"]


def test_public_surface():
    from rajepy_amd import classes, engine as E
    J = classes.JetModel
    assert list(inspect.signature(E.RTEngine.vis_adjoint).parameters) == \
        ["self", "vis", "nx", "nz", "su", "sv", "u", "v", "w"]
    assert inspect.signature(E.RTEngine.vis_adjoint).parameters["w"].default is None
    assert list(inspect.signature(E.image_scales).parameters) == ["freqs", "cell_rad"]
    p = inspect.signature(J.dirty_image_ff).parameters
    assert list(p) == ["self", "u_m", "v_m", "freq", "weights", "shape", "cell_as", "formal", "mfs"]
    assert [p[k].default for k in list(p)[4:]] == [None, None, None, False, False]
    p = inspect.signature(J.dirty_image_rrl).parameters
    assert list(p)[:5] == ["self", "rrl", "u_m", "v_m", "freq"] and p["mfs"].default is False
    assert list(inspect.signature(J.dirty_beam).parameters)[:4] == ["self", "u_m", "v_m", "freq"]
