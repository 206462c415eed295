"""rjp_vis (K10) without a GPU: the long-double reference the GPU tests hold the kernel to
(tests/vis_ref.py) against the FFT, analytic transforms and symmetries; its derived bound against a
float64 emulation (inside) and three planted mistakes (outside); the sky convention of
`engine.vis_scales`; the ABI the binding declares and the workspace query; and the Python paths of
JetModel.visibilities_* with a recording engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import vis_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YEAR = 31557600.0


# ---- the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("nx,nz", [(8, 6), (5, 3), (16, 9)])
def test_reference_equals_fft2_at_on_grid_points(nx, nz):
    """a = kx / nx, b = kz / nz: the sum is fft2's bin times the phase that moves the origin from
    pixel 0 to the map centre."""
    rng = np.random.default_rng(nx * 100 + nz)
    I = rng.normal(size=(nx, nz))
    F = np.fft.fft2(I)
    kx, kz = np.meshgrid(np.arange(nx), np.arange(nz), indexing="ij")
    a, b = (kx / nx).ravel(), (kz / nz).ravel()
    ref = R.vis_ref(I, a, b).astype(np.complex128)
    shift = np.exp(2j * np.pi * (a * (nx - 1) / 2 + b * (nz - 1) / 2))
    err = np.abs(ref - F.ravel() * shift).max() / np.abs(I).sum()
    print("reference against fft2: %.2e of sum |I|" % err)
    assert err < 2e-14


def test_reference_single_pixel_fringe_zero_spacing_and_hermitian_symmetry():
    nx, nz = 7, 10
    a = np.array([0.0, 0.3, -0.41, 0.07, 3.2])
    b = np.array([0.0, -0.2, 0.13, 0.45, -5.7])
    # one pixel of flux 2.5 at (5, 2): a pure phasor at its offset from the centre
    I = np.full((nx, nz), np.nan)
    I[5, 2] = 2.5
    want = 2.5 * np.exp(-2j * np.pi * (a * (5 - 3.0) + b * (2 - 4.5)))
    assert np.abs(R.vis_ref(I, a, b).astype(np.complex128) - want).max() < 1e-15 * 2.5 * 40
    # two equal pixels 4 cells apart in z: a fringe 2 cos(pi b 4) about their midpoint
    I[:] = 0.0
    I[3, 1] = I[3, 5] = 1.0
    want = 2.0 * np.cos(2 * np.pi * b * 2.0) * np.exp(-2j * np.pi * b * (3.0 - 4.5))
    assert np.abs(R.vis_ref(I, a, b).astype(np.complex128) - want).max() < 1e-14
    # V(0, 0) = nansum; V(-u, -v) = conj V(u, v) for a real map
    rng = np.random.default_rng(5)
    I = R.random_map(rng, 9, 14)
    ref = R.vis_ref(I, a, b)
    assert abs(complex(ref[0]) - np.nansum(I)) <= 1e-15 * R.sum_abs(I)
    neg = R.vis_ref(I, -a, -b)
    assert np.array_equal(neg.real, ref.real) and np.array_equal(neg.imag, -ref.imag)
    # a map that is NaN everywhere transforms to exact zeros; a non-finite point to NaN, alone
    assert np.all(R.vis_ref(np.full((4, 3), np.nan), a, b) == 0)
    a2 = a.copy()
    a2[2] = np.inf
    bad = R.vis_ref(I, a2, b)
    assert np.isnan(complex(bad[2])) and np.array_equal(np.delete(bad, 2), np.delete(ref, 2))


CASES = [(5, 3, 0.5), (64, 64, 0.5), (67, 131, 0.5), (67, 131, 8.0)]


@pytest.mark.parametrize("nx,nz,amax", CASES)
def test_emulation_inside_the_bound_and_planted_mistakes_outside(nx, nz, amax):
    rng = np.random.default_rng(nx * 1000 + nz)
    I = R.random_map(rng, nx, nz)
    a, b = R.random_points(rng, 12, amax)
    ref, S, bnd = R.vis_ref(I, a, b), R.sum_abs(I), R.bound(a, b, nx, nz)
    assert S > 0 and np.isnan(I).any() and bnd.max() < 1e-12
    good = R.worst_ratio(R.vis_emulated(I, a, b), ref, S, bnd)
    print("%d x %d, |a| <= %g: emulation at %.4f of the bound (%.2e .. %.2e)"
          % (nx, nz, amax, good, bnd.min(), bnd.max()))
    assert good <= 1.0
    for what, kw in (("centre n / 2", dict(centre_shift=0.5)), ("opposite sign", dict(sign=1.0)),
                     ("float32 phasor", dict(phasor_dtype=np.float32))):
        r = R.worst_ratio(R.vis_emulated(I, a, b, **kw), ref, S, bnd)
        assert r > 100.0, (what, r)


def test_bound_terms():
    """The four terms, by hand, at one point: 67 x 131, |a| = |b| = 0.5."""
    u = 2.0 ** -53
    want = 2 * np.pi * (0.5 * 33 + 0.5 * 65) * u + 2 * (2.01e-14 + 6 * u) + (67 + 131 + 24) * u
    got = float(R.bound([0.5], [-0.5], 67, 131)[0])
    assert abs(got / want - 1) < 1e-12 and 0.8e-13 < got < 1.4e-13
    assert float(R.bound([8.0], [8.0], 67, 131)[0]) < 7e-13


# ---- the convention ---------------------------------------------------------------------------------
class _FitsModel:
    nx, nz, csize = 6, 4, 0.5
    params = {"target": {"name": "t", "ra": "04:31:34.1", "dec": "+18:08:04.9", "dist": 120.}}

    def __str__(self):
        return "model"


def test_vis_scales_hand_worked_and_the_sign_of_su_against_cdelt1(tmp_path):
    from rajepy_amd import classes, engine as E
    freqs = np.array([5e9, 4.3e10])
    su, sv = E.vis_scales(freqs, 0.5, 120.)
    # 0.5 au at 120 pc subtends 0.5 / 120 arcsec; 206264.806247 arcsec per radian
    cell = (0.5 / 120.) / 206264.806247
    assert abs(cell ** 2 / E.solid_angle(0.5, 120.) - 1) < 1e-9
    for f, a, b in zip(freqs, su, sv):
        assert abs(b / (cell * f / 299792458.0) - 1) < 1e-9 and a == -b
    assert su.shape == sv.shape == (2,) and E.vis_scales(5e9, 0.5, 120.)[0].shape == (1,)
    # 1 km east-west baseline at 5 GHz: 16678 wavelengths, 3.4e-4 cycles per 4.17 mas cell
    assert abs(sv[0] * 1000. - 3.36909e-4) < 1e-9
    # the header save_fits writes: RA decreases with ix (CDELT1 < 0: su < 0), Dec increases with iz
    path = str(tmp_path / "m.fits")
    classes.JetModel.save_fits(_FitsModel(), np.zeros((4, 6)), path, "flux", freq=5e9)
    raw = open(path, "rb").read(2880 * 4).decode("ascii", "replace")
    cards = {raw[i:i + 8].strip(): raw[i + 10:i + 80] for i in range(0, len(raw), 80)}
    cd1, cd2 = float(cards["CDELT1"].split("/")[0]), float(cards["CDELT2"].split("/")[0])
    assert cd1 < 0 < cd2 and np.sign(su[0]) == np.sign(cd1) and np.sign(sv[0]) == np.sign(cd2)
    assert abs(np.radians(cd2) / cell - 1) < 1e-9
    # the phase centre is CRPIX (1-based): pixel (nx - 1) / 2, (nz - 1) / 2 counted from 0
    assert float(cards["CRPIX1"].split("/")[0]) - 1 == (6 - 1) / 2
    assert float(cards["CRPIX2"].split("/")[0]) - 1 == (4 - 1) / 2


# ---- the ABI ------------------------------------------------------------------------------------------
def test_header_version_symbols_and_argtypes():
    from rajepy_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    assert int(re.search(r"#define RJP_VERSION (\d+)", hdr).group(1)) == _lib.RJP_VERSION == 117
    assert "size_t rjp_vis_workspace(" in hdr and "int rjp_vis(" in hdr
    assert "2^29" in hdr[hdr.index("K10"):hdr.index("size_t rjp_vis_workspace(")]   # the phase's range
    res, args = _lib.SIGNATURES["rjp_vis_workspace"]
    assert res is C.c_size_t and args == [C.c_int32] * 4
    res, args = _lib.SIGNATURES["rjp_vis"]
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    assert res is C.c_int
    assert args == [vp, vp, C.c_int32, C.c_int32, C.c_int32, dp, dp, vp, vp, C.c_int32, vp, vp,
                    C.c_size_t, vp]
    lib = _lib.load()
    assert lib.rjp_version() == 117
    assert lib.rjp_vis.argtypes == args and lib.rjp_vis_workspace.restype is C.c_size_t


def test_workspace_query():
    from rajepy_amd import _lib
    ws = _lib.load().rjp_vis_workspace
    good = (3, 130, 65, 257)
    assert ws(*good) > 0
    for i in range(4):
        for bad in (0, -1):
            a = list(good)
            a[i] = bad
            assert ws(*a) == 0, a
    # one complex partial per (map, visibility) at the least
    assert ws(*good) >= 3 * 257 * 16
    for i, values in enumerate(((1, 2, 3, 64, 1000), (1, 63, 64, 65, 128, 129, 512, 513, 5000),
                                (1, 15, 16, 17, 1000), (1, 63, 64, 65, 257, 4096))):
        last = 0
        for v in values:
            a = list(good)
            a[i] = v
            assert ws(*a) >= last, (i, v)
            last = ws(*a)
    assert ws(64, 512, 512, 4096) <= 64 << 20          # the probe's case: megabytes, not the 2 GB of phasors


# ---- the Python paths -------------------------------------------------------------------------------
class _DeviceMaps:
    """Stands for a stack of maps on the device: it can be reshaped and nothing else -- any route
    to the host fails."""

    def __init__(self, n_maps, npix, tag):
        self.n_maps, self.npix, self.tag = n_maps, npix, tag

    def reshape(self, *shape):
        assert shape[0] == self.n_maps and shape[1] in (-1, self.npix), shape
        return self

    def numel(self):
        return self.n_maps * self.npix

    def cpu(self):
        raise AssertionError("maps must not be copied to the host")

    numpy = tolist = __array__ = cpu


class _RecordingEngine:
    def __init__(self):
        self.calls = []

    def _device_f64(self, values):
        if isinstance(values, torch.Tensor):
            return values
        return torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64).reshape(-1))

    def vis(self, maps, nx, nz, su, sv, u, v):
        assert isinstance(maps, _DeviceMaps) and isinstance(u, torch.Tensor)
        self.calls.append(dict(kind="vis", maps=maps, nx=nx, nz=nz, su=np.array(su),
                               sv=np.array(sv), u=u, v=v))
        M, K = maps.n_maps, u.numel()
        base = 1000.0 * len([c for c in self.calls if c["kind"] == "vis"])
        return torch.complex(base + torch.arange(M * K, dtype=torch.float64).reshape(M, K),
                             torch.ones(M, K, dtype=torch.float64))

    def ff_formal_sweep(self, fields, bursts, epochs_s, gff_mode, ctau, csrc, want_maps=False,
                        want_totals=True):
        assert want_maps and not want_totals
        self.calls.append(dict(kind="sweep", epochs=list(epochs_s)))
        return _DeviceMaps(len(epochs_s) * len(ctau), fields.npix, "sweep"), None

    def ff_maps(self, sumA, tavg, ctau, cflux, want_tau=True, want_flux=True, want_ftot=True):
        assert want_flux and not want_tau and not want_ftot
        self.calls.append(dict(kind="maps", epochs=sumA.shape[0]))
        return None, _DeviceMaps(sumA.shape[0] * len(ctau), sumA.shape[1], "maps"), None

    def ff_formal_grad(self, fields, bursts, epochs_s, gff_mode, ctau, csrc, want_maps=False):
        assert want_maps
        self.calls.append(dict(kind="grad", epochs=list(epochs_s)))
        n_par = 3 * (bursts.n[0] + bursts.n[1])
        return None, None, _DeviceMaps(len(epochs_s) * len(ctau) * n_par, fields.npix, "grad")


class _Fields:
    def __init__(self, npix):
        self.npix = npix


class _Bursts:
    n = (1, 2)


def _model(nx, nz, slots=True):
    from rajepy_amd import _lib, classes, engine as E
    J = classes.JetModel

    class Model:
        SCAN_CACHE_EPOCHS = J.SCAN_CACHE_EPOCHS
        VIS_STACK_BYTES = J.VIS_STACK_BYTES
        _vis_scales, _vis_chunk = J._vis_scales, J._vis_chunk
        visibilities_vs_time, visibilities_vs_time_jac = (J.visibilities_vs_time,
                                                          J.visibilities_vs_time_jac)
        _channel_coeffs = J._channel_coeffs

    m = Model()
    m.engine, m.nx, m.nz, m.csize = _RecordingEngine(), nx, nz, 0.5
    m.params = {"target": {"dist": 120.}, "properties": {"T_0": 1e4}}
    m.gff_mode, m._dtype = E.RJP_GFF_POWERLAW, _lib.RJP_F64
    m.device_fields, m._scan_cache, m.prefetched = _Fields(nx * nz), {}, []
    m._rjp_bursts = lambda: _Bursts()
    m._model_tavg = lambda: torch.zeros(nx * nz, dtype=torch.float64)
    # three bursts (one red, two blue) registered as ejections 0 -> blue 1, 1 -> red 0, 2 -> blue 0
    m._ejection_slots = lambda: ([(6, (1., 2., 3.)), (0, (10., 20., 30.)), (3, (.5, .25, .125))]
                                 if slots else [])

    def prefetch(times_s, want_em=True):
        assert want_em is False
        m.prefetched.append(list(times_s))
        for t in times_s:
            m._scan_cache[float(t)] = (torch.full((1, nx * nz), float(t), dtype=torch.float64), None)
    m.prefetch_epochs = prefetch
    return m


@pytest.mark.parametrize("formal", [True, False])
def test_visibilities_vs_time_is_one_vis_call_per_chunk_under_a_gib(formal):
    from rajepy_amd import engine as E
    nx = nz = 2048                                      # 32 MiB per map: 3 channels -> 10 epochs per GiB
    m = _model(nx, nz)
    times = np.arange(23, dtype=np.float64) * 0.1 * YEAR
    freqs = np.array([5e9, 2e10, 4e10])
    u, v = np.array([0., 100., -3e3, 2e4]), np.array([0., -50., 1e3, 1e4])
    out = m.visibilities_vs_time(times, u, v, freqs, formal=formal)
    assert out.shape == (23, 3, 4) and out.dtype == np.complex128
    calls = m.engine.calls
    vis = [c for c in calls if c["kind"] == "vis"]
    makers = [c for c in calls if c["kind"] == ("sweep" if formal else "maps")]
    assert len(vis) == len(makers) == 3 and len(calls) == 6
    sizes = [c["maps"].n_maps // 3 for c in vis]
    assert sizes == [10, 10, 3]
    su, sv = E.vis_scales(freqs, 0.5, 120.)
    for c, n in zip(vis, sizes):
        assert c["maps"].numel() * 8 <= 1 << 30 < 11 * 3 * nx * nz * 8
        assert c["maps"].tag == ("sweep" if formal else "maps")
        assert (c["nx"], c["nz"]) == (nx, nz)
        assert np.array_equal(c["su"], np.tile(su, n)) and np.array_equal(c["sv"], np.tile(sv, n))
        assert c["u"].tolist() == list(u) and c["v"].tolist() == list(v)
    if formal:
        assert [c["epochs"] for c in makers] == [list(times[:10]), list(times[10:20]), list(times[20:])]
        assert m.prefetched == []
    else:
        assert m.prefetched == [list(times[:10]), list(times[10:20]), list(times[20:])]
    # the values land where their epoch and channel belong
    assert out[0, 0, 0] == 1000. + 1j and out[9, 2, 3] == 1000. + 119. + 1j
    assert out[10, 0, 0] == 2000. + 1j and out[22, 2, 3] == 3000. + 35. + 1j
    # no epochs: no call
    m2 = _model(4, 4)
    assert m2.visibilities_vs_time([], u, v, freqs, formal=formal).shape == (0, 3, 4)
    assert m2.engine.calls == []


def test_isothermal_sweep_never_asks_one_prefetch_for_more_than_it_keeps():
    m = _model(4, 4)
    times = np.arange(150, dtype=np.float64)
    m.visibilities_vs_time(times, [0.], [0.], 5e9)
    assert [len(p) for p in m.prefetched] == [64, 64, 22]


def test_visibilities_vs_time_jac_chain_rule_and_chunks():
    nx = nz = 1024                                      # 8 MiB per map, 2 channels x 9 parameters: 7 epochs
    m = _model(nx, nz)
    times = np.arange(9, dtype=np.float64) * YEAR
    freqs = np.array([5e9, 4e10])
    u, v = np.array([0., 250.]), np.array([0., -80.])
    V, dV = m.visibilities_vs_time_jac(times, u, v, freqs)
    assert V.shape == (9, 2, 2) and dV.shape == (9, 2, 3, 3, 2)
    calls = m.engine.calls
    kinds = [c["kind"] for c in calls]
    # V through visibilities_vs_time(formal=True) (one chunk), then one grad + one vis per chunk
    assert kinds == ["sweep", "vis", "grad", "vis", "grad", "vis"]
    assert calls[0]["epochs"] == list(times)
    assert calls[2]["epochs"] == list(times[:7]) and calls[4]["epochs"] == list(times[7:])
    from rajepy_amd import engine as E
    su, sv = E.vis_scales(freqs, 0.5, 120.)
    for c, n in ((calls[3], 7), (calls[5], 2)):
        assert c["maps"].tag == "grad" and c["maps"].n_maps == n * 2 * 9
        assert c["maps"].numel() * 8 <= 1 << 30
        assert np.array_equal(c["su"], np.tile(np.repeat(su, 9), n))
        assert np.array_equal(c["sv"], np.tile(np.repeat(sv, 9), n))
    # dV[e, f, i, c, k] = raw[e, f, slot_i + c, k] * chain_i[c]; raw = base + flat index + 1j
    raw = lambda base, e, f, p, k: complex(base + ((e * 2 + f) * 9 + p) * 2 + k, 1.0)
    assert dV[0, 0, 0, 0, 0] == raw(2000., 0, 0, 6, 0) * 1.
    assert dV[3, 1, 1, 2, 1] == raw(2000., 3, 1, 0 + 2, 1) * 30.
    assert dV[6, 1, 2, 1, 0] == raw(2000., 6, 1, 3 + 1, 0) * .25
    assert dV[8, 0, 0, 2, 1] == raw(3000., 1, 0, 6 + 2, 1) * 3.
    assert V[0, 0, 0] == 1000. + 1j
    # no ejections: n_ej = 0, V alone; f32 storage refuses
    m0 = _model(8, 8, slots=False)
    V0, dV0 = m0.visibilities_vs_time_jac(times, u, v, freqs)
    assert V0.shape == (9, 2, 2) and dV0.shape == (9, 2, 0, 3, 2)
    assert [c["kind"] for c in m0.engine.calls] == ["sweep", "vis"]
    from rajepy_amd import _lib
    m0._dtype = _lib.RJP_F32
    with pytest.raises(ValueError, match="f64 storage"):
        m0.visibilities_vs_time_jac(times, u, v, freqs)


def test_public_surface():
    import inspect
    from rajepy_amd import classes, engine as E
    J = classes.JetModel
    assert list(inspect.signature(E.RTEngine.vis).parameters) == \
        ["self", "maps", "nx", "nz", "su", "sv", "u", "v"]
    assert inspect.signature(J.visibilities_ff).parameters["formal"].default is False
    p = inspect.signature(J.visibilities_rrl).parameters
    assert p["contsub"].default is True and p["formal"].default is False
    assert list(p)[:5] == ["self", "rrl", "u_m", "v_m", "freq"]
    assert inspect.signature(J.visibilities_vs_time).parameters["formal"].default is False
    assert list(inspect.signature(J.visibilities_vs_time_jac).parameters) == \
        ["self", "times_s", "u_m", "v_m", "freq"]
