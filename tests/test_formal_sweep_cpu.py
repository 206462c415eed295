"""rjp_ff_formal_sweep (K8) without a GPU: the ABI the binding declares, the workspace query, the
light-curve reference the GPU tests hold the kernel to (NumPy's formal solution summed per epoch,
pinned on the isothermal golden model against the oracle's flux maps), and the Python path of
`sweep_flux_vs_time(formal=True)` with a recording engine."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from oracle import rt_oracle as orc
from tests import gpu_util as U
from tests.test_gpu_formal_rt import _coeffs, np_formal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_version_symbols_and_argtypes():
    from rajepy_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    assert int(re.search(r"#define RJP_VERSION (\d+)", hdr).group(1)) == _lib.RJP_VERSION == 117
    assert "size_t rjp_ff_formal_sweep_workspace(" in hdr and "int rjp_ff_formal_sweep(" in hdr
    res, args = _lib.SIGNATURES["rjp_ff_formal_sweep_workspace"]
    assert res is C.c_size_t and args == [C.c_int32] * 5
    res, args = _lib.SIGNATURES["rjp_ff_formal_sweep"]
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    assert res is C.c_int
    assert args == [vp, C.POINTER(_lib.Fields), C.POINTER(_lib.Bursts), dp, C.c_int32, C.c_int32,
                    dp, dp, C.c_int32, vp, vp, vp, C.c_size_t, vp]
    lib = _lib.load()
    assert lib.rjp_version() == 117
    assert lib.rjp_ff_formal_sweep.argtypes == args
    assert lib.rjp_ff_formal_sweep_workspace.restype is C.c_size_t


def test_workspace_query():
    from rajepy_amd import _lib
    ws = _lib.load().rjp_ff_formal_sweep_workspace
    good = (4, 100, 37, 32, 3)
    assert ws(*good) > 0
    for i in range(5):
        for bad in (0, -1):
            a = list(good)
            a[i] = bad
            assert ws(*a) == 0, a
    # one partial per (epoch, channel, 16 sightlines of an x-row) at the least
    assert ws(*good) >= 4 * 3 * 32 * 3 * 8
    last = 0
    for E in (1, 2, 15, 16, 17, 63, 64, 65, 130, 1000):
        assert ws(4, 100, 37, E, 3) >= last
        last = ws(4, 100, 37, E, 3)
    last = 0
    for F in (1, 2, 3, 4, 5, 8, 9, 300):
        assert ws(4, 100, 37, 32, F) >= last
        last = ws(4, 100, 37, 32, F)
    assert ws(512, 4096, 512, 121, 8) >= 512 * 32 * 121 * 8 * 8


def test_numpy_light_curve_reference_on_the_isothermal_golden_model():
    """cfg1_example (q_T = q^d_T = 0): NumPy's formal solution on the oracle's per-cell optical
    depths, summed over the pixels, equals the nansum of the oracle's isothermal flux_ff at every
    golden epoch and frequency to 1e-12 -- the sum telescopes."""
    z, meta, p, g, jet = U.golden_dense("cfg1_example")
    freqs = np.asarray(z["freqs"], dtype=np.float64)
    mode, ctau, cflux = _coeffs(jet, freqs)
    for yr in z["years"]:
        jet.time = float(yr) * orc.YEAR
        with np.errstate(all="ignore"):
            ref = np_formal(jet.optical_depth_ff(freqs, collapse=False), jet.temperature, cflux)
            iso = jet.flux_ff(freqs)
        assert np.array_equal(np.isnan(ref), np.isnan(iso))
        lc, want = np.nansum(ref, axis=(1, 2)), np.nansum(iso, axis=(1, 2))
        assert (want > 0).all()
        np.testing.assert_allclose(lc, want, rtol=1e-12, atol=0)


class _RecordingEngine:
    def __init__(self):
        self.calls = []

    def _f64(self, *shape):
        return torch.empty(*shape, dtype=torch.float64)

    def ff_formal_sweep(self, fields, bursts, epochs_s, gff_mode, ctau, csrc, want_maps=False,
                        want_totals=True):
        self.calls.append(dict(fields=fields, bursts=bursts, epochs=list(epochs_s), mode=gff_mode,
                               ctau=np.array(ctau), csrc=np.array(csrc), want_maps=want_maps,
                               want_totals=want_totals))
        E, F = len(epochs_s), len(ctau)
        return None, torch.arange(E * F, dtype=torch.float64).reshape(E, F)

    def ff_step(self, *a, **k):
        raise AssertionError("formal=True must not take the isothermal step")


class _Model:
    def __init__(self):
        from rajepy_amd import engine as E
        self.engine = _RecordingEngine()
        self.device_fields = object()
        self.gff_mode = E.RJP_GFF_POWERLAW
        self.csize = 0.5
        self.params = {"target": {"dist": 120.}, "properties": {"T_0": 1e4}}
        self.the_bursts = object()

    def _rjp_bursts(self):
        return self.the_bursts

    def _model_tavg(self):
        raise AssertionError("the formal sweep reads no T_avg map")


def test_sweep_flux_vs_time_formal_is_one_call_without_maps():
    from rajepy_amd import classes, engine as E, parallel as par
    assert inspect.signature(par.sweep_flux_vs_time).parameters["formal"].default is False
    assert inspect.signature(classes.JetModel.flux_vs_time).parameters["formal"].default is False
    m = _Model()
    times = np.array([3., 1., 2., 1., 0.5]) * orc.YEAR
    freqs = np.array([5e9, 2e10, 4e10])
    out = par.sweep_flux_vs_time(m, times, freqs, formal=True)
    assert len(m.engine.calls) == 1
    c = m.engine.calls[0]
    assert c["epochs"] == [float(t) for t in times]
    assert c["want_maps"] is False and c["want_totals"] is True
    assert c["fields"] is m.device_fields and c["bursts"] is m.the_bursts
    assert c["mode"] == E.RJP_GFF_POWERLAW
    ctau, cflux = E.ff_channel_coeffs(freqs, 0.5, 120., E.RJP_GFF_POWERLAW, None)
    assert np.array_equal(c["ctau"], np.array(ctau)) and np.array_equal(c["csrc"], np.array(cflux))
    assert isinstance(out, np.ndarray)
    assert np.array_equal(out, np.arange(15, dtype=np.float64).reshape(5, 3))
    # a rank without epochs makes no call and contributes an empty block
    m2 = _Model()
    sh = par.EpochShards(times[:1], 2)
    assert len(sh.local(1)) == 0
    with pytest.raises(RuntimeError):
        # (no process group here: the gather of a 2-rank sweep cannot run; the point is that the
        # engine was not called for the empty shard before it)
        par.sweep_flux_vs_time(m2, times[:1], freqs, rank=1, world=2, formal=True)
    assert m2.engine.calls == []
