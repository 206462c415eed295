"""Device engine: owns the librjprt context of one GPU and the device-resident model fields.

PyTorch (ROCm) is used for device memory, streams and (elsewhere) torch.distributed only; all
arithmetic on the RT path happens inside librjprt's HIP kernels.  Nothing here falls back to
the CPU: without a GPU or without the built library, construction raises.
"""
import ctypes as C
import os
import weakref

import numpy as np

from . import _constants as con
from . import _lib
from ._lib import RJP_F32, RJP_F64, RJP_GFF_POWERLAW, RJP_GFF_SCALAR  # noqa: F401
from .imaging import (SIDEREAL_DAY_S, AntennaConfig, Geodetic, antenna_config_path,  # noqa: F401
                      beam_from_quadratic, beam_quadratic, fit_beam, gauss_results, gauss_start,
                      geodetic, image_rms, image_scales, observation_grid, observing_plan,
                      read_antenna_config, scale_biases, scale_kernel, taylor_hessian_inverse,
                      taylor_weights, thermal_sigma, vis_scales)
from .imaging import (UVFIT_MAX_COMP, uvfit_components, uvfit_results, uvfit_start,  # noqa: F401
                      uvfit_theta, uvfit_theta_from_imfit)
from .imaging import (AUTOMASK_DEFAULTS, automask_options, automask_step,  # noqa: F401
                      image_stats_results)
from .spectra import (SPECFIT_MAX_CHAN, SPECFIT_MAX_COMP, VOIGTFIT_MAX_COMP,  # noqa: F401
                      channel_widths, specfit_results, specfit_start, velocity_axis, voigt_results,
                      voigt_start)
from .calibration import (GAINCAL_MAX_ANT, gain_results, random_gains,  # noqa: F401
                          solution_intervals)
from .inference import (NORMAL_EQ_MAX_SEL, BurstFit, EjectionFit, LMResult,  # noqa: F401
                        lm_minimise, unpack_triangle)


def _torch():
    import torch
    return torch


def _ptr(t):
    """Device address of a tensor; NULL for None."""
    return t.data_ptr() if t is not None else None


def _ref(s):
    """An optional struct (rjp_bursts) by reference; NULL for None."""
    return C.byref(s) if s is not None else None


def _tensor_key(t):
    """(address, version) of a tensor: the version counter catches in-place edits under the same
    pointer, the pointer a new tensor (whose counter starts again)."""
    return (t.data_ptr(), t._version)


def lt_key(a0, ts, ts_lo, ts_hi):
    """What a launch-time-ordered layout was built from."""
    return _tensor_key(a0) + _tensor_key(ts) + (float(ts_lo), float(ts_hi))


def mom_cache_key(a0, ts, d_ts, ts_lo, ts_hi, bursts_red, bursts_blue):
    """What the cached moment maps are sums over: a0, the launch times (`d_ts`: the tensor the
    scan reads, `ts` or its unmasked copy), the range and WHICH jets have bursts."""
    return _tensor_key(a0) + _tensor_key(ts) + (d_ts, float(ts_lo), float(ts_hi),
                                                bool(bursts_red), bool(bursts_blue))


def unmasked_key(jet, ts, flag, rng):
    """What the unmasked launch-time copy was made from."""
    return (int(jet),) + _tensor_key(ts) + _tensor_key(flag) + (rng,)


class DeviceFields:
    """The packed per-cell state in HBM (include/rjprt.h `rjp_fields`).

    Derived state and its keys (DESIGN.md "Derived state"): everything built FROM `a0` / `ts` --
    the launch-time-ordered layout `lt`, the bucketed layout `srt`, the cached moment maps
    `mom_cache`, the unmasked launch-time copy -- is keyed on those tensors' address AND
    `_version`, so an in-place edit of `a0` or `ts` (a jet flag flipped, cells moved to other
    launch times) makes it stale: a stale item is dropped or rebuilt, never attached.  The
    launch-time range is the one exception: it is a DECLARATION the kernels watch (the range
    guard), measured once per `ts` tensor; an in-place edit that leaves it poisons the sightlines
    concerned and is reported by the next call.  In-place edits of the OTHER fields (nd, xi, temp,
    pf, em0) are the caller's duty: rebuild what depends on them (`RTEngine.compact`,
    `tau_layout`, `compute_y_bounds`), or go through `RTEngine.replace_field`, which does."""

    def __init__(self, shape, dtype, csize_au, nd, xi, temp, pf, ts=None, vy=None,
                 ff_raw=None, areas_raw=None):
        self.shape = tuple(int(s) for s in shape)
        self.dtype = int(dtype)
        self.csize_au = float(csize_au)
        self.nd, self.xi, self.temp, self.pf, self.ts, self.vy = nd, xi, temp, pf, ts, vy
        self.ff_raw, self.areas_raw = ff_raw, areas_raw
        self.ylo = self.yhi = None          # optional occupied y-range per sightline (int32)
        self.em0 = None                     # optional compact scan field (rjp_fields.d_em0)
        self.a0 = None                      # optional tau scan field (rjp_fields.d_a0) ...
        self.a0_mode = 0                    # ... and the Gaunt mode it was built for
        self.occupied_cells = 0             # cells inside the occupied y-ranges (0 = unknown)
        self.ts_range = None                # optional (ts_lo, ts_hi) of the finite launch times
        self._ts_range_of = None            # ... and the `ts` tensor it was measured on
        self.lt = None                      # optional launch-time-ordered layout (RTEngine.build_lt)
        self.mom_cache = None               # optional cache of the launch-time moment maps of a0
        self.srt = None                     # optional launch-time-bucketed layout (RTEngine.build_sorted)

    @property
    def ncells(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

    @property
    def npix(self):
        return self.shape[0] * self.shape[2]

    def struct(self):
        f = _lib.Fields()
        f.d_nd, f.d_xi, f.d_temp, f.d_pf = (_ptr(t) for t in
                                            (self.nd, self.xi, self.temp, self.pf))
        f.d_em0 = self.em0.data_ptr() if self.em0 is not None else None
        f.d_a0 = self.a0.data_ptr() if self.a0 is not None else None
        f.a0_mode = int(self.a0_mode)
        if (self.ts_range is not None and self.ts is not None and
                self._ts_range_of == self.ts.data_ptr()):
            f.ts_lo, f.ts_hi = self.ts_range
        f.d_ts = self.ts.data_ptr() if self.ts is not None else None
        f.d_vy = self.vy.data_ptr() if self.vy is not None else None
        f.nx, f.ny, f.nz = self.shape
        f.dtype = self.dtype
        f.csize_au = self.csize_au
        f.d_ylo = self.ylo.data_ptr() if self.ylo is not None else None
        f.d_yhi = self.yhi.data_ptr() if self.yhi is not None else None
        f.occupied_cells = int(self.occupied_cells) if self.ylo is not None else 0
        lt = self.lt
        if (lt is not None and self.a0 is not None and self.ts is not None and
                lt["key"] == lt_key(self.a0, self.ts, f.ts_lo, f.ts_hi)):
            # (the layout belongs to the a0 / ts -- address and version -- and the launch-time
            # range it was built from)
            f.d_lt_cells = lt["cells"].data_ptr()
            f.d_lt_rowoff = lt["rowoff"].data_ptr()
            f.d_lt_aux = lt["aux"].data_ptr()
            f.lt_K = int(lt["K"])
        return f

    def scan_fields(self, gff_mode, want_em=True):
        """Fields per cell one continuum grid pass streams: 2 on the tau layout (a0, ts; em0 as
        a third only with emission-measure maps), 3 on the compact one (em0, temp, ts), else the
        5 wide ones."""
        if (self.a0 is not None and self.a0_mode == gff_mode and self.dtype == RJP_F64 and
                (not want_em or self.em0 is not None)):
            return 3 if want_em else 2
        return 3 if self.em0 is not None else 5

    def nbytes(self, rrl=False, gff_mode=None, want_em=True):
        """Bytes one grid pass streams: the RRL scan reads the six wide fields; the continuum
        scan what `scan_fields` says (without `gff_mode`: the compact / wide figure)."""
        if rrl:
            n = 6
        elif gff_mode is None:
            n = 3 if self.em0 is not None else 5
        else:
            n = self.scan_fields(gff_mode, want_em)
        return n * self.ncells * self.dtype

    def drop_wide(self):
        """Free nd / xi / pf once the compact field is attached (continuum-only sweeps of
        grids that would not otherwise fit; the RRL and collapse=False calls need them)."""
        if self.em0 is None:
            raise ValueError("no compact layout attached")
        self.nd = self.xi = self.pf = None

    def drop_tau(self):
        """Detach the tau layout (scans fall back to the compact / wide one)."""
        self.a0 = None


def make_bursts(red, blue):
    """Build an rjp_bursts from per-jet lists of (t0_s, amp_rel, sigma_s)
    (classes.py:442-448: sigma = half_life * 2 / (2 sqrt(2 ln 2))).  Any number per jet, as
    the reference (classes.py:245-264)."""
    b = _lib.Bursts()
    b._keep = []
    for j, lst in enumerate((red, blue)):
        n = len(lst)
        b.n[j] = n
        cols = ([float(t0) for t0, _, _ in lst], [float(a) for _, a, _ in lst],
                [1.0 / (2.0 * float(sg) ** 2.0) for _, _, sg in lst])
        for name, col in zip(("t0", "amp_rel", "inv2s2"), cols):
            arr = (C.c_double * max(n, 1))(*col)
            b._keep.append(arr)
            getattr(b, name)[j] = C.cast(arr, C.POINTER(C.c_double))
    return b


class RTEngine:
    """One per process/rank: binds to `cuda:<device>`."""

    def __init__(self, device=0):
        torch = _torch()
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.RjprtError("no GPU visible to PyTorch: rajepy_amd needs an MI355X "
                                  "(there is no CPU fallback)")
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        torch.cuda.set_device(self.device)
        ctx = C.c_void_p()
        self._check(self.lib.rjp_ctx_create(self.device_index, C.byref(ctx)), None,
                   "rjp_ctx_create")
        self.ctx = ctx
        self._work = None
        self.use_compact = not (_lib.DEBUG and os.environ.get("RJP_NO_COMPACT"))
        self.use_tau = not (_lib.DEBUG and os.environ.get("RJP_NO_TAU"))
        # epoch sweeps by launch-time moments (rjp_fields.ts_lo / ts_hi): off = the epoch tiles
        self.use_moments = not (_lib.DEBUG and os.environ.get("RJP_NO_MOMENTS"))
        self.force_moments = False     # tests: skip the library's tiles-or-moments cost model
        self.use_lt = True             # False: ignore an attached launch-time-ordered layout
        # single-epoch scans of large maps on the tau layout take the burst factor from a table in
        # LDS (ff_scan_tab.hip; needs the launch-time range); False: always the Gaussians
        self.use_chi_table = True
        # ... and read only the launch-time bins inside the bursts' support from the bucketed
        # layout the producers attach (build_sorted); False: always the grid order (A/B runs)
        self.use_sorted = True
        self.srt_min_free = 0.2        # the layout is built only if this share of HBM stays free
        # ... with its Chebyshev moments of order srt_N (16, 20 or 24), from which the bins where
        # chi^2 is smooth are contracted instead of read; False: every bin of the support is read
        # (A/B runs).  The moments count in the srt_min_free rule: the layout is attached without
        # them when they do not fit.
        self.use_srt_moments = True
        self.srt_N = 20                # K1 at cfg4, 1 yr: 0.68 / 0.57 / 0.59 ms at N = 16 / 20 / 24
        # ... and with its packed state (rjp_srt_pack: launch times + 16-bit weights, 10 bytes per
        # cell), from which the bins that fail only against the table's own error are taken as
        # table-residual bins; False: those bins are read cell by cell (A/B runs, tests).  Counts
        # in the srt_min_free rule like the moments.
        self.use_srt_packed = True
        # ... and with the packed state its launch-time codes (rjp_srt_codes: 4 bytes per cell),
        # from which the table-residual bins stream 6 bytes per cell instead of 10; False: they
        # read the packed f64 launch times (A/B runs, tests).  Counts in the srt_min_free rule.
        self.use_srt_codes = True
        # keep the launch-time moment maps of a model that is swept repeatedly (2.7 GB at
        # 512 x 512 sightlines): from the second long sweep on only the contraction runs
        self.cache_moments = True
        self.last_moment_shape = (0, 0)
        self._unreported = {}          # fields whose moment cache a pass filled since the last
        #                                clean range-guard report (weak references by id)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.rjp_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- helpers ---------------------------------------------------------------------------
    GUARD_MESSAGE = "an earlier scan of this context met finite launch times outside"

    def _check(self, status, ctx=None, what=""):
        """`_lib.check`, and: an entry point that reports the range guard (RJP_ERR_ARG with the
        guard's message: some EARLIER, asynchronous pass met launch times outside its declared
        range and wrote NaN sums) voids whatever such passes filled."""
        try:
            _lib.check(status, ctx, what)
        except _lib.RjprtError as e:
            if self.GUARD_MESSAGE in str(e):
                self._void_unreported()
            raise

    def _call(self, name, *args):
        """`name`(ctx, *args, the current stream), its status checked under that name."""
        self._check(getattr(self.lib, name)(self.ctx, *args, self._stream()), self.ctx, name)

    def _void_unreported(self):
        """The moment maps filled since the last clean report may hold the NaNs of a pass the
        guard flagged: their recorded shape is void (the next long sweep makes its own pass).
        The layouts need no such rule: rjp_lt_count / rjp_srt_count check the range inside their
        own, synchronous counting pass and refuse, so none is ever built from a flagged pass."""
        for ref in self._unreported.values():
            fields = ref()
            mc = getattr(fields, "mom_cache", None)
            if mc is not None:
                mc["K"] = mc["N"] = 0
                mc.pop("held", None)
        self._unreported = {}

    def _stream(self):
        return C.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def _empty(self, n, dtype):
        torch = _torch()
        td = {RJP_F32: torch.float32, RJP_F64: torch.float64}[dtype]
        return torch.empty(int(n), dtype=td, device=self.device)

    def _f64(self, *shape):
        torch = _torch()
        return torch.empty(*shape, dtype=torch.float64, device=self.device)

    def _workspace(self, nbytes):
        torch = _torch()
        if self._work is None or self._work.numel() < nbytes:
            self._work = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self._work

    def _workspace_maps(self, nbytes):
        """The map stages' own scratch (per-wave flux partials): a scan and a map stage of two
        consecutive epochs may then run side by side on two streams."""
        torch = _torch()
        if getattr(self, "_work_m", None) is None or self._work_m.numel() < nbytes:
            self._work_m = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return self._work_m

    def synchronize(self):
        _torch().cuda.synchronize(self.device)

    # -- field producers ---------------------------------------------------------------------
    def upload_fields(self, nd, xi, temp, ff, areas, ts, red, vy=None, csize_au=1.0,
                      dtype=RJP_F64):
        """Host float64 grids (reference layout, classes.py:216-227) -> packed device state.
        `red` is a boolean grid (rr < 0)."""
        torch = _torch()
        shape = np.shape(nd)
        n = int(np.prod(shape))

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).to(
                self.device)

        def pack(src, den=None, redt=None):
            dst = self._empty(n, dtype)
            self._call("rjp_pack_field", src.data_ptr(), _ptr(den), _ptr(redt), dst.data_ptr(), n,
                       dtype)
            return dst

        red_t = torch.from_numpy(np.ascontiguousarray(red, dtype=np.uint8).ravel()).to(
            self.device)
        d_nd = pack(up(nd), None, red_t)
        d_xi = pack(up(xi))
        d_t = pack(up(temp))
        d_pf = pack(up(ff), up(areas))
        d_ts = pack(up(ts)) if ts is not None else None
        d_vy = pack(up(vy)) if vy is not None else None
        self.synchronize()
        return self.compact(DeviceFields(shape, dtype, csize_au, d_nd, d_xi, d_t, d_pf, d_ts,
                                         d_vy))

    def compact(self, fields):
        """Attach the compact scan layout (rjp_compact_fields): K1 then streams 3 fields
        (em0, temp, ts) instead of 5 -- bit-identical maps for f64 storage.  Fields with a
        negative path factor (nothing the reference's fill_factor / areas can produce) or,
        in f32 storage, a product outside the float range keep the wide layout.
        `RTEngine.use_compact = False` keeps every model on the wide layout (A/B runs; with
        RJP_DEBUG=1 the variable RJP_NO_COMPACT=1 sets it)."""
        torch = _torch()
        fields.em0 = None
        self._drop_derived_state(fields)
        if not self.use_compact:
            return fields
        em0 = self._empty(fields.ncells, fields.dtype)
        bad = torch.empty(1, dtype=torch.int64, device=self.device)
        fs = fields.struct()
        self._call("rjp_compact_fields", C.byref(fs), em0.data_ptr(), bad.data_ptr())
        if int(bad.item()) == 0:
            fields.em0 = em0
        return fields

    def tau_layout(self, fields, gff_mode):
        """Attach the tau scan layout for `gff_mode` (rjp_tau_field): a0 = em0 T^-1.5|-1.35,
        everything of a cell's optical depth that depends on neither frequency nor epoch.  K1
        then streams a0 and ts (16 B/cell; em0 as well only when EM maps are asked for) and
        returns bit-identical maps.  f64 storage with the compact field attached; anything else
        keeps its layout."""
        fields.a0 = None
        self._drop_derived_state(fields)
        if not self.use_tau or fields.dtype != RJP_F64 or fields.em0 is None:
            return fields
        a0 = self._f64(fields.ncells)
        fs = fields.struct()
        self._call("rjp_tau_field", C.byref(fs), int(gff_mode), a0.data_ptr())
        fields.a0, fields.a0_mode = a0, int(gff_mode)
        return fields

    @staticmethod
    def _drop_derived_state(fields):
        """What was built FROM a0 / em0 / ts goes whenever one of them is rebuilt: the
        launch-time-ordered layout, the cached moment maps, the unmasked launch-time copy.  (The
        caching allocator hands a rebuilt field the old one's address more often than not: these
        are never validated by pointer alone.)"""
        fields.lt = None
        fields.mom_cache = None
        fields._ts_unmasked = None
        fields.srt = None

    def tavg(self, fields):
        """T_avg map of the model, nanmean_y(T where T > 0) -> device tensor [P] (rjp_tavg):
        depends on neither frequency nor epoch, so a model asks once."""
        nx, ny, nz = fields.shape
        out = self._f64(fields.npix)
        wb = self.lib.rjp_ff_scan_workspace(nx, ny, nz, 1)
        work = self._workspace(wb)
        fs = fields.struct()
        self._call("rjp_tavg", C.byref(fs), out.data_ptr(), work.data_ptr(), work.numel())
        return out

    def launch_time_range(self, fields):
        """(min, max) of the finite launch times of `fields` (rjp_field_range), measured once
        per `ts` tensor: with it, scans of >= 12 epochs on the tau layout (EM maps: with em0) may
        take the moment path (include/rjprt.h `rjp_fields.ts_lo`)."""
        if fields.ts is None:
            return None
        if fields.ts_range is not None and fields._ts_range_of == fields.ts.data_ptr():
            return fields.ts_range
        part = self._f64(2 * _lib.RJP_RANGE_BLOCKS)
        self._call("rjp_field_range", fields.ts.data_ptr(), fields.ncells, fields.dtype,
                   part.data_ptr())
        h = part.cpu().numpy().reshape(-1, 2)
        lo, hi = float(h[:, 0].min()), float(h[:, 1].max())
        fields.ts_range = (lo, hi) if np.isfinite(lo) and np.isfinite(hi) and hi >= lo else None
        fields._ts_range_of = fields.ts.data_ptr()
        return fields.ts_range

    def build_lt(self, fields, K=20):
        """Attach the launch-time-ordered layout of (a0, ts) to `fields` (rjp_lt_count +
        rjp_lt_fill; include/rjprt.h `rjp_fields.d_lt_cells`): every group of 64 sightlines
        bucketed by (jet, launch-time bin), so that epoch sweeps of 12-32 epochs accumulate their
        Chebyshev moments in registers -- no LDS atomics, no moment maps in HBM.  A one-off per
        model (two passes + scattered 16-byte writes: ~50 ms for 1.07e9 cells, ~1.2 x the bytes of
        a0 + ts resident): worth it for a model that is swept many times.  Rebuild after `a0` or
        `ts` change, in place or not (a stale layout is ignored by `struct()`: its key holds the
        tensors' versions).  K bins per jet: fewer, wider bins
        pad less (rows are as long as the fullest of 64 lanes: 1.15 x at K = 16, 1.17 x at 20,
        1.22 x at 32 on the dense benchmark grid) but need a higher order for the same bursts
        (24 / 20 / 16 for the example's); 20 measured fastest there."""
        torch = _torch()
        fields.lt = None
        if fields.a0 is None or fields.ts is None or fields.dtype != RJP_F64:
            raise ValueError("the launch-time-ordered layout needs f64 fields with the tau "
                             "layout (a0) and launch times")
        if self.launch_time_range(fields) is None:
            raise ValueError("no finite launch time in the model")
        fs = fields.struct()
        nx, ny, nz = fields.shape
        n_off = self.lib.rjp_lt_rowoff_entries(nx, nz, int(K))
        if n_off == 0:
            raise ValueError("K must be 1..80")
        rowoff = torch.empty(n_off, dtype=torch.int32, device=self.device)
        total = C.c_int64()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        self._call("rjp_lt_count", C.byref(fs), int(K), rowoff.data_ptr(), C.byref(total))
        ev[1].record()
        # (allocating ~1.2 x the bytes of a0 + ts is the slow part of a first build: hipMalloc)
        cells = torch.empty(max(1, total.value) * 64 * 2, dtype=torch.float64, device=self.device)
        aux = torch.empty(3 * fields.npix, dtype=torch.float64, device=self.device)
        ev[2].record()
        self._call("rjp_lt_fill", C.byref(fs), int(K), rowoff.data_ptr(), cells.data_ptr(),
                   aux.data_ptr())
        ev[3].record()
        torch.cuda.synchronize(self.device)
        kernels_ms = ev[0].elapsed_time(ev[1]) + ev[2].elapsed_time(ev[3])
        fields.lt = {"cells": cells, "rowoff": rowoff, "aux": aux, "K": int(K),
                     "rows": int(total.value), "build_ms": kernels_ms,
                     "build_with_allocation_ms": ev[0].elapsed_time(ev[3]),
                     "bytes": cells.numel() * 8,
                     "key": lt_key(fields.a0, fields.ts, fs.ts_lo, fs.ts_hi)}
        return fields.lt

    @staticmethod
    def _srt_key(fields, fs):
        """What the launch-time-bucketed layout was built from: `_version` catches in-place edits
        of a0 / ts under the same pointer."""
        return (fields.a0.data_ptr(), fields.a0._version, fields.ts.data_ptr(),
                fields.ts._version, fs.ts_lo, fs.ts_hi, int(fields.a0_mode))

    def _srt_qualifies(self, fields):
        """Maps the single-epoch table path takes (include/rjprt.h `rjp_fields.ts_lo`: f64, tau
        layout, >= 32768 sightlines) -- the only scans that read the layout -- with sightlines of
        >= 256 rows: a scan reads <= 80 bytes of the index per sightline, <= 2 % of its cells'."""
        nx, ny, nz = fields.shape
        return (self.use_sorted and fields.dtype == RJP_F64 and fields.a0 is not None and
                fields.ts is not None and (nx * nz) // 2 >= 64 * 256 and ny >= 256)

    def build_sorted(self, fields, K=32):
        """Attach the launch-time-bucketed layout of (a0, ts) (rjp_srt_count + rjp_srt_fill;
        include/rjprt.h `rjp_fields.d_srt_cells`): per group of 64 sightlines every lane's cells
        sorted by (jet, launch-time bin), padded at the lane's end only.  A single-epoch scan then
        reads only the bins inside the bursts' support at its epoch.  Per-model state like a0:
        ~1.03 x the bytes of a0 + ts; built only when `srt_min_free` of the HBM stays free
        afterwards (returns None and attaches nothing otherwise).  Rebuild after `a0` or `ts`
        change (a stale layout is never attached: the key holds the tensors' versions).
        With `use_srt_moments` the layout's Chebyshev moments of order `srt_N` are built with it
        (rjp_srt_moments: 2 K (srt_N - 1) doubles per sightline, "mom" in the returned dict, None
        when they would break the `srt_min_free` rule); with `use_srt_packed` the packed state
        ("packed"), and with `use_srt_codes` its launch-time codes (["packed"]["pc"], with
        "pc_bytes" and "pc_build_ms"), each under the same rule."""
        torch = _torch()
        fields.srt = None
        if fields.a0 is None or fields.ts is None or fields.dtype != RJP_F64:
            raise ValueError("the launch-time-bucketed layout needs f64 fields with the tau "
                             "layout (a0) and launch times")
        if self.launch_time_range(fields) is None:
            return None
        fs = fields.struct()
        nx, ny, nz = fields.shape
        n_idx = self.lib.rjp_srt_index_entries(nx, nz, int(K))
        if n_idx == 0:
            raise ValueError("K must be 1..32")
        groups = (fields.npix + 63) // 64
        start = torch.empty(n_idx, dtype=torch.int32, device=self.device)
        rowbase = torch.empty(groups + 1, dtype=torch.int64, device=self.device)
        hist = (C.c_int64 * (2 * int(K)))()
        total = C.c_int64()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        self._call("rjp_srt_count", C.byref(fs), int(K), start.data_ptr(), rowbase.data_ptr(),
                   hist, C.byref(total))
        ev[1].record()
        need = total.value * 64 * 16 + n_idx * 8 + 3 * fields.npix * 8
        n_mom = (self.lib.rjp_srt_moment_entries(nx, nz, int(K), int(self.srt_N))
                 if self.use_srt_moments else 0)
        free, hbm = torch.cuda.mem_get_info(self.device)
        free += torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        if free - need < self.srt_min_free * hbm:
            return None
        if free - need - n_mom * 8 < self.srt_min_free * hbm:
            n_mom = 0                           # the layout fits, its moments do not
        n_prow = (self.lib.rjp_srt_packed_rows(nx, nz, total.value)
                  if n_mom and self.use_srt_packed else 0)
        if free - need - n_mom * 8 - n_prow * 64 * 10 < self.srt_min_free * hbm:
            n_prow = 0                          # ... or its packed state does not
        n_crow = n_prow if self.use_srt_codes else 0
        if free - need - n_mom * 8 - n_prow * 64 * 10 - n_crow * 64 * 4 < self.srt_min_free * hbm:
            n_crow = 0                          # ... or its launch-time codes do not
        cells = torch.empty(max(1, total.value) * 64 * 2, dtype=torch.float64, device=self.device)
        cum = torch.empty(n_idx, dtype=torch.float64, device=self.device)
        aux = torch.empty(3 * fields.npix, dtype=torch.float64, device=self.device)
        ev[2].record()
        self._call("rjp_srt_fill", C.byref(fs), int(K), start.data_ptr(), rowbase.data_ptr(),
                   cells.data_ptr(), cum.data_ptr(), aux.data_ptr())
        ev[3].record()
        mom, mom_ms = None, 0.0
        if n_mom:
            mom = torch.empty(n_mom, dtype=torch.float64, device=self.device)
            ev_m = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev_m[0].record()
            self._call("rjp_srt_moments", C.byref(fs), int(K), int(self.srt_N), start.data_ptr(),
                       rowbase.data_ptr(), cells.data_ptr(), mom.data_ptr())
            ev_m[1].record()
        packed = None
        if n_prow:
            # (one allocation of 10 bytes per cell: a freed block the size of a0 would be taken
            # for the next a0 in place of a0's own)
            buf = torch.empty(n_prow * 64 * 10, dtype=torch.uint8, device=self.device)
            pts = buf[:n_prow * 64 * 8].view(torch.float64)
            pw = buf[n_prow * 64 * 8:].view(torch.int16)
            ev_p = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev_p[0].record()
            fits = self._call_tiles("rjp_srt_pack", C.byref(fs), int(K), start.data_ptr(),
                                    rowbase.data_ptr(), cells.data_ptr(), pts.data_ptr(),
                                    pw.data_ptr())
            ev_p[1].record()
            torch.cuda.synchronize(self.device)
            if fits == 1:                       # (2: a weight outside the 16-bit format's range)
                packed = {"pts": pts, "pw": pw, "rows": int(n_prow), "bytes": n_prow * 64 * 10,
                          "build_ms": ev_p[0].elapsed_time(ev_p[1]), "version": cells._version,
                          "pc": None}
            if packed is not None and n_crow:
                pc = torch.empty(n_crow * 64, dtype=torch.int32, device=self.device)
                ev_c = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev_c[0].record()
                self._call_tiles("rjp_srt_codes", C.byref(fs), int(K), start.data_ptr(),
                                 rowbase.data_ptr(), cells.data_ptr(), pc.data_ptr())
                ev_c[1].record()
                torch.cuda.synchronize(self.device)
                packed.update(pc=pc, pc_bytes=n_crow * 64 * 4,
                              pc_build_ms=ev_c[0].elapsed_time(ev_c[1]))
        torch.cuda.synchronize(self.device)
        if mom is not None:
            mom_ms = ev_m[0].elapsed_time(ev_m[1])
        fields.srt = {"cells": cells, "start": start, "cum": cum, "rowbase": rowbase, "aux": aux,
                      "hist": hist, "K": int(K), "rows": int(total.value),
                      "build_ms": ev[0].elapsed_time(ev[1]) + ev[2].elapsed_time(ev[3]),
                      "build_with_allocation_ms": ev[0].elapsed_time(ev[3]),
                      "bytes": need, "key": self._srt_key(fields, fs),
                      "mom": mom, "N": int(self.srt_N) if mom is not None else 0,
                      "mom_build_ms": mom_ms, "mom_bytes": n_mom * 8, "packed": packed}
        return fields.srt

    def _attach_sorted(self, fields):
        """Producers: the bucketed layout right after a0, for maps that take the table path."""
        if self._srt_qualifies(fields):
            self.build_sorted(fields)
        return fields

    def compute_y_bounds(self, fields):
        """Attach the per-sightline occupied y-range to `fields` (rjp_y_bounds): later scans
        skip the rows no cell of which can contribute.  Recompute after changing a field."""
        torch = _torch()
        fields.ylo = fields.yhi = None
        fields.occupied_cells = 0
        lo = torch.empty(fields.npix, dtype=torch.int32, device=self.device)
        hi = torch.empty(fields.npix, dtype=torch.int32, device=self.device)
        fs = fields.struct()
        self._call("rjp_y_bounds", C.byref(fs), lo.data_ptr(), hi.data_ptr())
        fields.ylo, fields.yhi = lo, hi
        # (hint for the tiles-or-moments choice of long epoch sweeps, include/rjprt.h; summed by
        # the library: the first use of the equivalent torch ops costs ~0.2 s of lazy loading)
        n = C.c_int64()
        self._call("rjp_occupied_cells", lo.data_ptr(), hi.data_ptr(), fields.npix, C.byref(n))
        fields.occupied_cells = int(n.value)
        return lo, hi

    def replace_field(self, fields, name, host_array):
        """Re-upload one plain field (the reference's public setters: ts, ion_fraction,
        temperature; classes.py:857-859, 938-940, 998-1000)."""
        torch = _torch()
        assert name in ("xi", "temp", "ts", "vy")
        src = torch.from_numpy(np.ascontiguousarray(host_array, dtype=np.float64).ravel()).to(
            self.device)
        if src.numel() != fields.ncells:
            raise ValueError("grid shape mismatch")
        dst = self._empty(fields.ncells, fields.dtype)
        self._call("rjp_pack_field", src.data_ptr(), None, None, dst.data_ptr(), fields.ncells,
                   fields.dtype)
        self.synchronize()
        setattr(fields, name, dst)
        if name in ("ts", "xi", "temp"):
            fields.lt = None                    # the launch-time-ordered layout holds (a0, ts)
            fields.srt = None                   # ... and so does the bucketed one
            fields.mom_cache = None             # ... and the moment maps are sums over them
        if name == "ts":
            # what was measured on / derived from the old launch times (the new tensor may well
            # sit at the old one's address: never key these on the pointer alone)
            fields.ts_range = fields._ts_range_of = None
            fields._ts_unmasked = None
        had_tau = fields.a0 is not None
        if name == "xi" and fields.em0 is not None:
            self.compact(fields)                # em0 holds (nd xi)^2 pf
        if had_tau and name in ("xi", "temp"):
            self.tau_layout(fields, fields.a0_mode)     # a0 holds em0 T^-1.5|-1.35
        if fields.ylo is not None and name in ("xi", "temp"):
            self.compute_y_bounds(fields)       # the occupied range depends on these fields

    def _direct_em0(self, n, dtype):
        """f64 producers write the compact scan field in their own pass (f32 goes through
        rjp_compact_fields and its range check)."""
        if dtype != RJP_F64 or not self.use_compact:
            return None
        return self._f64(n)

    def _direct_a0(self, n, dtype, tau_mode):
        """... and the tau scan field when a Gaunt mode is named."""
        if tau_mode is None or dtype != RJP_F64 or not (self.use_compact and self.use_tau):
            return None
        return self._f64(n)

    def build_fields(self, geom, dtype=RJP_F64, want_ts=True, want_vy=True, want_raw=True,
                     want_vxz=False, want_wide=True, tau_mode=None):
        """K4: geometry -> packed fields on the device (`geom` is a _lib.Geometry).
        `want_wide=False` (f64, continuum only) skips nd / xi / pf: 24 B/cell resident.
        `tau_mode` = the model's Gaunt mode: K4 writes the tau scan field a0 in the same pass."""
        n = geom.nx * geom.ny * geom.nz
        em0 = self._direct_em0(n, dtype)
        a0 = self._direct_a0(n, dtype, tau_mode)
        if not want_wide and em0 is None:
            raise ValueError("want_wide=False needs the compact layout (f64 storage)")
        nd, xi, pf = ((self._empty(n, dtype) for _ in range(3)) if want_wide
                      else (None, None, None))
        temp = self._empty(n, dtype)
        ts = self._empty(n, dtype) if want_ts else None
        vy = self._empty(n, dtype) if want_vy else None
        ffr = self._f64(n) if want_raw else None
        arr = self._f64(n) if want_raw else None
        vxr = self._f64(n) if want_vxz else None
        vzr = self._f64(n) if want_vxz else None
        self._call("rjp_build_fields", C.byref(geom), dtype, _ptr(nd), _ptr(xi), temp.data_ptr(),
                   _ptr(pf), _ptr(ts), _ptr(vy), _ptr(ffr), _ptr(arr), _ptr(vxr), _ptr(vzr),
                   _ptr(em0), _ptr(a0), int(tau_mode or 0))
        out = DeviceFields((geom.nx, geom.ny, geom.nz), dtype, geom.csize, nd, xi, temp, pf,
                           ts, vy, ffr, arr)
        out.vx_raw, out.vz_raw = vxr, vzr
        if em0 is not None:
            out.em0 = em0
            if a0 is not None:
                out.a0, out.a0_mode = a0, int(tau_mode)
                self._attach_sorted(out)
            return out
        out = self.compact(out)
        if tau_mode is None:
            return out
        return self._attach_sorted(self.tau_layout(out, tau_mode))

    def build_wide(self, fields, geom):
        """Attach the wide fields a lean model left out (K4 again, writing nd / xi / pf / vy only):
        what the RRL scan, the collapse=False kernels, the grid accessors and the `ion_fraction` /
        `vel` setters need -- a continuum pipeline never asks (classes.JetModel._wide_fields)."""
        n = fields.ncells
        new = {k: self._empty(n, fields.dtype) for k in ("nd", "xi", "pf", "vy")
               if getattr(fields, k) is None}
        if not new:
            return fields
        nd, xi, pf, vy = (_ptr(new.get(k)) for k in ("nd", "xi", "pf", "vy"))
        self._call("rjp_build_fields", C.byref(geom), fields.dtype, nd, xi, None, pf, None, vy,
                   None, None, None, None, None, None, 0)
        for k, t in new.items():
            setattr(fields, k, t)
        return fields

    def synth_fields(self, shape, seed, temp_mode=0, dtype=RJP_F64, csize_au=0.5,
                     with_vy=False, cell0=0, wide=True, tau_mode=None, with_em0=True):
        """Measurement harness: dense synthetic fields generated on the device
        (SURVEY.md 8(d)); `shape` may be a sub-block starting at flat cell `cell0` of a
        grid whose z-extent is shape[2].  `wide=False` (f64) generates only the compact scan
        layout (em0, temp, ts): 24 B/cell.  `tau_mode`: also the tau scan field a0 for that
        Gaunt mode, in the same pass; with `with_em0=False` as well the generator leaves a0,
        temp, ts (scans without emission-measure maps: 16 B/cell streamed)."""
        nx, ny, nz = shape
        n = nx * ny * nz
        em0 = self._direct_em0(n, dtype)
        a0 = self._direct_a0(n, dtype, tau_mode)
        if not wide and em0 is None:
            raise ValueError("wide=False needs the compact layout (f64 storage)")
        if not with_em0:
            if wide or a0 is None:
                raise ValueError("with_em0=False is for wide=False with a tau_mode (f64 storage)")
            em0 = None
        nd, xi, pf = ((self._empty(n, dtype) for _ in range(3)) if wide else (None, None, None))
        temp, ts = self._empty(n, dtype), self._empty(n, dtype)
        vy = self._empty(n, dtype) if with_vy else None
        self._call("rjp_synth_fields", int(seed), int(temp_mode), int(nz), int(cell0), int(n),
                   dtype, _ptr(nd), _ptr(xi), temp.data_ptr(), _ptr(pf), ts.data_ptr(), _ptr(vy),
                   _ptr(em0), _ptr(a0), int(tau_mode or 0))
        out = DeviceFields(shape, dtype, csize_au, nd, xi, temp, pf, ts, vy)
        if a0 is not None:
            out.a0, out.a0_mode = a0, int(tau_mode)
        if em0 is not None:
            out.em0 = em0
        if em0 is not None or not with_em0:
            return self._attach_sorted(out) if a0 is not None else out
        out = self.compact(out)
        if tau_mode is None:
            return out
        return self._attach_sorted(self.tau_layout(out, tau_mode))

    # -- K1 / K2 -----------------------------------------------------------------------------
    def _scan_struct(self, fields, bursts, n_epochs=1):
        """`rjp_fields` for a free-free scan.  A model with bursts in ONE jet only scans a copy
        of the launch times in which the NaNs of the other jet's cells are cleared
        (rjp_unmask_launch_times): the reference's burst-less jet has a constant mass-loss rate,
        so a NaN launch time does not drop its cells (classes.py:232-233, 442-448).  The copy
        is kept with the fields and rebuilt when `ts` or the flag-carrying field changes."""
        if bursts is not None and (
                (self.use_moments and n_epochs >= 12 and fields.a0 is not None) or
                (self.use_chi_table and n_epochs == 1 and fields.dtype == RJP_F64 and
                 fields.ts is not None)):
            self.launch_time_range(fields)
        fs = fields.struct()
        if n_epochs == 1 and not self.use_chi_table:
            fs.ts_lo = fs.ts_hi = 0.0
        if not (self.use_lt and self.use_moments):
            fs.d_lt_cells = fs.d_lt_rowoff = fs.d_lt_aux = None
            fs.lt_K = 0
        srt = fields.srt
        if (srt is not None and n_epochs == 1 and self.use_sorted and self.use_chi_table and
                fields.a0 is not None and fields.ts is not None and
                srt["key"] == self._srt_key(fields, fs)):
            # (built from fields.ts itself: a jet without bursts gets its NaN launch times back
            # through the layout's aux sums, whatever copy of the launch times the scan is given)
            fs.d_srt_cells = srt["cells"].data_ptr()
            fs.d_srt_start = srt["start"].data_ptr()
            fs.d_srt_cum = srt["cum"].data_ptr()
            fs.d_srt_rowbase = srt["rowbase"].data_ptr()
            fs.d_srt_aux = srt["aux"].data_ptr()
            fs.h_srt_hist = C.cast(srt["hist"], C.c_void_p)
            fs.srt_K = srt["K"]
            if self.use_srt_moments and srt.get("mom") is not None:
                fs.d_srt_mom = srt["mom"].data_ptr()
                fs.srt_N = srt["N"]
                packed = srt.get("packed")
                # (the packed state restates the cells: cells edited in place detach it)
                if (self.use_srt_packed and packed is not None and
                        packed["version"] == srt["cells"]._version):
                    fs.d_srt_pts = packed["pts"].data_ptr()
                    fs.d_srt_pw = packed["pw"].data_ptr()
                    # (the codes share the packed state's version key)
                    if self.use_srt_codes and packed.get("pc") is not None:
                        fs.d_srt_pc = packed["pc"].data_ptr()
        if not self.use_moments and n_epochs != 1:
            fs.ts_lo = fs.ts_hi = 0.0
        elif self.force_moments:
            fs.occupied_cells = -1
        if bursts is None or fields.ts is None:
            return fs
        n_r, n_b = int(bursts.n[0]), int(bursts.n[1])
        if (n_r == 0) == (n_b == 0):
            return fs
        jet = 0 if n_r == 0 else 1
        flag = fields.a0 if fields.a0 is not None else (fields.em0 if fields.em0 is not None
                                                        else fields.nd)
        # (the copy's replacement value is the lower end of the launch-time range, so that the
        # copy obeys the range it is scanned under: measure the range first, key the copy on it)
        rng = self.launch_time_range(fields)
        full = fields.struct()
        key = unmasked_key(jet, fields.ts, flag, rng)
        cached = getattr(fields, "_ts_unmasked", None)
        if cached is None or cached[0] != key:
            out = self._empty(fields.ncells, fields.dtype)
            self._call("rjp_unmask_launch_times", C.byref(full), jet, out.data_ptr())
            cached = fields._ts_unmasked = (key, out)
        fs.d_ts = cached[1].data_ptr()
        return fs

    def ff_scan(self, fields, bursts, epochs_s, gff_mode, want_em=True, out=None,
                want_tavg=True):
        """-> (sumA[E,P], em[E,P] or None, tavg[P] or None) device tensors (float64).
        `want_tavg=False`: no T_avg map (a caller that keeps the model's map from `tavg()`; on
        the tau layout the scan then never reads the temperature field)."""
        E = len(epochs_s)
        P = fields.npix
        nx, ny, nz = fields.shape
        if out is None:
            sumA = self._f64(E, P)
            em = self._f64(E, P) if want_em else None
            tavg = self._f64(P) if want_tavg else None
        else:
            sumA, em, tavg = out
        wb = self.lib.rjp_ff_scan_workspace(nx, ny, nz, E)
        work = self._workspace(wb)
        fs = self._scan_struct(fields, bursts, E)
        mkey = self._attach_moment_cache(fields, bursts, fs, E, em is not None)
        ep = _lib.dbl_array(epochs_s)
        self._call("rjp_ff_scan", C.byref(fs), _ref(bursts), ep, E, int(gff_mode), sumA.data_ptr(),
                   _ptr(em), _ptr(tavg), work.data_ptr(), work.numel())
        if mkey is not None:
            self._note_moment_sweep(fields, mkey)
        return sumA, em, tavg

    def ff_step(self, fields, bursts, epochs_s, gff_mode, tavg, ctau, cflux, out):
        """K1 + K2 from ONE call into the library (rjp_ff_step): the scan of `epochs_s` and the map
        stage for the channels of (ctau, cflux), for callers whose step is shorter than two trips
        through ctypes (x-slabs of a sharded grid, small models).  `tavg`: the model's T_avg map;
        `out` = (sumA[E,P], em[E,P] | None, tau[E,F,P] | None, flux[E,F,P] | None,
        ftot[E,F] | None) device tensors."""
        sumA, em, tau, flux, ftot = out
        E, P, F = len(epochs_s), fields.npix, len(ctau)
        nx, ny, nz = fields.shape
        work = self._workspace(self.lib.rjp_ff_scan_workspace(nx, ny, nz, E))
        wm = self._workspace_maps(self.lib.rjp_ff_maps_workspace(P, E, F)) \
            if ftot is not None else None
        fs = self._scan_struct(fields, bursts, E)
        mkey = self._attach_moment_cache(fields, bursts, fs, E, em is not None)
        self._call("rjp_ff_step", C.byref(fs), _ref(bursts), _lib.dbl_array(epochs_s), E,
                   int(gff_mode), tavg.data_ptr(), _lib.dbl_array(ctau), _lib.dbl_array(cflux), F,
                   sumA.data_ptr(), _ptr(em), _ptr(tau), _ptr(flux), _ptr(ftot), work.data_ptr(),
                   work.numel(), _ptr(wm), wm.numel() if wm is not None else 0)
        if mkey is not None:
            self._note_moment_sweep(fields, mkey)
        return out

    def range_guard(self):
        """True when a scan of this engine met finite launch times outside the range its fields
        declared (rjp_range_guard; the sums of those sightlines are NaN).  Synchronises."""
        self.synchronize()
        raised = self.lib.rjp_range_guard(self.ctx) == 1
        if raised:
            self._void_unreported()
        else:
            self._unreported = {}     # (synchronised and clean: everything filled so far is good)
        return raised

    def _attach_moment_cache(self, fields, bursts, fs, n_epochs, want_em):
        """The caller-kept moment maps of include/rjprt.h `rjp_fields.d_mom_cache`.  A long sweep
        of a densely filled model gets the buffer at once: its own pass fills it, and every later
        sweep of the same fields (same launch times, same set of jets with bursts) is the
        contraction alone; a sparse model -- whose sweeps the library's cost model keeps on the
        epoch tiles -- reserves it only after a sweep HAS taken the moment path.  Returns the
        key the cache would be valid for (None: this scan cannot use one)."""
        if not (self.cache_moments and self.use_moments and n_epochs >= 12 and not want_em and
                bursts is not None and fields.a0 is not None and fields.ts is not None and
                fs.ts_lo != fs.ts_hi):
            return None
        key = mom_cache_key(fields.a0, fields.ts, fs.d_ts, fs.ts_lo, fs.ts_hi,
                            int(bursts.n[0]) > 0, int(bursts.n[1]) > 0)
        mc = fields.mom_cache
        if mc is None and (fields.ylo is None or
                           2 * int(fields.occupied_cells) >= fields.ncells):
            mc = self._reserve_moment_cache(fields, key)
        if mc is not None and mc.get("buf") is not None:
            if mc["key"] != key:
                mc["K"] = mc["N"] = 0
                mc["key"] = key
            fs.d_mom_cache = mc["buf"].data_ptr()
            fs.mom_cache_K, fs.mom_cache_N = mc["K"], mc["N"]
            # the call may start rewriting the buffer in another shape and then fail: the recorded
            # shape is void until `_note_moment_sweep` says what the buffer holds afterwards
            mc["held"] = (mc["K"], mc["N"])
            mc["K"] = mc["N"] = 0
        return key

    def _reserve_moment_cache(self, fields, key):
        nx, _, nz = fields.shape
        nbytes = self.lib.rjp_moment_cache_bytes(nx, nz)
        try:
            buf = _torch().empty(nbytes // 8, dtype=_torch().float64, device=self.device)
        except RuntimeError:                      # no room for it: sweeps keep their pass
            return None
        fields.mom_cache = {"buf": buf, "K": 0, "N": 0, "key": key}
        return fields.mom_cache

    def _note_moment_sweep(self, fields, key):
        path = self.last_scan_path()[0]
        mc = fields.mom_cache
        if path in ("moments", "cached"):
            if mc is None or mc.get("buf") is None:
                self._reserve_moment_cache(fields, key)       # the next sweep fills it
            else:
                mc["K"], mc["N"] = self.last_moment_shape     # this sweep's pass filled it
                mc["key"] = key
                mc.pop("held", None)
                if path == "moments":
                    # (an asynchronous pass: whether the range guard flagged it is known only
                    # when a later entry point reports -- `_check` then voids the shape)
                    self._unreported[id(fields)] = weakref.ref(fields)
        elif mc is not None:
            # another path ran (tiles, the launch-time-ordered layout): nothing was written -- the
            # buffer holds what it held; one that has never held moments is given back
            mc["K"], mc["N"] = mc.pop("held", (0, 0))
            if mc["K"] == 0:
                fields.mom_cache = None

    def last_scan_path(self):
        """('tiles' | 'moments' | 'lt' | 'table', worst relative error of the expansion) of the
        last rjp_ff_scan of this engine ('lt' = moments on the launch-time-ordered layout,
        'table' = single-epoch scan with the burst factor from a table in LDS)."""
        err = C.c_double()
        shape = (C.c_int32 * 2)()
        path = self.lib.rjp_last_scan_path(self.ctx, C.byref(err), shape)
        self.last_moment_shape = (int(shape[0]), int(shape[1]))      # (bins, order); (0, 0) = tiles
        return {0: "tiles", 1: "moments", 2: "lt", 3: "table", 4: "cached"}[path], err.value

    def last_scan_tiles(self):
        """[(e0, et, uniform, nsplit, vec)] of the epoch tiles the last rjp_ff_scan / rjp_ff_step of
        this engine launched (rjp_last_scan_tiles): first epoch, epochs, 1 where the tile ran the
        uniform-spacing recurrence, y-ranges, sightlines per lane.  [] after a scan on another
        path.  Host-only; for tests."""
        n = C.c_int32()
        rc = self.lib.rjp_last_scan_tiles(self.ctx, C.byref(n), None, 0)
        if n.value == 0:
            self._check(rc, self.ctx, "rjp_last_scan_tiles")
            return []
        buf = (C.c_int32 * (5 * n.value))()
        self._check(self.lib.rjp_last_scan_tiles(self.ctx, C.byref(n), buf, n.value), self.ctx,
                    "rjp_last_scan_tiles")
        return [tuple(int(buf[5 * k + i]) for i in range(5)) for k in range(n.value)]

    def last_scan_layout(self):
        """Which layout of (a0, ts) the last scan read (rjp_last_scan_layout): 'grid' (grid
        order) or 'sorted' (the launch-time-bucketed layout, only the bins inside the bursts'
        support).  `last_scan_path` says 'table' for both: chi comes from the table either way."""
        return {0: "grid", 1: "sorted"}[self.lib.rjp_last_scan_layout(self.ctx)]

    def last_srt_bins(self):
        """(contracted, read): the (jet, bin) decisions of the last scan on the bucketed layout
        with moments, summed over its groups of 64 sightlines (rjp_last_srt_bins; synchronises
        the device).  (0, 0) after a scan without moments."""
        c, r = C.c_int64(), C.c_int64()
        self._check(self.lib.rjp_last_srt_bins(self.ctx, C.byref(c), C.byref(r)), self.ctx,
                   "rjp_last_srt_bins")
        return int(c.value), int(r.value)

    def last_srt_resid(self):
        """The table-residual (group, jet, bin) triples of the last scan, a subset of
        `last_srt_bins()`'s read ones (rjp_last_srt_resid; synchronises the device)."""
        n = int(self.lib.rjp_last_srt_resid(self.ctx))
        if n < 0:
            self._check(n, self.ctx, "rjp_last_srt_resid")
        return n

    def last_srt_fallbacks(self):
        """The cells of the last scan's table-residual bins that were re-read from the layout's
        cells because their launch-time code could not decide the table piece
        (rjp_last_srt_fallbacks; synchronises the device).  0 for a scan without the codes."""
        n = int(self.lib.rjp_last_srt_fallbacks(self.ctx))
        if n < 0:
            self._check(n, self.ctx, "rjp_last_srt_fallbacks")
        return n

    def last_table_build_ms(self):
        """Host wall time of the last coefficient-table build (a new bursts / epochs request)."""
        return float(self.lib.rjp_last_table_build_ms(self.ctx))

    def time_ff_scan(self, fields, bursts, epochs_s, gff_mode, reps=5, want_em=True,
                     want_tavg=True):
        """Average device time [ms] of one rjp_ff_scan (HIP events on the launch stream)."""
        E = len(epochs_s)
        P = fields.npix
        nx, ny, nz = fields.shape
        sumA, em = self._f64(E, P), (self._f64(E, P) if want_em else None)
        tavg = self._f64(P) if want_tavg else None
        wb = self.lib.rjp_ff_scan_workspace(nx, ny, nz, E)
        work = self._workspace(wb)
        fs = self._scan_struct(fields, bursts, E)
        ep = _lib.dbl_array(epochs_s)
        ms = C.c_double()
        self._check(self.lib.rjp_time_ff_scan(
            self.ctx, C.byref(fs), _ref(bursts), ep, E,
            int(gff_mode), sumA.data_ptr(), _ptr(em),
            _ptr(tavg), work.data_ptr(), work.numel(),
            self._stream(), int(reps), C.byref(ms)), self.ctx, "rjp_time_ff_scan")
        return ms.value

    def ff_maps(self, sumA, tavg, ctau, cflux, want_tau=True, want_flux=True,
                want_ftot=True, out=None):
        """-> (tau[E,F,P], flux[E,F,P], ftot[E,F]) device tensors (None where not wanted)."""
        E, P = sumA.shape
        F = len(ctau)
        if out is None:
            tau = self._f64(E, F, P) if want_tau else None
            flux = self._f64(E, F, P) if want_flux else None
            ftot = self._f64(E, F) if want_ftot else None
        else:
            tau, flux, ftot = out
        wb = self.lib.rjp_ff_maps_workspace(P, E, F)
        work = self._workspace_maps(wb) if ftot is not None else None
        a, b = _lib.dbl_array(ctau), _lib.dbl_array(cflux)
        self._call("rjp_ff_maps", sumA.data_ptr(), tavg.data_ptr(), P, E, a, b, F, _ptr(tau),
                   _ptr(flux), _ptr(ftot), _ptr(work), work.numel() if work is not None else 0)
        return tau, flux, ftot

    def last_maps_launch(self):
        """(kernel, VEC, KP, blocks, nparts, fchunk) of the map stage the last `ff_maps` /
        `ff_step` of this engine launched (rjp_last_maps_launch): kernel 'small' | 'acc' | 'ftot'
        (None before the first), pixels per lane, pixel groups per lane, workgroups along the
        pixel axis, partial sums per (epoch, channel) (0 without totals), channels per workgroup.
        Host-only; for tests."""
        buf = (C.c_int32 * 6)()
        self._check(self.lib.rjp_last_maps_launch(self.ctx, buf), self.ctx, "rjp_last_maps_launch")
        return ({-1: None, 0: "small", 1: "acc", 2: "ftot"}[int(buf[0])],) + \
            tuple(int(v) for v in buf[1:])

    def ff_cells(self, fields, bursts, time_s, gff_mode, ctau):
        """collapse=False: per-cell free-free optical depths -> device tensor [F, N]."""
        F = len(ctau)
        out = self._f64(F, fields.ncells)
        fs = fields.struct()
        self._call("rjp_ff_cells", C.byref(fs), _ref(bursts), float(time_s), int(gff_mode),
                   _lib.dbl_array(ctau), F, out.data_ptr())
        return out

    def ff_formal(self, fields, bursts, time_s, gff_mode, ctau, csrc, out=None):
        """Free-free intensity by the formal solution along the line of sight (rjp_ff_formal):
        csrc[f] * sum_i T_i (1 - e^-dtau_i) exp(-sum_{j in front} dtau_j), observer at the iy = 0
        end of axis 1 -> device tensor [F, P] (float64), NaN where the sightline has no T > 0.
        `ctau` as for `ff_maps`; `csrc` = its `cflux` for Jy/pixel, or 2 nu^2 k / c^2 for
        W m^-2 Hz^-1 sr^-1.  One epoch (`time_s` [s]) per call; any layout of `fields`."""
        F = len(ctau)
        if out is None:
            out = self._f64(F, fields.npix)
        fs = fields.struct()
        self._call("rjp_ff_formal", C.byref(fs), _ref(bursts), float(time_s), int(gff_mode),
                   _lib.dbl_array(ctau), _lib.dbl_array(csrc), F, out.data_ptr())
        return out

    def ff_formal_sweep(self, fields, bursts, epochs_s, gff_mode, ctau, csrc, want_maps=False,
                        want_totals=True):
        """Epoch sweep of the formal solution (rjp_ff_formal_sweep): ONE pass over the fields for
        all of `epochs_s` [s] -> (maps[E, F, P] | None, ftot[E, F] | None) device tensors
        (float64).  `maps[e]` equals `ff_formal` at `epochs_s[e]` bit for bit; `ftot[e, f]` is the
        nansum of that map over the pixels, summed on the device in a fixed order -- with
        `want_maps=False` (light curves) no map touches memory.  The burst factor is evaluated
        once per (cell, epoch) whatever the number of channels.  Epochs in any order; `ctau`,
        `csrc` as for `ff_formal`; any layout of `fields`; no cached state is read or written."""
        E, F = len(epochs_s), len(ctau)
        if len(csrc) != F:
            raise ValueError("ff_formal_sweep: ctau and csrc must have one entry per channel")
        if not (want_maps or want_totals):
            raise ValueError("ff_formal_sweep: neither maps nor totals asked for")
        nx, ny, nz = fields.shape
        maps = self._f64(E, F, fields.npix) if want_maps else None
        ftot = self._f64(E, F) if want_totals else None
        work = None
        if want_totals:
            work = self._workspace(max(1, self.lib.rjp_ff_formal_sweep_workspace(nx, ny, nz, E, F)))
        fs = fields.struct()
        self._call("rjp_ff_formal_sweep", C.byref(fs), _ref(bursts), _lib.dbl_array(epochs_s), E,
                   int(gff_mode), _lib.dbl_array(ctau), _lib.dbl_array(csrc), F, _ptr(maps),
                   _ptr(ftot), _ptr(work), work.numel() if work is not None else 0)
        return maps, ftot

    def ff_grad(self, fields, bursts, epochs_s, gff_mode, tavg=None, ctau=None, cflux=None,
                want_maps=False):
        """Sensitivities to the burst parameters (rjp_ff_grad): one pass over (a0, ts) per tile of
        epochs gives S = sum_y |a0| chi^2 and its derivatives with respect to (t0, amp_rel, inv2s2)
        of every burst -- parameter k = 3 b + c, b counting the red jet's bursts first, then the
        blue jet's, as `make_bursts` lists them.
        -> (sumA[E, P], dsumA[E, n_par, P] | None, ftot[E, F] | None, dftot[E, F, n_par] | None)
        device tensors (float64): `dsumA` only with `want_maps`, the light curves `ftot` and their
        Jacobian `dftot` only with the channel coefficients (`tavg`, `ctau`, `cflux` as for
        `ff_maps`).  Needs the tau layout built for `gff_mode`, at least one burst and at most 8
        per jet; `fields.ts` is read as it is (the call applies the rule for a jet without bursts
        itself)."""
        E, P = len(epochs_s), fields.npix
        nx, ny, nz = fields.shape
        n_par = 3 * (int(bursts.n[0]) + int(bursts.n[1])) if bursts is not None else 0
        totals = ctau is not None
        if totals and (tavg is None or cflux is None or len(cflux) != len(ctau)):
            raise ValueError("the light-curve Jacobian needs tavg, ctau and cflux (same length)")
        F = len(ctau) if totals else 0
        sumA = self._f64(E, P)
        dsumA = self._f64(E, n_par, P) if want_maps else None
        ftot = self._f64(E, F) if totals else None
        dftot = self._f64(E, F, n_par) if totals else None
        work = self._workspace(max(1, self.lib.rjp_ff_grad_workspace(nx, ny, nz, E, n_par, F)))
        fs = fields.struct()
        self._call("rjp_ff_grad", C.byref(fs), _ref(bursts), _lib.dbl_array(epochs_s), E,
                   int(gff_mode), _ptr(tavg), _lib.dbl_array(ctau) if totals else None,
                   _lib.dbl_array(cflux) if totals else None, F, _ptr(sumA), _ptr(dsumA),
                   _ptr(ftot), _ptr(dftot), work.data_ptr(), work.numel())
        return sumA, dsumA, ftot, dftot

    def ff_formal_grad(self, fields, bursts, epochs_s, gff_mode, ctau, csrc, want_maps=False):
        """Sensitivities of the formal-solution light curves to the burst parameters
        (rjp_ff_formal_grad): ONE walk of the fields for all of `epochs_s` [s] gives the totals of
        `ff_formal_sweep` (bit for bit) and their exact derivatives with respect to (t0, amp_rel,
        inv2s2) of every burst -- parameter k = 3 b + c as in `ff_grad`.
        -> (ftot[E, F], dftot[E, F, n_par], dmaps[E, F, n_par, P] | None) device tensors (float64);
        `dmaps` (csrc[f] dI/dtheta_k per pixel, NaN where `ff_formal`'s map is) only with
        `want_maps`.  Any f64 layout of `fields`; at least one burst, at most 8 per jet;
        `fields.ts` is read as it is.  `ctau`, `csrc` as for `ff_formal`."""
        E, F = len(epochs_s), len(ctau)
        if len(csrc) != F:
            raise ValueError("ff_formal_grad: ctau and csrc must have one entry per channel")
        nx, ny, nz = fields.shape
        n_par = 3 * (int(bursts.n[0]) + int(bursts.n[1])) if bursts is not None else 0
        ftot = self._f64(E, F)
        dftot = self._f64(E, F, n_par)
        dmaps = self._f64(E, F, n_par, fields.npix) if want_maps else None
        work = self._workspace(max(1, self.lib.rjp_ff_formal_grad_workspace(nx, ny, nz, E, n_par, F)))
        fs = fields.struct()
        self._call("rjp_ff_formal_grad", C.byref(fs), _ref(bursts), _lib.dbl_array(epochs_s), E,
                   int(gff_mode), _lib.dbl_array(ctau), _lib.dbl_array(csrc), F, _ptr(ftot),
                   _ptr(dftot), _ptr(dmaps), work.data_ptr(), work.numel())
        return ftot, dftot, dmaps

    # -- K10 -----------------------------------------------------------------------------------
    def _device_f64(self, values):
        """Host array or tensor -> contiguous float64 vector on this engine's device."""
        torch = _torch()
        if not isinstance(values, torch.Tensor):
            values = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64).reshape(-1))
        return values.to(device=self.device, dtype=torch.float64).reshape(-1).contiguous()

    def _call_tiles(self, name, *args):
        """`_call` for the entry points that return their tile count (> 0) or a status (<= 0)."""
        tiles = getattr(self.lib, name)(self.ctx, *args, self._stream())
        if tiles <= 0:
            self._check(int(tiles), self.ctx, name)
        return int(tiles)

    def _vis_stack(self, who, vis):
        """A stack of visibility sets, complex128 [M, K] or float64 [M, K, 2] -> the latter."""
        torch = _torch()
        if isinstance(vis, torch.Tensor) and vis.dtype == torch.complex128:
            vis = torch.view_as_real(vis)
        if not (isinstance(vis, torch.Tensor) and vis.dtype == torch.float64 and
                vis.device == self.device and vis.is_contiguous() and vis.dim() == 3 and
                vis.shape[2] == 2 and vis.shape[0] >= 1 and vis.shape[1] >= 1):
            raise ValueError("%s: `vis` must be a contiguous complex128 [M, K] or float64 "
                             "[M, K, 2] tensor on %s" % (who, self.device))
        return vis

    @staticmethod
    def _map_scales(who, su, sv, M=None):
        """`su`, `sv` as host float64 vectors with one entry per map (M None: as many as given)."""
        su, sv = (np.ascontiguousarray(s, dtype=np.float64).reshape(-1) for s in (su, sv))
        if M is None and (su.size < 1 or sv.size != su.size):
            raise ValueError("%s: su and sv must have the same length >= 1" % who)
        if M is not None and (su.size != M or sv.size != M):
            raise ValueError("%s: su and sv must have one entry per map (%d)" % (who, M))
        return su, sv

    def _device_mask(self, who, mask, npix):
        """None, or `mask` (host array or tensor, non-zero = set) as uint8 [npix] on the device."""
        if mask is None:
            return None
        torch = _torch()
        if not isinstance(mask, torch.Tensor):
            mask = torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0))
        dmask = (mask != 0).to(device=self.device, dtype=torch.uint8).reshape(-1).contiguous()
        if dmask.numel() != npix:
            raise ValueError("%s: `mask` must have nx * nz entries" % who)
        return dmask

    def vis(self, maps, nx, nz, su, sv, u, v):
        """Model visibilities of a stack of maps (rjp_vis): the direct Fourier sum
        V[m, k] = sum_{ix, iz} maps[m, ix nz + iz] exp(-2 pi i (su[m] u[k] (ix - (nx-1)/2) +
        sv[m] v[k] (iz - (nz-1)/2))) -> complex128 device tensor [n_maps, n_vis].
        `maps`: float64 device tensor of n_maps * nx * nz values in the library's pixel order (any
        flux stack of this engine, or the derivative maps of `ff_formal_grad`); NaN pixels add
        nothing.  `su`, `sv` [n_maps]: cycles per cell per unit of `u`, `v` (`vis_scales` builds
        them for baselines in metres); `u`, `v` [n_vis]: host arrays or device tensors.  Sums in a
        fixed order: a repeated call gives the same bits."""
        torch = _torch()
        nx, nz = int(nx), int(nz)
        if not (isinstance(maps, torch.Tensor) and maps.dtype == torch.float64 and
                maps.device == self.device and maps.is_contiguous()):
            raise ValueError("vis: `maps` must be a contiguous float64 tensor on %s" % self.device)
        if nx < 1 or nz < 1 or maps.numel() == 0 or maps.numel() % (nx * nz):
            raise ValueError("vis: `maps` must hold a whole number (>= 1) of nx * nz maps")
        M = maps.numel() // (nx * nz)
        su, sv = self._map_scales("vis", su, sv, M)
        du, dv = self._device_f64(u), self._device_f64(v)
        K = du.numel()
        if K < 1 or dv.numel() != K:
            raise ValueError("vis: u and v must have the same length >= 1")
        out = self._f64(M, K, 2)
        work = self._workspace(max(1, self.lib.rjp_vis_workspace(M, nx, nz, K)))
        self._call("rjp_vis", maps.data_ptr(), M, nx, nz, _lib.dbl_array(su), _lib.dbl_array(sv),
                   du.data_ptr(), dv.data_ptr(), K, out.data_ptr(), work.data_ptr(), work.numel())
        return torch.view_as_complex(out)

    # -- K11 -----------------------------------------------------------------------------------
    def vis_adjoint(self, vis, nx, nz, su, sv, u, v, w=None):
        """Dirty images of a stack of visibility sets (rjp_vis_adjoint), the real transpose of
        `vis`: D[m, ix nz + iz] = sum_k w[k] Re(vis[m, k] exp(+2 pi i (su[m] u[k] (ix - (nx-1)/2) +
        sv[m] v[k] (iz - (nz-1)/2)))) -> float64 device tensor [n_maps, nx * nz], NOT normalised.
        `vis`: complex128 [n_maps, n_vis] or float64 [n_maps, n_vis, 2] device tensor (what `vis`
        returns); `nx`, `nz`, `su`, `sv` describe the OUTPUT grid (`image_scales` builds the scales
        of any cell size for baselines in metres); `u`, `v`, `w` [n_vis]: host arrays or device
        tensors, `w` None = all ones.  A visibility with a non-finite value, weight or baseline
        adds nothing.  Sums in a fixed order: a repeated call gives the same bits.  The number of
        tiles the call enqueued is kept in `last_vis_adjoint_tiles`."""
        nx, nz = int(nx), int(nz)
        vis = self._vis_stack("vis_adjoint", vis)
        if nx < 1 or nz < 1:
            raise ValueError("vis_adjoint: nx and nz must be positive")
        M, K = int(vis.shape[0]), int(vis.shape[1])
        su, sv = self._map_scales("vis_adjoint", su, sv, M)
        du, dv = self._device_f64(u), self._device_f64(v)
        dw = self._device_f64(w) if w is not None else None
        if du.numel() != K or dv.numel() != K or (dw is not None and dw.numel() != K):
            raise ValueError("vis_adjoint: u, v and w must have one entry per visibility (%d)" % K)
        out = self._f64(M, nx * nz)
        work = self._workspace(max(1, self.lib.rjp_vis_adjoint_workspace(M, nx, nz, K)))
        self.last_vis_adjoint_tiles = self._call_tiles(
            "rjp_vis_adjoint", vis.data_ptr(), M, K, _lib.dbl_array(su), _lib.dbl_array(sv),
            du.data_ptr(), dv.data_ptr(), _ptr(dw), nx, nz, out.data_ptr(), work.data_ptr(),
            work.numel())
        return out

    # -- K12 / K13 -----------------------------------------------------------------------------
    def _stack_f64(self, who, name, t, n):
        """`t` is a contiguous float64 tensor of `n` values on this engine's device."""
        torch = _torch()
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and
                t.device == self.device and t.is_contiguous() and t.numel() == n):
            raise ValueError("%s: `%s` must be a contiguous float64 tensor of %d values on %s"
                             % (who, name, n, self.device))

    def clean(self, res, nx, nz, psf, px, pz, n_iter, gain, thresh, mask=None, model=None):
        """Hogbom CLEAN minor cycles on a stack of dirty images (rjp_clean), one fused launch per
        iteration for the whole stack, nothing going to the host -> (cpix[M, n_iter] int32,
        cflux[M, n_iter] float64, ncomp[M] int32, peak[M] float64) device tensors; slots at and
        beyond ncomp[m] are not written.  `res`: float64 device tensor of M * nx * nz values, the
        dirty images on entry and the residuals on exit (IN PLACE).  `psf`: M beams or one shared
        beam of px * pz values, px and pz odd (2 nx - 1, 2 nz - 1: full Hogbom; smaller: the
        subtraction is windowed), used as given.  `thresh`: one number or one per map [the unit of
        `res`]; `mask`: None or nx * nz values, non-zero = may hold a component; `model`: a
        float64 tensor like `res` that every component's flux is ADDED to.  Per iteration and map:
        the unmasked finite pixel of largest |R| (lowest index on a tie); stop at |R| <= thresh;
        else f = gain R, R -= f B shifted to the pixel.  A second call on `res` continues the
        clean.  The same bits on every call.  The number of workgroups per iteration is kept in
        `last_clean_tiles`."""
        torch = _torch()
        nx, nz, px, pz, n_iter = int(nx), int(nz), int(px), int(pz), int(n_iter)
        if nx < 1 or nz < 1 or px < 1 or pz < 1 or n_iter < 1:
            raise ValueError("clean: nx, nz, px, pz and n_iter must be positive")
        if not (isinstance(res, torch.Tensor) and res.numel() >= nx * nz and
                res.numel() % (nx * nz) == 0):
            raise ValueError("clean: `res` must hold a whole number (>= 1) of nx * nz images")
        M = res.numel() // (nx * nz)
        self._stack_f64("clean", "res", res, M * nx * nz)
        if not (isinstance(psf, torch.Tensor) and psf.numel() in (px * pz, M * px * pz)):
            raise ValueError("clean: `psf` must hold one beam or one per map of px * pz values")
        n_psf = psf.numel() // (px * pz)
        self._stack_f64("clean", "psf", psf, n_psf * px * pz)
        if model is not None:
            self._stack_f64("clean", "model", model, M * nx * nz)
        dmask = self._device_mask("clean", mask, nx * nz)
        th = np.asarray(thresh, dtype=np.float64).reshape(-1)
        if th.size not in (1, M):
            raise ValueError("clean: `thresh` must be one number or one per map (%d)" % M)
        th = np.ascontiguousarray(np.broadcast_to(th, (M,)))
        cpix = torch.empty(M, n_iter, dtype=torch.int32, device=self.device)
        cflux = self._f64(M, n_iter)
        ncomp = torch.empty(M, dtype=torch.int32, device=self.device)
        peak = self._f64(M)
        work = self._workspace(max(1, self.lib.rjp_clean_workspace(M, nx, nz)))
        self.last_clean_tiles = self._call_tiles(
            "rjp_clean", res.data_ptr(), M, nx, nz, psf.data_ptr(), n_psf, px, pz, _ptr(dmask),
            _lib.dbl_array(th), float(gain), n_iter, cpix.data_ptr(), cflux.data_ptr(),
            ncomp.data_ptr(), _ptr(model), peak.data_ptr(), work.data_ptr(), work.numel())
        return cpix, cflux, ncomp, peak

    def restore(self, cpix, cflux, ncomp, beam_abc, nx, nz, add=None):
        """Clean components convolved with the clean beam, plus `add` (rjp_restore):
        out[m, q] = add[m, q] + sum_{c < ncomp[m]} cflux[m, c] exp(-(A dx^2 + 2 B dx dz + C dz^2))
        -> float64 device tensor [M, nx * nz].  `cpix`, `cflux` [M, stride], `ncomp` [M]: what
        `clean` returns; `beam_abc`: (A, B, C) in cells^-2, one triple or one per map
        (`beam_quadratic`); `add`: the residuals [M, nx * nz] or None.  Sum in list order, the
        same bits on every call."""
        torch = _torch()
        nx, nz = int(nx), int(nz)
        if nx < 1 or nz < 1:
            raise ValueError("restore: nx and nz must be positive")
        ok = lambda t, dt: (isinstance(t, torch.Tensor) and t.dtype == dt and
                            t.device == self.device and t.is_contiguous())
        if not (ok(cpix, torch.int32) and ok(cflux, torch.float64) and ok(ncomp, torch.int32) and
                cpix.dim() == 2 and cpix.shape == cflux.shape and cpix.shape[1] >= 1 and
                ncomp.numel() == cpix.shape[0] >= 1):
            raise ValueError("restore: cpix [M, S] int32, cflux [M, S] float64 and ncomp [M] int32 "
                             "must be contiguous tensors on %s" % self.device)
        M, S = int(cpix.shape[0]), int(cpix.shape[1])
        abc = np.asarray(beam_abc, dtype=np.float64).reshape(-1, 3)
        if abc.shape[0] == 1:
            abc = np.repeat(abc, M, axis=0)
        if abc.shape[0] != M:
            raise ValueError("restore: `beam_abc` must be one (A, B, C) or one per map (%d)" % M)
        if add is not None:
            self._stack_f64("restore", "add", add, M * nx * nz)
        out = self._f64(M, nx * nz)
        self._call_tiles("rjp_restore", cpix.data_ptr(), cflux.data_ptr(), ncomp.data_ptr(), M, S,
                         _lib.dbl_array(abc), _ptr(add), nx, nz, out.data_ptr())
        return out

    # -- convolution / K17 -----------------------------------------------------------------------
    def convolve2d(self, inp, nx, nz, ker, kx, kz, add=None):
        """A direct 2-D convolution of a stack of images (rjp_convolve2d):
        out[m][i, j] = add[m][i, j] + sum_{a, b} ker[a, b] inp[m][i - (a - ca), j - (b - cb)],
        the centre (ca, cb) = ((kx - 1) / 2, (kz - 1) / 2), `inp` zero outside the image -> a new
        float64 device tensor [M, nx * nz].  `inp`: float64 device tensor of M * nx * nz values;
        `ker`: one kernel or one per map of kx * kz values, kx and kz odd; `add`: a tensor like
        `inp` or None.  f64, one fma per term in kernel order: the same bits on every call.
        Nothing goes to the host.  The workgroup count is kept in `last_convolve2d_workgroups`."""
        torch = _torch()
        nx, nz, kx, kz = int(nx), int(nz), int(kx), int(kz)
        if nx < 1 or nz < 1 or kx < 1 or kz < 1:
            raise ValueError("convolve2d: nx, nz, kx and kz must be positive")
        if not (isinstance(inp, torch.Tensor) and inp.numel() >= nx * nz and
                inp.numel() % (nx * nz) == 0):
            raise ValueError("convolve2d: `inp` must hold a whole number (>= 1) of nx * nz images")
        M = inp.numel() // (nx * nz)
        self._stack_f64("convolve2d", "inp", inp, M * nx * nz)
        if not (isinstance(ker, torch.Tensor) and ker.numel() in (kx * kz, M * kx * kz)):
            raise ValueError("convolve2d: `ker` must hold one kernel or one per map of kx * kz "
                             "values")
        n_ker = ker.numel() // (kx * kz)
        self._stack_f64("convolve2d", "ker", ker, n_ker * kx * kz)
        if add is not None:
            self._stack_f64("convolve2d", "add", add, M * nx * nz)
        out = self._f64(M, nx * nz)
        self.last_convolve2d_workgroups = self._call_tiles(
            "rjp_convolve2d", inp.data_ptr(), M, nx, nz, ker.data_ptr(), n_ker, kx, kz, _ptr(add),
            out.data_ptr())
        return out

    def msclean(self, res, n_s, nx, nz, xpsf, px, pz, weight, n_iter, gain, thresh, mask=None,
                model=None):
        """Multi-scale CLEAN minor cycles on a stack of maps of `n_s` planes each (rjp_msclean),
        one fused launch per iteration for the whole stack, nothing going to the host -> (cpix
        [M, n_iter] int32, cscale [M, n_iter] int32, cflux [M, n_iter] float64, ncomp [M] int32,
        peak [M] float64) device tensors; slots at and beyond ncomp[m] are not written.  `res`:
        float64 device tensor of M * n_s * nx * nz values, the dirty image convolved with each
        scale on entry and the residual planes on exit (IN PLACE).  `xpsf`: the cross beams
        X[k][l], k <= l, as a packed upper triangle of n_s (n_s + 1) / 2 planes of px * pz values
        (odd), one set or one per map.  `weight`: host, [n_s] or [M, n_s], finite and >= 0 (0: the
        plane is updated, never picked).  `thresh`, `mask` as `clean`; `model`: a tensor like `res`
        that every component's flux is ADDED to, in the plane of its scale.  Per iteration and
        map: the largest weight[k] |R_k[p]| (lower k, then lower p on a tie); stop at <= thresh;
        else f = gain R_k[p] / X[k][k][centre] and R_l -= f X[k][l] shifted to p, for every l.
        The same bits on every call.  The number of workgroups per iteration is kept in
        `last_msclean_workgroups`."""
        torch = _torch()
        n_s, nx, nz, px, pz, n_iter = int(n_s), int(nx), int(nz), int(px), int(pz), int(n_iter)
        if n_s < 1 or nx < 1 or nz < 1 or px < 1 or pz < 1 or n_iter < 1:
            raise ValueError("msclean: n_s, nx, nz, px, pz and n_iter must be positive")
        per = n_s * nx * nz
        if not (isinstance(res, torch.Tensor) and res.numel() >= per and res.numel() % per == 0):
            raise ValueError("msclean: `res` must hold a whole number (>= 1) of n_s * nx * nz maps")
        M = res.numel() // per
        self._stack_f64("msclean", "res", res, M * per)
        tri = n_s * (n_s + 1) // 2 * px * pz
        if not (isinstance(xpsf, torch.Tensor) and xpsf.numel() in (tri, M * tri)):
            raise ValueError("msclean: `xpsf` must hold one set of n_s (n_s + 1) / 2 cross beams of "
                             "px * pz values, or one per map")
        n_psf = xpsf.numel() // tri
        self._stack_f64("msclean", "xpsf", xpsf, n_psf * tri)
        if model is not None:
            self._stack_f64("msclean", "model", model, M * per)
        dmask = self._device_mask("msclean", mask, nx * nz)
        w = np.asarray(weight, dtype=np.float64)
        if w.size not in (n_s, M * n_s):
            raise ValueError("msclean: `weight` must be one per plane (%d) or one per map and "
                             "plane" % n_s)
        w = np.ascontiguousarray(np.broadcast_to(w.reshape(-1, n_s), (M, n_s)))
        th = np.asarray(thresh, dtype=np.float64).reshape(-1)
        if th.size not in (1, M):
            raise ValueError("msclean: `thresh` must be one number or one per map (%d)" % M)
        th = np.ascontiguousarray(np.broadcast_to(th, (M,)))
        cpix = torch.empty(M, n_iter, dtype=torch.int32, device=self.device)
        cscale = torch.empty(M, n_iter, dtype=torch.int32, device=self.device)
        cflux = self._f64(M, n_iter)
        ncomp = torch.empty(M, dtype=torch.int32, device=self.device)
        peak = self._f64(M)
        work = self._workspace(max(1, self.lib.rjp_msclean_workspace(M, n_s, nx, nz)))
        self.last_msclean_workgroups = self._call_tiles(
            "rjp_msclean", res.data_ptr(), M, n_s, nx, nz, xpsf.data_ptr(), n_psf, px, pz,
            _lib.dbl_array(w), _ptr(dmask), _lib.dbl_array(th), float(gain), n_iter,
            cpix.data_ptr(), cscale.data_ptr(), cflux.data_ptr(), ncomp.data_ptr(), _ptr(model),
            peak.data_ptr(), work.data_ptr(), work.numel())
        return cpix, cscale, cflux, ncomp, peak

    def mtmfs(self, res, n_t, nx, nz, spsf, px, pz, hinv, n_iter, gain, thresh, mask=None,
              model=None):
        """Multi-term MFS CLEAN minor cycles on a stack of maps of `n_t` Taylor planes each
        (rjp_mtmfs), one fused launch per iteration for the whole stack, nothing going to the host
        -> (cpix [M, n_iter] int32, ccoef [M, n_iter, n_t] float64, ncomp [M] int32, peak [M]
        float64) device tensors; slots at and beyond ncomp[m] are not written.  `res`: float64
        device tensor of M * n_t * nx * nz values, the Taylor residual planes, updated IN PLACE.
        `spsf`: the spectral beams B_0 .. B_{2 n_t - 2} of px * pz values (odd), one set or one per
        map.  `hinv`: host, [n_t, n_t] or [M, n_t, n_t], the inverse of H[t][q] = B_{t+q}(centre)
        (`taylor_hessian_inverse`), every entry finite.  `thresh`, `mask` as `clean`; `model`: a
        tensor like `res` that every component's coefficients are ADDED to, term by term.  Per
        iteration and map: a_q = sum_t hinv[q][t] R_t[p]; the largest |a_0| (lower p on a tie);
        stop at <= thresh; else c_q = gain a_q and R_t -= sum_q c_q B_{t+q} shifted to p, for every
        t.  `peak`: the final max |a_0|.  The same bits on every call.  The number of workgroups
        per iteration is kept in `last_mtmfs_workgroups`."""
        torch = _torch()
        n_t, nx, nz, px, pz, n_iter = int(n_t), int(nx), int(nz), int(px), int(pz), int(n_iter)
        if n_t < 1 or nx < 1 or nz < 1 or px < 1 or pz < 1 or n_iter < 1:
            raise ValueError("mtmfs: n_t, nx, nz, px, pz and n_iter must be positive")
        per = n_t * nx * nz
        if not (isinstance(res, torch.Tensor) and res.numel() >= per and res.numel() % per == 0):
            raise ValueError("mtmfs: `res` must hold a whole number (>= 1) of n_t * nx * nz maps")
        M = res.numel() // per
        self._stack_f64("mtmfs", "res", res, M * per)
        nb = (2 * n_t - 1) * px * pz
        if not (isinstance(spsf, torch.Tensor) and spsf.numel() in (nb, M * nb)):
            raise ValueError("mtmfs: `spsf` must hold one set of 2 n_t - 1 spectral beams of "
                             "px * pz values, or one per map")
        n_psf = spsf.numel() // nb
        self._stack_f64("mtmfs", "spsf", spsf, n_psf * nb)
        if model is not None:
            self._stack_f64("mtmfs", "model", model, M * per)
        dmask = self._device_mask("mtmfs", mask, nx * nz)
        h = np.asarray(hinv, dtype=np.float64)
        if h.size not in (n_t * n_t, M * n_t * n_t):
            raise ValueError("mtmfs: `hinv` must be [n_t, n_t] = [%d, %d] or one per map"
                             % (n_t, n_t))
        h = np.ascontiguousarray(np.broadcast_to(h.reshape(-1, n_t, n_t), (M, n_t, n_t)))
        th = np.asarray(thresh, dtype=np.float64).reshape(-1)
        if th.size not in (1, M):
            raise ValueError("mtmfs: `thresh` must be one number or one per map (%d)" % M)
        th = np.ascontiguousarray(np.broadcast_to(th, (M,)))
        cpix = torch.empty(M, n_iter, dtype=torch.int32, device=self.device)
        ccoef = self._f64(M, n_iter, n_t)
        ncomp = torch.empty(M, dtype=torch.int32, device=self.device)
        peak = self._f64(M)
        work = self._workspace(max(1, self.lib.rjp_mtmfs_workspace(M, n_t, nx, nz)))
        self.last_mtmfs_workgroups = self._call_tiles(
            "rjp_mtmfs", res.data_ptr(), M, n_t, nx, nz, spsf.data_ptr(), n_psf, px, pz,
            _lib.dbl_array(h), _ptr(dmask), _lib.dbl_array(th), float(gain), n_iter,
            cpix.data_ptr(), ccoef.data_ptr(), ncomp.data_ptr(), _ptr(model), peak.data_ptr(),
            work.data_ptr(), work.numel())
        return cpix, ccoef, ncomp, peak

    # -- K18 -------------------------------------------------------------------------------------
    def _component_list(self, who, cpix, cflux, ncomp, cscale):
        """The component tensors of `clean` / `msclean` ([M, S] int32 / float64, [M] int32, and
        None or [M, S] int32 scales) checked -> (M, S)."""
        torch = _torch()
        ok = lambda t, dt: (isinstance(t, torch.Tensor) and t.dtype == dt and
                            t.device == self.device and t.is_contiguous())
        if not (ok(cpix, torch.int32) and ok(cflux, torch.float64) and ok(ncomp, torch.int32) and
                cpix.dim() == 2 and cpix.shape == cflux.shape and cpix.shape[1] >= 1 and
                ncomp.numel() == cpix.shape[0] >= 1 and
                (cscale is None or (ok(cscale, torch.int32) and cscale.shape == cpix.shape))):
            raise ValueError("%s: cpix [M, S] int32, cflux [M, S] float64, ncomp [M] int32 (and "
                             "cscale [M, S] int32) must be contiguous tensors on %s"
                             % (who, self.device))
        return int(cpix.shape[0]), int(cpix.shape[1])

    def vis_components(self, cpix, cflux, ncomp, nx, nz, su, sv, u, v, cscale=None, n_s=1,
                       gvis=None, vis_in=None, sign=1, out=None):
        """The visibilities of a list of clean components, added to (`sign` +1) or taken from
        (-1) `vis_in` (rjp_vis_components): out[m, k] = vis_in[m, k] + sign sum_s gvis[m, s, k]
        sum_{c < ncomp[m], cscale[m, c] = s} cflux[m, c] exp(-2 pi i (su[m] u[k] (ix_c - (nx-1)/2) +
        sv[m] v[k] (iz_c - (nz-1)/2))) -> complex128 device tensor [M, K].  `cpix`, `cflux`
        [M, S], `ncomp` [M]: what `clean` / `msclean` return (pixel = ix nz + iz); `cscale` [M, S]
        with `n_s` scales, None = all of scale 0; `gvis`: complex128 [M, n_s, K] (or float64
        [M, n_s, K, 2]), the transform of each scale's kernel at each visibility, None = 1 (needs
        n_s = 1); `vis_in`: complex128 [M, K] or None = 0; `out`: None or a tensor like `vis_in`
        (may be `vis_in` itself); `su`, `sv`, `u`, `v` as `vis`.  n_comp x n_vis phasors, formed
        as `vis` forms its own; sums in a fixed order: a repeated call gives the same bits.  Nothing
        goes to the host.  The workgroup count is kept in `last_vis_components_workgroups`."""
        torch = _torch()
        nx, nz, n_s, sign = int(nx), int(nz), int(n_s), int(sign)
        M, S = self._component_list("vis_components", cpix, cflux, ncomp, cscale)
        if nx < 1 or nz < 1 or n_s < 1:
            raise ValueError("vis_components: nx, nz and n_s must be positive")
        su, sv = self._map_scales("vis_components", su, sv, M)
        du, dv = self._device_f64(u), self._device_f64(v)
        K = du.numel()
        if K < 1 or dv.numel() != K:
            raise ValueError("vis_components: u and v must have the same length >= 1")
        if gvis is not None:
            if isinstance(gvis, torch.Tensor) and gvis.dtype == torch.complex128:
                gvis = torch.view_as_real(gvis)
            self._stack_f64("vis_components", "gvis", gvis, M * n_s * K * 2)
        vin = None
        if vis_in is not None:
            vin = self._vis_stack("vis_components", vis_in)
            if tuple(vin.shape) != (M, K, 2):
                raise ValueError("vis_components: `vis_in` must be [M, K] = [%d, %d]" % (M, K))
        if out is None:
            vout = self._f64(M, K, 2)
        else:
            vout = self._vis_stack("vis_components", out)
            if tuple(vout.shape) != (M, K, 2):
                raise ValueError("vis_components: `out` must be [M, K] = [%d, %d]" % (M, K))
        self.last_vis_components_workgroups = self._call_tiles(
            "rjp_vis_components", cpix.data_ptr(), _ptr(cscale), cflux.data_ptr(),
            ncomp.data_ptr(), M, S, n_s, nx, nz, _lib.dbl_array(su), _lib.dbl_array(sv),
            du.data_ptr(), dv.data_ptr(), K, _ptr(gvis), _ptr(vin), sign, vout.data_ptr())
        return torch.view_as_complex(vout)

    def components_image(self, cpix, cflux, ncomp, nx, nz, cscale=None, n_s=1):
        """The delta model image of a component list (rjp_components_image): out[m, s, q] = the
        sum, in list order from +0.0, of the fluxes of map m's components at pixel q with scale s
        -> float64 device tensor [M, n_s, nx * nz].  Arguments as `vis_components`.  A function of
        the list alone, no atomics: bit for bit what `clean` / `msclean` add into a zeroed
        `model`.  Nothing goes to the host."""
        nx, nz, n_s = int(nx), int(nz), int(n_s)
        M, S = self._component_list("components_image", cpix, cflux, ncomp, cscale)
        if nx < 1 or nz < 1 or n_s < 1:
            raise ValueError("components_image: nx, nz and n_s must be positive")
        out = self._f64(M, n_s, nx * nz)
        self._call_tiles("rjp_components_image", cpix.data_ptr(), _ptr(cscale), cflux.data_ptr(),
                         ncomp.data_ptr(), M, S, n_s, nx, nz, out.data_ptr())
        return out

    # -- K14 -------------------------------------------------------------------------------------
    def gaussfit(self, img, nx, nz, theta0, box=None, mask=None, n_iter=60, lambda0=1e-3,
                 xtol=1e-12, trace=False):
        """Levenberg-Marquardt fits of one elliptical Gaussian per map (rjp_gaussfit), one fused
        launch per iteration for the whole stack, nothing going to the host -> dict of device
        tensors: `theta` [M, 6] = (S, x0, z0, A, B, C) of S exp(-(A dx^2 + 2 B dx dz + C dz^2)),
        dx = ix - x0, dz = iz - z0 (the form of `beam_quadratic`, cells^-2), `chi2` [M], `cov`
        [M, 21] (the packed upper triangle of J^T J at `theta`, NOT inverted: `gauss_results`),
        `npix`, `niter`, `status` [M] int32 -- 1 converged, 0 `n_iter` exhausted, 2 stalled
        (lambda > 1e12), 3 degenerate (start not finite and positive definite, or fewer than 6
        counting pixels: `theta` keeps the start, the other outputs of that map are NaN / -1) --
        and with `trace` the rows [M, n_iter, 9] of (chi^2 of the trial, lambda, accepted, the
        trial), NaN beyond `niter`.  `img`: float64 device tensor of M * nx * nz values (read
        only); `theta0`: [M, 6] or one start for all (`gauss_start`); `box`: (i0, i1, j0, j1),
        inclusive, None = the whole image; `mask`: None or nx * nz values, non-zero = the pixel
        counts.  Non-finite pixels are skipped.  The same bits on every call.  The number of
        workgroups per iteration is kept in `last_gaussfit_tiles`."""
        torch = _torch()
        nx, nz, n_iter = int(nx), int(nz), int(n_iter)
        if nx < 1 or nz < 1 or n_iter < 1:
            raise ValueError("gaussfit: nx, nz and n_iter must be positive")
        if not (isinstance(img, torch.Tensor) and img.numel() >= nx * nz and
                img.numel() % (nx * nz) == 0):
            raise ValueError("gaussfit: `img` must hold a whole number (>= 1) of nx * nz images")
        M = img.numel() // (nx * nz)
        self._stack_f64("gaussfit", "img", img, M * nx * nz)
        b = (0, nx - 1, 0, nz - 1) if box is None else tuple(int(x) for x in np.ravel(box))
        if len(b) != 4 or not (0 <= b[0] <= b[1] < nx and 0 <= b[2] <= b[3] < nz):
            raise ValueError("gaussfit: the box (i0, i1, j0, j1) must lie inside the image")
        if not (np.isfinite(lambda0) and lambda0 > 0. and np.isfinite(xtol) and xtol > 0.):
            raise ValueError("gaussfit: `lambda0` and `xtol` must be finite and positive")
        dmask = self._device_mask("gaussfit", mask, nx * nz)
        if isinstance(theta0, torch.Tensor):
            theta = theta0.to(device=self.device, dtype=torch.float64).reshape(-1, 6)
        else:
            theta = torch.from_numpy(np.ascontiguousarray(theta0, dtype=np.float64)
                                     .reshape(-1, 6)).to(self.device)
        if theta.shape[0] == 1:
            theta = theta.expand(M, 6)
        if theta.shape[0] != M:
            raise ValueError("gaussfit: `theta0` must be one start (6 values) or one per map (%d)" % M)
        theta = theta.contiguous().clone()
        chi2 = torch.full((M,), float("nan"), dtype=torch.float64, device=self.device)
        cov = torch.full((M, 21), float("nan"), dtype=torch.float64, device=self.device)
        npix, niter, status = (torch.full((M,), -1, dtype=torch.int32, device=self.device)
                               for _ in range(3))
        tr = (torch.full((M, n_iter, 9), float("nan"), dtype=torch.float64, device=self.device)
              if trace else None)
        nbox = (b[1] - b[0] + 1) * (b[3] - b[2] + 1)
        work = self._workspace(max(1, self.lib.rjp_gaussfit_workspace(M, nbox)))
        self.last_gaussfit_tiles = self._call_tiles(
            "rjp_gaussfit", img.data_ptr(), M, nx, nz, (C.c_int32 * 4)(*b), _ptr(dmask),
            theta.data_ptr(), float(lambda0), float(xtol), n_iter, chi2.data_ptr(), cov.data_ptr(),
            npix.data_ptr(), niter.data_ptr(), status.data_ptr(), _ptr(tr), work.data_ptr(),
            work.numel())
        out = dict(theta=theta, chi2=chi2, cov=cov, npix=npix, niter=niter, status=status)
        if trace:
            out["trace"] = tr
        return out

    # -- K20 -------------------------------------------------------------------------------------
    def uvfit(self, vis, su, sv, u, v, theta0, weights=None, free=None, n_iter=60, lambda0=1e-3,
              xtol=1e-10, trace=False):
        """Levenberg-Marquardt fits of point / elliptical-Gaussian components to a stack of
        visibility sets (rjp_uvfit), one fused launch per iteration for the whole stack, nothing
        going to the host -> dict of device tensors: `theta` [M, P], P = 6 n_comp, per component
        (F, x, z, sxx, sxz, szz) of F exp(-2 pi^2 (sxx a^2 + 2 sxz a b + szz b^2)) exp(-2 pi i (a x +
        b z)), a = su[m] u[k], b = sv[m] v[k] in cycles per cell (flux, offset from the phase centre
        in cells, covariance in cells^2: `uvfit_theta`); `chi2` [M]; `cov` [M, P (P + 1) / 2] (the
        packed upper triangle of Re(J^H W J) at `theta`, identity rows for fixed parameters, NOT
        inverted: `uvfit_results`); `nvis`, `niter`, `status` [M] int32 -- 1 converged, 0 `n_iter`
        exhausted, 2 stalled (lambda > 1e12), 3 degenerate (start not finite or not positive
        semi-definite, or fewer than n_free / 2 counting visibilities: `theta` keeps the start,
        the other outputs of that map are NaN / -1) -- and with `trace` the rows [M, n_iter, 3 + P]
        of (chi^2 of the trial, lambda, accepted, the trial), NaN beyond `niter`.  `vis`: complex128
        [M, K] or float64 [M, K, 2] device tensor (read only); `su`, `sv` [M]; `u`, `v` [K]: host
        arrays or device tensors; `theta0`: [M, P] or one start [P] for all, P = 6 or 12;
        `weights`: None (all ones), [K] (shared) or [M, K]; `free`: None (all free) or P flags, one
        pattern for all maps -- a fixed parameter keeps its start (sizes fixed at 0: a point).  A
        visibility counts when Re V, Im V, u, v and the weight are finite and the weight > 0.  The
        same bits on every call.  The number of workgroups per iteration is kept in
        `last_uvfit_tiles`."""
        torch = _torch()
        n_iter = int(n_iter)
        if n_iter < 1:
            raise ValueError("uvfit: n_iter must be positive")
        dvis = self._vis_stack("uvfit", vis)
        M, K = int(dvis.shape[0]), int(dvis.shape[1])
        su, sv = self._map_scales("uvfit", su, sv, M)
        du, dv = self._device_f64(u), self._device_f64(v)
        if du.numel() != K or dv.numel() != K:
            raise ValueError("uvfit: u and v must have one entry per visibility (%d)" % K)
        if not (np.isfinite(lambda0) and lambda0 > 0. and np.isfinite(xtol) and xtol > 0.):
            raise ValueError("uvfit: `lambda0` and `xtol` must be finite and positive")
        if isinstance(theta0, torch.Tensor):
            theta = theta0.to(device=self.device, dtype=torch.float64)
        else:
            theta = torch.from_numpy(np.ascontiguousarray(theta0, dtype=np.float64)).to(self.device)
        if theta.dim() == 1:
            theta = theta.reshape(1, -1)
        P = int(theta.shape[-1]) if theta.dim() == 2 else 0
        if P < 6 or P % 6 != 0 or P // 6 > UVFIT_MAX_COMP:
            raise ValueError("uvfit: `theta0` must hold 6 values per component, 1 to %d components"
                             % UVFIT_MAX_COMP)
        if theta.shape[0] == 1:
            theta = theta.expand(M, P)
        if theta.shape[0] != M:
            raise ValueError("uvfit: `theta0` must be one start or one per map (%d)" % M)
        theta = theta.contiguous().clone()
        dw, w_maps = None, 1
        if weights is not None:
            dw = self._device_f64(weights)
            if dw.numel() not in (K, M * K):
                raise ValueError("uvfit: `weights` must be [K] or [M, K] = [%d, %d]" % (M, K))
            w_maps = dw.numel() // K
        hfree = None
        if free is not None:
            fr = np.ascontiguousarray(np.asarray(free) != 0, dtype=np.uint8).reshape(-1)
            if fr.size != P or not fr.any():
                raise ValueError("uvfit: `free` must hold %d flags, at least one of them set" % P)
            hfree = (C.c_uint8 * P)(*fr)
        T = P * (P + 1) // 2
        chi2 = torch.full((M,), float("nan"), dtype=torch.float64, device=self.device)
        cov = torch.full((M, T), float("nan"), dtype=torch.float64, device=self.device)
        nvis, niter, status = (torch.full((M,), -1, dtype=torch.int32, device=self.device)
                               for _ in range(3))
        tr = (torch.full((M, n_iter, 3 + P), float("nan"), dtype=torch.float64, device=self.device)
              if trace else None)
        work = self._workspace(max(1, self.lib.rjp_uvfit_workspace(M, K, P // 6)))
        self.last_uvfit_tiles = self._call_tiles(
            "rjp_uvfit", dvis.data_ptr(), M, K, _lib.dbl_array(su), _lib.dbl_array(sv),
            du.data_ptr(), dv.data_ptr(), _ptr(dw), w_maps, P // 6, hfree, theta.data_ptr(),
            float(lambda0), float(xtol), n_iter, chi2.data_ptr(), cov.data_ptr(), nvis.data_ptr(),
            niter.data_ptr(), status.data_ptr(), _ptr(tr), work.data_ptr(), work.numel())
        out = dict(theta=theta, chi2=chi2, cov=cov, nvis=nvis, niter=niter, status=status)
        if trace:
            out["trace"] = tr
        return out

    # -- K21 -------------------------------------------------------------------------------------
    def _line_cube(self, who, cube, x):
        """A cube [F, ...] of float64 channel planes on this device and its axis -> (cube, the
        axis as a host vector, F, n_pix)."""
        torch = _torch()
        x = np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x,
                                 dtype=np.float64).reshape(-1)
        F = x.size
        if not (isinstance(cube, torch.Tensor) and cube.dtype == torch.float64 and
                cube.device == self.device and cube.is_contiguous() and cube.dim() >= 2 and
                F >= 1 and cube.shape[0] == F and cube.numel() >= F):
            raise ValueError("%s: `cube` must be a contiguous float64 tensor [F, ...] on %s with one "
                             "plane per entry of `x` (%d)" % (who, self.device, F))
        if F > SPECFIT_MAX_CHAN:
            raise ValueError("%s: at most %d channels" % (who, SPECFIT_MAX_CHAN))
        return cube, x, F, cube.numel() // F

    def cube_moments(self, cube, x, dx, x_ref, clip=0., mask=None):
        """Moment maps of a line cube (rjp_cube_moments), one lane per pixel, nothing going to
        the host -> (`mom` [4, n_pix] float64 = (m0, m1, m2, peak), `ipeak` [n_pix] int32, `count`
        [n_pix] int32) device tensors.  `cube`: float64 device tensor [F, ...] of channel planes
        (read only: a `flux_rrl` stack, a `CleanResult.image`); `x`, `dx` [F]: HOST axis (any unit,
        any order, need not be uniform) and channel widths (>= 0: `velocity_axis`); `x_ref`: the
        origin the first moment is accumulated about (the mid-channel); `clip`: a channel counts
        when it is finite and |y| >= clip; `mask`: None or n_pix values, non-zero = live.  Over
        the counted channels in ascending order m0 = sum y dx, m1 = x_ref + sum y dx (x - x_ref) /
        m0, m2 = sqrt(sum y dx (x - m1)^2 / m0) (NaN below 0), the peak = the largest y (the lowest
        channel on a tie); no counted channel or m0 == 0: m0 = +0.0, the rest NaN, ipeak -1.  The
        bits of a pixel depend on its spectrum and the tables alone.  The number of workgroups is
        kept in `last_specfit_workgroups`."""
        torch = _torch()
        cube, x, F, npix = self._line_cube("cube_moments", cube, x)
        dx = np.ascontiguousarray(dx, dtype=np.float64).reshape(-1)
        if dx.size != F:
            raise ValueError("cube_moments: `dx` must have one entry per channel (%d)" % F)
        dmask = self._device_mask("cube_moments", mask, npix)
        mom = self._f64(4, npix)
        ipeak = torch.empty(npix, dtype=torch.int32, device=self.device)
        count = torch.empty(npix, dtype=torch.int32, device=self.device)
        self.last_specfit_workgroups = self._call_tiles(
            "rjp_cube_moments", cube.data_ptr(), npix, F, _lib.dbl_array(x), _lib.dbl_array(dx),
            float(x_ref), float(clip), _ptr(dmask), mom.data_ptr(), ipeak.data_ptr(),
            count.data_ptr())
        return mom, ipeak, count

    def specfit(self, cube, x, theta, x_ref, weights=None, free=None, n_comp=1, lambda0=1e-3,
                xtol=1e-10, n_iter=40, mask=None, trace=False):
        """One Levenberg-Marquardt fit per pixel of `n_comp` Gaussians plus a linear baseline,
        y(x) = sum_c A_c exp(-(x - x0_c)^2 / (2 s_c^2)) + b0 + b1 (x - x_ref), to a line cube
        (rjp_specfit): the whole fit of a pixel in ONE launch, one lane per pixel, nothing going to
        the host -> dict of device tensors: `theta` [P, n_pix], P = 3 n_comp + 2 parameter planes
        (A_0, x0_0, s_0, [A_1, x0_1, s_1,] b0, b1); `chi2` [n_pix]; `cov` [P (P + 1) / 2, n_pix]
        (the packed upper triangle of J^T W J at `theta`, identity rows for fixed parameters, NOT
        inverted: `specfit_results`); `nchan`, `niter`, `status` [n_pix] int32 -- 1 converged, 0
        `n_iter` exhausted, 2 stalled (lambda > 1e12), 3 degenerate (masked, a start that is not
        finite or has s <= 0, fewer counted channels than free parameters: `theta` keeps the
        start, the other outputs of that pixel are NaN / -1) -- and with `trace` the rows [n_pix,
        n_iter, 3 + P] of (chi^2 of the trial, lambda, accepted, the trial), NaN beyond `niter`.
        `cube`, `x`, `x_ref`, `mask` as `cube_moments`; `theta`: the start, [P, n_pix] or [P] for
        all (`specfit_start`; it is copied); `weights`: None (all ones) or [F] HOST values >= 0 (1
        / sigma^2 per channel, 0 = ignore); `free`: None (all free) or P flags, one pattern for
        all pixels -- b0 = b1 = 0 held is the fit of a continuum-subtracted cube.  A channel
        counts when it is finite and its weight > 0.  The iteration is `uvfit`'s.  The bits of a
        pixel depend on its spectrum and the tables alone."""
        return self._line_fit("specfit", "rjp_specfit", 3, SPECFIT_MAX_COMP, cube, x, theta, x_ref,
                              weights, free, n_comp, lambda0, xtol, n_iter, mask, trace)

    def _line_fit(self, who, symbol, per_comp, max_comp, cube, x, theta, x_ref, weights, free, n_comp,
                  lambda0, xtol, n_iter, mask, trace):
        """What `specfit` (K21) and `voigtfit` (K24) share: the checks, the buffers and the call of
        `symbol` with P = per_comp n_comp + 2 parameter planes -> the dict both return.  The number
        of workgroups is kept in `last_specfit_workgroups` (one grid for both: 64 pixels each)."""
        torch = _torch()
        n_iter, n_comp = int(n_iter), int(n_comp)
        if n_iter < 1:
            raise ValueError(who + ": n_iter must be positive")
        if not 1 <= n_comp <= max_comp:
            raise ValueError(who + ": n_comp must be 1 to %d" % max_comp)
        cube, x, F, npix = self._line_cube(who, cube, x)
        if not (np.isfinite(lambda0) and lambda0 > 0. and np.isfinite(xtol) and xtol > 0.):
            raise ValueError(who + ": `lambda0` and `xtol` must be finite and positive")
        P = per_comp * n_comp + 2
        if isinstance(theta, torch.Tensor):
            th = theta.to(device=self.device, dtype=torch.float64)
        else:
            th = torch.from_numpy(np.ascontiguousarray(theta, dtype=np.float64)).to(self.device)
        if th.dim() == 1:
            th = th.reshape(-1, 1).expand(-1, npix)
        if th.shape[0] != P or th.numel() != P * npix:
            raise ValueError(who + ": `theta` must be [P] or [P, n_pix] = [%d, %d]" % (P, npix))
        th = th.reshape(P, npix).contiguous().clone()
        hw = None
        if weights is not None:
            wv = np.ascontiguousarray(weights.detach().cpu().numpy()
                                      if isinstance(weights, torch.Tensor) else weights,
                                      dtype=np.float64).reshape(-1)
            if wv.size != F:
                raise ValueError(who + ": `weights` must have one entry per channel (%d)" % F)
            hw = _lib.dbl_array(wv)
        hfree = None
        if free is not None:
            fr = np.ascontiguousarray(np.asarray(free) != 0, dtype=np.uint8).reshape(-1)
            if fr.size != P or not fr.any():
                raise ValueError(who + ": `free` must hold %d flags, at least one of them set" % P)
            hfree = (C.c_uint8 * P)(*fr)
        dmask = self._device_mask(who, mask, npix)
        T = P * (P + 1) // 2
        chi2 = torch.full((npix,), float("nan"), dtype=torch.float64, device=self.device)
        cov = torch.full((T, npix), float("nan"), dtype=torch.float64, device=self.device)
        nchan, niter, status = (torch.full((npix,), -1, dtype=torch.int32, device=self.device)
                                for _ in range(3))
        tr = (torch.full((npix, n_iter, 3 + P), float("nan"), dtype=torch.float64,
                         device=self.device) if trace else None)
        self.last_specfit_workgroups = self._call_tiles(
            symbol, cube.data_ptr(), npix, F, _lib.dbl_array(x), float(x_ref), hw,
            _ptr(dmask), n_comp, hfree, th.data_ptr(), float(lambda0), float(xtol), n_iter,
            chi2.data_ptr(), cov.data_ptr(), nchan.data_ptr(), niter.data_ptr(),
            status.data_ptr(), _ptr(tr))
        out = dict(theta=th, chi2=chi2, cov=cov, nchan=nchan, niter=niter, status=status)
        if trace:
            out["trace"] = tr
        return out

    # -- K24 -------------------------------------------------------------------------------------
    def voigtfit(self, cube, x, theta, x_ref, weights=None, free=None, n_comp=1, lambda0=1e-3,
                 xtol=1e-10, n_iter=40, mask=None, trace=False):
        """One Levenberg-Marquardt fit per pixel of `n_comp` area-normalised Voigt profiles plus a
        linear baseline, y(x) = sum_c F_c Re w(u_c + i a_c) / (s_c sqrt(2 pi)) + b0 + b1 (x -
        x_ref), u = (x - x0) / (sqrt(2) s), a = g / (sqrt(2) s), to a line cube (rjp_voigtfit):
        `specfit` with the profile the model's own lines have -> the same dict of device tensors,
        with P = 4 n_comp + 2 parameter planes (F_0, x0_0, s_0, g_0, [F_1, x0_1, s_1, g_1,] b0,
        b1): F the component's integral over x, s the Doppler dispersion, g the Lorentz HWHM, both
        in the unit of `x`.  Every argument as `specfit`'s; `theta`: the start (`voigt_start`),
        degenerate (status 3) also where a g < 0; `free` may hold g at 0 (a Gaussian fit in area
        form) or s at a known thermal width.  A trial with an s <= 0 or a g < 0 is rejected.
        The number of workgroups is kept in `last_specfit_workgroups`."""
        return self._line_fit("voigtfit", "rjp_voigtfit", 4, VOIGTFIT_MAX_COMP, cube, x, theta, x_ref,
                              weights, free, n_comp, lambda0, xtol, n_iter, mask, trace)

    # -- K22 -------------------------------------------------------------------------------------
    GAIN_APPLY_MODES = {"corrupt": 0, "correct": 1}
    GAINCAL_MODES = {"ap": 0, "p": 1}

    def _gain_layout(self, who, vis, h_sol, n_ant):
        """A visibility stack [M, n_t n_bl] and the host interval table -> (float64 [M, K, 2], M,
        n_t, n_sol, the table as a ctypes int32 pointer into an array it keeps alive)."""
        dvis = self._vis_stack(who, vis)
        n_ant = int(n_ant)
        if not 2 <= n_ant <= GAINCAL_MAX_ANT:
            raise ValueError("%s: n_ant must be 2 to %d" % (who, GAINCAL_MAX_ANT))
        sol = np.ascontiguousarray(h_sol, dtype=np.int32).reshape(-1)
        n_t, n_bl = sol.size, n_ant * (n_ant - 1) // 2
        if n_t < 1 or int(dvis.shape[1]) != n_t * n_bl:
            raise ValueError("%s: `vis` must hold n_t x n_bl = %d x %d visibilities per map, in the "
                             "order of `uv_tracks`" % (who, n_t, n_bl))
        if sol[0] != 0 or np.any((np.diff(sol) != 0) & (np.diff(sol) != 1)):
            raise ValueError("%s: `h_sol` must start at 0 and rise in steps of 0 or 1" % who)
        ptr = sol.ctypes.data_as(C.POINTER(C.c_int32))
        ptr._keep = sol                          # (the table may be long: no element-wise copy)
        return dvis, int(dvis.shape[0]), n_t, int(sol[-1]) + 1, ptr

    def _gain_stack(self, who, gains, n_sol, n_ant):
        torch = _torch()
        if isinstance(gains, torch.Tensor) and gains.dtype == torch.complex128:
            gains = torch.view_as_real(gains)
        if not (isinstance(gains, torch.Tensor) and gains.dtype == torch.float64 and
                gains.device == self.device and gains.is_contiguous() and gains.dim() == 4 and
                tuple(gains.shape[1:]) == (n_sol, n_ant, 2) and gains.shape[0] >= 1):
            raise ValueError("%s: `gains` must be a contiguous complex128 [G, n_sol, n_ant] or "
                             "float64 [G, n_sol, n_ant, 2] = [G, %d, %d, 2] tensor on %s"
                             % (who, n_sol, n_ant, self.device))
        return gains

    def gain_apply(self, vis, gains, h_sol, n_ant, mode="corrupt", out=None):
        """Antenna gains times a stack of visibility sets (rjp_gain_apply), one thread per
        visibility, nothing going to the host -> complex128 device tensor [M, n_t n_bl].  `vis`:
        complex128 [M, n_t n_bl] (or float64 [..., 2]) in the order of `uv_tracks` (integration by
        integration, the pairs (p < q) p-major); `gains`: complex128 [G, n_sol, n_ant] (or float64
        [..., 2]), G = 1 (shared) or M; `h_sol` [n_t]: the HOST interval table
        (`solution_intervals`); `mode`: 'corrupt' (V g_p conj g_q) or 'correct' (V conj(c) / |c|^2,
        c = g_p conj g_q); `out`: None or a tensor like `vis` (may be `vis` itself).  A NaN gain or
        visibility gives a NaN visibility.  The workgroup count is kept in
        `last_gain_apply_workgroups`."""
        torch = _torch()
        if mode not in self.GAIN_APPLY_MODES:
            raise ValueError("gain_apply: mode must be 'corrupt' or 'correct'")
        dvis, M, n_t, n_sol, sol = self._gain_layout("gain_apply", vis, h_sol, n_ant)
        g = self._gain_stack("gain_apply", gains, n_sol, int(n_ant))
        if g.shape[0] not in (1, M):
            raise ValueError("gain_apply: `gains` must hold one set or one per map (%d)" % M)
        if out is None:
            vout = self._f64(*dvis.shape)
        else:
            vout = self._vis_stack("gain_apply", out)
            if tuple(vout.shape) != tuple(dvis.shape):
                raise ValueError("gain_apply: `out` must be shaped like `vis`")
        self.last_gain_apply_workgroups = self._call_tiles(
            "rjp_gain_apply", dvis.data_ptr(), M, n_t, int(n_ant), g.data_ptr(), int(g.shape[0]),
            sol, n_sol, self.GAIN_APPLY_MODES[mode], vout.data_ptr())
        return torch.view_as_complex(vout)

    def gaincal(self, vis, model, h_sol, n_ant, gains=None, weights=None, mode="ap", refant=0,
                min_bl=4, tol=1e-10, n_iter=300, trace=False):
        """Antenna gains of every (map, solution interval) of a stack of visibility sets against
        model visibilities (rjp_gaincal: StefCal, D_pq = g_p conj(g_q) M_pq), three launches and
        nothing going to the host -> dict of device tensors: `gains` complex128 [M, n_sol, n_ant]
        (NaN for a dead antenna and for every antenna of a status-3 solution; the reference
        antenna real and positive), `chi2` [M, n_sol, 2] (sum w |D - g_p conj(g_q) M|^2 at the
        start and at the solution), `nvis`, `niter`, `status` [M, n_sol] int32 -- 1 converged, 0
        `n_iter` exhausted, 2 a vanishing or non-finite denominator, 3 degenerate (too few live
        antennas, or a live antenna's start gain 0 or not finite: `chi2` NaN, `niter` -1) --,
        `live` [M, n_sol, n_ant] uint8 (0 for status 3), and with `trace` the gains after every
        step before referencing, float64 [M, n_sol, n_iter, n_ant, 2], NaN beyond `niter`.
        `vis`, `h_sol`, `n_ant` as `gain_apply`; `model`: complex128 [1 or M, n_t n_bl];
        `gains`: None (ones) or the start, complex128 [M, n_sol, n_ant] (it is copied: pass a
        result's `gains` to continue); `weights`: None, [n_t n_bl] or [M, n_t n_bl]; `mode`: 'ap'
        (amplitude and phase) or 'p' (phase only: every |g| = 1); `refant`: the antenna whose
        phase is 0, the lowest live one where it is dead; `min_bl`: an antenna with fewer
        partners with data is dead (applied until nothing changes).  A visibility counts when
        data, model and weight are finite, the weight > 0 and the model is not 0.  The same bits
        on every call; a solution's bits depend on its own interval alone."""
        torch = _torch()
        if mode not in self.GAINCAL_MODES:
            raise ValueError("gaincal: mode must be 'ap' or 'p'")
        n_iter, n_ant, refant, min_bl = int(n_iter), int(n_ant), int(refant), int(min_bl)
        if n_iter < 1 or min_bl < 1:
            raise ValueError("gaincal: n_iter and min_bl must be positive")
        if not (np.isfinite(tol) and tol > 0.):
            raise ValueError("gaincal: `tol` must be finite and positive")
        dvis, M, n_t, n_sol, sol = self._gain_layout("gaincal", vis, h_sol, n_ant)
        if not 0 <= refant < n_ant:
            raise ValueError("gaincal: refant must be 0 to n_ant - 1")
        K = int(dvis.shape[1])
        dmod = self._vis_stack("gaincal", model)
        if int(dmod.shape[1]) != K or dmod.shape[0] not in (1, M):
            raise ValueError("gaincal: `model` must be [1 or M, K] = [%d, %d]" % (M, K))
        dw, w_maps = None, 1
        if weights is not None:
            dw = self._device_f64(weights)
            if dw.numel() not in (K, M * K):
                raise ValueError("gaincal: `weights` must be [K] or [M, K] = [%d, %d]" % (M, K))
            w_maps = dw.numel() // K
        if gains is None:
            g = torch.zeros((M, n_sol, n_ant, 2), dtype=torch.float64, device=self.device)
            g[..., 0] = 1.
        else:
            g = self._gain_stack("gaincal", gains, n_sol, n_ant)
            if g.shape[0] != M:
                raise ValueError("gaincal: `gains` must hold one start per map (%d)" % M)
            g = g.clone()
        chi2 = torch.full((M, n_sol, 2), float("nan"), dtype=torch.float64, device=self.device)
        nvis, niter, status = (torch.full((M, n_sol), -1, dtype=torch.int32, device=self.device)
                               for _ in range(3))
        live = torch.zeros((M, n_sol, n_ant), dtype=torch.uint8, device=self.device)
        tr = (torch.full((M, n_sol, n_iter, n_ant, 2), float("nan"), dtype=torch.float64,
                         device=self.device) if trace else None)
        work = self._workspace(max(1, self.lib.rjp_gaincal_workspace(M, n_sol, n_ant)))
        self.last_gaincal_workgroups = self._call_tiles(
            "rjp_gaincal", dvis.data_ptr(), M, n_t, n_ant, dmod.data_ptr(), int(dmod.shape[0]),
            _ptr(dw), w_maps, sol, n_sol, self.GAINCAL_MODES[mode], refant, min_bl, float(tol),
            n_iter, g.data_ptr(), chi2.data_ptr(), nvis.data_ptr(), niter.data_ptr(),
            status.data_ptr(), live.data_ptr(), _ptr(tr), work.data_ptr(), work.numel())
        out = dict(gains=torch.view_as_complex(g), chi2=chi2, nvis=nvis, niter=niter,
                   status=status, live=live)
        if trace:
            out["trace"] = tr
        return out

    # -- K23 -------------------------------------------------------------------------------------
    def _sample_stack(self, who, name, t, lead):
        """A stack of complex (complex128 [...] or float64 [..., 2]) or real (float64 [...])
        samples with `lead` leading dimensions -> (float64 tensor, n_part)."""
        torch = _torch()
        if isinstance(t, torch.Tensor) and t.dtype == torch.complex128:
            t = torch.view_as_real(t)
        n_part = 2 if isinstance(t, torch.Tensor) and t.dim() == lead + 1 else 1
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and
                t.device == self.device and t.is_contiguous() and t.dim() == lead + n_part - 1 and
                t.numel() >= 1 and (n_part == 1 or t.shape[-1] == 2)):
            raise ValueError("%s: `%s` must be a contiguous complex128 or float64 tensor with %d "
                             "dimensions (float64 complex samples: one more, of 2) on %s"
                             % (who, name, lead, self.device))
        return t, n_part

    def normal_eq(self, data, model, dmodel, sel, weights=None):
        """The normal equations of a least-squares fit from stacks on the device (rjp_normal_eq),
        two launches and nothing going to the host -> (chi2, g[P], N_packed[P (P + 1) / 2], count)
        device tensors (float64; `count` int64), P = len(sel): chi^2 = sum w |data - model|^2,
        g_p = sum w Re(conj(J_p) r), N_pq = sum w Re(conj(J_p) J_q) (packed upper triangle, row by
        row) over the samples that count -- datum and weight finite, w > 0 -- and their number.
        `data`, `model`: complex128 [n_rows, n_vis] (or float64 [n_rows, n_vis, 2]) as `vis`
        returns them, or float64 [n_rows, n_vis] for real samples (a light curve: n_vis = 1);
        `dmodel`: [n_rows, n_par, n_vis] of the same kind, plane j = d model / d theta_j (`vis` of
        the derivative maps of `ff_formal_grad`, or its `dftot` as [E F, n_par, 1]); `sel`: the
        planes that take part, distinct, at most NORMAL_EQ_MAX_SEL -- the others are never read;
        with no plane (chi^2 and the count alone) `dmodel` may be None; `weights`: None, [n_vis]
        (shared by the rows) or [n_rows, n_vis].  Every sum in the order include/rjprt.h states:
        the same bits on every call.  The workgroup count is kept in `last_normal_eq_workgroups`."""
        torch = _torch()
        d, n_part = self._sample_stack("normal_eq", "data", data, 2)
        m, m_part = self._sample_stack("normal_eq", "model", model, 2)
        if m_part != n_part or tuple(m.shape) != tuple(d.shape):
            raise ValueError("normal_eq: `model` must be shaped like `data`")
        n_rows, n_vis = int(d.shape[0]), int(d.shape[1])
        sel = np.ascontiguousarray(sel, dtype=np.int32).reshape(-1)
        P = int(sel.size)
        if P > NORMAL_EQ_MAX_SEL:
            raise ValueError("normal_eq: at most %d planes" % NORMAL_EQ_MAX_SEL)
        n_par, dj = 0, None
        if P or dmodel is not None:
            dj, j_part = self._sample_stack("normal_eq", "dmodel", dmodel, 3)
            n_par = int(dj.shape[1])
            if j_part != n_part or (int(dj.shape[0]), int(dj.shape[2])) != (n_rows, n_vis):
                raise ValueError("normal_eq: `dmodel` must be [n_rows, n_par, n_vis] = [%d, n_par, "
                                 "%d] of the kind of `data`" % (n_rows, n_vis))
            if P and (sel.min() < 0 or sel.max() >= n_par or np.unique(sel).size != P):
                raise ValueError("normal_eq: `sel` must hold distinct planes in [0, %d)" % n_par)
        dw, w_rows = None, 1
        if weights is not None:
            dw = self._device_f64(weights)
            if dw.numel() not in (n_vis, n_rows * n_vis):
                raise ValueError("normal_eq: `weights` must be [n_vis] or [n_rows, n_vis] = [%d, %d]"
                                 % (n_rows, n_vis))
            w_rows = dw.numel() // n_vis
        out = self._f64(1 + P + P * (P + 1) // 2)
        count = torch.empty(1, dtype=torch.int64, device=self.device)
        work = self._workspace(max(1, self.lib.rjp_normal_eq_workspace(n_rows, n_vis, P)))
        self.last_normal_eq_workgroups = self._call_tiles(
            "rjp_normal_eq", d.data_ptr(), m.data_ptr(), _ptr(dj), n_rows, n_vis, n_part, n_par,
            sel.ctypes.data_as(C.POINTER(C.c_int32)), P, _ptr(dw), w_rows, out.data_ptr(),
            count.data_ptr(), work.data_ptr(), work.numel())
        return out[0], out[1:1 + P], out[1 + P:], count[0]

    # -- K25 -------------------------------------------------------------------------------------
    def _mask_stack(self, who, name, mask, npix, M=None):
        """`mask` (device tensor, any dtype, non-zero = set) -> (uint8 tensor [n, npix], n); with
        `M`, n must be 1 or M."""
        torch = _torch()
        if not (isinstance(mask, torch.Tensor) and mask.device == self.device and
                mask.numel() >= npix and mask.numel() % npix == 0):
            raise ValueError("%s: `%s` must be a tensor of a whole number (>= 1) of nx * nz masks "
                             "on %s" % (who, name, self.device))
        if mask.dtype != torch.uint8:
            mask = (mask != 0).to(torch.uint8)
        mask = mask.reshape(-1, npix).contiguous()
        n = int(mask.shape[0])
        if M is not None and n not in (1, M):
            raise ValueError("%s: `%s` must hold one mask or one per map (%d)" % (who, name, M))
        return mask, n

    def _check_cap_flag(self, who, work):
        """The first int32 of a K25 workspace: non-zero when a loop of the labelling ran into its
        cap (include/rjprt.h).  One 4-byte read, which waits for the call."""
        if int(work[:4].view(_torch().int32).item()) != 0:
            raise _lib.RjprtError("%s: a union-find loop ran into its iteration cap (the labels "
                                  "are not valid)" % who)

    def image_stats(self, img, nx, nz, mask=None, inside=True):
        """Robust statistics of a stack of images (rjp_image_stats), nothing going to the host ->
        float64 device tensor [M, 8]: count, n_nonfinite, min, max, median, mad, sum, sumsq per
        map, over the finite pixels that `mask` (None, one [nx * nz] or one per map; non-zero =
        set) selects -- inside it, or with `inside=False` outside it.  The median is the LOWER
        median (an element of the input), the MAD the same rank of |x - median|; an exact radix
        select, the same bits on every call (`image_stats_results` names the numbers).  The
        workgroup count is kept in `last_image_stats_workgroups`."""
        torch = _torch()
        nx, nz = int(nx), int(nz)
        if nx < 1 or nz < 1:
            raise ValueError("image_stats: nx and nz must be positive")
        if not (isinstance(img, torch.Tensor) and img.numel() >= nx * nz and
                img.numel() % (nx * nz) == 0):
            raise ValueError("image_stats: `img` must hold a whole number (>= 1) of nx * nz images")
        M = img.numel() // (nx * nz)
        self._stack_f64("image_stats", "img", img, M * nx * nz)
        dmask, n_mask = (None, 1) if mask is None else \
            self._mask_stack("image_stats", "mask", mask, nx * nz, M)
        stats = self._f64(M, 8)
        work = self._workspace(max(1, self.lib.rjp_image_stats_workspace(M, nx, nz)))
        self.last_image_stats_workgroups = self._call_tiles(
            "rjp_image_stats", img.data_ptr(), M, nx, nz, _ptr(dmask), n_mask, 1 if inside else 0,
            stats.data_ptr(), work.data_ptr(), work.numel())
        return stats

    def label_regions(self, mask, nx, nz, connectivity=1):
        """Connected components of a stack of masks (rjp_label_regions) -> (label[M, nx * nz] int32,
        area[M, nx * nz] int32, nreg[M] int32) device tensors: 0 on background, otherwise 1 + the
        smallest pixel index of the pixel's region; the region's pixel count on each of its pixels;
        the number of regions.  `mask`: device tensor of M * nx * nz values, non-zero = set;
        `connectivity` 1 (four neighbours) or 2 (eight).  Reads the workspace's cap flag (4 bytes)
        and raises if a loop ran into its cap."""
        torch = _torch()
        nx, nz = int(nx), int(nz)
        if nx < 1 or nz < 1:
            raise ValueError("label_regions: nx and nz must be positive")
        dmask, M = self._mask_stack("label_regions", "mask", mask, nx * nz)
        label = torch.empty(M, nx * nz, dtype=torch.int32, device=self.device)
        area = torch.empty(M, nx * nz, dtype=torch.int32, device=self.device)
        nreg = torch.empty(M, dtype=torch.int32, device=self.device)
        work = self._workspace(max(1, self.lib.rjp_label_regions_workspace(M, nx, nz)))
        self.last_label_regions_workgroups = self._call_tiles(
            "rjp_label_regions", dmask.data_ptr(), M, M, nx, nz, int(connectivity),
            label.data_ptr(), area.data_ptr(), nreg.data_ptr(), work.data_ptr(), work.numel())
        self._check_cap_flag("label_regions", work)
        return label, area, nreg

    def mask_grow(self, seed, constraint, nx, nz, n_iter, connectivity=1):
        """Geodesic dilation of a stack of masks (rjp_mask_grow) -> uint8 device tensor [M, nx * nz]
        (a new tensor; `seed` is not changed): `n_iter` steps of seed | (dilate(seed) & constraint),
        scipy.ndimage.binary_dilation(seed, structure, iterations=n_iter, mask=constraint); a seed
        pixel outside the constraint stays.  `n_iter` 0: the seed itself; < 0: until stable.
        `seed`: M * nx * nz values; `constraint`: one mask or one per map; non-zero = set."""
        nx, nz = int(nx), int(nz)
        if nx < 1 or nz < 1:
            raise ValueError("mask_grow: nx and nz must be positive")
        dseed, M = self._mask_stack("mask_grow", "seed", seed, nx * nz)
        dcon, n_con = self._mask_stack("mask_grow", "constraint", constraint, nx * nz, M)
        out = (dseed != 0).to(dseed.dtype)
        work = self._workspace(max(1, self.lib.rjp_mask_grow_workspace(M, nx, nz)))
        self.last_mask_grow_workgroups = self._call_tiles(
            "rjp_mask_grow", out.data_ptr(), dcon.data_ptr(), n_con, M, nx, nz, int(n_iter),
            int(connectivity), work.data_ptr(), work.numel())
        if int(n_iter) < 0:
            self._check_cap_flag("mask_grow", work)
        return out

    # -- K15 -------------------------------------------------------------------------------------
    UV_WEIGHT_MODES ={"uniform": 1, "briggs": 2}

    def uv_weights(self, u, v, su, sv, nx, nz, w=None, mode="briggs", robust=0.5,
                   want_density=False):
        """Uniform or Briggs imaging weights (rjp_uv_weights) of `n_vis` visibilities for each of
        M imaging grids -> float64 device tensor [M, K].  `u`, `v`, `w` [K]: host arrays or device
        tensors, `w` (the data weights the scheme starts from) None = all ones; `su`, `sv` [M]:
        cycles per cell per unit of `u`, `v` of the nx x nz IMAGE the weights are for
        (`image_scales`).  The cell of a visibility is (rint((su u) nx), rint((sv v) nz)) on the
        symmetric grid of (2 (nx // 2) + 1)(2 (nz // 2) + 1) cells; the density W of a cell is the
        sum of the weights in it and in its mirror cell, summed in fixed point (order-free, the
        same bits on every call); uniform: w / W, Briggs: w / (1 + f2 W) with
        f2 = (5 10^-robust)^2 (2 sum w) / sum W^2.  A visibility with a non-finite u, v or w, a
        negative w, or a cell outside the grid gets 0.  Nothing goes to the host:
        `last_uv_weight_stats` is a device tensor [M, 6] of (sum w, sum W^2, f2, counted, out of
        range, the fixed-point shift s), `last_uv_weight_density` the density [M, cells] when
        `want_density` (else None), `last_uv_weight_tiles` the workgroups of the scatter."""
        nx, nz = int(nx), int(nz)
        if nx < 1 or nz < 1:
            raise ValueError("uv_weights: nx and nz must be positive")
        if mode not in self.UV_WEIGHT_MODES:
            raise ValueError("uv_weights: `mode` must be 'uniform' or 'briggs' (natural weights "
                             "need no kernel)")
        robust = float(robust)
        if mode == "briggs" and not (-2. <= robust <= 2.):
            raise ValueError("uv_weights: `robust` must lie in [-2, 2]")
        su, sv = self._map_scales("uv_weights", su, sv)
        M = su.size
        du, dv = self._device_f64(u), self._device_f64(v)
        dw = self._device_f64(w) if w is not None else None
        K = du.numel()
        if K < 1 or dv.numel() != K or (dw is not None and dw.numel() != K):
            raise ValueError("uv_weights: u, v and w must have the same length >= 1")
        cells = (2 * (nx // 2) + 1) * (2 * (nz // 2) + 1)
        out = self._f64(M, K)
        stats = self._f64(M, 6)
        dens = self._f64(M, cells) if want_density else None
        work = self._workspace(max(1, self.lib.rjp_uv_weights_workspace(M, nx, nz, K)))
        self.last_uv_weight_tiles = self._call_tiles(
            "rjp_uv_weights", M, K, _lib.dbl_array(su), _lib.dbl_array(sv), du.data_ptr(),
            dv.data_ptr(), _ptr(dw), nx, nz, self.UV_WEIGHT_MODES[mode], robust, out.data_ptr(),
            stats.data_ptr(), _ptr(dens), work.data_ptr(), work.numel())
        self.last_uv_weight_stats = stats
        self.last_uv_weight_density = dens
        return out

    # -- K16 -------------------------------------------------------------------------------------
    def uv_tracks(self, xyz, gha_turns, dec_rad, up=None, min_el_rad=None, want_w=True):
        """(u, v, w) [m] of every baseline of an array at every integration (rjp_uv_tracks) ->
        three float64 device tensors [n_t, n_bl] (`w` None without `want_w`); n_bl =
        n_ant (n_ant - 1) / 2, pairs (i < j) in i-major order, b = xyz_j - xyz_i.  `xyz`
        [n_ant, 3]: geocentric (ITRF) positions [m]; `gha_turns` [n_t]: the Greenwich hour angle
        of the phase centre in TURNS (local hour angle minus east longitude); `dec_rad`: its
        declination.  With `up` [n_ant, 3] (unit local verticals: `geodetic`) and `min_el_rad`,
        a baseline with an antenna below the elevation limit is NaN in all three -- the flag
        `vis`, `vis_adjoint` and `uv_weights` honour; a non-finite hour angle flags its whole
        integration.  The same bits on every call; `last_uv_tracks_tiles`: the workgroups."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float64)
        gha = np.ascontiguousarray(gha_turns, dtype=np.float64).reshape(-1)
        if xyz.ndim != 2 or xyz.shape[1] != 3 or xyz.shape[0] < 2:
            raise ValueError("uv_tracks: `xyz` must be [n_ant >= 2, 3]")
        if gha.size < 1:
            raise ValueError("uv_tracks: `gha_turns` must hold at least one integration")
        A, T = int(xyz.shape[0]), int(gha.size)
        if (up is None) != (min_el_rad is None):
            raise ValueError("uv_tracks: `up` and `min_el_rad` go together")
        hup, sme = None, 0.0
        if up is not None:
            up = np.ascontiguousarray(up, dtype=np.float64)
            if up.shape != xyz.shape:
                raise ValueError("uv_tracks: `up` must have the shape of `xyz`")
            hup, sme = _lib.dbl_array(up), float(np.sin(min_el_rad))
        B = A * (A - 1) // 2
        if T * B > 2 ** 31 - 1:
            raise ValueError("uv_tracks: n_t * n_bl exceeds 2^31 - 1")
        u, v = self._f64(T, B), self._f64(T, B)
        w = self._f64(T, B) if want_w else None
        self.last_uv_tracks_tiles = self._call_tiles(
            "rjp_uv_tracks", _lib.dbl_array(xyz), A, _lib.dbl_array(gha), T, float(np.sin(dec_rad)),
            float(np.cos(dec_rad)), hup, sme, u.data_ptr(), v.data_ptr(), _ptr(w))
        return u, v, w

    def vis_noise(self, vis, sigma, seed=0, s=None, k0=0, m0=0, out=None):
        """Thermal noise added to a stack of visibility sets (rjp_vis_noise):
        out[m, k] = vis[m, k] + sigma[m] s[k] (g1 + i g2) with (g1, g2) one Box-Muller pair of
        the Philox4x32-10 block keyed by `seed` and counted by (k0 + k, m0 + m) -- a pure function
        of (seed, map, visibility): chunks called with their offsets `k0`, `m0` reproduce the
        bits of the whole.  `vis`: complex128 [M, K] or float64 [M, K, 2] device tensor; `sigma`:
        one rms [the unit of `vis`] of the real and of the imaginary part, or one per map (0 =
        that map is copied bit for bit); `s` [K]: per-visibility factors (host or device; None =
        ones; a non-finite one makes its visibility NaN in every map); `out`: None = a new
        tensor, or `vis` itself (in place).  Returns a tensor of the type of `vis`.
        `last_vis_noise_tiles`: the workgroups."""
        torch = _torch()
        cplx = isinstance(vis, torch.Tensor) and vis.dtype == torch.complex128
        v3 = self._vis_stack("vis_noise", vis)
        M, K = int(v3.shape[0]), int(v3.shape[1])
        sg = np.asarray(sigma, dtype=np.float64).reshape(-1)
        if sg.size not in (1, M):
            raise ValueError("vis_noise: `sigma` must be one number or one per map (%d)" % M)
        sg = np.ascontiguousarray(np.broadcast_to(sg, (M,)))
        ds = self._device_f64(s) if s is not None else None
        if ds is not None and ds.numel() != K:
            raise ValueError("vis_noise: `s` must have one entry per visibility (%d)" % K)
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("vis_noise: `seed` must fit 64 unsigned bits")
        if out is None:
            o3 = torch.empty_like(v3)
        elif out is vis:
            o3 = v3
        else:
            raise ValueError("vis_noise: `out` must be None or `vis` itself")
        self.last_vis_noise_tiles = self._call_tiles(
            "rjp_vis_noise", v3.data_ptr(), M, K, _lib.dbl_array(sg), _ptr(ds), seed, int(k0),
            int(m0), o3.data_ptr())
        return torch.view_as_complex(o3) if cplx else o3

    def rrl_cells(self, fields, bursts, time_s, line, nus):
        """collapse=False: per-cell RRL optical depths -> device tensor [F, N]."""
        F = len(nus)
        out = self._f64(F, fields.ncells)
        fs = fields.struct()
        self._call("rjp_rrl_cells", C.byref(fs), _ref(bursts), float(time_s), C.byref(line),
                   _lib.dbl_array(nus), F, out.data_ptr())
        return out

    # -- K3 ------------------------------------------------------------------------------------
    def rrl_scan(self, fields, bursts, time_s, line, nus):
        """-> tau_rrl[F,P] device tensor."""
        F = len(nus)
        tau = self._f64(F, fields.npix)
        fs = fields.struct()
        nu = _lib.dbl_array(nus)
        self._call("rjp_rrl_scan", C.byref(fs), _ref(bursts), float(time_s), C.byref(line), nu, F,
                   tau.data_ptr())
        return tau

    def rrl_formal(self, fields, bursts, time_s, gff_mode, line, nus, ctau, csrc, hnu_k,
                   add=None, out=None):
        """LTE recombination-line intensity by the formal solution along the line of sight
        (rjp_rrl_formal): csrc[f] * (I_tot - I_cont), the line's emission minus its absorption of
        what lies behind it, cell by cell with B_i = 1 / expm1(hnu_k[f] / T_i), observer at the
        iy = 0 end of axis 1 -> device tensor [F, P] (float64), NaN where the sightline has no
        T > 0; negative where the line absorbs against hotter gas behind.  `ctau` as for `ff_maps`;
        `csrc`, `hnu_k` = `rrl_channel_coeffs` (csrc divided by omega / 1e-26 for intensity).
        `add` [F, P]: added to the result (the formal continuum, for contsub=False).  One epoch
        (`time_s` [s]) per call; `fields` must hold the wide layout (nd, xi, temp, pf, vy)."""
        F = len(nus)
        if not (len(ctau) == len(csrc) == len(hnu_k) == F):
            raise ValueError("rrl_formal: nus, ctau, csrc and hnu_k must have one entry per channel")
        torch = _torch()
        for name, t in (("add", add), ("out", out)):
            # the kernel reads / writes F * P device doubles through the bare pointer
            if t is not None and not (t.dtype == torch.float64 and t.device == self.device and
                                      t.is_contiguous() and t.numel() == F * fields.npix):
                raise ValueError("rrl_formal: `%s` must be a contiguous float64 tensor of F * P "
                                 "values on %s" % (name, self.device))
        if out is None:
            out = self._f64(F, fields.npix)
        fs = fields.struct()
        self._call("rjp_rrl_formal", C.byref(fs), _ref(bursts), float(time_s), int(gff_mode),
                   C.byref(line), _lib.dbl_array(nus), _lib.dbl_array(ctau), _lib.dbl_array(csrc),
                   _lib.dbl_array(hnu_k), F, _ptr(add), out.data_ptr())
        return out

    def rrl_maps(self, tau_rrl, tau_ff, tavg, flux_ff, cflux_rrl, hnu_k, want_ftot=True):
        """-> (flux[F,P], ftot[F])."""
        F, P = tau_rrl.shape
        flux = self._f64(F, P)
        ftot = self._f64(F) if want_ftot else None
        wb = self.lib.rjp_ff_maps_workspace(P, 1, F)
        work = self._workspace_maps(wb) if want_ftot else None
        a, b = _lib.dbl_array(cflux_rrl), _lib.dbl_array(hnu_k)
        self._call("rjp_rrl_maps", tau_rrl.data_ptr(), tau_ff.data_ptr(), tavg.data_ptr(),
                   _ptr(flux_ff), P, a, b, F, flux.data_ptr(), _ptr(ftot), _ptr(work),
                   work.numel() if work is not None else 0)
        return flux, ftot


# -- host-side per-channel coefficients (scalars; classes.py:1395-1397, 1473-1475, 1519-1521) --
def solid_angle(csize_au, dist_pc):
    return np.arctan((csize_au * con.au) / (dist_pc * con.parsec)) ** 2.


def ff_channel_coeffs(freqs, csize_au, dist_pc, gff_mode, gff_values=None):
    """ctau[f], cflux[f] of include/rjprt.h `rjp_ff_maps`."""
    freqs = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    path0 = csize_au * con.au * 1e2
    if gff_mode == RJP_GFF_SCALAR:
        g = np.asarray(gff_values, dtype=np.float64)
        ctau = 0.018 * freqs ** -2. * path0 * g
    else:
        ctau = 0.018 * freqs ** -2. * path0 * (11.95 * freqs ** -0.1)
    cflux = 2. * freqs ** 2. * con.k / con.c ** 2. * solid_angle(csize_au, dist_pc) / 1e-26
    return ctau, cflux


def rrl_channel_coeffs(freqs, csize_au, dist_pc):
    """cflux_rrl[f], hnu_k[f] of `rjp_rrl_maps` (physics.py:571-574; rrls.py:444-449)."""
    freqs = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    p1 = 2. * con.h * 1e7 * freqs ** 3. / (con.c * 1e2) ** 2.
    cflux = p1 * 1e-7 * 1e4 * solid_angle(csize_au, dist_pc) / 1e-26
    hnu_k = con.h * 1e7 * freqs / (con.k * 1e7)
    return cflux, hnu_k
