"""Host-side mirror of RaJePy's `JetModel` / `ContinuumRun` / `RRLRun` / `Pipeline`
(reference: classes.py) for the radiative-transfer path: same constructor arguments,
method names, argument meaning, return shapes/dtypes, file names and error behaviour.

What is different underneath: the 3-D grids live in HBM as five/six packed fields plus two
derived scan fields (`engine.DeviceFields`), are BUILT on the GPU (`rjp_build_fields`) and
every line-of-sight reduction runs in librjprt's HIP kernels through the C-ABI of
include/rjprt.h.  One grid pass serves every continuum channel of an epoch (the reference
re-streams the grid per channel), up to 32 uniformly spaced epochs share a pass (16 when
fewer are left, else tiles of 8 / 4 / 2 / 1), and everything that depends on neither
frequency nor epoch -- the temperature factor of the optical depth, the T_avg map -- is
evaluated once per model.  There is no CPU fallback for any of it.
"""
import collections
import os
import pickle
import runpy
import time as _time

import numpy as np

from . import _constants as con
from . import _lib
from . import fits as _fits
from . import logger
# the imaging chain and its result types live in imaging.py; `JetModel` is a front to it
from .imaging import (CleanResult, Imager, Observation, UVTracks, Weighting,  # noqa: F401
                      _split_weights, _weighting_mode, image_scales, vis_scales)
from .spectra import Spectra, velocity_axis
from .calibration import Calibrator, SelfcalResult  # noqa: F401
from .inference import BurstFit, EjectionFit  # noqa: F401
from .maths import geometry as mgeom
from .maths import physics as mphys
from .maths import rrls as mrrl
from .miscellaneous import functions as miscf

_STORAGE = {'f64': _lib.RJP_F64, 'f32': _lib.RJP_F32, 8: _lib.RJP_F64, 4: _lib.RJP_F32}


def geometry_struct(params, nx, ny, nz, ix0=0, nx_total=0):
    """`rjp_geometry` (include/rjprt.h) from a model params dict with derived keys; with
    `ix0`/`nx_total` only rows [ix0, ix0+nx) of an nx_total-wide grid are described."""
    g, t, pl, pr = (params['geometry'], params['target'], params['power_laws'],
                    params['properties'])
    s = _lib.Geometry()
    s.nx, s.ny, s.nz = int(nx), int(ny), int(nz)
    s.rotation_ccw = 1 if g["rotation"].lower() == 'ccw' else 0
    s.csize = params['grid']['c_size']
    s.inc, s.pa = g['inc'], g['pa']
    s.w_0, s.r_0, s.mod_r_0, s.epsilon = g['w_0'], g['r_0'], g['mod_r_0'], g['epsilon']
    s.R_1, s.R_2, s.M_star, s.v_lsr = t['R_1'], t['R_2'], t['M_star'], t['v_lsr']
    s.n_0, s.x_0, s.T_0, s.v_0 = pr['n_0'], pr['x_0'], pr['T_0'], pr['v_0']
    s.q_n, s.q_x, s.q_T, s.q_v = pl['q_n'], pl['q_x'], pl['q_T'], pl['q_v']
    s.qd_n, s.qd_x, s.qd_T, s.qd_v = pl['q^d_n'], pl['q^d_x'], pl['q^d_T'], pl['q^d_v']
    s.rb_frac = pr['mlr_rj'] / pr['mlr_bj']
    s.ix0, s.nx_total = int(ix0), int(nx_total)
    return s


def build_model_fields(model, geom, **kw):
    """K4 for `geom` (the whole grid of `model`, or an x-slab of it).  Only the library's
    dedicated refusal of a logarithmic 2F1 case (RJP_ERR_DEGENERATE: q^d_v and the
    launch-time exponent differ by an integer) is answered with the host evaluation of the
    launch times; every other failure (bad geometry, HIP error, ABI mismatch) propagates."""
    eng = model.engine
    # fill factor and areas as separate arrays are redundant for a model (areas is 1 wherever
    # it is not NaN, so the path factor ff/areas IS the fill factor: the accessors read `pf`):
    # two grid-sized f64 arrays less to allocate and to write
    kw.setdefault("want_raw", False)
    # the tau scan field for the model's Gaunt branch is written in K4's own pass
    kw.setdefault("tau_mode", model.gff_mode)
    try:
        return eng.build_fields(geom, model._dtype, want_ts=True, **kw)
    except _lib.RjprtError as exc:
        if exc.status != _lib.RJP_ERR_DEGENERATE:
            raise
    dev = eng.build_fields(geom, model._dtype, want_ts=False, **kw)
    ts = model._host_launch_times(geom.ix0, geom.ix0 + geom.nx)
    eng.replace_field(dev, "ts", ts)
    return dev


def _dist_info():
    """(rank, world, torch.distributed or None) -- world > 1 only inside an initialised
    process group (one process per GPU, e.g. under torchrun)."""
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist.get_rank(), dist.get_world_size(), dist
    except ImportError:
        pass
    return 0, 1, None


def _to_host(tensor):
    """Device tensor -> NumPy array.  Large products go through page-locked memory (6x the
    pageable rate on MI355X: 19 ms instead of 121 ms for the 1.07 GB cfg4 cubes); the array
    returned is backed by that buffer, which PyTorch's host allocator recycles once the array
    is dropped."""
    import torch
    if tensor.is_cuda and tensor.numel() * tensor.element_size() >= (8 << 20):
        try:
            host = torch.empty(tensor.shape, dtype=tensor.dtype, pin_memory=True)
            host.copy_(tensor)
            return host.numpy()
        except RuntimeError:
            pass                                   # page-locked allocation refused: plain copy
    return tensor.cpu().numpy()


def ejection_chain_rule(t_0, peak_jml, half_life, ss_jml):
    """One ejection event as the kernels see it, and the derivatives of that conversion:
    -> ((t0, amp_rel, inv2s2), (dt0/dt_0, damp_rel/dpeak_jml, dinv2s2/dhalf_life)) with
    amp_rel = (peak_jml - ss_jml) / ss_jml, sigma = half_life / sqrt(2 ln 2) (classes.py:442-448)
    and inv2s2 = 1 / (2 sigma^2) = ln 2 / half_life^2.  The conversion is diagonal: each of
    (t_0 [s], peak_jml [kg/s], half_life [s]) moves exactly one kernel parameter."""
    sigma = half_life / np.sqrt(2. * np.log(2.))
    inv2s2 = 1. / (2. * sigma ** 2.)
    return ((t_0, (peak_jml - ss_jml) / ss_jml, inv2s2),
            (1., 1. / ss_jml, -2. * inv2s2 / half_life))


def ejection_burst(t_0, peak_jml, half_life, ss_jml):
    """One ejection event as `JetModel._bursts` and `engine.make_bursts` hold it: (t_0 [s], amp_rel,
    sigma [s]) with amp_rel = (peak_jml - ss_jml) / ss_jml and sigma = half_life 2 / (2 sqrt(2 ln 2))
    (classes.py:442-448) -- the one place `add_ejection_event`, `set_ejection_event` and the trial
    bursts of a fit (`inference.BurstFit`) take it from."""
    sigma = half_life * 2. / (2. * np.sqrt(2. * np.log(2.)))
    return (t_0, (peak_jml - ss_jml) / ss_jml, sigma)


def _load_params_file(py_file, checker):
    if not os.path.exists(py_file):
        raise FileNotFoundError(py_file + " does not exist")
    params = runpy.run_path(py_file)["params"]
    err = checker(params)
    if err is not None:
        raise err
    return params


def _vis_vs_time_chunks(self, times, u_d, v_d, freq, formal):
    """The chunks of `JetModel.visibilities_vs_time` on the device, for it and for
    `uvmodelfit_vs_time`: yields (first epoch, epochs, V), V the complex tensor [epochs * F, K]
    of the chunk, epoch-major.  `self`: the model."""
    eng = self.engine
    freqs, (ctau, cflux) = self._channel_coeffs(freq)
    F = len(freqs)
    su, sv = self._vis_scales(freqs)
    step = self._vis_chunk(F)
    if not formal:
        step = min(step, self.SCAN_CACHE_EPOCHS)     # what one prefetch keeps resident
    for e0 in range(0, len(times), step):
        chunk = times[e0:e0 + step]
        if formal:
            maps, _ = eng.ff_formal_sweep(self.device_fields, self._rjp_bursts(), chunk,
                                          self.gff_mode, ctau, cflux, want_maps=True,
                                          want_totals=False)
        else:
            import torch
            self.prefetch_epochs(chunk, want_em=False)
            rows = []
            for t in chunk:
                if t not in self._scan_cache:    # evicted by the chunk's own new epochs
                    self.prefetch_epochs([t], want_em=False)
                rows.append(self._scan_cache[t][0])
            sumA = torch.cat(rows, dim=0)
            maps = eng.ff_maps(sumA, self._model_tavg(), ctau, cflux, want_tau=False,
                               want_ftot=False)[1]
        V = eng.vis(maps.reshape(len(chunk) * F, -1), self.nx, self.nz,
                    np.tile(su, len(chunk)), np.tile(sv, len(chunk)), u_d, v_d)
        del maps
        yield e0, len(chunk), V
        del V


class JetModel:
    """Physical model of an ionised jet + its line-of-sight radiative transfer."""
    _arr_indexing = 'ij'

    # ------------------------------------------------------------------ construction ----
    @classmethod
    def load_model(cls, model_file, engine=None):
        """Restore a model saved by `JetModel.save` (classes.py:48-88)."""
        with open(os.path.expanduser(model_file), 'rb') as f:
            loaded = pickle.load(f)
        log = loaded.get('log')
        if log is None:
            log = logger.Log(os.path.expanduser('~') + os.sep + 'temp.log')
        new = cls(loaded["params"], log=log, engine=engine,
                  storage=loaded.get('storage', 'f64'))
        new.time = loaded['time']
        return new

    @staticmethod
    def lz_to_grid_dims(params):
        """Grid dimensions from the requested jet length l_z [arcsec] (classes.py:90-122)."""
        cs = params["grid"]["c_size"]
        g = params["geometry"]
        i_rads, pa_rads = np.radians(g["inc"]), np.radians(g["pa"])
        l_xz = params['grid']['l_z'] * params['target']['dist']
        xmax, ymax, zmax = (l_xz * np.sin(pa_rads), l_xz * np.tan(1.571 - i_rads),
                            l_xz * np.cos(pa_rads))
        rmax = mgeom.xyz_to_rwp(xmax, ymax, zmax, g["inc"], g["pa"])[0]
        wmax = mgeom.w_r(rmax, g["w_0"], g["mod_r_0"], g["r_0"], g["epsilon"])
        pad = 2 * int(np.ceil(np.abs(wmax / cs)))
        dims = [int(np.ceil(np.abs(v / cs))) + pad for v in (xmax, ymax, zmax)]
        return tuple(n if n % 2 == 0 else n + 1 for n in dims)

    @staticmethod
    def py_to_dict(py_file):
        """Model parameter file -> dict (classes.py:124-142)."""
        return _load_params_file(py_file, miscf.check_model_params)

    def __init__(self, params, log=None, engine=None, storage='f64'):
        if isinstance(params, dict):
            self._params = params
        elif isinstance(params, str):
            self._params = JetModel.py_to_dict(params)
        else:
            raise TypeError("Supplied arg params must be dict or file path (str)")
        if storage not in _STORAGE:
            raise ValueError("storage must be 'f64' or 'f32'")
        self._dtype = _STORAGE[storage]
        p = self._params
        self._name = p['target']['name']
        self._csize = p['grid']['c_size']

        # derived parameters, written back into the dict as the reference does
        # (classes.py:169-180)
        g, pl = p['geometry'], p['power_laws']
        g["mod_r_0"] = mgeom.mod_r_0(g['opang'], g['epsilon'], g['w_0'])
        pl["q_n"] = mphys.q_n(g["epsilon"], pl["q_v"])
        pl["q_tau"] = mphys.q_tau(g["epsilon"], pl["q_x"], pl["q_n"], pl["q_T"])

        if log is not None:
            self._log = log
        else:
            self._log = logger.Log(os.path.expanduser('~') + os.sep + 'temp.log',
                                   verbose=True)

        if p['grid'].get('l_z') is not None:
            nx, ny, nz = JetModel.lz_to_grid_dims(p)
            self.log.add_entry(
                "INFO", 'For a (bipolar) jet length of {:.1f}", cell size of {:.2f}au and '
                        'distance of {:.0f}pc, a grid size of (n_x, n_y, n_z) = ({}, {}, {}) '
                        'voxels is calculated'.format(p['grid']['l_z'], p["grid"]["c_size"],
                                                      p["target"]["dist"], nx, ny, nz))
        else:
            nx, ny, nz = ((p['grid'][k] + 1) // 2 * 2 for k in ('n_x', 'n_y', 'n_z'))
        p['grid']['n_x'], p['grid']['n_y'], p['grid']['n_z'] = nx, ny, nz
        self._nx, self._ny, self._nz = int(nx), int(ny), int(nz)

        pr = p["properties"]
        self._ss_jml_rb_frac = pr["mlr_rj"] / pr["mlr_bj"]
        self._ss_jml_bj = pr["mlr_bj"] * 1.989e30 / con.year          # classes.py:230-231
        self._ss_jml_rj = self._ss_jml_bj * self._ss_jml_rb_frac
        pr["n_0"] = mphys.n_0_from_mlr(pr["mlr_bj"], pr["v_0"], g["w_0"], pr["mu"],
                                       pl["q^d_n"], pl["q^d_v"], p["target"]["R_1"],
                                       p["target"]["R_2"])

        self._ejections = {}
        self._bursts = {'R': [], 'B': []}           # (t0 [s], amp_rel, sigma [s])
        for idx, t0 in enumerate(p['ejection']['t_0']):
            which = str(p['ejection']['which'][idx])
            for jet, ss in (('R', self._ss_jml_rj), ('B', self._ss_jml_bj)):
                if jet in which:
                    self.add_ejection_event(t0 * con.year, ss * p['ejection']['chi'][idx],
                                            p['ejection']['hl'][idx] * con.year, which=jet)
        self._time = 0. * con.year

        # device state (created lazily: constructing a model needs no GPU, using it does)
        self._engine = engine
        self._dev = None
        self._version = 0            # bumped whenever a field or the burst list changes
        self._scan_cache = collections.OrderedDict()   # time -> (sumA[1,P], em[1,P] | None) tensors
        self._tavg = None
        self._vxz = None
        self._rrl_cache = None
        self._dev_product = None     # device cube of the last product, for _save_cube

    # ------------------------------------------------------------------ bookkeeping ----
    def __str__(self):
        """The parameter table the reference prints and embeds in every FITS header
        (classes.py:268-361)."""
        p = self.params
        g, pl, pr, tg = p['geometry'], p['power_laws'], p['properties'], p['target']
        rows = [('epsilon', format(g['epsilon'], '+.3f')),
                ('opang', format(g['opang'], '+.0f') + ' deg'),
                ('q_v', format(pl['q_v'], '+.3f')), ('q_T', format(pl['q_T'], '+.3f')),
                ('q_x', format(pl['q_x'], '+.3f')), ('q_n', format(pl['q_n'], '+.3f')),
                ('q^d_v', format(pl['q^d_v'], '+.3f')), ('q^d_T', format(pl['q^d_T'], '+.3f')),
                ('q^d_x', format(pl['q^d_x'], '+.3f')), ('q^d_n', format(pl['q^d_n'], '+.3f')),
                ('q_tau', format(pl['q_tau'], '+.3f')),
                ('cell', format(p['grid']['c_size'], '.1f') + ' au'),
                ('w_0', format(g['w_0'], '.2f') + ' au'),
                ('r_0', format(g['r_0'], '.2f') + ' au'),
                ('v_0', format(pr['v_0'], '.0f') + ' km/s'),
                ('x_0', format(pr['x_0'], '.3f')),
                ('n_0', format(pr['n_0'], '.3e') + ' cm^-3'),
                ('T_0', format(pr['T_0'], '.0e') + ' K'),
                ('f_R2B', format(self._ss_jml_rb_frac, '.2e')),
                ('i', format(g['inc'], '+.1f') + ' deg'),
                ('theta', format(g['pa'], '+.1f') + ' deg'),
                ('D', format(tg['dist'], '+.0f') + ' pc'),
                ('M*', format(tg['M_star'], '+.1f') + ' Msol'),
                ('R_1', format(tg['R_1'], '+.1f') + ' au'),
                ('R_2', format(tg['R_2'], '+.1f') + ' au')]
        if len(p['ejection']['t_0']) > 0:
            rows.append(('t_now', format(self.time / con.year, '+.3f') + ' yr'))
        head = ('Parameter', 'Value')
        w1 = max(len(head[0]), *(len(r[0]) for r in rows)) + 2
        w2 = max(len(head[1]), *(len(r[1]) for r in rows)) + 2
        width = w1 + w2 + 3
        rule = '-' * width

        def line(cells, widths):
            return '|' + '|'.join(format(c, '^' + str(w)) for c, w in zip(cells, widths)) + '|\n'

        s = rule + '\n' + '/' + format('JET MODEL', '^' + str(width - 2)) + '/\n' + rule + '\n'
        s += line(head, (w1, w2)) + rule + '\n'
        for r in rows:
            s += line(r, (w1, w2))
        s += rule + '\n'
        s += '/' + format('BURSTS', '^' + str(width - 2)) + '/\n' + rule + '\n'
        ej = p["ejection"]
        if len(ej["t_0"]) == 0:
            return s + '|' + format(' None ', '-^' + str(width - 2)) + '|\n' + rule + '\n'
        base, extra = divmod(width - 4, 3)
        bw = [base + (1 if extra > 0 else 0), base + (1 if extra == 2 else 0), base]
        s += line(('t_0', 'FWHM', 'chi'), bw) + line(('[yr]', '[yr]', ''), bw) + rule + '\n'
        for i, t in enumerate(ej["t_0"]):
            s += line((format(t, '.2f'), format(ej["hl"][i], '.2f'),
                       format(ej["chi"][i], '.2f')), bw)
        return s + rule + '\n'

    @property
    def los_axis(self):
        return 1 if self._arr_indexing == 'ij' else 0

    @property
    def time(self):
        """Model time [s]."""
        return self._time

    @time.setter
    def time(self, new_time):
        self._time = new_time

    @property
    def log(self):
        return self._log

    @log.setter
    def log(self, new_log):
        self._log = new_log

    csize = property(lambda self: self._csize)
    nx = property(lambda self: self._nx)
    ny = property(lambda self: self._ny)
    nz = property(lambda self: self._nz)
    params = property(lambda self: self._params)
    name = property(lambda self: self._name)
    ejections = property(lambda self: self._ejections)

    def ss_jml(self, which):
        if which == 'R':
            return self._ss_jml_rj
        if which == 'B':
            return self._ss_jml_bj
        if 'R' in which and 'B' in which:
            return self._ss_jml_rj + self._ss_jml_bj
        raise ValueError("which must be one of 'R', 'B', or 'RB'")

    def add_ejection_event(self, t_0, peak_jml, half_life, which):
        """Gaussian mass-loss burst (classes.py:399-463): t_0, half_life [s], peak [kg/s]."""
        which = which.upper()                                    # classes.py:450, 455
        if which not in ('R', 'B'):
            raise ValueError("which must be 'R' or 'B'")
        ss = self._ss_jml_bj if which == 'B' else self._ss_jml_rj
        self._bursts[which].append(ejection_burst(t_0, peak_jml, half_life, ss))
        self._ejections[str(len(self._ejections) + 1)] = {
            't_0': t_0, 'peak_jml': peak_jml, 'half_life': half_life, 'which': which}
        self._invalidate()

    def set_ejection_event(self, key, t_0=None, peak_jml=None, half_life=None):
        """Change the ejection event `key` of `model.ejections` in place: the values given ([s],
        [kg/s], [s]; None keeps one) replace its entry and its burst as `add_ejection_event` would
        have made them, and what that invalidates is invalidated.  Its jet cannot change."""
        key = str(key)
        if key not in self._ejections:
            raise KeyError("no ejection event %r" % key)
        ej = self._ejections[key]
        which = ej['which']
        idx = [k for k, e in self._ejections.items() if e['which'] == which].index(key)
        new = dict(ej)
        for name, val in (('t_0', t_0), ('peak_jml', peak_jml), ('half_life', half_life)):
            if val is not None:
                new[name] = val
        ss = self._ss_jml_bj if which == 'B' else self._ss_jml_rj
        self._bursts[which][idx] = ejection_burst(new['t_0'], new['peak_jml'], new['half_life'], ss)
        self._ejections[key] = new
        self._invalidate()

    def jml_t(self, which):
        """Callable mdot(t) [kg/s] of the red and/or blue jet (classes.py:383-397)."""
        def mdot(t):
            tot = 0.
            for jet, ss in (('R', self._ss_jml_rj), ('B', self._ss_jml_bj)):
                if jet in which:
                    tot = tot + ss * self._chi_host(jet, t)
            return tot
        return mdot

    def _chi_host(self, jet, t):
        chi = 1.0
        for t0, amp_rel, sigma in self._bursts[jet]:
            chi = chi + amp_rel * np.exp(-(t - t0) ** 2. / (2. * sigma ** 2.))
        return chi

    # ------------------------------------------------------------------ device state ----
    @property
    def engine(self):
        if self._engine is None:
            from .engine import RTEngine
            # one process per GPU: LOCAL_RANK picks the device (RJP_DEVICE overrides it,
            # e.g. to rehearse several ranks on one GPU)
            self._engine = RTEngine(int(os.environ.get("RJP_DEVICE",
                                                       os.environ.get("LOCAL_RANK", "0"))))
        return self._engine

    def _invalidate(self):
        self._version = getattr(self, "_version", 0) + 1
        self._scan_cache = collections.OrderedDict()
        self._tavg = None
        self._rrl_cache = None

    @property
    def gff_mode(self):
        """classes.py:1388-1393: one Gaunt factor per channel iff q_T == 0."""
        return _lib.RJP_GFF_SCALAR if self.params['power_laws']['q_T'] == 0. \
            else _lib.RJP_GFF_POWERLAW

    @property
    def device_fields(self):
        """The packed HBM state; built on the GPU on first use (K4)."""
        if self._dev is None:
            if self.log:
                self.log.add_entry("INFO", "Calculating cells' fill factors/projected areas")
            then = _time.time()
            geom = geometry_struct(self.params, self.nx, self.ny, self.nz)
            # LEAN first (f64 storage): the continuum path reads a0, em0, temp, ts -- four
            # grid-sized arrays; nd / xi / pf / vy are built by the first call that needs them
            # (`_wide_fields`: RRL, collapse=False, grid accessors, the xi / vel setters), as
            # the reference's lazy properties do (classes.py:571-1000)
            eng = self.engine
            lean = self._dtype == _lib.RJP_F64 and eng.use_compact and eng.use_tau
            self._dev = build_model_fields(self, geom, want_wide=not lean, want_vy=not lean)
            # a jet fills a few per cent of its grid: record each sightline's occupied rows
            # once so that every later scan touches only those
            self.engine.compute_y_bounds(self._dev)
            self.engine.synchronize()
            if self.log:
                self.log.add_entry("INFO", _time.strftime(
                    'Finished in %Hh%Mm%Ss', _time.gmtime(_time.time() - then)))
        return self._dev

    def _wide_fields(self):
        """`device_fields` with nd, xi, pf and vy resident (built on first need)."""
        dev = self.device_fields
        if dev.nd is None or dev.xi is None or dev.pf is None or dev.vy is None:
            self.engine.build_wide(dev, geometry_struct(self.params, self.nx, self.ny, self.nz))
        return dev

    def _host_launch_times(self, x0=0, x1=None):
        """Launch times [s] of rows [x0, x1) of the grid evaluated on the host with scipy's
        hyp2f1, exactly as the reference does (maths/geometry.py:150-178) -- only for the
        logarithmic 2F1 cases the device series refuses (RJP_ERR_DEGENERATE)."""
        g = self.params['geometry']
        x1 = self.nx if x1 is None else x1
        ix, iy, iz = np.meshgrid(np.arange(x0, x1), np.arange(self.ny), np.arange(self.nz),
                                 indexing='ij')
        c = self.csize
        rr, ww, _ = mgeom.xyz_to_rwp(c * (ix - self.nx // 2) + c / 2., c * (iy - self.ny // 2) +
                                     c / 2., c * (iz - self.nz // 2) + c / 2., g["inc"], g["pa"])
        r = np.abs(rr)
        r = np.where((r < g['r_0']) & ((r + c / 2.) >= g['r_0']), (g['r_0'] + r + c / 2.) / 2., r)
        with np.errstate(all="ignore"):
            return mgeom.t_rw(r, ww, self.params) * con.year

    def _rjp_bursts(self):
        from .engine import make_bursts
        return make_bursts(self._bursts['R'], self._bursts['B'])

    def _grid(self, tensor):
        return tensor.cpu().numpy().astype(np.float64).reshape(self.nx, self.ny, self.nz)

    # ---- geometry accessors (host NumPy; plotting / inspection only, never on the RT path) --
    @property
    def indices(self):
        """Cell index grids (classes.py:465-474)."""
        return tuple(np.meshgrid(np.arange(self.nx), np.arange(self.ny), np.arange(self.nz),
                                 indexing=self._arr_indexing))

    ix = property(lambda self: self.indices[0])
    iy = property(lambda self: self.indices[1])
    iz = property(lambda self: self.indices[2])

    @property
    def grid(self):
        """Bottom-left-front cell corners [au] (classes.py:488-501)."""
        ix, iy, iz = self.indices
        return (self.csize * (ix - self.nx // 2), self.csize * (iy - self.ny // 2),
                self.csize * (iz - self.nz // 2))

    xx = property(lambda self: self.grid[0])
    yy = property(lambda self: self.grid[1])
    zz = property(lambda self: self.grid[2])
    xs = property(lambda self: self.csize * (np.arange(self.nx) - self.nx // 2))
    ys = property(lambda self: self.csize * (np.arange(self.ny) - self.ny // 2))
    zs = property(lambda self: self.csize * (np.arange(self.nz) - self.nz // 2))

    @property
    def grid_rwp(self):
        """Jet coordinates (r, w, phi) of the cell centroids (classes.py:515-526)."""
        xx, yy, zz = self.grid
        h = self.csize / 2.
        g = self.params["geometry"]
        return mgeom.xyz_to_rwp(xx + h, yy + h, zz + h, g["inc"], g["pa"])

    rr = property(lambda self: self.grid_rwp[0])
    ww = property(lambda self: self.grid_rwp[1])
    pp = property(lambda self: self.grid_rwp[2])

    @property
    def rreff(self):
        """Effective launching radius in the disc [au] (classes.py:543-557)."""
        g, t = self.params["geometry"], self.params["target"]
        r, w, _ = self.grid_rwp
        return mgeom.r_eff(w, t["R_1"], t["R_2"], g['w_0'], np.abs(r), g['mod_r_0'], g['r_0'],
                           g["epsilon"])

    @property
    def mass_density(self):
        """[g cm^-3] (classes.py:901-908)."""
        return self.params['properties']['mu'] * mphys.atomic_mass("H") * 1e3 * \
            self.number_density

    @property
    def pressure(self):
        """[dyn cm^-2] (classes.py:1002-1007)."""
        return self.number_density * self.temperature * con.k * 1e7

    # grids as host arrays (inspection / plotting / pickling; not on the RT path)
    @property
    def fill_factor(self):
        return self._grid(self.device_fields.ff_raw) if self.device_fields.ff_raw is not None \
            else self._grid(self._wide_fields().pf)

    @property
    def areas(self):
        d = self.device_fields
        return self._grid(d.areas_raw) if d.areas_raw is not None else \
            np.where(np.isnan(self._grid(self._wide_fields().pf)), np.nan, 1.0)

    @property
    def ts(self):
        """Time since launch of the material in each cell [s] (classes.py:838-855)."""
        return self.time - self._grid(self.device_fields.ts)

    @ts.setter
    def ts(self, new_ts):
        self.engine.replace_field(self.device_fields, "ts", new_ts)
        self._invalidate()

    @property
    def ion_fraction(self):
        return self._grid(self._wide_fields().xi)

    @ion_fraction.setter
    def ion_fraction(self, new_xis):
        self.engine.replace_field(self._wide_fields(), "xi", new_xis)
        self._invalidate()

    @property
    def temperature(self):
        return self._grid(self.device_fields.temp)

    @temperature.setter
    def temperature(self, new_ts):
        self.engine.replace_field(self.device_fields, "temp", new_ts)
        self._invalidate()

    @property
    def chi_xyz(self):
        """Burst factor per cell (classes.py:861-870)."""
        red = np.signbit(self._grid(self._wide_fields().nd))
        tl = self.ts
        return np.where(red, self._chi_host('R', tl), self._chi_host('B', tl))

    @property
    def number_density(self):
        return np.abs(self._grid(self._wide_fields().nd)) * self.chi_xyz

    @property
    def vel(self):
        """(v_x, v_y + v_lsr, v_z) [km/s] (classes.py:1009-1095).  Only v_y feeds the RT path
        and stays resident; the transverse components are built on demand."""
        if self._vxz is None:
            geom = geometry_struct(self.params, self.nx, self.ny, self.nz)
            tmp = self.engine.build_fields(geom, _lib.RJP_F64, want_ts=False, want_vy=False,
                                           want_raw=False, want_vxz=True)
            self._vxz = (self._grid(tmp.vx_raw), self._grid(tmp.vz_raw))
        return self._vxz[0], self._grid(self._wide_fields().vy), self._vxz[1]

    @vel.setter
    def vel(self, new_vs):
        """Install caller-supplied velocity grids (v_x, v_y, v_z) [km/s] (classes.py:1097-1099).
        The line-of-sight component feeds `optical_depth_rrl` (classes.py:1160-1161) and goes to
        the device; the transverse ones are kept for the getter."""
        vx, vy, vz = new_vs
        shape = (self.nx, self.ny, self.nz)
        vx, vy, vz = (np.asarray(v, dtype=np.float64) for v in (vx, vy, vz))
        if not (vx.shape == vy.shape == vz.shape == shape):
            raise ValueError("velocity grids must have the model's shape {}".format(shape))
        self.engine.replace_field(self._wide_fields(), "vy", vy)
        self._vxz = (vx.copy(), vz.copy())
        self._invalidate()

    # ------------------------------------------------------------------ K1 cache ----
    SCAN_CACHE_EPOCHS = 64       # base-map pairs kept on the device (2 x P x 8 B each)

    def _model_tavg(self):
        """T_avg = nanmean_y(T where T > 0) (classes.py:1471-1472, 1254-1256): depends on
        neither frequency nor epoch, so it is evaluated once per model (and again after the
        temperature grid is replaced through its setter)."""
        if self._tavg is None:
            self._tavg = self.engine.tavg(self.device_fields)
        return self._tavg

    def prefetch_epochs(self, times_s, want_em=True):
        """Scan the grid for several model times at once (8-32 epochs share one pass over
        HBM); later RT calls at those times reuse the base maps.  `want_em=False`: the
        optical-depth sums only, no emission-measure maps -- the only single-epoch scans that
        may read the launch-time-bucketed layout (include/rjprt.h `rjp_fields.d_srt_cells`);
        `emission_measure` scans again for an epoch cached that way."""
        todo = [t for t in dict.fromkeys(float(t) for t in times_s)
                if t not in self._scan_cache or (want_em and self._scan_cache[t][1] is None)]
        if not todo:
            return
        # the cache is bounded (a long sweep must not pin an [E, P] pair per epoch for ever):
        # at most SCAN_CACHE_EPOCHS epochs stay resident, oldest first out; a longer request
        # keeps its FIRST epochs, the ones a caller walking the list in order needs next
        todo = todo[:self.SCAN_CACHE_EPOCHS]
        dev = self.device_fields
        self._model_tavg()
        sumA, em, _ = self.engine.ff_scan(dev, self._rjp_bursts(), todo, self.gff_mode,
                                          want_em=want_em, want_tavg=False)
        for i, t in enumerate(todo):
            # own copies: a slice would keep the whole [E, P] result alive
            self._scan_cache[t] = (sumA[i:i + 1].clone(),
                                   em[i:i + 1].clone() if em is not None else None)
        while len(self._scan_cache) > self.SCAN_CACHE_EPOCHS:
            old = next(iter(self._scan_cache))
            if old in todo:
                break
            del self._scan_cache[old]

    def _base_maps(self, want_em=False):
        """(sumA, em | None, T_avg) of the model's time.  The emission-measure map is scanned only
        for the caller that reads it: without it a single-epoch scan streams two fields per cell
        instead of three and may take the launch-time-bucketed layout K4 attached."""
        t = float(self.time)
        hit = self._scan_cache.get(t)
        if hit is None or (want_em and hit[1] is None):
            self.prefetch_epochs([t], want_em=want_em)
        return self._scan_cache[t] + (self._model_tavg(),)

    def _map(self, tensor, lead=()):
        return _to_host(tensor).reshape(*lead, self.nx, self.nz)

    FITS_DEVICE_MIN_BYTES = 8 << 20      # products from this size on are laid out for FITS on the GPU

    def _ff_products(self, freq, tau=False, flux=False, intensity=False, device=False,
                     keep=False, formal=False):
        """`keep`: remember the device cube so that a following _save_cube can build the FITS
        payload (axis order + byte order) on the GPU instead of in three host passes.
        `formal`: flux / intensity by the formal solution along the line of sight
        (RTEngine.ff_formal) instead of the isothermal T_avg (1 - e^-tau)."""
        from . import engine as E
        scalar = np.isscalar(freq)
        freqs = np.atleast_1d(np.asarray(freq, dtype=np.float64))
        gv = None
        if self.gff_mode == _lib.RJP_GFF_SCALAR:
            gv = [mphys.gff(nu, self.params['properties']['T_0']) for nu in freqs]
        ctau, cflux = E.ff_channel_coeffs(freqs, self.csize, self.params["target"]["dist"],
                                          self.gff_mode, gv)
        if intensity:        # W m^-2 Hz^-1 sr^-1 (classes.py:1475, 1488)
            cflux = 2. * freqs ** 2. * con.k / con.c ** 2.
        if formal:
            if tau:
                raise ValueError("the formal solution gives intensities and fluxes, not tau")
            out = self.engine.ff_formal(self.device_fields, self._rjp_bursts(), float(self.time),
                                        self.gff_mode, ctau, cflux)
        else:
            sumA, _, tavg = self._base_maps()
            t, s, _ = self.engine.ff_maps(sumA, tavg, ctau, cflux, want_tau=tau,
                                          want_flux=flux or intensity, want_ftot=False)
            out = t if tau else s
        if device:
            return out.reshape(len(freqs), self.nx, self.nz)
        arr = self._map(out, (len(freqs),))
        self._dev_product = out.reshape(len(freqs), self.nx, self.nz) if keep else None
        return arr[0] if scalar else arr

    def _cells(self, freq, savefits, rrl=None):
        """collapse=False: un-summed per-cell optical depths, (n_x,n_y,n_z) for a scalar
        frequency, (F,n_x,n_y,n_z) for an array (classes.py:1176-1177, 1382-1383)."""
        from . import engine as E
        if savefits:
            # the reference's writer accepts 2-D / 3-D (freq, dec, ra) data only
            raise ValueError("Unexpected number of data dimensions (4)")
        scalar = np.isscalar(freq)
        freqs = np.atleast_1d(np.asarray(freq, dtype=np.float64))
        dev = self._wide_fields()
        if rrl is None:
            gv = None
            if self.gff_mode == _lib.RJP_GFF_SCALAR:
                gv = [mphys.gff(nu, self.params['properties']['T_0']) for nu in freqs]
            ctau, _ = E.ff_channel_coeffs(freqs, self.csize, self.params["target"]["dist"],
                                          self.gff_mode, gv)
            out = self.engine.ff_cells(dev, self._rjp_bursts(), float(self.time),
                                       self.gff_mode, ctau)
        else:
            out = self.engine.rrl_cells(dev, self._rjp_bursts(), float(self.time),
                                        _lib.Line(**mrrl.line_constants(rrl)), freqs)
        arr = _to_host(out).reshape(len(freqs), self.nx, self.ny, self.nz)
        return arr[0] if scalar else arr

    def flux_vs_time(self, times_s, freq, formal=False):
        """Light curves: total flux density [Jy] of the whole map at every (model time,
        frequency) -> array (len(times), len(freq)).  The reference gets these numbers by
        looping `time` and summing `flux_ff` maps (Pipeline results, classes.py:2461-2467);
        here the maps are reduced on the device and up to 32 epochs share one pass over HBM.
        Inside a torch.distributed group the epochs are shared out over the ranks.
        Memory: a DENSELY filled model keeps its launch-time moment maps after the first sweep of
        >= 12 epochs (1280 doubles per sightline: 2.7 GB at 512 x 512 sightlines) so that later
        sweeps -- other epochs, other burst parameters -- are contractions only; a pipeline that
        holds many such models sets `model.engine.cache_moments = False` (every sweep then makes
        its own pass over the grid), and a setter that replaces a field drops the maps.
        `formal=True`: every flux by the formal solution along the line of sight (the per-epoch
        `nansum(flux_ff(freq, formal=True))`), all epochs of a rank in one walk of the grid
        (`RTEngine.ff_formal_sweep`).  It equals the default curve where the temperature is
        constant along every sightline (q_T = q^d_T = 0) and differs wherever it varies -- by more
        than 1e-3 on a model with a temperature gradient; no cached state is involved (neither
        T_avg nor the moment maps are read or kept)."""
        from . import parallel
        rank, world, _ = _dist_info()
        return parallel.sweep_flux_vs_time(self, np.atleast_1d(np.asarray(times_s, float)),
                                           freq, rank=rank, world=world, formal=bool(formal))

    def _ejection_slots(self):
        """Per ejection, in the order of `self.ejections`: (first kernel parameter k = 3 b of its
        burst -- b counts the red jet's bursts first, then the blue jet's, the order of
        `_rjp_bursts` -- and the three chain-rule factors of `ejection_chain_rule`)."""
        seen = {'R': 0, 'B': 0}
        n_red = len(self._bursts['R'])
        out = []
        for ej in self._ejections.values():
            jet = ej['which']
            b = seen[jet] + (n_red if jet == 'B' else 0)
            seen[jet] += 1
            ss = self._ss_jml_rj if jet == 'R' else self._ss_jml_bj
            out.append((3 * b, ejection_chain_rule(ej['t_0'], ej['peak_jml'], ej['half_life'],
                                                   ss)[1]))
        return out

    def _grad_fields(self):
        """The device fields if the sensitivities can run on them, else ValueError with the reason."""
        if self._dtype != _lib.RJP_F64:
            raise ValueError("burst-parameter sensitivities need f64 storage: an f32 model has no "
                             "tau layout (rjp_fields.d_a0)")
        dev = self.device_fields
        if dev.a0 is None or dev.a0_mode != self.gff_mode or dev.ts is None:
            raise ValueError("burst-parameter sensitivities need the tau layout (a0, ts), which "
                             "this model does not have (negative path factors keep it on the wide "
                             "layout, or the engine's use_tau / use_compact is off)")
        return dev

    def _channel_coeffs(self, freq):
        from . import engine as E
        freqs = np.atleast_1d(np.asarray(freq, dtype=np.float64))
        gv = None
        if self.gff_mode == _lib.RJP_GFF_SCALAR:
            gv = [mphys.gff(nu, self.params['properties']['T_0']) for nu in freqs]
        return freqs, E.ff_channel_coeffs(freqs, self.csize, self.params["target"]["dist"],
                                          self.gff_mode, gv)

    def flux_vs_time_jac(self, times_s, freq, formal=False):
        """The light curves of `flux_vs_time` AND their exact derivatives with respect to the
        parameters of every ejection event: -> (flux[E, F] [Jy], jac[E, F, n_ej, 3]), the last axis
        (t_0 [s], peak_jml [kg/s], half_life [s]), `n_ej` in the order of `model.ejections`.
        One pass over the grid per tile of up to four epochs (`RTEngine.ff_grad`, rjp_ff_grad)
        instead of the 2 n_par + 1 sweeps of a central difference, and no truncation error.
        A model without ejections returns n_ej = 0; a model without the tau layout (f32 storage,
        negative path factors) raises ValueError; at most 8 bursts per jet.  Inside a
        torch.distributed group the call runs on the calling rank only (no collective).
        On a densely filled model that is swept again and again, differencing `flux_vs_time` with
        its launch-time moments cached (contractions only) is the faster route to the same
        Jacobian (512 x 4096 x 512 dense cells, 32 epochs, 15 parameters: 34 ms for the 30 sweeps
        against 211 ms here; against sweeps on the epoch tiles this call is 2.1-5.1 x faster,
        DESIGN.md section 3, K7); this call is the one for sparse jets, sweeps of fewer than 12
        epochs and exact derivatives.
        `formal=True`: the light curves of `flux_vs_time(formal=True)` (bit for bit) and THEIR
        derivatives, from one line-of-sight walk for all epochs (`RTEngine.ff_formal_grad`,
        rjp_ff_formal_grad) -- the route for a model whose temperature varies along the sightlines,
        where the two Jacobians differ by more than 1e-3.  Any f64 layout (a model with negative
        path factors included); f32 storage raises ValueError."""
        if formal:
            return self._flux_vs_time_jac_formal(times_s, freq)
        times = [float(t) for t in np.atleast_1d(np.asarray(times_s, float))]
        freqs, (ctau, cflux) = self._channel_coeffs(freq)
        dev = self._grad_fields()
        eng = self.engine
        slots = self._ejection_slots()
        jac = np.zeros((len(times), len(freqs), len(slots), 3))
        if not times:
            return np.zeros((0, len(freqs))), jac
        if not slots:
            sumA, _, _ = eng.ff_scan(dev, self._rjp_bursts(), times, self.gff_mode, want_em=False,
                                     want_tavg=False)
            ftot = eng.ff_maps(sumA, self._model_tavg(), ctau, cflux, want_tau=False,
                               want_flux=False)[2]
            return ftot.cpu().numpy(), jac
        _, _, ftot, dftot = eng.ff_grad(dev, self._rjp_bursts(), times, self.gff_mode,
                                        self._model_tavg(), ctau, cflux)
        raw = dftot.cpu().numpy()
        for i, (k, chain) in enumerate(slots):
            jac[:, :, i, :] = raw[:, :, k:k + 3] * np.asarray(chain)
        return ftot.cpu().numpy(), jac

    def _flux_vs_time_jac_formal(self, times_s, freq):
        if self._dtype != _lib.RJP_F64:
            raise ValueError("burst-parameter sensitivities need f64 storage")
        times = [float(t) for t in np.atleast_1d(np.asarray(times_s, float))]
        freqs, (ctau, cflux) = self._channel_coeffs(freq)
        slots = self._ejection_slots()
        jac = np.zeros((len(times), len(freqs), len(slots), 3))
        if not times or not slots:
            return np.asarray(self.flux_vs_time(times, freqs, formal=True)).reshape(
                len(times), len(freqs)), jac
        ftot, dftot, _ = self.engine.ff_formal_grad(self.device_fields, self._rjp_bursts(), times,
                                                    self.gff_mode, ctau, cflux)
        raw = dftot.cpu().numpy()
        for i, (k, chain) in enumerate(slots):
            jac[:, :, i, :] = raw[:, :, k:k + 3] * np.asarray(chain)
        return ftot.cpu().numpy(), jac

    def optical_depth_ff_jac(self, freq):
        """Derivatives of the `optical_depth_ff` maps at the model's time with respect to the
        parameters of every ejection event: -> [n_ej, 3, F, n_x, n_z] (axis 1: t_0 [s], peak_jml
        [kg/s], half_life [s]; `n_ej` in the order of `model.ejections`), i.e. ctau[f] dS/dtheta.
        Same requirements as `flux_vs_time_jac`."""
        freqs, (ctau, _) = self._channel_coeffs(freq)
        dev = self._grad_fields()
        slots = self._ejection_slots()
        out = np.zeros((len(slots), 3, len(freqs), self.nx, self.nz))
        if not slots:
            return out
        _, dsumA, _, _ = self.engine.ff_grad(dev, self._rjp_bursts(), [float(self.time)],
                                             self.gff_mode, want_maps=True)
        raw = dsumA.cpu().numpy()[0].reshape(-1, self.nx, self.nz)
        ct = np.asarray(ctau, dtype=np.float64)[:, None, None]
        for i, (k, chain) in enumerate(slots):
            for c in range(3):
                out[i, c] = ct * (raw[k + c] * chain[c])
        return out

    def prepare_epoch_sweeps(self, bins=20):
        """Optional, for a model whose light curves are computed MANY times (e.g. while fitting
        burst parameters): bucket the cells of every sightline by (jet, launch-time bin) once
        (`RTEngine.build_lt`, ~50 ms and ~1.2 x the bytes of two fields for 1e9 cells).  Sweeps of
        12-32 epochs (`flux_vs_time`) then keep their launch-time moments in registers: about a
        quarter faster than the first-sweep path on dense grids.  Returns the layout record; a
        setter that changes the fields (`ts`, `ion_fraction`, `temperature`) invalidates it."""
        return self.engine.build_lt(self.device_fields, int(bins))

    # ------------------------------------------------------------------ RT methods ----
    def emission_measure(self, savefits=False):
        """Emission measure along y [pc cm^-6] (classes.py:1101-1128)."""
        _, em, _ = self._base_maps(want_em=True)
        ems = self._map(em)
        if savefits:
            self.save_fits(np.transpose(ems, (1, 0)), savefits, 'em')
        return ems

    def optical_depth_ff(self, freq, savefits=False, collapse=True):
        """Free-free optical depth along y (classes.py:1353-1447)."""
        if not collapse:
            return self._cells(freq, savefits)
        tff = self._ff_products(freq, tau=True, keep=bool(savefits))
        self._save_cube(tff, savefits, 'tau', freq)
        return tff

    def intensity_ff(self, freq, savefits=False, formal=False):
        """Radio intensity [W m^-2 Hz^-1 sr^-1] (classes.py:1449-1496).  `formal=True`: by the
        formal solution along the line of sight (every cell's emission attenuated by the cells in
        front of it, observer at the iy = 0 end of axis 1) instead of the reference's isothermal
        T_avg (1 - e^-tau); the two agree where T is constant along the sightline."""
        ints = self._ff_products(freq, intensity=True, keep=bool(savefits), formal=formal)
        self._save_cube(ints, savefits, 'intensity', freq, formal=formal)
        return ints

    def flux_ff(self, freq, savefits=False, formal=False):
        """Flux density [Jy/pixel] (classes.py:1498-1541).  `formal`: see `intensity_ff`."""
        fluxes = self._ff_products(freq, flux=True, keep=bool(savefits), formal=formal)
        self._save_cube(fluxes, savefits, 'flux', freq, formal=formal)
        return fluxes

    def _rrl_tau_device(self, rrl, freqs):
        """tau_rrl[F, P] on the device.  The last cube is kept: `Pipeline` asks for the optical
        depths and then for the fluxes of the same line, channels and epoch
        (classes.py:2437, 2450), and the Voigt scan is the expensive kernel."""
        key = (rrl, tuple(float(f) for f in freqs), float(self.time), self._version)
        if self._rrl_cache is not None and self._rrl_cache[0] == key:
            return self._rrl_cache[1]
        line = _lib.Line(**mrrl.line_constants(rrl))
        tau = self.engine.rrl_scan(self._wide_fields(), self._rjp_bursts(), float(self.time),
                                   line, freqs)
        self._rrl_cache = (key, tau)
        return tau

    def optical_depth_rrl(self, rrl, freq, lte=True, savefits=False, collapse=True):
        """RRL optical depth along y (classes.py:1130-1229)."""
        if not collapse:
            return self._cells(freq, savefits, rrl=rrl)
        scalar = np.isscalar(freq)
        freqs = np.atleast_1d(np.asarray(freq, dtype=np.float64))
        dev = self._rrl_tau_device(rrl, freqs)
        tau = self._map(dev, (len(freqs),))
        tau = tau[0] if scalar else tau
        self._dev_product = dev.reshape(len(freqs), self.nx, self.nz) if savefits else None
        self._save_cube(tau, savefits, 'tau', freq)
        return tau

    def _rrl_flux(self, rrl, freq, lte, contsub, intensity=False, formal=False, device=False):
        """`device`: the [F, P] device cube itself, nothing copied to the host."""
        from . import engine as E
        if not lte:
            raise ValueError("Non-LTE RRL calculations not yet supported")   # classes.py:1261
        scalar = np.isscalar(freq)
        freqs = np.atleast_1d(np.asarray(freq, dtype=np.float64))
        F, P = len(freqs), self.nx * self.nz
        if formal:
            # the line by the formal solution (RTEngine.rrl_formal); with contsub=False on top of
            # the formal continuum, which keeps the reference's Rayleigh-Jeans convention
            gv = None
            if self.gff_mode == _lib.RJP_GFF_SCALAR:
                gv = [mphys.gff(nu, self.params['properties']['T_0']) for nu in freqs]
            ctau, _ = E.ff_channel_coeffs(freqs, self.csize, self.params["target"]["dist"],
                                          self.gff_mode, gv)
            cfl, hnu = E.rrl_channel_coeffs(freqs, self.csize, self.params["target"]["dist"])
            if intensity:
                cfl = cfl / (E.solid_angle(self.csize, self.params["target"]["dist"]) / 1e-26)
            add = None
            if not contsub:
                add = self._ff_products(freqs, flux=True, device=True, formal=True).reshape(F, P)
            flux = self.engine.rrl_formal(self._wide_fields(), self._rjp_bursts(),
                                          float(self.time), self.gff_mode,
                                          _lib.Line(**mrrl.line_constants(rrl)), freqs, ctau, cfl,
                                          hnu, add=add)
            if device:
                return flux
            out = self._map(flux, (F,))
            self._dev_product = flux.reshape(F, self.nx, self.nz)
            return out[0] if scalar else out
        tau_rrl = self._rrl_tau_device(rrl, freqs)
        tau_ff = self._ff_products(freqs, tau=True, device=True).reshape(F, P)
        flux_ff = None
        if not contsub:
            flux_ff = self._ff_products(freqs, flux=True, device=True).reshape(F, P)
        cfl, hnu = E.rrl_channel_coeffs(freqs, self.csize, self.params["target"]["dist"])
        if intensity:
            cfl = cfl / (E.solid_angle(self.csize, self.params["target"]["dist"]) / 1e-26)
        flux, _ = self.engine.rrl_maps(tau_rrl, tau_ff, self._model_tavg(), flux_ff, cfl, hnu,
                                       want_ftot=False)
        if device:
            return flux
        out = self._map(flux, (F,))
        self._dev_product = flux.reshape(F, self.nx, self.nz)
        return out[0] if scalar else out

    def intensity_rrl(self, rrl, freq, lte=True, savefits=False, formal=False):
        """RRL intensity [W m^-2 Hz^-1 sr^-1] (classes.py:1231-1290).  Arrays of
        frequencies are handled channel by channel; the reference's own array branch raises
        (it passes the whole array where a scalar is meant, classes.py:1266-1271).
        `formal=True`: by the formal solution along the line of sight (every cell's line emission
        minus its absorption of what lies behind it, observer at the iy = 0 end of axis 1)
        instead of the reference's isothermal B(T_avg) e^-tau_ff (1 - e^-tau_rrl); the two agree
        where T is constant along the sightline, and only the formal one can be negative."""
        ints = self._rrl_flux(rrl, freq, lte, contsub=True, intensity=True, formal=formal)
        self._save_cube(ints, savefits, 'intensity', freq, formal=formal)
        return ints

    def flux_rrl(self, rrl, freq, lte=True, contsub=True, savefits=False, formal=False):
        """RRL flux [Jy/pixel], continuum-subtracted unless contsub=False
        (classes.py:1292-1351).  `formal`: see `intensity_rrl`; with contsub=False the continuum
        added is `flux_ff(formal=True)`."""
        fluxes = self._rrl_flux(rrl, freq, lte, contsub, formal=formal)
        self._save_cube(fluxes, savefits, 'flux', freq, formal=formal)
        return fluxes

    # ------------------------------------------------------------------ visibilities ----
    VIS_STACK_BYTES = 1 << 30    # most bytes of maps one `RTEngine.vis` call of a sweep transforms

    def _vis_scales(self, freqs):
        return vis_scales(freqs, self.csize, self.params["target"]["dist"])

    def _vis_chunk(self, maps_per_epoch):
        """Epochs per chunk of a sweep so that the map stack stays under VIS_STACK_BYTES."""
        per = int(maps_per_epoch) * self.nx * self.nz * 8
        return max(1, self.VIS_STACK_BYTES // per)

    @property
    def _imager(self):
        """`imaging.Imager` on this model's grid, made at every use: VIS_STACK_BYTES as it is then."""
        return Imager(self.engine, self.nx, self.nz, self.csize, self.params["target"]["dist"],
                      self.VIS_STACK_BYTES)

    def _flux_maps(self, freqs, rrl=None, contsub=True, formal=False):
        """The `flux_ff` maps, or with `rrl` the `flux_rrl` maps -> device stack [F, nx * nz]."""
        if rrl is None:
            maps = self._ff_products(freqs, flux=True, device=True, formal=formal)
        else:
            maps = self._rrl_flux(rrl, freqs, True, contsub, formal=formal, device=True)
        return maps.reshape(len(freqs), -1)

    def _model_vis(self, u_m, v_m, freq, weighting=None, maps=True, **which):
        """What the `visibilities_*`, `dirty_*` and `clean_image_*` methods start with -> (the
        imager, V, u_d, v_d, freqs), the last four as its methods take them, on the device: V the
        model visibilities [F, K] of `_flux_maps(freqs, **which)`; None without `maps`."""
        freqs = np.atleast_1d(np.asarray(freq, dtype=np.float64))
        _weighting_mode(weighting)            # (refuses an unknown scheme before any work)
        im = self._imager
        u_d, v_d = im.engine._device_f64(u_m), im.engine._device_f64(v_m)
        V = im.model_vis(self._flux_maps(freqs, **which), freqs, u_d, v_d) if maps else None
        return im, V, u_d, v_d, freqs

    def _observe(self, which, antennalist, freq, t_obs_s, t_int_s, min_el_deg, hourangle_h, *args):
        """`observe_ff` / `observe_rrl`: the tracks and the maps `_flux_maps(freqs, **which)`, then
        `Imager._observe` with `args`, the noise and imaging arguments in its order."""
        freqs = np.atleast_1d(np.asarray(freq, dtype=np.float64))
        tracks = antennalist if isinstance(antennalist, UVTracks) else \
            self.uv_tracks(antennalist, t_obs_s, t_int_s, min_el_deg, hourangle_h)
        return self._imager._observe(self._flux_maps(freqs, **which), freqs, tracks, t_int_s, *args)

    def visibilities_ff(self, u_m, v_m, freq, formal=False):
        """Noise-free model visibilities [Jy] of the `flux_ff` maps at the model's time, at the
        baselines (`u_m`, `v_m`) in metres -> complex array (F, K).  The direct Fourier sum of
        every channel's map at its own (u, v) / lambda (`RTEngine.vis`, rjp_vis; convention:
        `engine.vis_scales` -- phase centre = map centre, RA decreasing with ix); the maps stay on
        the device.  V(0, 0) is the total flux `flux_vs_time` returns.  `formal`: as `flux_ff`.
        Inside a torch.distributed group the call runs on the calling rank only."""
        return self._model_vis(u_m, v_m, freq, formal=formal)[1].cpu().numpy()

    def visibilities_rrl(self, rrl, u_m, v_m, freq, contsub=True, formal=False):
        """Model visibilities [Jy] of the `flux_rrl` maps (same arguments) -> complex (F, K); see
        `visibilities_ff`."""
        V = self._model_vis(u_m, v_m, freq, rrl=rrl, contsub=contsub, formal=formal)[1]
        return V.cpu().numpy()

    def visibilities_vs_time(self, times_s, u_m, v_m, freq, formal=False):
        """Model visibilities [Jy] of the continuum at every (model time, frequency, baseline)
        -> complex array (E, F, K): `visibilities_ff` at each of `times_s` [s], without touching
        `model.time`.  `formal=True`: the maps of one line-of-sight walk per chunk of epochs
        (`RTEngine.ff_formal_sweep`), else the isothermal maps (`prefetch_epochs` + `ff_maps`);
        epochs are processed in chunks whose map stack stays under 1 GiB.  Calling rank only."""
        times = [float(t) for t in np.atleast_1d(np.asarray(times_s, float))]
        freqs = self._channel_coeffs(freq)[0]
        u_d, v_d = self.engine._device_f64(u_m), self.engine._device_f64(v_m)
        out = np.zeros((len(times), len(freqs), int(u_d.numel())), dtype=np.complex128)
        for e0, n, V in _vis_vs_time_chunks(self, times, u_d, v_d, freq, formal):
            out[e0:e0 + n] = V.cpu().numpy().reshape(n, len(freqs), -1)
            del V
        return out

    def visibilities_vs_time_jac(self, times_s, u_m, v_m, freq):
        """The visibilities of `visibilities_vs_time(formal=True)` (bit for bit) AND their exact
        derivatives with respect to the parameters of every ejection event -> (V[E, F, K],
        dV[E, F, n_ej, 3, K]), axis 3 = (t_0 [s], peak_jml [kg/s], half_life [s]), `n_ej` in the
        order of `model.ejections`: the transform is linear, so the derivative maps of
        `RTEngine.ff_formal_grad` go through the same `RTEngine.vis` and `ejection_chain_rule`,
        as `flux_vs_time_jac(formal=True)` does for the totals (dV at u = v = 0 is its Jacobian).
        Chunks of epochs whose derivative maps stay under 1 GiB.  f32 storage raises ValueError;
        a model without ejections returns n_ej = 0.  Calling rank only."""
        if self._dtype != _lib.RJP_F64:
            raise ValueError("burst-parameter sensitivities need f64 storage")
        eng = self.engine
        times = [float(t) for t in np.atleast_1d(np.asarray(times_s, float))]
        freqs, (ctau, cflux) = self._channel_coeffs(freq)
        F = len(freqs)
        u_d, v_d = eng._device_f64(u_m), eng._device_f64(v_m)
        K = int(u_d.numel())
        slots = self._ejection_slots()
        V = self.visibilities_vs_time(times, u_d, v_d, freqs, formal=True)
        dV = np.zeros((len(times), F, len(slots), 3, K), dtype=np.complex128)
        if not times or not slots:
            return V, dV
        bursts = self._rjp_bursts()
        n_par = 3 * (int(bursts.n[0]) + int(bursts.n[1]))
        su, sv = self._vis_scales(freqs)
        su, sv = np.repeat(su, n_par), np.repeat(sv, n_par)
        step = self._vis_chunk(F * n_par)
        for e0 in range(0, len(times), step):
            chunk = times[e0:e0 + step]
            dmaps = eng.ff_formal_grad(self.device_fields, bursts, chunk, self.gff_mode, ctau,
                                       cflux, want_maps=True)[2]
            raw = eng.vis(dmaps.reshape(len(chunk) * F * n_par, -1), self.nx, self.nz,
                          np.tile(su, len(chunk)), np.tile(sv, len(chunk)), u_d, v_d)
            raw = raw.cpu().numpy().reshape(len(chunk), F, n_par, K)
            del dmaps
            for i, (k, chain) in enumerate(slots):
                dV[e0:e0 + len(chunk), :, i] = raw[:, :, k:k + 3] * np.asarray(chain)[:, None]
        return V, dV

    # ------------------------------------------------------------------ dirty images ----
    def dirty_image_ff(self, u_m, v_m, freq, weights=None, shape=None, cell_as=None, formal=False,
                       mfs=False):
        """Dirty images [Jy / beam] of the `flux_ff` maps as an array with the baselines (`u_m`,
        `v_m`) in metres sees them -> float64 (F, ni, nj): `visibilities_ff`'s direct Fourier sum
        followed by its transpose (`RTEngine.vis_adjoint`, rjp_vis_adjoint), no gridding and no
        deconvolution -- what CASA tclean with niter = 0 makes of the simulated measurement set,
        without the measurement set.  `weights` [K]: the imaging weights (None = natural, all
        ones); the image is divided by their sum, so a point source of S Jy at the phase centre
        peaks at S.  `shape` = (ni, nj) and `cell_as` [arcsec] describe the imaging grid (the
        model's own by default; the reference images at a quarter of the beam on >= 500 pixels);
        convention: `engine.image_scales`.  `formal`: as `flux_ff`.  `mfs=True`: the channels go
        into ONE image (1, ni, nj), every channel at its own (u, v) / lambda, as tclean
        specmode='mfs' combines them.  A baseline with a non-finite u, v or weight is flagged.
        Uniform or Briggs weights -- the reference's tclean(weighting='briggs', robust=0.5),
        classes.py:2775-2776 -- come from `weights=Weighting("briggs", robust=0.5, weights=w)`
        (this method's parameter list is fixed; `dirty_image_rrl`, `dirty_beam` and the
        `clean_image_*` methods take `weighting=` and `robust=` instead): the imaging weights are
        computed on the device (`RTEngine.uv_weights`, rjp_uv_weights) from the density of the
        (u, v) points on this image's grid, one density per channel -- with `mfs` one over all
        channels' points --, `w` being the data weights the scheme starts from; a baseline outside
        the grid's Fourier cells (more than half a cycle per cell) or with a negative weight is
        then flagged too.  A plain array, None or scheme "natural" is the natural weighting.
        Calling rank only."""
        weights, weighting, robust = _split_weights(weights)
        im, *vis = self._model_vis(u_m, v_m, freq, weighting, formal=formal)
        return im._dirty_images(*vis, weights, shape, cell_as, mfs, weighting=weighting, robust=robust)

    def dirty_image_rrl(self, rrl, u_m, v_m, freq, weights=None, shape=None, cell_as=None,
                        contsub=True, formal=False, mfs=False, weighting=None, robust=0.5):
        """Dirty images [Jy / beam] of the `flux_rrl` maps (same arguments) -> (F, ni, nj); see
        `dirty_image_ff`.  `weighting`: None / "natural", "uniform" or "briggs" (with `robust`)."""
        im, *vis = self._model_vis(u_m, v_m, freq, weighting, rrl=rrl, contsub=contsub, formal=formal)
        return im._dirty_images(*vis, weights, shape, cell_as, mfs, weighting=weighting, robust=robust)

    def dirty_beam(self, u_m, v_m, freq, weights=None, shape=None, cell_as=None, mfs=False,
                   weighting=None, robust=0.5):
        """The dirty beam (point-spread function) of the (u, v) coverage at every frequency ->
        float64 (F, ni, nj), or (1, ni, nj) with `mfs`: `dirty_image_ff` of visibilities that are
        all 1.  At the centre pixel of an odd-sized grid every phase is exactly 0 and the beam
        is 1 (to the last bit with unit weights); it is symmetric under point reflection.
        `weighting`, `robust`: as `dirty_image_rrl`; the weights are those of an IMAGE on this
        grid."""
        im, _, u_d, v_d, freqs = self._model_vis(u_m, v_m, freq, weighting, maps=False)
        return im._dirty_images(im._unit_vis(len(freqs), int(u_d.numel())), u_d, v_d, freqs, weights,
                                shape, cell_as, mfs, weighting=weighting, robust=robust)

    def imaging_weights(self, u_m, v_m, freq, weights=None, shape=None, cell_as=None,
                        weighting="briggs", robust=0.5, mfs=False):
        """The imaging weights the `dirty_image_*` / `clean_image_*` methods use with these
        arguments -> (float64 host array (F, K), dict): one row per channel (with `mfs` the
        [F, K] weights of the one density over all channels' points), computed on the device
        (`RTEngine.uv_weights`) in chunks of channels that stay under VIS_STACK_BYTES.  The dict
        holds one array [F] (one entry with `mfs`) per statistic: 'sum_w' (the counted data
        weights), 'sum_w2' (sum of the squared density), 'f2' (0 unless Briggs), 'counted',
        'out_of_range', 'shift', 'sum_wout' and 'noise_factor' =
        sqrt(sum(w'^2 / w) sum(w)) / sum(w') over the counted visibilities with w > 0: the
        thermal rms relative to natural weighting, >= 1.  "natural" / None returns the data
        weights with the flagged ones set to 0 and a factor of 1."""
        return self._imager.imaging_weights(u_m, v_m, freq, weights, shape, cell_as, weighting,
                                            robust, mfs)

    # ------------------------------------------------------------------ CLEAN ----
    def clean_image_ff(self, u_m, v_m, freq, weights=None, shape=None, cell_as=None, formal=False,
                       mfs=False, niter=500, gain=0.1, threshold_jy=0.0, mask=None, beam=None,
                       psf_shape=None, imfit=None, weighting=None, robust=0.5, automask=None,
                       scales=None, scale_bias=None, nterms=1, reffreq_hz=None, alpha_cut_jy=None,
                       major_cycles=0, cyclefactor=1.5, cycleniter=None,
                       min_psf_fraction=0.05, max_psf_fraction=0.8):
        """CLEANed, restored images [Jy / clean beam] of the `flux_ff` maps as an array with the
        baselines (`u_m`, `v_m`) in metres sees them: `dirty_image_ff` and `dirty_beam` (same
        arguments, kept on the device), Hogbom's CLEAN of every image with its own beam
        (`RTEngine.clean`, rjp_clean) and the components convolved with a Gaussian clean beam plus
        the residual (`RTEngine.restore`, rjp_restore) -- what the reference gets from CASA tclean
        (classes.py:2770-2808), whose defaults `niter`, `gain`, `threshold_jy` [Jy / beam] are.
        -> `CleanResult`: `image`, `residual`, `model` (F, ni, nj) -- (1, ni, nj) with `mfs` --
        `components` (per map an array [n, 3] of (ix, iz, flux [Jy]) in the order found), `beam`
        (per map (bmaj_as, bmin_as, bpa_deg), convention: `engine.beam_quadratic`) and
        `peak_residual` (per map, the masked max |residual|).
        `mask`: None, a box (i0, i1, j0, j1) of inclusive pixel corners or a boolean (ni, nj)
        array: where components may lie.  `beam`: None = fitted to the main lobe of every map's
        dirty beam (`engine.fit_beam`), or (bmaj_as, bmin_as, bpa_deg).  `psf_shape`: the (odd)
        grid the dirty beam is computed on, None = (2 ni - 1, 2 nj - 1), full Hogbom; smaller =
        the subtraction is windowed.  Everything else as `dirty_image_ff`.  Calling rank only.
        `imfit`: None = no fit; True, or a dict of `box` (i0, i1, j0, j1), `theta0` ([F, 6] or one
        start), `n_iter`, `rms` [Jy / beam] = one elliptical Gaussian is fitted to every restored
        image on the device (`RTEngine.gaussfit`, rjp_gaussfit; start: `engine.gauss_start`) before
        it is copied -- what the reference gets from CASA imfit (classes.py:2790-2840) -- and
        `CleanResult.imfit` holds one dict per map (`engine.gauss_results`).  The default box is
        the bounding box of `mask`, the whole image without one.
        `weighting`: None / "natural" (the path as it was), "uniform" or "briggs" with `robust` --
        the reference's tclean(weighting='briggs', robust=0.5), classes.py:2775-2776: imaging
        weights from the (u, v) density on the IMAGE's grid (`RTEngine.uv_weights`), one density
        per channel (one over all channels with `mfs`), shared by the image and its beam;
        `weights` are the data weights the scheme starts from (see `dirty_image_ff`).
        `scales`: None = Hogbom as above; a list of scale sizes in IMAGE PIXELS, as tclean takes
        `scales` = multi-scale CLEAN (K17: `RTEngine.msclean`, rjp_msclean, with the scale kernels
        of `engine.scale_kernel` applied by `RTEngine.convolve2d`).  Plane 0 is always the delta
        scale (picked only if 0 is among `scales`), the other scales follow ascending; every
        component is a scale kernel of unit sum times its flux, picked by bias x flux with the
        biases `scale_bias` (None = `engine.scale_biases`, 1 - 0.6 s / s_max; else one per plane).
        `components` rows are then (ix, iz, flux [Jy], scale [pixels]), `model` is the sum of the
        scales' delta models convolved with their kernels, `residual` the raw (delta-scale)
        residual, `peak_residual` its masked max, `threshold_jy` bounds the score, and components
        lie at least the largest kernel's half width from the border (ValueError if the mask
        leaves no such pixel).  The kernels carry no prolate-spheroidal taper: not CASA's bits.
        `nterms`: 1 = the path as it was; 2 .. 4 with `mfs` = multi-term MFS CLEAN (K19:
        `RTEngine.mtmfs`, rjp_mtmfs), tclean(deconvolver='mtmfs', nterms=...) at a single scale
        (the reference's Tclean task lists `nterms`, casa/tasks.py:243-246; Sault & Wieringa 1994,
        Rau & Cornwell 2011; this project's definition, no CASA parity).  The sky is I(nu) =
        sum_t I_t w^t, w = (nu - `reffreq_hz`) / `reffreq_hz` (None = the mid-point of the lowest
        and the highest channel); the Taylor dirty images and the spectral beams are the `mfs`
        image of the visibilities times w^t (`engine.taylor_weights`), the Hessian of the beams'
        centres is inverted on the host (`engine.taylor_hessian_inverse`, which refuses a band
        too narrow for `nterms`).  `image` is then tt0, `residual` the raw R_0, `model` the tt0
        delta model, `components` rows (ix, iz, c_0 .. c_{nterms-1}), `peak_residual` and
        `threshold_jy` act on |a_0|, term 0 of the principal solution, and `CleanResult.taylor`
        holds per map `tt`, `residual_tt`, `model_tt` (nterms, ni, nj), `alpha` = tt1 / tt0 where
        tt0 > `alpha_cut_jy` (None = 0.1 of the largest tt0) and NaN elsewhere, `beta` = tt2 / tt0
        - alpha (alpha - 1) / 2 (None below three terms), `alpha_cut_jy`, `reffreq_hz`, `hessian`
        and `hinv`.  Not with `scales` or `major_cycles` (ValueError).
        `major_cycles`: 0 = minor cycles only, as above -- the residual is then the one the minor
        cycles kept in the image plane, the data's only when `psf_shape` is the full window.
        N >= 1 = at most N minor runs, and after every one the residual is recomputed from the
        visibilities: V minus the visibilities of the whole component list (K18:
        `RTEngine.vis_components`, rjp_vis_components), imaged like the dirty image -- tclean's
        major cycles (the reference's Tclean task carries the controls, casa/tasks.py:259-262).
        Every run but the last stops at max(threshold_jy, clip(`cyclefactor` x sidelobe,
        `min_psf_fraction`, `max_psf_fraction`) x the run's peak residual), the last at
        `threshold_jy`; `cycleniter` (None = no limit) bounds the iterations of one run, `niter`
        the whole list.  sidelobe = the largest |dirty beam| in the `psf_shape` window outside
        twice the clean beam's half-power ellipse: this project's definition, not CASA's.
        `residual`, `model`, `image` and `peak_residual` are then functions of the final list and
        the data whatever the window, and `CleanResult.major` holds per map `runs` (dicts `start`,
        `n`, `peak`, `threshold`), `sidelobe` and `vis_residual` (complex [K]; [F K] with `mfs`).
        `automask`: None = the mask is `mask`, as above.  True, or a dict of `sidelobe_threshold`
        (3.0), `noise_threshold` (5.0), `low_noise_threshold` (1.5), `min_beam_frac` (0.3),
        `grow_iterations` (75), `connectivity` (1), `nsigma` (0.0) = every map is cleaned under a
        mask of its own, made on the device from its residual (K25: `RTEngine.image_stats`,
        `label_regions`, `mask_grow`; the convention is `engine.automask_step`) and bounded by
        `mask` -- tclean's usemask='auto-multithresh' without its smoothing, second prune and
        negative threshold; this project's definition, no CASA parity.  Seeds are the pixels above
        max(sidelobe_threshold x sidelobe x peak, median + noise_threshold x sigma), sigma = 1.4826
        x the MAD of the residual outside the mask so far; seed regions smaller than
        `min_beam_frac` of the beam area are dropped and the rest grown `grow_iterations` steps
        inside the pixels above the low threshold.  Without major cycles the mask is made once,
        from the dirty image; with them at the top of every run, and it only grows.  `nsigma` > 0:
        a run also stops at nsigma x that update's sigma (tclean's `nsigma` on a robust noise from
        the residual).  One `RTEngine.clean` call per map instead of one per chunk.
        `CleanResult.automask` holds per map `mask` (bool (ni, nj)) and `runs` (one dict per
        update).  Not with `scales` or `nterms` > 1 (ValueError)."""
        im, *vis = self._model_vis(u_m, v_m, freq, weighting, formal=formal)
        return im._clean_images(*vis, weights, shape, cell_as, mfs, niter, gain, threshold_jy, mask,
                                beam, psf_shape, imfit, weighting=weighting, robust=robust,
                                scales=scales, scale_bias=scale_bias, nterms=nterms, reffreq_hz=reffreq_hz,
                                alpha_cut_jy=alpha_cut_jy, major_cycles=major_cycles,
                                cyclefactor=cyclefactor,
                                cycleniter=cycleniter, min_psf_fraction=min_psf_fraction,
                                max_psf_fraction=max_psf_fraction,
                                # (named only when set: without it the call is the one it was, also for
                                # a stand-in `Imager` with the earlier parameter list)
                                **({} if automask is None else dict(automask=automask)))

    def clean_image_rrl(self, rrl, u_m, v_m, freq, weights=None, shape=None, cell_as=None,
                        contsub=True, formal=False, mfs=False, niter=500, gain=0.1,
                        threshold_jy=0.0, mask=None, beam=None, psf_shape=None, imfit=None,
                        weighting=None, robust=0.5, automask=None, scales=None, scale_bias=None,
                        nterms=1, reffreq_hz=None, alpha_cut_jy=None,
                        major_cycles=0, cyclefactor=1.5, cycleniter=None,
                        min_psf_fraction=0.05, max_psf_fraction=0.8):
        """CLEANed, restored images of the `flux_rrl` maps (same arguments) -> `CleanResult`; see
        `clean_image_ff`."""
        im, *vis = self._model_vis(u_m, v_m, freq, weighting, rrl=rrl, contsub=contsub, formal=formal)
        return im._clean_images(*vis, weights, shape, cell_as, mfs, niter, gain, threshold_jy, mask,
                                beam, psf_shape, imfit, weighting=weighting, robust=robust,
                                scales=scales, scale_bias=scale_bias, nterms=nterms, reffreq_hz=reffreq_hz,
                                alpha_cut_jy=alpha_cut_jy, major_cycles=major_cycles,
                                cyclefactor=cyclefactor,
                                cycleniter=cycleniter, min_psf_fraction=min_psf_fraction,
                                max_psf_fraction=max_psf_fraction,
                                # (named only when set: without it the call is the one it was, also for
                                # a stand-in `Imager` with the earlier parameter list)
                                **({} if automask is None else dict(automask=automask)))

    # ------------------------------------------------------------------ synthetic observations ----
    def uv_tracks(self, antennalist, t_obs_s, t_int_s, min_el_deg=None, hourangle_h=0.):
        """The (u, v, w) tracks of an array observing this model's target -> `UVTracks`: what the
        reference leaves to CASA simobserve (classes.py:2490-2608), without dates.
        `antennalist`: the path of an antenna list (`engine.read_antenna_config`) or an
        `engine.AntennaConfig`.  The target's declination comes from `params['target']`; the
        array's latitude and longitude are those of its mean position (`engine.geodetic`); the
        integrations are those of `engine.observing_plan` for `t_obs_s` seconds on source in
        integrations of `t_int_s`, every day centred on the LOCAL hour angle `hourangle_h`, and
        the Greenwich hour angle is the local one minus the east longitude.  `min_el_deg`: the
        elevation limit -- it sets the time per day the target is up, and a baseline with an
        antenna below it (by that antenna's own vertical) is NaN in u, v and w, the flag every
        imaging method honours; None = the horizon for the plan and no flags.
        `u_m`, `v_m`, `w_m`: float64 DEVICE tensors [n_t * n_bl], visibility k = t n_bl + b
        (`RTEngine.uv_tracks`, rjp_uv_tracks); `ha_h` [n_t] (hours) and `day` [n_t]: host arrays
        per integration; `ant1`, `ant2` [n_bl]: the antennas of baseline b = xyz[ant2] -
        xyz[ant1]; `max_baseline_m`.  Calling rank only."""
        tg = self.params['target']
        return self._imager.uv_tracks(antennalist, miscf.sexagesimal_to_deg(tg['ra'], tg['dec'])[1],
                                      t_obs_s, t_int_s, min_el_deg, hourangle_h)

    def observe_ff(self, antennalist, freq, t_obs_s, t_int_s, min_el_deg=None, hourangle_h=0.,
                   sigma_jy=None, sefd_jy=None, chanwidth_hz=None, seed=0, nsigma=0.,
                   weights=None, shape=None, cell_as=None, formal=False, mfs=False, niter=500,
                   gain=0.1, threshold_jy=0.0, mask=None, beam=None, psf_shape=None, imfit=None,
                   weighting=None, robust=0.5, automask=None, scales=None, scale_bias=None,
                   nterms=1, reffreq_hz=None, alpha_cut_jy=None, major_cycles=0,
                   cyclefactor=1.5, cycleniter=None, min_psf_fraction=0.05, max_psf_fraction=0.8):
        """A synthetic observation of the `flux_ff` maps, start to end on the device -- the
        reference's simobserve -> tclean -> imfit chain (classes.py:2490-2850) -> `Observation`:
        `tracks` (`uv_tracks` of `antennalist`, `t_obs_s`, `t_int_s`, `min_el_deg`,
        `hourangle_h`; a `UVTracks` made earlier is taken as it is), `vis_clean` (complex host
        array (F, K), `visibilities_ff` at the tracks; NaN at flagged baselines), `vis` (the same
        plus thermal noise: `RTEngine.vis_noise`, rjp_vis_noise, keyed by `seed`; channel f is
        map f and visibility k = t n_bl + b of the counter, so every day, integration, baseline
        and channel has its own draw and a seed reproduces the bits), `sigma` [F] (the rms [Jy]
        of the real and of the imaginary part of one visibility), `image_rms` (per image,
        `engine.image_rms` of the imaging weights actually used; 0 without noise) and `clean`
        (the `CleanResult` of the NOISY visibilities, every imaging keyword as `clean_image_ff`).
        Noise: `sigma_jy` (one rms or one per channel), or `sefd_jy` with `chanwidth_hz`
        (`engine.thermal_sigma` at `t_int_s`, two polarisations); neither = noise-free, and the
        result equals `clean_image_ff` at the same tracks bit for bit.  `nsigma` > 0: the CLEAN
        threshold of every image is max(threshold_jy, nsigma image_rms), tclean's `nsigma` with
        the analytic rms in place of CASA's robust estimate.  With `imfit` and noise, `image_rms`
        is the fit's default `rms`.  Calling rank only."""
        _weighting_mode(weighting)            # (refuses an unknown scheme before any work)
        return self._observe(dict(formal=formal), antennalist, freq, t_obs_s, t_int_s, min_el_deg,
                             hourangle_h, sigma_jy, sefd_jy, chanwidth_hz, seed, nsigma, weights,
                             shape, cell_as, mfs, niter, gain, threshold_jy, mask, beam, psf_shape,
                             imfit, weighting, robust, automask, scales, scale_bias, nterms,
                             reffreq_hz, alpha_cut_jy, major_cycles, cyclefactor, cycleniter,
                             min_psf_fraction, max_psf_fraction)

    def observe_rrl(self, rrl, antennalist, freq, t_obs_s, t_int_s, min_el_deg=None,
                    hourangle_h=0., sigma_jy=None, sefd_jy=None, chanwidth_hz=None, seed=0,
                    nsigma=0., weights=None, shape=None, cell_as=None, contsub=True, formal=False,
                    mfs=False, niter=500, gain=0.1, threshold_jy=0.0, mask=None, beam=None,
                    psf_shape=None, imfit=None, weighting=None, robust=0.5, automask=None,
                    scales=None, scale_bias=None, nterms=1, reffreq_hz=None, alpha_cut_jy=None,
                    major_cycles=0, cyclefactor=1.5, cycleniter=None,
                    min_psf_fraction=0.05, max_psf_fraction=0.8):
        """A synthetic observation of the `flux_rrl` maps -> `Observation`; see `observe_ff`."""
        _weighting_mode(weighting)            # (refuses an unknown scheme before any work)
        return self._observe(dict(rrl=rrl, contsub=contsub, formal=formal), antennalist, freq,
                             t_obs_s, t_int_s, min_el_deg, hourangle_h, sigma_jy, sefd_jy,
                             chanwidth_hz, seed, nsigma, weights, shape, cell_as, mfs, niter, gain,
                             threshold_jy, mask, beam, psf_shape, imfit, weighting, robust,
                             automask, scales, scale_bias, nterms, reffreq_hz, alpha_cut_jy,
                             major_cycles, cyclefactor, cycleniter, min_psf_fraction,
                             max_psf_fraction)

    # ------------------------------------------------------------------ imstat, automask ----
    def imstat(self, images, mask=None, inside=True):
        """Robust statistics of each of `images` -- (F, ni, nj) or (ni, nj), a host array or a
        device tensor, such as a `CleanResult.residual` -- on the device (`RTEngine.image_stats`,
        rjp_image_stats) -> list of dicts, one per image (`engine.image_stats_results`): `npts`,
        `min`, `max`, `median` (the lower median), `medabsdevmed`, `sigma_robust`, `sum`, `mean`,
        `rms`, `sigma`, over the finite pixels.  `mask`: None, or (ni, nj) / (F, ni, nj), non-zero
        = set: the pixels inside it count, with `inside=False` those outside.  Calling rank only."""
        return self._imager.imstat(images, mask, inside)

    def automask(self, images, beam, sidelobe=0., mask=None, prev=None, **options):
        """One update of the automatic clean mask for images already made -> (masks bool
        (F, ni, nj), info: one dict per image); see the `automask` keyword of `clean_image_ff`,
        whose options `options` are.  `beam`: the clean beam (bmaj_as, bmin_as, bpa_deg), one or
        one per image; `sidelobe`: the beam's sidelobe level, one or one per image
        (`CleanResult.major[m]['sidelobe']`); `mask`: None or (ni, nj), what bounds the automatic
        mask; `prev`: None or (F, ni, nj), the masks so far.  Calling rank only."""
        return self._imager.automask(images, beam, sidelobe, mask, prev, options)

    # ------------------------------------------------------------------ imfit ----
    def imfit(self, images, beam, cell_as=None, box=None, theta0=None, n_iter=60, rms=None):
        """One elliptical Gaussian fitted to each of `images` -- (F, ni, nj) or (ni, nj), a host
        array or a device tensor, such as a `CleanResult.image` -- on the device
        (`RTEngine.gaussfit`) -> list of dicts, one per image (`engine.gauss_results`); what the
        reference gets from CASA imfit (classes.py:2790-2840).  `beam`: the clean beam
        (bmaj_as, bmin_as, bpa_deg), one or one per image (`CleanResult.beam`); `cell_as`: the
        cell in arcsec, None = the model's; `box`, `theta0`, `n_iter`, `rms` as the `imfit`
        keyword of `clean_image_ff`.  Calling rank only."""
        return self._imager.imfit(images, beam, cell_as, box, theta0, n_iter, rms)

    # ------------------------------------------------------------------ uvmodelfit ----
    def uvmodelfit(self, vis, u_m, v_m, freq, weights=None, cell_as=None, comps=1, comptype=None,
                   theta0=None, free=None, mfs=False, n_iter=60):
        """Point / elliptical-Gaussian components fitted to the visibilities `vis` -- (F, K)
        complex, a host array or a device tensor, such as `Observation.vis` -- in the uv plane on
        the device (`RTEngine.uvfit`, rjp_uvfit) -> one list of component dicts per channel
        (`engine.uvfit_results`): what radio astronomers get from CASA uvmodelfit or difmap
        modelfit; no weighting scheme, CLEAN or beam enters.  `u_m`, `v_m` [K]: baselines in
        metres; `freq`: the F channels; `weights`: None, [K] or [F, K], the data weights (1 /
        sigma^2 makes the errors exact); `cell_as`: the cell the parameters are counted in, None =
        the model's; `comps`: 1 or 2 components; `comptype`: None (Gaussians) or 'G' / 'P' per
        component, a 'P' being a point whose sizes are held at 0; `theta0`: the start, [6 comps]
        or [F, 6 comps] (`engine.uvfit_theta` builds a component), None = `engine.uvfit_start`
        (one component only); `free`: None or 6 comps flags, one pattern for all channels (a
        cleared flag holds the parameter at its start); `mfs=True`: ONE model for all channels --
        they are concatenated into one set of F K visibilities with the baselines in cycles per
        cell -- and one list is returned.  Nothing goes to the host before the fit ends.  Calling
        rank only."""
        return self._imager.uvmodelfit(vis, u_m, v_m, freq, weights, cell_as, comps, comptype,
                                       theta0, free, mfs, n_iter)

    def uvmodelfit_ff(self, u_m, v_m, freq, formal=False, weights=None, cell_as=None, comps=1,
                      comptype=None, theta0=None, free=None, mfs=False, n_iter=60):
        """`uvmodelfit` of the model's own noise-free `visibilities_ff` (same bits), which stay on
        the device.  `formal`: as `flux_ff`.  Calling rank only."""
        im, V, u_d, v_d, freqs = self._model_vis(u_m, v_m, freq, formal=formal)
        return im.uvmodelfit(V, u_d, v_d, freqs, weights, cell_as, comps, comptype, theta0, free,
                             mfs, n_iter)

    def uvmodelfit_vs_time(self, times_s, u_m, v_m, freq, formal=False, weights=None, cell_as=None,
                           comps=1, comptype=None, theta0=None, free=None, n_iter=60):
        """`uvmodelfit` of `visibilities_vs_time` at every (model time, frequency) -> results
        indexed [E][F][component]: one `RTEngine.uvfit` call per chunk of epochs, the
        visibilities staying on the device -- the proper motion of a knot from a sweep of epochs.
        `theta0`: None, one start [6 comps] or one per (epoch, channel) [E, F, 6 comps]; `weights`:
        None, [K] or [F, K]; the other arguments as `uvmodelfit`.  Calling rank only."""
        import torch
        im = self._imager
        eng = im.engine
        times = [float(t) for t in np.atleast_1d(np.asarray(times_s, float))]
        freqs = np.atleast_1d(np.asarray(freq, dtype=np.float64))
        F = len(freqs)
        nc, fr, point = im._uvfit_options(comps, comptype, theta0, free)
        cell = im._image_grid(None, cell_as)[2]
        su, sv = image_scales(freqs, cell)
        u_d, v_d = eng._device_f64(u_m), eng._device_f64(v_m)
        K = int(u_d.numel())
        w_d = eng._device_f64(weights) if weights is not None else None
        if w_d is not None and w_d.numel() not in (K, F * K):
            raise ValueError("uvmodelfit: `weights` must be [K] or [F, K] = [%d, %d]" % (F, K))
        th = None
        if theta0 is not None:
            th = theta0 if isinstance(theta0, torch.Tensor) else \
                torch.from_numpy(np.ascontiguousarray(theta0, dtype=np.float64))
            th = th.to(eng.device)
            if th.dim() not in (1, 3) or (th.dim() == 3 and
                                          tuple(th.shape[:2]) != (len(times), F)):
                raise ValueError("uvmodelfit_vs_time: `theta0` must be [6 comps] or [E, F, 6 comps]")
        out = []
        for e0, n, V in _vis_vs_time_chunks(self, times, u_d, v_d, freqs, formal):
            w_c = w_d.reshape(F, K).repeat(n, 1) if w_d is not None and w_d.numel() == F * K and \
                F > 1 else w_d
            th_c = th[e0:e0 + n].reshape(n * F, -1) if th is not None and th.dim() == 3 else th
            res = im._uvfit_stack(V, np.tile(su, n), np.tile(sv, n), u_d, v_d, w_c, th_c, fr,
                                  point, int(n_iter), cell)[0]
            out += [res[i * F:(i + 1) * F] for i in range(n)]
            del V
        return out

    # ------------------------------------------------------------------ spectral axis ----
    def _rrl_velocity_axis(self, rrl, freq):
        element, n, dn = mrrl.rrl_parser(rrl)
        return velocity_axis(freq, mrrl.rrl_nu_0(element, n, dn))

    def moments(self, cube, x, dx=None, clip=0., mask=None):
        """Moment maps of any line cube `cube` -- (F, ni, nj), a host array or a device tensor,
        such as `clean_image_rrl(...).image` -- along its axis `x` [F] on the device
        (`RTEngine.cube_moments`, rjp_cube_moments) -> dict of device tensors (ni, nj): 'm0' (the
        integrated line, sum y dx), 'm1' (the intensity-weighted axis value: the velocity field),
        'm2' (the intensity-weighted dispersion: the line width), 'peak', 'ipeak', 'count' -- what
        radio astronomers get from CASA immoments.  `dx`: the channel widths, None = half the
        distance between the neighbours (`engine.velocity_axis`); `clip`: only channels with |y|
        >= clip count; `mask`: None or (ni, nj), non-zero = live.  Calling rank only."""
        return Spectra(self.engine).moments(cube, x, dx, clip, mask)

    def specfit(self, cube, x, weights=None, comps=1, theta0=None, free=None, n_iter=40,
                mask=None, scale_errors=True):
        """One or two Gaussians plus a linear baseline fitted to every sightline of any line cube
        (as `moments`) on the device (`RTEngine.specfit`, rjp_specfit) -> dict of device tensors
        (ni, nj) (`engine.specfit_results`: 'peak', 'centre', 'sigma', 'fwhm', 'integral' and
        their 'e_*' errors per component, 'b0', 'b1', 'chi2', 'reduced_chi2', 'nchan', 'status',
        'niter') -- what radio astronomers get from CASA specfit.  `weights`: None or [F], 1 /
        sigma^2 per channel (for `sigma` per channel pass `sigma ** -2` and scale_errors=False);
        `comps`: 1 or 2; `theta0`: the start, [P] or [P, ni * nj], P = 3 comps + 2, None = from the
        moments (`engine.specfit_start`, one component only); `free`: None or P flags, one pattern
        for all pixels.  Calling rank only."""
        return Spectra(self.engine).specfit(cube, x, weights, comps, theta0, free, n_iter, mask,
                                            scale_errors)

    def moments_rrl(self, rrl, freq, contsub=True, formal=False, clip_jy=0.):
        """`moments` of the model's own `flux_rrl` cube (same arguments), which stays on the
        device, along the radio velocity axis of the line [km/s] (`engine.velocity_axis` about
        `maths.rrls.rrl_nu_0`): 'm0' in Jy km/s per pixel, 'm1' and 'm2' in km/s.  Calling rank
        only."""
        v, dv = self._rrl_velocity_axis(rrl, freq)
        cube = self._flux_maps(np.atleast_1d(np.asarray(freq, dtype=np.float64)), rrl=rrl,
                               contsub=contsub, formal=formal)
        return Spectra(self.engine).moments(cube.reshape(len(v), self.nx, self.nz), v, dv, clip_jy)

    def specfit_rrl(self, rrl, freq, contsub=True, formal=False, weights=None, comps=1,
                    theta0=None, free=None, n_iter=40):
        """`specfit` of the model's own `flux_rrl` cube (same arguments), which stays on the
        device, along the radio velocity axis of the line [km/s].  With contsub=True and
        free=None the baseline is held at 0.  Calling rank only."""
        v, _ = self._rrl_velocity_axis(rrl, freq)
        cube = self._flux_maps(np.atleast_1d(np.asarray(freq, dtype=np.float64)), rrl=rrl,
                               contsub=contsub, formal=formal)
        if free is None and contsub:
            free = [1] * (3 * int(comps)) + [0, 0]
        return Spectra(self.engine).specfit(cube.reshape(len(v), self.nx, self.nz), v, weights,
                                            comps, theta0, free, n_iter)

    def voigtfit(self, cube, x, weights=None, comps=1, theta0=None, free=None, n_iter=40,
                 mask=None, scale_errors=True):
        """One or two Voigt profiles plus a linear baseline fitted to every sightline of any line
        cube (as `moments`) on the device (`RTEngine.voigtfit`, rjp_voigtfit) -> dict of device
        tensors (ni, nj) (`engine.voigt_results`: 'integral', 'centre', 'sigma', 'fwhm_g',
        'hwhm_l', 'fwhm_l', 'peak', 'fwhm' and their 'e_*' errors per component, 'b0', 'b1',
        'chi2', 'reduced_chi2', 'nchan', 'status', 'niter'): the Doppler width gives T, the
        Lorentz width n_e.  Arguments as `specfit`'s with P = 4 comps + 2 parameters (F, x0, s, g
        per component, b0, b1); `theta0` None = `engine.voigt_start` (one component only).
        Calling rank only."""
        return Spectra(self.engine).voigtfit(cube, x, weights, comps, theta0, free, n_iter, mask,
                                             scale_errors)

    def voigtfit_rrl(self, rrl, freq, quantity="flux", contsub=True, formal=False, weights=None,
                     comps=1, theta0=None, free=None, n_iter=40):
        """`voigtfit` of one of the model's own cubes of the line `rrl` over the channels `freq`,
        which stays on the device, along the radio velocity axis of the line [km/s].
        quantity="flux": the `flux_rrl` cube (`contsub`, `formal` as there); quantity="tau": the
        line's optical-depth cube (no flux is computed) -- tau(nu) of a thin uniform sightline is
        one exact Voigt profile, so the fitted widths mean something there.  With free=None the
        baseline is held at 0 for "tau" and for a continuum-subtracted "flux".  Calling rank
        only."""
        if quantity not in ("flux", "tau"):
            raise ValueError("voigtfit_rrl: `quantity` must be 'flux' or 'tau'")
        v, _ = self._rrl_velocity_axis(rrl, freq)
        freqs = np.atleast_1d(np.asarray(freq, dtype=np.float64))
        if quantity == "tau":
            cube = self._rrl_tau_device(rrl, freqs)
        else:
            cube = self._flux_maps(freqs, rrl=rrl, contsub=contsub, formal=formal)
        if free is None and (quantity == "tau" or contsub):
            free = [1] * (4 * int(comps)) + [0, 0]
        return Spectra(self.engine).voigtfit(cube.reshape(len(v), self.nx, self.nz), v, weights,
                                             comps, theta0, free, n_iter)

    # ------------------------------------------------------------------ antenna gains (K22) ----
    def corrupt_gains(self, vis, tracks, gains, h_sol):
        """The visibilities `vis` -- (F, K) complex, a host array or a device tensor in the order
        of `tracks` (`uv_tracks`), such as `observe_ff(...).vis` -- times antenna gains: V_pq g_p
        conj(g_q) (`RTEngine.gain_apply`, rjp_gain_apply) -> complex128 device tensor (F, K); what
        CASA simobserve's `corrupt` does for gains.  `gains`: complex (n_sol, n_ant), shared by the
        channels, or (F, n_sol, n_ant) (`engine.random_gains` draws some); `h_sol` [n_t]: the
        interval of every integration (`engine.solution_intervals`).  A NaN gain flags the
        visibilities of its antenna.  Calling rank only."""
        return Calibrator(self.engine).corrupt(vis, tracks, gains, h_sol)

    def gaincal(self, vis, model_vis, tracks, solint_s="int", calmode="ap", refant=0,
                minblperant=4, weights=None, tol=1e-10, n_iter=300):
        """Antenna gains per channel and solution interval that bring `model_vis` to `vis` (both
        (F, K) as in `corrupt_gains`; `model_vis` may be (1, K)), D_pq = g_p conj(g_q) M_pq, by
        StefCal on the device (`RTEngine.gaincal`, rjp_gaincal: one launch iterates every
        (channel, interval) to the end) -> (gains, results): complex128 device tensor (F, n_sol,
        n_ant), NaN for an antenna without a solution, and `engine.gain_results` (device tensors
        'amp', 'phase_deg', 'live', 'status', 'chi2_start', 'chi2', 'nvis', 'niter') plus 'h_sol',
        the host interval table to apply them with -- what radio astronomers get from CASA gaincal.
        `solint_s`: seconds, 'int' or 'inf' (`engine.solution_intervals`; never across two days);
        `calmode`: 'ap' or 'p' (phase only); `refant`: the antenna of phase 0; `minblperant`: an
        antenna with fewer baselines with data in an interval gets no solution there; `weights`:
        None, [K] or [F, K]; status 1 converged (`tol`, relative), 0 `n_iter` exhausted, 2 broken
        down, 3 too few antennas.  This project's definition, no CASA parity.  Calling rank only."""
        return Calibrator(self.engine).gaincal(vis, model_vis, tracks, solint_s, calmode, refant,
                                               minblperant, weights, tol, n_iter)

    def applycal(self, vis, tracks, gains, h_sol):
        """`vis` corrected by antenna gains, V_pq / (g_p conj(g_q)) (arguments and result as
        `corrupt_gains`, whose inverse it is) -- CASA applycal.  Calling rank only."""
        return Calibrator(self.engine).applycal(vis, tracks, gains, h_sol)

    def selfcal_ff(self, vis, tracks, freq, rounds=(dict(solint_s="inf", calmode="p"),),
                   **clean_kwargs):
        """Self-calibration of the visibilities `vis` (F, K) at the channels `freq` -> `SelfcalResult`
        (`clean`, `vis`, `gains`, `history`).  Every round -- a dict of `gaincal`'s keywords --
        CLEANs the current data as `clean_image_ff` does (keywords `weights`, `shape`, `cell_as`,
        `mfs`, `niter`, `gain`, `threshold_jy`, `mask`, `beam`, `psf_shape`, `weighting`,
        `robust`), forms the visibilities of the component list (`RTEngine.vis_components`),
        solves `gaincal` of the current data against them and corrects the ORIGINAL data by the
        product of all gains so far; `clean` is one more CLEAN, of the corrected data `vis`.
        `gains`: complex128 device tensor (F, n_t, n_ant), the product per integration (apply
        with h_sol = arange(n_t)); `history`: per round 'peak_residual' of its CLEAN, 'chi2_start'
        and 'chi2' summed over the solved solutions, 'status' (how many solutions ended with
        each).  An antenna without a solution flags its data.  Calling rank only."""
        return Calibrator(self.engine, self._imager).selfcal(vis, tracks, freq, list(rounds),
                                                             **clean_kwargs)

    # ------------------------------------------------------------------ burst fits (K23) ----
    def fit_ejections_flux(self, times_s, freq, flux, sigma=None, formal=False, free=None, tie=None,
                           theta0=None, n_iter=30, lambda0=1e-3, xtol=1e-8, update=False,
                           trace=False):
        """The (t_0 [s], peak_jml [kg/s], half_life [s]) of every entry of `model.ejections`
        fitted to the light curves `flux` (E, F) [Jy] at `times_s` [s] and `freq` -- the mass-loss
        history behind multi-epoch fluxes -> `EjectionFit`.  Levenberg-Marquardt on the host
        (`inference.lm_minimise`, the rule of the device fits) around the exact derivatives of
        `flux_vs_time_jac` (`formal`: as there), reduced to normal equations on the device
        (`RTEngine.normal_eq`, rjp_normal_eq); a rejected trial costs one sweep and no
        derivatives.  `sigma`: None, a number or (E, F), the errors of `flux` (weights 1 /
        sigma^2); a NaN flux is skipped.  `free`, `tie`, `theta0`: `BurstFit.layout` -- `free`
        None (all), boolean [n_ej, 3] or {key: names}: of a named ejection only these are fitted; `tie` groups of
        (key, name) sharing one fit value (tie the two halves of an 'RB' event: a light curve
        cannot separate them); `theta0` the start, None = the model's values.  Feasible:
        everything finite, peak_jml > 0, half_life > 0.  Result: `ejections` (like
        `model.ejections`, plus e_t_0, e_peak_jml, e_half_life: sqrt(diag N^-1 x reduced chi^2)),
        `theta` [n_ej, 3], `cov` = N^-1 over the free fit parameters (exact for weights 1 /
        sigma^2), `chi2`, `reduced_chi2`, `ndata`, `status` (1 converged: the step below `xtol`
        of half_life, |peak_jml|, half_life; 0 `n_iter` trials; 2 stalled; 3 an infeasible start
        or too few data: nothing fitted), `niter`, `trace`.  The model is not touched during the
        fit; `update` writes the result back (`set_ejection_event`).  A model without ejections
        or with f32 storage raises ValueError.  Calling rank only."""
        return BurstFit(self).fit_flux(times_s, freq, flux, sigma, formal, free, tie, theta0,
                                       n_iter, lambda0, xtol, update, trace)

    def fit_ejections_vis(self, times_s, u_m, v_m, freq, vis, weights=None, free=None, tie=None,
                          theta0=None, n_iter=30, lambda0=1e-3, xtol=1e-8, update=False,
                          trace=False):
        """As `fit_ejections_flux`, to visibilities `vis` (E, F, K) complex [Jy] (host array or
        device tensor) at the baselines `u_m`, `v_m` [m]: [K] shared by the epochs, or [E, K] when
        every epoch has its own coverage (pad with weight 0; one `RTEngine.vis` call per epoch
        then).  Formal solution only, as `visibilities_vs_time_jac`, whose model and derivatives
        these are: chunks of epochs whose derivative maps stay under 1 GiB go through
        `ff_formal_grad(want_maps=True)`, `vis` and `normal_eq`; no map, visibility or derivative
        goes to the host.  `weights`: None, [K], [E, K] or [E, F, K]; a visibility with a NaN part
        or a weight that is not finite and positive is skipped.  Calling rank only."""
        return BurstFit(self).fit_vis(times_s, u_m, v_m, freq, vis, weights, free, tie, theta0,
                                      n_iter, lambda0, xtol, update, trace)

    # ------------------------------------------------------------------ products ----
    FORMAL_HISTORY ="Formal solution along the line of sight, observer at iy = 0"

    def _save_cube(self, data, savefits, image_type, freq, formal=False):
        dev, self._dev_product = getattr(self, "_dev_product", None), None
        if not savefits:
            return
        if (dev is not None and np.ndim(data) == 3 and tuple(dev.shape) == np.shape(data) and
                dev.numel() * 8 >= self.FITS_DEVICE_MIN_BYTES):
            # (F, n_x, n_z) -> FITS order (F, dec = z, ra = x), big-endian, on the GPU: the
            # host only receives the bytes and writes them
            import torch
            t = dev.transpose(1, 2).contiguous()
            be = t.view(torch.uint8).reshape(-1, 8).flip(1).contiguous()
            arr = _fits.BigEndian(t.shape, _to_host(be.reshape(-1)))
        elif np.ndim(data) == 3:
            # views, not copies: the writer lays the bytes out in one pass
            arr = np.transpose(data, (0, 2, 1))
        else:
            arr = np.transpose(data, (1, 0))
        self.save_fits(arr, savefits, image_type, freq,
                       history=self.FORMAL_HISTORY if formal else None)

    def save_fits(self, data, filename, image_type, freq=None, history=None):
        """Write a map/cube with the reference's header (classes.py:1543-1652); `history`: one
        more HISTORY line (the formal-solution products say so)."""
        if image_type not in ('flux', 'tau', 'em', 'intensity'):
            raise ValueError("arg image_type must be one of 'flux', 'tau' or 'em'")
        ndims = len(data.shape if isinstance(data, _fits.BigEndian) else np.shape(data))
        if ndims not in (2, 3):
            raise ValueError(f"Unexpected number of data dimensions ({ndims})")
        tg = self.params['target']
        _, dec_deg = miscf.sexagesimal_to_deg(tg['ra'], tg['dec'])
        # astropy's hourangle -> degree scale factor is (15 pi/180)/(pi/180), not a literal 15
        ra_deg = miscf.parse_sexagesimal(tg['ra']) * ((15. * (np.pi / 180.)) / (np.pi / 180.))
        csize_deg = np.degrees(np.arctan(self.csize * con.au / (tg['dist'] * con.parsec)))
        h = _fits.Header()
        h.set('AUTHOR', 'S.J.D.Purser')
        h.set('OBJECT', tg['name'])
        h.set('CTYPE1', 'RA---TAN', 'x-coord type is RA Tan Gnomonic projection')
        h.set('CTYPE2', 'DEC--TAN', 'y-coord type is DEC Tan Gnomonic projection')
        h.set('EQUINOX', 2000., 'Equinox of coordinates')
        h.set('CRPIX1', self.nx / 2 + 0.5, 'Reference pixel in RA')
        h.set('CRPIX2', self.nz / 2 + 0.5, 'Reference pixel in DEC')
        h.set('CRVAL1', ra_deg, 'Reference pixel value in RA (deg)')
        h.set('CRVAL2', dec_deg, 'Reference pixel value in DEC (deg)')
        h.set('CDELT1', -csize_deg, 'Pixel increment in RA (deg)')
        h.set('CDELT2', csize_deg, 'Pixel size in DEC (deg)')
        if image_type in ('flux', 'tau', 'intensity'):
            if ndims == 3:
                nchan = len(freq)
                chan_width = float(freq[1] - freq[0]) if nchan != 1 else 1.
                h.set('CTYPE3', 'FREQ', 'Spectral axis (frequency)')
                h.set('CRPIX3', nchan / 2. + 0.5, 'Reference frequency (channel number)')
                h.set('CRVAL3', float(freq[len(freq) // 2 - 1] + chan_width / 2),
                      'Reference frequency (Hz)')
                h.set('CDELT3', chan_width, 'Frequency increment (Hz)')
            else:
                f0 = float(freq[0]) if not np.isscalar(freq) else float(freq)
                h.set('CDELT3', 1., 'Frequency increment (Hz)')
                h.set('CRPIX3', 0.5, 'Reference frequency (channel number)')
                h.set('CRVAL3', f0, 'Reference frequency (Hz)')
        h.set('BUNIT', {'flux': 'Jy pixel^-1', 'intensity': 'W m^-2 Hz^-1 sr^-1',
                        'em': 'pc cm^-6', 'tau': 'dimensionless'}[image_type])
        lines = self.__str__().split('\n')
        h.add_history((' ' * (72 - len(lines[0]))).join(lines))
        if history is not None:
            h.add_history(history)
        _fits.writeto(filename, data, h)

    def save(self, filename):
        """Pickle the model state (classes.py:1704-1713).  The grids themselves are not
        stored: they are rebuilt on the GPU in milliseconds."""
        ps = {'params': self._params, 'areas': None, 'ffs': None, 'time': self.time,
              'log': self.log, 'storage': 'f64' if self._dtype == _lib.RJP_F64 else 'f32'}
        self.log.add_entry("INFO", "Saving physical model to {}".format(filename))
        with open(filename, "wb") as f:
            pickle.dump(ps, f)


class ContinuumRun:
    """One (epoch, frequency band) radiative-transfer run (classes.py:1716-1900)."""

    def __init__(self, dcy, year, freq=None, bandwidth=None, chanwidth=None, t_obs=None,
                 t_int=None, tscop=None):
        self._year, self._dcy, self._obs_type = year, dcy, 'continuum'
        self._freq, self._t_obs, self._t_int, self._tscop = freq, t_obs, t_int, tscop
        self._products, self._results = {}, {}
        self._bandwidth = bandwidth if bandwidth is not None else 1.
        self._chanwidth = chanwidth if chanwidth is not None else 1.
        self.completed = False
        self.radiative_transfer = freq is not None
        self.simobserve = all(v is not None for v in (tscop, bandwidth, chanwidth, t_obs,
                                                      t_int))

    line = None

    def _row(self):
        val = [self._year, self._obs_type.capitalize(), self._tscop, self._t_obs, self._t_int,
               self.line, self._freq, self._bandwidth, self._chanwidth,
               self.radiative_transfer, self.simobserve, self.completed]
        return ['-' if v is None else v for v in val]

    def __str__(self):
        return _run_table([self._row()], "grid")

    @property
    def results(self):
        return self._results

    @results.setter
    def results(self, new_results):
        if not isinstance(new_results, dict):
            raise TypeError("setter method for results attribute requires dict")
        self._results = new_results

    @property
    def products(self):
        return self._products

    @products.setter
    def products(self, new_products):
        if not isinstance(new_products, dict):
            raise TypeError("setter method for products attribute requires dict")
        self._products = new_products

    obs_type = property(lambda self: self._obs_type)
    year = property(lambda self: self._year)
    freq = property(lambda self: self._freq)
    bandwidth = property(lambda self: self._bandwidth)
    chanwidth = property(lambda self: self._chanwidth)
    t_obs = property(lambda self: self._t_obs)
    t_int = property(lambda self: self._t_int)
    tscop = property(lambda self: self._tscop)

    @property
    def dcy(self):
        return self._dcy

    @dcy.setter
    def dcy(self, path):
        self._dcy = path

    @property
    def day(self):
        return int(self.year * 365.)

    @property
    def model_dcy(self):
        return os.sep.join([self.dcy, f'Day{self.day}'])

    def _tag(self):
        return miscf.freq_str(self.freq)

    @property
    def rt_dcy(self):
        if not self.radiative_transfer:
            return None
        return os.sep.join([self.model_dcy, self._tag()])

    def _fits(self, kind):
        return self.rt_dcy + os.sep + '_'.join([kind, 'Day' + str(self.day),
                                                self._tag()]) + '.fits'

    fits_flux = property(lambda self: self._fits('Flux'))
    fits_tau = property(lambda self: self._fits('Tau'))
    fits_em = property(lambda self: self._fits('EM'))

    @property
    def nchan(self):
        return int(self.bandwidth / self.chanwidth)

    @property
    def chan_freqs(self):
        chan1 = self.freq - self.bandwidth / 2. + self.chanwidth / 2.
        return chan1 + np.arange(self.nchan) * self.chanwidth


class RRLRun(ContinuumRun):
    """One (epoch, recombination line) run (classes.py:1903-1967)."""

    def __init__(self, dcy, year, line=None, bandwidth=None, chanwidth=None, t_obs=None,
                 t_int=None, tscp=None):
        freq = mrrl.rrl_nu_0(*mrrl.rrl_parser(line))
        super().__init__(dcy, year, freq, bandwidth, chanwidth, t_obs, t_int, tscp)
        self.line = line
        self._obs_type = 'rrl'

    def _tag(self):
        return self.line


_RUN_HDR = ['Year', 'Type', 'Telescope', 't_obs', 't_int', 'Line', 'Frequency', 'Bandwidth',
            'Channel width', 'Radiative Transfer?', 'Synthetic Obs.?', 'Completed?']
_RUN_UNITS = ['yr', '', '', 's', 's', '', 'Hz', 'Hz', 'Hz', '', '', '']
_RUN_FMT = ['.2f', '', '', '.0f', '.0f', '', '.3e', '.3e', '.3e', '', '', '']


def _run_table(rows, tablefmt, **kw):
    import tabulate
    head = [h + ('\n[' + u + ']' if u else '') for h, u in zip(_RUN_HDR, _RUN_UNITS)]
    return tabulate.tabulate(rows, head, tablefmt=tablefmt, floatfmt=_RUN_FMT, **kw)


class Pipeline:
    """Runs the radiative transfer of every (epoch x band/line) of a pipeline-params file
    and writes the reference's products (classes.py:1970-2868, RT section 2386-2479).
    The CASA synthetic-observation section is outside this core."""

    @classmethod
    def load_pipeline(cls, load_file):
        home = os.path.expanduser('~')
        with open(os.path.expanduser(load_file), 'rb') as f:
            loaded = pickle.load(f)
        for run in loaded['runs']:
            run.dcy = run.dcy.replace('~', home)
        loaded['model_file'] = loaded['model_file'].replace('~', home)
        loaded['params']['dcys']['model_dcy'] = \
            loaded['params']['dcys']['model_dcy'].replace('~', home)
        jm = JetModel.load_model(loaded["model_file"])
        new = cls(jm, loaded["params"], log=loaded.get('log'))
        new.runs = loaded["runs"]
        return new

    @staticmethod
    def py_to_dict(py_file):
        return _load_params_file(py_file, miscf.check_pline_params)

    def __init__(self, jetmodel, params, log=None):
        if not isinstance(jetmodel, JetModel):
            raise TypeError("Supplied arg jetmodel must be JetModel instance not {}"
                            "".format(type(jetmodel)))
        self.model = jetmodel
        if isinstance(params, dict):
            err = miscf.check_pline_params(params)
            if err:
                raise err
            self._params = params
        elif isinstance(params, str):
            self._params = Pipeline.py_to_dict(params)
        else:
            raise TypeError("Supplied arg params must be dict or full path (str)")

        self.dcy = self.params['dcys']['model_dcy'].rstrip(os.sep)
        self.model_file = self.dcy + os.sep + "jetmodel.save"
        self.save_file = self.dcy + os.sep + "pipeline.save"
        log_name = "Pipeline_{}.log".format(_time.strftime("%Y%m%d%H-%M-%S",
                                                           _time.localtime()))
        created = not os.path.exists(self.dcy)
        if created:
            os.makedirs(self.dcy, exist_ok=True)      # several ranks may get here together
        self._log = log if log is not None else logger.Log(os.sep.join([self.dcy, log_name]))
        if created:
            self.log.add_entry("INFO", f"Creating pipeline directory, {self.dcy}")
        if self.model.log is None:
            self.model.log = self.log
        elif self.model.log is not self.log:
            merged = logger.Log.combine_logs(self.log, self.model.log, self.log.filename,
                                             delete_old_logs=True)
            self.log = self.model.log = merged

        for band in ('continuum', 'rrls'):
            if self.params[band]['times'] is not None:
                self.params[band]['times'].sort()
            else:
                self.params[band]['times'] = np.array([])

        def pick(v, i):
            return v[i] if miscf.is_iter(v) else v

        runs = []
        c = self.params['continuum']
        self.log.add_entry("INFO", "Reading continuum runs into pipeline")
        for t in c['times']:
            for i, freq in enumerate(c['freqs']):
                runs.append(ContinuumRun(self.dcy, t, freq, pick(c['bws'], i),
                                         pick(c['chanws'], i), pick(c['t_obs'], i),
                                         pick(c['t_ints'], i), pick(c['tscps'], i)))
        if not runs:
            self.log.add_entry("WARNING", "No continuum runs found", timestamp=True)
        r = self.params['rrls']
        self.log.add_entry("INFO", "Reading radio recombination line runs into pipeline")
        n0 = len(runs)
        for t in r['times']:
            for i, line in enumerate(r['lines']):
                runs.append(RRLRun(self.dcy, t, str(line), pick(r['bws'], i),
                                   pick(r['chanws'], i), pick(r['t_obs'], i),
                                   pick(r['t_ints'], i), pick(r['tscps'], i)))
        if len(runs) == n0:
            self.log.add_entry("WARNING", "No RRL runs found", timestamp=True)
        self._runs = runs
        self.log.add_entry("INFO", self.__str__(), timestamp=True)

    def __str__(self):
        return _run_table([run._row() for run in self.runs], "psql", numalign='center',
                          stralign='center')

    params = property(lambda self: self._params)

    @property
    def runs(self):
        return self._runs

    @runs.setter
    def runs(self, new_runs):
        self._runs = new_runs

    @property
    def log(self):
        return self._log

    @log.setter
    def log(self, new_log):
        self._log = new_log

    def save(self, save_file, absolute_directories=False):
        """Pickle the pipeline state (classes.py:2215-2258).  Without `absolute_directories` the
        FILE holds the paths with the home directory as '~'; the runs and parameters of this
        pipeline keep their absolute paths (the products of a run stay where they are)."""
        import copy
        home = os.path.expanduser('~')
        runs, params, mf = self.runs, self._params, self.model_file
        if not absolute_directories:
            runs = [copy.copy(run) for run in self.runs]
            for run in runs:
                run.dcy = run.dcy.replace(home, '~')
            params = dict(self._params, dcys=dict(self._params['dcys']))
            params['dcys']['model_dcy'] = params['dcys']['model_dcy'].replace(home, '~')
            mf = mf.replace(home, '~')
        self.log.add_entry("INFO", "Saving pipeline to " + save_file)
        with open(save_file, 'wb') as f:
            pickle.dump({"runs": runs, "params": params, "model_file": mf,
                         'log': self.log}, f)

    def execute(self, simobserve=True, verbose=True, dryrun=False, resume=True, clobber=False,
                formal=False, formal_rrl=False, antenna_configs=None, sefd_jy=None, seed=0):
        """Radiative transfer for every run; writes EM/Tau/Flux FITS products, records
        `results['flux']`, pickles model and pipeline state (classes.py:2296-2479).
        `formal=True`: the flux cubes of continuum runs (and `results['flux']` from them) by the
        formal solution along the line of sight (`JetModel.flux_ff(formal=True)`).
        `formal_rrl=True`: those of radio-recombination-line runs by
        `JetModel.flux_rrl(formal=True)`; the Tau products are unchanged.  `formal=True` alone
        covers continuum runs only: a run table with an RRL run is then refused before any run
        starts; `formal=True, formal_rrl=True` makes both kinds of run formal.
        `simobserve=True` with `antenna_configs` -- a directory of antenna lists, by default the
        environment variable RAJEPY_ANTENNA_CONFIGS; this package ships none -- observes every run
        that names a telescope on the device (`_synthetic_observation`): `sefd_jy` sets the
        thermal noise (None = noise-free), `seed` its draw (run #i uses seed + i - 1).  Without
        a directory the synthetic observations are skipped with a warning, as before."""
        if formal and not formal_rrl and any(r.obs_type != 'continuum' for r in self.runs):
            raise ValueError("formal=True: the formal solution covers continuum runs only; the "
                             "run table holds radio-recombination-line runs (formal_rrl=True "
                             "makes those formal too)")
        self.log.add_entry("INFO", "Beginning pipeline execution")
        if verbose != self.log.verbose:
            self.log.verbose = verbose
        if antenna_configs is None:
            antenna_configs = os.environ.get("RAJEPY_ANTENNA_CONFIGS") or None
        self._observe = None
        if simobserve and antenna_configs is None:
            self.log.add_entry("WARNING", "CASA synthetic observations are outside the "
                                          "radiative-transfer core and are skipped")
        elif simobserve:
            self._observe = {"dir": os.path.expanduser(str(antenna_configs)), "sefd_jy": sefd_jy,
                             "seed": int(seed)}
        if resume and os.path.exists(self.model_file):
            self.model = JetModel.load_model(self.model_file, engine=self.model._engine)

        # Multi-GPU (one process per GPU inside an initialised torch.distributed group): the
        # EPOCHS of the run table are dealt round-robin to the ranks -- every epoch is a pass
        # over the grid, each rank holds its own copy of the model on its GPU and writes the
        # products of its runs; only the run results are exchanged at the end.
        rank, world, dist = _dist_info()
        years = sorted({float(r.year) for r in self.runs})
        owner = {y: i % world for i, y in enumerate(years)}
        mine = [i for i, r in enumerate(self.runs) if owner[float(r.year)] == rank]
        self._multi_rank = world > 1
        self._formal = bool(formal)
        self._formal_rrl = bool(formal_rrl)

        pending = []
        if not dryrun:
            pending = [self.runs[i].year * con.year for i in mine
                       if self.runs[i].radiative_transfer and
                       not (self.runs[i].completed and resume and not clobber)]
            pending = list(dict.fromkeys(pending))

        # A rank that fails must still reach the gather and the barrier below, or its peers
        # would wait in the collective until the RCCL timeout: per-run failures are recorded
        # and re-raised on EVERY rank after the exchange.
        failure = None
        for idx in mine:
            run = self.runs[idx]
            self.model.time = run.year * con.year
            self.log.add_entry("INFO", "Executing run #{} -> Details:\n{}"
                                       "".format(idx + 1, run.__str__()))
            if run.completed and resume and not clobber:
                self.log.add_entry("INFO", "Run #{} previously completed, skipping"
                                           "".format(idx + 1), timestamp=False)
                continue
            try:
                if not os.path.exists(run.rt_dcy):
                    self.log.add_entry("INFO", "{} doesn't exist, creating"
                                               "".format(run.rt_dcy), timestamp=False)
                    os.makedirs(run.rt_dcy, exist_ok=True)
                if not dryrun and run.radiative_transfer:
                    t_now = float(self.model.time)
                    if t_now in pending:
                        # one pass over HBM serves up to 32 of the epochs still to come; the
                        # whole chunk leaves the list, so the next pass starts where this one
                        # ended (ceil(N / 32) scans for N epochs)
                        k = pending.index(t_now)
                        self.model.prefetch_epochs(pending[k:k + 32])
                        del pending[:k + 32]
                    self._radiative_transfer(idx, run, clobber)
                    if self._observe is not None and run.simobserve:
                        self._synthetic_observation(idx, run)
            except KeyboardInterrupt:
                self.log.add_entry("ERROR", "Pipeline interrupted by user, saving state")
                failure = (idx, "KeyboardInterrupt", "Pipeline interrupted by user")
                break
            except Exception as exc:                      # noqa: BLE001 -- re-raised below
                if world == 1:
                    raise
                self.log.add_entry("ERROR", "Run #{} failed on rank {}: {}: {}".format(
                    idx + 1, rank, type(exc).__name__, exc))
                failure = (idx, type(exc).__name__, str(exc))
                break
            run.completed = True                                   # classes.py:2853

        failures = [failure] if failure else []
        if dist is not None:
            # (inside an initialised group of ANY size, so that a one-rank RCCL group exercises
            # exactly the collectives an eight-rank one does)
            # one small object gather: {run index: (results, completed)} + the failure (if
            # any) of every rank
            local = {"runs": {i: (self.runs[i].results, self.runs[i].completed) for i in mine},
                     "failure": failure, "rank": rank}
            parts = [None] * world
            dist.all_gather_object(parts, local)
            failures = []
            for part in parts:
                for i, (res, done) in part["runs"].items():
                    self.runs[i].results = res
                    self.runs[i].completed = done
                if part["failure"]:
                    failures.append(part["failure"] + (part["rank"],))
        if rank == 0:
            self.save(self.save_file)
            self.model.save(self.model_file)
        if dist is not None:
            dist.barrier()
        if failures:
            f = failures[0]
            if f[1] == "KeyboardInterrupt":
                raise KeyboardInterrupt(f[2])
            where = " on rank %d" % f[3] if len(f) > 3 else ""
            raise RuntimeError("Pipeline run #%d failed%s: %s: %s (state saved; completed "
                               "runs are skipped on resume)" % (f[0] + 1, where, f[1], f[2]))

    def radio_plot(self, run, percentile=5., savefig=False):
        """The reference draws flux / optical depth / emission measure panels with matplotlib
        (`classes.py:3015-3183`); plotting is outside this package: the
        FITS products of `run` hold the same maps."""
        raise NotImplementedError("rajepy_amd produces no plots; read the run's FITS products "
                                  "(run.products) instead")

    def _radiative_transfer(self, idx, run, clobber):
        m = self.model
        self.log.add_entry("INFO", "Conducting radiative transfer at "
                                   f"{run.freq / 1e9:.1f}GHz for a model time of "
                                   f"{run.year:.1f}yr")
        if not os.path.exists(run.fits_em) or clobber:
            self.log.add_entry("INFO", f"Emission measures saved to {run.fits_em}")
            m.emission_measure(savefits=run.fits_em)
        else:
            self.log.add_entry("INFO", f"Emission measures already exist -> {run.fits_em}",
                               timestamp=False)
        rrl = run.obs_type != 'continuum'
        if not os.path.exists(run.fits_tau) or clobber:
            self.log.add_entry("INFO", f"Computing optical depths and saving to {run.fits_tau}")
            if rrl:
                m.optical_depth_rrl(run.line, run.chan_freqs, savefits=run.fits_tau)
            else:
                m.optical_depth_ff(run.chan_freqs, savefits=run.fits_tau)
        else:
            self.log.add_entry("INFO", f"Optical depths already exist -> {run.fits_tau}",
                               timestamp=False)
        if not os.path.exists(run.fits_flux) or clobber:
            self.log.add_entry("INFO", f"Calculating fluxes and saving to {run.fits_flux}")
            if rrl:
                fluxes = m.flux_rrl(run.line, run.chan_freqs, contsub=False,
                                    savefits=run.fits_flux,
                                    formal=getattr(self, "_formal_rrl", False))
            else:
                fluxes = m.flux_ff(run.chan_freqs, savefits=run.fits_flux,
                                   formal=getattr(self, "_formal", False))
        else:
            self.log.add_entry("INFO", f"Fluxes already exist -> {run.fits_flux}",
                               timestamp=False)
            fluxes = _fits.read(run.fits_flux)[0]
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            if not rrl:
                # classes.py:2461-2467: total of the channel-averaged map
                flux = np.nansum(np.nanmean(fluxes, axis=0))
                self.log.add_entry("INFO", f"Total, average, channel flux of {flux:.2e}Jy "
                                           "calculated")
            else:
                flux = np.nansum(np.nansum(fluxes, axis=1), axis=1)     # classes.py:2471
        self.runs[idx].results['flux'] = flux
        if not getattr(self, "_multi_rank", False):
            # single process: checkpoint after every run as the reference does
            # (classes.py:2475-2479); with several ranks rank 0 saves once at the end
            if not os.path.exists(self.model_file):
                m.save(self.model_file)
            self.save(self.save_file, absolute_directories=True)

    # the reference's imaging of a synthetic observation (classes.py:2770-2782)
    OBSERVE_IMAGING = {"weighting": "briggs", "robust": 0.5, "niter": 500, "nsigma": 3.}

    def _observation_setup(self, run, max_baseline_m):
        """(cell [arcsec], side [cells], box) a run is imaged with: `engine.observation_grid` for
        the model's larger angular extent, and the box (i0, i1, j0, j1) of the model's extent
        about the image centre -- the mask the reference hands tclean (classes.py:2688-2759)."""
        from . import engine as E
        m = self.model
        cm_as = np.degrees(np.arctan(m.csize * con.au /
                                     (m.params['target']['dist'] * con.parsec))) * 3600.
        cell_as, side = E.observation_grid(max_baseline_m, run.freq, max(m.nx, m.nz) * cm_as)
        c = (side - 1) / 2.
        hx, hz = 0.5 * m.nx * cm_as / cell_as, 0.5 * m.nz * cm_as / cell_as
        box = (max(0, int(np.floor(c - hx))), min(side - 1, int(np.ceil(c + hx))),
               max(0, int(np.floor(c - hz))), min(side - 1, int(np.ceil(c + hz))))
        return cell_as, side, box

    def _synthetic_observation(self, idx, run):
        """The synthetic observation of one run on the device -- tracks of the run's array,
        model visibilities, thermal noise, Briggs-weighted CLEAN down to 3 sigma inside the
        model's box and, for continuum runs, a Gaussian fit (`JetModel.observe_ff` /
        `observe_rrl`): the reference's simobserve -> tclean -> imfit script
        (classes.py:2490-2850) without CASA.  Continuum runs are imaged as one multi-frequency
        image, line runs as a cube.  Products: `clean_image` (FITS), `ms_clean` and `ms_noisy`
        (.npz of u, v, w [m], vis [F, K], sigma [F], freqs [F], ant1, ant2 [K]; not measurement
        sets); `results['imfit']` for continuum runs.  An antenna list that is missing or cannot
        be read, or a target that never rises, is an ERROR entry and `results['imfit'] = None`,
        as the reference reacts to a failed script."""
        from . import engine as E
        m, so = self.model, self._observe
        tscop, t_cfg = (str(x) for x in run.tscop)
        rrl = run.obs_type != 'continuum'
        path = E.antenna_config_path(so["dir"], tscop, t_cfg)
        try:
            if path is None:
                raise ValueError("no antenna list for (%s, %s) in %s" % (tscop, t_cfg, so["dir"]))
            cfg = E.read_antenna_config(path)
            tracks = m.uv_tracks(cfg, run.t_obs, run.t_int, min_el_deg=self.params['min_el'])
        except (ValueError, OSError) as exc:
            self.log.add_entry("ERROR", "Run #{}'s synthetic observation failed: {}"
                                        "".format(idx + 1, exc))
            run.results['imfit'] = None
            return
        cell_as, side, box = self._observation_setup(run, tracks.max_baseline_m)
        freqs = run.chan_freqs
        self.log.add_entry("INFO", "Synthetic observation with {} ({} antennas, {} integrations): "
                                   "cell size of {:.2e}arcsec on {} x {} cells"
                                   "".format(os.path.basename(path), len(cfg.names),
                                             len(tracks.ha_h), cell_as, side, side),
                           timestamp=False)
        im = self.OBSERVE_IMAGING
        kw = dict(sefd_jy=so["sefd_jy"], chanwidth_hz=run.chanwidth if so["sefd_jy"] is not None
                  else None, seed=(so["seed"] + idx) % 2 ** 64, nsigma=im["nsigma"],
                  shape=(side, side), cell_as=cell_as, niter=im["niter"], mask=box,
                  weighting=im["weighting"], robust=im["robust"])
        if rrl:
            obs = m.observe_rrl(run.line, tracks, freqs, run.t_obs, run.t_int, contsub=False,
                                formal=getattr(self, "_formal_rrl", False), mfs=False, **kw)
        else:
            obs = m.observe_ff(tracks, freqs, run.t_obs, run.t_int, mfs=True, imfit=True,
                               formal=getattr(self, "_formal", False), **kw)
        stem = 'SynObs.' + os.path.basename(path)[:-len('.cfg')]
        dcy = run.rt_dcy + os.sep + 'SynObs'
        os.makedirs(dcy, exist_ok=True)
        ms_clean, ms_noisy = (dcy + os.sep + stem + tail for tail in ('.ms.npz', '.noisy.ms.npz'))
        n_t = len(tracks.ha_h)
        common = dict(u=_to_host(tracks.u_m), v=_to_host(tracks.v_m), w=_to_host(tracks.w_m),
                      sigma=obs.sigma, freqs=np.asarray(freqs, dtype=np.float64),
                      ant1=np.tile(tracks.ant1, n_t), ant2=np.tile(tracks.ant2, n_t))
        _save_npz(ms_clean, vis=obs.vis_clean, **common)
        _save_npz(ms_noisy, vis=obs.vis, **common)
        fitsfile = run.rt_dcy + os.sep + stem + '.noisy.imaging.fits'
        self._save_clean_image(fitsfile, obs, freqs, cell_as, rrl)
        if not rrl:
            run.results['imfit'] = obs.clean.imfit[0]
        run.products['ms_noisy'], run.products['ms_clean'] = ms_noisy, ms_clean
        run.products['clean_image'] = fitsfile
        self.log.add_entry("INFO", "Run #{}'s synthetic observations completed with noisy "
                                   "visibilities saved to {}, clean visibilities saved to {}, and "
                                   "final, clean image saved to {}"
                                   "".format(idx + 1, ms_noisy, ms_clean, fitsfile))

    def _save_clean_image(self, filename, obs, freqs, cell_as, cube):
        """The restored image(s) of an `Observation` as FITS: (F or 1, dec, ra) in Jy / beam on
        the imaging grid of `cell_as`, the first image's clean beam in BMAJ / BMIN / BPA."""
        tg = self.model.params['target']
        _, dec_deg = miscf.sexagesimal_to_deg(tg['ra'], tg['dec'])
        ra_deg = miscf.parse_sexagesimal(tg['ra']) * ((15. * (np.pi / 180.)) / (np.pi / 180.))
        img = obs.clean.image
        n, ni, nj = img.shape
        h = _fits.Header()
        h.set('OBJECT', tg['name'])
        h.set('CTYPE1', 'RA---TAN', 'x-coord type is RA Tan Gnomonic projection')
        h.set('CTYPE2', 'DEC--TAN', 'y-coord type is DEC Tan Gnomonic projection')
        h.set('EQUINOX', 2000., 'Equinox of coordinates')
        h.set('CRPIX1', ni / 2 + 0.5, 'Reference pixel in RA')
        h.set('CRPIX2', nj / 2 + 0.5, 'Reference pixel in DEC')
        h.set('CRVAL1', ra_deg, 'Reference pixel value in RA (deg)')
        h.set('CRVAL2', dec_deg, 'Reference pixel value in DEC (deg)')
        h.set('CDELT1', -cell_as / 3600., 'Pixel increment in RA (deg)')
        h.set('CDELT2', cell_as / 3600., 'Pixel size in DEC (deg)')
        h.set('CTYPE3', 'FREQ', 'Spectral axis (frequency)')
        if cube and n > 1:
            dnu = float(freqs[1] - freqs[0])
            h.set('CRPIX3', 1., 'Reference frequency (channel number)')
            h.set('CRVAL3', float(freqs[0]), 'Reference frequency (Hz)')
            h.set('CDELT3', dnu, 'Frequency increment (Hz)')
        else:
            h.set('CRPIX3', 1., 'Reference frequency (channel number)')
            h.set('CRVAL3', float(np.mean(freqs)), 'Reference frequency (Hz)')
            h.set('CDELT3', float(np.ptp(freqs)) if len(freqs) > 1 else 1.,
                  'Frequency increment (Hz)')
        bmaj, bmin, bpa = obs.clean.beam[0]
        h.set('BMAJ', bmaj / 3600., 'Clean beam major axis FWHM (deg)')
        h.set('BMIN', bmin / 3600., 'Clean beam minor axis FWHM (deg)')
        h.set('BPA', bpa, 'Clean beam position angle (deg)')
        h.set('BUNIT', 'Jy/beam')
        h.set('NOISERMS', float(obs.image_rms[0]), 'Thermal rms of the first image (Jy/beam)')
        lines = self.model.__str__().split('\n')
        h.add_history((' ' * (72 - len(lines[0]))).join(lines))
        _fits.writeto(filename, np.transpose(img, (0, 2, 1)), h)


def _save_npz(filename, **arrays):
    """An uncompressed .npz whose bytes depend on the arrays alone (np.savez stamps every member
    with the time of writing): two runs with the same seed write identical files."""
    import zipfile
    with zipfile.ZipFile(filename, "w", zipfile.ZIP_STORED, allowZip64=True) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[name]), allow_pickle=False)
