"""Antenna-based complex gains -- corrupt, gaincal, applycal and self-calibration (K22: what radio
astronomers get from CASA simobserve's `corrupt`, gaincal and applycal) -- as one unit: the
host-side conventions (solution intervals, seeded gains, the results of a solve) and the
`Calibrator` front, which takes visibilities as device tensors through `RTEngine.gain_apply` /
`RTEngine.gaincal`.  `JetModel` is a front to it.  `engine` re-exports the helpers; this imports
neither `engine` nor `classes`.
"""
import collections

import numpy as np

from .imaging import SIDEREAL_DAY_S, image_scales

GAINCAL_MAX_ANT = 64
CALMODES = ("ap", "p")

# what `JetModel.selfcal_ff` returns: `clean` (the `CleanResult` of the corrected data), `vis`
# (complex128 device tensor [F, K]: the ORIGINAL data corrected by `gains`), `gains` (complex128
# device tensor [F, n_t, n_ant]: the product of every round's gains, per integration -- apply
# with h_sol = arange(n_t)), `history` (one dict per round)
SelfcalResult = collections.namedtuple("SelfcalResult", ["clean", "vis", "gains", "history"])


def solution_intervals(ha_h, day, solint_s):
    """`h_sol` [n_t] int32, the solution interval of every integration of a track (`UVTracks.ha_h`
    [hours, one turn per sidereal day], `UVTracks.day`).  An interval never spans two days.
    `solint_s`: 'int' (one interval per integration), 'inf' (one per day) or seconds: within a day
    integration i falls into bin floor((t_i - t_first) / solint_s + 1e-9), t the hour angle in
    seconds of time, and a new interval starts wherever the bin or the day changes -- so empty bins
    are passed over, and `h_sol` starts at 0 and rises in steps of 0 or 1."""
    ha = np.asarray(ha_h, dtype=np.float64).reshape(-1)
    dy = np.asarray(day).reshape(-1)
    if ha.size < 1 or dy.size != ha.size:
        raise ValueError("solution_intervals: `ha_h` and `day` must have one entry per integration")
    if isinstance(solint_s, str):
        if solint_s not in ("int", "inf"):
            raise ValueError("solution_intervals: `solint_s` must be 'int', 'inf' or seconds")
        bins = np.arange(ha.size) if solint_s == "int" else np.zeros(ha.size, dtype=np.int64)
    else:
        sol = float(solint_s)
        if not (sol > 0. and np.isfinite(sol)):
            raise ValueError("solution_intervals: `solint_s` must be positive")
        t = ha / 24. * SIDEREAL_DAY_S
        first = np.array([t[np.nonzero(dy == d)[0][0]] for d in dy])
        bins = np.floor((t - first) / sol + 1e-9).astype(np.int64)
    new = np.ones(ha.size, dtype=bool)
    new[1:] = (bins[1:] != bins[:-1]) | (dy[1:] != dy[:-1])
    return (np.cumsum(new) - 1).astype(np.int32)


def random_gains(n_sol, n_ant, amp_rms, phase_rms_deg, seed, refant=0):
    """Seeded antenna gains -> complex128 host array (n_sol, n_ant): amplitude 1 + amp_rms N(0, 1),
    phase phase_rms_deg N(0, 1) degrees, independent per antenna and interval, from
    numpy.random.default_rng(seed) -- all amplitudes drawn first, then all phases, each (n_sol,
    n_ant) in C order.  `refant`: that antenna's phase is 0 (its amplitude stays); None = no
    reference.  The sizes are tiny: the host draws them."""
    n_sol, n_ant = int(n_sol), int(n_ant)
    if n_sol < 1 or n_ant < 2:
        raise ValueError("random_gains: n_sol >= 1 and n_ant >= 2")
    rng = np.random.default_rng(seed)
    amp = 1. + float(amp_rms) * rng.standard_normal((n_sol, n_ant))
    ph = np.radians(float(phase_rms_deg)) * rng.standard_normal((n_sol, n_ant))
    if refant is not None:
        ph[:, int(refant)] = 0.
    return amp * np.exp(1j * ph)


def gain_results(gains, chi2, nvis, niter, status, live):
    """Per-solution maps of a solve (`RTEngine.gaincal`'s outputs) -> dict of tensors on the same
    device: 'amp' and 'phase_deg' [M, n_sol, n_ant] (NaN where the antenna is dead or the solution
    has status 3), 'live' [M, n_sol, n_ant] bool, 'status', 'nvis', 'niter' [M, n_sol], 'chi2_start'
    and 'chi2' [M, n_sol] (NaN for status 3)."""
    import torch
    g = gains if gains.is_complex() else torch.view_as_complex(gains)
    return dict(amp=g.abs(), phase_deg=torch.rad2deg(torch.angle(g)), live=live != 0, status=status,
                chi2_start=chi2[..., 0], chi2=chi2[..., 1], nvis=nvis, niter=niter)


class Calibrator:
    """Antenna gains of (F, K) visibility sets on the device of an `RTEngine`; `imager`: the
    `imaging.Imager` that `selfcal` CLEANs with."""

    CLEAN_KEYS = ("weights", "shape", "cell_as", "mfs", "niter", "gain", "threshold_jy", "mask",
                  "beam", "psf_shape", "weighting", "robust")

    def __init__(self, engine, imager=None):
        self.engine = engine
        self.imager = imager

    def _vis(self, who, vis):
        """(F, K) complex, host array or device tensor -> complex128 device tensor [F, K]."""
        import torch
        if not isinstance(vis, torch.Tensor):
            vis = torch.from_numpy(np.ascontiguousarray(vis, dtype=np.complex128))
        if vis.dim() == 1:
            vis = vis.reshape(1, -1)
        if vis.dim() != 2 or not vis.is_complex():
            raise ValueError("%s: visibilities must be complex (F, K)" % who)
        return vis.to(device=self.engine.device, dtype=torch.complex128).contiguous()

    def _gains(self, who, gains):
        """(n_sol, n_ant) or (G, n_sol, n_ant) complex -> complex128 device [G, n_sol, n_ant]."""
        import torch
        if not isinstance(gains, torch.Tensor):
            gains = torch.from_numpy(np.ascontiguousarray(gains, dtype=np.complex128))
        if gains.dim() == 2:
            gains = gains.reshape(1, *gains.shape)
        if gains.dim() != 3 or not gains.is_complex():
            raise ValueError("%s: gains must be complex (n_sol, n_ant) or (F, n_sol, n_ant)" % who)
        return gains.to(device=self.engine.device, dtype=torch.complex128).contiguous()

    @staticmethod
    def n_ant(tracks):
        return int(np.max(tracks.ant2)) + 1

    def corrupt(self, vis, tracks, gains, h_sol):
        return self.engine.gain_apply(self._vis("corrupt_gains", vis),
                                      self._gains("corrupt_gains", gains), h_sol,
                                      self.n_ant(tracks), mode="corrupt")

    def applycal(self, vis, tracks, gains, h_sol):
        return self.engine.gain_apply(self._vis("applycal", vis), self._gains("applycal", gains),
                                      h_sol, self.n_ant(tracks), mode="correct")

    def gaincal(self, vis, model_vis, tracks, solint_s="int", calmode="ap", refant=0, minblperant=4,
                weights=None, tol=1e-10, n_iter=300):
        """-> (gains complex128 device tensor [F, n_sol, n_ant], `gain_results` plus 'h_sol')."""
        if calmode not in CALMODES:
            raise ValueError("gaincal: calmode must be 'ap' or 'p'")
        h_sol = solution_intervals(tracks.ha_h, tracks.day, solint_s)
        out = self.engine.gaincal(self._vis("gaincal", vis), self._vis("gaincal", model_vis), h_sol,
                                  self.n_ant(tracks), weights=weights, mode=calmode, refant=refant,
                                  min_bl=minblperant, tol=tol, n_iter=n_iter)
        res = gain_results(out["gains"], out["chi2"], out["nvis"], out["niter"], out["status"],
                           out["live"])
        res["h_sol"] = h_sol
        return out["gains"], res

    def _component_vis(self, clean, freqs, u_d, v_d, shape, cell_as, mfs):
        """The visibilities [F, K] of a `CleanResult`'s component lists (`RTEngine.vis_components`):
        channel f sees its own list, or with `mfs` the one list, at its own (u, v) / lambda."""
        import torch
        eng = self.engine
        ni, nj, cell = self.imager._image_grid(shape, cell_as)
        F = len(freqs)
        lists = [clean.components[0 if mfs else f] for f in range(F)]
        S = max(1, max(len(c) for c in lists))
        cpix, cflux = np.zeros((F, S), dtype=np.int32), np.zeros((F, S))
        for f, c in enumerate(lists):
            cpix[f, :len(c)] = np.rint(c[:, 0] * nj + c[:, 1]).astype(np.int32)
            cflux[f, :len(c)] = c[:, 2]
        ncomp = np.array([len(c) for c in lists], dtype=np.int32)
        su, sv = image_scales(freqs, cell)
        to = lambda a: torch.from_numpy(a).to(eng.device)
        return eng.vis_components(to(cpix), to(cflux), to(ncomp), ni, nj, su, sv, u_d, v_d)

    def selfcal(self, vis, tracks, freq, rounds, **clean_kwargs):
        """Self-calibration -> `SelfcalResult`.  Per round (a dict of `gaincal`'s keywords:
        solint_s, calmode, refant, minblperant, tol, n_iter): CLEAN the current data, the
        visibilities of its component list, `gaincal` of the current data against them, and the
        ORIGINAL data corrected by the product of all gains so far; after the last round one more
        CLEAN, of the corrected data."""
        import torch
        eng, im = self.engine, self.imager
        bad = set(clean_kwargs) - set(self.CLEAN_KEYS)
        if bad:
            raise ValueError("selfcal: unknown CLEAN arguments %s (taken: %s)"
                             % (sorted(bad), ", ".join(self.CLEAN_KEYS)))
        if not rounds:
            raise ValueError("selfcal: at least one round")
        kw = dict(weights=None, shape=None, cell_as=None, mfs=False, niter=500, gain=0.1,
                  threshold_jy=0.0, mask=None, beam=None, psf_shape=None, weighting=None, robust=0.5)
        kw.update(clean_kwargs)
        freqs = np.atleast_1d(np.asarray(freq, dtype=np.float64))
        V0 = self._vis("selfcal", vis)
        if V0.shape[0] != freqs.size:
            raise ValueError("selfcal: one visibility set per channel (%d)" % freqs.size)
        u_d, v_d = tracks.u_m, tracks.v_m
        n_ant, n_t = self.n_ant(tracks), len(tracks.ha_h)
        h_int = np.arange(n_t, dtype=np.int32)
        clean = lambda V: im._clean_images(
            V, u_d, v_d, freqs, kw["weights"], kw["shape"], kw["cell_as"], kw["mfs"], kw["niter"],
            kw["gain"], kw["threshold_jy"], kw["mask"], kw["beam"], kw["psf_shape"],
            weighting=kw["weighting"], robust=kw["robust"])
        cur, total, history = V0, None, []
        for rnd in rounds:
            res = clean(cur)
            model = self._component_vis(res, freqs, u_d, v_d, kw["shape"], kw["cell_as"], kw["mfs"])
            g, out = self.gaincal(cur, model, tracks, **dict(rnd))
            per_t = g[:, torch.from_numpy(out["h_sol"].astype(np.int64)).to(eng.device), :]
            total = per_t if total is None else total * per_t
            cur = eng.gain_apply(V0, total.contiguous(), h_int, n_ant, mode="correct")
            st = out["status"].reshape(-1)
            solved = st != 3
            history.append(dict(
                peak_residual=float(np.max(np.abs(res.peak_residual))),
                chi2_start=float(out["chi2_start"].reshape(-1)[solved].sum()),
                chi2=float(out["chi2"].reshape(-1)[solved].sum()),
                dynamic_range=float(np.max(np.abs(res.image)) / np.sqrt(np.mean(res.residual ** 2))),
                status={k: int((st == k).sum()) for k in range(4)}, solutions=out))
        return SelfcalResult(clean(cur), cur, total, history)
