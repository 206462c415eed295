"""Fits of the model's own parameters -- the ejection bursts' (t_0, peak_jml, half_life) -- to
light curves and visibilities (K23), as one unit: the Levenberg-Marquardt loop on the host
(`lm_minimise`, the decision rule of csrc/lm_common.h in float64, around a callback), and the
`BurstFit` front, which evaluates the model and its exact derivatives on the device (`ff_grad`,
`ff_formal_grad`, `vis`) and reduces them to normal equations there (`RTEngine.normal_eq`,
rjp_normal_eq): per evaluation 1 + P + P (P + 1) / 2 doubles and a count come back per chunk, no
map, visibility or derivative.  `JetModel.fit_ejections_flux` / `fit_ejections_vis` are fronts to
it.  `engine` re-exports the helpers; this imports neither `engine` nor `classes` at load time.
"""
import collections

import numpy as np

from . import _lib

NORMAL_EQ_MAX_SEL = 48                 # RJP_NORMAL_EQ_MAX_SEL: 3 x (8 + 8) bursts
PARAM_NAMES = ("t_0", "peak_jml", "half_life")
LAM_MIN, LAM_MAX = 1e-12, 1e12

# what `lm_minimise` returns: `theta`, `chi2`, `N`, `g` at the last accepted point (N with the
# identity's rows for fixed parameters), `status`, `niter` (trials evaluated), `lam`, `trace`
LMResult = collections.namedtuple("LMResult", ["theta", "chi2", "N", "g", "status", "niter", "lam",
                                               "trace"])

# what `JetModel.fit_ejections_*` return: `ejections` (shaped like `model.ejections`, plus e_t_0,
# e_peak_jml, e_half_life), `theta` [n_ej, 3], `cov` (N^-1 over the free fit parameters, in their
# order), `chi2`, `reduced_chi2`, `ndata` (real numbers that count), `status`, `niter`, `trace`
EjectionFit = collections.namedtuple("EjectionFit", ["ejections", "theta", "cov", "chi2",
                                                     "reduced_chi2", "ndata", "status", "niter",
                                                     "trace"])


def unpack_triangle(packed, P):
    """The symmetric P x P matrix of a packed upper triangle (row by row: rjp_normal_eq's N)."""
    M = np.zeros((P, P), dtype=np.float64)
    iu = np.triu_indices(P)
    M[iu] = np.asarray(packed, dtype=np.float64)
    M.T[iu] = M[iu]
    return M


def cholesky_solve(M, g):
    """(delta, ok) of M delta = g by an unblocked Cholesky in float64, as lm_solve makes it; ok
    False: a pivot is not > 0."""
    M, g = np.asarray(M, dtype=np.float64), np.asarray(g, dtype=np.float64)
    P = M.shape[0]
    L = np.zeros((P, P))
    ok = True
    with np.errstate(all="ignore"):
        for j in range(P):
            d = M[j, j] - np.dot(L[j, :j], L[j, :j])
            ok = ok and bool(d > 0.)
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, P):
                L[i, j] = (M[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
        y = np.zeros(P)
        for i in range(P):
            y[i] = (g[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
        x = np.zeros(P)
        for i in range(P - 1, -1, -1):
            x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x, ok


def take_sums(free, N, g):
    """(N, g) of an accepted trial with the identity's rows and g_i = 0 for a fixed parameter."""
    free = np.asarray(free, dtype=bool)
    N = np.where(np.outer(free, free), np.asarray(N, dtype=np.float64), np.eye(free.size))
    return N, np.where(free, np.asarray(g, dtype=np.float64), 0.)


def lm_minimise(evaluate, theta0, free=None, feasible=None, scales=None, n_iter=30, lambda0=1e-3,
                xtol=1e-8, trace=False):
    """Levenberg-Marquardt on the host, the decision rule of csrc/lm_common.h in float64 ->
    `LMResult`.  `evaluate(theta, want_jac)` -> (chi2, g, N): chi^2 = sum w |r|^2, g = Re(J^H W r),
    N = Re(J^H W J) (full P x P) at `theta`; with `want_jac` False only chi2 is read (g, N may be
    None).  Trial t = 1 .. n_iter (the first: the start, with chi2_cur = +inf), in this order:
      1. accept iff the trial is feasible, its chi2 finite and < chi2_cur: theta, chi2, N, g become
         the trial's and lambda <- max(lambda / 10, 1e-12) (accepting the start leaves lambda0);
         else lambda <- 10 lambda.  A fixed parameter (`free` False) has the identity's row and
         column in N and g = 0: its step is exactly 0;
      2. chi2_cur = 0 -> status 1.  Else (N + lambda diag N) delta = g by Cholesky; a pivot that
         is not > 0 counts as a reject (lambda <- 10 lambda, again); lambda > 1e12 -> status 2;
      3. max_i |delta_i| / s_i <= xtol, s = `scales(theta_cur)` -> status 1 (tested on every
         proposed step); n_iter trials done -> status 0; else the next trial is theta_cur + delta.
    status 3: a start that is not finite or not feasible, or whose chi2 is not finite; nothing was
    fitted.  Only a trial that would be accepted is evaluated with `want_jac` (the start at once):
    a rejected trial costs no derivatives, and an infeasible one no evaluation at all.
    `feasible(theta)` -> bool (None: always), `scales(theta)` -> [P] (None: ones); `trace`: a list
    of one dict per trial (chi2, lam -- the lambda that proposed it --, accepted, theta, and for an
    accepted trial N and g as taken over)."""
    theta0 = np.array(theta0, dtype=np.float64).reshape(-1)
    P = theta0.size
    free = np.ones(P, dtype=bool) if free is None else np.asarray(free, dtype=bool).reshape(-1)
    if free.size != P:
        raise ValueError("lm_minimise: `free` must have one entry per parameter")
    n_iter = int(n_iter)
    if n_iter < 1 or not (lambda0 > 0. and np.isfinite(lambda0) and xtol > 0. and np.isfinite(xtol)):
        raise ValueError("lm_minimise: n_iter >= 1, lambda0 and xtol finite and positive")
    feasible = feasible or (lambda th: True)
    scales = scales or (lambda th: np.ones(P))
    rows = [] if trace else None
    nan = float("nan")
    if not (np.all(np.isfinite(theta0)) and feasible(theta0)):
        return LMResult(theta0, nan, None, None, 3, 0, float(lambda0), rows)
    cur, chi_cur, N, g = None, float("inf"), None, None
    lam = lam_used = float(lambda0)
    trial, status, it = theta0, 0, 0
    for it in range(1, n_iter + 1):
        first = it == 1
        ok_t = feasible(trial)
        g_t = N_t = None
        if first:
            chi_t, g_t, N_t = evaluate(trial, True)
        else:
            chi_t = evaluate(trial, False)[0] if ok_t else nan
        chi_t = float(chi_t)
        if first and not np.isfinite(chi_t):
            return LMResult(theta0, nan, None, None, 3, 1, lam, rows)
        acc = bool(ok_t and np.isfinite(chi_t) and chi_t < chi_cur)
        if acc:
            if not first:
                _, g_t, N_t = evaluate(trial, True)
                lam = max(lam / 10., LAM_MIN)
            cur, chi_cur = trial, chi_t
            N, g = take_sums(free, N_t, g_t)
        else:
            lam *= 10.
        if trace:
            rows.append(dict(chi2=chi_t, lam=lam_used, accepted=acc, theta=trial.copy(),
                             N=N.copy() if acc else None, g=g.copy() if acc else None))
        if chi_cur == 0.:
            status = 1
            break
        while True:
            if lam > LAM_MAX:
                status = 2
                break
            diag = np.diag(N)
            delta, ok = cholesky_solve(N + np.diag(lam * diag), g)
            if ok:
                break
            lam *= 10.
        if status == 2:
            break
        with np.errstate(all="ignore"):
            worst = np.max(np.abs(delta) / np.asarray(scales(cur), dtype=np.float64))
        if not np.any(np.isnan(delta)) and worst <= xtol:
            status = 1
            break
        if it == n_iter:
            status = 0
            break
        trial, lam_used = cur + delta, lam
    return LMResult(cur, chi_cur, N, g, status, it, lam, rows)


class _Trial:
    """What `JetModel._ejection_slots` reads, at a trial's values: the model is not touched."""

    def __init__(self, model, ejections):
        self._ss_jml_rj, self._ss_jml_bj = model._ss_jml_rj, model._ss_jml_bj
        self._ejections = ejections
        from .classes import ejection_burst
        self._bursts = {'R': [], 'B': []}
        for ej in ejections.values():
            ss = self._ss_jml_bj if ej['which'] == 'B' else self._ss_jml_rj
            self._bursts[ej['which']].append(ejection_burst(ej['t_0'], ej['peak_jml'], ej['half_life'], ss))


class BurstFit:
    """The front behind `JetModel.fit_ejections_flux` / `fit_ejections_vis`: the parameters are
    the physical (t_0 [s], peak_jml [kg/s], half_life [s]) of every entry of `model.ejections`, in
    that order; their conversion to kernel parameters and its diagonal chain rule are
    `JetModel._ejection_slots` / `ejection_chain_rule`, evaluated at each trial; trial bursts go to
    the engine explicitly (`make_bursts`): the model is not mutated during a fit."""

    def __init__(self, model):
        self.model = model
        self.last_count = 0

    engine = property(lambda self: self.model.engine)      # (made on first use: the layout needs none)

    # ---- the parameter layout ---------------------------------------------------------------
    def layout(self, free=None, tie=None, theta0=None):
        """-> dict: `keys` (ejection keys in order), `phys0` [n_ej, 3] (the start), `group` [3 n_ej]
        (the fit parameter of every physical one), `ratio` [3 n_ej] (physical = ratio x fit value),
        `T` [3 n_ej, n_fit] (the same as a matrix: N_fit = T^T N T, g_fit = T^T g), `theta0`
        [n_fit], `free_fit` [n_fit] and `free_phys` [3 n_ej] (a group is free iff all its members
        are).  `free`: None (all), a boolean [n_ej, 3] (True: fitted) or a dict {ejection key:
        names}: of an ejection the dict names, ONLY the named parameters are fitted and the others
        held ([] holds all three); an ejection it does not name stays free; `tie`: a list
        of groups of (key, name) that share one fit value -- members that start at the same value
        stay bit-equal, members that start at different values keep their ratio to the group's
        first member (the peaks of the two halves of an 'RB' event differ by the jets' steady
        mass-loss rates); `theta0`: None (the model's ejections), [n_ej, 3] or a dict {key: {name:
        value}} of the values that differ from the model's."""
        ej = self.model.ejections
        keys = list(ej)
        n_ej = len(keys)
        if n_ej == 0:
            raise ValueError("fit_ejections: the model has no ejections to fit")
        if 3 * n_ej > NORMAL_EQ_MAX_SEL:
            raise ValueError("fit_ejections: at most %d ejections" % (NORMAL_EQ_MAX_SEL // 3))
        phys0 = np.array([[ej[k][n] for n in PARAM_NAMES] for k in keys], dtype=np.float64)
        if isinstance(theta0, dict):
            for k, vals in theta0.items():
                for n, v in vals.items():
                    phys0[keys.index(str(k)), PARAM_NAMES.index(n)] = float(v)
        elif theta0 is not None:
            phys0 = np.array(theta0, dtype=np.float64).reshape(n_ej, 3)
        if free is None:
            fp = np.ones((n_ej, 3), dtype=bool)
        elif isinstance(free, dict):
            fp = np.ones((n_ej, 3), dtype=bool)
            for k, names in free.items():
                fp[keys.index(str(k))] = False
                for n in ([names] if isinstance(names, str) else names):
                    fp[keys.index(str(k)), PARAM_NAMES.index(n)] = True
        else:
            fp = np.array(free, dtype=bool).reshape(n_ej, 3)
        head = np.arange(3 * n_ej)                     # the first member of every parameter's group
        tied = set()
        for grp in (tie or []):
            idx = sorted(3 * keys.index(str(k)) + PARAM_NAMES.index(n) for k, n in grp)
            if len(set(idx)) != len(idx) or len(idx) < 2:
                raise ValueError("fit_ejections: a tie needs two or more different parameters")
            if tied & set(idx):
                raise ValueError("fit_ejections: a parameter may be tied once")
            tied |= set(idx)
            head[idx] = idx[0]
        heads = sorted(set(head.tolist()))
        group = np.array([heads.index(h) for h in head])
        p0 = phys0.reshape(-1)
        ratio = np.ones(3 * n_ej)
        for i in range(3 * n_ej):
            if p0[i] != p0[head[i]]:
                if p0[head[i]] == 0. or not np.isfinite(p0[i] / p0[head[i]]):
                    raise ValueError("fit_ejections: tied parameters that start at different "
                                     "values keep their ratio, which needs a non-zero first member")
                ratio[i] = p0[i] / p0[head[i]]
        T = np.zeros((3 * n_ej, len(heads)))
        T[np.arange(3 * n_ej), group] = ratio
        free_fit = np.array([bool(np.all(fp.reshape(-1)[group == gidx])) for gidx in range(len(heads))])
        return dict(keys=keys, phys0=phys0, group=group, ratio=ratio, T=T, theta0=p0[heads].copy(),
                    free_fit=free_fit, free_phys=free_fit[group], heads=np.array(heads))

    @staticmethod
    def physical(lay, theta):
        """Fit values -> the physical parameters [n_ej, 3] (ratio 1: the same bits)."""
        theta = np.asarray(theta, dtype=np.float64)
        return (lay["ratio"] * theta[lay["group"]]).reshape(-1, 3)

    def trial_ejections(self, lay, phys):
        ej = self.model.ejections
        return {k: dict(t_0=float(phys[i, 0]), peak_jml=float(phys[i, 1]),
                        half_life=float(phys[i, 2]), which=ej[k]['which'])
                for i, k in enumerate(lay["keys"])}

    @staticmethod
    def feasible(phys):
        phys = np.asarray(phys)
        return bool(np.all(np.isfinite(phys)) and np.all(phys[:, 1] > 0.) and np.all(phys[:, 2] > 0.))

    @staticmethod
    def step_scales(lay, phys):
        """Per fit parameter, from its group's first member: half_life for t_0 and half_life,
        |peak_jml| for peak_jml."""
        s = np.stack([phys[:, 2], np.abs(phys[:, 1]), phys[:, 2]], axis=1).reshape(-1)
        return s[lay["heads"]]

    def _kernel_side(self, lay, phys):
        """A trial -> (rjp_bursts, n_par, sel [P_sel] kernel planes, chain [P_sel], where [P_sel]
        physical parameter of every plane): the free physical parameters only."""
        from .engine import make_bursts
        trial = _Trial(self.model, self.trial_ejections(lay, phys))
        slots = type(self.model)._ejection_slots(trial)
        bursts = make_bursts(trial._bursts['R'], trial._bursts['B'])
        sel, chain, where = [], [], []
        for i, (k, ch) in enumerate(slots):
            for c in range(3):
                if lay["free_phys"][3 * i + c]:
                    sel.append(k + c)
                    chain.append(ch[c])
                    where.append(3 * i + c)
        return bursts, 3 * len(slots), np.array(sel, dtype=np.int32), np.array(chain), np.array(where, dtype=np.int64)

    @staticmethod
    def to_fit_space(lay, chain, where, chi2, g_raw, N_packed):
        """Kernel-plane sums -> (chi2, g_fit, N_fit): the diagonal chain rule, then the ties,
        N_fit = T^T N T and g_fit = T^T g."""
        n_phys = lay["T"].shape[0]
        P = len(where)
        g = np.zeros(n_phys)
        N = np.zeros((n_phys, n_phys))
        if P:
            g[where] = chain * np.asarray(g_raw, dtype=np.float64)
            N[np.ix_(where, where)] = unpack_triangle(N_packed, P) * np.outer(chain, chain)
        T = lay["T"]
        return float(chi2), T.T @ g, T.T @ N @ T

    # ---- the loop -----------------------------------------------------------------------------
    def _run(self, lay, sums, n_part, n_iter, lambda0, xtol, update, trace):
        """`sums(bursts, n_par, sel, want_jac)` -> (chi2, g_raw, N_packed, count) on the host."""
        def evaluate(theta, want_jac):
            phys = self.physical(lay, theta)
            bursts, n_par, sel, chain, where = self._kernel_side(lay, phys)
            if not want_jac:
                sel, chain, where = sel[:0], chain[:0], where[:0]
            chi2, g_raw, N_packed, count = sums(bursts, n_par, sel, want_jac)
            self.last_count = int(count)
            return self.to_fit_space(lay, chain, where, chi2, g_raw, N_packed)

        res = lm_minimise(evaluate, lay["theta0"], lay["free_fit"],
                          lambda th: self.feasible(self.physical(lay, th)),
                          lambda th: self.step_scales(lay, self.physical(lay, th)),
                          n_iter, lambda0, xtol, trace)
        n_free = int(lay["free_fit"].sum())
        ndata = n_part * self.last_count
        if res.status != 3 and ndata < n_free:
            res = res._replace(status=3)
        if res.status == 3:
            return EjectionFit(None, lay["phys0"], None, float("nan"), float("nan"), ndata, 3,
                               res.niter, res.trace)
        phys = self.physical(lay, res.theta)
        fr = np.nonzero(lay["free_fit"])[0]
        with np.errstate(all="ignore"):
            # (inverted on a unit diagonal: the parameters span 20 orders of magnitude)
            d = 1. / np.sqrt(np.diag(res.N)[fr])
            cov = np.linalg.inv(res.N[np.ix_(fr, fr)] * np.outer(d, d)) * np.outer(d, d) if n_free \
                else np.zeros((0, 0))
            red = res.chi2 / (ndata - n_free) if ndata > n_free else float("nan")
            err_fit = np.zeros(lay["free_fit"].size)
            err_fit[fr] = np.sqrt(np.diag(cov) * (red if np.isfinite(red) else 1.))
        err = (np.abs(lay["ratio"]) * err_fit[lay["group"]]).reshape(-1, 3)
        ej = self.trial_ejections(lay, phys)
        for i, k in enumerate(lay["keys"]):
            ej[k].update(e_t_0=float(err[i, 0]), e_peak_jml=float(err[i, 1]),
                         e_half_life=float(err[i, 2]))
        if update:
            for i, k in enumerate(lay["keys"]):
                self.model.set_ejection_event(k, t_0=phys[i, 0], peak_jml=phys[i, 1],
                                              half_life=phys[i, 2])
        return EjectionFit(ej, phys, cov, res.chi2, red, ndata, res.status, res.niter, res.trace)

    @staticmethod
    def _host_sums(parts):
        """Per-chunk device results added on the host in chunk order."""
        chi2, g, N, count = 0., 0., 0., 0
        for c2, gg, NN, cnt in parts:
            chi2 = chi2 + float(c2.cpu())
            g = g + gg.cpu().numpy()
            N = N + NN.cpu().numpy()
            count += int(cnt.cpu())
        return chi2, g, N, count

    def _stack(self, who, values, shape, complex_=False):
        """Host array or device tensor -> contiguous device tensor of `shape`."""
        import torch
        dt = torch.complex128 if complex_ else torch.float64
        if not isinstance(values, torch.Tensor):
            values = torch.from_numpy(np.ascontiguousarray(
                values, dtype=np.complex128 if complex_ else np.float64))
        if values.numel() != int(np.prod(shape)):
            raise ValueError("%s: expected %s values" % (who, " x ".join(str(s) for s in shape)))
        return values.to(device=self.engine.device, dtype=dt).reshape(*shape).contiguous()

    def fit_flux(self, times_s, freq, flux, sigma=None, formal=False, free=None, tie=None,
                 theta0=None, n_iter=30, lambda0=1e-3, xtol=1e-8, update=False, trace=False):
        model, eng = self.model, self.engine
        lay = self.layout(free, tie, theta0)
        times = [float(t) for t in np.atleast_1d(np.asarray(times_s, float))]
        freqs, (ctau, cflux) = model._channel_coeffs(freq)
        E, F = len(times), len(freqs)
        if formal:
            if model._dtype != _lib.RJP_F64:
                raise ValueError("burst-parameter sensitivities need f64 storage")
            dev = model.device_fields
        else:
            dev = model._grad_fields()
        data = self._stack("fit_ejections_flux: `flux`", flux, (E * F, 1))
        w = None
        if sigma is not None:
            if not hasattr(sigma, "dim"):
                sigma = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (E, F))
            sg = self._stack("fit_ejections_flux: `sigma`", sigma, (E * F, 1))
            w = 1. / (sg * sg)
        gff = model.gff_mode

        def sums(bursts, n_par, sel, want_jac):
            if want_jac:
                if formal:
                    ftot, dftot, _ = eng.ff_formal_grad(dev, bursts, times, gff, ctau, cflux)
                else:
                    _, _, ftot, dftot = eng.ff_grad(dev, bursts, times, gff, model._model_tavg(),
                                                    ctau, cflux)
                dftot = dftot.reshape(E * F, n_par, 1)
            else:
                if formal:
                    ftot = eng.ff_formal_sweep(dev, bursts, times, gff, ctau, cflux)[1]
                else:
                    sumA = eng.ff_scan(dev, bursts, times, gff, want_em=False, want_tavg=False)[0]
                    ftot = eng.ff_maps(sumA, model._model_tavg(), ctau, cflux, want_tau=False,
                                       want_flux=False)[2]
                dftot = None
            return self._host_sums([eng.normal_eq(data, ftot.reshape(E * F, 1), dftot, sel, w)])

        return self._run(lay, sums, 1, n_iter, lambda0, xtol, update, trace)

    def fit_vis(self, times_s, u_m, v_m, freq, vis, weights=None, free=None, tie=None,
                theta0=None, n_iter=30, lambda0=1e-3, xtol=1e-8, update=False, trace=False):
        model, eng = self.model, self.engine
        if model._dtype != _lib.RJP_F64:
            raise ValueError("burst-parameter sensitivities need f64 storage")
        lay = self.layout(free, tie, theta0)
        times = [float(t) for t in np.atleast_1d(np.asarray(times_s, float))]
        freqs, (ctau, cflux) = model._channel_coeffs(freq)
        E, F = len(times), len(freqs)
        u_d, v_d = eng._device_f64(u_m), eng._device_f64(v_m)
        per_epoch = (u_m.dim() if hasattr(u_m, "dim") else np.ndim(u_m)) == 2
        K = int(u_d.numel()) // (E if per_epoch else 1)
        if K < 1 or u_d.numel() != v_d.numel() or u_d.numel() != K * (E if per_epoch else 1):
            raise ValueError("fit_ejections_vis: `u_m`, `v_m` must be [K] or [E, K]")
        data = self._stack("fit_ejections_vis: `vis`", vis, (E * F, K), complex_=True)
        w = None
        if weights is not None:
            w = eng._device_f64(weights)
            if w.numel() == E * K and E * K != K:
                w = w.reshape(E, 1, K).expand(E, F, K).reshape(E * F, K).contiguous()
            elif w.numel() == E * F * K:
                w = w.reshape(E * F, K)
            elif w.numel() != K:
                raise ValueError("fit_ejections_vis: `weights` must be [K], [E, K] or [E, F, K]")
        su, sv = model._vis_scales(freqs)
        dev, gff, nx, nz = model.device_fields, model.gff_mode, model.nx, model.nz

        def to_vis(maps, e0, n, per_map):
            """The visibilities [n F per_map, K] of the chunk's maps [n, F, per_map, npix]."""
            s_u, s_v = np.repeat(su, per_map), np.repeat(sv, per_map)
            if not per_epoch:
                return eng.vis(maps.reshape(n * F * per_map, -1), nx, nz, np.tile(s_u, n),
                               np.tile(s_v, n), u_d, v_d)
            import torch
            return torch.cat([eng.vis(maps[i].reshape(F * per_map, -1), nx, nz, s_u, s_v,
                                      u_d.reshape(E, K)[e0 + i], v_d.reshape(E, K)[e0 + i])
                              for i in range(n)], dim=0)

        kept = dict(key=None, V={})       # the model visibilities of the last trial, per chunk

        def sums(bursts, n_par, sel, want_jac):
            # chunks of epochs whose derivative maps stay under the model's limit (1 GiB)
            step = model._vis_chunk(F * max(1, n_par))
            key = tuple(float(col[j][i]) for j in range(2) for i in range(bursts.n[j])
                        for col in (bursts.t0, bursts.amp_rel, bursts.inv2s2))
            if kept["key"] != key:
                kept.update(key=key, V={})
            parts = []
            for e0 in range(0, E, step):
                chunk = times[e0:e0 + step]
                n = len(chunk)
                V = kept["V"].get(e0)      # an accepted trial's derivatives reuse the trial's own V
                if V is None:
                    maps, _ = eng.ff_formal_sweep(dev, bursts, chunk, gff, ctau, cflux,
                                                  want_maps=True, want_totals=False)
                    V = kept["V"][e0] = to_vis(maps.reshape(n, F, 1, -1), e0, n, 1)
                    del maps
                dV = None
                if want_jac:
                    dmaps = eng.ff_formal_grad(dev, bursts, chunk, gff, ctau, cflux,
                                               want_maps=True)[2]
                    dV = to_vis(dmaps.reshape(n, F, n_par, -1), e0, n, n_par).reshape(n * F, n_par, K)
                    del dmaps
                wc = w if w is None or w.numel() == K else w[e0 * F:(e0 + n) * F]
                parts.append(eng.normal_eq(data[e0 * F:(e0 + n) * F], V, dV, sel, wc))
            return self._host_sums(parts)

        return self._run(lay, sums, 2, n_iter, lambda0, xtol, update, trace)
