"""The spectral axis of a line cube -- moment maps and per-sightline Gaussian fits (K21: what radio
astronomers get from CASA immoments and specfit) and per-sightline Voigt fits (K24) -- as one unit: the host-side conventions (the
velocity axis, the start of a fit, its results with errors) and the `Spectra` front, which takes
cubes as device tensors through `RTEngine.cube_moments` / `RTEngine.specfit` / `RTEngine.voigtfit`.  `JetModel` is a
front to it.  `engine` re-exports the helpers; this imports neither `engine` nor `classes`.
"""
import numpy as np

from . import _constants as con

SPECFIT_MAX_COMP = 2
SPECFIT_MAX_CHAN = 4096
VOIGTFIT_MAX_COMP = 2
FWHM_PER_SIGMA = float(np.sqrt(8. * np.log(2.)))
SQRT_2PI = float(np.sqrt(2. * np.pi))


def velocity_axis(freqs, nu0):
    """(v [F], dv [F]) in km/s of the channels `freqs` [Hz] about the rest frequency `nu0` [Hz]
    (`maths.rrls.rrl_nu_0`) in the radio convention v = c (nu0 - nu) / nu0, and the channel widths:
    half the distance between the neighbours on either side, one-sided at the ends (the distance
    to the one neighbour); a single channel has width 0.  Ascending frequencies give a descending
    axis, which the K21 entry points take as it is."""
    nu = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    v = con.c * (float(nu0) - nu) / float(nu0) / 1e3
    return v, channel_widths(v)


def channel_widths(x):
    """dx [F] of an axis `x`: half the distance between the neighbours on either side, the
    distance to the one neighbour at the ends, 0 for a single channel."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    dx = np.zeros_like(x)
    if x.size > 1:
        dx[1:-1] = 0.5 * np.abs(x[2:] - x[:-2])
        dx[0], dx[-1] = abs(x[1] - x[0]), abs(x[-1] - x[-2])
    return dx


def n_params(n_comp):
    return 3 * int(n_comp) + 2


def specfit_start(mom, ipeak, x, n_comp=1):
    """The start of a one-component fit from the moment maps, in plain torch on the device of
    `mom` -> theta [5, n_pix]: A = the peak, x0 = x[ipeak], s = m2 -- twice the local channel
    spacing where m2 is NaN or 0 --, b0 = b1 = 0.  `mom` [4, n_pix] and `ipeak` [n_pix] as
    `RTEngine.cube_moments` returns them, `x` [F] the axis.  A pixel without a peak (ipeak -1)
    starts from NaN and ends degenerate (status 3).  Two components need a caller's start."""
    import torch
    if int(n_comp) != 1:
        raise ValueError("specfit_start: only one component can be started from the moments; "
                         "pass `theta0` for two")
    xd = torch.as_tensor(np.asarray(x, dtype=np.float64) if not isinstance(x, torch.Tensor) else x,
                         dtype=torch.float64, device=mom.device).reshape(-1)
    F = xd.numel()
    ip = ipeak.to(torch.int64).reshape(-1)
    ic = ip.clamp(0, F - 1)
    if F > 1:
        lo, hi = (ic - 1).clamp(0, F - 1), (ic + 1).clamp(0, F - 1)
        spacing = (xd[hi] - xd[lo]).abs() / (hi - lo).to(torch.float64)
    else:
        spacing = torch.ones_like(xd[ic])
    m2 = mom[2].reshape(-1)
    s = torch.where(torch.isfinite(m2) & (m2 > 0), m2, 2. * spacing)
    nan = torch.full_like(s, float("nan"))
    live = ip >= 0
    zero = torch.zeros_like(s)
    return torch.stack([torch.where(live, mom[3].reshape(-1), nan), torch.where(live, xd[ic], nan),
                        torch.where(live, s, nan), zero, zero.clone()])


def _tri(P):
    return [(i, j) for i in range(P) for j in range(i, P)]


def specfit_results(theta, cov, chi2, nchan, status, free=None, scale_errors=True):
    """Per-pixel maps of a fit (`RTEngine.specfit`'s `theta` [P, n], `cov` [P (P + 1) / 2, n],
    `chi2`, `nchan`, `status` [n]) -> dict of tensors on the same device.  Per component c (a list
    of n_comp tensors under each key): 'peak' (A), 'centre' (x0), 'sigma' (s), 'fwhm' = s sqrt(8 ln
    2), 'integral' = A s sqrt(2 pi), and 'e_peak', 'e_centre', 'e_sigma', 'e_fwhm', 'e_integral';
    'b0', 'b1', 'e_b0', 'e_b1'; 'chi2', 'reduced_chi2' = chi2 / (nchan - n_free), 'nchan', 'status'.
    Errors: the square roots of the diagonal of (N_ff)^-1, N_ff the rows and columns of the free
    parameters of `cov` (a batched `torch.linalg.inv` on the device), times sqrt(reduced chi^2)
    with `scale_errors` (unit weights: the scatter sets the scale; weights 1 / sigma^2: pass
    False for the formal errors); a fixed parameter's error is 0; by first-order propagation
    var(fwhm) = 8 ln 2 var(s) and var(integral) = 2 pi (s^2 var(A) + A^2 var(s) + 2 A s cov(A, s)).
    NaN wherever status == 3, a singular N_ff, or (for the scaled errors) nchan == n_free."""
    import torch
    P, n = int(theta.shape[0]), int(theta.shape[1])
    nc = (P - 2) // 3
    fr = np.ones(P, dtype=bool) if free is None else np.asarray(free).reshape(-1) != 0
    if fr.size != P or not fr.any():
        raise ValueError("specfit_results: `free` must hold %d flags, at least one of them set" % P)
    idx = [int(i) for i in np.nonzero(fr)[0]]
    bad = status.reshape(-1) == 3
    nan = float("nan")
    N = torch.zeros((n, P, P), dtype=torch.float64, device=theta.device)
    for k, (i, j) in enumerate(_tri(P)):
        N[:, i, j] = cov[k]
        N[:, j, i] = cov[k]
    Nff = N[:, idx][:, :, idx]
    eye = torch.eye(len(idx), dtype=torch.float64, device=theta.device)
    Nff = torch.where(bad[:, None, None] | ~torch.isfinite(Nff).all(dim=(1, 2), keepdim=True), eye, Nff)
    inv, info = torch.linalg.inv_ex(Nff)
    C = torch.zeros((n, P, P), dtype=torch.float64, device=theta.device)
    sub = torch.where((info != 0)[:, None, None], torch.full_like(inv, nan), inv)
    for a, i in enumerate(idx):
        for b, j in enumerate(idx):
            C[:, i, j] = sub[:, a, b]
    dof = (nchan.reshape(-1) - len(idx)).to(torch.float64)
    red = torch.where(dof > 0, chi2.reshape(-1) / dof, torch.full_like(dof, nan))
    if scale_errors:
        C = C * red[:, None, None]
    blank = lambda t: torch.where(bad, torch.full_like(t, nan), t)
    sd = lambda v: blank(torch.sqrt(v))
    out = {k: [] for k in ("peak", "centre", "sigma", "fwhm", "integral", "e_peak", "e_centre",
                           "e_sigma", "e_fwhm", "e_integral")}
    for c in range(nc):
        A, x0, s = theta[3 * c], theta[3 * c + 1], theta[3 * c + 2]
        vA, vs, cAs = C[:, 3 * c, 3 * c], C[:, 3 * c + 2, 3 * c + 2], C[:, 3 * c, 3 * c + 2]
        out["peak"].append(blank(A))
        out["centre"].append(blank(x0))
        out["sigma"].append(blank(s))
        out["fwhm"].append(blank(s * FWHM_PER_SIGMA))
        out["integral"].append(blank(A * s * SQRT_2PI))
        out["e_peak"].append(sd(vA))
        out["e_centre"].append(sd(C[:, 3 * c + 1, 3 * c + 1]))
        out["e_sigma"].append(sd(vs))
        out["e_fwhm"].append(sd(vs) * FWHM_PER_SIGMA)
        out["e_integral"].append(sd(2. * np.pi * (s * s * vA + A * A * vs + 2. * A * s * cAs)))
    out.update(b0=blank(theta[P - 2]), b1=blank(theta[P - 1]), e_b0=sd(C[:, P - 2, P - 2]),
               e_b1=sd(C[:, P - 1, P - 1]), chi2=blank(chi2.reshape(-1)), reduced_chi2=blank(red),
               nchan=nchan.reshape(-1), status=status.reshape(-1))
    return out


def voigt_n_params(n_comp):
    return 4 * int(n_comp) + 2


def voigt_start(cube, mom, ipeak, x):
    """The start of a one-component Voigt fit (`RTEngine.voigtfit`) from the cube and its moment
    maps, in plain torch on the device of `mom` -> theta [6, n_pix] = (F, x0, s, g, b0, b1): F = m0,
    x0 = x[ipeak]; with hw = half the extent |x_hi - x_lo| of the channels at or above half the peak
    (finite ones), at least one local channel spacing, s = hw / 1.1774 / 1.5 and g = hw / 2 -- a
    start between the two limits, from which the area form converges for g / s from 0 to 20;
    b0 = b1 = 0.  `cube` [F, n_pix], `mom` [4, n_pix] and `ipeak` [n_pix] as `RTEngine.cube_moments`
    returns them, `x` [F] the axis.  A pixel without a peak (ipeak -1) starts from NaN and ends
    degenerate (status 3).  Two components need a caller's start."""
    import torch
    xd = torch.as_tensor(np.asarray(x, dtype=np.float64) if not isinstance(x, torch.Tensor) else x,
                         dtype=torch.float64, device=mom.device).reshape(-1)
    F = xd.numel()
    y = cube.reshape(F, -1)
    ip = ipeak.to(torch.int64).reshape(-1)
    ic = ip.clamp(0, F - 1)
    if F > 1:
        lo, hi = (ic - 1).clamp(0, F - 1), (ic + 1).clamp(0, F - 1)
        spacing = (xd[hi] - xd[lo]).abs() / (hi - lo).to(torch.float64)
    else:
        spacing = torch.ones_like(xd[ic])
    above = torch.isfinite(y) & (y >= 0.5 * mom[3].reshape(1, -1))
    big = torch.finfo(torch.float64).max
    xs = xd.reshape(-1, 1).expand(-1, y.shape[1])
    x_hi = torch.where(above, xs, torch.full_like(xs, -big)).amax(dim=0)
    x_lo = torch.where(above, xs, torch.full_like(xs, big)).amin(dim=0)
    hw = torch.maximum(0.5 * (x_hi - x_lo), spacing)
    live = ip >= 0
    nan = torch.full_like(hw, float("nan"))
    zero = torch.zeros_like(hw)
    pick = lambda t: torch.where(live, t, nan)
    return torch.stack([pick(mom[0].reshape(-1)), pick(xd[ic]), pick(hw / 1.1774 / 1.5),
                        pick(hw / 2.), zero, zero.clone()])


def _erfcx(a):
    """exp(a^2) erfc(a) in torch (`torch.special.erfcx`: no overflow, no cancellation)."""
    import torch
    return torch.special.erfcx(a)


def voigt_results(theta, cov, chi2, nchan, status, free=None, scale_errors=True):
    """Per-pixel maps of a Voigt fit (`RTEngine.voigtfit`'s `theta` [P, n], `cov` [P (P + 1) / 2,
    n], `chi2`, `nchan`, `status` [n]) -> dict of tensors on the same device, parallel to
    `specfit_results`.  Per component c (a list of n_comp tensors under each key): 'integral' (F),
    'centre' (x0), 'sigma' (s, the Doppler dispersion), 'fwhm_g' = s sqrt(8 ln 2), 'hwhm_l' (g, the
    Lorentz HWHM), 'fwhm_l' = 2 g, 'peak' = F erfcx(a) / (s sqrt(2 pi)) with a = g / (sqrt(2) s) (the
    profile at its centre: w(i a) = erfcx(a)), 'fwhm' = 0.5346 f_L + sqrt(0.2166 f_L^2 + f_G^2)
    (Olivero and Longbothum 1977: accurate to 0.02 % of the Voigt profile's true FWHM), and their
    'e_*' errors; 'b0', 'b1', 'e_b0', 'e_b1'; 'chi2', 'reduced_chi2' = chi2 / (nchan - n_free),
    'nchan', 'status'.  Errors as in `specfit_results`: the square roots of the diagonal of
    (N_ff)^-1 over the free parameters, times sqrt(reduced chi^2) with `scale_errors`; a fixed
    parameter's error is 0; the derived ones by first-order propagation: e_fwhm_g = sqrt(8 ln 2)
    e_s, e_fwhm_l = 2 e_g, var(fwhm) and var(peak) from the gradients with respect to (F, s, g) and
    their 3 x 3 covariance block (d erfcx / da = 2 a erfcx(a) - 2 / sqrt(pi)).  NaN wherever status
    == 3, a singular N_ff, or (for the scaled errors) nchan == n_free."""
    import torch
    P, n = int(theta.shape[0]), int(theta.shape[1])
    nc = (P - 2) // 4
    fr = np.ones(P, dtype=bool) if free is None else np.asarray(free).reshape(-1) != 0
    if fr.size != P or not fr.any():
        raise ValueError("voigt_results: `free` must hold %d flags, at least one of them set" % P)
    idx = [int(i) for i in np.nonzero(fr)[0]]
    bad = status.reshape(-1) == 3
    nan = float("nan")
    N = torch.zeros((n, P, P), dtype=torch.float64, device=theta.device)
    for k, (i, j) in enumerate(_tri(P)):
        N[:, i, j] = cov[k]
        N[:, j, i] = cov[k]
    Nff = N[:, idx][:, :, idx]
    eye = torch.eye(len(idx), dtype=torch.float64, device=theta.device)
    Nff = torch.where(bad[:, None, None] | ~torch.isfinite(Nff).all(dim=(1, 2), keepdim=True), eye, Nff)
    inv, info = torch.linalg.inv_ex(Nff)
    C = torch.zeros((n, P, P), dtype=torch.float64, device=theta.device)
    sub = torch.where((info != 0)[:, None, None], torch.full_like(inv, nan), inv)
    for a, i in enumerate(idx):
        for b, j in enumerate(idx):
            C[:, i, j] = sub[:, a, b]
    dof = (nchan.reshape(-1) - len(idx)).to(torch.float64)
    red = torch.where(dof > 0, chi2.reshape(-1) / dof, torch.full_like(dof, nan))
    if scale_errors:
        C = C * red[:, None, None]
    blank = lambda t: torch.where(bad, torch.full_like(t, nan), t)
    sd = lambda v: blank(torch.sqrt(v))
    keys = ("integral", "centre", "sigma", "fwhm_g", "hwhm_l", "fwhm_l", "peak", "fwhm")
    out = {k: [] for k in keys + tuple("e_" + k for k in keys)}
    inv_sqrt_pi = float(1. / np.sqrt(np.pi))
    for c in range(nc):
        o = 4 * c
        Fk, x0, s, g = theta[o], theta[o + 1], theta[o + 2], theta[o + 3]
        a = g / (float(np.sqrt(2.)) * s)
        ex = _erfcx(a)
        dex = 2. * a * ex - 2. * inv_sqrt_pi
        norm = 1. / (s * SQRT_2PI)
        peak = Fk * ex * norm
        fG, fL = s * FWHM_PER_SIGMA, 2. * g
        root = torch.sqrt(0.2166 * fL * fL + fG * fG)
        # gradients with respect to (F, s, g)
        g_peak = (ex * norm, -(Fk * norm / s) * (ex + a * dex), Fk * norm * dex / (float(np.sqrt(2.)) * s))
        g_fwhm = (torch.zeros_like(s), FWHM_PER_SIGMA * fG / root, 2. * (0.5346 + 0.2166 * fL / root))
        cols = (o, o + 2, o + 3)
        var = lambda gr: sum(gr[i] * gr[j] * C[:, cols[i], cols[j]] for i in range(3) for j in range(3))
        vals = dict(integral=Fk, centre=x0, sigma=s, fwhm_g=fG, hwhm_l=g, fwhm_l=fL, peak=peak,
                    fwhm=0.5346 * fL + root)
        errs = dict(integral=sd(C[:, o, o]), centre=sd(C[:, o + 1, o + 1]), sigma=sd(C[:, o + 2, o + 2]),
                    fwhm_g=sd(C[:, o + 2, o + 2]) * FWHM_PER_SIGMA, hwhm_l=sd(C[:, o + 3, o + 3]),
                    fwhm_l=2. * sd(C[:, o + 3, o + 3]), peak=sd(var(g_peak)), fwhm=sd(var(g_fwhm)))
        for k in keys:
            out[k].append(blank(vals[k]))
            out["e_" + k].append(errs[k])
    out.update(b0=blank(theta[P - 2]), b1=blank(theta[P - 1]), e_b0=sd(C[:, P - 2, P - 2]),
               e_b1=sd(C[:, P - 1, P - 1]), chi2=blank(chi2.reshape(-1)), reduced_chi2=blank(red),
               nchan=nchan.reshape(-1), status=status.reshape(-1))
    return out


class Spectra:
    """Moment maps and line fits of (F, ni, nj) cubes on the device of an `RTEngine`."""

    def __init__(self, engine):
        self.engine = engine

    def _cube(self, who, cube):
        """(F, ni, nj) or (F, n_pix), host array or device tensor -> (device [F, n_pix], shape)."""
        import torch
        if not isinstance(cube, torch.Tensor):
            cube = torch.from_numpy(np.ascontiguousarray(cube, dtype=np.float64))
        if cube.dim() not in (2, 3) or cube.numel() < 1:
            raise ValueError("%s: `cube` must be (F, ni, nj) or (F, n_pix)" % who)
        d = cube.to(device=self.engine.device, dtype=torch.float64).contiguous()
        return d.reshape(d.shape[0], -1), tuple(d.shape[1:])

    @staticmethod
    def _x_ref(x):
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        return x, float(x[x.size // 2])

    def moments(self, cube, x, dx=None, clip=0., mask=None):
        """`RTEngine.cube_moments` of a cube with the mid-channel as `x_ref` -> dict of device
        tensors shaped like a plane of the cube: 'm0', 'm1', 'm2', 'peak', 'ipeak', 'count'.
        `dx`: the channel widths, None = those of `velocity_axis` (half the distance between the
        neighbours, one-sided at the ends) on `x`."""
        d, shape = self._cube("moments", cube)
        x, x_ref = self._x_ref(x)
        if dx is None:
            dx = channel_widths(x)
        mom, ipeak, count = self.engine.cube_moments(d, x, dx, x_ref, clip, mask)
        out = {k: mom[i].reshape(shape) for i, k in enumerate(("m0", "m1", "m2", "peak"))}
        out.update(ipeak=ipeak.reshape(shape), count=count.reshape(shape))
        return out

    def specfit(self, cube, x, weights=None, comps=1, theta0=None, free=None, n_iter=40, mask=None,
                scale_errors=True):
        """`RTEngine.specfit` of a cube with the mid-channel as `x_ref`, started from the moments
        (`specfit_start`) unless `theta0` ([P] or [P, n_pix]; needed for two components) is given
        -> `specfit_results`, every map shaped like a plane of the cube, plus 'niter'."""
        import torch
        d, shape = self._cube("specfit", cube)
        x, x_ref = self._x_ref(x)
        comps = int(comps)
        P = n_params(comps)
        npix = d.shape[1]
        if theta0 is None:
            mom, ipeak, _ = self.engine.cube_moments(d, x, channel_widths(x), x_ref, 0., mask)
            theta = specfit_start(mom, ipeak, x, comps)
        else:
            theta = theta0 if isinstance(theta0, torch.Tensor) else \
                torch.from_numpy(np.ascontiguousarray(theta0, dtype=np.float64))
            theta = theta.to(device=self.engine.device, dtype=torch.float64)
            if theta.dim() == 1:
                theta = theta.reshape(-1, 1).expand(-1, npix)
            theta = theta.reshape(theta.shape[0], -1)
        fit = self.engine.specfit(d, x, theta, x_ref, weights=weights, free=free, n_comp=comps,
                                  n_iter=n_iter, mask=mask)
        res = specfit_results(fit["theta"], fit["cov"], fit["chi2"], fit["nchan"], fit["status"],
                              free if free is not None else np.ones(P, dtype=bool), scale_errors)
        res["niter"] = fit["niter"]
        return {k: ([t.reshape(shape) for t in v] if isinstance(v, list) else v.reshape(shape))
                for k, v in res.items()}

    def voigtfit(self, cube, x, weights=None, comps=1, theta0=None, free=None, n_iter=40, mask=None,
                 scale_errors=True):
        """`RTEngine.voigtfit` of a cube with the mid-channel as `x_ref`, started from the cube and
        its moments (`voigt_start`) unless `theta0` ([P] or [P, n_pix], P = 4 comps + 2; needed for
        two components) is given -> `voigt_results`, every map shaped like a plane of the cube,
        plus 'niter'."""
        import torch
        d, shape = self._cube("voigtfit", cube)
        x, x_ref = self._x_ref(x)
        comps = int(comps)
        P = voigt_n_params(comps)
        npix = d.shape[1]
        if theta0 is None:
            if comps != 1:
                raise ValueError("voigtfit: only one component can be started from the moments; "
                                 "pass `theta0` for two")
            mom, ipeak, _ = self.engine.cube_moments(d, x, channel_widths(x), x_ref, 0., mask)
            theta = voigt_start(d, mom, ipeak, x)
        else:
            theta = theta0 if isinstance(theta0, torch.Tensor) else \
                torch.from_numpy(np.ascontiguousarray(theta0, dtype=np.float64))
            theta = theta.to(device=self.engine.device, dtype=torch.float64)
            if theta.dim() == 1:
                theta = theta.reshape(-1, 1).expand(-1, npix)
            theta = theta.reshape(theta.shape[0], -1)
        fit = self.engine.voigtfit(d, x, theta, x_ref, weights=weights, free=free, n_comp=comps,
                                   n_iter=n_iter, mask=mask)
        res = voigt_results(fit["theta"], fit["cov"], fit["chi2"], fit["nchan"], fit["status"],
                            free if free is not None else np.ones(P, dtype=bool), scale_errors)
        res["niter"] = fit["niter"]
        return {k: ([t.reshape(shape) for t in v] if isinstance(v, list) else v.reshape(shape))
                for k, v in res.items()}
