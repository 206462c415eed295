"""What tests/test_fit_ejections_reference_cpu.py and tests/test_gpu_fit_ejections.py share: the
`tilted` model of the oracle as a `JetModel`, the choices of the fits (epochs, channels, ties,
start, tolerances, the noise and its seed) and device-free evaluations of the model -- light curves
and their Jacobian from tests/ff_grad_ref.py (K7, isothermal), visibilities and their Jacobian from
tests/ff_formal_grad_ref.py (K9's walk) through a direct Fourier sum in the convention of
`RTEngine.vis`, thermal noise from tests/observe_ref.py's float64 emulation of rjp_vis_noise -- as
the `sums` callback of `BurstFit._run`, so that the very loop, layout, chain rule and ties of the
device fits run on the CPU.  No GPU, no test."""
import copy
import functools
import os

import numpy as np

from rajepy_amd import classes, imaging, inference, logger
from rajepy_amd import engine as E
from rajepy_amd.maths import physics as ph
from tests import ff_formal_grad_ref as R9
from tests import ff_grad_ref as R7
from tests import gpu_util as U
from tests import normal_eq_ref as K
from tests import observe_ref as O

YEAR = 31557600.0
FIXTURE = os.path.join(U.GOLDEN, "antenna_configs", "vla.a.cfg")
# (0.15 + 0.25 i yr: past the second burst's maximum, where the curves turn over -- the smallest pivot of
# the scaled N is 4e-4; epochs that end on the rise, such as 0.3 .. 1.35 yr, leave it at 2e-7)
EPOCHS_YR = (0.15, 0.40, 0.65, 0.90, 1.15, 1.40, 1.65, 1.90)
CHANNELS = 2                                             # the first two golden channels: 5 and 1.5 GHz
RB_TIE = [[("1", n), ("2", n)] for n in ("t_0", "peak_jml", "half_life")]
START = np.array([[1.02, 0.98, 1.02], [1.02, 0.98, 1.02], [0.98, 1.02, 0.98]])   # x the truth: 2 % off
# (from 4-5 % off the same fit wanders along the valley of the third event's peak for 47 trials before it
# converges to the same point: the rule's factor-of-ten lambda steps, not the data, set that pace)
RECOVERY = 1.1e-12      # MEASURED by the CPU test: the worst relative error of the noise-free fit (1.01e-12)
# The step test stops a fit when the PROPOSED step is below XTOL of its scale (half_life, |peak_jml|,
# half_life), and that step is not taken: what the rule itself guarantees of a converged fit is an error
# of the order of XTOL, so XTOL has to lie below RECOVERY for the bar to follow from status 1.
N_ITER, XTOL = 30, 1e-12
# The noisy fits: thermal noise of NOISE_REL x the largest |V| per real and imaginary part from
# rjp_vis_noise with NOISE_SEED (chosen by the CPU test, which says how), weights 1 / sigma^2.  A step of
# 1e-6 of a scale is far inside every error bar.
NOISE_SEED, NOISE_REL = 1, 1e-3
NOISY_ITER, NOISY_XTOL = 60, 1e-6


def tilted(tmp_path, engine=None):
    p = copy.deepcopy(U.load_golden("tilted")[2])
    for k in ("mod_r_0",):
        p["geometry"].pop(k, None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return classes.JetModel(p, log=logger.Log(str(tmp_path / "m.log"), verbose=False), engine=engine)


def truth_of(jm):
    return np.array([[ej[n] for n in inference.PARAM_NAMES] for ej in jm.ejections.values()])


def channel_coeffs(p, csize, freqs):
    mode = E.RJP_GFF_SCALAR if p["power_laws"]["q_T"] == 0. else E.RJP_GFF_POWERLAW
    gv = [ph.gff(nu, p["properties"]["T_0"]) for nu in freqs] if mode == E.RJP_GFF_SCALAR else None
    return E.ff_channel_coeffs(freqs, csize, p["target"]["dist"], mode, gv)


@functools.lru_cache(maxsize=1)
def host_fields():
    """The 468 sightlines of `tilted` that meet the jet, as [468, n_y, 1] arrays; a cell outside the
    jet (NaN: a skipped term) becomes a weight of 0 at launch time 0 and temperature 0, which adds the
    same nothing without NaN arithmetic."""
    z, meta, p, g, jet = U.golden_dense("tilted")
    a0 = U.golden_a0(g, p["power_laws"]["q_T"])
    with np.errstate(all="ignore"):
        hot = g["temp"] > 0
        tavg = np.where(hot, g["temp"], 0.0).sum(axis=1) / hot.sum(axis=1)        # NaN where no T > 0
    freqs = np.asarray(z["freqs"], dtype=np.float64)[:CHANNELS]
    ctau, cflux = channel_coeffs(p, jet.csize, freqs)
    ix, iz = np.nonzero(np.isfinite(a0).any(axis=1))
    inside = np.isfinite(a0[ix, :, iz])
    crop = lambda a: np.where(inside, a[ix, :, iz], 0.0)[:, :, None]
    nx, ny, nz = a0.shape
    su, sv = imaging.vis_scales(freqs, jet.csize, p["target"]["dist"])
    return dict(a0=crop(a0), ts=crop(g["ts"]), temp=crop(g["temp"]), tavg=tavg[ix, iz][:, None], freqs=freqs,
                ctau=np.asarray(ctau), cflux=np.asarray(cflux), su=su, sv=sv,
                x=ix - (nx - 1) / 2.0, z=iz - (nz - 1) / 2.0)


def light_curves(bursts):
    """(F [E, F], dF [E, F, n_par]) of per-jet burst lists at EPOCHS_YR by the K7 reference."""
    h = host_fields()
    F, dF = [], []
    for yr in EPOCHS_YR:
        tot = R7.totals(R7.planes(h["a0"], h["ts"], bursts, yr * YEAR), h["tavg"], h["ctau"], h["cflux"])
        F.append(tot["F"])
        dF.append(tot["dF"])
    return np.array(F), np.array(dF)


def visibilities(bursts, u, v):
    """(V [E, F, K], dV [E, F, n_par, K]) complex128 at EPOCHS_YR: K9's reference walk (the formal
    solution and its derivative maps) and V = sum_p I_p exp(-2 pi i (su u x_p + sv v z_p))."""
    h = host_fields()
    V, dV = [], []
    for yr in EPOCHS_YR:
        res = R9.walk(h["a0"], h["ts"], h["temp"], bursts, yr * YEAR, h["ctau"], h["cflux"])
        I = np.asarray(res["I"][:, :, 0], dtype=np.float64)                    # [F, pix]
        dI = np.asarray(res["dI"][:, :, :, 0], dtype=np.float64)               # [F, n_par, pix]
        ph_ = np.exp(-2j * np.pi * (h["su"][:, None, None] * u[None, None, :] * h["x"][None, :, None] +
                                    h["sv"][:, None, None] * v[None, None, :] * h["z"][None, :, None]))
        V.append(np.einsum("fp,fpk->fk", I, ph_))
        dV.append(np.einsum("fnp,fpk->fnk", dI, ph_))
    return np.array(V), np.array(dV)


def bursts_of(jm):
    return [jm._bursts["R"], jm._bursts["B"]]


def _lists(bursts):
    """An rjp_bursts struct back to the per-jet lists (t0, amp_rel, sigma) the references take."""
    return [[(bursts.t0[j][i], bursts.amp_rel[j][i], (0.5 / bursts.inv2s2[j][i]) ** 0.5)
             for i in range(bursts.n[j])] for j in range(2)]


def flux_sums(data, sigma=None):
    """The `sums` callback of BurstFit._run for light curves: what the device path computes with ff_grad
    and rjp_normal_eq, here with the K7 reference and the float64 emulation of tests/normal_eq_ref.py."""
    w = None if sigma is None else np.full((data.size, 1), 1.0 / sigma ** 2)

    def sums(bursts, n_par, sel, want_jac):
        F, dF = light_curves(_lists(bursts))
        out = K.sums(data.reshape(-1, 1), F.reshape(-1, 1), dF.reshape(-1, n_par, 1), sel, w, 1, T=np.float64)
        return float(out["chi2"]), out["g"], out["N"], out["count"]
    return sums


def vis_sums(data, u, v, w=None):
    """... and for visibilities [E, F, K] with weights [K] or [E F, K]."""
    Kv = u.size

    def sums(bursts, n_par, sel, want_jac):
        V, dV = visibilities(_lists(bursts), u, v)
        out = K.sums(data.reshape(-1, Kv), V.reshape(-1, Kv), dV.reshape(-1, n_par, Kv), sel, w, 2, T=np.float64)
        return float(out["chi2"]), out["g"], out["N"], out["count"]
    return sums


def fit(jm, sums, n_part, theta0, trace=False, n_iter=N_ITER, xtol=XTOL):
    bf = inference.BurstFit(jm)
    lay = bf.layout(None, RB_TIE, theta0)
    return bf._run(lay, sums, n_part, n_iter, 1e-3, xtol, False, trace), lay


def host_baselines(jm):
    """(u, v) [39] in metres: every ninth baseline of one 60 s integration of the 27-antenna fixture at
    the model's declination, by the host half of `JetModel.uv_tracks` and the float64 track reference
    (the device's tracks agree with it to a few ulp)."""
    from rajepy_amd.miscellaneous import functions as miscf
    cfg = imaging.read_antenna_config(FIXTURE)
    geo = imaging.geodetic(cfg.xyz)
    tg = jm.params["target"]
    dec = miscf.sexagesimal_to_deg(tg["ra"], tg["dec"])[1]
    ha, _ = imaging.observing_plan(dec, geo.lat0_deg, 60.0, 60.0, 0., 0.)
    t = O.tracks_ref(cfg.xyz, ha - geo.lon0_deg / 360., np.sin(np.radians(dec)), np.cos(np.radians(dec)),
                     dtype=np.float64)
    return t["u"].reshape(-1)[:351:9].copy(), t["v"].reshape(-1)[:351:9].copy()


def noisy(V, seed=NOISE_SEED):
    """(V + thermal noise [E, F, K], sigma): rjp_vis_noise's float64 emulation on the stack [E F, K]."""
    sigma = NOISE_REL * float(np.abs(V).max())
    M, Kv = V.shape[0] * V.shape[1], V.shape[2]
    ri = np.stack([V.real, V.imag], axis=-1).reshape(M, Kv, 2)
    out = O.noise_f64(ri, np.full(M, sigma), None, seed)
    return (out[..., 0] + 1j * out[..., 1]).reshape(V.shape), sigma


def laws(R, truth, n_free):
    """The chi^2 and normal laws of a fit with known sigma: -> (|reduced chi2 - 1| / (5 sqrt(2 / nu)), the
    worst |theta - truth| / (5 reported errors)); both must be <= 1."""
    nu = R.ndata - n_free
    pulls = [abs(R.theta[i, c] - truth[i, c]) / (5.0 * ej["e_" + name])
             for i, ej in enumerate(R.ejections.values()) for c, name in enumerate(inference.PARAM_NAMES)]
    return abs(R.reduced_chi2 - 1.0) / (5.0 * np.sqrt(2.0 / nu)), max(pulls)

