"""SHA-256 of every result array of a fixed list of small imaging calls, through the public
`JetModel` API only: run it at two commits and compare the lines -- equal digests are equal bits.

The smallest model of the GPU imaging tests (cfg1_example), 3 channels, 45 baselines x 3
integrations of ten antennas of tests/golden/antenna_configs/vla.a.cfg with one NaN baseline,
images of (17, 15) cells; VIS_STACK_BYTES is set per call so that the 3 channels split into
chunks of 2 + 1.  A call that raises prints the exception instead: that, too, must not change.

    python tools/imaging_digest.py        (needs a GPU; reads nothing outside the repository)
"""
import copy
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rajepy_amd import classes, engine as E, logger      # noqa: E402
from tests import gpu_util as U                          # noqa: E402

YEAR = 31557600.0
SHAPE, WINDOW = (17, 15), (9, 11)
NPIX, NPSF = SHAPE[0] * SHAPE[1], (2 * SHAPE[0] - 1) * (2 * SHAPE[1] - 1)


def digest(name, value):
    """One line per array of `value`: arrays, tuples / lists / dicts of them, fit dicts."""
    if isinstance(value, dict):
        if all(isinstance(v, np.ndarray) for v in value.values()):
            for k in sorted(value):
                digest(name + "." + k, value[k])
        else:
            text = json.dumps(value, sort_keys=True, default=lambda x: np.asarray(x).tolist())
            print("%-44s %s" % (name, hashlib.sha256(text.encode()).hexdigest()))
    elif isinstance(value, classes.CleanResult):
        for k in value._fields:
            digest(name + "." + k, getattr(value, k))
        digest(name + ".imfit", value.imfit)
    elif isinstance(value, classes.Observation):
        for k in ("vis_clean", "vis", "sigma", "image_rms", "clean"):
            digest(name + "." + k, getattr(value, k))
    elif isinstance(value, (list, tuple)):
        for i, v in enumerate(value):
            digest("%s[%d]" % (name, i), v)
    elif value is None:
        print("%-44s None" % name)
    else:
        a = np.ascontiguousarray(value)
        live = np.abs(a[np.isfinite(a)])                 # (so that a NaN-only result shows)
        print("%-44s %s %s %s finite=%d max=%.3e" % (name, hashlib.sha256(a.tobytes()).hexdigest(),
                                                     a.dtype, a.shape, live.size,
                                                     live.max() if live.size else 0.))


def main():
    z, meta, p = U.load_golden("cfg1_example")
    p = copy.deepcopy(p)
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    eng = E.RTEngine(0)
    log = logger.Log(os.path.join(tempfile.mkdtemp(), "model.log"), verbose=False)
    jm = classes.JetModel(p, log=log, engine=eng)
    jm.time = 1.0 * YEAR
    freqs = np.asarray(z["freqs"], dtype=np.float64)[:3]
    rf = np.asarray(z["rrl_freqs"], dtype=np.float64)[2:5]
    line = meta["rrl"]

    cfg = E.read_antenna_config(os.path.join(U.GOLDEN, "antenna_configs", "vla.a.cfg"))
    pick = list(range(0, 27, 3)) + [1]                   # ten antennas over the three arms
    cfg = E.AntennaConfig([cfg.names[i] for i in pick], cfg.xyz[pick], cfg.diameters[pick],
                          cfg.observatory)
    tracks = jm.uv_tracks(cfg, 180., 60., min_el_deg=10.)
    u_d = tracks.u_m.clone()
    u_d[7] = float("nan")
    tracks = tracks._replace(u_m=u_d)
    u, v = tracks.u_m.cpu().numpy(), tracks.v_m.cpu().numpy()
    K = u.size
    w = 0.5 + (np.arange(K) % 7) / 7.
    cell_as = E.observation_grid(tracks.max_baseline_m, max(freqs.max(), rf.max()), 1.0)[0]
    grid = dict(shape=SHAPE, cell_as=cell_as)
    digest("uv_tracks", [u, v, tracks.w_m.cpu().numpy(), tracks.ha_h, tracks.day])

    def call(name, budget, fn, *args, **kw):
        jm.VIS_STACK_BYTES = int(budget)
        try:
            digest(name, fn(*args, **kw))
        except Exception as exc:                         # the refusal is the result
            print("%-44s %s: %s" % (name, type(exc).__name__, exc))
        finally:
            del jm.VIS_STACK_BYTES

    big = classes.JetModel.VIS_STACK_BYTES
    call("visibilities_ff", big, jm.visibilities_ff, u, v, freqs)
    call("visibilities_rrl", big, jm.visibilities_rrl, line, u, v, rf)
    for tag, weights, scheme, robust in (("natural", None, None, 0.5), ("natural+w", w, None, 0.5),
                                         ("uniform", w, "uniform", 0.5), ("briggs", w, "briggs", -0.5)):
        for mfs in (False, True):
            t = "%s%s" % (tag, ".mfs" if mfs else "")
            ff_w = weights if scheme is None else classes.Weighting(scheme, robust, weights)
            call("dirty_image_ff." + t, 2 * NPIX * 8, jm.dirty_image_ff, u, v, freqs, weights=ff_w,
                 mfs=mfs, **grid)
            call("dirty_image_rrl." + t, 2 * NPIX * 8, jm.dirty_image_rrl, line, u, v, rf,
                 weights=weights, mfs=mfs, weighting=scheme, robust=robust, **grid)
            call("dirty_beam." + t, 2 * NPIX * 8, jm.dirty_beam, u, v, freqs, weights=weights,
                 mfs=mfs, weighting=scheme, robust=robust, **grid)
            call("imaging_weights." + t, 2 * K * 8, jm.imaging_weights, u, v, freqs, weights=weights,
                 mfs=mfs, weighting=scheme, robust=robust, **grid)
    full, win = 2 * (3 * NPIX + NPSF) * 8, 2 * (3 * NPIX + WINDOW[0] * WINDOW[1]) * 8
    call("clean_image_ff.box.window", win, jm.clean_image_ff, u, v, freqs, weights=w, niter=40,
         gain=0.2, mask=(3, 13, 2, 12), psf_shape=WINDOW, **grid)
    call("clean_image_ff.thresholds", full, jm.clean_image_ff, u, v, freqs, niter=40,
         threshold_jy=np.array([1e-7, 2e-7, 4e-7]), **grid)
    call("clean_image_ff.imfit.briggs", full, jm.clean_image_ff, u, v, freqs, weights=w, niter=40,
         imfit=True, weighting="briggs", robust=0.5, **grid)
    call("clean_image_ff.imfit.mfs", full, jm.clean_image_ff, u, v, freqs, niter=40, imfit=True,
         mfs=True, formal=True, **grid)
    call("observe_ff.noise_free", full, jm.observe_ff, tracks, freqs, 180., 60., niter=40, **grid)
    call("observe_ff.noisy.mfs.imfit", full, jm.observe_ff, tracks, freqs, 180., 60.,
         sigma_jy=1e-5, seed=7, nsigma=3., mfs=True, imfit=True, niter=40, weighting="briggs", **grid)
    call("observe_rrl.cube", win, jm.observe_rrl, line, tracks, rf, 180., 60., sigma_jy=[1e-5, 2e-5, 0.],
         seed=7, weights=w, niter=40, psf_shape=WINDOW, **grid)
    eng.close()


if __name__ == "__main__":
    main()
