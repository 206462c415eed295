"""The inputs of K24's tests, built once and shared: tests/test_voigtfit_reference_cpu.py runs the
float64 emulation (tests/voigtfit_ref.py) on them, tests/test_gpu_voigtfit.py the device.  A case
is a dict: Y [n_pix, n_chan], x, x_ref, w (or None), live (or None), free (or None), theta0
[n_pix, P], truth [n_pix, P] (or None), n_comp, follow (the pixels the reference follows: following
costs a 30-digit w(z) per channel and trial)."""
import numpy as np

from tests import voigtfit_ref as R

LAM0, XTOL, N_ITER = 1e-3, 1e-10, 40
# On noisy data the last steps before |delta| / scale <= 1e-10 change chi^2 by less than its rounding:
# their accept decisions could not be judged.  The noisy cases stop at 1e-6.
XTOL_NOISY = 1e-6
# (n_comp, baseline free, n_chan, n_pix): P_free channels (an exactly determined fit) to 257 channels,
# 1 to 257 pixels (every tail of a wave, five workgroups)
SIZED = [(1, False, 4, 1), (1, True, 6, 63), (1, False, 33, 64), (1, True, 64, 65), (1, False, 257, 3),
         (2, False, 34, 257), (2, True, 41, 130), (2, True, 10, 2)]


def axis(kind, n_chan, half=300.0):
    """uniform ascending, descending, or non-uniform (a smooth stretch) over +-half"""
    t = np.linspace(-1.0, 1.0, n_chan) if n_chan > 1 else np.zeros(1)
    if kind == 1:
        t = t[::-1].copy()
    if kind == 2:
        t = t + 0.25 * t * t * np.sign(t)
        t = t / 1.25
    return half * t


def weights(kind, n_chan, rng):
    if kind == 0:
        return None
    w = rng.uniform(0.5, 2.0, n_chan)
    if kind == 2 and n_chan > 12:
        w[rng.choice(n_chan, n_chan // 8, replace=False)] = 0.0
    return w


def make(theta, x, x_ref, n_comp):
    return np.array([R.profile(t, x, x_ref, n_comp).astype(np.float64) for t in theta])


def truth_one(n_pix, rng, ratio_lo=0.05, ratio_hi=20.0):
    """(F, x0, s, g, b0, b1) with g / s log-uniform in the range and the wider of the two 8 to 40"""
    ratio = np.exp(rng.uniform(np.log(ratio_lo), np.log(ratio_hi), n_pix))
    wide = rng.uniform(8.0, 40.0, n_pix)
    s = np.where(ratio > 1, wide / ratio, wide)
    g = s * ratio
    return np.stack([rng.uniform(50.0, 500.0, n_pix), rng.uniform(-40.0, 40.0, n_pix), s, g,
                     np.zeros(n_pix), np.zeros(n_pix)], axis=1)


def start_one(Y, x):
    """`voigt_start` on the host (tests hold the torch version to this), baseline 0"""
    n = Y.shape[0]
    th = np.full((n, 6), np.nan)
    dx = np.zeros_like(x)
    if x.size > 1:
        dx[1:-1] = 0.5 * np.abs(x[2:] - x[:-2])
        dx[0], dx[-1] = abs(x[1] - x[0]), abs(x[-1] - x[-2])
    for p in range(n):
        y = Y[p]
        ok = np.isfinite(y)
        if not ok.any() or np.sum(y[ok] * dx[ok]) == 0.0:
            continue
        yy = np.where(ok, y, -np.inf)
        ip = int(np.argmax(yy))
        lo, hi = max(ip - 1, 0), min(ip + 1, x.size - 1)
        spacing = abs(x[hi] - x[lo]) / (hi - lo) if hi > lo else 1.0
        above = ok & (yy >= 0.5 * yy[ip])
        hw = max(0.5 * (x[above].max() - x[above].min()), spacing)
        th[p] = [np.sum(y[ok] * dx[ok]), x[ip], hw / 1.1774 / 1.5, hw / 2.0, 0.0, 0.0]
    return th


def sized(n_comp, bl, n_chan, n_pix):
    rng = np.random.default_rng(2400 + 1000 * n_comp + 10 * n_chan + int(bl))
    kind = (n_chan + n_comp) % 3
    x = axis(kind, n_chan)
    x_ref = float(x[n_chan // 2])
    w = weights(n_chan % 3, n_chan, rng)
    t1 = truth_one(n_pix, rng, 0.1, 10.0)
    P = 4 * n_comp + 2
    truth = np.zeros((n_pix, P))
    truth[:, :4] = t1[:, :4]
    if n_comp == 2:
        t2 = truth_one(n_pix, rng, 0.2, 5.0)
        t2[:, 1] = truth[:, 1] + np.where(rng.uniform(size=n_pix) < 0.5, -1, 1) * rng.uniform(90., 140., n_pix)
        t2[:, 2:4] = np.maximum(0.5 * t2[:, 2:4], 8.0)       # (no line narrower than a channel here: `narrow`)
        truth[:, 4:8] = t2[:, :4]
    if bl:
        truth[:, P - 2] = rng.uniform(-0.2, 0.2, n_pix)
        truth[:, P - 1] = rng.uniform(-1e-3, 1e-3, n_pix)
    Y = make(truth, x, x_ref, n_comp)
    noisy = n_chan % 2 == 1 and n_chan > P
    if noisy:
        Y = Y + 0.01 * Y.max(axis=1, keepdims=True) * rng.standard_normal(Y.shape)
    # (two blended components are started closer: a 15 % start, and a 4 % one, leave a few of 257 short of
    # convergence after 40 trials, on the emulation as on the device)
    off, dx0 = (0.15, 4.0) if n_comp == 1 else (0.02, 0.5)
    theta0 = truth * (1.0 + off * rng.uniform(-1, 1, truth.shape))
    theta0[:, 1::4][:, :n_comp] = truth[:, 1::4][:, :n_comp] + rng.uniform(-dx0, dx0, (n_pix, n_comp))
    if not bl:
        theta0[:, P - 2:] = 0.0
    free = None if bl else [1] * (4 * n_comp) + [0, 0]
    follow = sorted(set([0, n_pix - 1, n_pix // 2]))[: (3 if n_chan <= 65 else 1)]
    return dict(Y=Y, x=x, x_ref=x_ref, w=w, live=None, free=free, theta0=theta0,
                truth=None if noisy else truth, n_comp=n_comp, follow=follow, noisy=noisy,
                xtol=XTOL_NOISY if noisy else XTOL)


def must_converge(case):
    """noise-free data on at least 33 channels: every pixel must end with status 1 at the truth"""
    return case["truth"] is not None and case["Y"].shape[1] >= 33


def scaled_error(theta, truth, n_comp=1):
    """max |theta - truth| / scale, the step scales of the rule at the truth (line parameters)"""
    worst = 0.0
    for p in range(theta.shape[0]):
        s = R.scales(truth[p], n_comp)
        worst = max(worst, float(np.max(np.abs(theta[p] - truth[p])[:4 * n_comp] / s[:4 * n_comp])))
    return worst


def ratios():
    """g / s from exactly 0 to 20 on 48 channels over +-300, from `start_one`:
    (s, g) = (9.1, 0.5), (9.1, 9), (9.1, 60), (20, 2), (20, 200), (21.4, 130), (20, 0) and (8, 160)"""
    x = axis(0, 48)
    sg = [(9.1, 0.5), (9.1, 9.0), (9.1, 60.0), (20.0, 2.0), (20.0, 200.0), (21.4, 130.0), (20.0, 0.0),
          (8.0, 160.0)]
    truth = np.array([[100.0, 3.0 + p, s, g, 0.0, 0.0] for p, (s, g) in enumerate(sg)])
    Y = make(truth, x, 0.0, 1)
    return dict(Y=Y, x=x, x_ref=0.0, w=None, live=None, free=[1, 1, 1, 1, 0, 0], theta0=start_one(Y, x),
                truth=truth, n_comp=1, follow=list(range(len(sg))))


def held():
    """g held at 0 on Gaussian data (a Gaussian fit in area form: pixels 0-2) and s held at the known
    thermal width (pixels 3-5), two calls' worth of `free` -> (case_g0, case_s)"""
    x = axis(2, 48)
    rng = np.random.default_rng(2431)
    t = truth_one(6, rng, 0.2, 5.0)
    tg = t[:3].copy()
    tg[:, 3] = 0.0
    Yg = make(tg, x, 0.0, 1)
    th0 = start_one(Yg, x)
    th0[:, 3] = 0.0
    a = dict(Y=Yg, x=x, x_ref=0.0, w=None, live=None, free=[1, 1, 1, 0, 0, 0], theta0=th0, truth=tg,
             n_comp=1, follow=[0, 2])
    ts = t[3:].copy()
    Ys = make(ts, x, 0.0, 1)
    th0 = start_one(Ys, x)
    th0[:, 2] = ts[:, 2]
    b = dict(Y=Ys, x=x, x_ref=0.0, w=None, live=None, free=[1, 1, 0, 1, 0, 0], theta0=th0, truth=ts,
             n_comp=1, follow=[0, 2])
    return a, b


def bad_data():
    """NaN / inf channels (0, 1), an all-NaN pixel (2), a starved one (3: three counted channels for
    four free parameters), a masked one (4), a sound one (5), weights with zeros"""
    x = axis(0, 40)
    rng = np.random.default_rng(2432)
    truth = truth_one(6, rng, 0.3, 3.0)
    Y = make(truth, x, 0.0, 1)
    theta0 = start_one(Y, x)
    Y[0, [3, 17, 30]] = np.nan
    Y[1, [0, 21]] = [np.inf, -np.inf]
    Y[2, :] = np.nan
    Y[3, :] = np.nan
    Y[3, [18, 20, 22]] = 1.0
    w = np.ones(40)
    w[[5, 6]] = 0.0
    live = np.array([1, 1, 1, 1, 0, 1], dtype=np.uint8)
    theta0[2] = theta0[3] = theta0[5]
    return dict(Y=Y, x=x, x_ref=0.0, w=w, live=live, free=[1, 1, 1, 1, 0, 0], theta0=theta0, truth=truth,
                n_comp=1, follow=[0, 1, 2, 3, 4, 5], degenerate=[2, 3, 4])


def degenerate_starts():
    """starts with s = 0 (0), s < 0 (1), g < 0 (2), NaN (3), inf (4); a sound one with g = 0 (5)"""
    x = axis(1, 40)
    rng = np.random.default_rng(2433)
    truth = truth_one(6, rng, 0.3, 3.0)
    Y = make(truth, x, 0.0, 1)
    theta0 = start_one(Y, x)
    theta0[0, 2] = 0.0
    theta0[1, 2] = -3.0
    theta0[2, 3] = -1e-300
    theta0[3, 0] = np.nan
    theta0[4, 5] = np.inf
    theta0[5, 3] = 0.0
    return dict(Y=Y, x=x, x_ref=0.0, w=None, live=None, free=[1, 1, 1, 1, 0, 0], theta0=theta0, truth=truth,
                n_comp=1, follow=[0, 1, 2, 3, 4, 5], degenerate=[0, 1, 2, 3, 4])


def negative_g_trial():
    """Gaussian data (g = 0 exactly) with g free and a start at g = 0.3 s: the first step proposes a
    g < 0, which the rule rejects as infeasible (pixel 0: the emulation's trace shows the rejected
    row); pixel 1 the same from g = 0."""
    x = axis(0, 48)
    truth = np.array([[100.0, 3.0, 20.0, 0.0, 0.0, 0.0], [80.0, -5.0, 15.0, 0.0, 0.0, 0.0]])
    Y = make(truth, x, 0.0, 1)
    theta0 = truth.copy()
    theta0[0, 2:4] = [17.0, 6.0]
    theta0[1, 2:4] = [17.0, 0.0]
    return dict(Y=Y, x=x, x_ref=0.0, w=None, live=None, free=[1, 1, 1, 1, 0, 0], theta0=theta0, truth=truth,
                n_comp=1, follow=[0, 1])


def narrow():
    """the line narrower than a channel: s = 5, g = 0 on 12.8-unit channels (the documented hard
    case: no convergence is asked, the trace is followed) and s = 5, g = 4 beside it"""
    x = axis(0, 48)
    truth = np.array([[100.0, 3.0, 5.0, 0.0, 0.0, 0.0], [100.0, -2.0, 5.0, 4.0, 0.0, 0.0]])
    Y = make(truth, x, 0.0, 1)
    return dict(Y=Y, x=x, x_ref=0.0, w=None, live=None, free=[1, 1, 1, 1, 0, 0], theta0=start_one(Y, x),
                truth=truth, n_comp=1, follow=[0, 1])


def flat(bl):
    """flat spectra: zeros (0), a constant (1), beside a sound line (2, on a baseline where that is
    free: a free baseline parameter at 0 has no scale to converge against); the baseline free or held"""
    x = axis(0, 40)
    truth = np.array([[100.0, 3.0, 20.0, 10.0, 0.3 if bl else 0.0, 1e-3 if bl else 0.0]])
    Y = np.vstack([np.zeros(40), np.full(40, 0.5), make(truth, x, 0.0, 1)[0]])
    theta0 = np.array([[1.0, 0.0, 20.0, 5.0, 0.0, 0.0], [1.0, 0.0, 20.0, 5.0, 0.0, 0.0],
                       [90.0, 0.0, 17.0, 12.0, 0.0, 0.0]])
    return dict(Y=Y, x=x, x_ref=0.0, w=None, live=None, free=None if bl else [1, 1, 1, 1, 0, 0],
                theta0=theta0, truth=None, n_comp=1, follow=[0, 1, 2])


def big_stack(n_pix=130 * 65, n_chan=64):
    """130 x 65 noise-free sightlines with random g / s in [0.05, 20] on 64 channels over +-300"""
    rng = np.random.default_rng(2440)
    x = axis(0, n_chan)
    truth = truth_one(n_pix, rng)
    u = (x[None, :] - truth[:, 1:2]) / (np.sqrt(2.0) * truth[:, 2:3])
    a = truth[:, 3:4] / (np.sqrt(2.0) * truth[:, 2:3])
    K, _ = R.w_dev(u, np.broadcast_to(a, u.shape))
    Y = truth[:, 0:1] * K / (truth[:, 2:3] * np.sqrt(2.0 * np.pi))
    return dict(Y=Y, x=x, x_ref=0.0, w=None, live=None, free=[1, 1, 1, 1, 0, 0], theta0=None, truth=truth,
                n_comp=1, follow=[])

# The worst |theta - truth| / scale of the float64 emulation on every 13th sightline of `big_stack`
# from `start_one` (tests/test_voigtfit_reference_cpu.py measures 9.88e-11 and holds it to this); the
# device is held to ten times it on every sightline.
BIG_RECOVERY = 1.0e-10
