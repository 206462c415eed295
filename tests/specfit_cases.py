"""The inputs of tests/test_gpu_specfit.py's raw-call cases, shared with
tests/test_specfit_reference_cpu.py, which runs the float64 emulations of tests/specfit_ref.py on
every one of them: inside the bounds, converging where the GPU test demands convergence, and
reaching every path of the iteration.  Analytic data: the model itself in float64 NumPy.  A case
is a dict(Y [n_pix, C] (pixel first; the cube is its transpose), x [C], w [C] or None, x_ref,
theta0 [n_pix, P], free [P] or None, live [n_pix] uint8 or None, truth [n_pix, P] or None)."""
import numpy as np

from tests import specfit_ref as K

N_ITER = 40
LAM0, XTOL = 1e-3, 1e-10
N_PIX = [1, 63, 64, 65, 257]               # every tail of a wave, more than one workgroup
AXES = ["uniform", "descending", "nonuniform"]
WEIGHTS = [None, "chan", "zeros"]
CONFIGS = [(1, False), (1, True), (2, False), (2, True)]      # (n_comp, a free baseline)
BIG = (130, 65, 40)                         # the noise-free stack fitted from specfit_start


def free_flags(n_comp, bl):
    return np.array([1] * (3 * n_comp) + [int(bl)] * 2, dtype=np.uint8)


def chans(n_comp, bl):
    """The channel counts of the sized cases: P_free (an exactly determined fit), P_free + 1, 8,
    64 and 257."""
    pf = 3 * n_comp + 2 * int(bl)
    return sorted({pf, pf + 1, max(8, pf), 64, 257})


SIZED = [(nc, bl, c) for nc, bl in CONFIGS for c in chans(nc, bl)]


def axis(kind, n_chan, rng):
    if n_chan == 1:
        return np.array([0.7])
    x = np.linspace(-30.0, 30.0, n_chan)
    if kind == "descending":
        x = x[::-1].copy()
    elif kind == "nonuniform":
        x = np.cumsum(rng.uniform(0.5, 1.5, n_chan))
        x = (x - x.mean()) * (60.0 / (x[-1] - x[0]))
    return x


def truths(n_pix, n_comp, bl, rng):
    t = np.zeros((n_pix, 3 * n_comp + 2))
    t[:, 0], t[:, 1], t[:, 2] = rng.uniform(0.5, 2.0, n_pix), rng.uniform(-8, 8, n_pix), rng.uniform(3, 7, n_pix)
    if n_comp == 2:
        t[:, 3] = rng.uniform(0.3, 0.8, n_pix) * np.where(rng.uniform(size=n_pix) < 0.3, -1, 1)
        t[:, 4], t[:, 5] = t[:, 1] + rng.uniform(14, 18, n_pix), rng.uniform(2, 4, n_pix)
    if bl:
        t[:, -2], t[:, -1] = rng.uniform(0.1, 0.3, n_pix), rng.uniform(0.002, 0.01, n_pix)
    return t


def off(truth, bl):
    """A start 20-25 % off in amplitude and width and one unit off in position."""
    t = np.array(truth, dtype=np.float64)
    t[..., 0:-2:3] *= 1.2
    t[..., 1:-2:3] += 1.0
    t[..., 2:-2:3] *= 1.25
    if bl:
        t[..., -2] *= 1.1
        t[..., -1] *= 0.9
    return t


def analytic(theta, x, x_ref):
    return K.model(theta, x, x_ref, np.float64)[0]


def weights(kind, n_chan, rng):
    if kind is None:
        return None
    w = rng.lognormal(0.0, 0.5, n_chan)
    if kind == "zeros" and n_chan >= 64:
        w[rng.choice(n_chan, n_chan // 8, replace=False)] = 0.0
    return w


def sized(n_comp, bl, n_chan, noise=None):
    """The sized case (n_comp, baseline free, n_chan): n_pix, the axis, the weights and the noise
    are taken in turn from N_PIX, AXES, WEIGHTS and (none, 0.02) by the case's index."""
    k = SIZED.index((n_comp, bl, n_chan))
    rng = np.random.default_rng(100 + k)
    n_pix = N_PIX[k % len(N_PIX)]
    x = axis(AXES[k % 3], n_chan, rng)
    x_ref = float(x[n_chan // 2])
    w = weights(WEIGHTS[(k // 2) % 3], n_chan, rng)
    truth = truths(n_pix, n_comp, bl, rng)
    Y = analytic(truth, x, x_ref)
    noise = (0.02 if k % 4 == 3 else 0.0) if noise is None else noise
    if noise:
        Y = Y + noise * rng.standard_normal(Y.shape)
    return dict(Y=Y, x=x, w=w, x_ref=x_ref, theta0=off(truth, bl), free=free_flags(n_comp, bl),
                live=None, truth=truth, noise=noise, n_comp=n_comp)


def must_converge(case):
    """The sized cases the GPU test holds to 1e-9 of the truth: noise-free, 64 channels or more."""
    return case["noise"] == 0.0 and case["x"].size >= 64


def bad_data(n_comp, bl=True):
    """65 pixels x 64 channels, 20 % of the channels NaN / inf at random; pixel 3 all NaN, pixel 7
    with one counted channel fewer than free parameters, pixel 11 masked, pixel 13 with exactly as
    many as free parameters; per-channel weights with zeros."""
    rng = np.random.default_rng(7 + n_comp)
    n_pix, n_chan = 65, 64
    x = axis("uniform", n_chan, rng)
    x_ref = float(x[32])
    w = weights("zeros", n_chan, rng)
    truth = truths(n_pix, n_comp, bl, rng)
    Y = analytic(truth, x, x_ref)
    bad = rng.uniform(size=Y.shape) < 0.2
    Y[bad] = np.where(rng.uniform(size=int(bad.sum())) < 0.5, np.nan, np.inf)
    Y[3] = np.nan
    pf = int(free_flags(n_comp, bl).sum())
    good = np.nonzero(w > 0)[0]
    for p, keep in ((7, pf - 1), (13, pf)):
        row = np.full(n_chan, np.nan)
        sel = good[np.linspace(8, good.size - 9, keep).astype(int)]
        row[sel] = analytic(truth[p:p + 1], x, x_ref)[0][sel]
        Y[p] = row
    live = np.ones(n_pix, dtype=np.uint8)
    live[11] = 0
    return dict(Y=Y, x=x, w=w, x_ref=x_ref, theta0=off(truth, bl), free=free_flags(n_comp, bl),
                live=live, truth=truth, noise=0.0, n_comp=n_comp, degenerate=[3, 7, 11])


def degenerate_starts():
    """Five pixels of one component, baseline held: starts with s = 0, s < 0, a NaN amplitude and
    a NaN baseline -- status 3, nothing written -- and a sound one, fitted as if alone."""
    rng = np.random.default_rng(21)
    x = axis("uniform", 64, rng)
    x_ref = float(x[32])
    truth = truths(5, 1, False, rng)
    Y = analytic(truth, x, x_ref)
    th0 = off(truth, False)
    th0[0, 2], th0[1, 2], th0[2, 0], th0[3, 3] = 0.0, -2.0, np.nan, np.nan
    return dict(Y=Y, x=x, w=None, x_ref=x_ref, theta0=th0, free=free_flags(1, False), live=None,
                truth=truth, noise=0.0, n_comp=1, degenerate=[0, 1, 2, 3])


def narrow():
    """A line narrower than a channel (s = 0.2 spacings) on 64 pixels, started at two spacings:
    one channel sees the line.  Judged by the trace alone."""
    rng = np.random.default_rng(33)
    x = axis("uniform", 32, rng)
    sp = x[1] - x[0]
    x_ref = float(x[16])
    truth = truths(64, 1, False, rng)
    truth[:, 2] = 0.2 * sp
    truth[:, 1] = x[rng.integers(8, 24, 64)] + rng.uniform(-0.3, 0.3, 64) * sp
    th0 = truth.copy()
    th0[:, 2] = 2 * sp
    return dict(Y=analytic(truth, x, x_ref), x=x, w=None, x_ref=x_ref, theta0=th0,
                free=free_flags(1, False), live=None, truth=truth, noise=0.0, n_comp=1)


def flat(bl):
    """Flat spectra: pixel 0 all zero, pixel 1 constant 0.5, pixel 2 a pure slope, pixel 3 a sound
    line, pixel 4 a sound line whose start lies so far off the axis that its envelope is an exact 0
    in every channel: the line's columns of N vanish, every pivot fails, the fit stalls (status 2).
    With the baseline held the Gaussian of pixels 0-2 must stretch or vanish."""
    rng = np.random.default_rng(44)
    x = axis("uniform", 48, rng)
    x_ref = float(x[24])
    truth = truths(5, 1, bl, rng)
    Y = analytic(truth, x, x_ref)
    Y[0], Y[1], Y[2] = 0.0, 0.5, 0.01 * (x - x_ref)
    th0 = off(truth, bl)
    th0[4, 1] = 1e4
    return dict(Y=Y, x=x, w=None, x_ref=x_ref, theta0=th0, free=free_flags(1, bl),
                live=None, truth=None, noise=0.0, n_comp=1)


def held():
    """One component with x0 and b1 held at their start, the rest free: a mixed pattern (the
    general kernel with identity rows)."""
    rng = np.random.default_rng(55)
    x = axis("nonuniform", 64, rng)
    x_ref = float(x[32])
    truth = truths(63, 1, True, rng)
    th0 = off(truth, True)
    th0[:, 1], th0[:, 4] = truth[:, 1], truth[:, 4]
    return dict(Y=analytic(truth, x, x_ref), x=x, w=weights("chan", 64, rng), x_ref=x_ref,
                theta0=th0, free=np.array([1, 0, 1, 1, 0], dtype=np.uint8), live=None, truth=truth,
                noise=0.0, n_comp=1)


def big():
    """130 x 65 noise-free sightlines of 40 channels, one component, baseline held: fitted from
    the moments' start to 1e-9 of the truth on EVERY pixel."""
    rng = np.random.default_rng(66)
    n_pix = BIG[0] * BIG[1]
    x = axis("uniform", BIG[2], rng)
    x_ref = float(x[BIG[2] // 2])
    truth = truths(n_pix, 1, False, rng)
    truth[:, 2] = rng.uniform(3, 6, n_pix)
    return dict(Y=analytic(truth, x, x_ref), x=x, w=None, x_ref=x_ref, theta0=None,
                free=free_flags(1, False), live=None, truth=truth, noise=0.0, n_comp=1)


def channel_widths(x):
    dx = np.zeros_like(x)
    if x.size > 1:
        dx[1:-1] = 0.5 * np.abs(x[2:] - x[:-2])
        dx[0], dx[-1] = abs(x[1] - x[0]), abs(x[-1] - x[-2])
    return dx


def start_from_moments(Y, x, x_ref):
    """`rajepy_amd.spectra.specfit_start` in NumPy on the float64 emulation of the moments."""
    n = Y.shape[0]
    dx = channel_widths(x)
    th = np.zeros((n, 5))
    for p in range(n):
        m = K.moments(Y[p], x, dx, x_ref, 0.0, True, np.float64)
        if m["ipeak"] < 0:
            th[p, :3] = np.nan
            continue
        i = m["ipeak"]
        lo, hi = max(i - 1, 0), min(i + 1, x.size - 1)
        sp = abs(x[hi] - x[lo]) / (hi - lo) if hi > lo else 1.0
        s = m["m2"] if np.isfinite(m["m2"]) and m["m2"] > 0 else 2 * sp
        th[p, :3] = m["peak"], x[i], s
    return th


def scaled_error(theta, truth):
    sc = np.stack([K.scales(t) for t in np.atleast_2d(truth)]).astype(np.float64)
    return float(np.max(np.abs(np.atleast_2d(theta) - np.atleast_2d(truth)) / sc))


# ---- moments -------------------------------------------------------------------------------------
MOMENT_SIZES = [(1, 1), (63, 2), (64, 8), (65, 64), (257, 257)]     # (n_pix, n_chan)


def moment_case(n_pix, n_chan):
    """Emission lines with noise on the axis AXES[k], 10 % NaN / inf channels, an all-NaN pixel,
    a masked pixel, a clip of 0.05 (0 for the two smallest)."""
    k = MOMENT_SIZES.index((n_pix, n_chan))
    rng = np.random.default_rng(200 + k)
    x = axis(AXES[k % 3], n_chan, rng)
    x_ref = float(x[n_chan // 2])
    dx = channel_widths(x) if n_chan > 1 else np.array([1.5])
    truth = truths(n_pix, 1, False, rng)
    Y = analytic(truth, x, x_ref) + 0.02 * rng.standard_normal((n_pix, n_chan))
    if n_chan >= 8:
        bad = rng.uniform(size=Y.shape) < 0.1
        Y[bad] = np.where(rng.uniform(size=int(bad.sum())) < 0.5, np.nan, -np.inf)
    live = np.ones(n_pix, dtype=np.uint8)
    if n_pix > 20:
        Y[5] = np.nan
        live[9] = 0
    return dict(Y=Y, x=x, dx=dx, x_ref=x_ref, clip=0.05 if n_chan >= 8 else 0.0, live=live)


def moment_special():
    """Seven hand-made pixels of 6 channels, dx = 1, x = 0 .. 5, x_ref = 2, clip = 0.5:
    0 a tie of the peak (channels 1 and 4); 1 |y| exactly at the clip (counted) and just below
    (not); 2 y = (1, -1): m0 an exact 0; 3 nothing above the clip; 4 emission and absorption mixed
    with s2 / m0 < 0; 5 all NaN; 6 a masked pixel."""
    x = np.arange(6.0)
    Y = np.zeros((7, 6))
    Y[0] = [0.6, 2.0, 1.0, 0.7, 2.0, 0.6]
    Y[1] = [0.5, np.nextafter(0.5, 0), -0.5, 3.0, 0.1, 0.0]
    Y[2] = [1.0, -1.0, 0.0, 0.0, 0.2, np.nan]
    Y[3] = [0.4, -0.4, 0.1, 0.0, 0.3, 0.2]
    Y[4] = [-1.0, 0.0, 3.0, 0.0, 0.0, -1.0]
    Y[5] = np.nan
    Y[6] = [1.0, 2.0, 3.0, 2.0, 1.0, 0.5]
    live = np.ones(7, dtype=np.uint8)
    live[6] = 0
    return dict(Y=Y, x=x, dx=np.ones(6), x_ref=2.0, clip=0.5, live=live)
