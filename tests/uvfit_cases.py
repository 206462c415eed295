"""The inputs of tests/test_gpu_uvfit.py's raw-call cases, shared with
tests/test_uvfit_reference_cpu.py, which runs the float64 emulation of tests/uvfit_ref.py on every
one of them: inside the bounds, and converging where the GPU test demands convergence.  Analytic
data: the model itself in float64 NumPy at random (u, v) points of at most 0.25 cycles per cell."""
import numpy as np

from tests import uvfit_ref as K

N_VIS = [1, 2, 3, 5, 6, 255, 257, 1024, 1025, 2049, 262145]
N_VIS_TWO = [5, 6, 255, 257, 1025, 2049, 262145]      # with two components
SU = np.array([-1.0, 0.7, -1.3])                       # a map's own scales, signs included
SV = np.array([1.0, -0.8, 1.1])
# (F, x, z, sxx, sxz, szz): elongated and rotated, a negative flux, a sub-cell offset
ONE = np.array([[1.3, 2.3, -1.8, 6.0, 1.5, 3.0], [-0.7, -1.45, 2.35, 2.0, -0.9, 4.5],
                [2.5, 0.05, 0.49, 3.0, 0.0, 3.0]])
TWO = np.array([[1.3, 2.3, -1.8, 6.0, 1.5, 3.0, 0.4, -5.1, 4.2, 2.0, -0.5, 1.0],
                [0.9, -3.1, 1.2, 2.5, 0.4, 5.0, 0.6, 4.4, -3.7, 1.5, 0.3, 1.2],
                [2.5, 0.05, 0.49, 3.0, 0.0, 3.0, -0.5, 6.2, 5.3, 1.0, 0.2, 2.0]])
POINT_GAUSS = np.array([0.8, -4.2, 3.1, 0.0, 0.0, 0.0, 1.3, 2.3, -1.8, 6.0, 1.5, 3.0])
FREE_POINT_GAUSS = np.array([1, 1, 1, 0, 0, 0] + [1] * 6, dtype=np.uint8)
FREE_HELD = np.array([1, 0, 0, 1, 1, 1], dtype=np.uint8)     # a held position
N_ITER = 40
LAM0, XTOL = 1e-3, 1e-10


def off(truth):
    """A start 30-40 % off in flux and size and half a cell off in position."""
    t = np.array(truth, dtype=np.float64)
    t[..., 0::6] *= 1.3
    t[..., 1::6] += 0.5
    t[..., 2::6] -= 0.4
    t[..., 3::6] *= 1.4
    t[..., 5::6] *= 0.7
    return t


def analytic(theta, a, b):
    M = K.model(theta, a, b, np.float64, with_jac=False)[0]
    return M[0] + 1j * M[1]


def sized(n_vis, n_comp, noise=0.0):
    """The case of `n_vis` visibilities: 1 + n_vis % 3 maps with their own scales, weights none /
    shared / per map in turn -> dict(V [M, K], u, v, su, sv, w, theta0 [M, P], truth [M, P])."""
    M = 1 + n_vis % 3
    if n_vis > 100000:
        M = 1
    rng = np.random.default_rng(1000 * n_comp + n_vis % 997)
    u, v = rng.uniform(-0.19, 0.19, n_vis), rng.uniform(-0.19, 0.19, n_vis)
    truth = (ONE if n_comp == 1 else TWO)[:M]
    su, sv = SU[:M], SV[:M]
    V = np.stack([analytic(truth[m], su[m] * u, sv[m] * v) for m in range(M)])
    if noise:
        V = V + noise * (rng.standard_normal(V.shape) + 1j * rng.standard_normal(V.shape))
    kind = N_VIS.index(n_vis) % 3
    w = None if kind == 0 else rng.lognormal(0.0, 0.5, n_vis if kind == 1 else (M, n_vis))
    return dict(V=V, u=u, v=v, su=su, sv=sv, w=w, theta0=off(truth), truth=truth, free=None)


def flagged(n_comp=1, n_vis=1500, seed=77):
    """20 % of the visibilities flagged, every kind in turn (NaN / inf in Re V, Im V, u, v, w; w = 0;
    w < 0), per-map weights, and an all-flagged map (NaN weights) between two live ones."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-0.19, 0.19, n_vis), rng.uniform(-0.19, 0.19, n_vis)
    truth = (ONE if n_comp == 1 else TWO)[:3]
    V = np.stack([analytic(truth[m], SU[m] * u, SV[m] * v) for m in range(3)])
    w = rng.lognormal(0.0, 0.5, (3, n_vis))
    bad = rng.choice(n_vis, n_vis // 5, replace=False)
    for i, k in enumerate(bad):
        kind = i % 9
        if kind == 0:
            V[:, k] = complex(np.nan, 1.0)
        elif kind == 1:
            V[:, k] = complex(1.0, np.inf)
        elif kind == 2:
            u[k] = np.nan
        elif kind == 3:
            v[k] = -np.inf
        elif kind == 4:
            w[:, k] = np.nan
        elif kind == 5:
            w[:, k] = np.inf
        elif kind == 6:
            w[:, k] = 0.0
        elif kind == 7:
            w[:, k] = -1.0
        else:
            V[0, k] = complex(np.nan, np.nan)          # (this map alone)
    w[1, :] = np.nan
    return dict(V=V, u=u, v=v, su=SU, sv=SV, w=w, theta0=off(truth), truth=truth, free=None)


def fixed(which, n_vis=700, seed=5):
    """"point+gauss": two components, the first a point whose sizes are held at 0; "held": one
    component whose position is held at its (true) start."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-0.19, 0.19, n_vis), rng.uniform(-0.19, 0.19, n_vis)
    if which == "point+gauss":
        truth, free = POINT_GAUSS[None], FREE_POINT_GAUSS
        th0 = off(truth)
    else:
        truth, free = ONE[:1], FREE_HELD
        th0 = off(truth)
        th0[:, 1:3] = truth[:, 1:3]
    V = analytic(truth[0], SU[0] * u, SV[0] * v)[None]
    return dict(V=V, u=u, v=v, su=SU[:1], sv=SV[:1], w=None, theta0=th0, truth=truth, free=free)


def moving(n_vis=800, seed=8):
    """Two components that move linearly over 5 epochs, seen in 2 channels (scales 1 and 0.8): one
    stack of 10 maps, epoch-major; a map's parameters are in ITS cells.  The velocities per epoch
    are (0.3, -0.2) and (-0.5, 0.45) cells."""
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-0.24, 0.24, n_vis), rng.uniform(-0.24, 0.24, n_vis)
    truth = np.zeros((5, 2, 12))
    for e in range(5):
        truth[e, :] = [1.0, 0.3 * e, -0.2 * e, 0.5, 0.1, 0.4, 0.6, 5.0 - 0.5 * e, 4.0 + 0.45 * e, 2.0, 0.3, 1.5]
    truth = truth.reshape(10, 12)
    su = np.tile([1.0, 0.8], 5)
    V = np.stack([analytic(truth[m], su[m] * u, su[m] * v) for m in range(10)])
    return dict(V=V, u=u, v=v, su=su, sv=su, w=None, free=None, theta0=off(truth), truth=truth)


def stack():
    """Four maps side by side: one at its fixed point (a point source of 1.5 at the phase centre
    against V = 1.5: phase 0, envelope 1, chi^2 an exact 0), one that starts outside the PSD cone,
    one that is fitted, one that starts from a NaN."""
    base = sized(1025, 1)
    Kn = base["u"].size
    V = np.stack([np.full(Kn, 1.5 + 0j), base["V"][0], base["V"][0], base["V"][0]])
    th_good = base["theta0"][0]
    outside = th_good.copy()
    outside[3:] = [1.0, 2.0, 1.0]                                      # sxx szz < sxz^2
    nan = th_good.copy()
    nan[2] = np.nan
    th0 = np.stack([[1.5, 0, 0, 0, 0, 0], outside, th_good, nan])
    return dict(base, V=V, su=np.full(4, SU[0]), sv=np.full(4, SV[0]), theta0=th0, w=None,
                truth=np.stack([th0[0], base["truth"][0], base["truth"][0], base["truth"][0]]))


def per_map(case, m):
    """Map m of a case as tests/uvfit_ref.py takes it: ((V, a, b, w) of the counting visibilities,
    n_vis, theta0, free); a = su u and b = sv v are the float64 products the device forms (NumPy's
    are the same IEEE products)."""
    u, v = case["u"], case["v"]
    with np.errstate(invalid="ignore"):
        a, b = case["su"][m] * u, case["sv"][m] * v
    w = case["w"]
    if w is not None and np.ndim(w) == 2:
        w = w[m]
    return K.counting(case["V"][m], a, b, w, u, v), u.size, case["theta0"][m], case["free"]
