"""The inputs of the rjp_mtmfs (K19) cases, shared by tests/test_gpu_mtmfs.py (the device, judged by
mtmfs_ref.follow) and tests/test_mtmfs_reference_cpu.py (a float64 emulation of the device's chains on
the same inputs, inside the bounds; and the non-vacuity of every case).  Each case is built once from
its seed and never changed.

A case: planes R0 [M, n_t, nx, nz] (point sources with Taylor spectra seen through the spectral beams,
plus a smooth random field and noise), beams B [n_psf, 2 n_t - 1, px, pz] (sinc-like, B_0(centre) = 1,
B_q scaled by the band's moments), Hinv [M, n_t, n_t], a mask or None, thresholds [M], gain, n_iter and
`live` [M]: the maps that hold anything to clean (an all-NaN map does not)."""
import numpy as np

from tests import mtmfs_ref as K

#        name            nx   nz  n_t M n_psf window     n_iter gain  mask   special
CASES = [
    ("1x1",              1,   1,  2, 1, 1, None,          3, 0.1, False, None),
    ("5x3 nt3",          5,   3,  3, 2, 2, None,         20, 0.1, True,  None),
    ("5x3 nt1",          5,   3,  1, 1, 1, None,         20, 0.1, False, None),
    ("32x32 one tile",  32,  32,  2, 1, 1, (9, 9),       40, 0.1, False, None),
    ("31x33 odd npix",  31,  33,  4, 3, 1, None,         30, 0.1, False, "nan"),
    ("31x33 nt3",       31,  33,  3, 2, 2, (9, 9),       25, 0.1, True,  None),
    ("67x131 full",     67, 131,  2, 2, 2, None,        200, 0.1, False, "stop"),
    ("67x131 gain 1",   67, 131,  3, 1, 1, (9, 9),       12, 1.0, False, None),
    ("67x131 nt1",      67, 131,  1, 3, 3, (31, 31),     37, 0.1, True,  None),
    ("130x65 nt4",     130,  65,  4, 2, 1, (41, 25),     37, 0.1, True,  None),
]
NAMES = [c[0] for c in CASES]
_BUILT = {}


def box(nx, nz):
    mask = np.zeros((nx, nz), dtype=bool)
    mask[nx // 5:nx - nx // 6, nz // 4:nz] = True
    return mask


def first_peak(R0, hinv, mask):
    """max |a_0| over the candidates of the planes on entry (float64), 0 when there is none."""
    ok = K._cands(R0, mask)
    with np.errstate(invalid="ignore"):
        a0 = np.abs(K.solve(hinv[0], R0, dtype=np.float64))
    return float(a0[ok].max()) if ok.any() else 0.0


def build(name):
    if name in _BUILT:
        return _BUILT[name]
    i = NAMES.index(name)
    _, nx, nz, n_t, M, n_psf, window, n_iter, gain, masked, special = CASES[i]
    rng = np.random.default_rng(19000 + i)
    px, pz = (2 * nx - 1, 2 * nz - 1) if window is None else window
    sets = [K.spectral_beams(rng, n_t, px, pz) for _ in range(n_psf)]
    B = np.stack([s[0] for s in sets])
    hinv = np.stack([sets[m if n_psf > 1 else 0][2] for m in range(M)])
    mask = box(nx, nz) if masked else None
    R0 = np.empty((M, n_t, nx, nz))
    for m in range(M):
        src = None
        if nx * nz > 2048:
            # strong sources in the first, a middle and the last tile, then random ones
            def spec(i0):
                return [i0] + [i0 * float(rng.uniform(-1.0, 1.0)) for _ in range(n_t - 1)]
            src = [(nx - 2, nz - 3, spec(1.0)), (nx // 2, nz // 2, spec(-0.9)), (nx // 5 + 1, nz // 4 + 2, spec(0.8)),
                   (int(rng.integers(nx)), int(rng.integers(nz)), spec(0.5))]
        R0[m] = K.taylor_planes(rng, nx, nz, B[m if n_psf > 1 else 0], n_t, sources=src)
    live = np.ones(M, dtype=bool)
    if special == "nan":
        # map 0: a NaN in ONE plane at the strongest pixel's neighbour and an infinity elsewhere; map 1:
        # NaN everywhere, beside live maps; map 2 untouched
        p = int(np.argmax(np.abs(R0[0, 0])))
        R0[0, 1].ravel()[min(p + 1, nx * nz - 1)] = np.nan
        R0[0, n_t - 1, nx // 2, nz // 2] = np.inf
        R0[1] = np.nan
        live[1] = False
    # an exact tie of two untouched pixels: pixel 0's values copied to the last pixel, plane by plane
    if nx * nz > 1 and special != "nan":
        R0[M - 1, :, nx - 1, nz - 1] = R0[M - 1, :, 0, 0]
    top = np.array([first_peak(R0[m], hinv[m], mask) for m in range(M)])
    thresh = np.zeros(M)
    if special == "stop":
        thresh[0] = 0.3 * top[0]              # map 0 stops early while map 1 runs on
    for a in (R0, B, hinv, thresh):
        a.setflags(write=False)
    _BUILT[name] = dict(name=name, R0=R0, B=B, hinv=hinv, mask=mask, thresh=thresh, gain=gain, n_iter=n_iter,
                        live=live, n_t=n_t, top=top)
    return _BUILT[name]
