"""Reference for rjp_vis_adjoint (K11, vis_adjoint.hip): the transpose of K10's direct Fourier sum
in NumPy long double, the host restatement of the kernel's tiling rule, and the bound the device is
held to -- derived here term by term from the kernel's arithmetic, not measured on any device.

    D[ix, iz] = sum_k w[k] Re( V[k] exp(+2 pi i (a[k] (ix - (nx-1)/2) + b[k] (iz - (nz-1)/2))) )

`a`, `b` are float64 cycles per cell AS THE DEVICE FORMS THEM (one float64 product su * u, as in
tests/vis_ref.py).  Visibility k is FLAGGED -- adds nothing -- when any of Re V, Im V, w, a, b is
non-finite (su, sv are finite, so a, b are non-finite exactly when u, v are).  The reference takes
a, b, w, V as exact, forms every phase in long double (53 + 8 bits: exact), reduces it with rint,
evaluates long-double cos / sin and sums in long double: its own error is a few 2^-64 per term.

THE BOUND, per pixel, on |got - ref| relative to S = sum_k |w_k| |V_k| over the unflagged
visibilities, u = 2^-53.  Per visibility the kernel evaluates (cx, sx) = sincos_2pi(fl(a jx)),
(cz, sz) = sincos_2pi(fl(b jz)), pr = fl(w Re V), pi = fl(w Im V), P = (fma(-pi, sx, fl(pr cx)),
fma(pi, cx, fl(pr sx))), and adds to the pixel acc = fma(P_im, -sz, fma(P_re, cz, acc)); the
visibilities of one k-split in index order, then the splits' partial sums in split order.
  1. rounding of the double products a jx, b jz: visibility k's phase moves by
     t_k = 2 pi (|a_k| (nx - 1) / 2 + |b_k| (nz - 1) / 2) u radians at most, its term by
     |w_k V_k| t_k:                          sum_k |w_k V_k| t_k / S   (<= max_k t_k)
  2. sincos_2pi, once per factor (the constants of tests/vis_ref.py: truncation 2.01e-14 in
     modulus, reduction and Horner chains 6 u):                          2 (2.01e-14 + 6 u)
  3. the complex product w V Ex: pr, pi carry one rounding each (u (|pr| + |pi|) into either
     component of P), a component of P two more (the product, and the FMA's result:
     <= 2 u (|pr| + |pi|)); |pr| + |pi| <= sqrt 2 |w V|, and a pixel weighs the two components by
     |cz| + |sz| <= sqrt 2:                  3 sqrt 2 sqrt 2 u =              6 u
  4. accumulation: the chain of 2 FMAs per visibility is at most 2 n_k deep (n_k: the longest
     k-split, <= n_vis), the combine adds n_split - 1 more; a sum at depth d is off by
     <= d u / (1 - d u) sum |terms|, and |P_re cz| + |P_im sz| <= |P| = |w V| (1 + 3 u):
                                             (2 n_k + n_split + 4) u  (/ (1 - ...))
Second-order products of these terms are below 1e-26.  About 0.5e-13 at |a|, |b| <= 0.5 and a few
hundred visibilities, 6e-13 at 8 cycles per cell on 67 x 131: term 1 is the baseline's price."""
import numpy as np

from tests import vis_ref as R

LD = np.longdouble
U = R.U
PRODUCT_ROUND = 6.0 * U          # term 3
ACC_EXTRA = 4                    # term 4's slack beyond 2 n_k + n_split

# ---- the tiling rule of vis_adjoint.hip, restated ---------------------------------------------------
TILE_COLS, CHUNK, MIN_SPLIT, FILL = 128, 16, 64, 256


def tiling(n_maps, nx, nz, n_vis):
    """-> dict(row_tiles, col_tiles, k_splits, k_per_split, workgroups): tiles of 128 rows (64 for
    nx <= 64) x 128 columns; fewer than 256 of them: the visibilities are split
    min(ceil(256 / tiles), ceil(n_vis / 64)) ways into ranges of whole 16-chunks."""
    tr = 128 if nx > 64 else 64
    rt, ct = -(-nx // tr), -(-nz // TILE_COLS)
    tiles = n_maps * rt * ct
    ns = 1
    if tiles < FILL:
        ns = min(-(-FILL // tiles), -(-n_vis // MIN_SPLIT))
    kper = -(-(-(-n_vis // ns)) // CHUNK) * CHUNK
    ns = -(-n_vis // kper)
    return dict(row_tiles=rt, col_tiles=ct, k_splits=ns, k_per_split=kper, workgroups=tiles * ns)


def workspace_bytes(n_maps, nx, nz, n_vis):
    """rjp_vis_adjoint_workspace as host arithmetic: 0 for a bad argument, one partial image per
    (map, k-split), 16 bytes without a split."""
    if min(n_maps, nx, nz, n_vis) < 1:
        return 0
    ns = tiling(n_maps, nx, nz, n_vis)["k_splits"]
    return 16 if ns == 1 else n_maps * ns * nx * nz * 8


# ---- the reference ------------------------------------------------------------------------------------
def unflagged(V, a, b, w=None):
    """-> bool [K]: the visibilities that count."""
    V = np.asarray(V, dtype=np.complex128)
    ok = np.isfinite(V.real) & np.isfinite(V.imag) & np.isfinite(a) & np.isfinite(b)
    return ok if w is None else ok & np.isfinite(w)


def _clean(V, a, b, w):
    V = np.asarray(V, dtype=np.complex128).reshape(-1)
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    w = np.ones(V.size) if w is None else np.asarray(w, dtype=np.float64).reshape(-1)
    assert a.size == b.size == w.size == V.size
    ok = unflagged(V, a, b, w)
    z = lambda t: np.where(ok, t, 0.0)
    return z(V.real), z(V.imag), z(a), z(b), z(w), ok


def vis_adjoint_ref(V, a, b, nx, nz, w=None):
    """-> longdouble [nx, nz]: the sum above for one visibility set V[K] (complex128) at the points
    (a[k], b[k]) in cycles per cell with the weights w[k] (None: ones)."""
    R._check_longdouble()
    vr, vi, a, b, w, _ = _clean(V, a, b, w)
    ex, ez = np.conj(R._phasors(a, nx)), np.conj(R._phasors(b, nz))      # e^{+2 pi i c j}
    wl = w.astype(LD)
    pr, pi = wl * vr.astype(LD), wl * vi.astype(LD)
    Pre = pr[:, None] * ex.real - pi[:, None] * ex.imag                  # [K, nx]
    Pim = pr[:, None] * ex.imag + pi[:, None] * ex.real
    return Pre.T @ ez.real - Pim.T @ ez.imag


def sum_abs(V, a, b, w=None):
    """S = sum_k |w_k| |V_k| over the unflagged visibilities."""
    vr, vi, _, _, w, _ = _clean(V, a, b, w)
    return float((np.abs(w).astype(LD) * np.hypot(vr.astype(LD), vi.astype(LD))).sum())


def bound(V, a, b, nx, nz, w=None, k_splits=1, k_per_split=None):
    """The derived bound on |got - ref| / S per pixel (see the module's head)."""
    vr, vi, a, b, w, ok = _clean(V, a, b, w)
    amp = np.abs(w) * np.hypot(vr, vi)
    S = amp.sum()
    t = 2.0 * np.pi * (np.abs(a) * (nx - 1) / 2.0 + np.abs(b) * (nz - 1) / 2.0) * U
    t1 = float((amp * t).sum() / S) if S > 0 else 0.0
    nk = len(a) if k_per_split is None else min(len(a), k_per_split)
    d = (2 * nk + k_splits + ACC_EXTRA) * U
    return t1 + 2.0 * (R.SINCOS_TRUNC + R.SINCOS_ROUND) + PRODUCT_ROUND + d / (1.0 - d)


def worst_ratio(got, ref, S, bnd):
    """max over the pixels of |got - ref| / (bound S); got: float64 [nx, nz]."""
    err = np.abs((np.asarray(got, dtype=np.float64).astype(LD) - ref).astype(np.float64))
    return float(err.max() / (bnd * S))


# ---- a float64 emulation of the kernel's arithmetic, and planted mistakes ---------------------------
def vis_adjoint_emulated(V, a, b, nx, nz, w=None, k_per_split=None, centre_shift=0.0, sign=1.0,
                         phasor_dtype=np.float64, drop_weight=False):
    """The device's arithmetic in NumPy float64: phases as one double product, rint reduction, the
    complex product w V Ex, the pixel sums as a sequential chain over the visibilities of a k-split
    and the splits added in order.  `centre_shift` = 0.5 uses n / 2 as the centre, `sign` = -1 the
    opposite phase convention, `phasor_dtype` = float32 rounds the phasors, `drop_weight` leaves w
    out: the planted mistakes the bound must reject."""
    vr, vi, a, b, w, _ = _clean(V, a, b, w)
    if drop_weight:
        w = np.where(w != 0.0, 1.0, 0.0)
    K = len(a)
    kper = K if k_per_split is None else k_per_split
    jx = np.arange(nx) - ((nx - 1) / 2.0 + centre_shift)
    jz = np.arange(nz) - ((nz - 1) / 2.0 + centre_shift)
    cast = lambda t: t.astype(phasor_dtype).astype(np.float64)
    total = np.zeros((nx, nz))
    for k0 in range(0, K, kper):
        acc = np.zeros((nx, nz))
        for k in range(k0, min(K, k0 + kper)):
            px = a[k] * jx
            px = px - np.rint(px)
            pz = b[k] * jz
            pz = pz - np.rint(pz)
            cx, sx = cast(np.cos(2 * np.pi * px)), cast(sign * np.sin(2 * np.pi * px))
            cz, sz = cast(np.cos(2 * np.pi * pz)), cast(sign * np.sin(2 * np.pi * pz))
            pr, pi = w[k] * vr[k], w[k] * vi[k]
            Pre, Pim = pr * cx - pi * sx, pr * sx + pi * cx
            acc += Pre[:, None] * cz[None, :]
            acc += Pim[:, None] * -sz[None, :]
        total = acc if k0 == 0 else total + acc
    return total


# ---- the cases of tests/test_gpu_vis_adjoint.py -------------------------------------------------------
SHAPES = R.SHAPES                          # (1, 1), (1, 7), (5, 3), (64, 64), (67, 131), (130, 65)
N_VIS = R.N_VIS + [1000]                   # 1, 63, 64, 65, 257 and one long set


def random_vis(rng, n, flagged=0.2):
    """Complex visibilities over four decades of amplitude and weights over one, `flagged` of the
    set flagged through one of Re V, Im V, w (NaN or an infinity)."""
    V = rng.lognormal(0.0, 2.0, n) * np.exp(2j * np.pi * rng.random(n))
    w = rng.lognormal(0.0, 0.5, n)
    bad = np.flatnonzero(rng.random(n) < flagged)
    for i, k in enumerate(bad):
        which = i % 4
        if which == 0:
            V[k] = complex(np.nan, V[k].imag)
        elif which == 1:
            V[k] = complex(V[k].real, np.inf)
        elif which == 2:
            w[k] = np.nan
        else:
            w[k] = -np.inf
    return V, w
