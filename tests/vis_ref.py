"""Reference for rjp_vis (K10, vis.hip): the direct Fourier sum in NumPy long double, and the bound
the device is held to -- derived here term by term, not measured on any device.

    V[k] = sum_{ix, iz} I[ix, iz] exp(-2 pi i (a[k] (ix - (nx-1)/2) + b[k] (iz - (nz-1)/2)))

`a`, `b` are float64 cycles per cell AS THE DEVICE FORMS THEM: one float64 product su * u (IEEE, so
`su * u` in NumPy is the same number).  The reference takes them as exact, forms every phase in long
double (53 + 8 bits: exact), reduces it with rint and evaluates long-double cos / sin; a NaN pixel is
0 (nansum).  Its own error is a few 2^-64 per term: 1e-19 (nx + nz), nothing beside the bound.

THE BOUND, per visibility, on |got - ref| of the real and the imaginary part alike, relative to
S = sum |I| (the finite pixels), u = 2^-53.  The device evaluates Ez[iz] = e^{-2 pi i fl(b jz)} and
Ex[ix] likewise with sincos_2pi, then W[ix] = sum_iz I Ez (a chain of FMAs) and V = sum_ix Ex W
(FMAs and adds, at most nx + 20 deep whatever the tiling):
  1. rounding of the double product a j (and b j): the phase moves by 2 pi |a j| u radians at most,
     |j| <= (n - 1) / 2:                     2 pi (|a| (nx - 1) / 2 + |b| (nz - 1) / 2) u
  2. sincos_2pi, once per factor: truncation as its header states it (sine < 2e-14, cosine < 1e-15:
     the phasor is off by < 2.01e-14 in modulus) plus the rounding of its reduction (the multiple of
     a quarter turn comes off exactly, by FMA; the product with 2 pi costs 1.5 u (pi / 4)) and of its
     two Horner chains (< 3 u): < 6 u          2 (2.01e-14 + 6 u)
  3. the products I Ez and Ex W are formed inside FMAs: their rounding is the accumulation's
  4. accumulation: a sum at depth d is off by <= d u / (1 - d u) sum |terms|.  A component of W[ix]
     is a chain of nz FMAs on I cos or I sin; through V = sum_ix Ex W its error reaches a component
     of V weighted by |cos_x cos_z| + |sin_x sin_z| <= 1: nz u S.  A component of V sums
     |cos Wr| + |sin Wi| <= |W[ix]| <= sum_iz |I| at depth <= nx + 20: (nx + 20) u S.
                                             (nx + nz + 24) u  (/ (1 - (nx + nz + 24) u))
Second-order products of these terms are below 1e-26.  0.4-0.9e-13 for |a|, |b| <= 0.5 on the shapes
of the tests, 6e-13 at 8 cycles per cell on 67 x 131: term 1 is the baseline's price.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SINCOS_TRUNC = 2.01e-14          # |(2e-14, 1e-15)|: the header of sincos_2pi (rjp_device.h)
SINCOS_ROUND = 6.0 * U
ACC_EXTRA = 24                   # the depth of V's sum beyond nx (<= 20), and slack


def _check_longdouble():
    assert np.finfo(LD).eps < 2.0 ** -60, "this reference needs an 80-bit (or wider) long double"


def _phasors(c, n):
    """e^{-2 pi i c j}, j = index - (n - 1) / 2 -> clongdouble [len(c), n]."""
    j = np.arange(n, dtype=LD) - LD(n - 1) / LD(2)
    two_pi = LD(8) * np.arctan(LD(1))
    with np.errstate(invalid="ignore"):                # (a non-finite point: NaN, on purpose)
        ph = np.asarray(c, dtype=np.float64).astype(LD)[:, None] * j[None, :]
        ph = ph - np.rint(ph)
        return np.cos(two_pi * ph) - 1j * np.sin(two_pi * ph)


def vis_ref(I, a, b):
    """-> complex clongdouble [K]: the sum above for one map I[nx, nz] (float64, NaN = no pixel) at
    the K points (a[k], b[k]) in cycles per cell.  A non-finite a[k] or b[k] gives NaN."""
    _check_longdouble()
    I = np.asarray(I, dtype=np.float64)
    nx, nz = I.shape
    Il = np.where(np.isnan(I), 0.0, I).astype(LD).astype(np.clongdouble)
    ex, ez = _phasors(a, nx), _phasors(b, nz)
    with np.errstate(invalid="ignore"):
        W = ez @ Il.T                                  # [K, nx]
        return (W * ex).sum(axis=1)


def sum_abs(I):
    I = np.asarray(I, dtype=np.float64)
    return float(np.abs(np.where(np.isnan(I), 0.0, I)).astype(LD).sum())


def bound(a, b, nx, nz):
    """The derived bound on |got - ref| / sum |I| per visibility (see the module's head)."""
    a, b = np.abs(np.asarray(a, dtype=np.float64)), np.abs(np.asarray(b, dtype=np.float64))
    d = (nx + nz + ACC_EXTRA) * U
    return (2.0 * np.pi * (a * (nx - 1) / 2.0 + b * (nz - 1) / 2.0) * U +
            2.0 * (SINCOS_TRUNC + SINCOS_ROUND) + d / (1.0 - d))


def worst_ratio(got, ref, S, bnd):
    """max over the visibilities of max(|Re err|, |Im err|) / (bound S); got: complex128 [K]."""
    ref = np.asarray(ref)
    er = np.abs((np.asarray(got).real.astype(LD) - ref.real).astype(np.float64))
    ei = np.abs((np.asarray(got).imag.astype(LD) - ref.imag).astype(np.float64))
    return float(np.max(np.maximum(er, ei) / (bnd * S)))


# ---- a float64 emulation of the factorised sum, and three planted mistakes ----------------------
def vis_emulated(I, a, b, centre_shift=0.0, sign=-1.0, phasor_dtype=np.float64):
    """The device's arithmetic in NumPy float64: phases as one double product, rint reduction,
    W = sum_iz I Ez as a sequential chain, V = sum_ix Ex W.  `centre_shift` = 0.5 uses n / 2 as the
    centre, `sign` = +1 the opposite phase convention, `phasor_dtype` = float32 rounds the phasors:
    the planted mistakes the bound must reject."""
    I = np.asarray(I, dtype=np.float64)
    nx, nz = I.shape
    I0 = np.where(np.isnan(I), 0.0, I)
    jx = np.arange(nx) - ((nx - 1) / 2.0 + centre_shift)
    jz = np.arange(nz) - ((nz - 1) / 2.0 + centre_shift)
    out = np.zeros(len(a), dtype=np.complex128)
    for k in range(len(a)):
        px = a[k] * jx
        px = px - np.rint(px)
        pz = b[k] * jz
        pz = pz - np.rint(pz)
        cast = lambda t: t.astype(phasor_dtype).astype(np.float64)
        exr, exi = cast(np.cos(2 * np.pi * px)), cast(sign * np.sin(2 * np.pi * px))
        ezr, ezi = cast(np.cos(2 * np.pi * pz)), cast(sign * np.sin(2 * np.pi * pz))
        wr, wi = np.zeros(nx), np.zeros(nx)
        for z in range(nz):
            wr += I0[:, z] * ezr[z]
            wi += I0[:, z] * ezi[z]
        vr = vi = 0.0
        for x in range(nx):
            vr += wr[x] * exr[x] - wi[x] * exi[x]
            vi += wr[x] * exi[x] + wi[x] * exr[x]
        out[k] = complex(vr, vi)
    return out


# ---- the cases of tests/test_gpu_vis.py -----------------------------------------------------------
SHAPES = [(1, 1), (1, 7), (5, 3), (64, 64), (67, 131), (130, 65)]
N_VIS = [1, 63, 64, 65, 257]


def random_map(rng, nx, nz, nan_share=0.2):
    """Log-normal intensities over four decades, `nan_share` of the pixels NaN."""
    I = rng.lognormal(0.0, 2.0, (nx, nz))
    I[rng.random((nx, nz)) < nan_share] = np.nan
    return I


def random_points(rng, n, amax):
    """(a, b) uniform in [-amax, amax] cycles per cell, the zero spacing first."""
    a, b = rng.uniform(-amax, amax, n), rng.uniform(-amax, amax, n)
    a[0] = b[0] = 0.0
    return a, b
