"""Reference for rjp_vis_components (K18, vis_components.hip) and rjp_components_image: the direct sum
over a component list in NumPy long double, and the bound the device is held to -- derived here term
by term, not measured on any device.

    out[k] = in[k] + sign sum_s G[s, k] sum_{c < n, s_c = s} f_c exp(-2 pi i (a[k] jx_c + b[k] jz_c))
    jx_c = ix_c - (nx-1)/2,  jz_c = iz_c - (nz-1)/2,  p_c = ix_c nz + iz_c

`a`, `b` are float64 cycles per cell AS THE DEVICE FORMS THEM (one float64 product su * u), taken as
exact; every phase is formed in long double (exact), reduced with rint and evaluated by long-double
cos / sin; G and `in` are the float64 numbers the device reads.  A component adds nothing if its flux
is not finite, its pixel lies outside [0, nx nz) or its scale outside [0, n_s); the list is cut at
min(max(n, 0), stride).  The reference's own error is a few 2^-64 per term.

THE BOUND, per visibility, on |got - ref| of the real and the imaginary part alike, relative to
S[k] = sum_c |f_c| |G[s_c, k]| + |in[k]|, u = 2^-53.  The device's order (the head of
vis_components.hip): per scale, four slices of the list (slice w = the components c with
(c mod 256) / 64 = w) each summed in list order as P = sum f E, E = Ex Ez the product of two phasors
from sincos_2pi; T[w] += G P once per scale; out = in + (((T0 + T1) + T2) + T3).
  1. rounding of the double products a jx and b jz: the phase moves by 2 pi |a jx| u radians at most,
     the phasor by as much in modulus:     2 pi (|a| (nx - 1) / 2 + |b| (nz - 1) / 2) u
  2. sincos_2pi, once per factor: truncation as its header states it (|(2e-14, 1e-15)| = 2.01e-14)
     plus < 6 u of rounding (tests/vis_ref.py, term 2); the product E = Ex Ez = (fma(cx, cz, -(sx sz)),
     fma(sx, cz, cx sz)) rounds twice per part, < 2 u, and carries both factors' errors:
     2 (2.01e-14 + 6 u) + 2 u PER PART of E.  Through the product with G an error e in each part of
     P reaches a part of G P as (|G.re| + |G.im|) e <= sqrt(2) |G| e:
                                           sqrt(2) (2 (2.01e-14 + 6 u) + 2 u)
  3. accumulation of P: a chain of at most d = 64 ceil(n / 256) fmas on terms |f E.part| <= |f|,
     off by <= d u / (1 - d u) sum |f| per part, times sqrt(2) through G as in 2:
                                           sqrt(2) d u / (1 - d u)
  4. the product with G: T.re = fma(-G.im, P.im, fma(G.re, P.re, T.re)), a chain of 2 n_s fmas on
     terms with |G.re P.re| + |G.im P.im| <= |G| |P| <= |G| sum |f|:      2 n_s u
  5. the three adds of the slices and the add to `in`, each rounding a number <= S (1 + ...):  4 u
Second-order products of these are below 1e-26.  About 1e-13 for |a|, |b| <= 0.5 and 1000 components,
6e-13 at 8 cycles per cell on 67 x 131: term 1 is the baseline's price, as for K10.
"""
import numpy as np

from tests import vis_ref as VR

LD = np.longdouble
U = VR.U
SLICE, CHUNK = 64, 256                      # vis_components.hip: kVcC = 256 = 4 slices of 64
ROOT2 = float(np.sqrt(2.0))
PHASOR_PART = 2.0 * (VR.SINCOS_TRUNC + VR.SINCOS_ROUND) + 2.0 * U


# the refusals of check_vis_components / check_components_image (rjp_args.h), in the order made
MSG = {
    "null": "rjp_vis_components: NULL components, scales, baselines or output",
    "sizes": "rjp_vis_components: n_maps, comp_stride, n_s, nx, nz and n_vis must be positive",
    "sign": "rjp_vis_components: sign must be +1 or -1",
    "gvis": "rjp_vis_components: a NULL d_gvis (G = 1) needs n_s = 1",
    "scales": "rjp_vis_components: non-finite h_su / h_sv",
    "npix": "rjp_vis_components: nx * nz exceeds 2^31 - 1",
    "wgs": "rjp_vis_components: more than 2^31 - 1 workgroups",
    "img_null": "rjp_components_image: NULL components or output",
    "img_sizes": "rjp_components_image: n_maps, comp_stride, n_s, nx and nz must be positive",
    "img_npix": "rjp_components_image: nx * nz exceeds 2^31 - 1",
    "img_wgs": "rjp_components_image: more than 2^31 - 1 workgroups",
}


def workgroups(n_maps, n_vis):
    """vis_components.hip's grid: 64 visibilities of one map per workgroup."""
    return n_maps * -(-n_vis // SLICE)


def image_workgroups(n_maps, n_s, nx, nz):
    """components_image's grid: 256 pixels of one plane per workgroup."""
    return n_maps * n_s * -(-(nx * nz) // 256)


def clamp(n, stride):
    return min(max(int(n), 0), int(stride))


def valid(cpix, cflux, cscale, n, nx, nz, n_s):
    """The first `n` entries of one map's list that add something -> (pix, flux, scale, index)."""
    p = np.asarray(cpix[:n], dtype=np.int64)
    f = np.asarray(cflux[:n], dtype=np.float64)
    s = np.zeros(n, dtype=np.int64) if cscale is None else np.asarray(cscale[:n], dtype=np.int64)
    ok = np.isfinite(f) & (p >= 0) & (p < nx * nz) & (s >= 0) & (s < n_s)
    return p[ok], f[ok], s[ok], np.nonzero(ok)[0]


def _unit(c, j):
    """e^{-2 pi i c j} in long double: c float64 [K], j exact half-integers [n] -> [K, n]."""
    two_pi = LD(8) * np.arctan(LD(1))
    with np.errstate(invalid="ignore"):
        ph = np.asarray(c, dtype=np.float64).astype(LD)[:, None] * np.asarray(j, dtype=LD)[None, :]
        ph = ph - np.rint(ph)
        return np.cos(two_pi * ph) - 1j * np.sin(two_pi * ph)


def vis_components_ref(cpix, cflux, cscale, ncomp, nx, nz, a, b, n_s=1, G=None, vin=None, sign=1):
    """One map -> (out clongdouble [K], S float64 [K]).  cpix / cflux / cscale: the map's row of the
    list (cscale None = all 0); `ncomp` already clamped; a, b [K]; G None or complex128 [n_s, K]; vin
    None or complex128 [K]."""
    VR._check_longdouble()
    K = len(a)
    p, f, s, _ = valid(cpix, cflux, cscale, ncomp, nx, nz, n_s)
    jx = (p // nz).astype(LD) - LD(nx - 1) / LD(2)
    jz = (p % nz).astype(LD) - LD(nz - 1) / LD(2)
    out = np.zeros(K, dtype=np.clongdouble) if vin is None else np.asarray(vin).astype(np.clongdouble)
    S = np.zeros(K) if vin is None else np.abs(np.asarray(vin, dtype=np.complex128))
    S = np.where(np.isfinite(S), S, 0.0)
    if len(p):
        with np.errstate(invalid="ignore"):
            E = _unit(a, jx) * _unit(b, jz)                                  # [K, n]
            g = np.ones((K, len(p)), dtype=np.clongdouble) if G is None else \
                np.asarray(G, dtype=np.complex128).astype(np.clongdouble)[s, :].T
            out = out + LD(sign) * (g * E * f.astype(LD)[None, :]).sum(axis=1)
            S = S + (np.abs(g).astype(np.float64) * np.abs(f)[None, :]).sum(axis=1)
    bad = ~(np.isfinite(np.asarray(a, dtype=np.float64)) & np.isfinite(np.asarray(b, dtype=np.float64)))
    out = np.where(bad, np.clongdouble(complex(np.nan, np.nan)), out)
    return out, S


def bound(a, b, nx, nz, ncomp, n_s=1):
    """The derived bound on |got - ref| / S per visibility (see the module's head)."""
    a, b = np.abs(np.asarray(a, dtype=np.float64)), np.abs(np.asarray(b, dtype=np.float64))
    d = SLICE * -(-max(int(ncomp), 1) // CHUNK) * U
    return (2.0 * np.pi * (a * (nx - 1) / 2.0 + b * (nz - 1) / 2.0) * U + ROOT2 * PHASOR_PART +
            ROOT2 * d / (1.0 - d) + 2.0 * n_s * U + 4.0 * U)


def worst_ratio(got, ref, S, bnd):
    """max over the visibilities with finite reference of max(|Re err|, |Im err|) / (bound S)."""
    ref, got = np.asarray(ref), np.asarray(got)
    keep = np.isfinite(ref.real.astype(np.float64)) & np.isfinite(ref.imag.astype(np.float64)) & (S > 0)
    if not keep.any():
        return 0.0
    er = np.abs((got.real.astype(LD) - ref.real).astype(np.float64))[keep]
    ei = np.abs((got.imag.astype(LD) - ref.imag).astype(np.float64))[keep]
    return float(np.max(np.maximum(er, ei) / (np.broadcast_to(bnd, S.shape)[keep] * S[keep])))


def components_image_ref(cpix, cflux, cscale, ncomp, nx, nz, n_s=1):
    """One map -> float64 [n_s, nx nz]: a sequential Python sum in list order from +0.0."""
    out = np.zeros((n_s, nx * nz))
    p, f, s, _ = valid(cpix, cflux, cscale, ncomp, nx, nz, n_s)
    for pc, fc, sc in zip(p, f, s):
        out[sc, pc] = out[sc, pc] + fc
    return out


# ---- a float64 emulation of the stated order, and four planted mistakes ---------------------------
def vis_components_emulated(cpix, cflux, cscale, ncomp, nx, nz, a, b, n_s=1, G=None, vin=None, sign=1,
                            centre_shift=0.0, phase_sign=-1.0, phasor_dtype=np.float64,
                            g_shift=0):
    """The device's arithmetic in NumPy float64 (products and adds where the device fuses them): the
    scales outside, four slices in list order, G once per slice and scale, the slices in slice
    order, `in` last.  `centre_shift` = 0.5 uses n / 2 as the centre, `phase_sign` = +1 the opposite
    convention, `phasor_dtype` = float32 rounds the phasors, `g_shift` = 1 takes G of the next scale
    (cyclically): the planted mistakes the bound must reject."""
    K = len(a)
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p, f, s, idx = valid(cpix, cflux, cscale, ncomp, nx, nz, n_s)
    jx = (p // nz) - ((nx - 1) / 2.0 + centre_shift)
    jz = (p % nz) - ((nz - 1) / 2.0 + centre_shift)
    sl = (idx % CHUNK) // SLICE
    cast = lambda t: t.astype(phasor_dtype).astype(np.float64)
    T = np.zeros((4, K), dtype=np.complex128)
    for sc in range(n_s):
        for w in range(4):
            pr, pi = np.zeros(K), np.zeros(K)
            for c in np.nonzero((s == sc) & (sl == w))[0]:
                px, pz = a * jx[c], b * jz[c]
                px, pz = px - np.rint(px), pz - np.rint(pz)
                cx, sx = cast(np.cos(2 * np.pi * px)), cast(np.sin(2 * np.pi * px))
                cz, sz = cast(np.cos(2 * np.pi * pz)), cast(np.sin(2 * np.pi * pz))
                cr, si = cx * cz - sx * sz, sx * cz + cx * sz
                fc = sign * f[c]
                pr = pr + fc * cr
                pi = pi + phase_sign * fc * si
            if G is None:
                T[w] = (T[w].real + pr) + 1j * (T[w].imag + pi)
            else:
                g = np.asarray(G, dtype=np.complex128)[(sc + g_shift) % n_s]
                T[w] = ((T[w].real + g.real * pr) - g.imag * pi) + \
                    1j * ((T[w].imag + g.real * pi) + g.imag * pr)
    tot = ((T[0] + T[1]) + T[2]) + T[3]
    return tot if vin is None else np.asarray(vin, dtype=np.complex128) + tot


# ---- the cases of tests/test_gpu_vis_components.py ---------------------------------------------------
SHAPES = [(1, 1), (5, 3), (67, 131)]
N_VIS = [1, 63, 64, 65, 257]
N_COMP = [0, 1, 63, 64, 65, 1000]


def random_list(rng, nx, nz, stride, n_s=1, dup_share=0.3):
    """A row of `stride` components: pixels uniform over the grid with `dup_share` of them repeating
    an earlier one, fluxes of both signs over three decades, scales uniform in [0, n_s)."""
    npix = nx * nz
    p = rng.integers(0, npix, stride)
    for c in range(1, stride):
        if rng.random() < dup_share:
            p[c] = p[rng.integers(0, c)]
    f = rng.lognormal(0.0, 1.5, stride) * rng.choice([-1.0, 1.0], stride)
    s = rng.integers(0, n_s, stride)
    return p.astype(np.int32), f, s.astype(np.int32)


def random_g(rng, n_s, K):
    """A transform per scale and visibility: moduli in (0, 1], any phase; scale 0 is the delta: 1."""
    g = rng.uniform(0.05, 1.0, (n_s, K)) * np.exp(2j * np.pi * rng.random((n_s, K)))
    g[0] = 1.0
    return g.astype(np.complex128)
