"""The CLEAN major-cycle loop of `Imager._clean_images` (major_cycles >= 1) restated in NumPy float64,
with the operators it is made of: the direct Fourier sum and its adjoint, the visibilities of a
component list, Hogbom's minor cycles (tests/clean_ref.py), the sidelobe level, the per-run
threshold and the truncation at `niter`.  Nothing here runs on a device.

THE LOOP, per map, N = major_cycles, thr the user's threshold, `left` = niter at the start:
  setup   D = dirty image of V, B = dirty beam on the `psf_shape` window, (A, B, C) the clean beam's form
  sidelobe = max |B| over the window's pixels with A dx^2 + 2 B dx dz + C dz^2 >= 4 ln 2 (outside twice
          the half-power ellipse; THIS project's definition, not CASA's), 0 when there is none
  run r = 1 .. N on the residual R (R = D before the first):
          peak = masked max |R|;  stop when peak <= thr or left = 0
          t = thr on run N, else max(thr, clip(cyclefactor sidelobe, min_psf_fraction, max_psf_fraction) peak)
          minor cycles on R with threshold t and min(cycleniter or niter, left) iterations; of what
          they find only the first `left` are kept (CLEAN's picks are sequential: exactly what
          n_iter = left would have found); the list grows, left shrinks
          V_res = V - vis(whole list), from the ORIGINAL V;  R = dirty image of V_res
  the residual is the last R: a function of the list and the data, whatever the beam window.

THE EXPERIMENT (seed 7): a 33 x 33 image, 300 random baselines at <= 0.25 cycles per cell, point sources
of 1, 0.5 and 0.3 Jy and a 3 x 3 patch of 0.05; gain 0.1, niter 2000, threshold 1e-6; a round clean beam
of 2.4 cells FWHM (the dirty beam's main lobe is too narrow for a fit); sidelobe = 0.238.  True peak =
max |dirty image of (V - the components' visibilities)|.  Measured with this module
(tests/test_major_cycles_reference_cpu.py asserts and prints them):
    beam window   run                  reported peak   true peak   minor-only / this
    65 x 65       minor only           9.1e-5          9.1e-5      (identity D = R + sum f B_full: 1.4e-15)
    9 x 9         minor only           0.13            0.40        (identity missed by 0.53)
    9 x 9         8 re-imagings        7.8e-4          7.8e-4      511
    17 x 17       minor only           0.025           0.34        (identity missed by 0.36)
    17 x 17       8 re-imagings        4.2e-4          4.2e-4      790
(The write-up that proposed the loop quoted 4.7e-4 = 1 / 850 and 2.7e-4 = 1 / 1250 for the same seed.  It
took the sidelobe as max |B| outside a radius of 3 cells of the FULL beam, 0.187 here; the loop defines it
in the beam window outside twice the half-power ellipse of the clean beam -- 2.4 cells FWHM here, so
from 2.4 cells out -- which gives 0.238 and higher thresholds on every run before the last.  The
threshold rule itself is the one stated above, unchanged.)
The runs of the 9 x 9 case kept 15, 38, 43, 78, 79, 139, 132 and 1476 components at thresholds 0.35,
0.12, 0.043, 0.016, 6.7e-3, 2.6e-3, 1.2e-3 and 1e-6.
"""
import numpy as np

from tests import clean_ref as C

FOUR_LN2 = 4.0 * np.log(2.0)
DBL_MAX = float(np.finfo(np.float64).max)
BEAM_FWHM = 2.4                  # cells: the round clean beam of the experiment
CLEAN_BEAM = (FOUR_LN2 / BEAM_FWHM ** 2, 0.0, FOUR_LN2 / BEAM_FWHM ** 2)


def phasors(c, n):
    """e^{-2 pi i c j}, j = index - (n - 1) / 2 -> complex128 [len(c), n]."""
    j = np.arange(n) - (n - 1) / 2.0
    return np.exp(-2j * np.pi * np.outer(c, j))


def vis(I, a, b):
    """K10 in float64: V[k] = sum I[x, z] e^{-2 pi i (a jx + b jz)}."""
    return np.einsum("kx,xz,kz->k", phasors(a, I.shape[0]), I, phasors(b, I.shape[1]))


def dirty(V, a, b, nx, nz, w=None):
    """K11 over the sum of the weights: D = sum_k w_k Re(V_k e^{+2 pi i (a jx + b jz)}) / sum w."""
    w = np.ones(len(a)) if w is None else np.asarray(w, dtype=np.float64)
    return np.real(np.einsum("k,kx,kz->xz", V * w, np.conj(phasors(a, nx)), np.conj(phasors(b, nz)))) / w.sum()


def beam(a, b, px, pz, w=None):
    return dirty(np.ones(len(a), dtype=np.complex128), a, b, px, pz, w)


def crop(Bfull, px, pz):
    cx, cz = (Bfull.shape[0] - 1) // 2, (Bfull.shape[1] - 1) // 2
    hx, hz = (px - 1) // 2, (pz - 1) // 2
    return np.ascontiguousarray(Bfull[cx - hx:cx + hx + 1, cz - hz:cz + hz + 1])


def comp_vis(cpix, cflux, nx, nz, a, b):
    """K18 without scales in float64: the visibilities of the list."""
    cpix = np.asarray(cpix, dtype=np.int64)
    if len(cpix) == 0:
        return np.zeros(len(a), dtype=np.complex128)
    jx, jz = cpix // nz - (nx - 1) / 2.0, cpix % nz - (nz - 1) / 2.0
    ph = np.exp(-2j * np.pi * (np.outer(a, jx) + np.outer(b, jz)))
    return ph @ np.asarray(cflux, dtype=np.float64)


def true_residual(V, a, b, nx, nz, cpix, cflux, w=None):
    return dirty(V - comp_vis(cpix, cflux, nx, nz, a, b), a, b, nx, nz, w)


def masked_peak(R, mask=None):
    ok = C.candidates(R, mask)
    return float(np.abs(R[ok]).max()) if ok.any() else 0.0


def sidelobe(B, abc):
    """max |B| over the window's pixels outside twice the half-power ellipse of the clean beam."""
    A, Bq, Cq = abc
    dx = (np.arange(B.shape[0]) - (B.shape[0] - 1) // 2)[:, None].astype(np.float64)
    dz = (np.arange(B.shape[1]) - (B.shape[1] - 1) // 2)[None, :].astype(np.float64)
    out = A * dx * dx + 2.0 * Bq * dx * dz + Cq * dz * dz >= FOUR_LN2
    return float(np.abs(B[out]).max()) if out.any() else 0.0


def run_threshold(thr, peak, side, cyclefactor, min_frac, max_frac, last):
    """The threshold of one minor run (the module's head)."""
    if last:
        return float(thr)
    return max(float(thr), min(max(cyclefactor * side, min_frac), max_frac) * peak)


def run_iterations(niter, cycleniter, left):
    """n_r = min(cycleniter or niter, max_m left[m]); `left`: one number or one per map."""
    return int(min(cycleniter if cycleniter else niter, np.max(left)))


def keep(found, left):
    """How many of the `found` components of a run a map keeps."""
    return int(min(found, left))


def major_cycles(V, a, b, nx, nz, B, abc, niter, gain, thr, N, cyclefactor=1.5, cycleniter=None,
                 min_frac=0.05, max_frac=0.8, mask=None, w=None):
    """The loop for one map -> dict(cpix, cflux, runs [{start, n, peak, threshold}], sidelobe,
    residual [nx, nz], vis_residual [K], residuals [the R every run started from])."""
    D = dirty(V, a, b, nx, nz, w)
    side = sidelobe(B, abc)
    cpix, cflux, runs, seen = [], [], [], []
    R, left, Vres = D, int(niter), V.copy()
    for r in range(1, N + 1):
        peak = masked_peak(R, mask)
        if left == 0 or not peak > thr:
            break
        t = run_threshold(thr, peak, side, cyclefactor, min_frac, max_frac, r == N)
        n_r = run_iterations(niter, cycleniter, left)
        cp, cf, _ = C.hogbom(R, B, mask, t, gain, n_r, dtype=np.float64)
        n = keep(len(cp), left)
        runs.append(dict(start=len(cpix), n=n, peak=peak, threshold=t))
        seen.append(R)
        cpix += [int(p) for p in cp[:n]]
        cflux += [float(f) for f in cf[:n]]
        left -= n
        Vres = V - comp_vis(cpix, cflux, nx, nz, a, b)
        R = dirty(Vres, a, b, nx, nz, w)
    return dict(cpix=np.array(cpix, dtype=np.int64), cflux=np.array(cflux), runs=runs, sidelobe=side,
                residual=R, vis_residual=Vres, residuals=seen)


# ---- the experiment -------------------------------------------------------------------------------------
def experiment(seed=7, n=33, K=300, amax=0.25):
    """-> dict(a, b, sky, V, D, Bfull): the setup of the module's head."""
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(-amax, amax, K), rng.uniform(-amax, amax, K)
    sky = np.zeros((n, n))
    sky[16, 16], sky[10, 22], sky[25, 8] = 1.0, 0.5, 0.3
    sky[12:15, 12:15] += 0.05
    V = vis(sky, a, b)
    return dict(a=a, b=b, sky=sky, V=V, D=dirty(V, a, b, n, n), Bfull=beam(a, b, 2 * n - 1, 2 * n - 1), n=n)


def conservation_error(D, Bfull, cpix, cflux, R):
    """max |D - R - sum f B_full(. - p)|: zero to rounding iff R is the true residual."""
    nx, nz = D.shape
    S = np.zeros(D.shape)
    for p, f in zip(cpix, cflux):
        im, bm = C.window(nx, nz, Bfull.shape[0], Bfull.shape[1], int(p) // nz, int(p) % nz)
        S[im] += f * Bfull[bm]
    return float(np.abs(D - R - S).max())
