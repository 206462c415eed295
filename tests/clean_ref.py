"""Reference for rjp_clean (K12) and rjp_restore (K13): Hogbom's CLEAN in long double, and the
checker that FOLLOWS the device.

Two correct implementations can legitimately part ways on a near-tie of two pixels, after which
their component lists have nothing in common.  So `follow` does not compare pick sequences: for
each component (p_c, f_c) the device recorded it checks the pick against its own long-double
residual R_ref -- which it then updates with the DEVICE's flux -- and leaves no case out:
    the pick is unmasked and finite,
    |R_ref[p_c]| >= max_mask |R_ref| - 2 b_t                     (it was a maximum, within the error)
    |f_c - gain R_ref[p_c]| <= gain b_t + u gain |R_ref[p_c]|    (see below)
    |R_ref[p_c]| > thresh - b_t                                  (it was above the threshold)
    no untouched pixel of lower index ties exactly with an untouched pick   (both still hold D)
and at the end: ncomp < n_iter only if max_mask |R_ref| <= thresh + b; the device's residual equals
R_ref within b per pixel; d_peak agrees within b; d_model equals the long-double scatter of the
list within ncomp u sum |f|; the slots at and beyond ncomp still hold the caller's poison.

The bound, term by term (u = 2^-53).  The device updates R[q] <- fma(-f, B, R[q]): ONE rounding per
update (`roundings` = 1; a float64 emulation without a fused multiply-add makes two), each at most
u times the magnitude of the result, which never exceeds env[q] = |D[q]| + sum_c |f_c| |B[q - p_c]|:
    b[q] = (updates of q so far) x roundings x u x env[q],        b_t = max_mask b.
The flux f = fl(gain R) is one more rounding of a product, u gain |R| (exact for gain = 1): the
second term of the flux check.  R_ref itself is rounded at 2^-64, 2048 times finer.
Independently of any pick, `conservation` evaluates D = R + sum_c f_c B(. - p_c) per pixel in long
double from the device's list, at the same bound."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TILE = 1024               # pixels per tile (clean.hip kClT)
REDUCE_PASS = 256         # partials one pass of the redundant reduction covers (kClB)


def tiling(n_maps, nx, nz):
    """clean.hip's tile rule restated: tiles of 1024 consecutive pixels of the flat image."""
    tiles = (nx * nz + TILE - 1) // TILE
    return {"tiles": tiles, "workgroups": tiles * n_maps}


def workspace_bytes(n_maps, nx, nz):
    """Two halves of (value f64, pixel i32) per map and tile, rounded up to 16 bytes."""
    return (tiling(n_maps, nx, nz)["workgroups"] * 24 + 15) // 16 * 16


def window(nx, nz, px, pz, ix, iz, cx=None, cz=None):
    """(image slices, beam slices) of the beam centred on pixel (ix, iz), clipped to the image."""
    cx = (px - 1) // 2 if cx is None else cx
    cz = (pz - 1) // 2 if cz is None else cz
    x0, x1 = max(0, ix - cx), min(nx, ix - cx + px)
    z0, z1 = max(0, iz - cz), min(nz, iz - cz + pz)
    return ((slice(x0, x1), slice(z0, z1)),
            (slice(x0 - ix + cx, x1 - ix + cx), slice(z0 - iz + cz, z1 - iz + cz)))


def candidates(R, mask):
    """Pixels that may be picked: unmasked and finite."""
    ok = np.isfinite(R.astype(np.float64))
    return ok if mask is None else ok & (np.asarray(mask) != 0)


def hogbom(D, B, mask, thresh, gain, n_iter, dtype=LD, centre=None, use_gain=True, use_abs=True,
           tie_low=True):
    """Hogbom's CLEAN of the image D [nx, nz] with the beam B [px, pz] in `dtype` arithmetic ->
    (cpix, cflux, residual).  dtype=LD is the reference, dtype=float64 the emulation of the
    device (two roundings per update: NumPy has no fused multiply-add).  The other switches plant
    mistakes: `centre` = a wrong beam centre (cx, cz), `use_gain=False` forgets the gain,
    `use_abs=False` takes the arg-max of R instead of |R|, `tie_low=False` the HIGHEST index of a
    tie."""
    nx, nz = D.shape
    px, pz = B.shape
    R = D.astype(dtype).copy()
    Bd = B.astype(dtype)
    cx, cz = (None, None) if centre is None else centre
    cpix, cflux = [], []
    for _ in range(n_iter):
        ok = candidates(R, mask)
        if not ok.any():
            break
        key = np.where(ok, np.abs(R) if use_abs else R, -np.inf).ravel()
        best = key.max()
        where = np.nonzero(key == best)[0]
        p = int(where[0] if tie_low else where[-1])
        v = R.ravel()[p]
        if not abs(v) > thresh:
            break
        f = (dtype(gain) * v) if use_gain else v
        cpix.append(p)
        cflux.append(f)
        im, bm = window(nx, nz, px, pz, p // nz, p % nz, cx, cz)
        R[im] = R[im] - f * Bd[bm]
    return np.array(cpix, dtype=np.int64), np.array(cflux, dtype=dtype), R


def follow(D, B, mask, thresh, gain, n_iter, cpix, cflux, ncomp, res, peak=None, model=None,
           model0=None, poison_pix=None, poison_flux=None, roundings=1):
    """Check what the device (or an emulation) made of the image D [nx, nz]: see the module's
    docstring.  `cpix`, `cflux`: the map's full rows [n_iter]; `res` the residual [nx, nz];
    `model0`: what d_model held on entry (zeros by default).  Raises AssertionError with the
    failing rule; -> the worst ratio (error / bound) over every check that has a bound."""
    nx, nz = D.shape
    px, pz = B.shape
    ncomp = int(ncomp)
    assert 0 <= ncomp <= n_iter, ("ncomp", ncomp)
    R = D.astype(LD).copy()
    absB = np.abs(B).astype(np.float64)
    BL = B.astype(LD)
    env = np.abs(np.where(np.isfinite(D), D, 0.0)).astype(np.float64)
    cnt = np.zeros(D.shape)
    g = LD(gain)
    worst = 0.0

    def ratio(err, bnd, rule):
        nonlocal worst
        err, bnd = float(err), float(bnd)
        assert err <= bnd, (rule, err, bnd)
        if bnd > 0:
            worst = max(worst, err / bnd)

    for c in range(ncomp):
        p, f = int(cpix[c]), LD(cflux[c])
        ok = candidates(R, mask)
        assert 0 <= p < nx * nz and ok.ravel()[p], ("component %d on a masked / non-finite pixel" % c, p)
        b = cnt * roundings * U * env
        bt = float(b[ok].max())
        top = float(np.abs(R[ok]).max())
        v = R.ravel()[p]
        ratio(top - float(abs(v)), 2 * bt, "component %d is not a maximum" % c)
        ratio(abs(f - g * v), gain * bt + (U * gain * float(abs(v)) if gain != 1.0 else 0.0) +
              2.0 ** -63 * float(abs(v)), "flux of component %d" % c)
        assert float(abs(v)) > thresh - bt, ("component %d below the threshold" % c, float(abs(v)))
        if cnt.ravel()[p] == 0:
            # a pixel nothing has touched yet holds D on the device too: an exact tie with an
            # untouched pixel of lower index is decidable, and the lower index must have won
            tie = (ok & (cnt == 0) & (np.abs(R) == abs(v))).ravel()
            assert not tie[:p].any(), ("component %d: a tie did not go to the lowest index" % c, p)
        im, bm = window(nx, nz, px, pz, p // nz, p % nz)
        R[im] = R[im] - f * BL[bm]
        env[im] += float(abs(f)) * absB[bm]
        cnt[im] += 1
    b = cnt * roundings * U * env
    ok = candidates(R, mask)
    top = float(np.abs(R[ok]).max()) if ok.any() else 0.0
    bt = float(b[ok].max()) if ok.any() else 0.0
    if ncomp < n_iter:
        assert top <= thresh + bt, ("stopped above the threshold", top, thresh)
    res = np.asarray(res, dtype=np.float64).reshape(nx, nz)
    fin = np.isfinite(D)
    assert np.array_equal(res[~fin], D[~fin], equal_nan=True), "a non-finite pixel changed"
    with np.errstate(invalid="ignore"):            # inf - inf at the non-finite pixels, left out
        err = np.abs(res.astype(LD) - R)[fin].astype(np.float64)
    assert np.all(err <= b[fin]), ("residual", float((err - b[fin]).max()))
    if (b[fin] > 0).any():
        worst = max(worst, float((err[b[fin] > 0] / b[fin][b[fin] > 0]).max()))
    if peak is not None:
        ratio(abs(float(peak) - top), bt, "d_peak")
    if model is not None:
        want = (np.zeros(D.shape) if model0 is None else model0).astype(LD).ravel().copy()
        for c in range(ncomp):
            want[int(cpix[c])] += LD(cflux[c])
        tol = ncomp * U * float(np.abs(np.asarray(cflux[:ncomp], dtype=np.float64)).sum())
        if model0 is not None:
            tol += ncomp * U * float(np.abs(model0).max())
        assert np.all(np.abs(np.asarray(model).astype(LD).ravel() - want) <= tol), "d_model"
    if poison_pix is not None:
        assert np.all(np.asarray(cpix[ncomp:]) == poison_pix), "a slot beyond ncomp was written"
    if poison_flux is not None:
        tail = np.asarray(cflux[ncomp:], dtype=np.float64)
        assert np.array_equal(tail, np.full(tail.shape, poison_flux), equal_nan=True), \
            "a slot beyond ncomp was written"
    return worst


def conservation(D, B, cpix, cflux, ncomp, res, roundings=1):
    """D = R + sum_c f_c B(. - p_c) per pixel, in long double from the list alone (no pick is
    looked at) -> the worst |D - R - sum| / b over the pixels that were updated."""
    nx, nz = D.shape
    px, pz = B.shape
    S = np.zeros(D.shape, dtype=LD)
    env = np.abs(np.where(np.isfinite(D), D, 0.0)).astype(np.float64)
    cnt = np.zeros(D.shape)
    for c in range(int(ncomp)):
        p, f = int(cpix[c]), LD(cflux[c])
        im, bm = window(nx, nz, px, pz, p // nz, p % nz)
        S[im] += f * B.astype(LD)[bm]
        env[im] += float(abs(f)) * np.abs(B)[bm]
        cnt[im] += 1
    fin = np.isfinite(D)
    with np.errstate(invalid="ignore"):
        err = np.abs(D.astype(LD) - np.asarray(res, dtype=np.float64).reshape(nx, nz).astype(LD) - S)
    err = err[fin].astype(np.float64)
    b = (cnt * roundings * U * env)[fin]
    assert np.all(err <= b), ("conservation", float((err - b).max()))
    return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0


# ---- inputs ---------------------------------------------------------------------------------------
def random_beam(rng, px, pz, n_vis=40):
    """A dirty beam of random (u, v) coverage on an odd grid: exactly 1 at the centre, point
    symmetric, sidelobes of a few tenths."""
    jx = np.arange(px) - (px - 1) / 2
    jz = np.arange(pz) - (pz - 1) / 2
    a = rng.uniform(-0.25, 0.25, n_vis)
    b = rng.uniform(-0.25, 0.25, n_vis)
    ph = 2 * np.pi * (a[:, None, None] * jx[None, :, None] + b[:, None, None] * jz[None, None, :])
    beam = np.cos(ph).mean(axis=0)
    beam[(px - 1) // 2, (pz - 1) // 2] = 1.0
    return np.ascontiguousarray(beam)


def random_image(rng, nx, nz, full_beam, n_src=5, noise=1e-3, sources=None):
    """A few point sources convolved with `full_beam` ([2 nx - 1, 2 nz - 1], or any smaller odd
    window of a beam) plus continuous noise at `noise` of the peak: near-ties have measure zero."""
    D = np.zeros((nx, nz))
    src = sources if sources is not None else [
        (int(rng.integers(nx)), int(rng.integers(nz)), float(rng.uniform(0.3, 1.0)) *
         (1 if rng.random() < 0.8 else -1)) for _ in range(n_src)]
    for ix, iz, s in src:
        im, bm = window(nx, nz, full_beam.shape[0], full_beam.shape[1], ix, iz)
        D[im] += s * full_beam[bm]
    return D + noise * np.abs(D).max() * rng.standard_normal(D.shape)


def restore_ref(cpix, cflux, ncomp, abc, nx, nz, add=None):
    """K13 in long double -> (out [nx, nz] LD, bound [nx, nz]); a term whose exponent lies below
    -700 counts as exactly 0, as the device's does.  The bound, term by term (g_c the Gaussian of
    component c at the pixel, T_c = A dx^2 + |2 B dx dz| + C dz^2 >= |exponent|):
        sum_c |f_c| g_c (1e-14 + 6 T_c u)    exp_any's stated error, and the roundings of its
                                             argument (three products of two factors, two sums)
      + (ncomp + 2) u sum_c |f_c| g_c        one fma per term
      + u |out|                              the residual, added last
      + 1e-300 sum |f_c|                     a term within a rounding of the -700 cut."""
    A, B, C = (LD(x) for x in abc)
    qx = np.arange(nx, dtype=LD)[:, None]
    qz = np.arange(nz, dtype=LD)[None, :]
    out = np.zeros((nx, nz), dtype=LD)
    scale = np.zeros((nx, nz), dtype=LD)
    bound = np.zeros((nx, nz), dtype=LD)
    n = int(ncomp)
    for c in range(n):
        p = int(cpix[c])
        dx, dz = qx - (p // nz), qz - (p % nz)
        e = -(A * dx * dx + 2 * B * dx * dz + C * dz * dz)
        T = A * dx * dx + abs(2 * B * dx * dz) + C * dz * dz
        g = np.where(e < -700, LD(0), np.exp(np.maximum(e, LD(-800))))
        out += LD(cflux[c]) * g
        scale += abs(LD(cflux[c])) * g
        bound += abs(LD(cflux[c])) * g * (1e-14 + 6 * T * U)
    bound += (n + 2) * U * scale + 1e-300 * float(np.abs(np.asarray(cflux[:n], dtype=np.float64)).sum())
    if add is not None:
        out = out + np.asarray(add, dtype=np.float64).reshape(nx, nz).astype(LD)
    return out, (bound + U * np.abs(out)).astype(np.float64)
