"""Reference for rjp_convolve2d and rjp_msclean (K17): a long-double convolution in the stated term
order, and a long-double multi-scale CLEAN that FOLLOWS a given component list, as clean_ref.py does
for K12 (two correct cleans may part ways on a near-tie, after which their lists have nothing in
common).

Convolution.  out[i, j] = add[i, j] + sum_{a, b} ker[a, b] in[i - (a - ca), j - (b - cb)], a outer and
b inner, both ascending, `in` zero outside the image (the terms are taken, as products with 0, so a
NaN or infinite kernel value or pixel spreads exactly as IEEE arithmetic spreads it).  The device
makes one fma per term, kx kz roundings, each at most u = 2^-53 times a partial sum that never exceeds
scale = |add| + sum |ker| |in|; one more u covers the reference's own rounding at 2^-64 many times
over:  bound = (kx kz + 1) u scale.  (A float64 emulation without a fused multiply-add makes two
roundings per term: `roundings` = 2.)

Multi-scale CLEAN.  n_s planes R_k, cross beams X[k][l] (packed upper triangle, `tri`), weights w_k.
`follow` keeps its own long-double planes, which it updates with the DEVICE's (pixel, scale, flux),
and checks for every component c = (p, k, f):
    plane k has weight > 0, the pixel is unmasked and R_ref_k[p] finite;
    max score - w_k |R_ref_k[p]| <= 2 b_t + 2 u max score          (it was a maximum)
    |f - gain R_ref_k[p] / X_kk| <= 3 u |gain R / X_kk| + gain b_k[p] / |X_kk|
    w_k |R_ref_k[p]| > thresh - b_t - u score                      (it was above the threshold)
    no untouched candidate that comes first in (scale, pixel) order ties exactly with an untouched
    pick (both still hold their input bits, so the float64 scores are the device's)
and at the end: ncomp < n_iter only if max score <= thresh + b_t + u max score; every plane equals
R_ref within b per pixel; d_peak within b_t + u max score; the model planes equal the scatter of the
list within ncomp u sum |f|; the slots beyond ncomp hold the caller's poison.
The bound, term by term.  The device updates R_l[q] <- fma(-f, X, R_l[q]): one rounding per update,
at most u times the result, which never exceeds env_l[q] = |R0_l[q]| + sum_c |f_c| |X[k_c][l][q - p_c]|:
    b_l[q] = (updates of q in plane l so far) x roundings x u x env_l[q],   b_t = max w_l b_l[q]
over the candidates.  The score is one rounded product, u s; f is one rounded product and one rounded
division of a value within b of the reference's: 2 u |f| and gain b / |X_kk| (a third u is slack for
the reference's own roundings).
`conservation` evaluates R_l = R0_l - sum_c f_c X[k_c][l](. - p_c) on ALL planes from the list alone."""
import numpy as np

from tests import clean_ref as C

LD = np.longdouble
U = 2.0 ** -53
TILE = C.TILE
REDUCE_PASS = C.REDUCE_PASS
CONV_TILE = (16, 64)          # rows x columns of output per workgroup (RJP_CONV_TILE_X / _Z)
CONV_LDS = 8192               # doubles of LDS per workgroup (convolve.hip kCvLds)
CONV_MAX_K = 255

MSG = {
    "conv_null": "rjp_convolve2d: NULL input, kernels or output",
    "conv_sizes": "rjp_convolve2d: n_maps, nx, nz, kx and kz must be positive",
    "conv_even": "rjp_convolve2d: kx and kz must be odd (the kernel's centre is a pixel)",
    "conv_max": "rjp_convolve2d: kx and kz must not exceed RJP_CONV_MAX_K (255)",
    "conv_nker": "rjp_convolve2d: n_ker must be 1 or n_maps",
    "conv_npix": "rjp_convolve2d: nx * nz exceeds 2^31 - 1",
    "conv_wgs": "rjp_convolve2d: more than 2^31 - 1 workgroups",
    "null": "rjp_msclean: NULL planes, cross beams, weights, thresholds or component outputs",
    "sizes": "rjp_msclean: n_maps, n_s, nx, nz, px and pz must be positive",
    "even": "rjp_msclean: px and pz must be odd (the beam's centre is a pixel)",
    "npsf": "rjp_msclean: n_psf must be 1 or n_maps",
    "npix": "rjp_msclean: nx * nz exceeds 2^31 - 1",
    "gain": "rjp_msclean: gain must lie in (0, 1]",
    "niter": "rjp_msclean: n_iter < 1",
    "thresh": "rjp_msclean: negative or non-finite threshold",
    "weight": "rjp_msclean: negative or non-finite weight",
    "wgs": "rjp_msclean: more than 2^31 - 1 workgroups",
    "work": "rjp_msclean: workspace smaller than rjp_msclean_workspace()",
}


# ---- the tile rules, restated -----------------------------------------------------------------------
def conv_workgroups(n_maps, nx, nz):
    tx, tz = CONV_TILE
    return n_maps * ((nx + tx - 1) // tx) * ((nz + tz - 1) // tz)


def conv_chunk_rows(kx, kz):
    """Kernel rows per LDS chunk: the most for which (16 + ka - 1)(64 + kz - 1) + ka kz doubles fit."""
    w = CONV_TILE[1] + kz - 1
    return min(kx, (CONV_LDS - (CONV_TILE[0] - 1) * w) // (w + kz))


def ms_workgroups(n_maps, n_s, nx, nz):
    return n_maps * n_s * ((nx * nz + TILE - 1) // TILE)


def ms_workspace_bytes(n_maps, n_s, nx, nz):
    """Two halves of (value f64, pixel i32) per map, plane and tile, rounded up to 16 bytes."""
    return (ms_workgroups(n_maps, n_s, nx, nz) * 24 + 15) // 16 * 16


def tri(k, l, n_s):
    """The plane of X[k][l] in the packed upper triangle (row order); X[l][k] is the same plane."""
    a, b = min(k, l), max(k, l)
    return a * n_s - a * (a - 1) // 2 + (b - a)


# ---- the convolution ---------------------------------------------------------------------------------
def conv(inp, ker, add=None, dtype=LD, flip=True):
    """-> (out [nx, nz] in `dtype`, scale [nx, nz] float64 = |add| + sum |ker| |in|).  `flip=False`
    plants the mistake of a correlation: in[i + (a - ca), j + (b - cb)]."""
    inp, ker = np.asarray(inp), np.asarray(ker)
    nx, nz = inp.shape
    kx, kz = ker.shape
    ca, cb = (kx - 1) // 2, (kz - 1) // 2
    pad = np.zeros((nx + kx - 1, nz + kz - 1), dtype=dtype)
    pad[ca:ca + nx, cb:cb + nz] = inp.astype(dtype)
    with np.errstate(invalid="ignore"):
        apad = np.abs(np.where(np.isfinite(pad.astype(np.float64)), pad, 0)).astype(np.float64)
    out = np.zeros((nx, nz), dtype=dtype) if add is None else np.asarray(add).astype(dtype).copy()
    with np.errstate(invalid="ignore"):
        scale = np.abs(np.where(np.isfinite(out.astype(np.float64)), out, 0)).astype(np.float64)
    kd = ker.astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(kx):
            for b in range(kz):
                # in[i - (a - ca)] = pad[i - a + 2 ca] = pad[i + (kx - 1 - a)]
                ra, rb = (kx - 1 - a, kz - 1 - b) if flip else (a, b)
                out += kd[a, b] * pad[ra:ra + nx, rb:rb + nz]
                if np.isfinite(float(ker[a, b])):
                    scale += abs(float(ker[a, b])) * apad[ra:ra + nx, rb:rb + nz]
    return out, scale


def conv_bound(kx, kz, scale, roundings=1):
    return (roundings * kx * kz + 1) * U * scale


def check_conv(got, inp, ker, add=None, roundings=1, **planted):
    """`got` against the long-double sum per pixel: the NaN pattern exactly the reference's, infinite
    values equal, the rest within the bound -> the worst error / bound."""
    want, scale = conv(inp, ker, add, **planted)
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    w64 = want.astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(w64)), "the NaN pattern differs from the reference's"
    inf = np.isinf(w64)
    assert np.array_equal(got[inf], w64[inf]), "an infinite pixel differs"
    fin = np.isfinite(w64)
    err = np.abs(got[fin].astype(LD) - want[fin]).astype(np.float64)
    bnd = conv_bound(ker.shape[0], ker.shape[1], scale[fin], roundings)
    assert np.all(err <= bnd), ("convolution", float((err - bnd).max()))
    return float((err[bnd > 0] / bnd[bnd > 0]).max()) if (bnd > 0).any() else 0.0


# ---- the multi-scale CLEAN ------------------------------------------------------------------------------
def _cands(R, weight, mask):
    """[n_s, nx, nz] bool: planes of weight > 0, pixels unmasked and finite."""
    ok = np.isfinite(R.astype(np.float64)) & (np.asarray(weight)[:, None, None] > 0)
    return ok if mask is None else ok & (np.asarray(mask) != 0)[None]


def dead(X, weight, n_s):
    cx, cz = (X.shape[1] - 1) // 2, (X.shape[2] - 1) // 2
    d = np.array([float(X[tri(k, k, n_s), cx, cz]) for k in range(n_s)])
    return bool(np.any((np.asarray(weight) > 0) & ((d == 0) | ~np.isfinite(d))))


def msclean(R0, X, weight, mask, thresh, gain, n_iter, dtype=LD, transpose_lower=False, divide=True,
            tie_low_scale=True, update_all=True):
    """Multi-scale CLEAN of the planes R0 [n_s, nx, nz] with the cross beams X [n_s (n_s + 1) / 2, px,
    pz] in `dtype` arithmetic -> (cpix, cscale, cflux, planes).  dtype=LD is the free-running reference,
    float64 the emulation of the device (two roundings per update).  The switches plant mistakes:
    `transpose_lower` = X[l][k], k > l, read from the TRANSPOSED plane (point reflection about the
    centre); `divide=False` = f without the division; `tie_low_scale=False` = a tie goes to the
    higher scale; `update_all=False` = only the picked plane is updated."""
    n_s, nx, nz = R0.shape
    px, pz = X.shape[1:]
    R = R0.astype(dtype).copy()
    Xd = X.astype(dtype)
    w = np.asarray(weight, dtype=dtype)
    cpix, cscale, cflux = [], [], []
    if dead(X, weight, n_s):
        return np.array([], dtype=np.int64), np.array([], dtype=np.int64), np.array([], dtype=dtype), R
    for _ in range(n_iter):
        ok = _cands(R, weight, mask)
        if not ok.any():
            break
        key = np.where(ok, w[:, None, None] * np.abs(R), -np.inf).reshape(n_s, -1)
        where = np.argwhere(key == key.max())               # (scale, pixel) in lexicographic order
        k, p = (int(x) for x in (where[0] if tie_low_scale else where[-1]))
        v = R[k].ravel()[p]
        if not key.max() > thresh:
            break
        f = dtype(gain) * v
        if divide:
            f = f / Xd[tri(k, k, n_s), (px - 1) // 2, (pz - 1) // 2]
        cpix.append(p), cscale.append(k), cflux.append(f)
        im, bm = C.window(nx, nz, px, pz, p // nz, p % nz)
        for l in range(n_s) if update_all else (k,):
            plane = Xd[tri(k, l, n_s)]
            if transpose_lower and k > l:
                plane = plane[::-1, ::-1]
            R[l][im] = R[l][im] - f * plane[bm]
    return (np.array(cpix, dtype=np.int64), np.array(cscale, dtype=np.int64),
            np.array(cflux, dtype=dtype), R)


def follow(R0, X, weight, mask, thresh, gain, n_iter, cpix, cscale, cflux, ncomp, res, peak=None,
           model=None, model0=None, poison_pix=None, poison_flux=None, roundings=1):
    """Check what the device (or an emulation) made of the planes R0 [n_s, nx, nz]: see the module's
    docstring.  `cpix`, `cscale`, `cflux`: the map's full rows [n_iter]; `res` the planes on exit.
    Raises AssertionError naming the rule; -> the worst error / bound."""
    n_s, nx, nz = R0.shape
    px, pz = X.shape[1:]
    cx, cz = (px - 1) // 2, (pz - 1) // 2
    ncomp = int(ncomp)
    assert 0 <= ncomp <= n_iter, ("ncomp", ncomp)
    res = np.asarray(res, dtype=np.float64).reshape(n_s, nx, nz)
    w64 = np.asarray(weight, dtype=np.float64)
    if dead(X, weight, n_s):
        assert ncomp == 0 and np.array_equal(res, R0, equal_nan=True), "a dead map was cleaned"
        assert peak is None or float(peak) == 0.0
        return 0.0
    R = R0.astype(LD).copy()
    XL, absX = X.astype(LD), np.abs(X).astype(np.float64)
    w = w64.astype(LD)[:, None, None]
    env = np.abs(np.where(np.isfinite(R0), R0, 0.0)).astype(np.float64)
    cnt = np.zeros(R0.shape)
    g = LD(gain)
    worst = 0.0

    def ratio(err, bnd, rule):
        nonlocal worst
        err, bnd = float(err), float(bnd)
        assert err <= bnd, (rule, err, bnd)
        if bnd > 0:
            worst = max(worst, err / bnd)

    def state():
        ok = _cands(R, weight, mask)
        b = cnt * roundings * U * env
        if not ok.any():
            return ok, b, 0.0, 0.0
        return ok, b, float((w64[:, None, None] * b)[ok].max()), float((w * np.abs(R))[ok].max())

    for c in range(ncomp):
        p, k, f = int(cpix[c]), int(cscale[c]), LD(cflux[c])
        ok, b, bt, top = state()
        assert 0 <= k < n_s and 0 <= p < nx * nz and ok[k].ravel()[p], \
            ("component %d on a masked / non-finite pixel or a plane of weight 0" % c, k, p)
        v = R[k].ravel()[p]
        s = float(w64[k] * abs(v))
        ratio(top - s, 2 * bt + 2 * U * top, "component %d is not a maximum" % c)
        xkk = XL[tri(k, k, n_s), cx, cz]
        ft = g * v / xkk
        ratio(abs(f - ft), 3 * U * float(abs(ft)) + gain * float(b[k].ravel()[p]) / float(abs(xkk)),
              "flux of component %d" % c)
        assert s > thresh - bt - U * s, ("component %d below the threshold" % c, s)
        if cnt[k].ravel()[p] == 0:
            # untouched pixels hold their input bits on the device too: an exact tie of the float64
            # scores is decidable, and the lower scale, then the lower pixel, must have won
            s64 = w64[:, None, None] * np.abs(R0)
            tie = (ok & (cnt == 0) & (s64 == w64[k] * abs(float(R0[k].ravel()[p])))).reshape(n_s, -1)
            assert not tie[:k].any() and not tie[k, :p].any(), \
                ("component %d: a tie did not go to the lower scale, then the lower pixel" % c, k, p)
        im, bm = C.window(nx, nz, px, pz, p // nz, p % nz)
        for l in range(n_s):
            t = tri(k, l, n_s)
            R[l][im] = R[l][im] - f * XL[t][bm]
            env[l][im] += float(abs(f)) * absX[t][bm]
            cnt[l][im] += 1
    ok, b, bt, top = state()
    if ncomp < n_iter:
        assert top <= thresh + bt + U * top, ("stopped above the threshold", top, thresh)
    fin = np.isfinite(R0)
    assert np.array_equal(res[~fin], R0[~fin], equal_nan=True), "a non-finite pixel changed"
    with np.errstate(invalid="ignore"):
        err = np.abs(res.astype(LD) - R)[fin].astype(np.float64)
    assert np.all(err <= b[fin]), ("residual planes", float((err - b[fin]).max()))
    if (b[fin] > 0).any():
        worst = max(worst, float((err[b[fin] > 0] / b[fin][b[fin] > 0]).max()))
    if peak is not None:
        ratio(abs(float(peak) - top), bt + U * top, "d_peak")
    if model is not None:
        want = (np.zeros(R0.shape) if model0 is None else model0).astype(LD).reshape(n_s, -1).copy()
        for c in range(ncomp):
            want[int(cscale[c]), int(cpix[c])] += LD(cflux[c])
        tol = ncomp * U * float(np.abs(np.asarray(cflux[:ncomp], dtype=np.float64)).sum())
        if model0 is not None:
            tol += ncomp * U * float(np.abs(model0).max())
        assert np.all(np.abs(np.asarray(model).astype(LD).reshape(n_s, -1) - want) <= tol), "d_model"
    if poison_pix is not None:
        assert np.all(np.asarray(cpix[ncomp:]) == poison_pix), "a pixel slot beyond ncomp was written"
        assert np.all(np.asarray(cscale[ncomp:]) == poison_pix), "a scale slot beyond ncomp was written"
    if poison_flux is not None:
        tail = np.asarray(cflux[ncomp:], dtype=np.float64)
        assert np.array_equal(tail, np.full(tail.shape, poison_flux), equal_nan=True), \
            "a flux slot beyond ncomp was written"
    return worst


def conservation(R0, X, cpix, cscale, cflux, ncomp, res, roundings=1):
    """R_l = R0_l - sum_c f_c X[k_c][l](. - p_c) on every plane, in long double from the list alone
    -> the worst error / bound over the pixels that were updated."""
    n_s, nx, nz = R0.shape
    px, pz = X.shape[1:]
    S = np.zeros(R0.shape, dtype=LD)
    env = np.abs(np.where(np.isfinite(R0), R0, 0.0)).astype(np.float64)
    cnt = np.zeros(R0.shape)
    for c in range(int(ncomp)):
        p, k, f = int(cpix[c]), int(cscale[c]), LD(cflux[c])
        im, bm = C.window(nx, nz, px, pz, p // nz, p % nz)
        for l in range(n_s):
            t = tri(k, l, n_s)
            S[l][im] += f * X[t].astype(LD)[bm]
            env[l][im] += float(abs(f)) * np.abs(X[t])[bm]
            cnt[l][im] += 1
    fin = np.isfinite(R0)
    with np.errstate(invalid="ignore"):
        err = np.abs(R0.astype(LD) - np.asarray(res, dtype=np.float64).reshape(R0.shape).astype(LD) - S)
    err = err[fin].astype(np.float64)
    b = (cnt * roundings * U * env)[fin]
    assert np.all(err <= b), ("conservation", float((err - b).max()))
    return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0


# ---- inputs --------------------------------------------------------------------------------------------
def conv64(x, k):
    """A float64 convolution for building inputs (no claim on its rounding)."""
    return conv(x, k, dtype=np.float64)[0]


def scale_problem(rng, nx, nz, scales, psf=None, n_src=4, noise=1e-3):
    """A multi-scale problem the way the imaging chain builds it: a random dirty beam on a grid
    4 h_max larger than the beam window, the cross beams X[k][l] = m_k * m_l * B cropped to the
    window, a dirty image of a few sources of mixed scales, the planes R0_l = m_l * D and the
    weights 1 / X_kk(centre) -> (R0 [n_s, nx, nz], X [tri, px, pz], weight [n_s]).  `scales`: the
    planes' scales, the first one 0; `psf`: the beam window (px, pz), default full (2 nx - 1, 2 nz - 1)."""
    from rajepy_amd.imaging import scale_kernel
    kers = [scale_kernel(s) for s in scales]
    n_s = len(scales)
    hmax = max(k.shape[0] // 2 for k in kers)
    px, pz = (2 * nx - 1, 2 * nz - 1) if psf is None else psf
    g = 2 * hmax
    big = C.random_beam(rng, px + 2 * g, pz + 2 * g)
    single = [conv64(big, k) for k in kers]
    X = np.stack([conv64(single[k], kers[l])[g:g + px, g:g + pz] for k in range(n_s)
                  for l in range(k, n_s)])
    B = big[g:g + px, g:g + pz]
    D = np.zeros((nx, nz))
    for _ in range(n_src):
        ix, iz = int(rng.integers(nx)), int(rng.integers(nz))
        src = np.zeros((nx, nz))
        src[ix, iz] = float(rng.uniform(0.3, 1.0)) * (1 if rng.random() < 0.8 else -1)
        src = conv64(src, kers[int(rng.integers(n_s))])
        for jx, jz in np.argwhere(src != 0):
            im, bm = C.window(nx, nz, px, pz, int(jx), int(jz))
            D[im] += src[jx, jz] * B[bm]
    D += noise * max(np.abs(D).max(), 1e-3) * rng.standard_normal(D.shape)
    R0 = np.stack([conv64(D, k) for k in kers])
    cx, cz = (px - 1) // 2, (pz - 1) // 2
    weight = np.array([1.0 / X[tri(k, k, n_s), cx, cz] for k in range(n_s)])
    return np.ascontiguousarray(R0), np.ascontiguousarray(X), weight
