"""Reference for rjp_mtmfs (K19): a long-double multi-term MFS CLEAN that FOLLOWS a given component
list, as clean_ref.py does for K12 and msclean_ref.py for K17 (two correct cleans may part ways on a
near-tie, after which their lists have nothing in common).

The algorithm (include/rjprt.h, K19).  n_t Taylor planes R_t, spectral beams B_0 .. B_{2 n_t - 2}, the
inverse Hessian Hinv [n_t, n_t].  At a pixel p, a_q(p) = sum_t Hinv[q][t] R_t[p].  The candidates are
the unmasked pixels that are finite in ALL planes; p* has the largest |a_0|, the lowest p on a tie; the
map stops with no candidate or |a_0(p*)| <= thresh; else c_q = gain a_q(p*), and for every plane t
R_t[x] -= sum_q c_q B_{t+q}[x - p* + centre] inside the beam window (a pixel that is non-finite in
plane t is left as it is in that plane and updated in the others).

`follow` keeps its own long-double planes, which it updates with the DEVICE's (pixel, c_0 .. c_{n_t-1}),
and checks for every component c = (p, c_0 ..):
    p is unmasked and finite in every plane of R_ref;
    max |a_0_ref| - |a_0_ref(p)| <= 2 A_0                          (it was a maximum)
    |c_q - gain a_q_ref(p)| <= gain A_q(p) + 2 u |gain a_q_ref(p)|  for every q
    |a_0_ref(p)| > thresh - A_0(p)                                  (it was above the threshold)
    no untouched candidate of lower index holds, plane by plane, exactly the input values of an
    untouched pick (both still hold their input bits in every plane, so the device's chains give
    the same a_0 for both: an exact tie, and the lower pixel must have won)
and at the end: ncomp < n_iter only if max |a_0_ref| <= thresh + A_0; every plane equals R_ref within
b_t per pixel, and its non-finite pixels hold their input bits; d_peak within A_0 + u max|a_0|; the
model planes equal the scatter of the list within ncomp u sum |c_t|; the slots beyond ncomp hold the
caller's poison.

The bounds, term by term (u = 2^-53).
  Update.  The device forms r = fma(-c_q, B_{t+q}, r) for q = 0 .. n_t - 1: n_t roundings per update
  of a pixel of plane t, each at most u times a partial result that never exceeds
      env_t[x] = |R0_t[x]| + sum_c sum_q |c_q| |B_{t+q}[x - p_c]|,
  so    b_t[x] = (updates of x so far) x n_t x roundings x u x env_t[x]
  (`roundings` = 1 with a fused multiply-add, 2 for a float64 emulation without one).  R_ref itself is
  rounded at 2^-64, 2048 times finer.
  Principal solution.  a_q = Hinv[q][0] R_0, then n_t - 1 fmas: n_t roundings, each at most u times a
  partial sum that never exceeds S_q[p] = sum_t |Hinv[q][t]| |R_t[p]|, on planes that are each within
  b_t of the reference's:
      A_q[p] = n_t x roundings x u x S_q[p] + sum_t |Hinv[q][t]| b_t[p],     A_0 = max over candidates.
  The pick compares two such values, hence 2 A_0.  c_q = fl(gain a_q) is one more rounding, u |c_q|
  (a second u is slack for the reference's own roundings).
`conservation` evaluates D_t = R_t + sum_c sum_q c_q B_{t+q}(. - p_c) on ALL planes from the list alone,
at the bound b_t."""
import numpy as np

from tests import clean_ref as C

LD = np.longdouble
U = 2.0 ** -53
TILE = C.TILE
MAX_NT = 4

MSG = {
    "null": "rjp_mtmfs: NULL planes, spectral beams, inverse Hessians, thresholds or component outputs",
    "sizes": "rjp_mtmfs: n_maps, n_t, nx, nz, px and pz must be positive",
    "nt": "rjp_mtmfs: n_t must not exceed RJP_MTMFS_MAX_NT (4)",
    "even": "rjp_mtmfs: px and pz must be odd (the beam's centre is a pixel)",
    "npsf": "rjp_mtmfs: n_psf must be 1 or n_maps",
    "npix": "rjp_mtmfs: nx * nz exceeds 2^31 - 1",
    "gain": "rjp_mtmfs: gain must lie in (0, 1]",
    "niter": "rjp_mtmfs: n_iter < 1",
    "thresh": "rjp_mtmfs: negative or non-finite threshold",
    "hinv": "rjp_mtmfs: non-finite h_hinv",
    "wgs": "rjp_mtmfs: more than 2^31 - 1 workgroups",
    "work": "rjp_mtmfs: workspace smaller than rjp_mtmfs_workspace()",
}


# ---- the tile rule, restated ---------------------------------------------------------------------------
def workgroups(n_maps, nx, nz):
    """One workgroup per map and tile of 1024 pixels: it holds all n_t planes of its tile."""
    return n_maps * ((nx * nz + TILE - 1) // TILE)


def workspace_bytes(n_maps, n_t, nx, nz):
    """Two halves of (n_t values f64, pixel i32) per map and tile, rounded up to 16 bytes."""
    return (workgroups(n_maps, nx, nz) * 2 * (8 * n_t + 4) + 15) // 16 * 16


def _cands(R, mask):
    """[nx, nz] bool: unmasked pixels that are finite in ALL planes."""
    ok = np.isfinite(R.astype(np.float64)).all(axis=0)
    return ok if mask is None else ok & (np.asarray(mask) != 0)


def solve(h_row, R, dtype=LD):
    """sum_t h_row[t] R[t] in the chain's order: one product, then one multiply-add per plane."""
    a = dtype(h_row[0]) * R[0]
    for t in range(1, len(h_row)):
        a = a + dtype(h_row[t]) * R[t]
    return a


# ---- the free-running clean (the reference in long double, the emulation in float64) ----------------------
def mtmfs(R0, B, hinv, mask, thresh, gain, n_iter, dtype=LD, beam_abs_diff=False, pick_r0=False,
          update_q0_only=False, gain_twice=False, hinv_row0=False):
    """Multi-term MFS CLEAN of the planes R0 [n_t, nx, nz] with the beams B [2 n_t - 1, px, pz] in
    `dtype` arithmetic -> (cpix, ccoef [n, n_t], planes).  dtype=LD is the free-running reference,
    float64 the emulation of the device (two roundings where the device has one fma).  The switches
    plant mistakes: `beam_abs_diff` = B_{|t-q|} for B_{t+q}; `pick_r0` = the pick made on |R_0|;
    `update_q0_only` = the update with the q = 0 term only; `gain_twice` = the coefficients carry the
    gain and the update applies it again; `hinv_row0` = row 0 of Hinv used for every a_q."""
    n_t, nx, nz = R0.shape
    px, pz = B.shape[1:]
    R = R0.astype(dtype).copy()
    Bd = B.astype(dtype)
    H = np.asarray(hinv, dtype=np.float64)
    cpix, ccoef = [], []
    with np.errstate(invalid="ignore"):
        for _ in range(n_iter):
            ok = _cands(R, mask)
            if not ok.any():
                break
            a0 = R[0] if pick_r0 else solve(H[0], R, dtype)
            key = np.where(ok, np.abs(a0), -np.inf).ravel()
            p = int(np.nonzero(key == key.max())[0][0])
            if not key.max() > thresh:
                break
            v = [R[t].ravel()[p] for t in range(n_t)]
            c = [dtype(gain) * solve(H[0 if hinv_row0 else q], v, dtype) for q in range(n_t)]
            cpix.append(p), ccoef.append(c)
            im, bm = C.window(nx, nz, px, pz, p // nz, p % nz)
            for t in range(n_t):
                r = R[t][im]
                fin = np.isfinite(r.astype(np.float64))
                for q in range(1 if update_q0_only else n_t):
                    f = c[q] * dtype(gain) if gain_twice else c[q]
                    r = np.where(fin, r - f * Bd[abs(t - q) if beam_abs_diff else t + q][bm], r)
                R[t][im] = r
    return (np.array(cpix, dtype=np.int64), np.array(ccoef, dtype=dtype).reshape(len(cpix), n_t), R)


# ---- the checker that follows the device -------------------------------------------------------------------
def follow(R0, B, hinv, mask, thresh, gain, n_iter, cpix, ccoef, ncomp, res, peak=None, model=None,
           model0=None, poison_pix=None, poison_coef=None, roundings=1):
    """Check what the device (or an emulation) made of the planes R0 [n_t, nx, nz]: see the module's
    docstring.  `cpix` [n_iter], `ccoef` [n_iter, n_t]: the map's full rows; `res` the planes on exit.
    Raises AssertionError naming the rule; -> dict of the worst error / bound per rule (`pick`, `coef`,
    `planes`, `peak`)."""
    n_t, nx, nz = R0.shape
    px, pz = B.shape[1:]
    assert B.shape[0] == 2 * n_t - 1
    ncomp = int(ncomp)
    assert 0 <= ncomp <= n_iter, ("ncomp", ncomp)
    res = np.asarray(res, dtype=np.float64).reshape(n_t, nx, nz)
    ccoef = np.asarray(ccoef, dtype=np.float64).reshape(-1, n_t)
    H = np.asarray(hinv, dtype=np.float64).reshape(n_t, n_t)
    absH = np.abs(H)
    R = R0.astype(LD).copy()
    fin0 = np.isfinite(R0)
    BL, absB = B.astype(LD), np.abs(B).astype(np.float64)
    env = np.abs(np.where(fin0, R0, 0.0)).astype(np.float64)
    cnt = np.zeros(R0.shape)
    g = LD(gain)
    worst = dict(pick=0.0, coef=0.0, planes=0.0, peak=0.0)

    def ratio(err, bnd, rule, key):
        err, bnd = float(err), float(bnd)
        assert err <= bnd, (rule, err, bnd)
        if bnd > 0:
            worst[key] = max(worst[key], err / bnd)

    def state():
        """candidates, b [n_t, nx, nz], A [n_t, nx, nz] (A[q] the bound of a_q), a_0, its max, max A_0"""
        ok = _cands(R, mask)
        b = cnt * n_t * roundings * U * env
        with np.errstate(invalid="ignore"):
            absR = np.abs(np.where(np.isfinite(R.astype(np.float64)), R, 0)).astype(np.float64)
            A = np.stack([n_t * roundings * U * np.tensordot(absH[q], absR, axes=1) +
                          np.tensordot(absH[q], b, axes=1) for q in range(n_t)])
            a0 = solve(H[0], R)
        if not ok.any():
            return ok, b, A, a0, 0.0, 0.0
        return ok, b, A, a0, float(np.abs(a0)[ok].max()), float(A[0][ok].max())

    for c in range(ncomp):
        p = int(cpix[c])
        ok, b, A, a0, top, A0 = state()
        assert 0 <= p < nx * nz and ok.ravel()[p], \
            ("component %d on a masked pixel or one that is not finite in every plane" % c, p)
        v = [R[t].ravel()[p] for t in range(n_t)]
        mine = float(abs(a0.ravel()[p]))
        ratio(top - mine, 2 * A0, "component %d is not a maximum of |a_0|" % c, "pick")
        for q in range(n_t):
            want = g * solve(H[q], v)
            ratio(abs(LD(ccoef[c, q]) - want), gain * float(A[q].ravel()[p]) + 2 * U * float(abs(want)),
                  "coefficient %d of component %d" % (q, c), "coef")
        assert mine > thresh - float(A[0].ravel()[p]), ("component %d below the threshold" % c, mine)
        if not cnt[:, p // nz, p % nz].any():
            # untouched pixels hold their input bits on the device too, in every plane: a candidate that
            # holds the pick's values plane by plane ties exactly, whatever the chain's roundings
            same = (R0 == R0[:, p // nz, p % nz][:, None, None]).all(axis=0)
            tie = (ok & (cnt == 0).all(axis=0) & same).ravel()
            assert not tie[:p].any(), ("component %d: a tie did not go to the lowest index" % c, p)
        im, bm = C.window(nx, nz, px, pz, p // nz, p % nz)
        for t in range(n_t):
            for q in range(n_t):
                R[t][im] = R[t][im] - LD(ccoef[c, q]) * BL[t + q][bm]
                env[t][im] += float(abs(ccoef[c, q])) * absB[t + q][bm]
            cnt[t][im] += 1
    ok, b, A, a0, top, A0 = state()
    if ncomp < n_iter:
        assert top <= thresh + A0, ("stopped above the threshold", top, thresh)
    assert np.array_equal(res[~fin0], R0[~fin0], equal_nan=True), "a non-finite pixel changed"
    with np.errstate(invalid="ignore"):
        err = np.abs(res.astype(LD) - R)[fin0].astype(np.float64)
    bf = b[fin0]
    assert np.all(err <= bf), ("residual planes", float((err - bf).max()))
    if (bf > 0).any():
        worst["planes"] = float((err[bf > 0] / bf[bf > 0]).max())
    if peak is not None:
        ratio(abs(float(peak) - top), A0 + U * top, "d_peak", "peak")
    if model is not None:
        want = (np.zeros(R0.shape) if model0 is None else model0).astype(LD).reshape(n_t, -1).copy()
        for c in range(ncomp):
            for t in range(n_t):
                want[t, int(cpix[c])] += LD(ccoef[c, t])
        tol = ncomp * U * float(np.abs(ccoef[:ncomp]).sum())
        if model0 is not None:
            tol += ncomp * U * float(np.abs(model0).max())
        assert np.all(np.abs(np.asarray(model).astype(LD).reshape(n_t, -1) - want) <= tol), "d_model"
    if poison_pix is not None:
        assert np.all(np.asarray(cpix[ncomp:]) == poison_pix), "a pixel slot beyond ncomp was written"
    if poison_coef is not None:
        tail = ccoef[ncomp:]
        assert np.array_equal(tail, np.full(tail.shape, poison_coef), equal_nan=True), \
            "a coefficient slot beyond ncomp was written"
    return worst


def conservation(R0, B, cpix, ccoef, ncomp, res, roundings=1):
    """D_t = R_t + sum_c sum_q c_q B_{t+q}(. - p_c) on every plane, in long double from the list alone
    (no pick is looked at) -> the worst error / bound over the pixels that were updated."""
    n_t, nx, nz = R0.shape
    px, pz = B.shape[1:]
    ccoef = np.asarray(ccoef, dtype=np.float64).reshape(-1, n_t)
    S = np.zeros(R0.shape, dtype=LD)
    env = np.abs(np.where(np.isfinite(R0), R0, 0.0)).astype(np.float64)
    cnt = np.zeros(R0.shape)
    BL, absB = B.astype(LD), np.abs(B)
    for c in range(int(ncomp)):
        p = int(cpix[c])
        im, bm = C.window(nx, nz, px, pz, p // nz, p % nz)
        for t in range(n_t):
            for q in range(n_t):
                S[t][im] += LD(ccoef[c, q]) * BL[t + q][bm]
                env[t][im] += float(abs(ccoef[c, q])) * absB[t + q][bm]
            cnt[t][im] += 1
    fin = np.isfinite(R0)
    with np.errstate(invalid="ignore"):
        err = np.abs(R0.astype(LD) - np.asarray(res, dtype=np.float64).reshape(R0.shape).astype(LD) - S)
    err = err[fin].astype(np.float64)
    b = (cnt * n_t * roundings * U * env)[fin]
    assert np.all(err <= b), ("conservation", float((err - b).max()))
    return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0


# ---- inputs --------------------------------------------------------------------------------------------
BAND_W = np.linspace(-0.1, 0.3, 8)            # w_f of eight channels, the reference frequency off-centre
                                               # (odd moments that are not zero: Hinv is a full matrix)


def band_weights(w, n):
    """[n, F]: row q = w^q, as imaging.taylor_weights forms them."""
    out = np.ones((n, len(w)))
    for q in range(1, n):
        out[q] = out[q - 1] * w
    return out


def channel_beams(rng, px, pz, w=BAND_W, n_vis=30):
    """The dirty beams [F, px, pz] of one random (u, v) coverage seen at the channels w_f, whose
    baselines in wavelengths scale with 1 + w_f: sinc-like, each exactly 1 at the centre."""
    jx = np.arange(px) - (px - 1) / 2
    jz = np.arange(pz) - (pz - 1) / 2
    a = rng.uniform(-0.2, 0.2, n_vis)
    b = rng.uniform(-0.2, 0.2, n_vis)
    out = np.empty((len(w), px, pz))
    for f, wf in enumerate(w):
        ph = 2 * np.pi * (1.0 + wf) * (a[:, None, None] * jx[None, :, None] + b[:, None, None] * jz[None, None, :])
        out[f] = np.cos(ph).mean(axis=0)
        out[f, (px - 1) // 2, (pz - 1) // 2] = 1.0
    return out


def spectral_beams(rng, n_t, px, pz, w=BAND_W, n_vis=30, tw=None, channels=None):
    """The spectral beams of `channel_beams` (or of `channels`) -> (B [2 n_t - 1, px, pz], H, Hinv).
    B_q = mean_f w_f^q beam_f, B_0 exactly 1 at the centre, B_q(centre) the q-th moment of the band;
    with n_t = 1, Hinv is exactly [[1.0]].  `tw`: other Taylor weights [2 n_t - 1, F] (a planted
    mistake)."""
    from rajepy_amd.imaging import taylor_hessian_inverse
    cb = channel_beams(rng, px, pz, w, n_vis) if channels is None else channels
    tw = band_weights(w, 2 * n_t - 1) if tw is None else tw
    B = np.tensordot(tw, cb, axes=1) / len(w)
    if np.all(tw[0] == 1.0):
        B[0, (px - 1) // 2, (pz - 1) // 2] = 1.0
    H, Hinv = taylor_hessian_inverse(B[:, (px - 1) // 2, (pz - 1) // 2])
    if n_t == 1:
        Hinv = np.array([[1.0]])
    return np.ascontiguousarray(B), H, Hinv


def taylor_planes(rng, nx, nz, B, n_t, sources=None, n_src=5, noise=1e-3):
    """Taylor dirty planes of a few point sources with spectra sum_q I_q w^q plus a smooth random
    field and continuous noise (near-ties have measure zero): R_t = sum_src sum_q I_q B_{t+q}(. - p)
    -> [n_t, nx, nz].  `sources`: (ix, iz, (I_0 .. I_{n_t-1})) to use instead of random ones."""
    px, pz = B.shape[1:]
    if sources is None:
        sources = []
        for _ in range(n_src):
            i0 = float(rng.uniform(0.3, 1.0)) * (1 if rng.random() < 0.8 else -1)
            coef = [i0] + [i0 * float(rng.uniform(-1.0, 1.0)) for _ in range(n_t - 1)]
            sources.append((int(rng.integers(nx)), int(rng.integers(nz)), coef))
    R = np.zeros((n_t, nx, nz))
    for ix, iz, coef in sources:
        im, bm = C.window(nx, nz, px, pz, ix, iz)
        for t in range(n_t):
            for q in range(n_t):
                R[t][im] += coef[q] * B[t + q][bm]
    x = np.arange(nx)[:, None] / max(nx, 2)
    z = np.arange(nz)[None, :] / max(nz, 2)
    top = max(np.abs(R[0]).max(), 1e-3)
    for t in range(n_t):
        smooth = np.sin(2 * np.pi * (x * rng.uniform(0.5, 2) + z * rng.uniform(0.5, 2) + rng.random()))
        R[t] += noise * top * (0.2 ** t) * (smooth + rng.standard_normal((nx, nz)))
    return np.ascontiguousarray(R)
