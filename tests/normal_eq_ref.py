"""Reference for rjp_normal_eq (K23): a NumPy restatement of the definition in include/rjprt.h in
numpy.longdouble, with DERIVED bounds, and the cases tests/test_gpu_normal_eq.py runs (which
tests/test_normal_eq_reference_cpu.py holds a float64 emulation and planted mistakes to first).
Shares nothing with the kernel: plain sums over whole arrays, no tiles.

Definition.  data, model [n_rows, n_vis] complex (n_part = 2) or real (n_part = 1), dmodel [n_rows,
n_par, n_vis], sel [P], w None, [n_vis] or [n_rows, n_vis].  A sample counts when every part of its
datum and its weight are finite and w > 0.  Over the counting samples, with r = data - model and
J_p = dmodel[:, sel[p]]:
    chi2 = sum w |r|^2,   g_p = sum w Re(conj(J_p) r),   N_pq = sum w Re(conj(J_p) J_q)   (p <= q)
and count their number.  Written over real parts -- Re(conj(a) b) = ar br + ai bi -- every entry is
a sum of m = n_part n real terms w a b (n = count).

The bound (derived, not measured).  Let u = 2^-53.  The device forms every term as one rounded
product w b times a inside a fused multiply-add, and adds the terms in some order (slices, tiles:
any order will do for what follows).  A sum of m non-zero terms, however it is bracketed, passes
each term through at most m - 1 inexact additions (adding an exact 0 -- a sample that does not
count, an empty slice or tile -- is exact), and the product w b costs one more rounding, so the
computed entry is sum_i t_i (1 + e_i) with |e_i| <= (1 + u)^m - 1.  For m u << 1 that is below
(m + 1) u; the bound used is
    |N_pq - exact| <= (m + 4) u sum w (|Jr_p Jr_q| + |Ji_p Ji_q|),
the 4 covering the second-order terms (and an emulation without FMA, which rounds a (w b) once
more).  For g and chi2 the residual itself is rounded, r = fl(y - m) = (y - m)(1 + d), |d| <= u per
part -- the exact sums are defined with the exact y - m -- which adds u |y - m| per factor of r:
    |g_p - exact|  <= (m + 5) u sum w (|Jr_p| |yr - mr| + |Ji_p| |yi - mi|)
    |chi2 - exact| <= (m + 6) u sum w |y - m|^2.
The long-double sums below carry an error of their own of at most m eps_LD times the same sums
(eps_LD = 2^-63 where long double is wider), which is added to each bound.  An entry whose exact
terms contain a NaN is NaN on both sides (`nan` flags it) and is compared as such.
"""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53
EPS_LD = float(np.finfo(LD).eps)
TILE = 512                     # samples per workgroup of the first launch (include/rjprt.h)
MAX_SEL = 48

MSG = {
    "null": "rjp_normal_eq: NULL data, model or outputs",
    "count": "rjp_normal_eq: n_rows and n_vis must be positive",
    "part": "rjp_normal_eq: n_part must be 1 (real) or 2 (complex)",
    "nsel": "rjp_normal_eq: n_sel must lie in 0 .. RJP_NORMAL_EQ_MAX_SEL (48)",
    "needs": "rjp_normal_eq: NULL derivatives or selection with n_sel > 0",
    "npar": "rjp_normal_eq: n_par < n_sel",
    "range": "rjp_normal_eq: h_sel outside 0 .. n_par - 1",
    "repeat": "rjp_normal_eq: h_sel repeats an index",
    "wrows": "rjp_normal_eq: w_rows must be 1 or n_rows",
    "wgs": "rjp_normal_eq: more than 2^31 - 1 workgroups",
    "work": "rjp_normal_eq: workspace smaller than rjp_normal_eq_workspace()",
}


def workgroups(n_rows, n_vis):
    """The return value: tiles of TILE consecutive flattened samples."""
    return (n_rows * n_vis + TILE - 1) // TILE


def n_out(P):
    return 1 + P + P * (P + 1) // 2


def workspace_bytes(n_rows, n_vis, P):
    return workgroups(n_rows, n_vis) * (n_out(P) + 1) * 8


def tri_list(P):
    return [(i, j) for i in range(P) for j in range(i, P)]


def _parts(z, n_part, T):
    """[..., n_part] real parts of a complex or real array in dtype T."""
    z = np.asarray(z)
    if n_part == 2:
        return np.stack([z.real.astype(T), z.imag.astype(T)], axis=-1)
    return z.astype(T)[..., None]


def counting(data, w, n_part):
    d = _parts(data, n_part, np.float64)
    ok = np.all(np.isfinite(d), axis=-1)
    if w is not None:
        wf = np.broadcast_to(np.asarray(w, dtype=np.float64), ok.shape)
        ok = ok & np.isfinite(wf) & (wf > 0)
    return ok


def sums(data, model, dmodel, sel, w, n_part, T=LD, mistake=None):
    """-> dict(chi2, g [P], N [P (P + 1) / 2], count) in dtype T, and with T = LD the sums of the
    absolute terms a_chi2, a_g, a_N the bounds are built from.  `mistake`: a planted one."""
    sel = [int(s) for s in sel]
    P = len(sel)
    ok = counting(data, w, n_part)                                    # [R, K]
    wf = np.ones(ok.shape) if w is None else np.broadcast_to(np.asarray(w, dtype=np.float64), ok.shape)
    wt = np.where(ok, wf, 0.0).astype(T)
    if mistake == "w_squared":
        wt = wt * wt
    y, m = _parts(data, n_part, T), _parts(model, n_part, T)
    with np.errstate(all="ignore"):
        r = np.where(ok[..., None], y - m, 0)                          # [R, K, part]
        if T is not LD:
            r = r.astype(np.float64)
        planes = list(range(P)) if mistake == "ignore_sel" else sel
        if P:
            J = _parts(np.asarray(dmodel)[:, planes], n_part, T)        # [R, P, K, part]
            keep = ok if mistake != "add_noncounting" else np.ones_like(ok)
            J = np.where(keep[:, None, :, None], J, 0)
        else:
            J = np.zeros((ok.shape[0], 0, ok.shape[1], n_part), dtype=T)
        if mistake == "drop_imag" and n_part == 2:
            J, r = J.copy(), r.copy()
            J[..., 1] = 0
            r[..., 1] = 0
        wJ = wt[:, None, :, None] * J if mistake != "add_noncounting" else \
            np.where(ok, wt, 1.0).astype(T)[:, None, :, None] * J
        wr = wt[..., None] * r
        sign = np.ones(n_part, dtype=T)
        if mistake == "no_conj" and n_part == 2:
            sign[1] = -1                                               # Re(J_p J_q): ar br - ai bi
        out = dict(count=int(ok.sum()))
        out["chi2"] = np.sum(r * wr, dtype=T)
        out["g"] = np.array([np.sum(J[:, p] * wr * sign, dtype=T) for p in range(P)], dtype=T)
        out["N"] = np.array([np.sum(J[:, p] * wJ[:, q] * sign, dtype=T) for p, q in tri_list(P)], dtype=T)
        if T is LD and mistake is None:
            out["a_chi2"] = np.sum(np.abs(r * wr), dtype=T)
            out["a_g"] = np.array([np.sum(np.abs(J[:, p] * wr), dtype=T) for p in range(P)], dtype=T)
            out["a_N"] = np.array([np.sum(np.abs(J[:, p] * wJ[:, q]), dtype=T) for p, q in tri_list(P)],
                                  dtype=T)
    return out


def reference(case):
    return sums(case["data"], case["model"], case["dmodel"], case["sel"], case["w"], case["n_part"])


def emulate(case, mistake=None):
    """The same sums in float64 (no FMA, NumPy's own order): what the bound must admit."""
    return sums(case["data"], case["model"], case["dmodel"], case["sel"], case["w"], case["n_part"],
                T=np.float64, mistake=mistake)


def bounds(ref, n_part):
    m = n_part * ref["count"]
    own = m * EPS_LD if EPS_LD < 2 * U53 else 0.0
    return dict(chi2=((m + 6) * U53 + own) * ref["a_chi2"], g=((m + 5) * U53 + own) * ref["a_g"],
                N=((m + 4) * U53 + own) * ref["a_N"])


def judge(got, ref, n_part, extra=None):
    """The worst |got - ref| / bound over chi2, g and N (0 / 0 = 0; a NaN on one side alone = inf);
    the count must be exact.  `extra`: dict of additional absolute allowances per key."""
    assert int(got["count"]) == ref["count"], (got["count"], ref["count"])
    b = bounds(ref, n_part)
    worst = 0.0
    for key in ("chi2", "g", "N"):
        x = np.atleast_1d(np.asarray(got[key], dtype=LD))
        y = np.atleast_1d(np.asarray(ref[key], dtype=LD))
        lim = np.atleast_1d(np.asarray(b[key], dtype=LD))
        if extra is not None:
            lim = lim + np.atleast_1d(np.asarray(extra[key], dtype=LD))
        assert x.shape == y.shape, (key, x.shape, y.shape)
        nx, ny = np.isnan(x), np.isnan(y)
        if np.any(nx != ny):
            return float("inf")
        with np.errstate(all="ignore"):
            err = np.abs(np.where(ny, 0, x - y))
            ratio = np.where(err == 0, 0, err / lim)
        if ratio.size:
            worst = max(worst, float(np.max(np.where(ny, 0, ratio))))
    return worst


# ---- the cases of the GPU test ---------------------------------------------------------------------
# (n_rows, n_vis, n_part, n_sel, n_par, weights): n_vis of 1, a tile - 1, a tile, a tile + 1, three
# tiles and a tail; every n_sel at which the kernel changes its instantiation (7 | 8, 15 | 16, 31 |
# 32) on a small stack
SIZED = [
    (1, 1, 1, 0, 0, "none"), (5, 1, 1, 3, 9, "rows"), (2, 511, 2, 1, 4, "shared"),
    (1, 512, 2, 17, 20, "none"), (3, 513, 2, 47, 48, "rows"), (2, 1573, 2, 48, 50, "shared"),
    (4, 1573, 1, 3, 6, "rows"), (3, 512, 1, 17, 18, "none"), (5, 513, 2, 0, 3, "shared"),
    (2, 511, 1, 48, 48, "rows"), (1, 1573, 2, 3, 9, "none"),
    (2, 40, 2, 7, 9, "rows"), (2, 40, 2, 8, 9, "shared"), (2, 40, 1, 15, 33, "none"),
    (2, 40, 2, 16, 33, "rows"), (2, 40, 2, 31, 33, "shared"), (2, 40, 1, 32, 33, "rows"),
]


def sized(n_rows, n_vis, n_part, n_sel, n_par, wkind, seed=20261021):
    """A case with everything the definition speaks of: weights with zeros, negatives, NaN and inf;
    NaN and inf data; NaN derivatives (and model) in every sample that does not count; from three
    rows on a row with nothing counting; `sel` a random choice of planes in random order."""
    rng = np.random.default_rng([seed, n_rows, n_vis, n_part, n_sel, n_par])
    shape = (n_rows, n_vis)

    def draw(*s):
        a = rng.standard_normal(s)
        return a + 1j * rng.standard_normal(s) if n_part == 2 else a

    model = draw(*shape)
    data = model + 0.1 * draw(*shape)
    dmodel = draw(n_rows, n_par, n_vis) * (10.0 ** rng.uniform(-3, 3, size=(1, n_par, 1))) if n_par else None
    w = None
    if wkind != "none":
        w = rng.uniform(0.5, 2.0, size=shape if wkind == "rows" else (n_vis,))
        bad = rng.random(w.shape) < 0.15
        w[bad] = rng.choice([0.0, -1.0, np.nan, np.inf, -np.inf], size=int(bad.sum()))
    bad = rng.random(shape) < 0.1
    vals = rng.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
    if n_part == 2:
        with np.errstate(invalid="ignore"):
            vals = np.where(rng.random(vals.size) < 0.5, vals + 0j, 1j * vals + 1.0)
    data[bad] = vals
    if n_rows >= 3:
        data[1] = np.nan
    sel = rng.permutation(n_par)[:n_sel].astype(np.int32)
    case = dict(data=data, model=model, dmodel=dmodel, sel=sel, w=w, n_part=n_part, n_par=n_par)
    dead = ~counting(data, w, n_part)
    model[dead] = np.nan
    if n_par:
        dmodel[np.broadcast_to(dead[:, None, :], dmodel.shape)] = np.nan
    return case


def nan_plane(seed=7):
    """One counting sample with a NaN derivative in plane sel[2]: exactly the entries that touch
    that plane are NaN.  -> (case, j)"""
    case = sized(2, 600, 2, 5, 8, "shared", seed)
    ok = counting(case["data"], case["w"], 2)
    r, k = np.argwhere(ok)[len(np.argwhere(ok)) // 2]
    case["dmodel"][r, case["sel"][2], k] = np.nan
    return case, 2


def touches(P, j):
    """Which entries of g [P] and N [T] involve plane j."""
    return (np.arange(P) == j, np.array([j in pq for pq in tri_list(P)]))
