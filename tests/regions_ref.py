"""Reference for K25 (rjp_image_stats, rjp_label_regions, rjp_mask_grow; include/rjprt.h) and for
the automatic-mask convention built on them (rajepy_amd.imaging.automask_step): NumPy and
scipy.ndimage restatements of the definitions, plus plain-Python emulations of the device's own
algorithms (radix select, tile union-find with a border merge) and planted mistakes.

Everything but two numbers is held BIT FOR BIT: masks, labels, areas and counts are integers, and
min, max, median and MAD are elements of the input (the MAD of one correctly rounded subtraction).

The bound on `sum` and `sumsq` (any order).  The device adds the n counting values of a map in a
fixed tree; the test does not lean on which.  For ANY order of n - 1 floating-point additions of n
numbers, every input passes through at most n - 1 roundings, each a factor (1 + d), |d| <= u = 2^-53,
so |computed - exact| <= gamma_{n-1} sum |x_i| with gamma_k = k u / (1 - k u) (Higham, Accuracy and
Stability, section 4.2); additions cannot underflow.  For the squares the device forms fma(x, x, q):
the product is not rounded on its own, so the terms are the exact squares and each of the n fused
steps is one rounding of a sum (the first, from +0, included): gamma_n sum x_i^2.  A fused step whose
result is subnormal is rounded absolutely instead, by at most 2^-1075, so n 2^-1075 is added.  A
square sum beyond the largest double is +inf on the device and is judged as that.  The exact values
come from long double (64-bit significand here); their own error, gamma-like with u = 2^-64, is
added to the bound.  No part of the bound comes from a measurement."""
import math

import numpy as np
from scipy import ndimage

U53, U64 = 2.0 ** -53, 2.0 ** -64
TILE_X, TILE_Z = 16, 64          # the tile the emulation of the labelling uses (regions.hip's)
HALO = 8                         # RJP_GROW_HALO
STAT_TILE = 2048

MESSAGES = {
    "stats_null": "rjp_image_stats: NULL image or output",
    "stats_size": "rjp_image_stats: n_maps, nx and nz must be positive",
    "stats_maps": "rjp_image_stats: n_maps exceeds RJP_REGIONS_MAX_MAPS (65535)",
    "stats_nx": "rjp_image_stats: nx exceeds RJP_REGIONS_MAX_NX (1048560)",
    "stats_pix": "rjp_image_stats: nx * nz exceeds 2^31 - 1",
    "stats_nmask": "rjp_image_stats: n_mask must be 1 or n_maps",
    "stats_wgs": "rjp_image_stats: more than 2^31 - 1 workgroups",
    "stats_work": "rjp_image_stats: workspace smaller than rjp_image_stats_workspace()",
    "stats_align": "rjp_image_stats: d_work is not 8-byte aligned",
    "label_null": "rjp_label_regions: NULL mask or outputs",
    "label_size": "rjp_label_regions: n_maps, nx and nz must be positive",
    "label_maps": "rjp_label_regions: n_maps exceeds RJP_REGIONS_MAX_MAPS (65535)",
    "label_nx": "rjp_label_regions: nx exceeds RJP_REGIONS_MAX_NX (1048560)",
    "label_pix": "rjp_label_regions: nx * nz exceeds 2^31 - 1",
    "label_nmask": "rjp_label_regions: n_mask must be 1 or n_maps",
    "label_conn": "rjp_label_regions: connectivity must be 1 (four neighbours) or 2 (eight)",
    "label_work": "rjp_label_regions: workspace smaller than rjp_label_regions_workspace()",
    "label_align": "rjp_label_regions: d_work is not 8-byte aligned",
    "grow_null": "rjp_mask_grow: NULL seed or constraint",
    "grow_size": "rjp_mask_grow: n_maps, nx and nz must be positive",
    "grow_maps": "rjp_mask_grow: n_maps exceeds RJP_REGIONS_MAX_MAPS (65535)",
    "grow_nx": "rjp_mask_grow: nx exceeds RJP_REGIONS_MAX_NX (1048560)",
    "grow_pix": "rjp_mask_grow: nx * nz exceeds 2^31 - 1",
    "grow_nmask": "rjp_mask_grow: n_mask must be 1 or n_maps",
    "grow_conn": "rjp_mask_grow: connectivity must be 1 (four neighbours) or 2 (eight)",
    "grow_work": "rjp_mask_grow: workspace smaller than rjp_mask_grow_workspace()",
    "grow_align": "rjp_mask_grow: d_work is not 8-byte aligned",
}


def stats_workspace(n_maps, nx, nz):
    tiles = (nx * nz + STAT_TILE - 1) // STAT_TILE
    return n_maps * (32 + 2048 * 4 + tiles * 48)


def label_workspace(n_maps, nx, nz):
    return 256 + 2 * n_maps * nx * nz * 4


def grow_workspace(n_maps, nx, nz):
    return 256 + (n_maps * nx * nz + 7) // 8 * 8 + 3 * n_maps * nx * nz * 4


def stats_workgroups(n_maps, nx, nz):
    return n_maps * ((nx * nz + STAT_TILE - 1) // STAT_TILE)


def region_workgroups(n_maps, nx, nz):
    return n_maps * ((nx + TILE_X - 1) // TILE_X) * ((nz + TILE_Z - 1) // TILE_Z)


# ---- statistics -----------------------------------------------------------------------------------
def keys(x):
    """The order-preserving uint64 key of float64 values: IEEE total order, -0.0 < +0.0."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def values(k):
    k = np.asarray(k, dtype=np.uint64)
    b = np.where(k >> np.uint64(63) != 0, k & np.uint64((1 << 63) - 1), ~k)
    return b.view(np.float64)


def selected(img, mask, inside):
    """(counting pixels, selected non-finite pixels) of one map."""
    img = np.asarray(img, dtype=np.float64).ravel()
    sel = np.ones(img.size, dtype=bool) if mask is None else \
        ((np.asarray(mask).ravel() != 0) == bool(inside))
    fin = np.isfinite(img)
    return sel & fin, sel & ~fin


def rank_element(x, upper=False):
    """The element of rank (n - 1) / 2 of x in the total order (`upper`: n / 2, a planted mistake),
    by np.partition on the keys."""
    k = keys(x)
    r = k.size // 2 if upper else (k.size - 1) // 2
    return float(values(np.partition(k, r)[r:r + 1])[0])


def image_stats(img, mask=None, inside=True, upper=False, mad_of_abs=False):
    """One map -> dict(count, n_nonfinite, min, max, median, mad as float64; sum, sumsq, abs_sum as
    long double).  `upper`, `mad_of_abs`: planted mistakes."""
    img = np.asarray(img, dtype=np.float64).ravel()
    cnt, bad = selected(img, mask, inside)
    x = img[cnt]
    out = dict(count=float(x.size), n_nonfinite=float(bad.sum()))
    if x.size == 0:
        out.update(min=np.nan, max=np.nan, median=np.nan, mad=np.nan, sum=np.longdouble(0),
                   sumsq=np.longdouble(0), abs_sum=np.longdouble(0))
        return out
    k = keys(x)
    out["min"] = float(values(k.min().reshape(1))[0])
    out["max"] = float(values(k.max().reshape(1))[0])
    med = rank_element(x, upper)
    with np.errstate(over="ignore"):
        dev = np.abs(x) if mad_of_abs else np.abs(x - med)
    out["median"], out["mad"] = med, rank_element(dev, upper)
    xl = x.astype(np.longdouble)
    out["sum"], out["sumsq"], out["abs_sum"] = xl.sum(), (xl * xl).sum(), np.abs(xl).sum()
    return out


def sum_bounds(ref):
    """(bound on |sum - exact|, bound on |sumsq - exact|) by the docstring's argument."""
    n = int(ref["count"])
    if n == 0:
        return 0.0, 0.0

    def gamma(k, u):
        return k * u / (1.0 - k * u)
    b_sum = (gamma(max(n - 1, 0), U53) + gamma(n, U64)) * float(ref["abs_sum"])
    b_sq = (gamma(n, U53) + gamma(2 * n, U64)) * float(ref["sumsq"]) + n * 2.0 ** -1075
    return b_sum, b_sq


def radix_select(x):
    """The device's selection in plain NumPy: six digits of 11, 11, 11, 11, 11, 9 bits of the key
    from the top; per digit a histogram of the values whose higher bits equal the prefix, the bin
    that holds the rank, the rank reduced.  -> the lower median of x (x non-empty)."""
    k = keys(x)
    rank, prefix = (k.size - 1) // 2, 0
    for p in range(6):
        shift, bits = (53 - 11 * p, 11) if p < 5 else (0, 9)
        live = k if p == 0 else k[(k >> np.uint64(shift + bits)) == np.uint64(prefix)]
        h = np.bincount(((live >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int64),
                        minlength=1 << bits)
        c = np.cumsum(h)
        d = int(np.searchsorted(c, rank, side="right"))
        rank -= int(c[d - 1]) if d else 0
        prefix = (prefix << bits) | d
    return float(values(np.array([prefix], dtype=np.uint64))[0])


def emulate_stats(img, mask=None, inside=True):
    """median and MAD as the device selects them."""
    img = np.asarray(img, dtype=np.float64).ravel()
    cnt, _ = selected(img, mask, inside)
    x = img[cnt]
    if x.size == 0:
        return np.nan, np.nan
    med = radix_select(x)
    with np.errstate(over="ignore"):
        return med, radix_select(np.abs(x - med))


# ---- labels -----------------------------------------------------------------------------------------
def structure(connectivity):
    return ndimage.generate_binary_structure(2, int(connectivity))


def label_regions(mask, nx, nz, connectivity, first_found=False):
    """One mask -> (label int32 [nx nz]: 0 or 1 + the smallest pixel index of the region, area int32,
    n_regions).  `first_found`: scipy's own numbering, a planted mistake."""
    m = (np.asarray(mask).reshape(nx, nz) != 0)
    lab, n = ndimage.label(m, structure=structure(connectivity))
    lab = lab.ravel()
    if first_found:
        return lab.astype(np.int32), np.bincount(lab, minlength=n + 1)[lab].astype(np.int32) * (lab > 0), n
    idx = np.arange(nx * nz)
    first = np.full(n + 1, nx * nz, dtype=np.int64)
    np.minimum.at(first, lab, idx)
    first[0] = -1
    count = np.bincount(lab, minlength=n + 1)
    count[0] = 0
    return (first[lab] + 1).astype(np.int32), count[lab].astype(np.int32), n


def emulate_labels(mask, nx, nz, connectivity, tx=TILE_X, tz=TILE_Z):
    """The device's algorithm in plain Python: union-find inside every tx x tz tile on local
    indices, the local roots written as global parents, then the unions of the backward neighbours
    that lie in other tiles, then a flatten -> label int32 [nx nz]."""
    m = (np.asarray(mask).reshape(nx, nz) != 0)
    par = np.full(nx * nz, -1, dtype=np.int64)

    def find(p, i):
        while p[i] != i:
            i = p[i]
        return i

    def union(p, a, b):
        a, b = find(p, a), find(p, b)
        if a != b:
            p[max(a, b)] = min(a, b)

    back = [(0, -1), (-1, 0)] + ([(-1, -1), (-1, 1)] if connectivity == 2 else [])
    for x0 in range(0, nx, tx):
        for z0 in range(0, nz, tz):
            loc = np.full(tx * tz, -1, dtype=np.int64)
            for lx in range(min(tx, nx - x0)):
                for lz in range(min(tz, nz - z0)):
                    if m[x0 + lx, z0 + lz]:
                        loc[lx * tz + lz] = lx * tz + lz
            for l in np.nonzero(loc >= 0)[0]:
                lx, lz = divmod(int(l), tz)
                for dx, dz in back:
                    ax, az = lx + dx, lz + dz
                    if 0 <= ax < tx and 0 <= az < tz and loc[ax * tz + az] >= 0:
                        union(loc, int(l), ax * tz + az)
            for l in np.nonzero(loc >= 0)[0]:
                r = find(loc, int(l))
                lx, lz = divmod(int(l), tz)
                par[(x0 + lx) * nz + z0 + lz] = (x0 + r // tz) * nz + z0 + r % tz
    for p in np.nonzero(par >= 0)[0]:
        ix, iz = divmod(int(p), nz)
        for dx, dz in back:
            ax, az = ix + dx, iz + dz
            if 0 <= ax < nx and 0 <= az < nz and par[ax * nz + az] >= 0 and \
                    (ax // tx, az // tz) != (ix // tx, iz // tz):
                union(par, int(p), ax * nz + az)
    out = np.zeros(nx * nz, dtype=np.int32)
    for p in np.nonzero(par >= 0)[0]:
        out[p] = find(par, int(p)) + 1
    return out


# ---- growth -----------------------------------------------------------------------------------------
def mask_grow(seed, constraint, nx, nz, n_iter, connectivity, unconstrained=False, extra=0,
              drop_outside=False):
    """n_iter steps of seed | (dilate(seed) & constraint) -> bool [nx nz]; 0: the seed; < 0: until
    stable.  `unconstrained`, `extra` (steps too many), `drop_outside`: planted mistakes."""
    s = (np.asarray(seed).reshape(nx, nz) != 0)
    c = (np.asarray(constraint).reshape(nx, nz) != 0)
    if drop_outside:
        s = s & c
    if n_iter == 0:
        return s.ravel().copy()
    it = 0 if n_iter < 0 else n_iter + extra
    return ndimage.binary_dilation(s, structure=structure(connectivity), iterations=it,
                                   mask=None if unconstrained else c).ravel()


# ---- the automatic mask, restated from the convention ------------------------------------------------
DEFAULTS = dict(sidelobe_threshold=3.0, noise_threshold=5.0, low_noise_threshold=1.5,
                min_beam_frac=0.3, grow_iterations=75, connectivity=1, nsigma=0.0)


def automask_step(R, prev, user_mask, sidelobe, abc, opts, ni, nj):
    """One update of the masks of a stack R [M, ni nj] (host arrays) -> (masks bool [M, ni nj],
    info: one dict per map).  `prev` [M, ni nj] bool, `user_mask` [ni nj] bool or None, `sidelobe`
    [M], `abc` [M][3] the clean beams' quadratic forms, `opts` the full option dict."""
    R = np.asarray(R, dtype=np.float64)
    M = R.shape[0]
    masks, info = np.zeros((M, ni * nj), dtype=bool), []
    for m in range(M):
        st = image_stats(R[m], prev[m], inside=False)
        if st["count"] == 0:
            st = image_stats(R[m])
        median, sigma = st["median"], 1.4826 * st["mad"]
        peak = image_stats(R[m])["max"]
        t_noise = median + opts["noise_threshold"] * sigma
        t_side = opts["sidelobe_threshold"] * float(sidelobe[m]) * peak
        T = max(t_side, t_noise)
        T_low = min(T, median + opts["low_noise_threshold"] * sigma)
        fin = np.isfinite(R[m])
        um = np.ones(ni * nj, dtype=bool) if user_mask is None else np.asarray(user_mask).ravel() != 0
        with np.errstate(invalid="ignore"):
            seed = fin & (R[m] > T) & um
            con = fin & (R[m] > T_low) & um
        A, B, C = (float(v) for v in abc[m])
        omega = math.pi / math.sqrt(A * C - B * B)
        min_pixels = max(1, int(math.ceil(opts["min_beam_frac"] * omega)))
        lab, area, n_regions = label_regions(seed, ni, nj, opts["connectivity"])
        kept = seed & (area >= min_pixels)
        n_kept = int(np.unique(lab[kept]).size)
        grown = mask_grow(kept, con, ni, nj, opts["grow_iterations"], opts["connectivity"])
        masks[m] = prev[m] | grown
        info.append(dict(median=median, sigma=sigma, peak=peak, T=T, T_low=T_low,
                         n_regions=int(n_regions), n_kept=n_kept, n_seed=int(seed.sum()),
                         n_mask=int(masks[m].sum())))
    return masks, info
