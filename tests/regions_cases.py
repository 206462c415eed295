"""The cases of K25 (rjp_image_stats, rjp_label_regions, rjp_mask_grow) that the CPU file
(tests/test_regions_reference_cpu.py: the device's algorithms emulated in plain Python) and the GPU
file (tests/test_gpu_regions.py: the kernels) share.  Everything is deterministic."""
import numpy as np

from tests import regions_ref as K

TX, TZ, H = K.TILE_X, K.TILE_Z, K.HALO


# ---- statistics -------------------------------------------------------------------------------------
# (nx, nz): 1 pixel .. 65 793 = 273 x 241 pixels -- every tail of a wave (63, 64, 65), of a workgroup
# (255 .. 257), of a tile of 2048 (2047 .. 2049) and 33 tiles per map
STAT_SHAPES = [(1, 1), (1, 2), (3, 1), (7, 9), (1, 64), (5, 13), (15, 17), (16, 16), (257, 1),
               (23, 89), (32, 64), (2049, 1), (273, 241)]


def _values(kind, n, rng):
    if kind == "normal":
        return rng.standard_normal(n)
    if kind == "equal":
        return np.full(n, 3.5)
    if kind == "ties":                        # a run of equal values across the median's rank
        x = np.sort(rng.integers(-3, 4, n).astype(np.float64))
        x[n // 4:3 * n // 4 + 1] = 1.0
        return rng.permutation(x)
    if kind in ("zeros_lo", "zeros_hi"):      # -0.0 | +0.0 with the boundary on either side of the rank
        r = (n - 1) // 2
        n_neg = max(0, r - 1) if kind == "zeros_lo" else r + 1      # values below +0.0
        x = np.full(n, 0.0)
        x[:n_neg] = -0.0
        x[:n_neg // 3] = -1.0
        x[n - (n - n_neg) // 3:] = 1.0
        return rng.permutation(x)
    if kind == "subnormal":
        return rng.integers(-40, 41, n).astype(np.float64) * 5e-324
    if kind == "huge":                        # beyond 2^+-500, both signs
        e = rng.integers(500, 600, n) * rng.choice([-1, 1], n)
        return rng.choice([-1.0, 1.0], n) * (1.0 + rng.random(n)) * 2.0 ** e.astype(np.float64)
    if kind == "negative":
        return -np.abs(rng.standard_normal(n)) - 0.5
    if kind == "nonfinite":
        x = rng.standard_normal(n)
        bad = rng.random(n) < 0.2
        x[bad] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum()))
        return x
    if kind == "nan":
        return np.full(n, np.nan)
    raise KeyError(kind)


STAT_KINDS = ["normal", "equal", "ties", "zeros_lo", "zeros_hi", "subnormal", "huge", "negative",
              "nonfinite"]
# mask kinds: none; one mask for all maps, inside / outside; one per map; one that selects nothing
STAT_MASKS = ["none", "shared_in", "shared_out", "per_map_in", "per_map_out", "nothing"]


def stat_case(shape, kind, mkind, n_maps, seed=0):
    """-> dict(img [M, npix], mask None | [n_mask, npix] uint8, inside, nx, nz).  With three maps the
    middle one is all NaN beside two live ones."""
    nx, nz = shape
    n = nx * nz
    rng = np.random.default_rng([seed, nx, nz, STAT_KINDS.index(kind), STAT_MASKS.index(mkind), n_maps])
    img = np.stack([_values("nan" if (n_maps == 3 and m == 1) else kind, n, rng) for m in range(n_maps)])
    mask, inside = None, True
    if mkind != "none":
        n_mask = n_maps if mkind.startswith("per_map") else 1
        inside = not mkind.endswith("_out")
        mask = (rng.random((n_mask, n)) < 0.4).astype(np.uint8) * rng.integers(1, 255, (n_mask, n)).astype(np.uint8)
        if mkind == "nothing":
            mask[:] = 0
    return dict(img=img, mask=mask, inside=inside, nx=nx, nz=nz)


def stat_cases():
    """(id, case): every value kind on a few sizes (odd and even counts) without a mask; every mask
    kind on normal and non-finite values; every size once."""
    out = []
    for kind in STAT_KINDS:
        for shape in [(5, 13), (16, 16), (23, 89), (2049, 1)]:
            out.append(("%s-%dx%d" % (kind, *shape), stat_case(shape, kind, "none", 1)))
    for mkind in STAT_MASKS[1:]:
        for kind in ("normal", "nonfinite"):
            out.append(("%s-%s-3maps" % (kind, mkind), stat_case((23, 89), kind, mkind, 3)))
    for shape in STAT_SHAPES:
        out.append(("normal-%dx%d-2maps" % shape, stat_case(shape, "normal", "none", 2)))
    out.append(("nonfinite-273x241-3maps", stat_case((273, 241), "nonfinite", "per_map_out", 3)))
    out.append(("ties-273x241", stat_case((273, 241), "ties", "none", 1)))
    return out


# ---- labels -------------------------------------------------------------------------------------------
# 1 x 1, 1 x N, N x 1, one tile, one tile plus a pixel either way, and >= 3 x 3 tiles twice
# (130 x 65 and 67 x 131 are the issue's; with the 16 x 64 tile they are 9 x 2 and 5 x 3 tiles, so 130 x 131,
# 9 x 3 tiles, is added: three tiles either way for every pattern of the big shapes)
LABEL_SHAPES = [(1, 1), (1, 37), (37, 1), (TX, TZ), (TX + 1, TZ), (TX, TZ + 1), (TX + 1, TZ + 1),
                (130, 65), (67, 131), (130, 131)]
BIG = [(130, 65), (67, 131), (130, 131)]


def serpentine(nx, nz):
    """Rows 0, 2, 4, ... full, joined alternately at the last and the first column: ONE region
    through every row -- the long equivalence chain."""
    m = np.zeros((nx, nz), dtype=np.uint8)
    m[0::2] = 1
    for k, ix in enumerate(range(1, nx, 2)):
        m[ix, nz - 1 if k % 2 == 0 else 0] = 1
    return m


def pattern(name, nx, nz, seed=0):
    rng = np.random.default_rng([seed, nx, nz])
    m = np.zeros((nx, nz), dtype=np.uint8)
    if name == "empty":
        pass
    elif name == "full":
        m[:] = 1
    elif name == "checker":
        m[(np.add.outer(np.arange(nx), np.arange(nz)) % 2) == 0] = 1
    elif name == "serpentine":
        m = serpentine(nx, nz)
    elif name == "corner":                   # two regions that touch only diagonally at a tile corner
        m[TX - 3:TX, TZ - 3:TZ] = 1
        m[TX:TX + 1, TZ:TZ + 1] = 1
    elif name == "u":                        # arms in one tile, joined only through the next tile
        m[3, 5:TZ + 7] = 1
        m[9, 5:TZ + 7] = 1
        m[3:10, TZ + 6] = 1
    elif name.startswith("random"):
        m = (rng.random((nx, nz)) < float(name[6:])).astype(np.uint8) * 7
    else:
        raise KeyError(name)
    return m.reshape(-1)


def label_cases():
    """(id, dict(mask [n_mask, npix], n_maps, nx, nz)), to be run at both connectivities."""
    out = []
    for nx, nz in LABEL_SHAPES:
        for name in ("empty", "full", "checker", "random0.5"):
            out.append(("%s-%dx%d" % (name, nx, nz), dict(mask=pattern(name, nx, nz)[None], n_maps=1, nx=nx, nz=nz)))
    for nx, nz in BIG:
        for d in ("0.1", "0.59", "0.9"):
            out.append(("random%s-%dx%d" % (d, nx, nz),
                        dict(mask=pattern("random" + d, nx, nz)[None], n_maps=1, nx=nx, nz=nz)))
    out.append(("serpentine-130x65", dict(mask=pattern("serpentine", 130, 65)[None], n_maps=1, nx=130, nz=65)))
    out.append(("serpentine-130x131", dict(mask=pattern("serpentine", 130, 131)[None], n_maps=1, nx=130, nz=131)))
    out.append(("corner-67x131", dict(mask=pattern("corner", 67, 131)[None], n_maps=1, nx=67, nz=131)))
    out.append(("u-67x131", dict(mask=pattern("u", 67, 131)[None], n_maps=1, nx=67, nz=131)))
    three = np.stack([pattern("random0.1", 67, 131, 1), pattern("random0.59", 67, 131, 2),
                      pattern("serpentine", 67, 131)])
    out.append(("3maps-67x131", dict(mask=three, n_maps=3, nx=67, nz=131)))
    out.append(("shared-3maps-67x131", dict(mask=three[1:2], n_maps=3, nx=67, nz=131)))
    return out


# ---- growth -------------------------------------------------------------------------------------------
GROW_ITERS = [0, 1, H - 1, H, H + 1, 75, -1]
GROW_SHAPES = LABEL_SHAPES                 # the same shapes: one tile exactly and a pixel more either way included


def corridor(nx, nz):
    """A one-pixel corridor along row 20 and down the last column (longer than 75 steps, across
    tile borders both ways), the seed at its first pixel."""
    c = np.zeros((nx, nz), dtype=np.uint8)
    c[20, :] = 1
    c[20:, nz - 1] = 1
    s = np.zeros((nx, nz), dtype=np.uint8)
    s[20, 0] = 1
    return s.reshape(-1), c.reshape(-1)


def grow_inputs(name, nx, nz, seed=0):
    rng = np.random.default_rng([seed, nx, nz, 5])
    n = nx * nz
    if name == "random":                    # sparse seeds, some of them outside the constraint
        con = (rng.random(n) < 0.7).astype(np.uint8) * 3
        s = (rng.random(n) < 0.02).astype(np.uint8) * 9
        s[0] = 1
        out = np.nonzero(con == 0)[0]
        if out.size:
            s[out[0]] = 1                    # a seed pixel outside the constraint: it stays
        return s, con
    if name == "empty":
        return np.zeros(n, dtype=np.uint8), (rng.random(n) < 0.7).astype(np.uint8)
    if name == "ones":
        s = np.zeros(n, dtype=np.uint8)
        s[n // 2] = 1
        return s, np.ones(n, dtype=np.uint8)
    if name == "corridor":
        return corridor(nx, nz)
    raise KeyError(name)


def grow_cases():
    """(id, dict(seed [M, npix], con [n_mask, npix], n_maps, nx, nz)), to be run at every n_iter of
    GROW_ITERS and both connectivities."""
    out = []
    for nx, nz in GROW_SHAPES:
        for name in ("random", "empty", "ones"):
            s, c = grow_inputs(name, nx, nz)
            out.append(("%s-%dx%d" % (name, nx, nz), dict(seed=s[None], con=c[None], n_maps=1, nx=nx, nz=nz)))
    for nx, nz in BIG:
        s, c = grow_inputs("corridor", nx, nz)
        out.append(("corridor-%dx%d" % (nx, nz), dict(seed=s[None], con=c[None], n_maps=1, nx=nx, nz=nz)))
    nx, nz = 67, 131
    seeds = np.stack([grow_inputs("random", nx, nz, k)[0] for k in range(3)])
    cons = np.stack([grow_inputs("random", nx, nz, k)[1] for k in range(3)])
    out.append(("3maps-67x131", dict(seed=seeds, con=cons, n_maps=3, nx=nx, nz=nz)))
    out.append(("shared-3maps-67x131", dict(seed=seeds, con=cons[:1], n_maps=3, nx=nx, nz=nz)))
    return out
