"""The reference of rjp_uv_tracks and rjp_vis_noise (K16): the contract of include/rjprt.h restated
on the host, in Python integers (Philox4x32-10) and np.longdouble (everything that rounds).

BOUNDS (u = 2^-53), derived from the operations the header states, not from what the kernels give.

Tracks, per component, with B = |bx| + |by| + |bz|, b = xyz_j - xyz_i:
  1. the three differences are float64 subtractions: relative error u each, and every coefficient
     that multiplies them (sinG, cosG, sin_dec, cos_dec and their products) is at most 1: <= 1 u B;
  2. sinG, cosG come from the library's sine / cosine of an argument in turns.  The hour angle is
     reduced exactly (g - rint(g) is exact in float64), the truncation of the two polynomials is
     stated in rjp_device.h (< 2e-14 and < 1e-15: SINCOS_TRUNC = 2.01e-14 covers both) and its own
     roundings are the 6 u of tests/vis_ref.py: <= (2.01e-14 + 6 u) B;
  3. products and sums: u takes one product and one FMA (2 roundings), v and w one product, two
     FMAs and one more product (4 roundings), each of a value that is at most B: <= 4 u B.
  sum: (C_T u + 2.1e-14) B with C_T = 1 + 6 + 4 = 11, taken as 12.
Noise, per part, with a = sigma s_k r:
  1. u1, u2 are exact (53-bit odd integers times 2^-53);
  2. log: the HIP math API documents 1 ULP for the double-precision log
     (ROCm documentation, "HIP math API", double-precision mathematical functions) = 2 u relative;
     the factor -2 is exact and the square root halves it: 1 u on r;
  3. sqrt: the same table documents 1 ULP = 2 u;
  4. sigma s_k and (sigma s_k) r: two products, 2 u;
  5. sine / cosine as above: 6 u and the truncation 2.01e-14, absolute, times a;
  6. the final FMA rounds the sum once: u |out|.
  sum: |out - ref| <= u |ref| + a (C_N u + 2.1e-14), C_N = 1 + 2 + 2 + 6 = 11, taken as 12.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SINCOS_TRUNC = 2.1e-14
C_T = 12
C_N = 12
PI_LD = LD(4) * np.arctan(LD(1))

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

# the seed of the statistics (CPU) and of the GPU tests: every 5-sigma condition of
# test_observe_reference_cpu.py holds for the reference's own 2^20 normals at this seed
SEED = 20240516

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

TRACKS_MESSAGES = {
    "null": "rjp_uv_tracks: NULL positions, hour angles or outputs",
    "n_ant": "rjp_uv_tracks: n_ant < 2",
    "n_t": "rjp_uv_tracks: n_t < 1",
    "xyz": "rjp_uv_tracks: non-finite h_xyz",
    "dec": "rjp_uv_tracks: non-finite sin_dec / cos_dec",
    "unit": "rjp_uv_tracks: sin_dec^2 + cos_dec^2 differs from 1 by more than 1e-12",
    "size": "rjp_uv_tracks: n_t * n_bl exceeds 2^31 - 1",
}
NOISE_MESSAGES = {
    "null": "rjp_vis_noise: NULL visibilities, sigmas or output",
    "sizes": "rjp_vis_noise: n_maps and n_vis must be positive",
    "sigma": "rjp_vis_noise: negative or non-finite h_sigma",
    "k0": "rjp_vis_noise: k0 must be >= 0 and k0 + n_vis at most 2^63 - 1",
    "m0": "rjp_vis_noise: m0 must be >= 0 and m0 + n_maps at most 2^31 - 1",
}


# ---- Philox4x32-10 ---------------------------------------------------------------------------------
def philox_int(counter, key):
    """Philox4x32-10 in Python integers -> the four output words."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_np(c0, c1, c2, c3, k0, k1):
    """The same on uint64 arrays that hold 32-bit words (every product fits 64 bits)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in
                      np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & MASK), np.uint64(int(k1) & MASK)
    m, s = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ k0, p1 & m, (p0 >> s) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return c0, c1, c2, c3


def counter_words(seed, k, m, carry=True, swap=False):
    """(c0, c1, c2, c3, key0, key1) of visibility index `k` (k0 + k, Python ints or an int array
    below 2^63) and map index `m` (m0 + m).  `carry=False`, `swap=True`: planted mistakes."""
    k = np.asarray(k, dtype=np.uint64)
    m = np.asarray(m, dtype=np.uint64)
    lo, hi = k & np.uint64(MASK), k >> np.uint64(32)
    if not carry:                       # the second word forgets what the first overflowed into
        hi = np.zeros_like(hi) + (np.uint64(int(np.min(k))) >> np.uint64(32))
    if swap:
        return m, np.zeros_like(m), lo, np.zeros_like(lo), seed & MASK, (seed >> 32) & MASK
    return lo, hi, m, np.zeros_like(m), seed & MASK, (seed >> 32) & MASK


def unit_int(hi, lo):
    """The 53-bit odd integer 2 n + 1 of n = (hi << 20) | (lo >> 12)."""
    return 2 * ((int(hi) << 20) | (int(lo) >> 12)) + 1


def unit_ld(hi, lo):
    """u = (2 n + 1) 2^-53 as longdouble (exact: 53 bits), from uint64 arrays of 32-bit words."""
    n = (np.asarray(hi, dtype=np.uint64) << np.uint64(20)) | (np.asarray(lo, dtype=np.uint64) >> np.uint64(12))
    return (LD(2) * n.astype(LD) + LD(1)) * LD(2.0 ** -53)


def normals(seed, k, m, carry=True, swap=False, swap_trig=False):
    """(r, g1, g2) in longdouble of the visibilities `k` (absolute indices) of map `m`."""
    k, m = np.broadcast_arrays(np.asarray(k, dtype=np.uint64), np.asarray(m, dtype=np.uint64))
    c0, c1, c2, c3, key0, key1 = counter_words(int(seed), k, m, carry, swap)
    x0, x1, x2, x3 = philox_np(c0, c1, c2, c3, key0, key1)
    u1, u2 = unit_ld(x0, x1), unit_ld(x2, x3)
    r = np.sqrt(LD(-2) * np.log(u1))
    cs, sn = np.cos(LD(2) * PI_LD * u2), np.sin(LD(2) * PI_LD * u2)
    if swap_trig:
        cs, sn = sn, cs
    return r, r * cs, r * sn


def noise_ref(V, sigma, s, seed, k0=0, m0=0, **mistake):
    """rjp_vis_noise on V [M, K, 2] (float64) -> (ref longdouble [M, K, 2], bound float64 [M, K, 2],
    copy [M] bool: the maps that are copied bit for bit).  NaN where the contract says NaN."""
    V = np.asarray(V, dtype=np.float64)
    M, K = V.shape[:2]
    sigma = np.asarray(sigma, dtype=np.float64).reshape(M)
    sk = np.ones(K) if s is None else np.asarray(s, dtype=np.float64).reshape(K)
    kk = (np.arange(K, dtype=np.uint64) + np.uint64(int(k0)))[None, :]
    mm = (np.arange(M, dtype=np.uint64) + np.uint64(int(m0)))[:, None]
    r, g1, g2 = normals(seed, kk, mm, **mistake)
    with np.errstate(invalid="ignore"):
        a = sigma.astype(LD)[:, None] * sk.astype(LD)[None, :]
    ref = np.stack([V[..., 0].astype(LD) + a * g1, V[..., 1].astype(LD) + a * g2], axis=-1)
    copy = sigma == 0.0
    ref[copy] = V[copy].astype(LD)
    bad = ~np.isfinite(sk)
    ref[:, bad, :] = np.nan
    with np.errstate(invalid="ignore"):
        amp = np.abs((a * r).astype(np.float64))[..., None]
        bound = U * np.abs(ref.astype(np.float64)) + amp * (C_N * U + SINCOS_TRUNC)
    bound[copy] = 0.0
    return ref, bound, copy


def noise_f64(V, sigma, s, seed, k0=0, m0=0, round_u=False, **mistake):
    """A float64 emulation of the kernel (NumPy's log / sin / cos instead of the device's): what
    the bound must admit.  `round_u`: a planted mistake -- the uniform from 53 random bits rounded
    to nearest, (n53 + 0.5) 2^-53 evaluated in float64, which reaches 1."""
    V = np.asarray(V, dtype=np.float64)
    M, K = V.shape[:2]
    sigma = np.asarray(sigma, dtype=np.float64).reshape(M)
    sk = np.ones(K) if s is None else np.asarray(s, dtype=np.float64).reshape(K)
    kk = (np.arange(K, dtype=np.uint64) + np.uint64(int(k0)))[None, :]
    mm = (np.arange(M, dtype=np.uint64) + np.uint64(int(m0)))[:, None]
    kk, mm = np.broadcast_arrays(kk, mm)
    c0, c1, c2, c3, key0, key1 = counter_words(int(seed), kk, mm, mistake.get("carry", True),
                                               mistake.get("swap", False))
    x0, x1, x2, x3 = philox_np(c0, c1, c2, c3, key0, key1)
    if round_u:
        u1, u2 = bad_unit_f64(x0, x1), bad_unit_f64(x2, x3)
    else:
        u1, u2 = unit_ld(x0, x1).astype(np.float64), unit_ld(x2, x3).astype(np.float64)
    with np.errstate(divide="ignore"):
        r = np.sqrt(-2.0 * np.log(u1))
    cs, sn = np.cos(2.0 * np.pi * u2), np.sin(2.0 * np.pi * u2)
    if mistake.get("swap_trig", False):
        cs, sn = sn, cs
    ar = (sigma[:, None] * sk[None, :]) * r
    out = np.stack([V[..., 0] + ar * cs, V[..., 1] + ar * sn], axis=-1)
    out[sigma == 0.0] = V[sigma == 0.0]
    out[:, ~np.isfinite(sk), :] = np.nan
    return out


def bad_unit_f64(hi, lo):
    """The planted 53-bit uniform: all of hi and the top 21 bits of lo, plus a half, in float64 --
    2^53 - 1 + 0.5 rounds to 2^53 and the uniform to 1."""
    n = (np.asarray(hi, dtype=np.uint64) << np.uint64(21)) | (np.asarray(lo, dtype=np.uint64) >> np.uint64(11))
    return (n.astype(np.float64) + 0.5) * 2.0 ** -53


# ---- tracks ----------------------------------------------------------------------------------------
def pairs(n_ant, j_major=False):
    """(ant1, ant2) of the baselines in the contract's order: i < j, i-major."""
    if j_major:                                 # sorted by the SECOND antenna first: the mistake
        return (np.array([i for j in range(n_ant) for i in range(j)]),
                np.array([j for j in range(n_ant) for i in range(j)]))
    return np.triu_indices(n_ant, 1)


def tracks_ref(xyz, gha, sin_dec, cos_dec, up=None, sin_min_el=None, dtype=LD, radians=False,
               neg_g=False, reverse_b=False, j_major=False):
    """rjp_uv_tracks -> dict of u, v, w [n_t, n_bl] in `dtype` (NaN where flagged), `flag`
    [n_t, n_bl] bool, `B` [n_bl] = |bx| + |by| + |bz| (float64 differences, as the kernel forms
    them), `bound` [n_bl], and `margin`: the smallest |up_i . s - sin_min_el| over finite
    integrations (a test keeps it well above the rounding of the dot product).  The keywords after
    `dtype` plant mistakes; dtype=np.float64 is the emulation the bound must admit."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    gha = np.asarray(gha, dtype=np.float64).reshape(-1)
    i, j = pairs(len(xyz), j_major)
    b64 = xyz[i] - xyz[j] if reverse_b else xyz[j] - xyz[i]
    b = b64.astype(dtype)
    fin = np.isfinite(gha)
    g = np.where(fin, gha, 0.0)
    g = (g - np.rint(g)).astype(dtype)
    two_pi = dtype(2) * (PI_LD if dtype is LD else dtype(np.pi))
    G = g if radians else two_pi * g
    if neg_g:
        G = -G
    sG, cG = np.sin(G)[:, None], np.cos(G)[:, None]
    sd, cd = dtype(sin_dec), dtype(cos_dec)
    bx, by, bz = b[None, :, 0], b[None, :, 1], b[None, :, 2]
    u = sG * bx + cG * by
    v = -sd * cG * bx + sd * sG * by + cd * bz
    w = cd * cG * bx - cd * sG * by + sd * bz
    flag = np.broadcast_to(~fin[:, None], u.shape).copy()
    margin = np.inf
    if up is not None:
        upl = np.asarray(up, dtype=np.float64).astype(dtype)
        sx, sy = cd * cG, -cd * sG                                   # [n_t, 1]
        e = upl[None, :, 0] * sx + upl[None, :, 1] * sy + upl[None, :, 2] * sd    # [n_t, n_ant]
        low = e < dtype(sin_min_el)
        flag |= low[:, i] | low[:, j]
        if fin.any():
            margin = float(np.min(np.abs(e[fin] - dtype(sin_min_el))))
    u, v, w = (np.where(flag, dtype(np.nan), x) for x in (u, v, w))
    B = np.abs(b64).sum(axis=1)
    return dict(u=u, v=v, w=w, flag=flag, B=B, bound=(C_T * U + SINCOS_TRUNC) * B, margin=margin,
                ant1=i, ant2=j)


def random_array(n_ant, seed, radius_m=2.0e4, lat_deg=34.0, lon_deg=-107.6):
    """`n_ant` antennas scattered over a disc of `radius_m` on the WGS84 sphere-ish surface near
    (lat, lon) -> (xyz [n_ant, 3], up [n_ant, 3]); geocentric metres, unit verticals."""
    rng = np.random.default_rng(seed)
    lat = np.radians(lat_deg) + rng.uniform(-1, 1, n_ant) * radius_m / 6.37e6
    lon = np.radians(lon_deg) + rng.uniform(-1, 1, n_ant) * radius_m / 6.37e6 / np.cos(np.radians(lat_deg))
    up = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=1)
    return up * (6.37e6 + rng.uniform(0, 100, n_ant))[:, None], up


def read_fixture(path):
    """The antenna list of tests/golden/antenna_configs read without the code under test."""
    names, xyz = [], []
    for line in open(path):
        if line.strip() and not line.startswith("#"):
            c = line.split()
            xyz.append([float(x) for x in c[:3]])
            names.append(c[4])
    return names, np.array(xyz)
