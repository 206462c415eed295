"""The inputs of the K22 tests, shared by tests/test_gpu_gaincal.py (the device) and
tests/test_gaincal_reference_cpu.py (the float64 emulation on the same inputs): a case is the dict
`gaincal_ref.follow` takes, plus `planted` (the gains the data were made with, or None) and
`converges` (whether the GPU test demands status 1 and the planted gains back to 1e-9).

Input choice (a prototype of the iteration was run on the CPU): model amplitudes uniform in [0.5,
2], planted gains 1 +- 0.2 in amplitude and +-60 degrees in phase, unit start, tol = 1e-12 converge
in at most 110 steps for 3 to 64 antennas; log-normal amplitudes do not always.  So the convergence
cases use the bounded amplitudes with n_iter = 300, and the CPU emulation asserts that they
converge, so that no GPU case is vacuous."""
import numpy as np

from tests import gaincal_ref as K

TOL, N_ITER = 1e-12, 300


def table(kind, n_t):
    """'one' (a single interval), 'int' (one per integration), 'uneven' (lengths 1, 2, 3, 1, 2, 3 ...)."""
    if kind == "one":
        return np.zeros(n_t, dtype=np.int32)
    if kind == "int":
        return np.arange(n_t, dtype=np.int32)
    h, s, t = [], 0, 0
    while t < n_t:
        for _ in range(1 + s % 3):
            if t < n_t:
                h.append(s)
                t += 1
        s += 1
    return np.array(h, dtype=np.int32)


def planted_gains(rng, M, S, n_ant, mode, refant):
    amp = 1.0 + 0.2 * rng.uniform(-1, 1, (M, S, n_ant)) if mode == 0 else np.ones((M, S, n_ant))
    ph = np.radians(60.0) * rng.uniform(-1, 1, (M, S, n_ant))
    ph[..., refant] = 0.0
    return amp * np.exp(1j * ph)


def model(rng, MM, T, nb):
    return rng.uniform(0.5, 2.0, (MM, T, nb)) * np.exp(2j * np.pi * rng.uniform(0, 1, (MM, T, nb)))


def corrupt(Mod, G, h_sol, n_ant, M):
    p, q = K.pairs(n_ant)
    g = G[:, np.asarray(h_sol)]                                           # [M, T, n_ant]
    return g[:, :, p] * np.conj(g[:, :, q]) * np.broadcast_to(Mod, (M,) + Mod.shape[1:])


def make(n_ant, n_t, sol, M, MM, wkind, mode=0, refant=0, min_bl=None, seed=0, flag=0.0, tol=TOL,
         n_iter=N_ITER):
    rng = np.random.default_rng(1000 * n_ant + n_t + seed)
    h_sol = table(sol, n_t)
    S, nb = int(h_sol[-1]) + 1, K.n_bl(n_ant)
    G = planted_gains(rng, M, S, n_ant, mode, refant)
    Mod = model(rng, MM, n_t, nb)
    D = corrupt(Mod, G, h_sol, n_ant, M)
    w = None
    if wkind is not None:
        w = rng.uniform(0.5, 2.0, (1 if wkind == "shared" else M, n_t, nb))
    if flag > 0:
        # a share of the visibilities flagged in each of the four ways
        sel = lambda: rng.uniform(0, 1, D.shape) < flag / 4
        D = np.where(sel(), np.nan + 0j, D)
        D = np.where(sel(), D.real + 1j * np.inf, D)
        Mod = np.where(sel()[:MM], np.nan + 1j * np.nan, Mod)
        Mod = np.where(sel()[:MM], 0j, Mod)
        if w is not None:
            w = np.where(sel()[:w.shape[0]], 0.0, w)
            w = np.where(sel()[:w.shape[0]], -1.0, w)
    return dict(D=D, Mod=Mod, w=w, h_sol=h_sol, n_ant=n_ant, mode=mode, refant=refant,
                min_bl=min(4, n_ant - 1) if min_bl is None else min_bl, tol=tol, n_iter=n_iter,
                g_start=np.ones((M, S, n_ant), dtype=np.complex128), planted=G, converges=True)


# (n_ant, n_t, table, maps, model maps, weights, mode): every antenna count of the issue, 1 to 257
# integrations, n_sol = 1, n_t and uneven, 1-3 maps, the model shared and per map, weights none,
# shared and per map
SIZED = [(2, 1, "one", 1, 1, None, 1), (3, 5, "one", 2, 1, "shared", 0), (4, 7, "one", 3, 3, "per map", 0),
         (5, 16, "int", 1, 1, None, 1), (27, 33, "uneven", 2, 1, "shared", 0), (64, 6, "uneven", 1, 1, None, 0),
         (27, 2, "int", 1, 1, "per map", 1), (7, 257, "uneven", 1, 1, "shared", 0)]


def sized(n_ant, n_t, sol, M, MM, wkind, mode):
    # (the longest case carries 30 % flagged visibilities, with zeros in the weights)
    return make(n_ant, n_t, sol, M, MM, wkind, mode, refant=n_ant // 2, flag=0.3 if n_t == 257 else 0.0)


def named(name):
    if name == "dead antenna":
        # antenna 2 wholly flagged in interval 1 only: NaN there, the others solved
        c = make(6, 6, "uneven", 2, 1, "shared", min_bl=2, seed=1)
        p, q = K.pairs(6)
        sel = (p == 2) | (q == 2)
        ta, tb = K.intervals(c["h_sol"])[1]
        c["D"][:, ta:tb, sel] = np.nan
        return c
    if name == "cascade":
        # five antennas, min_bl = 2: {0, 1, 2} a triangle, 3 sees 0 and 4, 4 sees 3 alone -- 4 leaves
        # in the first sweep, 3 in the second
        c = make(5, 4, "one", 1, 1, None, min_bl=2, seed=2)
        p, q = K.pairs(5)
        keep = {(0, 1), (0, 2), (1, 2), (0, 3), (3, 4)}
        sel = np.array([(a, b) not in keep for a, b in zip(p, q)])
        c["Mod"][:, :, sel] = 0.0
        return c
    if name == "empty interval":
        # nothing counts in interval 0 of map 1 (all weights 0): status 3 there alone
        c = make(4, 5, "uneven", 2, 1, "per map", seed=3)
        ta, tb = K.intervals(c["h_sol"])[0]
        c["w"][1, ta:tb] = 0.0
        return c
    if name == "bad start":
        # a start gain of 0 in solution (0, 0), NaN in (0, 2): status 3; the others solved
        c = make(4, 3, "int", 1, 1, None, seed=4)
        c["g_start"][0, 0, 1] = 0.0
        c["g_start"][0, 2, 3] = np.nan
        return c
    if name == "den zero":
        # |M|^2 ~ 1e-320 counts (> 0) but times |g|^2 = 1e-6 it underflows to 0: status 2 at step 1
        c = make(4, 2, "one", 1, 1, None, seed=5)
        c["Mod"] = c["Mod"] * 1e-160
        c["D"] = c["D"] * 1e-160
        c["g_start"][:] = 1e-3
        c["converges"] = False
        return c
    if name == "exhausted":
        c = make(5, 3, "one", 2, 2, None, seed=6, n_iter=5)
        c["converges"] = False
        return c
    raise KeyError(name)


NAMED = ["dead antenna", "cascade", "empty interval", "bad start", "den zero", "exhausted"]


def recovered(case, gains):
    """The worst |g - planted| / |planted| over the live antennas of the solved solutions, both
    referenced to the antenna the solution was referenced to (the one with Im g = +0 exactly)."""
    worst = 0.0
    G = case["planted"]
    for m in range(gains.shape[0]):
        for s in range(gains.shape[1]):
            g = gains[m, s]
            ok = np.isfinite(g.real)
            if not ok.any():
                continue
            r = case["refant"] if ok[case["refant"]] else int(np.nonzero(ok)[0][0])
            want = G[m, s] * np.conj(G[m, s, r]) / abs(G[m, s, r])
            worst = max(worst, float((abs(g - want) / abs(want))[ok].max()))
    return worst
