"""A long-double NumPy reference of K22 (rjp_gain_apply, rjp_gaincal; include/rjprt.h is the
definition) and a float64 emulation of the device's arithmetic.  No GPU, no library.

The reference FOLLOWS the device (`follow`), as K20's and K21's do: StefCal is a fixed-point
iteration, and two correct implementations part ways after a few steps at rounding level, so the
judgement is made one step at a time from the device's own previous gains (its trace).  It checks,
per (map, interval):

  (a) n_pq summed (d_nvis) and the workspace's A, B against the long-double sums of the inputs;
  (b) the live set, exactly, and status 3 with its untouched outputs;
  (c) for every step k the device's g(k) against ONE long-double step from the device's g(k - 1);
  (d) the convergence decision where it lies outside the margin of the two bounds, status, d_niter,
      the breakdown (status 2) only where the reference's denominator may vanish;
  (e) the referencing of the last step's gains, Im g_r = +0.0, NaN on dead antennas, poisoned trace
      rows at and beyond d_niter;
  (f) both chi^2 against the long-double residual of the gains the device wrote.

Every bound is derived here, none is measured.  u = 2^-53; "|z|_1" = |Re z| + |Im z|.

  A, B of a pair with L counting integrations.  A term of Re A is w (Dr Mr + Di Mi): the product
  Di Mi, the fma that adds Dr Mr and the fma that adds w times it to the chain round once each, the
  chain L times in all: |dA| <= (L + 3) u sum w (|Dr Mr| + |Di Mi|) =: eA, the same for Im A;
  |dB| <= (L + 3) u B =: eB (m2 rounds twice); each rounding may instead cost 2^-1074 where the
  numbers are subnormal, (L + 3) 2^-1074 in all (2 N 2^-1074 for a chi^2 of N visibilities).  (An emulation without fma rounds once more per
  term; it stays inside with these constants only because a bound is a worst case.)

  One step at antenna p over n - 1 partners in four chains of at most c = ceil(n / 4) terms.  A
  component of num is a sum of 2 (n - 1) products, each chain entry rounding once, the two
  additions of the combination once each: with S_p = sum_q |g_q|_1 |A_pq|_1
      e_num = (2 c + 2) u S_p + sum_q |g_q|_1 eA_pq.
  den: |g_q|^2 rounds twice, the chain c times, the combination twice: with T_p = sum_q |g_q|^2 B_pq
      e_den = (c + 4) u T_p + sum_q |g_q|^2 (1 + 2 u) eB_pq.
  mode 0: h = num / den per component: e_h = (e_num + |h| e_den) / (den - e_den) + u |h|.
  mode 1: a = sqrt(fma(nr, nr, ni ni)) has |da| <= sqrt(2) e_num + 2 u a =: e_a, and
      e_h = (e_num + |h| e_a) / (a - e_a) + u |h|.
  odd k: g' = h, e_g = e_h.  even k: g' = 0.5 (h + g), the addition rounds once, the halving is
  exact: e_g = 0.5 e_h + u |g'|.

  The decision compares d = max |g' - g| with tol max |g'|, each |z| = sqrt(fma(zr, zr, zi zi)) of
  numbers the trace holds exactly: the subtraction, the product, the fma and the root round once
  each, at most 3 u relative on either side, and tol max rounds once more.  Outside
  d (1 +- 4 u) <> tol gmax (1 -+ 4 u) the decision is demanded.

  Referencing: a = |g_r| (2 u relative), c = conj(g_r) / a (3 u), the rotated gain one product and
  one fma: |dg| <= 5 u |g|_1 (|c| <= 1 up to 3 u) -- asserted at 6 u |g|_1.

  chi^2 of one visibility: c = g_p conj g_q per component within 2 u |g_p|_1 |g_q|_1 =: e_c; c M
  within e_c |M|_1 + 2 u |c|_1 |M|_1; the residual component e within that plus u |e| =: de; the two
  terms w e^2 within w (2 |e| de + de^2) + 2 u w e^2, and the chain of a lane (2 L ceil(n_bl / 256)
  terms) plus the fold (8 additions): e_chi = sum w (2 |e| de + de^2) + (2 L ceil(n_bl / 256) + 10) u chi^2.

  rjp_gain_apply, per component: mode 0, e_c |V|_1 + 2 u |c|_1 |V|_1; mode 1, with t = V conj c
  (dt = the same), n2 = |c|^2 (dn = 2 |c|_1 e_c + 2 u n2): dt / n2 + |t| dn / n2^2 + u |out|, the
  denominators taken at n2 - dn.
"""
import numpy as np

LD = np.longdouble
CLD = np.clongdouble
U = 2.0 ** -53
MAX_ANT = 64
SUB = np.longdouble(2.0) ** -1074          # the spacing of the subnormals: what a rounding there costs
TINY = 2.0 ** -1000          # below this a float64 denominator may have underflowed

MSG_A = {
    "nulls": "rjp_gain_apply: NULL visibilities, gains, intervals or output",
    "sizes": "rjp_gain_apply: n_maps, n_t and n_sol must be positive",
    "ant": "rjp_gain_apply: n_ant must lie in 2 .. RJP_GAINCAL_MAX_ANT (64)",
    "sol": "rjp_gain_apply: h_sol must start at 0, rise in steps of 0 or 1 and end at n_sol - 1",
    "maps": "rjp_gain_apply: g_maps must be 1 or n_maps",
    "mode": "rjp_gain_apply: mode must be 0 (corrupt) or 1 (correct)",
    "wgs": "rjp_gain_apply: more than 2^31 - 1 workgroups",
}
MSG_G = {
    "nulls": "rjp_gaincal: NULL visibilities, model, intervals, gains or outputs",
    "sizes": "rjp_gaincal: n_maps, n_t and n_sol must be positive",
    "ant": "rjp_gaincal: n_ant must lie in 2 .. RJP_GAINCAL_MAX_ANT (64)",
    "sol": "rjp_gaincal: h_sol must start at 0, rise in steps of 0 or 1 and end at n_sol - 1",
    "mmaps": "rjp_gaincal: model_maps must be 1 or n_maps",
    "wmaps": "rjp_gaincal: w_maps must be 1 or n_maps",
    "mode": "rjp_gaincal: mode must be 0 (amplitude and phase) or 1 (phase only)",
    "refant": "rjp_gaincal: refant outside 0 .. n_ant - 1",
    "minbl": "rjp_gaincal: min_bl < 1",
    "tol": "rjp_gaincal: tol must be finite and positive",
    "iter": "rjp_gaincal: n_iter < 1",
    "wgs": "rjp_gaincal: more than 2^31 - 1 workgroups",
    "work": "rjp_gaincal: workspace smaller than rjp_gaincal_workspace()",
}
PARTS = {}


def part(name, r):
    PARTS[name] = max(PARTS.get(name, 0.0), float(r))
    return float(r)


def n_bl(n_ant):
    return n_ant * (n_ant - 1) // 2


def pairs(n_ant):
    """(p [n_bl], q [n_bl]) of the p-major list of pairs p < q."""
    return np.triu_indices(n_ant, 1)


def workspace_bytes(n_maps, n_sol, n_ant):
    ms, tri = n_maps * n_sol, n_bl(n_ant)
    return 8 * ms * (3 * tri + 2 * n_ant) + (4 * ms * tri + 7) // 8 * 8


def apply_workgroups(n_maps, n_t, n_ant):
    return (n_maps * n_t * n_bl(n_ant) + 255) // 256


def gaincal_workgroups(n_maps, n_sol, n_ant):
    return (n_maps * n_sol * n_bl(n_ant) + 255) // 256 + 2 * n_maps * n_sol


def split_workspace(work, n_maps, n_sol, n_ant):
    """The workspace bytes -> (A complex [ms, n_bl], B [ms, n_bl], g0 complex [ms, n_ant], n [ms, n_bl])."""
    ms, tri = n_maps * n_sol, n_bl(n_ant)
    d = np.frombuffer(work.tobytes()[:8 * ms * (3 * tri + 2 * n_ant)], dtype=np.float64)
    ab = d[:ms * 3 * tri].reshape(ms, 3, tri)
    g0 = d[ms * 3 * tri:].reshape(ms, n_ant, 2)
    off = 8 * ms * (3 * tri + 2 * n_ant)
    n = np.frombuffer(work.tobytes()[off:off + 4 * ms * tri], dtype=np.int32).reshape(ms, tri)
    return ab[:, 0] + 1j * ab[:, 1], ab[:, 2], g0[..., 0] + 1j * g0[..., 1], n


def intervals(h_sol):
    """[(ta, tb)] of every interval of a table."""
    h = np.asarray(h_sol)
    assert h[0] == 0 and np.all((np.diff(h) == 0) | (np.diff(h) == 1))
    starts = [0] + [t for t in range(1, h.size) if h[t] != h[t - 1]] + [h.size]
    return list(zip(starts[:-1], starts[1:]))


def counting(D, M, w):
    """The counting rule on [T, n_bl] slices (float64 arithmetic for m2, as the definition says)."""
    with np.errstate(all="ignore"):
        m2 = M.real * M.real + M.imag * M.imag
        ok = np.isfinite(D.real) & np.isfinite(D.imag) & np.isfinite(M.real) & np.isfinite(M.imag) & (m2 > 0)
        if w is not None:
            ok &= np.isfinite(w) & (w > 0)
    return ok


def _clean(D, M, w, ok):
    one = np.ones(D.shape) if w is None else w
    z = lambda a: np.where(ok, a, 0.0).astype(LD)
    return z(D.real), z(D.imag), z(M.real), z(M.imag), z(one)


def accumulate(D, M, w):
    """One interval's [L, n_bl] slices -> dict: A (complex long double [n_bl]), B, n, eA, eB."""
    ok = counting(D, M, w)
    dr, di, mr, mi, wt = _clean(D, M, w, ok)
    n = ok.sum(axis=0)
    A = np.zeros(D.shape[1], dtype=CLD)
    A.real = (wt * (dr * mr + di * mi)).sum(axis=0)
    A.imag = (wt * (di * mr - dr * mi)).sum(axis=0)
    B = (wt * (mr * mr + mi * mi)).sum(axis=0)
    SA = np.maximum((wt * (abs(dr * mr) + abs(di * mi))).sum(axis=0), (wt * (abs(di * mr) + abs(dr * mi))).sum(axis=0))
    return dict(A=A, B=B, n=n, eA=(n + 3) * (U * SA + SUB), eB=(n + 3) * (U * B + SUB))


def full(x, n_ant, herm):
    """A per-pair vector -> the [n_ant, n_ant] matrix (x_qp = conj x_pq with `herm`), zero diagonal."""
    p, q = pairs(n_ant)
    X = np.zeros((n_ant, n_ant), dtype=x.dtype)
    X[p, q] = x
    X[q, p] = np.conj(x) if herm else x
    return X


def live_set(Bpos, n_ant, min_bl):
    """The live antennas from the [n_ant, n_ant] pattern B_pq > 0, by the definition's sweeps."""
    live = np.ones(n_ant, dtype=bool)
    while True:
        cnt = (Bpos & live[None, :]).sum(axis=1)
        drop = live & (cnt < min_bl)
        if not drop.any():
            return live
        live = live & ~drop


def one_step(acc, g, live, n_ant, mode, k):
    """One long-double step from the gains g (complex, any precision) -> (g' complex long double,
    e_g per component, den (or |num|) and its bound, for the breakdown rule)."""
    g = np.where(live, np.asarray(g, dtype=CLD), 0)
    A, B = full(acc["A"], n_ant, True), full(acc["B"], n_ant, False)
    eA, eB = full(acc["eA"], n_ant, False), full(acc["eB"], n_ant, False)
    g1 = abs(g.real) + abs(g.imag)
    g2 = g.real ** 2 + g.imag ** 2
    c = -(-n_ant // 4)
    num = A @ g
    S = (abs(A.real) + abs(A.imag)) @ g1
    e_num = (2 * c + 2) * U * S + eA @ g1
    if mode == 0:
        div = B @ g2
        e_div = (c + 4) * U * div + (eB @ g2) * (1 + 2 * U)
    else:
        div = abs(num)
        e_div = np.sqrt(LD(2)) * e_num + 2 * U * div
    with np.errstate(all="ignore"):
        h = num / div
        hmax = np.maximum(abs(h.real), abs(h.imag))
        e_h = (e_num + hmax * e_div) / (div - e_div) + U * hmax
    if k % 2 == 1:
        gn, e_g = h, e_h
    else:
        gn = 0.5 * (h + g)
        e_g = 0.5 * e_h + U * np.maximum(abs(gn.real), abs(gn.imag))
    return gn, e_g, div, e_div


def reference_rotate(g, live, refant):
    g = np.asarray(g, dtype=CLD)
    r = refant if live[refant] else int(np.nonzero(live)[0][0])
    c = np.conj(g[r]) / abs(g[r])
    out = g * c
    out[r] = out[r].real
    return np.where(live, out, np.nan), r


def chi2_ref(D, M, w, g, live, n_ant):
    """sum w |D - g_p conj(g_q) M|^2 over the counting visibilities of live pairs -> (chi2, bound)."""
    ok = counting(D, M, w)
    p, q = pairs(n_ant)
    ok = ok & (live[p] & live[q])[None, :]
    dr, di, mr, mi, wt = _clean(D, M, w, ok)
    gl = np.where(live, np.asarray(g, dtype=CLD), 0)
    c = gl[p] * np.conj(gl[q])
    g1 = abs(gl.real) + abs(gl.imag)
    e_c = 2 * U * g1[p] * g1[q]
    c1, m1 = abs(c.real) + abs(c.imag), abs(mr) + abs(mi)
    er = dr - (c.real * mr - c.imag * mi)
    ei = di - (c.real * mi + c.imag * mr)
    de_r = (e_c + 2 * U * c1) * m1 + U * abs(er)
    de_i = (e_c + 2 * U * c1) * m1 + U * abs(ei)
    chi = (wt * (er * er + ei * ei)).sum()
    L = D.shape[0]
    lanes = -(-n_bl(n_ant) // 256)
    bound = (wt * (2 * abs(er) * de_r + de_r ** 2 + 2 * abs(ei) * de_i + de_i ** 2)).sum() + \
        (2 * L * lanes + 10) * U * chi + 2 * ok.sum() * SUB
    return chi, bound


def apply_ref(V, gp, gq, mode):
    """rjp_gain_apply of arrays of visibilities and their two gains -> (out complex long double, bound
    per component)."""
    with np.errstate(all="ignore"):
        V, gp, gq = (np.asarray(a, dtype=CLD) for a in (V, gp, gq))
        c = gp * np.conj(gq)
        l1 = lambda z: abs(z.real) + abs(z.imag)
        e_c = 2 * U * l1(gp) * l1(gq)
        dt = (e_c + 2 * U * l1(c)) * l1(V)
        if mode == 0:
            out = c * V
            return out, dt + U * l1(out)
        n2 = c.real ** 2 + c.imag ** 2
        dn = 2 * l1(c) * e_c + 2 * U * n2
        t = V * np.conj(c)
        out = t / n2
        return out, dt / (n2 - dn) + l1(t) * dn / (n2 - dn) ** 2 + U * l1(out)


def check_apply(V, gains, h_sol, n_ant, mode, out):
    """[M, T, n_bl] complex data, [G, S, n_ant] gains, the device's `out` -> worst error / bound;
    NaN exactly where a gain or the visibility is not finite (or, correcting, the product is 0)."""
    p, q = pairs(n_ant)
    worst = 0.0
    for m in range(V.shape[0]):
        g = gains[0 if gains.shape[0] == 1 else m][np.asarray(h_sol)]              # [T, n_ant]
        ref, bound = apply_ref(V[m], g[:, p], g[:, q], mode)
        bad = ~(np.isfinite(ref.real) & np.isfinite(ref.imag))
        got = out[m]
        assert np.all(np.isnan(got.real[bad]) | np.isnan(got.imag[bad])), "a flagged visibility came out finite"
        assert np.all(np.isfinite(got.real[~bad]) & np.isfinite(got.imag[~bad]))
        if (~bad).any():
            err = np.maximum(abs(got.real - ref.real), abs(got.imag - ref.imag))[~bad]
            b = bound[~bad] + LD(5e-324)
            worst = max(worst, float((err / b).max()))
    return part("apply", worst)


def follow(case, out, poison_f, poison_i, poison_t, poison_live=0xA5):
    """Checks (a)-(f) of a raw rjp_gaincal call.  `case`: D [M, T, n_bl], Mod [1 or M, T, n_bl]
    complex, w None or [1 or M, T, n_bl], h_sol, n_ant, mode, refant, min_bl, tol, n_iter, g_start
    [M, S, n_ant] complex.  `out`: gains [M, S, n_ant] complex, chi2 [M, S, 2], nvis, niter, status
    [M, S], live [M, S, n_ant], trace [M, S, n_iter, n_ant] complex, work (bytes as uint8).  ->
    the worst error / bound; discrete disagreements raise AssertionError."""
    D, Mod, w = case["D"], case["Mod"], case["w"]
    n_ant, mode, refant, min_bl = case["n_ant"], case["mode"], case["refant"], case["min_bl"]
    tol, n_iter, g_start = case["tol"], case["n_iter"], case["g_start"]
    M = D.shape[0]
    iv = intervals(case["h_sol"])
    S = len(iv)
    wa, wb, wg0, wn = split_workspace(out["work"], M, S, n_ant)
    isp = lambda a, v: np.array_equal(np.asarray(a), np.full(np.shape(a), v, dtype=np.asarray(a).dtype))
    worst = 0.0
    for m in range(M):
        for s, (ta, tb) in enumerate(iv):
            Dm, Mm = D[m, ta:tb], Mod[0 if Mod.shape[0] == 1 else m, ta:tb]
            wm = None if w is None else w[0 if w.shape[0] == 1 else m, ta:tb]
            acc = accumulate(Dm, Mm, wm)
            ms = m * S + s
            # (a)
            assert np.array_equal(wn[ms], acc["n"]), ("n_pq", m, s)
            assert out["nvis"][m, s] == acc["n"].sum(), ("nvis", m, s)
            errA = np.maximum(abs(wa[ms].real - acc["A"].real), abs(wa[ms].imag - acc["A"].imag))
            worst = max(worst, part("A", (errA / (acc["eA"] + LD(1e-4000))).max()))
            worst = max(worst, part("B", (abs(wb[ms] - acc["B"]) / (acc["eB"] + LD(1e-4000))).max()))
            # (b)
            live = live_set(full(acc["B"], n_ant, False) > 0, n_ant, min_bl)
            g0 = g_start[m, s]
            bad0 = live & ~(np.isfinite(g0.real) & np.isfinite(g0.imag) & (g0 != 0))
            st, nit = int(out["status"][m, s]), int(out["niter"][m, s])
            tr = out["trace"][m, s] if out.get("trace") is not None else None
            if live.sum() < (3 if mode == 0 else 2) or bad0.any():
                assert st == 3, ("status 3 expected", m, s, st)
                assert np.all(np.isnan(out["gains"][m, s].real) & np.isnan(out["gains"][m, s].imag))
                assert nit == poison_i and isp(out["live"][m, s], poison_live)
                assert isp(out["chi2"][m, s], poison_f) and (tr is None or isp(tr.view(np.float64), poison_t))
                continue
            assert st != 3, ("status 3 not expected", m, s)
            assert np.array_equal(out["live"][m, s] != 0, live) and out["live"][m, s].max() <= 1, ("live", m, s)
            assert wg0[ms].tobytes() == np.ascontiguousarray(g0).tobytes(), "the start gains in the workspace"
            # (c), (d)
            g, k, status = g0.copy(), 0, None
            while status is None:
                k += 1
                gn, e_g, div, e_div = one_step(acc, g, live, n_ant, mode, k)
                may_break = bool(np.any((div - e_div <= TINY)[live]) or not np.all(np.isfinite(gn[live])))
                if st == 2 and nit == k - 1:
                    assert may_break, ("breakdown without cause", m, s, k)
                    status = 2
                    break
                assert not np.any((div <= 0)[live]), ("a vanishing denominator went unnoticed", m, s, k)
                assert tr is not None, "following needs the trace"
                dev = tr[k - 1]
                assert np.all(np.isnan(dev.real[~live]) & np.isnan(dev.imag[~live])), "dead antennas in the trace"
                err = np.maximum(abs(dev.real - gn.real), abs(dev.imag - gn.imag))[live]
                worst = max(worst, part("step", (err / e_g[live]).max()))
                d = abs((dev.astype(CLD) - g.astype(CLD))[live]).max()
                gm = abs(dev.astype(CLD)[live]).max()
                g = np.where(live, dev, g)
                if d * (1 + 4 * U) < tol * gm * (1 - 4 * U):
                    must = 1
                elif d * (1 - 4 * U) > tol * gm * (1 + 4 * U):
                    must = 0
                else:
                    must = None
                if nit == k:
                    assert st in (0, 1), (m, s, st)
                    if st == 1:
                        assert must != 0, ("converged too early", m, s, k)
                    else:
                        assert k == n_iter and must != 1, ("the decision", m, s, k, must)
                    status = st
                else:
                    assert must in (None, 0) and k < n_iter, ("the iteration went on", m, s, k)
            assert st == status and nit == (k - 1 if status == 2 else k), ("niter", m, s)
            if tr is not None:
                assert isp(tr[nit:].view(np.float64), poison_t), "trace rows beyond d_niter"
            # (e)
            ref, r = reference_rotate(g, live, refant)
            got = out["gains"][m, s]
            assert np.all(np.isnan(got.real[~live]) & np.isnan(got.imag[~live])), "dead antennas"
            assert got.imag[r] == 0.0 and not np.signbit(got.imag[r]) and got.real[r] > 0
            g1 = (abs(g.real) + abs(g.imag))[live]
            err = np.maximum(abs(got.real - ref.real), abs(got.imag - ref.imag))[live]
            worst = max(worst, part("referencing", (err / (6 * U * g1)).max()))
            # (f)
            for j, gg in enumerate((g0, got)):
                chi, bound = chi2_ref(Dm, Mm, wm, gg, live, n_ant)
                worst = max(worst, part("chi2", abs(out["chi2"][m, s, j] - chi) / (bound + LD(1e-4000))))
    return worst


# ---- the float64 emulation -------------------------------------------------------------------------
def emulate(case, mistake=None, poison_f=7.25, poison_i=-77, poison_t=-7.5, poison_live=0xA5):
    """The three kernels in float64 NumPy, in the definition's order of operations (without fma), on
    a case of `follow` -> an `out` of the same shape, poisoned where the device writes nothing.
    `mistake`: one of the planted ones (tests/test_gaincal_reference_cpu.py)."""
    D, Mod, w = case["D"], case["Mod"], case["w"]
    n_ant, mode, refant, min_bl = case["n_ant"], case["mode"], case["refant"], case["min_bl"]
    tol, n_iter = case["tol"], case["n_iter"]
    M, T, nb = D.shape
    iv = intervals(case["h_sol"])
    S = len(iv)
    p, q = pairs(n_ant)
    gains = case["g_start"].astype(np.complex128).copy()
    chi2 = np.full((M, S, 2), poison_f)
    nvis, niter, status = (np.full((M, S), poison_i, dtype=np.int32) for _ in range(3))
    livo = np.full((M, S, n_ant), poison_live, dtype=np.uint8)
    trace = np.full((M, S, n_iter, n_ant), poison_t + 1j * poison_t)
    wab = np.zeros((M * S, 3, nb))
    wg0 = np.zeros((M * S, n_ant, 2))
    wn = np.zeros((M * S, nb), dtype=np.int32)
    c4 = lambda x: (x[0] + x[1]) + (x[2] + x[3])
    for m in range(M):
        for s, (ta, tb) in enumerate(iv):
            if mistake == "range_off_by_one":
                tb = min(tb + 1, T)
            Dm, Mm = D[m, ta:tb], Mod[0 if Mod.shape[0] == 1 else m, ta:tb]
            wm = None if w is None else w[0 if w.shape[0] == 1 else m, ta:tb]
            ok = counting(Dm, Mm, wm)
            ar, ai, b = np.zeros(nb), np.zeros(nb), np.zeros(nb)
            with np.errstate(all="ignore"):
                for t in range(tb - ta):
                    o = ok[t]
                    wt = np.ones(nb) if (wm is None or mistake == "no_weight") else wm[t]
                    dr, di, mr, mi = Dm[t].real, Dm[t].imag, Mm[t].real, Mm[t].imag
                    ar = np.where(o, ar + wt * (dr * mr + di * mi), ar)
                    ai = np.where(o, ai + wt * (di * mr - dr * mi), ai)
                    b = np.where(o, b + wt * (mr * mr + mi * mi), b)
            ms = m * S + s
            wab[ms], wn[ms] = (ar, ai, b), ok.sum(axis=0)
            nvis[m, s] = ok.sum()
            A, B = full(ar + 1j * ai, n_ant, mistake != "aqp_not_conj"), full(b, n_ant, False)
            live = live_set(B > 0, n_ant, min_bl)
            g = gains[m, s].copy()
            bad0 = live & ~(np.isfinite(g.real) & np.isfinite(g.imag) & (g != 0))
            if live.sum() < (3 if mode == 0 else 2) or bad0.any():
                gains[m, s] = np.nan + 1j * np.nan
                status[m, s] = 3
                continue
            wg0[ms, :, 0], wg0[ms, :, 1] = g.real, g.imag
            livo[m, s] = live
            g0 = g.copy()
            st, it = 0, 0
            for k in range(1, n_iter + 1):
                gq = np.conj(g) if mistake == "gq_not_conj" else g
                nr, ni, dn = np.zeros((4, n_ant)), np.zeros((4, n_ant)), np.zeros((4, n_ant))
                with np.errstate(all="ignore"):
                    for qq in range(n_ant):
                        if not live[qq]:
                            continue
                        use = live & (np.arange(n_ant) != qq)
                        j = qq % 4
                        a_r, a_i = A[:, qq].real, A[:, qq].imag
                        nr[j] = np.where(use, (nr[j] + gq[qq].real * a_r) - gq[qq].imag * a_i, nr[j])
                        ni[j] = np.where(use, (ni[j] + gq[qq].real * a_i) + gq[qq].imag * a_r, ni[j])
                        dn[j] = np.where(use, dn[j] + (g[qq].real ** 2 + g[qq].imag ** 2) * B[:, qq], dn[j])
                    numr, numi = c4(nr), c4(ni)
                    div = c4(dn) if mode == 0 else np.sqrt(numr * numr + numi * numi)
                    hr, hi = numr / div, numi / div
                okp = ~live | (np.isfinite(div) & (div > 0) & np.isfinite(hr) & np.isfinite(hi))
                if not okp.all():
                    st, it = 2, k - 1
                    break
                h = hr + 1j * hi
                avg = (k % 2 == 0) != (mistake == "avg_odd")
                gn = np.where(live, 0.5 * (h + g) if avg else h, g)
                d = np.abs((gn - g)[live]).max()
                gm = np.abs(gn[live]).max()
                g = gn
                trace[m, s, k - 1] = np.where(live, g, np.nan + 1j * np.nan)
                it = k
                if d <= tol * gm:
                    st = 1
                    break
            r = refant if live[refant] else int(np.nonzero(live)[0][0])
            c = (g[r] if mistake == "ref_sign" else np.conj(g[r])) / abs(g[r])
            gr = g * c
            gr[r] = gr[r].real + 0j
            gains[m, s] = np.where(live, gr, np.nan + 1j * np.nan)
            niter[m, s], status[m, s] = it, st
            for j, gg in enumerate((g0, gains[m, s])):
                gl = np.where(live, gg, 0)
                cc = gl[p] * np.conj(gl[q])
                okl = ok & (live[p] & live[q])[None, :]
                with np.errstate(all="ignore"):
                    e = np.where(okl, Dm - cc[None, :] * Mm, 0)
                    wt = 1.0 if (wm is None or mistake == "no_weight") else np.where(okl, wm, 0)
                    chi2[m, s, j] = (wt * (e.real ** 2 + e.imag ** 2)).sum()
    work = np.concatenate([wab.reshape(-1).view(np.uint8), wg0.reshape(-1).view(np.uint8),
                           wn.reshape(-1).view(np.uint8)])
    return dict(gains=gains, chi2=chi2, nvis=nvis, niter=niter, status=status, live=livo, trace=trace,
                work=work)
