"""rjp_gain_apply and rjp_gaincal (K22, gaincal.hip: antenna-based complex gains -- corrupt,
gaincal, applycal) through the C-ABI, RTEngine and JetModel, against tests/gaincal_ref.py -- a
long-double NumPy reference that judges every visibility of an apply and FOLLOWS the device's trace
of every solve (checks (a)-(f) of its docstring, every bound derived there, none measured), which
tests/test_gaincal_reference_cpu.py pins to hand-worked cases, to a float64 emulation on these very
inputs (tests/gaincal_cases.py: inside the bounds, and converging where convergence is asked here)
and to planted mistakes (outside).

Every raw call runs with guard bands around every buffer and poisoned outputs.  The 1e-9 on the
noise-free solves comes from tol = 1e-12 and the linear rate the CPU emulation observed (its own
error on every case is below 1e-10: asserted on the CPU).  The module prints the worst error /
bound per group."""
import copy
import ctypes
import os

import numpy as np
import pytest

from tests import gaincal_cases as C
from tests import gaincal_ref as K
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
YEAR = 31557600.0
WORST = {}
P_F, P_I, P_T, P_L = 7.25, -77, -7.5, 0xA5
GUARD = 33                             # elements of guard band on either side (odd: the payload of a
                                       # float64 buffer then starts 8 bytes off a 16-byte line)
FIXTURE = os.path.join(U.GOLDEN, "antenna_configs", "vla.a.cfg")
KEYS = ("gains", "chi2", "nvis", "niter", "status", "live", "trace")


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()
    print("\nworst error / bound per group: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    print("worst share per check: " + ", ".join("%s %.3f" % kv for kv in sorted(K.PARTS.items())))


def note(kind, r):
    WORST[kind] = max(WORST.get(kind, 0.0), float(r))
    assert r <= 1.0, (kind, r)


class Band:
    """A device buffer of `n` elements between two guard bands of `guard` poisoned elements."""

    def __init__(self, eng, n, dtype, fill, guard=GUARD):
        import torch
        self.t = torch.full((guard + n + guard,), fill, dtype=dtype, device=eng.device)
        self.n, self.g, self.fill = n, guard, fill
        self.ptr = self.t.data_ptr() + guard * self.t.element_size()

    def set(self, host):
        import torch
        self.t[self.g:self.g + self.n] = torch.from_numpy(np.ascontiguousarray(host).ravel()).to(self.t.device)
        return self

    def get(self):
        h = self.t.cpu().numpy()
        for band in (h[:self.g], h[self.g + self.n:]):
            assert np.array_equal(band, np.full(band.shape, self.fill, dtype=h.dtype)), "a guard band was written"
        return h[self.g:self.g + self.n].copy()


def ri(z):
    """complex [...] -> float64 [..., 2]"""
    z = np.asarray(z, dtype=np.complex128)
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))


def cx(a):
    return a[..., 0] + 1j * a[..., 1]


def i32(a):
    return (ctypes.c_int32 * len(a))(*[int(x) for x in a])


def run_apply(eng, V, gains, h_sol, n_ant, mode, guard=GUARD, in_place=False):
    """One raw rjp_gain_apply call, every buffer between guard bands -> complex [M, T, n_bl]."""
    import torch
    M, T, nb = V.shape
    G, S = gains.shape[0], gains.shape[1]
    vb = Band(eng, V.size * 2, torch.float64, -1e300, guard).set(ri(V))
    gb = Band(eng, gains.size * 2, torch.float64, -1e300, guard).set(ri(gains))
    ob = vb if in_place else Band(eng, V.size * 2, torch.float64, P_F, guard)
    ret = eng.lib.rjp_gain_apply(eng.ctx, vb.ptr, M, T, n_ant, gb.ptr, G, i32(h_sol), S, mode, ob.ptr,
                                 eng._stream())
    eng.synchronize()
    assert ret == K.apply_workgroups(M, T, n_ant), (ret, eng.lib.rjp_last_error(eng.ctx))
    assert gb.get().tobytes() == ri(gains).tobytes(), "the gains were written"
    if not in_place:
        assert vb.get().tobytes() == ri(V).tobytes(), "the visibilities were written"
    return cx(ob.get().reshape(M, T, nb, 2))


def run_gaincal(eng, case, g_start=None, n_iter=None, want_trace=True, guard=GUARD):
    """One raw rjp_gaincal call on a case of tests/gaincal_cases.py, every buffer between guard
    bands, the outputs poisoned -> the `out` of gaincal_ref.follow (host arrays), plus `ret`."""
    import torch
    f64, i32t, u8 = torch.float64, torch.int32, torch.uint8
    D, Mod, w = case["D"], case["Mod"], case["w"]
    M, T, nb = D.shape
    n_ant = case["n_ant"]
    n_iter = case["n_iter"] if n_iter is None else n_iter
    S = int(case["h_sol"][-1]) + 1
    g0 = case["g_start"] if g_start is None else g_start
    db = Band(eng, D.size * 2, f64, -1e300, guard).set(ri(D))
    mb = Band(eng, Mod.size * 2, f64, -1e300, guard).set(ri(Mod))
    wb = Band(eng, w.size, f64, -1e300, guard).set(w) if w is not None else None
    gb = Band(eng, M * S * n_ant * 2, f64, P_F, guard).set(ri(g0))
    chi2 = Band(eng, M * S * 2, f64, P_F, guard)
    nvis, niter, status = (Band(eng, M * S, i32t, P_I, guard) for _ in range(3))
    live = Band(eng, M * S * n_ant, u8, P_L, guard)
    trace = Band(eng, M * S * n_iter * n_ant * 2, f64, P_T, guard)
    nbytes = eng.lib.rjp_gaincal_workspace(M, S, n_ant)
    assert nbytes == K.workspace_bytes(M, S, n_ant)
    work = Band(eng, nbytes, u8, 0x5A, 64)
    ret = eng.lib.rjp_gaincal(eng.ctx, db.ptr, M, T, n_ant, mb.ptr, Mod.shape[0], wb.ptr if wb else None,
                              w.shape[0] if w is not None else 1, i32(case["h_sol"]), S, case["mode"],
                              case["refant"], case["min_bl"], case["tol"], n_iter, gb.ptr, chi2.ptr, nvis.ptr,
                              niter.ptr, status.ptr, live.ptr, trace.ptr if want_trace else None, work.ptr,
                              nbytes, eng._stream())
    eng.synchronize()
    assert ret == K.gaincal_workgroups(M, S, n_ant), (ret, eng.lib.rjp_last_error(eng.ctx))
    assert db.get().tobytes() == ri(D).tobytes() and mb.get().tobytes() == ri(Mod).tobytes(), "inputs written"
    if wb:
        assert wb.get().tobytes() == np.ascontiguousarray(w).tobytes()
    return dict(gains=cx(gb.get().reshape(M, S, n_ant, 2)), chi2=chi2.get().reshape(M, S, 2),
                nvis=nvis.get().reshape(M, S), niter=niter.get().reshape(M, S), status=status.get().reshape(M, S),
                live=live.get().reshape(M, S, n_ant), trace=cx(trace.get().reshape(M, S, n_iter, n_ant, 2)),
                work=work.get(), ret=ret)


def follow(kind, case, out, g_start=None, n_iter=None):
    c = dict(case)
    if g_start is not None:
        c["g_start"] = g_start
    if n_iter is not None:
        c["n_iter"] = n_iter
    note(kind, K.follow(c, out, P_F, P_I, P_T, P_L))


def same_bits(a, b, keys=KEYS):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), "a second call changed " + k


def demand_convergence(case, out):
    st = out["status"]
    assert np.all((st == 1) | (st == 3)), st
    assert C.recovered(case, out["gains"]) <= 1e-9


# ---- 1: the solve ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,n_t,sol,M,MM,wkind,mode", C.SIZED)
def test_sized_cases_follow_the_reference_and_recover_the_planted_gains(eng, n_ant, n_t, sol, M, MM, wkind, mode):
    """2 (phase only), 3, 4, 5, 7, 27 and 64 antennas, 1 to 257 integrations, n_sol = 1, n_t and
    uneven, 1-3 maps, the model shared and per map, weights none / shared / per map, 30 % of the
    longest case flagged (NaN and inf data, NaN and zero model, zero and negative weights); every
    base 8 bytes off a 16-byte boundary, and once more 16 bytes on; identical bits on a repeated
    call and without the trace."""
    case = C.sized(n_ant, n_t, sol, M, MM, wkind, mode)
    out = run_gaincal(eng, case)
    follow("sized", case, out)
    demand_convergence(case, out)
    same_bits(out, run_gaincal(eng, case))
    same_bits(out, run_gaincal(eng, case, guard=GUARD + 1))
    bare = run_gaincal(eng, case, want_trace=False)
    same_bits(out, bare, KEYS[:-1])
    assert np.all(bare["trace"].real == P_T) and np.all(bare["trace"].imag == P_T)


@pytest.mark.parametrize("name", C.NAMED)
def test_named_cases(eng, name):
    """An antenna wholly flagged in one interval only; the min_bl cascade that removes two antennas;
    an interval with nothing counting; start gains of 0 and NaN; a denominator that underflows to 0;
    n_iter exhausted, and the continued call."""
    case = C.named(name)
    out = run_gaincal(eng, case)
    follow(name, case, out)
    st = out["status"]
    if case["converges"]:
        demand_convergence(case, out)
    if name == "dead antenna":
        assert np.all(st == 1)
        dead = np.isnan(out["gains"].real)
        want = np.zeros_like(dead)
        want[:, 1, 2] = True
        assert np.array_equal(dead, want) and np.array_equal(out["live"] == 0, want)
    elif name == "cascade":
        assert out["live"][0, 0].tolist() == [1, 1, 1, 0, 0] and st[0, 0] == 1
    elif name == "empty interval":
        assert st[1, 0] == 3 and out["nvis"][1, 0] == 0 and (st == 3).sum() == 1
    elif name == "bad start":
        assert st[0].tolist() == [3, 1, 3]
    elif name == "den zero":
        assert st[0, 0] == 2 and out["niter"][0, 0] == 0
    elif name == "exhausted":
        assert np.all(st == 0) and np.all(out["niter"] == 5)
        more = run_gaincal(eng, case, g_start=out["gains"], n_iter=C.N_ITER)
        follow(name, case, more, g_start=out["gains"], n_iter=C.N_ITER)
        demand_convergence(case, more)
    same_bits(out, run_gaincal(eng, case))


def test_a_solution_does_not_depend_on_its_place(eng):
    """An interval alone, among the others, and in another map slot: the same bits."""
    case = C.sized(27, 33, "uneven", 2, 1, "shared", 0)
    whole = run_gaincal(eng, case)
    iv = K.intervals(case["h_sol"])
    s = 5
    ta, tb = iv[s]
    alone = dict(case, D=case["D"][:1, ta:tb], Mod=case["Mod"][:, ta:tb], w=case["w"][:, ta:tb],
                 h_sol=np.zeros(tb - ta, dtype=np.int32), g_start=case["g_start"][:1, s:s + 1])
    a = run_gaincal(eng, alone)
    follow("placement", alone, a)
    moved = dict(alone, D=np.concatenate([case["D"][1:, ta:tb], case["D"][:1, ta:tb]]),
                 g_start=np.ones((2, 1, 27), dtype=np.complex128))
    b = run_gaincal(eng, moved)
    for k in KEYS:
        assert a[k][0, 0].tobytes() == whole[k][0, s].tobytes() == b[k][1, 0].tobytes(), k


# ---- 2: apply -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ant,n_t,M,G", [(2, 1, 1, 1), (5, 7, 3, 1), (27, 9, 2, 2), (64, 3, 1, 1)])
def test_gain_apply_per_visibility(eng, n_ant, n_t, M, G):
    """Corrupt and correct against the reference at its bound per visibility; NaN gains and NaN
    visibilities flag; in place; corrupt then correct returns the data within the apply bound."""
    rng = np.random.default_rng(n_ant)
    h_sol = C.table("uneven", n_t)
    S, nb = int(h_sol[-1]) + 1, K.n_bl(n_ant)
    gains = C.planted_gains(rng, G, S, n_ant, 0, 0)
    V = C.model(rng, M, n_t, nb)
    if n_ant > 2:
        gains[0, 0, 1] = np.nan
        V[0, 0, nb - 1] = np.nan + 1j
        gains[G - 1, S - 1, 2] = 0.0                              # correcting by it: 0 / 0
    p, q = K.pairs(n_ant)
    for mode in (0, 1):
        out = run_apply(eng, V, gains, h_sol, n_ant, mode)
        note("apply", K.check_apply(V, gains, h_sol, n_ant, mode, out))
        assert run_apply(eng, V, gains, h_sol, n_ant, mode, in_place=True).tobytes() == out.tobytes()
        assert run_apply(eng, V, gains, h_sol, n_ant, mode, guard=GUARD + 1).tobytes() == out.tobytes()
    there = run_apply(eng, V, gains, h_sol, n_ant, 0)
    back = run_apply(eng, there, gains, h_sol, n_ant, 1)
    for m in range(M):
        g = gains[0 if G == 1 else m][h_sol]
        _, b0 = K.apply_ref(V[m], g[:, p], g[:, q], 0)
        _, b1 = K.apply_ref(there[m], g[:, p], g[:, q], 1)
        with np.errstate(all="ignore"):
            bound = 2 * b0 / abs(g[:, p] * np.conj(g[:, q])) + b1
            ok = np.isfinite(back[m].real) & np.isfinite(bound)
            err = np.maximum(abs(back[m].real - V[m].real), abs(back[m].imag - V[m].imag))
        assert ok.sum() >= (V[m].size * 3) // 5
        note("round trip", float((err[ok] / bound[ok]).max()))


def test_applycal_with_the_solved_gains_brings_chi2_down(eng):
    """The data corrected by the solved gains, solved once more from unit gains: chi^2 at the start
    of that call is the residual of the corrected data, held to the reference like any chi^2, and
    is at rounding level of sum w |M|^2."""
    case = C.sized(27, 33, "uneven", 2, 1, "shared", 0)
    out = run_gaincal(eng, case)
    fixed = run_apply(eng, case["D"], out["gains"], case["h_sol"], 27, 1)
    again = dict(case, D=fixed)
    out2 = run_gaincal(eng, again)
    follow("applycal", again, out2)
    scale = (case["w"] * abs(case["Mod"]) ** 2).sum() / out2["chi2"].shape[1]
    assert np.all(out2["chi2"][..., 0] <= 1e-18 * scale) and np.all(out2["chi2"][..., 0] < out["chi2"][..., 0])
    assert np.all(out2["status"] == 1)


# ---- 3: refusals --------------------------------------------------------------------------------------
def test_every_refusal_with_its_message(eng):
    import torch
    from rajepy_amd import _lib
    n_ant, T, M = 4, 3, 2
    nb = K.n_bl(n_ant)
    f64 = torch.float64
    vis = Band(eng, M * T * nb * 2, f64, 1.0)
    g = Band(eng, M * T * n_ant * 2, f64, P_F)
    outb = Band(eng, M * T * nb * 2, f64, P_F)
    chi2 = Band(eng, M * T * 2, f64, P_F)
    ints = [Band(eng, M * T, torch.int32, P_I) for _ in range(3)]
    live = Band(eng, M * T * n_ant, torch.uint8, P_L)
    nbytes = eng.lib.rjp_gaincal_workspace(M, T, n_ant)
    work = Band(eng, nbytes, torch.uint8, 0x5A)
    sol = [0, 1, 2]
    A = dict(vis=vis.ptr, M=M, T=T, n_ant=n_ant, g=g.ptr, G=1, sol=i32(sol), S=3, mode=0, out=outb.ptr)

    def apply_(key, code=_lib.RJP_ERR_ARG, **kw):
        a = dict(A, **kw)
        ret = eng.lib.rjp_gain_apply(eng.ctx, a["vis"], a["M"], a["T"], a["n_ant"], a["g"], a["G"], a["sol"],
                                     a["S"], a["mode"], a["out"], eng._stream())
        assert ret == code, (key, kw, ret)
        assert eng.lib.rjp_last_error(eng.ctx).decode() == K.MSG_A[key], (key, kw)

    for kw in (dict(vis=None), dict(g=None), dict(sol=None), dict(out=None)):
        apply_("nulls", **kw)
    for kw in (dict(M=0), dict(T=0), dict(S=0), dict(M=-1)):
        apply_("sizes", **kw)
    for kw in (dict(n_ant=1), dict(n_ant=65)):
        apply_("ant", **kw)
    for kw in (dict(sol=i32([1, 1, 2])), dict(sol=i32([0, 2, 2])), dict(sol=i32([0, 1, 0])), dict(S=2), dict(S=4)):
        apply_("sol", **kw)
    for kw in (dict(G=0), dict(G=3)):
        apply_("maps", **kw)
    for kw in (dict(mode=2), dict(mode=-1)):
        apply_("mode", **kw)
    apply_("wgs", M=2 ** 28, n_ant=64)

    Gc = dict(vis=vis.ptr, M=M, T=T, n_ant=n_ant, mod=vis.ptr, MM=1, w=None, WM=1, sol=i32(sol), S=3, mode=0,
              refant=0, min_bl=1, tol=1e-10, n_iter=5, g=g.ptr, chi2=chi2.ptr, nvis=ints[0].ptr,
              niter=ints[1].ptr, status=ints[2].ptr, live=live.ptr, trace=None, work=work.ptr, nbytes=nbytes)

    def cal(key, code=_lib.RJP_ERR_ARG, **kw):
        a = dict(Gc, **kw)
        ret = eng.lib.rjp_gaincal(eng.ctx, a["vis"], a["M"], a["T"], a["n_ant"], a["mod"], a["MM"], a["w"],
                                  a["WM"], a["sol"], a["S"], a["mode"], a["refant"], a["min_bl"], a["tol"],
                                  a["n_iter"], a["g"], a["chi2"], a["nvis"], a["niter"], a["status"], a["live"],
                                  a["trace"], a["work"], a["nbytes"], eng._stream())
        assert ret == code, (key, kw, ret)
        assert eng.lib.rjp_last_error(eng.ctx).decode() == K.MSG_G[key], (key, kw)

    for k in ("vis", "mod", "sol", "g", "chi2", "nvis", "niter", "status", "live"):
        cal("nulls", **{k: None})
    for kw in (dict(M=0), dict(T=-2), dict(S=0)):
        cal("sizes", **kw)
    for kw in (dict(n_ant=1), dict(n_ant=65)):
        cal("ant", **kw)
    for kw in (dict(sol=i32([0, 0, 2])), dict(S=2)):
        cal("sol", **kw)
    for kw in (dict(MM=0), dict(MM=3)):
        cal("mmaps", **kw)
    for kw in (dict(w=vis.ptr, WM=0), dict(w=vis.ptr, WM=3)):
        cal("wmaps", **kw)
    cal("mode", mode=2)
    for kw in (dict(refant=-1), dict(refant=4)):
        cal("refant", **kw)
    cal("minbl", min_bl=0)
    for kw in (dict(tol=0.0), dict(tol=-1.0), dict(tol=float("inf")), dict(tol=float("nan"))):
        cal("tol", **kw)
    cal("iter", n_iter=0)
    cal("wgs", M=2 ** 29)
    for kw in (dict(work=None), dict(nbytes=nbytes - 1), dict(nbytes=0)):
        cal("work", code=_lib.RJP_ERR_WORKSPACE, **kw)
    assert eng.lib.rjp_gaincal_workspace(0, 1, 4) == 0 and eng.lib.rjp_gaincal_workspace(1, 1, 65) == 0
    eng.synchronize()
    # nothing was touched
    for b in [g, outb, chi2, live, work] + ints:
        h = b.get()
        assert np.array_equal(h, np.full(h.shape, b.fill, dtype=h.dtype))
    # and the arguments as they stand are taken
    cal_ok = dict(Gc)
    g.set(ri(np.ones((M, T, n_ant))))
    ret = eng.lib.rjp_gaincal(eng.ctx, cal_ok["vis"], M, T, n_ant, cal_ok["mod"], 1, None, 1, cal_ok["sol"], 3, 0, 0,
                              1, 1e-10, 5, g.ptr, chi2.ptr, ints[0].ptr, ints[1].ptr, ints[2].ptr, live.ptr, None,
                              work.ptr, nbytes, eng._stream())
    eng.synchronize()
    assert ret == K.gaincal_workgroups(M, T, n_ant)
    assert np.all(ints[2].get() == 1) and np.all(ints[0].get() == nb)


# ---- 4: the chain ---------------------------------------------------------------------------------------
def _params(tag):
    p = copy.deepcopy(U.load_golden(tag)[2])
    p["geometry"].pop("mod_r_0", None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


T_OBS, T_INT, MIN_EL = 600., 60., 20.


def dynamic_range(res):
    return float(np.max(np.abs(res.image)) / np.sqrt(np.mean(res.residual ** 2)))


def test_the_chain_on_the_example_model(eng, tmp_path):
    """The golden example model with the 27-antenna fixture: `observe_ff` without noise,
    `corrupt_gains` with seeded 30 degree rms phases per antenna and integration; `gaincal` against
    `visibilities_ff` recovers the planted gains to 1e-9 (the float64 emulation on the device's own
    visibilities converges: asserted first); `selfcal_ff` with two phase rounds lowers every
    converged solution's chi^2 and ends with a smaller peak residual than the corrupted data's
    CLEAN.  The dynamic ranges are printed, not asserted beyond "better than corrupted"."""
    from rajepy_amd import classes, logger
    from rajepy_amd import engine as E
    jm = classes.JetModel(_params("cfg1_example"), log=logger.Log(str(tmp_path / "model.log"), verbose=False),
                          engine=eng)
    jm.time = 1.0 * YEAR
    freqs = np.array([4.9e9, 5.1e9])
    tr = jm.uv_tracks(FIXTURE, T_OBS, T_INT, min_el_deg=MIN_EL)
    n_t, n_ant = len(tr.ha_h), 27
    cell_as = E.observation_grid(tr.max_baseline_m, 5e9, 1.0)[0]
    kw = dict(shape=(48, 40), cell_as=cell_as, niter=200)
    obs = jm.observe_ff(tr, freqs, T_OBS, T_INT, **kw)
    Vm = jm.visibilities_ff(tr.u_m, tr.v_m, freqs)
    h_sol = E.solution_intervals(tr.ha_h, tr.day, "int")
    assert h_sol.tolist() == list(range(n_t))
    planted = E.random_gains(n_t, n_ant, 0.0, 30.0, seed=5)
    Vc = jm.corrupt_gains(obs.vis, tr, planted, h_sol)
    assert Vc.is_cuda and tuple(Vc.shape) == (2, n_t * 351)
    nb = K.n_bl(n_ant)
    case = dict(D=Vc.cpu().numpy().reshape(2, n_t, nb), Mod=Vm.reshape(2, n_t, nb), w=None, h_sol=h_sol,
                n_ant=n_ant, mode=1, refant=0, min_bl=4, tol=1e-12, n_iter=300,
                g_start=np.ones((2, n_t, n_ant), dtype=np.complex128),
                planted=np.broadcast_to(planted, (2, n_t, n_ant)))
    emu = K.emulate(case)
    assert np.all(emu["status"] == 1), "the emulation does not converge: the case would be vacuous"
    gains, res = jm.gaincal(Vc, Vm, tr, solint_s="int", calmode="p", refant=0, tol=1e-12)
    assert gains.is_cuda and res["h_sol"].tolist() == h_sol.tolist()
    assert bool((res["status"] == 1).all()) and bool(res["live"].all())
    rec = C.recovered(case, gains.cpu().numpy())
    print("\nthe chain: planted gains recovered to %.2e in at most %d steps" % (rec, int(res["niter"].max())))
    assert rec <= 1e-9
    back = jm.applycal(Vc, tr, gains, h_sol).cpu().numpy()
    assert np.nanmax(abs(back - obs.vis)) <= 1e-9 * np.nanmax(abs(obs.vis))
    # self-calibration: two phase rounds
    sc = jm.selfcal_ff(Vc, tr, freqs, rounds=[dict(solint_s="int", calmode="p"),
                                                dict(solint_s="int", calmode="p")], **kw)
    assert len(sc.history) == 2 and tuple(sc.gains.shape) == (2, n_t, n_ant) and sc.vis.is_cuda
    for h in sc.history:
        r = h["solutions"]
        done = (r["status"] == 1)
        assert bool(done.any()) and bool((r["chi2"][done] <= r["chi2_start"][done]).all())
    corrupted_peak = sc.history[0]["peak_residual"]
    final_peak = float(np.max(np.abs(sc.clean.peak_residual)))
    print("dynamic range: uncorrupted %.1f, corrupted %.1f, self-calibrated %.1f; peak residual %.3e -> %.3e"
          % (dynamic_range(obs.clean), sc.history[0]["dynamic_range"], dynamic_range(sc.clean),
             corrupted_peak, final_peak))
    assert final_peak < corrupted_peak
    assert dynamic_range(sc.clean) > sc.history[0]["dynamic_range"]
