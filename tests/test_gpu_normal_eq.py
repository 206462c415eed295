"""rjp_normal_eq (K23, normal_eq.hip: the normal equations of a fit from data, model and derivative
stacks) through the raw C-ABI and RTEngine, against tests/normal_eq_ref.py -- a long-double NumPy
restatement of the definition that judges every entry at a DERIVED bound (its docstring), which
tests/test_normal_eq_reference_cpu.py pins to hand-worked cases, to a float64 emulation on these
very inputs (inside the bound) and to planted mistakes (outside).

Every raw call runs with guard bands around every buffer (their payloads 8 bytes off a 16-byte
line) and poisoned outputs.  The module prints the worst error / bound."""
import ctypes

import numpy as np
import pytest

from tests import normal_eq_ref as K

pytestmark = pytest.mark.gpu
WORST = {}
P_F, P_I, P_W = 7.25, -77, 0xA5
GUARD = 33                             # odd: the payload of a float64 buffer starts 8 bytes off a 16-byte line


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()
    print("\nworst error / bound per group: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


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


def parts(z, n_part):
    """complex [...] -> float64 [..., 2]; real stays"""
    if n_part == 1:
        return np.ascontiguousarray(z, dtype=np.float64)
    z = np.asarray(z, dtype=np.complex128)
    return np.ascontiguousarray(np.stack([z.real, z.imag], axis=-1))


def i32(a):
    return (ctypes.c_int32 * max(1, len(a)))(*[int(x) for x in a])


def run(eng, case, guard=GUARD, poison=P_W):
    """One raw rjp_normal_eq call on a case of tests/normal_eq_ref.py, every buffer between guard
    bands, the workspace filled with `poison` beforehand -> dict(chi2, g, N, count, raw)."""
    import torch
    f64 = torch.float64
    n_part, sel, w = case["n_part"], case["sel"], case["w"]
    R, V = case["data"].shape
    P = len(sel)
    db = Band(eng, R * V * n_part, f64, -1e300, guard).set(parts(case["data"], n_part))
    mb = Band(eng, R * V * n_part, f64, -1e300, guard).set(parts(case["model"], n_part))
    jb = None
    if case["dmodel"] is not None:
        jb = Band(eng, case["dmodel"].size * n_part, f64, -1e300, guard).set(parts(case["dmodel"], n_part))
    wb = Band(eng, w.size, f64, -1e300, guard).set(w) if w is not None else None
    ob = Band(eng, K.n_out(P), f64, P_F, guard)
    cb = Band(eng, 1, torch.int64, P_I, guard)
    need = eng.lib.rjp_normal_eq_workspace(R, V, P)
    assert need == K.workspace_bytes(R, V, P)
    kb = Band(eng, need, torch.uint8, poison, guard * 8)
    w_rows = 1 if w is None or w.ndim == 1 else R
    ret = eng.lib.rjp_normal_eq(eng.ctx, db.ptr, mb.ptr, jb.ptr if jb else None, R, V, n_part, case["n_par"],
                                i32(sel), P, wb.ptr if wb else None, w_rows, ob.ptr, cb.ptr, kb.ptr, need,
                                eng._stream())
    eng.synchronize()
    assert ret == K.workgroups(R, V), (ret, eng.lib.rjp_last_error(eng.ctx))
    for band, host in ((db, case["data"]), (mb, case["model"]), (jb, case["dmodel"])):
        if band is not None:
            assert band.get().tobytes() == parts(host, n_part).tobytes(), "an input was written"
    kb.get()
    out = ob.get()
    return dict(chi2=out[0], g=out[1:1 + P], N=out[1 + P:], count=int(cb.get()[0]), raw=out.tobytes())


@pytest.mark.parametrize("n_rows,n_vis,n_part,n_sel,n_par,wkind", K.SIZED)
def test_the_sized_cases_between_guard_bands(eng, n_rows, n_vis, n_part, n_sel, n_par, wkind):
    """Entry by entry at the derived bound; the count exact; every output finite although every
    sample that does not count carries NaN derivatives and a NaN model; the same bits on a repeated
    call, with other guard bands and with the workspace poisoned differently."""
    case = K.sized(n_rows, n_vis, n_part, n_sel, n_par, wkind)
    ref = K.reference(case)
    got = run(eng, case)
    note("sized n_part %d" % n_part, K.judge(got, ref, n_part))
    assert np.all(np.isfinite(got["g"])) and np.all(np.isfinite(got["N"])) and np.isfinite(got["chi2"])
    if n_rows * n_vis > 1:
        assert 0 < got["count"] < n_rows * n_vis, "the case would be vacuous"
    assert run(eng, case)["raw"] == got["raw"], "a repeated call gave other bits"
    assert run(eng, case, guard=GUARD + 2, poison=0x00)["raw"] == got["raw"], "the workspace's content entered"


def test_a_sum_does_not_depend_on_what_else_is_selected(eng):
    """The value of a sum depends on the inputs and the tile size alone: the entries of planes (a,
    b) have the same bits whether 2, 9, 20 or 40 planes are selected (four instantiations)."""
    base = K.sized(3, 700, 2, 40, 44, "rows")
    full = run(eng, base)
    P = 40
    tl = K.tri_list(P)
    for n in (2, 9, 20):
        sub = run(eng, dict(base, sel=base["sel"][:n]))
        assert sub["chi2"].tobytes() == full["chi2"].tobytes()
        assert sub["g"].tobytes() == full["g"][:n].tobytes()
        want = np.array([full["N"][tl.index(pq)] for pq in K.tri_list(n)])
        assert sub["N"].tobytes() == want.tobytes()


def test_a_counting_sample_with_a_nan_derivative(eng):
    """Exactly the entries that touch that plane are NaN; the others keep their bound."""
    case, j = K.nan_plane()
    got = run(eng, case)
    tg, tN = K.touches(len(case["sel"]), j)
    assert np.array_equal(np.isnan(got["g"]), tg) and np.array_equal(np.isnan(got["N"]), tN)
    assert np.isfinite(got["chi2"])
    note("nan plane", K.judge(got, K.reference(case), 2))


def test_nothing_counts(eng):
    case = K.sized(2, 40, 2, 3, 5, "rows")
    case["data"][:] = np.nan
    got = run(eng, case)
    assert got["count"] == 0 and got["chi2"] == 0.0 and not got["g"].any() and not got["N"].any()


def test_engine_normal_eq(eng):
    """RTEngine.normal_eq on device tensors: complex and real stacks, shared and per-row weights,
    the bits of the raw call."""
    import torch
    for c in ((3, 513, 2, 47, 48, "rows"), (4, 1573, 1, 3, 6, "rows"), (2, 511, 2, 1, 4, "shared"),
              (5, 513, 2, 0, 3, "shared")):
        case = K.sized(*c)
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
        chi2, g, N, count = eng.normal_eq(dev(case["data"]), dev(case["model"]), dev(case["dmodel"]),
                                          case["sel"], dev(case["w"]))
        assert eng.last_normal_eq_workgroups == K.workgroups(c[0], c[1])
        raw = run(eng, case)
        assert float(chi2) == raw["chi2"] and int(count) == raw["count"]
        assert g.cpu().numpy().tobytes() == raw["g"].tobytes() and N.cpu().numpy().tobytes() == raw["N"].tobytes()
    with pytest.raises(ValueError):
        eng.normal_eq(dev(case["data"]), dev(case["model"]), dev(case["dmodel"]), [0, 0])
    with pytest.raises(ValueError):
        eng.normal_eq(dev(case["data"]), dev(case["model"]), dev(case["dmodel"]), [3])
    with pytest.raises(ValueError):
        eng.normal_eq(dev(case["data"]), dev(case["model"][:2]), None, [])


def test_every_refusal_leaves_the_outputs_untouched(eng):
    import torch
    from rajepy_amd import _lib
    case = K.sized(3, 40, 2, 3, 6, "rows")
    f64 = torch.float64
    R, V, P = 3, 40, 3
    db = Band(eng, R * V * 2, f64, -1e300).set(parts(case["data"], 2))
    mb = Band(eng, R * V * 2, f64, -1e300).set(parts(case["model"], 2))
    jb = Band(eng, R * 6 * V * 2, f64, -1e300).set(parts(case["dmodel"], 2))
    wb = Band(eng, R * V, f64, -1e300).set(case["w"])
    ob = Band(eng, K.n_out(48), f64, P_F)
    cb = Band(eng, 1, torch.int64, P_I)
    need = K.workspace_bytes(R, V, 48)
    kb = Band(eng, need, torch.uint8, P_W, GUARD * 8)        # (the workspace holds 8-byte words)
    good = dict(ctx=eng.ctx, data=db.ptr, model=mb.ptr, dmodel=jb.ptr, n_rows=R, n_vis=V, n_part=2, n_par=6,
                sel=[4, 0, 5], n_sel=3, w=wb.ptr, w_rows=R, out=ob.ptr, count=cb.ptr, work=kb.ptr, nbytes=need)

    def call(**kw):
        a = dict(good, **kw)
        sel = None if a["sel"] is None else i32(a["sel"])
        return eng.lib.rjp_normal_eq(a["ctx"], a["data"], a["model"], a["dmodel"], a["n_rows"], a["n_vis"],
                                     a["n_part"], a["n_par"], sel, a["n_sel"], a["w"], a["w_rows"], a["out"],
                                     a["count"], a["work"], a["nbytes"], eng._stream())

    assert call(ctx=None) == _lib.RJP_ERR_ARG
    bad = [("null", dict(data=None)), ("null", dict(model=None)), ("null", dict(out=None)),
           ("null", dict(count=None)), ("count", dict(n_rows=0)), ("count", dict(n_vis=0)),
           ("part", dict(n_part=0)), ("part", dict(n_part=3)), ("nsel", dict(n_sel=-1)),
           ("nsel", dict(n_sel=49, n_par=60)), ("needs", dict(dmodel=None)), ("needs", dict(sel=None)),
           ("npar", dict(n_par=2)), ("range", dict(sel=[4, -1, 5])), ("range", dict(sel=[4, 6, 5])),
           ("repeat", dict(sel=[4, 0, 4])), ("wrows", dict(w_rows=0)), ("wrows", dict(w_rows=2)),
           ("wgs", dict(n_rows=(2 ** 31 - 1) * 512 + 1, n_vis=1, w=None))]
    for key, kw in bad:
        assert call(**kw) == _lib.RJP_ERR_ARG, (key, kw)
        assert eng.lib.rjp_last_error(eng.ctx).decode() == K.MSG[key], (key, kw)
    for kw in (dict(work=None), dict(nbytes=K.workspace_bytes(R, V, 3) - 1)):
        assert call(**kw) == _lib.RJP_ERR_WORKSPACE
        assert eng.lib.rjp_last_error(eng.ctx).decode() == K.MSG["work"]
    assert eng.lib.rjp_normal_eq_workspace(0, 5, 3) == 0 and eng.lib.rjp_normal_eq_workspace(5, 5, 49) == 0
    assert eng.lib.rjp_normal_eq_workspace(5, 0, 3) == 0 and eng.lib.rjp_normal_eq_workspace(2 ** 40, 2 ** 20, 3) == 0
    eng.synchronize()
    assert np.all(ob.get() == P_F) and cb.get()[0] == P_I and np.all(kb.get() == P_W)
    # and the same buffers take a valid call afterwards
    assert call() == K.workgroups(R, V)
    eng.synchronize()
    assert cb.get()[0] == K.reference(dict(case, sel=[4, 0, 5]))["count"]
