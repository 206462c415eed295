"""The key rules of the derived state (DESIGN.md "Derived state"), driven alone: CPU torch tensors
have `data_ptr()` and `_version` like device ones, and a stub engine reports the path a sweep
"took".  No library is loaded and nothing runs on a GPU: what is checked is the bookkeeping of
rajepy_amd/engine.py -- which items `DeviceFields.struct()` and `RTEngine._attach_moment_cache`
hand to a scan, and what `_note_moment_sweep` / the range-guard report leave recorded."""
import types

import pytest
import torch

from rajepy_amd import _lib
from rajepy_amd import engine as E

N = 2 * 6 * 4


def _fields():
    t = lambda v: torch.full((N,), float(v), dtype=torch.float64)
    f = E.DeviceFields((2, 6, 4), E.RJP_F64, 0.5, None, None, t(1e4), None, ts=t(3.0))
    f.a0 = t(2.0)
    f.ts_range = (1.0, 5.0)
    f._ts_range_of = f.ts.data_ptr()
    return f


def _attach_lt(f, K=8):
    fs = f.struct()
    f.lt = {"cells": torch.zeros(4, dtype=torch.float64), "rowoff": torch.zeros(4, dtype=torch.int32),
            "aux": torch.zeros(4, dtype=torch.float64), "K": K,
            "key": E.lt_key(f.a0, f.ts, fs.ts_lo, fs.ts_hi)}
    return f.lt


class StubEngine(E.RTEngine):
    """RTEngine's bookkeeping without a context: `path` is what the "library" reports."""

    def __init__(self):
        self.cache_moments = self.use_moments = True
        self.device = torch.device("cpu")
        self.lib = types.SimpleNamespace(rjp_moment_cache_bytes=lambda nx, nz: 1280 * 8 * nx * nz)
        self.ctx = None
        self._unreported = {}
        self.path, self.shape = "moments", (53, 12)

    def last_scan_path(self):
        self.last_moment_shape = self.shape if self.path in ("moments", "cached", "lt") else (0, 0)
        return self.path, 0.0

    def close(self):
        pass

    def sweep(self, f, bursts, path, fail=None, n_epochs=16, want_em=False):
        """One ff_scan's worth of bookkeeping -> the struct the library would have been given."""
        fs = f.struct()
        mkey = self._attach_moment_cache(f, bursts, fs, n_epochs, want_em)
        if fail is not None:
            with pytest.raises(_lib.RjprtError):
                self._check(_lib.RJP_ERR_ARG, None, "rjp_ff_scan")
            return fs
        # (what the library does with the struct it was given)
        self.path = "cached" if (path == "moments" and fs.d_mom_cache and
                                 (fs.mom_cache_K, fs.mom_cache_N) == self.shape) else path
        if mkey is not None:
            self._note_moment_sweep(f, mkey)
        return fs


@pytest.fixture
def stub(monkeypatch):
    s = StubEngine()
    msg = {"text": "boom"}
    s.msg = msg

    def fake_check(status, ctx=None, what=""):
        if status != _lib.RJP_OK:
            raise _lib.RjprtError("%s failed (status %d): %s" % (what, status, msg["text"]), status)
    monkeypatch.setattr(_lib, "check", fake_check)
    return s


BOTH = types.SimpleNamespace(n=[2, 1])
RED = types.SimpleNamespace(n=[1, 0])
GUARD_TEXT = ("an earlier scan of this context met finite launch times outside fields.ts_lo / "
              "ts_hi: the sums of those sightlines were set to NaN")


# ---- the keys ---------------------------------------------------------------------------------
def test_keys_follow_pointer_and_version():
    a0, ts = torch.ones(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64)
    k0 = E.lt_key(a0, ts, 0.0, 1.0)
    assert k0 == E.lt_key(a0, ts, 0.0, 1.0)
    ts[3] = 0.5                                          # in place: same pointer, new version
    assert E.lt_key(a0, ts, 0.0, 1.0) != k0
    k1 = E.lt_key(a0, ts, 0.0, 1.0)
    a0.neg_()
    assert E.lt_key(a0, ts, 0.0, 1.0) != k1
    assert E.lt_key(a0, ts, 0.0, 2.0) != E.lt_key(a0, ts, 0.0, 1.0)
    # a view shares the counter: an edit through it counts
    k2 = E.lt_key(a0, ts, 0.0, 1.0)
    ts.view(2, 4)[1, 1] = 0.25
    assert E.lt_key(a0, ts, 0.0, 1.0) != k2
    # the moment cache: also the tensor scanned and the set of jets with bursts
    m = E.mom_cache_key(a0, ts, ts.data_ptr(), 0.0, 1.0, True, True)
    assert m == E.mom_cache_key(a0, ts, ts.data_ptr(), 0.0, 1.0, 1, 2)
    assert m != E.mom_cache_key(a0, ts, ts.data_ptr(), 0.0, 1.0, True, False)
    assert m != E.mom_cache_key(a0, ts, ts.data_ptr() + 8, 0.0, 1.0, True, True)
    ts[0] = 0.75
    assert m != E.mom_cache_key(a0, ts, ts.data_ptr(), 0.0, 1.0, True, True)
    # the unmasked copy: launch times AND the flag-carrying field
    u = E.unmasked_key(0, ts, a0, (0.0, 1.0))
    a0[2] = -a0[2]
    assert u != E.unmasked_key(0, ts, a0, (0.0, 1.0))
    assert E.unmasked_key(0, ts, a0, (0.0, 1.0)) != E.unmasked_key(1, ts, a0, (0.0, 1.0))


def test_struct_attaches_lt_only_for_what_it_was_built_from():
    f = _fields()
    lt = _attach_lt(f)
    fs = f.struct()
    assert fs.d_lt_cells == lt["cells"].data_ptr() and fs.lt_K == 8
    assert (fs.ts_lo, fs.ts_hi) == (1.0, 5.0)
    # an in-place, in-range edit of the launch times
    f.ts[5] = 2.0
    assert f.struct().d_lt_cells is None and f.struct().lt_K == 0
    _attach_lt(f)
    assert f.struct().d_lt_cells is not None
    # a jet flag flipped in place
    f.a0[7] = -f.a0[7]
    assert f.struct().d_lt_cells is None
    _attach_lt(f)
    # another declared range
    f.ts_range = (1.0, 6.0)
    assert f.struct().d_lt_cells is None
    f.ts_range = (1.0, 5.0)
    assert f.struct().d_lt_cells is not None
    # a new tensor of equal contents (its version counter starts again: the pointer differs)
    old = f.ts
    f.ts = old.clone()
    f._ts_range_of = f.ts.data_ptr()
    assert f.struct().d_lt_cells is None
    f.ts = old
    f._ts_range_of = old.data_ptr()
    assert f.struct().d_lt_cells is not None
    # the range belongs to the tensor it was measured on
    f._ts_range_of = 0
    fs = f.struct()
    assert (fs.ts_lo, fs.ts_hi) == (0.0, 0.0) and fs.d_lt_cells is None
    f.a0 = None
    assert f.struct().d_lt_cells is None


def test_the_declared_range_survives_an_in_place_edit():
    """The range is a declaration the kernels' guard watches, not a cache of the contents: an
    in-place edit leaves it attached (an edit that leaves it is the guard's to report)."""
    f = _fields()
    f.ts[0] = 99.0
    fs = f.struct()
    assert (fs.ts_lo, fs.ts_hi) == (1.0, 5.0)


# ---- the moment cache's bookkeeping ---------------------------------------------------------------
def test_cache_fills_serves_and_refills(stub):
    f = _fields()
    fs = stub.sweep(f, BOTH, "moments")
    assert fs.d_mom_cache == f.mom_cache["buf"].data_ptr()         # a dense model: at once
    assert (fs.mom_cache_K, fs.mom_cache_N) == (0, 0)
    assert (f.mom_cache["K"], f.mom_cache["N"]) == (53, 12) and "held" not in f.mom_cache
    fs = stub.sweep(f, BOTH, "moments")
    assert (fs.mom_cache_K, fs.mom_cache_N) == (53, 12) and stub.path == "cached"
    assert (f.mom_cache["K"], f.mom_cache["N"]) == (53, 12)
    # other burst parameters, same jets: the key does not hold them
    fs = stub.sweep(f, types.SimpleNamespace(n=[5, 3]), "moments")
    assert stub.path == "cached"
    # another SET of jets: offered empty, refilled
    fs = stub.sweep(f, RED, "moments")
    assert (fs.mom_cache_K, fs.mom_cache_N) == (0, 0) and stub.path == "moments"
    assert f.mom_cache["K"] == 53
    assert stub.sweep(f, RED, "moments").mom_cache_K == 53
    assert stub.sweep(f, BOTH, "moments").mom_cache_K == 0
    # what cannot use the cache leaves it alone: EM maps, short sweeps, the switch
    for kw in ({"want_em": True}, {"n_epochs": 11}):
        fs = stub.sweep(f, BOTH, "moments", **kw)
        assert fs.d_mom_cache is None and f.mom_cache["K"] == 53
    stub.cache_moments = False
    assert stub.sweep(f, BOTH, "moments").d_mom_cache is None
    stub.cache_moments = True


@pytest.mark.parametrize("edit", ["ts", "a0"])
def test_an_in_place_edit_empties_the_cache(stub, edit):
    f = _fields()
    stub.sweep(f, BOTH, "moments")
    assert stub.sweep(f, BOTH, "moments").mom_cache_K == 53
    if edit == "ts":
        f.ts[4] = 4.5
    else:
        f.a0[4] = -f.a0[4]
    fs = stub.sweep(f, BOTH, "moments")
    assert (fs.mom_cache_K, fs.mom_cache_N) == (0, 0) and stub.path == "moments"
    assert stub.sweep(f, BOTH, "moments").mom_cache_K == 53


def test_another_path_ran(stub):
    """tiles / lt: nothing was written -- a filled buffer holds what it held, one that never
    held moments is given back."""
    f = _fields()
    stub.sweep(f, BOTH, "tiles")
    assert f.mom_cache is None
    stub.sweep(f, BOTH, "moments")
    stub.sweep(f, BOTH, "lt")
    assert (f.mom_cache["K"], f.mom_cache["N"]) == (53, 12) and "held" not in f.mom_cache
    assert stub.sweep(f, BOTH, "moments").mom_cache_K == 53
    # ... but not across a key change: the buffer was offered EMPTY, so it holds nothing valid
    f.ts[1] = 1.5
    stub.sweep(f, BOTH, "tiles")
    assert f.mom_cache is None


def test_a_sparse_model_reserves_after_a_moment_sweep(stub):
    f = _fields()
    f.ylo = f.yhi = torch.zeros(8, dtype=torch.int32)
    f.occupied_cells = N // 4
    fs = stub.sweep(f, BOTH, "tiles")
    assert fs.d_mom_cache is None and f.mom_cache is None
    fs = stub.sweep(f, BOTH, "moments")
    assert fs.d_mom_cache is None and f.mom_cache["K"] == 0           # reserved
    stub.sweep(f, BOTH, "moments")
    assert f.mom_cache["K"] == 53


def test_a_failed_call_voids_the_recorded_shape(stub):
    f = _fields()
    stub.sweep(f, BOTH, "moments")
    stub.sweep(f, BOTH, "moments", fail="boom")        # may have started rewriting the buffer
    assert (f.mom_cache["K"], f.mom_cache["N"]) == (0, 0)
    fs = stub.sweep(f, BOTH, "moments")
    assert fs.mom_cache_K == 0 and stub.path == "moments" and f.mom_cache["K"] == 53


def test_a_guard_report_voids_what_was_filled_since_the_last_clean_one(stub):
    f, g, h = _fields(), _fields(), _fields()
    stub.sweep(f, BOTH, "moments")                     # filled, reported clean below
    stub.lib.rjp_range_guard = lambda ctx: 0
    stub.synchronize = lambda: None
    assert not stub.range_guard() and stub._unreported == {}
    stub.sweep(g, BOTH, "moments")                     # filled by the pass the guard flags
    stub.sweep(h, BOTH, "moments")
    stub.sweep(h, BOTH, "moments")                     # ("cached": served, nothing new)
    assert g.mom_cache["K"] == 53 and set(stub._unreported) == {id(g), id(h)}
    # any entry point raises the guard's message: here a sweep of ANOTHER model
    stub.msg["text"] = GUARD_TEXT
    stub.sweep(f, BOTH, "moments", fail="guard")
    assert (g.mom_cache["K"], g.mom_cache["N"]) == (0, 0)
    assert (h.mom_cache["K"], h.mom_cache["N"]) == (0, 0)
    assert f.mom_cache["K"] == 0                       # (its own call failed: void as well)
    assert stub._unreported == {}
    # an error that is not the guard's voids nothing else
    stub.sweep(g, BOTH, "moments")
    stub.msg["text"] = "bad gff_mode"
    stub.sweep(f, BOTH, "moments", fail="other")
    assert g.mom_cache["K"] == 53
    # the query reports it: the same
    stub.lib.rjp_range_guard = lambda ctx: 1
    assert stub.range_guard()
    assert g.mom_cache["K"] == 0 and stub._unreported == {}
    # fields that are gone by then are skipped
    stub.sweep(g, BOTH, "moments")
    del g
    assert stub.range_guard()


def test_rebuilding_a0_or_ts_drops_everything_built_from_them():
    f = _fields()
    _attach_lt(f)
    f.mom_cache, f.srt, f._ts_unmasked = {"K": 53}, {"K": 32}, ("key", None)
    E.RTEngine._drop_derived_state(f)
    assert f.lt is None and f.mom_cache is None and f.srt is None and f._ts_unmasked is None
