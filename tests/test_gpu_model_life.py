"""Derived state across a model's life, with the engine in its shipped configuration (cache_moments,
use_lt, use_sorted, use_srt_moments, use_chi_table all on, nothing forced): sequences of scans,
sweeps, burst changes, setter calls, in-place edits and layout builds, and after EVERY step the
question whether the maps belong to the current fields.

Truth lives on the host: every model is kept as float64 arrays (nd, xi, temp, ff, areas, ts, rr)
plus its burst lists, and every mutation is applied to them in lock-step with the device model.
Two references judge each result, neither of which reads engine state:
 (a) tests/gpu_util.ref_single_epoch per epoch on a host-formed a0 (U.golden_a0), plain NumPy for
     the emission measure and T_avg -- whole maps, identical zero / NaN / inf patterns; a sweep is
     judged at its first, its last and one seed-chosen epoch;
 (b) a stateless device run: a new DeviceFields uploaded from the host truth into a second engine
     with cache_moments, use_lt, use_sorted and use_moments off -- all [E, P] entries.
Tolerances (the project's own): single-epoch table / sorted / hybrid scans U.single_epoch_bound(n_y),
scans that keep the Gaussians U.GAUSS_RTOL; sweeps 1e-10 against (a) and 5e-11 against (b); EM and
T_avg 1e-11.  Against (b) a single-epoch map is held to the sum of the two runs' bounds against
the truth.

Shapes: MID (128 x 480 x 256) reaches the single-epoch paths (table on the grid order, the bucketed
layout with bins read and contracted) and keeps its sweeps on the epoch tiles; TALL (8 x 2048 x 256)
is where the library's cost model (ff_moments.hip) takes the launch-time moments for sweeps of 17
irregular or >= 32 uniform epochs (4.2e6 cells x 4.7 ps + 2048 sightlines x 4.7 ns = 29 us against
0.8 x 4.2e6 x 32 x 0.40 ps = 43 us by the tiles) and the tiles for 12 uniform ones; BOTH
(128 x 960 x 256) qualifies for the single-epoch layouts AND the moments (302 us against 322 us).

Measured on one MI355X: see DESIGN.md ("Derived state")."""
import copy
import time

import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
YEAR = orc.YEAR
T0 = time.time()
MID, TALL, BOTH = (128, 480, 256), (8, 2048, 256), (128, 960, 256)
SWEEP_VS_REF, SWEEP_VS_STATELESS, EM_RTOL = 1e-10, 5e-11, 1e-11
SEED = 20250915
JETS = ("RB", "R", "B", "", "RB")                        # the cycle of jets with bursts
SEEN = set()                                             # paths the random walks observed
WANTED = {"tiles", "moments", "cached", "lt", "table/grid", "table/sorted/read",
          "table/sorted/contracted"}
GUARD_TEXT = "earlier scan"


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    # the shipped configuration: nothing is switched
    assert (e.cache_moments and e.use_lt and e.use_sorted and e.use_srt_moments and
            e.use_chi_table and e.use_moments and not e.force_moments)
    yield e
    e.close()
    print("wall time of this module so far: %.0f s" % (time.time() - T0))


@pytest.fixture(scope="module")
def ref_eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    e.cache_moments = e.use_lt = e.use_sorted = e.use_moments = False
    yield e
    e.close()


_BASE = {}


def base_fields(shape, seed, temp_mode):
    """Host grids of a dense synthetic model (cached per module: the hash costs seconds); 2 % of
    the launch times are NaN, so that a jet WITHOUT bursts has cells only chi == 1 keeps."""
    key = (shape, seed, temp_mode)
    if key not in _BASE:
        g = U.synth_host(shape, seed, temp_mode)
        g.pop("vy")
        rng = np.random.default_rng(seed)
        g["ts"] = np.where(rng.random(shape) < 0.02, np.nan, g["ts"])
        _BASE[key] = g
    return {k: v.copy() for k, v in _BASE[key].items()}


def random_bursts(rng, jets):
    mk = lambda: [(rng.uniform(0.2, 2.2) * YEAR, 10.0 ** rng.uniform(-0.3, 1.0),
                   rng.uniform(0.15, 0.45) * YEAR) for _ in range(int(rng.integers(1, 4)))]
    return (mk() if "R" in jets else [], mk() if "B" in jets else [])


def sweep_epochs(rng, n):
    if n == 17:                                          # the irregular list
        return [float(t) for t in np.sort(rng.uniform(0.0, 5.0, 17)) * YEAR]
    return [float(t) for t in np.linspace(rng.uniform(0.0, 0.8), rng.uniform(3.0, 5.0), n) * YEAR]


class Life:
    """One model: the device fields of the engine under test, the host truth, the two judges."""

    def __init__(self, eng, ref_eng, shape, seed, temp_mode=0, name="model", prepare=None):
        from rajepy_amd import engine as E
        self.eng, self.ref_eng, self.shape, self.name = eng, ref_eng, shape, name
        self.mode = E.RJP_GFF_SCALAR if temp_mode == 0 else E.RJP_GFF_POWERLAW
        self.q_T = 0.0 if temp_mode == 0 else -0.5
        self.csize = 0.5
        self.g = base_fields(shape, seed, temp_mode)
        if prepare is not None:
            prepare(self.g)
        self.f = self._upload(eng)
        eng._attach_sorted(self.f)                       # (what the producers do after a0)
        self.bursts = U.example_burst_lists()
        self.jets = 0                                    # index into JETS
        self.state = 0                                   # bumped with every change of the truth
        self.log = []
        self._host = {}                                  # (state, what) -> derived host arrays
        self._refs = {}
        self._stateless = (None, None)
        self.paths, self.seen = [], set()

    def _upload(self, engine):
        g = self.g
        f = engine.upload_fields(g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"],
                                 g["rr"] < 0, csize_au=self.csize, dtype=8)
        return engine.tau_layout(f, self.mode)

    # ---- the host truth ------------------------------------------------------------------------
    def touched(self):
        self.state += 1
        self._host = {k: v for k, v in self._host.items() if k[0] == self.state}
        self._refs = {k: v for k, v in self._refs.items() if k[0] == self.state}

    def host(self, what):
        key = (self.state, what)
        if key not in self._host:
            g = self.g
            if what == "a0":
                v = U.golden_a0(g, self.q_T)
            elif what == "em0":                          # (n x)^2 ff / areas, jet in the sign
                v = (g["nd"] * g["xi"]) ** 2. * (g["ff"] / g["areas"])
                v = np.where(g["rr"] < 0, -v, v)
            else:
                with np.errstate(all="ignore"):
                    v = np.nanmean(np.where(g["temp"] > 0., g["temp"], np.nan), axis=1).ravel()
            self._host[key] = v
        return self._host[key]

    def ref(self, t, what="a0"):
        """(a): sum_y |w| chi^2 at epoch t, w = a0 (the tau sums) or em0 x path (the EM)."""
        key = (self.state, repr(self.bursts), float(t), what)
        if key not in self._refs:
            r = U.ref_single_epoch(self.host(what), self.g["ts"], self.bursts, t).ravel()
            if what == "em0":
                r = r * (self.csize * orc.AU / orc.PARSEC)
            self._refs[key] = r
        return self._refs[key]

    def stateless(self):
        """(b): fresh device fields from the host truth in the second engine."""
        if self._stateless[0] != self.state:
            self._stateless = (None, None)               # (free the old ones first)
            self._stateless = (self.state, self._upload(self.ref_eng))
        return self._stateless[1]

    # ---- scans -----------------------------------------------------------------------------------
    def _b(self):
        from rajepy_amd import engine as E
        return E.make_bursts(*self.bursts)

    def _note(self, what):
        eng = self.eng
        eng.synchronize()
        path, layout = eng.last_scan_path()[0], eng.last_scan_layout()
        bins = eng.last_srt_bins() if (path == "table" and layout == "sorted") else (0, 0)
        seen = {path} if path != "table" else set()
        if path == "table" and layout == "grid":
            seen.add("table/grid")
        if path == "table" and layout == "sorted":
            if bins[1] > 0 or bins == (0, 0):
                seen.add("table/sorted/read")
            if bins[0] > 0:
                seen.add("table/sorted/contracted")
        self.paths.append((what, path, layout, bins))
        self.seen |= seen
        self.log[-1] += " -> %s/%s%s" % (path, layout, bins if any(bins) else "")
        return path, layout, seen

    def _tol1(self, path):
        return U.single_epoch_bound(self.shape[1]) if path == "table" else U.GAUSS_RTOL

    def single(self, t, want_em=False):
        """A single-epoch scan judged by (a) and (b); -> (path, layout, seen)."""
        eng, ref_eng = self.eng, self.ref_eng
        self.log.append("%s: scan %.3f yr%s" % (self.name, t / YEAR, " +EM" if want_em else ""))
        sumA, em, _ = eng.ff_scan(self.f, self._b(), [t], self.mode, want_em=want_em,
                                  want_tavg=False)
        path, layout, seen = self._note("single")
        assert not eng.range_guard()
        got = sumA.cpu().numpy()[0]
        tag = (self.name, "scan", t / YEAR, path, layout)
        U.against(got, self.ref(t), self._tol1(path), tag + ("a",))
        if want_em:
            U.against(em.cpu().numpy()[0], self.ref(t, "em0"), EM_RTOL, tag + ("EM a",))
        r = ref_eng.ff_scan(self.stateless(), self._b(), [t], self.mode, want_em=want_em,
                            want_tavg=False)
        ref_eng.synchronize()
        tol_b = self._tol1(path) + self._tol1(ref_eng.last_scan_path()[0])
        U.against(got, r[0].cpu().numpy()[0], tol_b, tag + ("b",))
        if want_em:
            U.against(em.cpu().numpy()[0], r[1].cpu().numpy()[0], 2 * EM_RTOL, tag + ("EM b",))
        self.tavg()
        return path, layout, seen

    def tavg(self):
        got = self.eng.tavg(self.f).cpu().numpy()
        U.against(got, self.host("tavg"), EM_RTOL, (self.name, "T_avg"))

    def ff_step(self, t):
        """rjp_ff_step for three channels at one epoch: sums, tau and flux cubes against (a)."""
        from rajepy_amd import engine as E
        from rajepy_amd.maths import physics as ph
        eng = self.eng
        self.log.append("%s: ff_step %.3f yr" % (self.name, t / YEAR))
        nu = np.array([1e9, 5e9, 4.3e10])
        gv = [ph.gff(f, 1e4) for f in nu] if self.mode == E.RJP_GFF_SCALAR else None
        ctau, cflux = E.ff_channel_coeffs(nu, self.csize, 120., self.mode, gv)
        P, F, ny = self.f.npix, len(nu), self.shape[1]
        out = (eng._f64(1, P), None, eng._f64(1, F, P), eng._f64(1, F, P), eng._f64(1, F))
        eng.ff_step(self.f, self._b(), [t], self.mode, eng.tavg(self.f), ctau, cflux, out)
        path, layout, seen = self._note("ff_step")
        assert not eng.range_guard()
        tol, ref, tavg = self._tol1(path), self.ref(t), self.host("tavg")
        tag = (self.name, "ff_step", t / YEAR, path, layout)
        U.against(out[0].cpu().numpy()[0], ref, tol, tag + ("sumA",))
        tau, flux = out[2].cpu().numpy()[0], out[3].cpu().numpy()[0]
        for k in range(F):
            tau_ref = ctau[k] * ref
            U.against(tau[k], tau_ref, tol + 2.0 ** -52, tag + ("tau",))
            # (1 - e^-tau to 4e-15, rjp_device.h; T_avg a mean of n_y terms)
            U.against(flux[k], cflux[k] * tavg * (-np.expm1(-tau_ref)),
                      tol + EM_RTOL + 4e-15 + (ny + 4) * 2.0 ** -53, tag + ("flux",))
        return path, layout, seen

    def sweep(self, epochs, want_em=False, pick=None, skip=()):
        """An epoch sweep judged by (a) at its first, last and one chosen epoch and by (b)
        everywhere; `skip`: sightlines left out of the comparison (the guard scenarios judge
        them on their own).  -> (path, [E, P] sums, seen)."""
        eng, ref_eng = self.eng, self.ref_eng
        n = len(epochs)
        self.log.append("%s: sweep of %d%s" % (self.name, n, " +EM" if want_em else ""))
        sumA, em, _ = eng.ff_scan(self.f, self._b(), epochs, self.mode, want_em=want_em,
                                  want_tavg=False)
        path, layout, seen = self._note("sweep")
        got = sumA.cpu().numpy()
        got_em = em.cpu().numpy() if want_em else None
        keep = np.ones(self.f.npix, dtype=bool)
        keep[list(skip)] = False
        tag = (self.name, "sweep", n, path)
        for e in sorted({0, n - 1, (n // 2 if pick is None else int(pick)) % n}):
            U.against(got[e][keep], self.ref(epochs[e])[keep], SWEEP_VS_REF, tag + (e, "a"))
            if want_em:
                U.against(got_em[e][keep], self.ref(epochs[e], "em0")[keep], EM_RTOL,
                          tag + (e, "EM a"))
        r = ref_eng.ff_scan(self.stateless(), self._b(), epochs, self.mode, want_em=want_em,
                            want_tavg=False)
        ref_eng.synchronize()
        assert ref_eng.last_scan_path()[0] == "tiles"
        U.against(got[:, keep], r[0].cpu().numpy()[:, keep], SWEEP_VS_STATELESS, tag + ("b",))
        if want_em:
            U.against(got_em[:, keep], r[1].cpu().numpy()[:, keep], 2 * EM_RTOL, tag + ("EM b",))
        return path, got, seen

    # ---- mutations: the device model and the host truth in lock-step -----------------------------
    def set_bursts(self, bursts, jets=None):
        if jets is not None:
            self.jets = jets
        self.bursts = bursts
        self.log.append("%s: bursts %d + %d" % (self.name, len(bursts[0]), len(bursts[1])))

    def replace(self, name, new):
        self.log.append("%s: replace_field(%s)" % (self.name, name))
        self.g[name] = np.ascontiguousarray(new, dtype=np.float64)
        self.touched()
        self.eng.replace_field(self.f, name, self.g[name])

    def block(self, rng, frac=0.25):
        """A random box of up to `frac` of the cells."""
        out = []
        for n in self.shape:
            w = max(1, int(n * rng.uniform(0.3, 1.0) * frac ** (1. / 3.)))
            a = int(rng.integers(0, n - w + 1))
            out.append(slice(a, a + w))
        return tuple(out)

    def edit_ts(self, rng, block=None):
        """An in-place, in-range edit: a block of cells moved to other launch-time bins."""
        import torch
        block = block or self.block(rng)
        ts = self.g["ts"]
        lo, hi = np.nanmin(ts), np.nanmax(ts)
        new = rng.uniform(lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo), ts[block].shape)
        self.log.append("%s: in-place ts[%s]" % (self.name, _fmt(block)))
        ts[block] = new
        self.touched()
        self.f.ts.view(self.shape)[block] = torch.from_numpy(new).to(self.eng.device)
        return block

    def flip_a0(self, rng, block=None):
        """A jet-flag change in place: the sign bit of a0 (and of em0 / nd, which carry it on the
        other layouts)."""
        block = block or self.block(rng)
        self.log.append("%s: in-place flip a0[%s]" % (self.name, _fmt(block)))
        self.g["rr"][block] *= -1.0
        self.touched()
        for t in (self.f.a0, self.f.em0, self.f.nd):
            if t is not None:
                t.view(self.shape)[block].neg_()
        return block

    def build(self, what, K=None):
        eng = self.eng
        self.log.append("%s: %s" % (self.name, what))
        if what == "build_lt":
            eng.build_lt(self.f, K or 20)
        elif what == "build_sorted":
            eng.build_sorted(self.f)
        elif what == "compute_y_bounds":
            eng.compute_y_bounds(self.f)
        else:
            self.f.lt = None

    # ---- the range guard ---------------------------------------------------------------------------
    def guard_cycle(self, epochs, raiser="single", prime="sweep"):
        """Launch times edited IN PLACE to outside the declared range: a sweep that bins by launch
        time gives NaN on exactly those sightlines, the next call raises RJP_ERR_ARG once, and
        after the repair everything is finite and correct again, with nothing kept from the bad
        pass.  (NaN sums by design, not a fault: the kernels bounds-check and poison.)"""
        from rajepy_amd import _lib
        eng, f = self.eng, self.f
        nx, ny, nz = self.shape
        if prime == "sweep":
            self.sweep(epochs)                           # clean, and the range is declared by now
            assert not eng.range_guard()
        else:
            # a sweep on the launch-time-ordered layout, which is then dropped: the range is
            # declared and has been checked for these launch times, but nothing is cached -- the
            # flagged pass will be the FIRST to fill the cache
            self.build("build_lt", 20)
            assert self.sweep(epochs)[0] == "lt"
            self.build("drop_lt")
            assert f.mom_cache is None
        lo, hi = f.ts_range
        ts3 = f.ts.view(self.shape)
        hit = [(1, 5, 7), (nx - 1, ny - 1, nz - 1), (nx // 2, 0, nz // 2)]
        saved = [ts3[i].item() for i in hit]
        self.log.append("%s: in-place ts outside the range" % self.name)
        for i, v in zip(hit, (hi + 0.25 * (hi - lo), lo - 1.0, hi * 10.0)):
            ts3[i] = v
        pix = sorted({x * nz + z for (x, _, z) in hit})
        one_jet = (len(self.bursts[0]) == 0) != (len(self.bursts[1]) == 0)
        try:
            path, bad, _ = self.sweep(epochs, skip=pix)
        except _lib.RjprtError as e:
            # bursts in ONE jet: the scan reads the unmasked copy, which the edit made stale --
            # the rebuilt copy may be a tensor the context has not seen under this range, and
            # then the first-use check REFUSES the call outright instead of poisoning
            assert one_jet and e.status == _lib.RJP_ERR_ARG and "nothing was enqueued" in str(e)
            path = bad = None
            self.log[-1] += " -> refused"
        if bad is None:
            return self._after_the_guard(epochs, hit, saved)
        assert path == "moments", path                  # (a pass over the edited launch times)
        # (a hit cell of a jet WITHOUT bursts has chi == 1 whatever its launch time: its
        # sightline may be poisoned or right, and is not judged)
        must = sorted({x * nz + z for (x, y, z) in hit
                       if len(self.bursts[0 if self.g["rr"][x, y, z] < 0 else 1])})
        assert np.isnan(bad[:, must]).all(), "out-of-range launch times were clamped, not poisoned"
        self.log.append("%s: the next call" % self.name)
        with pytest.raises(_lib.RjprtError) as ei:
            if raiser == "single":
                eng.ff_scan(f, self._b(), [epochs[0]], self.mode, want_em=False, want_tavg=False)
            else:
                eng.tavg(f)
        assert ei.value.status == _lib.RJP_ERR_ARG and GUARD_TEXT in str(ei.value)
        # nothing filled by the flagged pass is still recorded as valid
        mc = f.mom_cache
        assert mc is None or (mc["K"], mc["N"]) == (0, 0), "moment maps of the flagged pass kept"
        self._after_the_guard(epochs, hit, saved)

    def _after_the_guard(self, epochs, hit, saved):
        eng, f = self.eng, self.f
        ts3 = f.ts.view(self.shape)
        mc = f.mom_cache
        assert mc is None or (mc["K"], mc["N"]) == (0, 0)
        assert f.struct().d_lt_cells is None
        self.log.append("%s: repair" % self.name)
        for i, v in zip(hit, saved):
            ts3[i] = v
        for k in range(3):                               # every later sweep: finite and correct
            path, got, _ = self.sweep(epochs)
            assert np.isfinite(got).all()
            assert not eng.range_guard()
            assert path == ("moments" if k == 0 else "cached"), (k, path)
        mc = f.mom_cache
        assert mc is not None and mc["K"] > 0


def _fmt(block):
    return ",".join("%d:%d" % (s.start, s.stop) for s in block)


def uniform32(a=0.0, b=5.0, n=32):
    return [float(t) for t in np.linspace(a, b, n) * YEAR]


# ---- deterministic scenarios -----------------------------------------------------------------------
def test_scenario_1_the_cache_serves_other_epochs_and_bursts_and_refills_for_other_jets(eng, ref_eng):
    m = Life(eng, ref_eng, TALL, SEED, name="tall")
    rng = np.random.default_rng(1)
    assert m.sweep(uniform32())[0] == "moments"
    assert (m.f.mom_cache["K"], m.f.mom_cache["N"]) != (0, 0)
    assert m.sweep(sweep_epochs(rng, 17))[0] == "cached"         # other epochs
    m.set_bursts(random_bursts(rng, "RB"))
    assert m.sweep(uniform32(0.1, 4.0))[0] == "cached"           # other burst parameters
    m.set_bursts(U.example_burst_lists("R"), jets=1)
    assert m.sweep(uniform32())[0] == "moments"                  # one jet: refilled
    assert m.sweep(sweep_epochs(rng, 17))[0] == "cached"
    m.set_bursts(U.example_burst_lists(), jets=0)
    assert m.sweep(uniform32())[0] == "moments"                  # both again: refilled
    assert m.sweep(uniform32(0.2, 4.5, 40))[0] == "cached"


def _differs(m, before, after, block):
    """The edit matters: the sightlines under `block` moved by far more than any tolerance."""
    nz = m.shape[2]
    pix = [x * nz + z for x in range(block[0].start, block[0].stop)
           for z in range(block[2].start, block[2].stop)]
    rel = np.abs(after[:, pix] - before[:, pix]) / before[:, pix]
    assert np.nanmax(rel) > 1e-6, "the edit did not change the maps: the scenario tests nothing"


BLOCK = (slice(2, 6), slice(100, 1500), slice(40, 200))


@pytest.mark.parametrize("edit", ["ts", "a0"])
def test_scenario_2_the_lt_layout_follows_an_in_place_edit(eng, ref_eng, edit):
    """Sweeps on the launch-time-ordered layout never read d_ts or d_a0: after an in-place edit of
    the launch times (or of the jet flag, with bursts in one jet only so that the flag changes
    chi) the result must follow the edit.  Whether the layout is rebuilt, dropped or the sweep
    falls back is the engine's choice; returning the old maps is the failure."""
    m = Life(eng, ref_eng, TALL, SEED + 1, name="tall")
    if edit == "a0":
        m.set_bursts(U.example_burst_lists("R"), jets=1)
    m.build("build_lt", 20)
    path, before, _ = m.sweep(uniform32())
    assert path == "lt"
    if edit == "ts":
        m.edit_ts(np.random.default_rng(2), BLOCK)
    else:
        m.flip_a0(np.random.default_rng(3), BLOCK)
    path, after, _ = m.sweep(uniform32())                # judged against the EDITED fields
    _differs(m, before, after, BLOCK)
    print("scenario 2 (%s): the sweep after the edit took %s" % (edit, path))
    m.build("build_lt", 20)                              # rebuilt: attached again, and right
    assert m.f.struct().d_lt_cells is not None
    assert m.sweep(uniform32(0.1, 4.8))[0] in ("lt", "cached")   # (a filled cache comes first)


@pytest.mark.parametrize("jets", ["RB", "R"])
def test_scenario_3_the_moment_cache_follows_an_in_place_edit_of_the_launch_times(eng, ref_eng, jets):
    """With bursts in one jet only the scan reads the unmasked launch-time copy: it follows too."""
    m = Life(eng, ref_eng, TALL, SEED + 2, name="tall")
    m.set_bursts(U.example_burst_lists(None if jets == "RB" else jets), jets=JETS.index(jets))
    assert m.sweep(uniform32())[0] == "moments"
    path, before, _ = m.sweep(uniform32())
    assert path == "cached"
    if jets == "R":
        assert m.f._ts_unmasked is not None
    m.edit_ts(np.random.default_rng(4), BLOCK)
    path, after, _ = m.sweep(uniform32())
    _differs(m, before, after, BLOCK)
    assert path == "moments"                             # refilled from the edited launch times
    assert m.sweep(uniform32())[0] == "cached"
    m.flip_a0(np.random.default_rng(5), BLOCK)
    path, flipped, _ = m.sweep(uniform32())
    assert path == "moments"
    if jets == "R":
        _differs(m, after, flipped, BLOCK)


@pytest.mark.parametrize("attached,raiser", [("cache", "single"), ("cache", "tavg"), ("lt", "single"),
                                             ("nothing", "tavg")])
def test_scenario_4_a_guard_report_voids_what_the_flagged_pass_filled(eng, ref_eng, attached, raiser):
    """With the filled cache or the layout attached the edited launch times must be READ (a pass,
    NaN on their sightlines, the report); with nothing attached the flagged pass is the one that
    fills the cache, and the report -- raised here by a call that is no sweep -- must void it."""
    m = Life(eng, ref_eng, TALL, SEED + 3, name="tall")
    if attached == "lt":
        m.build("build_lt", 20)
        assert m.sweep(uniform32())[0] == "lt"
    elif attached == "cache":
        assert m.sweep(uniform32())[0] == "moments"
        assert m.sweep(uniform32())[0] == "cached"
    try:
        m.guard_cycle(uniform32(), raiser, prime="range" if attached == "nothing" else "sweep")
    finally:
        eng.range_guard()


def _pin_free_blocks():
    """Allocate every free block of 1 MiB or more that the caching allocator still holds after
    `empty_cache()`, each at its exact size, smallest first (a request is served by the smallest
    block that fits) -> the tensors, to be kept alive by the caller."""
    import torch
    held = []
    for _ in range(4):
        free = sorted(b["size"] for seg in torch.cuda.memory_snapshot()
                      if seg["segment_type"] == "large"
                      for b in seg["blocks"] if b["state"] == "inactive" and b["size"] >= 1 << 20)
        if not free:
            break
        held += [torch.empty(n, dtype=torch.uint8, device="cuda") for n in free]
    return held


@pytest.mark.parametrize("name", ["temp", "xi"])
def test_scenario_5_replace_field_with_everything_attached(eng, ref_eng, name):
    """lt, srt + moments, the filled moment cache and the y-ranges attached, then the setter: a0,
    em0, T_avg, the y-ranges and every layout follow, on the FIRST call after the replacement --
    with the rebuilt a0 (and em0) at the OLD one's address, which the test forces (the replaced
    field's old tensor is kept alive and the allocator's cache emptied, so the block the engine
    frees is the only one of its size) and asserts.  The allocator's cache is emptied BEFORE the
    model is built as well, and what it cannot give back (the free parts of segments that
    something earlier in the process still holds a tensor in) is taken out of play: every
    grid-sized tensor of the model then sits in a segment of its own, so that a freed a0 cannot
    merge with a free neighbour (the block handed out would then start at the neighbour's
    address)."""
    import gc
    import torch
    def hole(g):                                         # cells that count for T_avg only
        g["nd"][:, 700:, :40] = np.nan
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    pinned = _pin_free_blocks()                          # (held to the end of the scenario)
    m = Life(eng, ref_eng, BOTH, SEED + 4, temp_mode=1, name="both", prepare=hole)
    f = m.f
    m.build("compute_y_bounds")
    assert f.srt is not None and f.srt["mom"] is not None
    assert m.sweep(uniform32())[0] == "moments"          # fills the cache ...
    m.build("build_lt", 20)                              # ... before the layout takes the sweeps
    assert m.sweep(uniform32())[0] == "cached"
    path, layout, _ = m.single(1.0 * YEAR)
    assert (path, layout) == ("table", "sorted")
    rng = np.random.default_rng(6)
    fac = rng.uniform(0.6, 1.5, (m.shape[0], 1, m.shape[2]))
    new = m.g[name] * fac
    if name == "temp":
        new[:, 700:, :40] = np.nan                       # (the occupied y-ranges shrink)
    keep_old = getattr(f, name)                          # its block must not be up for reuse
    old = {k: getattr(f, k).data_ptr() for k in ("a0", "em0")}
    vers = f.a0._version
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    m.replace(name, new)
    assert f.a0.data_ptr() == old["a0"] and f.a0._version == vers, "a0 not at its old address"
    if name == "xi":
        assert f.em0.data_ptr() == old["em0"], "em0 not at its old address"
    del keep_old, pinned
    assert f.lt is None and f.srt is None and f.mom_cache is None
    assert f.struct().d_lt_cells is None
    path, layout, _ = m.single(1.0 * YEAR, want_em=True)         # first call: a0, em0, T_avg
    assert (path, layout) == ("table", "grid")
    assert m.sweep(uniform32())[0] == "moments"          # the FIRST sweep: its own pass
    # the y-ranges follow the new field: rows with T > 0 or n, x, ff / areas all non-NaN
    # (include/rjprt.h `rjp_y_bounds`), restated on the host
    g = m.g
    with np.errstate(all="ignore"):
        occ = (g["temp"] > 0) | ~np.isnan(g["nd"] * g["xi"] * (g["ff"] / g["areas"]))
    ny = m.shape[1]
    assert occ.any(axis=1).all()
    ylo = np.argmax(occ, axis=1).ravel()
    yhi = (ny - np.argmax(occ[:, ::-1, :], axis=1)).ravel()
    assert np.array_equal(f.ylo.cpu().numpy(), ylo) and np.array_equal(f.yhi.cpu().numpy(), yhi)
    assert f.occupied_cells == int((yhi - ylo).sum())
    assert (f.occupied_cells < f.ncells) == (name == "temp")
    m.build("build_sorted")
    m.build("build_lt", 20)
    path, layout, _ = m.single(1.0 * YEAR)
    assert (path, layout) == ("table", "sorted")
    assert m.sweep(uniform32())[0] == "cached"


def test_scenario_6_only_a_layout_of_the_new_launch_times_is_read(eng, ref_eng):
    m = Life(eng, ref_eng, MID, SEED + 5, name="mid")
    f = m.f
    assert f.srt is not None
    for years in (1.0, 0.3):
        assert m.single(years * YEAR)[:2] == ("table", "sorted")
    old = f.ts.data_ptr()
    m.replace("ts", np.where(np.isnan(m.g["ts"]), np.nan, 0.8 * m.g["ts"][::-1] + 0.1 * YEAR))
    assert f.srt is None
    for years in (1.0, 0.3):
        assert m.single(years * YEAR)[:2] == ("table", "grid")
    m.build("build_sorted")
    for years in (1.0, 0.3):
        assert m.single(years * YEAR)[:2] == ("table", "sorted")
    # an in-place edit: the layout is stale, never read
    m.edit_ts(np.random.default_rng(7), (slice(10, 90), slice(50, 400), slice(20, 200)))
    assert m.single(1.0 * YEAR)[:2] == ("table", "grid")
    m.build("build_sorted")
    assert m.single(1.0 * YEAR)[:2] == ("table", "sorted")
    print("scenario 6: the new launch times %s the old tensor's address" % (
        "sit at" if f.ts.data_ptr() == old else "do not sit at"))


# ---- random walks ------------------------------------------------------------------------------------
OPS = [("single", 4.0), ("single_em", 1.5), ("ff_step", 1.0), ("sweep", 6.0), ("sweep_em", 1.5),
       ("bursts", 1.5), ("jets", 1.0), ("replace_ts", 0.7), ("replace_temp", 0.7),
       ("replace_xi", 0.7), ("edit_ts", 1.5), ("flip_a0", 1.0), ("build_lt", 2.0),
       ("build_sorted", 1.5), ("compute_y_bounds", 0.7), ("drop_lt", 0.5), ("guard", 0.7)]
N_OPS = 14
ON_MID = {"single": 0.8, "single_em": 0.8, "ff_step": 0.8, "build_sorted": 0.9, "sweep": 0.25,
          "sweep_em": 0.25, "build_lt": 0.3, "drop_lt": 0.3, "guard": 0.0}


SWEEP_LENGTHS = (12, 17, 32, 33, 40)
# seeds picked with `predict_paths` out of 0..59: six whose TALL model should sweep on the
# launch-time-ordered layout before anything fills the cache (11 such sweeps), six with guard
# cycles, cached sweeps and many single-epoch scans of a MID model whose bucketed layout is valid
WALK_SEEDS = (0, 10, 19, 24, 31, 59, 1, 11, 27, 36, 39, 46)


def plan_walk(seed):
    """The walk of `seed`: N_OPS x (operation, model index, sweep length) -- everything that
    decides which PATH a step can take is drawn here, from the seed alone, so that the seeds can
    be chosen on the host (see `predict_paths`); epochs, burst parameters and edited blocks are
    drawn while the walk runs."""
    rng = np.random.default_rng(40000 + seed)
    names, w = [o for o, _ in OPS], np.array([x for _, x in OPS])
    ops = [str(o) for o in rng.choice(names, size=N_OPS, p=w / w.sum())]
    return [(op, 0 if rng.random() < ON_MID.get(op, 0.5) else 1, int(rng.choice(SWEEP_LENGTHS)))
            for op in ops]


def predict_paths(plan):
    """Which sweep paths the TALL model of a walk should take, by the rules of DESIGN.md's table
    and the library's cost model (host arithmetic only; used to pick WALK_SEEDS and printed
    beside what the device did -- a forecast, not a check: new burst parameters may need another
    moment shape, which refills the cache where this says "cached")."""
    jets, cache, lt, out = 0, False, False, []
    for op, model, n in plan:
        if model != 1:
            continue
        if op in ("sweep", "sweep_em"):
            em = op == "sweep_em"
            moments = (n >= 17 and not em) or (n == 40 and em)       # (the cost model on TALL)
            if JETS[jets] == "":
                path = "tiles"
            elif cache and not em:
                path = "cached"
            elif lt and not em and n <= 32:
                path = "lt"
            else:
                path = "moments" if moments else "tiles"
                cache = cache or (path == "moments" and not em)
            out.append(path)
        elif op == "jets":
            jets, cache = (jets + 1) % 4, False
        elif op in ("edit_ts", "flip_a0", "replace_ts", "replace_temp", "replace_xi"):
            cache = lt = False
        elif op == "build_lt":
            lt = True
        elif op == "drop_lt":
            lt = False
        elif op == "guard":
            if JETS[jets] == "":
                jets = 0
            out += [None, "moments", "moments", "cached", "cached"]  # (the first: whatever held)
            cache, lt = True, False
    return out


def _step(rng, op, m, n):
    """One operation of the alphabet on model `m`."""
    if op in ("single", "single_em"):
        m.single(rng.uniform(0.2, 2.5) * YEAR, want_em=op == "single_em")
    elif op == "ff_step":
        m.ff_step(rng.uniform(0.2, 2.5) * YEAR)
    elif op in ("sweep", "sweep_em"):
        m.sweep(sweep_epochs(rng, n), want_em=op == "sweep_em", pick=rng.integers(0, n))
    elif op == "bursts":
        m.set_bursts(random_bursts(rng, JETS[m.jets]))
    elif op == "jets":
        j = (m.jets + 1) % 4
        m.set_bursts(random_bursts(rng, JETS[j]), jets=j)
    elif op == "replace_ts":
        ts = m.g["ts"]
        m.replace("ts", rng.uniform(0.7, 1.0) * ts + rng.uniform(0.0, 0.3) * YEAR)
    elif op in ("replace_temp", "replace_xi"):
        k = op[8:]
        m.replace(k, m.g[k] * rng.uniform(0.7, 1.3, (m.shape[0], 1, m.shape[2])))
    elif op == "edit_ts":
        m.edit_ts(rng)
    elif op == "flip_a0":
        m.flip_a0(rng)
    elif op == "build_lt":
        m.build("build_lt", int(rng.choice([16, 20, 24])))
    elif op == "guard":
        if JETS[m.jets] == "":                           # (no bursts, no launch-time bins: the
            m.set_bursts(random_bursts(rng, "RB"), jets=0)   # walk moves on to both jets first)
        m.guard_cycle(uniform32())
    else:
        m.build(op)


@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_random_walk(eng, ref_eng, seed):
    """N_OPS operations drawn from the alphabet, on two models (MID for the single-epoch paths,
    TALL for the sweeps' moment paths), every scan judged by both references."""
    rng = np.random.default_rng(50000 + seed)
    models = [Life(eng, ref_eng, MID, SEED + 10 + seed, temp_mode=seed % 2, name="mid"),
              Life(eng, ref_eng, TALL, SEED + 30 + seed, temp_mode=(seed + 1) % 2, name="tall")]
    plan = plan_walk(seed)
    done = []
    try:
        for op, k, n in plan:
            m = models[k]
            done.append("%s@%s" % (op, m.name))
            _step(rng, op, m, n)
            assert not eng.range_guard()
    except Exception as e:
        log = [line for m in models for line in m.log[-6:]]
        raise AssertionError("walk seed %d failed at step %d of %s\nlast scans: %s\n%s: %s" % (
            seed, len(done), done, log, type(e).__name__, e)) from e
    finally:
        eng.range_guard()
        for m in models:
            SEEN.update(m.seen)
    assert len(done) == N_OPS
    print("walk %d: %s" % (seed, " ".join(done)))
    print("   paths: %s" % sorted({p[1] + "/" + p[2] for m in models for p in m.paths}))
    print("   sweeps of tall: forecast %s, took %s" % (
        predict_paths(plan), [p[1] for p in models[1].paths if p[0] == "sweep"]))


def test_the_walks_saw_every_path():
    """Conditions, not measurements: every path the engine can take was judged in some walk."""
    assert WANTED <= SEEN, "never observed by a walk: %s" % sorted(WANTED - SEEN)


# ---- JetModel level ----------------------------------------------------------------------------------
FREQS = np.array([1e9, 5e9, 4.3e10])


class JetLife:
    """A JetModel, the host truth of its fields and an OracleJet on them."""

    def __init__(self, jm, params, g):
        self.jm, self.params, self.g = jm, params, g
        self.extra = []                                  # bursts added after construction
        self.set = {}                                    # fields replaced through the setters
        self._remake()

    def _remake(self):
        g = self.g
        t = getattr(getattr(self, "jet", None), "time", 0.0)
        self.jet = orc.OracleJet.from_fields(copy.deepcopy(self.params), g["nd"], g["xi"],
                                             g["temp"], g["ff"], g["areas"], g["ts"], g["rr"],
                                             g["vy"])
        self.jet.time = t
        for t0, chi, hl, which in self.extra:
            ss = self.jet._ss_jml_rj if which == "R" else self.jet._ss_jml_bj
            self.jet.bursts[which].append((t0, chi * ss, hl))

    def at(self, t):
        self.jm.time = self.jet.time = t

    def add_burst(self, t0, chi, hl, which):
        self.jm.add_ejection_event(t0, chi * self.jm.ss_jml(which), hl, which)
        self.extra.append((t0, chi, hl, which))
        self._remake()

    def setter(self, name, new):
        key = {"ts": "ts", "temperature": "temp", "ion_fraction": "xi", "vel": "vy"}[name]
        self.g[key] = new[1] if name == "vel" else new
        self.set[name] = new
        setattr(self.jm, name, new)
        self._remake()

    def check(self, what=("tau", "flux"), rtol_tau=1e-10, rtol_flux=1e-9):
        jm, jet = self.jm, self.jet
        with np.errstate(all="ignore"):
            if "tau" in what:
                got, ref = jm.optical_depth_ff(FREQS), jet.optical_depth_ff(FREQS)
                assert np.array_equal(got == 0, ref == 0)
                np.testing.assert_allclose(got, ref, rtol=rtol_tau, atol=0)
            if "flux" in what:
                got, ref = jm.flux_ff(FREQS), jet.flux_ff(FREQS)
                assert np.array_equal(np.isnan(got), np.isnan(ref))
                np.testing.assert_allclose(got, ref, rtol=rtol_flux, atol=0)
            if "em" in what:
                np.testing.assert_allclose(jm.emission_measure(), jet.emission_measure(),
                                           rtol=rtol_flux, atol=0)
            if "formal" in what:
                from rajepy_amd import engine as E
                from rajepy_amd.maths import physics as ph
                from tests.test_gpu_formal_rt import np_formal
                gv = [ph.gff(nu, self.params["properties"]["T_0"]) for nu in FREQS] \
                    if jm.gff_mode == E.RJP_GFF_SCALAR else None
                _, cflux = E.ff_channel_coeffs(FREQS, jm.csize, self.params["target"]["dist"],
                                               jm.gff_mode, gv)
                ref = np_formal(jet.optical_depth_ff(FREQS, collapse=False), self.g["temp"], cflux)
                got = jm.flux_ff(FREQS, formal=True)
                assert np.array_equal(np.isnan(got), np.isnan(ref))
                np.testing.assert_allclose(got, ref, rtol=1e-10, atol=0)
            if "rrl" in what:
                rf = orc.chan_freqs(22364174326.22781, 8e5, 1e5)
                np.testing.assert_allclose(jm.optical_depth_rrl("H66a", rf),
                                           jet.optical_depth_rrl("H66a", rf), rtol=1e-8, atol=1e-300)

    def light_curve(self, times, fresh=None):
        """flux_vs_time against the oracle's summed flux maps at the first, last and middle epoch
        (1e-9, as tests/test_gpu_model.py) and, everywhere, against a fresh model's (1e-10)."""
        jm, jet = self.jm, self.jet
        lc = jm.flux_vs_time(times, FREQS)
        path = jm.engine.last_scan_path()[0]
        keep = jet.time
        for e in sorted({0, len(times) // 2, len(times) - 1}):
            jet.time = times[e]
            with np.errstate(all="ignore"):
                np.testing.assert_allclose(lc[e], np.nansum(jet.flux_ff(FREQS), axis=(1, 2)),
                                           rtol=1e-9)
        jet.time = keep
        if fresh is not None:
            np.testing.assert_allclose(lc, fresh.flux_vs_time(times, FREQS), rtol=1e-10)
        return path


def _fresh_like(life, make):
    """A new JetModel given the same fields: built the same way, the same bursts added, the
    replaced fields installed through the setters."""
    jm = make()
    for t0, chi, hl, which in life.extra:
        jm.add_ejection_event(t0, chi * jm.ss_jml(which), hl, which)
    for name, new in life.set.items():
        setattr(jm, name, new)
    return jm


def _against_fresh(life, make, times):
    fresh = _fresh_like(life, make)
    fresh.time = life.jm.time
    for fn in ("optical_depth_ff", "flux_ff"):
        np.testing.assert_allclose(getattr(life.jm, fn)(FREQS), getattr(fresh, fn)(FREQS),
                                   rtol=1e-11, atol=0)
    np.testing.assert_allclose(life.jm.emission_measure(), fresh.emission_measure(), rtol=1e-11)
    life.light_curve(times, fresh)
    return fresh


def _jet_life(life, make, dense):
    """The interleaved life of a JetModel; `dense`: the cost model gives its sweeps the moments."""
    jm = life.jm
    eng = jm.engine
    t24 = np.linspace(0.0, 4.0, 24) * YEAR
    t32 = np.linspace(0.2, 4.6, 32) * YEAR
    life.at(1.0 * YEAR)
    life.check(("tau", "flux", "em"))
    jm.prefetch_epochs([0.5 * YEAR, 1.0 * YEAR, 2.0 * YEAR], want_em=False)
    life.at(2.0 * YEAR)
    life.check(("tau", "em"))
    p1 = life.light_curve(t32)
    p2 = life.light_curve(t24)
    if dense:
        assert (p1, p2) == ("moments", "cached")
    life.add_burst(1.6 * YEAR, 7.0, 0.3 * YEAR, "B")
    life.check(("tau", "flux"))                          # (the scan cache went with the bursts)
    life.light_curve(t24)
    info = jm.prepare_epoch_sweeps(20)
    assert info["K"] == 20
    path = life.light_curve(t32)
    assert path == "cached" if dense else path in ("lt", "cached"), path
    _against_fresh(life, make, t24)
    # the setters, each followed by the products that read what it changed
    g = life.g
    rng = np.random.default_rng(11)
    life.setter("ts", np.where(np.isnan(g["ts"]), np.nan, 0.85 * g["ts"] + 0.05 * YEAR))
    assert jm.device_fields.struct().d_lt_cells is None
    life.at(1.3 * YEAR)
    life.check(("tau", "flux"))
    life.light_curve(t32)
    jm.prepare_epoch_sweeps(16)
    life.light_curve(t24)
    life.setter("temperature", g["temp"] * rng.uniform(0.7, 1.4, g["temp"].shape))
    life.check(("tau", "flux", "formal"))
    life.light_curve(t32)
    life.at(0.6 * YEAR)
    life.check(("tau", "rrl"))
    life.setter("ion_fraction", g["xi"] * rng.uniform(0.5, 1.0, g["xi"].shape))
    life.check(("tau", "em", "formal"))
    life.light_curve(t24)
    still = np.zeros_like(g["vy"])
    life.setter("vel", (still, g["vy"] + rng.normal(0.0, 3.0, g["vy"].shape), still))
    life.check(("rrl", "tau"))
    life.at(2.4 * YEAR)
    life.check(("rrl", "flux", "em"))
    life.add_burst(0.9 * YEAR, 3.0, 0.25 * YEAR, "R")
    life.check(("tau", "flux"))
    jm.prepare_epoch_sweeps(24)
    life.light_curve(t32)
    _against_fresh(life, make, t32)
    assert not eng.range_guard()


def test_jetmodel_life_of_the_example_jet(eng, tmp_path):
    from rajepy_amd import classes, logger
    from tests.test_host_logic import example_params
    log = logger.Log(str(tmp_path / "a.log"), verbose=False)
    make = lambda: classes.JetModel(example_params(), log=log, engine=eng)
    z, meta, p, g, jet = U.golden_dense("cfg1_example")
    _jet_life(JetLife(make(), p, g), make, dense=False)


def test_jetmodel_life_of_a_dense_synthetic_model(eng, tmp_path):
    """Dense fields uploaded into a JetModel: its sweeps of 32 epochs take the moments by the cost
    model (5.2e5 cells x 4.7 ps + 256 sightlines x 4.7 ns = 3.7 us against 0.8 x 6.7 us) and keep
    the cache."""
    from rajepy_amd import classes, logger
    shape = (4, 2048, 64)
    g = U.synth_host(shape, SEED + 50, 0)
    p = copy.deepcopy(U.load_golden("cfg1_example")[2])
    p["ejection"] = U.example_bursts_params()
    p["grid"].update(n_x=shape[0], n_y=shape[1], n_z=shape[2])
    log = logger.Log(str(tmp_path / "a.log"), verbose=False)

    def make():
        q = copy.deepcopy(p)
        q["geometry"].pop("mod_r_0", None)
        for k in ("q_n", "q_tau"):
            q["power_laws"].pop(k, None)
        q["properties"].pop("n_0", None)
        jm = classes.JetModel(q, log=log, engine=eng)
        dev = eng.upload_fields(g["nd"], g["xi"], g["temp"], g["ff"], g["areas"], g["ts"],
                                g["rr"] < 0, vy=g["vy"], csize_au=jm.csize, dtype=8)
        eng.tau_layout(dev, jm.gff_mode)
        eng.compute_y_bounds(dev)
        jm._dev = dev
        return jm

    life = JetLife(make(), p, {k: v.copy() for k, v in g.items()})
    _jet_life(life, make, dense=True)
