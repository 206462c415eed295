"""The free-free map stage (K2: rjp_ff_maps, and the second half of rjp_ff_step) against the
long-double reference and the term-by-term bounds of tests/ff_maps_ref.py, which
tests/test_ff_maps_reference_cpu.py pins on the CPU.  Every case says which of the four launch
shapes it ran (rjp_last_maps_launch against the restated rule): the small-map kernel, the cube
kernel with per-lane accumulators at one and at four pixel groups per lane, the totals-only
kernel -- each at both lane widths, at its tails, with every edge value planted.  Then rjp_ff_step
on a sightline the launch-time range guard has poisoned."""
import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import ff_maps_ref as M
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
BAND = 512                     # doubles of guard band on either side of every output
SENT = -7.25                   # what the bands hold
WORST = {}                     # kernel name -> worst error / bound seen, printed as it grows


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    e.cache_moments = False
    yield e
    e.close()


class _Banded:
    """n doubles between two guard bands; `shift`: the payload starts 8 bytes off a 16-byte
    boundary."""

    def __init__(self, eng, n, shift=False):
        import torch
        self.n, self.o = n, BAND + (1 if shift else 0)
        self.buf = torch.full((n + 2 * BAND + 2,), SENT, dtype=torch.float64, device=eng.device)
        self.t = self.buf[self.o:self.o + n]
        assert self.t.data_ptr() % 16 == (8 if shift else 0)

    def intact(self):
        return bool((self.buf[:self.o] == SENT).all()) and bool((self.buf[self.o + self.n:] == SENT).all())


def _note(kernel, r):
    for what, v in r.items():
        key = "%s %s" % (kernel, what)
        if v > WORST.get(key, -1.0):
            WORST[key] = v
    print("worst error / bound of %s so far: " % kernel +
          ", ".join("%s %.3f" % (k[len(kernel) + 1:], v) for k, v in sorted(WORST.items())
                    if k.startswith(kernel + " ")))


def _kernel_name(L):
    return {"small": "ff_maps_kernel", "ftot": "ff_ftot_kernel",
            "acc": "ff_maps_acc_kernel<KP=%d>" % L.kp}[L.kernel] + "<VEC=%d>" % L.vec


def _call(eng, k, dA, dT, c, want, shifted):
    """One rjp_ff_maps with the outputs of `want` (subset of 'tau', 'flux', 'ftot'), banded
    outputs and a banded workspace of exactly rjp_ff_maps_workspace() bytes -> (outputs by name,
    the launch reported).  Asserts the bands and the launch rule."""
    from rajepy_amd import _lib
    E, F, P = k.E, k.F, k.npix
    out = {n: _Banded(eng, E * F * P if n != "ftot" else E * F, shift=(shifted == n))
           for n in want}
    wb = int(eng.lib.rjp_ff_maps_workspace(P, E, F))
    assert wb % 8 == 0
    work = _Banded(eng, wb // 8)
    ptr = lambda n: out[n].t.data_ptr() if n in out else None
    eng._call("rjp_ff_maps", dA.data_ptr(), dT.data_ptr(), P, E, _lib.dbl_array(c["ctau"]),
              _lib.dbl_array(c["cflux"]), F, ptr("tau"), ptr("flux"), ptr("ftot"),
              work.t.data_ptr() if "ftot" in want else None, wb if "ftot" in want else 0)
    got = eng.last_maps_launch()
    eng.synchronize()
    aligned = shifted is None or (shifted != "tavg" and shifted not in want)
    rule = M.launch_rule(P, E, F, "tau" in want, "flux" in want, "ftot" in want, aligned=aligned)
    assert got == tuple(rule), (want, got, rule)
    for n, b in list(out.items()) + [("workspace", work)]:
        assert b.intact(), "%s: written outside its buffer" % n
    if "ftot" not in want:
        assert bool((work.t == SENT).all()), "the workspace was touched without totals"
    shape = {"tau": (E, F, P), "flux": (E, F, P), "ftot": (E, F)}
    return {n: out[n].t.view(shape[n]) for n in want}, rule


def _bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


@pytest.mark.parametrize("k", M.GPU_CASES, ids=M.case_id)
def test_every_launch_shape_against_the_reference(eng, k):
    """One case of ff_maps_ref.GPU_CASES: the launch reported is the restated rule's; tau, flux and
    totals inside their bounds with the NaN pattern of the reference, +0.0 and the A = inf values
    bit for bit; every combination of NULL outputs that still writes a cube, and a repeated call,
    return the same bits; nothing is written outside the outputs or the exact-size workspace."""
    import torch
    c = M.make_case(k.npix, k.E, k.F)
    dA = torch.from_numpy(c["A"]).to(eng.device)
    if k.misaligned == "tavg":
        dT = torch.empty(k.npix + 3, dtype=torch.float64, device=eng.device)[1:k.npix + 1]
        assert dT.data_ptr() % 16 == 8
        dT.copy_(torch.from_numpy(c["tavg"]))
    else:
        dT = torch.from_numpy(c["tavg"]).to(eng.device)
    full = ("tau", "flux", "ftot") if k.outputs == "all" else ("ftot",)
    first, L = _call(eng, k, dA, dT, c, full, k.misaligned)
    assert L == M.case_launch(k)
    if k.misaligned:
        assert L.vec == 1 and k.npix % 2 == 0
    host = {n: t.cpu().numpy() for n, t in first.items()}
    r = M.judge(c, L, host.get("tau"), host.get("flux"), host["ftot"])
    print("%s %s: error / bound %s" % (M.case_id(k), _kernel_name(L), r))
    _note(_kernel_name(L), r)
    assert all(v <= 1.0 for v in r.values()), r
    assert np.isfinite(host["ftot"]).all()                 # NaN pixels are absent from the totals
    if k.outputs == "all":
        tau, flux = host["tau"], host["flux"]
        px = lambda kind, v: M.pixel_of(c, kind, v)
        # the NaN pattern is the reference's
        nan_a, nan_t = np.isnan(c["A"]), np.isnan(c["tavg"])
        assert np.array_equal(np.isnan(tau), np.broadcast_to(nan_a[:, None, :], tau.shape))
        assert np.array_equal(np.isnan(flux),
                              np.broadcast_to((nan_a | nan_t[None, :])[:, None, :], flux.shape))
        p = px("A", 0.0)
        if p is not None and not nan_t[p]:                  # +0.0 bit for bit
            assert np.all(tau[:, :, p].view(np.int64) == 0)
            assert np.all(flux[:, :, p].view(np.int64) == 0)
        p = px("A", np.inf)
        if p is not None and not nan_t[p]:
            assert np.all(tau[:, :, p] == np.inf)
            want = np.broadcast_to((c["cflux"] * c["tavg"][p])[None, :], flux[:, :, p].shape)
            assert np.array_equal(flux[:, :, p].view(np.int64),
                                  np.ascontiguousarray(want).view(np.int64))
        # every combination of NULL outputs that still writes a cube: the same bits
        for want in (("tau", "flux"), ("tau", "ftot"), ("flux", "ftot"), ("tau",), ("flux",)):
            got, L2 = _call(eng, k, dA, dT, c, want, k.misaligned)
            for n in want:
                if n != "ftot" or L2[:4] == L[:4]:      # (another lane width sums in another order)
                    assert _bits(got[n], first[n]), (want, n)
                else:
                    r2 = M.judge(c, L2, ftot=got[n].cpu().numpy())
                    assert r2["ftot"] <= 1.0, (want, r2)
    again, _ = _call(eng, k, dA, dT, c, full, k.misaligned)
    for n in full:
        assert _bits(again[n], first[n]), "a repeated call changed %s" % n


def test_totals_only_against_the_cube_kernels_totals(eng):
    """The two families group the flux product differently and sum in different orders: their
    totals agree to the sum of their bounds, not bit for bit."""
    import torch
    k = M.Case(2050, 3, 33, "all", None)
    c = M.make_case(k.npix, k.E, k.F)
    dA, dT = torch.from_numpy(c["A"]).to(eng.device), torch.from_numpy(c["tavg"]).to(eng.device)
    cube, L = _call(eng, k, dA, dT, c, ("tau", "flux", "ftot"), None)
    only, Lf = _call(eng, k, dA, dT, c, ("ftot",), None)
    assert L.kernel == "small" and Lf.kernel == "ftot"
    a = M.judge(c, L, ftot=cube["ftot"].cpu().numpy())["ftot"]
    b = M.judge(c, Lf, ftot=only["ftot"].cpu().numpy())["ftot"]
    print("totals of 2050 x 3 x 33: error / bound %.3f with the cubes, %.3f alone" % (a, b))
    assert a <= 1.0 and b <= 1.0


# ---- rjp_ff_step on a poisoned sightline ----------------------------------------------------------
def _bursts():
    from rajepy_amd.engine import make_bursts
    ej = U.example_bursts_params()
    red, blue = [], []
    for t0, hl, chi, which in zip(ej["t_0"], ej["hl"], ej["chi"], ej["which"]):
        sig = hl * orc.YEAR * 2. / (2. * np.sqrt(2. * np.log(2.)))
        for jet, lst in (("R", red), ("B", blue)):
            if jet in str(which):
                lst.append((t0 * orc.YEAR, chi - 1., sig))
    return make_bursts(red, blue)


@pytest.mark.parametrize("form", ["maps", "light curve"])
def test_step_on_a_poisoned_sightline(eng, form):
    """Launch times edited in place to values outside the declared range (as
    tests/test_gpu_round5.py does): the scan of rjp_ff_step writes NaN sums on those sightlines
    and its map stage, enqueued behind it in the same call, must not turn them into the flux of an
    optically thick sightline.  tau and flux are NaN on exactly those sightlines, the totals are
    the reference's over the others.  The flag is reported once, either way of asking: to
    range_guard() (after the maps) or by the next entry point, which is refused and enqueues
    nothing (after the light curve)."""
    import torch
    from rajepy_amd import _lib, engine as E
    from rajepy_amd.maths import physics as ph
    shape = (64, 64, 512)                        # 32768 sightlines x 64 rows: the table path
    nx, ny, nz = shape
    fields = eng.synth_fields(shape, 20240511 + 3, 0, 8, csize_au=0.5, wide=False,
                              tau_mode=E.RJP_GFF_SCALAR)
    b, ep = _bursts(), [1.0 * orc.YEAR]
    freqs = np.geomspace(1e9, 5e10, 5)
    ctau, cflux = E.ff_channel_coeffs(freqs, 0.5, 120., E.RJP_GFF_SCALAR,
                                      [ph.gff(nu, 1e4) for nu in freqs])
    ctau, cflux = np.asarray(ctau, dtype=np.float64), np.asarray(cflux, dtype=np.float64)
    tavg = eng.tavg(fields)
    P, F = fields.npix, len(freqs)
    want_maps = form == "maps"

    def step():
        out = (eng._f64(1, P), None, eng._f64(1, F, P) if want_maps else None,
               eng._f64(1, F, P) if want_maps else None, eng._f64(1, F))
        eng.ff_step(fields, b, ep, E.RJP_GFF_SCALAR, tavg, ctau, cflux, out)
        return out
    try:
        good = step()                                     # the first, accepted call
        assert eng.last_scan_path()[0] == "table"
        eng.synchronize()
        assert not eng.range_guard()
        lo, hi = fields.ts_range
        ts3 = fields.ts.view(nx, ny, nz)
        hit = [(3, 5, 7), (nx - 1, ny - 1, nz - 1), (10, 0, nz // 2)]
        saved = [ts3[i].item() for i in hit]
        ts3[hit[0]] = hi + 0.25 * (hi - lo)
        ts3[hit[1]] = lo - 1.0
        ts3[hit[2]] = hi * 10.0
        sumA, _, tau, flux, ftot = step()
        L = M.launch_rule(P, 1, F, want_maps, want_maps, True)
        assert eng.last_maps_launch() == tuple(L)
        eng.synchronize()
        pix = sorted({x * nz + z for (x, _, z) in hit})
        touched = set(pix) | {p ^ 1 for p in pix}          # two sightlines per lane
        A = sumA.cpu().numpy()
        nanpix = set(np.nonzero(np.isnan(A[0]))[0].tolist())
        assert set(pix) <= nanpix <= touched, (pix, sorted(nanpix))
        nan = np.isnan(A[0])
        c = dict(A=A, tavg=tavg.cpu().numpy(), ctau=ctau, cflux=cflux)
        assert (~np.isnan(c["tavg"][nan])).any()           # a flux there WOULD be finite
        if want_maps:
            th, fh = tau.cpu().numpy(), flux.cpu().numpy()
            assert np.array_equal(np.isnan(th[0]), np.broadcast_to(nan, (F, P)))
            assert np.array_equal(np.isnan(fh[0]),
                                  np.broadcast_to(nan | np.isnan(c["tavg"]), (F, P)))
            r = M.judge(c, L, th, fh, ftot.cpu().numpy())
        else:
            r = M.judge(c, L, ftot=ftot.cpu().numpy())
        print("step on %d poisoned sightlines, %s: error / bound %s" % (len(nanpix), form, r))
        _note("rjp_ff_step, " + _kernel_name(L), r)
        assert all(v <= 1.0 for v in r.values()), r
        assert np.isfinite(ftot.cpu().numpy()).all()
        # the poisoned sightlines are LEFT OUT of the light curve: what they gave before is missing
        gone = M.flux_ref(ctau, cflux, good[0].cpu().numpy()[0], c["tavg"])[:, sorted(nanpix)]
        drop = good[4].cpu().numpy()[0] - ftot.cpu().numpy()[0]
        np.testing.assert_allclose(drop, np.nansum(gone, axis=1).astype(np.float64), rtol=1e-6,
                                   atol=1e-9 * float(np.abs(ftot.cpu().numpy()).max()))
        if want_maps:
            assert eng.range_guard()                      # reports 1, and clears the flag
        else:
            marker = eng._f64(1, F).fill_(SENT)
            with pytest.raises(_lib.RjprtError) as ei:
                eng.ff_maps(good[0], tavg, ctau, cflux, want_tau=False, want_flux=False,
                            out=(None, None, marker))
            assert ei.value.status == _lib.RJP_ERR_ARG and "earlier scan" in str(ei.value)
            eng.synchronize()
            assert bool((marker == SENT).all()), "the refused call enqueued a map stage"
        for i, v in zip(hit, saved):
            ts3[i] = v
        again = step()
        eng.synchronize()
        assert not eng.range_guard()
        for a, g in zip(again, good):
            if a is not None:
                assert _bits(a, g)
    finally:
        eng.range_guard()


def test_last_maps_launch_before_any_map_stage_and_null_arguments():
    import ctypes as C
    from rajepy_amd import _lib
    from rajepy_amd.engine import RTEngine
    fresh = RTEngine(0)
    try:
        assert fresh.last_maps_launch() == (None, 0, 0, 0, 0, 0)
        buf = (C.c_int32 * 6)(*([-9] * 6))
        assert fresh.lib.rjp_last_maps_launch(None, buf) == _lib.RJP_ERR_ARG
        assert fresh.lib.rjp_last_maps_launch(fresh.ctx, None) == _lib.RJP_ERR_ARG
        assert list(buf) == [-9] * 6
    finally:
        fresh.close()
