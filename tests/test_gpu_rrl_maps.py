"""The isothermal recombination-line map stage (rjp_rrl_maps: rrl_maps_kernel and the totals of
sum_partials_kernel) against the long-double reference and the term-by-term bound of
tests/rrl_maps_ref.py, which tests/test_rrl_maps_reference_cpu.py pins on the CPU: tail shapes
with every edge value planted, the radio band (where exp(x) - 1 for the Planck factor loses five
to six digits), the calling forms, and the products of JetModel on the two golden models."""
import numpy as np
import pytest

from tests import gpu_util as U
from tests import rrl_maps_ref as R

pytestmark = pytest.mark.gpu
YEAR = 31536000.0
_REF = {}                # case name -> (inputs, reference, bound): computed once, never changed


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()


def _reference(name, make):
    if name not in _REF:
        c = make()
        _REF[name] = (c, R.flux_ref(*R.args_of(c)), R.flux_bound(*R.args_of(c)))
    return _REF[name]


def _dev(eng, c):
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(eng.device)
    return up(c["tau_rrl"]), up(c["tau_ff"]), up(c["tavg"]), up(c["flux_ff"])


def _run(eng, c, **kw):
    t_l, t_c, tavg, cont = _dev(eng, c)
    flux, ftot = eng.rrl_maps(t_l, t_c, tavg, cont, c["cflux"], c["hnu_k"], **kw)
    eng.synchronize()
    return flux.cpu().numpy(), None if ftot is None else ftot.cpu().numpy()


def _judge(what, flux, ftot, ref, bound):
    """Prints and returns the worst measured / bound of the flux and of the totals."""
    assert np.array_equal(np.isnan(flux), np.isnan(ref))
    rf = R.worst_ratio(flux, ref, bound)
    rt = R.worst_ratio(ftot, R.ftot_ref(ref), R.ftot_bound(ref, bound))
    print("%s: measured / bound: flux %.3f, ftot %.3f" % (what, rf, rt))
    return rf, rt


# ---- tails and tiles ------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ff", [False, True], ids=["contsub", "total"])
@pytest.mark.parametrize("P,F", R.TAIL_SHAPES)
def test_tails_and_edge_values(eng, P, F, with_ff):
    """Every tail shape (one lane, a partial wave, a full wave, a partial and a full workgroup,
    one lane of a second, many workgroups, more workgroup partials than sum_partials_kernel has
    lanes), log-uniform inputs, the edge values of rrl_maps_ref.PLANTS at fixed pixels."""
    name = "tails-%dx%d-%s" % (P, F, "total" if with_ff else "contsub")
    c, ref, bound = _reference(name, lambda: R.tail_case(P, F, with_ff))
    flux, ftot = _run(eng, c)
    rf, rt = _judge(name, flux, ftot, ref, bound)
    assert rf <= 1.0 and rt <= 1.0
    assert np.isfinite(ftot).all()                          # NaN pixels are absent from the totals
    px = lambda n, v: R.pixel_of(n, v, P)
    if px("tau_rrl", 0.0) is not None:
        for n, _, v in R.PLANTS:
            assert px(n, v) is not None
        assert np.isnan(flux[:, px("tavg", np.nan)]).all()
        for v in (0.0, 745.0, 1e4):                         # 0 or subnormal line, never NaN
            assert np.isfinite(flux[:, px("tau_ff", v)]).all()
        if with_ff:
            assert np.isnan(flux[:, px("flux_ff", np.nan)]).all()
            assert np.isnan(flux).sum() == 2 * F
        else:
            # no line opacity: +0.0 bit for bit
            assert np.all(flux[:, px("tau_rrl", 0.0)].view(np.int64) == 0)
            assert np.isfinite(flux[:, px("flux_ff", np.nan)]).all()      # the line is kept
            assert np.isnan(flux).sum() == F
            for v in (745.0, 1e4):
                assert np.all(np.abs(flux[:, px("tau_ff", v)]) < 2.0 ** -1022)


# ---- the radio band --------------------------------------------------------------------------------
def test_radio_band(eng):
    """1, 5, 22, 50 GHz against 5e3 ... 2e4 K, x = h nu / k T from 2e-6 to 5e-4, thin and thick in
    line and continuum, P = 4097.  Measured on an MI355X: 8909 times the bound for the flux (94
    for the totals) with the Planck factor as 1 / (exp(x) - 1), 0.106 (0.025) of it with
    1 / expm1(x)."""
    c, ref, bound = _reference("radio", R.radio_case)
    flux, ftot = _run(eng, c)
    rf, rt = _judge("radio", flux, ftot, ref, bound)
    assert rf <= 1.0 and rt <= 1.0


# ---- calling forms -----------------------------------------------------------------------------------
def test_calling_forms_return_the_same_bits(eng):
    """want_ftot=False: the same flux; totals only (d_flux = NULL at the entry point): the same
    totals; the call repeated: nothing changes."""
    import torch
    from rajepy_amd import _lib
    c, ref, bound = _reference("tails-4097x5-total", lambda: R.tail_case(4097, 5, True))
    F, P = ref.shape
    t_l, t_c, tavg, cont = _dev(eng, c)
    bits = lambda t: t.view(torch.int64)
    flux, ftot = eng.rrl_maps(t_l, t_c, tavg, cont, c["cflux"], c["hnu_k"])
    rf, rt = _judge("calling forms", flux.cpu().numpy(), ftot.cpu().numpy(), ref, bound)
    assert rf <= 1.0 and rt <= 1.0
    only, none = eng.rrl_maps(t_l, t_c, tavg, cont, c["cflux"], c["hnu_k"], want_ftot=False)
    assert none is None and torch.equal(bits(only), bits(flux))
    again, tot2 = eng.rrl_maps(t_l, t_c, tavg, cont, c["cflux"], c["hnu_k"])
    assert torch.equal(bits(again), bits(flux)) and torch.equal(bits(tot2), bits(ftot))
    tot3 = torch.full((F,), float("nan"), dtype=torch.float64, device=eng.device)
    work = torch.empty(int(eng.lib.rjp_ff_maps_workspace(P, 1, F)), dtype=torch.uint8,
                       device=eng.device)
    eng._call("rjp_rrl_maps", t_l.data_ptr(), t_c.data_ptr(), tavg.data_ptr(), cont.data_ptr(), P,
              _lib.dbl_array(c["cflux"]), _lib.dbl_array(c["hnu_k"]), F, None, tot3.data_ptr(),
              work.data_ptr(), work.numel())
    eng.synchronize()
    assert torch.equal(bits(tot3), bits(ftot))


def test_per_call_tables_of_queued_calls(eng):
    """Calls queued without synchronisation that alternate and cycle through more (cflux, hnu_k)
    tables of equal length than the staging ring holds (8): each result against its own tables."""
    P, F = 700, 3
    base = R.tail_case(P, F, True)
    t_l, t_c, tavg, cont = _dev(eng, base)
    tables = [(base["cflux"] * (k + 1), base["hnu_k"] * (1.0 + 0.25 * k)) for k in range(11)]
    order = [0, 1, 0, 0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 0, 1, 10, 0]
    outs = [(k,) + eng.rrl_maps(t_l, t_c, tavg, cont, *tables[k]) for k in order]
    eng.synchronize()
    worst = [0.0, 0.0]
    for k, flux, ftot in outs:
        c = dict(base, cflux=tables[k][0], hnu_k=tables[k][1])
        rf, rt = R.ratios(flux.cpu().numpy(), ftot.cpu().numpy(), c)
        worst = [max(worst[0], rf), max(worst[1], rt)]
        assert rf <= 1.0 and rt <= 1.0, (k, rf, rt)
    print("queued calls: measured / bound: flux %.3f, ftot %.3f" % tuple(worst))


# ---- through JetModel -----------------------------------------------------------------------------
def _params(tag):
    from tests.test_gpu_model import tilted_params
    from tests.test_host_logic import example_params
    return example_params() if tag == "cfg1_example" else tilted_params()


@pytest.mark.parametrize("tag", ["cfg1_example", "tilted"])
def test_jetmodel_products_follow_their_own_maps(tmp_path, tag):
    """flux_rrl with and without the continuum and intensity_rrl, judged by the reference fed the
    model's own device maps (optical depths, T_avg, flux_ff): the coefficients of _rrl_flux (the
    intensity's division by omega / 1e-26) and its choice of continuum.  Then at a second epoch:
    the products follow that epoch's maps (the line cube and the map caches are per epoch)."""
    from rajepy_amd import classes, logger
    from rajepy_amd import engine as E
    z, meta, _ = U.load_golden(tag)
    jm = classes.JetModel(_params(tag), log=logger.Log(str(tmp_path / "a.log"), verbose=False))
    rf, rrl = np.asarray(z["rrl_freqs"], dtype=np.float64), meta["rrl"]
    F, P = len(rf), jm.nx * jm.nz
    dist = jm.params["target"]["dist"]
    cfl, hnu = E.rrl_channel_coeffs(rf, jm.csize, dist)
    cint = cfl / (E.solid_angle(jm.csize, dist) / 1e-26)
    seen, worst = [], 0.0
    for t in (float(z["years"][0]) * YEAR, float(z["years"][1]) * YEAR):
        jm.time = t
        sub = jm.flux_rrl(rrl, rf, contsub=True).reshape(F, P)
        tot = jm.flux_rrl(rrl, rf, contsub=False).reshape(F, P)
        ints = jm.intensity_rrl(rrl, rf).reshape(F, P)
        t_l = jm.optical_depth_rrl(rrl, rf).reshape(F, P)
        t_c = jm.optical_depth_ff(rf).reshape(F, P)
        cont = jm.flux_ff(rf).reshape(F, P)
        tavg = jm._model_tavg().cpu().numpy().reshape(P)
        assert np.isnan(tavg).any() and np.isfinite(sub).sum() > 100
        for what, got, ff, coef in (("contsub", sub, None, cfl), ("total", tot, cont, cfl),
                                    ("intensity", ints, None, cint)):
            args = (t_l, t_c, tavg, ff, coef, hnu)
            r = R.worst_ratio(got, R.flux_ref(*args), R.flux_bound(*args))
            print("%s, t = %.2f yr, %s: measured / bound %.3f" % (tag, t / YEAR, what, r))
            worst = max(worst, r)
        seen.append((t_l, sub))
    assert worst <= 1.0
    # the second epoch is another model state: its maps and products differ from the first's
    assert not np.array_equal(seen[0][0], seen[1][0])
    assert not np.array_equal(np.nan_to_num(seen[0][1]), np.nan_to_num(seen[1][1]))
