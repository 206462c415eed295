"""The NumPy reference of the RRL formal solution (tests/rrl_formal_ref.py), pinned on the two golden
models through the oracle before tests/test_gpu_rrl_formal.py holds the kernel to it: the
recurrence equals the difference of the two chains, and on the isothermal model the reference's
own product B(T_avg) e^-tau_ff (1 - e^-tau_rrl).  No GPU."""
import inspect
import os

import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import gpu_util as U
from tests import rrl_formal_ref as R


def _oracle_case(tag):
    from rajepy_amd import engine as E
    z, meta, p, g, jet = U.golden_dense(tag)
    jet.time = float(z["years"][0]) * orc.YEAR
    rf = np.asarray(z["rrl_freqs"], dtype=np.float64)
    with np.errstate(all="ignore"):
        c = jet.optical_depth_ff(rf, collapse=False)
        l = jet.optical_depth_rrl(meta["rrl"], rf, collapse=False)
    csrc, hnu_k = E.rrl_channel_coeffs(rf, jet.csize, p["target"]["dist"])
    return z, jet, c, l, csrc, hnu_k


@pytest.mark.parametrize("tag", ["cfg1_example", "tilted"])
def test_recurrence_equals_the_chain_difference_and_the_isothermal_product(tag):
    z, jet, c, l, csrc, hnu_k = _oracle_case(tag)
    rec = R.np_rrl_formal(c, l, jet.temperature, hnu_k, csrc)
    chains = R.np_rrl_formal_chains(c, l, jet.temperature, hnu_k, csrc)
    assert np.array_equal(np.isnan(rec), np.isnan(chains))
    top = np.nanmax(np.abs(rec), axis=(1, 2))[:, None, None]
    assert np.nanmax(np.abs(rec - chains) / top) <= 1e-10
    gold = z["flux_rrl_contsub"]
    assert np.array_equal(np.isnan(rec), np.isnan(gold))
    line = np.isfinite(gold) & (gold != 0.0)
    assert line.sum() > 100
    rel = np.abs(rec[line] / gold[line] - 1.0)
    if tag == "cfg1_example":
        # T is constant along every sightline: the sum telescopes to the reference's product
        assert rel.max() <= 1e-11, rel.max()
        assert R.within(rec, gold, 1e-11) <= 1.0
    else:
        # q_T = -0.05, q^d_T = -0.1: the isothermal product mis-weights the cells
        assert np.mean(rel > 1e-3) >= 0.5, np.mean(rel > 1e-3)
        assert rel.max() < 0.1


def test_two_cells_closed_form():
    """Cold in front of hot, both with line and continuum opacity: the recurrence against the
    closed form of two cells; negative when the hot cell behind is thick in the continuum."""
    c = np.array([0.3, 40.0]).reshape(1, 1, 2, 1)
    l = np.array([0.2, 0.5]).reshape(1, 1, 2, 1)
    temp = np.array([5e3, 2e4]).reshape(1, 2, 1)
    hk = np.array([1.07])
    B = 1.0 / np.expm1(hk[0] / temp.ravel())
    c1, c2, l1, l2 = 0.3, 40.0, 0.2, 0.5
    tot = B[0] * -np.expm1(-(c1 + l1)) + B[1] * -np.expm1(-(c2 + l2)) * np.exp(-(c1 + l1))
    cont = B[0] * -np.expm1(-c1) + B[1] * -np.expm1(-c2) * np.exp(-c1)
    got = R.np_rrl_formal(c, l, temp, hk, [1.0])[0, 0, 0]
    assert got == pytest.approx(tot - cont, rel=1e-12)
    assert got < 0.0
    mirror = R.np_rrl_formal(c[:, :, ::-1], l[:, :, ::-1], temp[:, ::-1], hk, [1.0])[0, 0, 0]
    assert mirror > 0.0


def test_pipeline_execute_accepts_formal_rrl(tmp_path):
    """`formal_rrl` is a keyword of Pipeline.execute (default False); formal=True alone still
    refuses a run table with an RRL run, formal=True with formal_rrl=True does not."""
    from rajepy_amd import classes, logger
    from tests.test_host_logic import example_params, pline_params
    par = inspect.signature(classes.Pipeline.execute).parameters
    assert par["formal_rrl"].default is False
    dcy = str(tmp_path / "out")
    os.makedirs(dcy)
    log = logger.Log(os.path.join(dcy, "model.log"), verbose=False)
    jm = classes.JetModel(example_params(), log=log)
    pl = classes.Pipeline(jm, pline_params(dcy), log=log)
    assert any(r.obs_type != "continuum" for r in pl.runs)
    with pytest.raises(ValueError):
        pl.execute(simobserve=False, verbose=False, dryrun=True, formal=True)
    for kw in ({"formal_rrl": True}, {"formal": True, "formal_rrl": True}):
        pl.execute(simobserve=False, verbose=False, dryrun=True, resume=False, **kw)
    assert par["formal"].default is False
