"""The reference of the burst-parameter sensitivities (tests/ff_grad_ref.py) held to the project's
independent single-epoch sum (gpu_util.ref_single_epoch), to Richardson-extrapolated central
differences of it, and to hand-worked cases; the host chain rule of JetModel.flux_vs_time_jac
(classes.ejection_chain_rule) held to differences of the conversion.  No GPU."""
import copy
import math

import numpy as np
import pytest

from oracle import rt_oracle as orc
from tests import ff_grad_ref as R
from tests import gpu_util as U

YEAR = orc.YEAR


def _perturbed(bursts, b, c, rel):
    """The burst lists with kernel parameter (b, c) moved by `rel` (of sigma for t0, of itself for
    amp_rel and inv2s2); -> (lists, the absolute step in the kernel parameter)."""
    out = [list(bursts[0]), list(bursts[1])]
    j, i = (0, b) if b < len(bursts[0]) else (1, b - len(bursts[0]))
    t0, amp, sg = out[j][i]
    k = 1.0 / (2.0 * sg ** 2)
    if c == 0:
        step = rel * sg
        out[j][i] = (t0 + step, amp, sg)
    elif c == 1:
        step = rel * amp
        out[j][i] = (t0, amp + step, sg)
    else:
        step = rel * k
        out[j][i] = (t0, amp, math.sqrt(1.0 / (2.0 * (k + step))))
    return out, step


def test_reference_sum_is_ref_single_epoch():
    a0, ts = R.synth_a0_ts((4, 96, 16), 20261001, "cells")
    bursts = U.example_burst_lists()
    for t in (0.8, 1.3, 2.5):
        ref = R.planes(a0, ts, bursts, t * YEAR)
        want = U.ref_single_epoch(a0, ts, bursts, t * YEAR)
        np.testing.assert_allclose(ref["S"].astype(np.float64), want, rtol=4e-16 * 96, atol=0)
        np.testing.assert_allclose(ref["absS"].astype(np.float64), want, rtol=4e-16 * 96, atol=0)


def test_planes_against_richardson_differences():
    """Every plane against (4 D(h / 2) - D(h)) / 3 of central differences of ref_single_epoch at
    relative steps 1e-3 and 5e-4 (of sigma for t0): <= 1e-9 of the plane's largest value (the
    h^4 term that is left; observed 2e-12)."""
    shape = (4, 96, 16)
    a0, ts = R.synth_a0_ts(shape, 20261001, "halves")
    bursts = U.example_burst_lists()
    t = 1.3 * YEAR
    ref = R.planes(a0, ts, bursts, t)
    nb = len(bursts[0]) + len(bursts[1])
    assert ref["D"].shape[0] == 3 * nb == 15
    worst = 0.0
    for b in range(nb):
        for c in range(3):
            est = []
            for rel in (1e-3, 5e-4):
                up, step = _perturbed(bursts, b, c, +rel)
                dn, _ = _perturbed(bursts, b, c, -rel)
                est.append((U.ref_single_epoch(a0, ts, up, t, threads=1) -
                            U.ref_single_epoch(a0, ts, dn, t, threads=1)) / (2.0 * step))
            rich = (4.0 * est[1] - est[0]) / 3.0
            got = ref["D"][3 * b + c].astype(np.float64)
            scale = np.abs(got).max()
            assert scale > 0
            err = float(np.abs(got - rich).max() / scale)
            worst = max(worst, err)
            assert err <= 1e-9, (b, c, err)
    print("worst plane against Richardson differences: %.2e of its largest value" % worst)


def test_chain_rule_against_differences():
    from rajepy_amd import classes
    ss = 1.3e17
    for t_0, peak, hl in ((0.5 * YEAR, 5.0 * ss, 0.15 * YEAR), (2.0 * YEAR, 0.4 * ss, 0.5 * YEAR),
                          (-0.3 * YEAR, 11.0 * ss, 0.02 * YEAR)):
        (t0, amp, inv), (d0, d1, d2) = classes.ejection_chain_rule(t_0, peak, hl, ss)
        want = R.chain_rule(t_0, peak, hl, ss)
        np.testing.assert_allclose((t0, amp, inv), want, rtol=1e-15)
        h = 1e-5
        fd0 = (R.chain_rule(t_0 + h * YEAR, peak, hl, ss)[0] -
               R.chain_rule(t_0 - h * YEAR, peak, hl, ss)[0]) / (2 * h * YEAR)
        fd1 = (R.chain_rule(t_0, peak * (1 + h), hl, ss)[1] -
               R.chain_rule(t_0, peak * (1 - h), hl, ss)[1]) / (2 * h * peak)
        fd2 = (R.chain_rule(t_0, peak, hl * (1 + h), ss)[2] -
               R.chain_rule(t_0, peak, hl * (1 - h), ss)[2]) / (2 * h * hl)
        # central differences at a relative step 1e-5: truncation 1e-10, rounding 1e-11
        np.testing.assert_allclose((d0, d1, d2), (fd0, fd1, fd2), rtol=1e-8)
        # the conversion is diagonal: a parameter moves no other kernel parameter
        assert R.chain_rule(t_0 + YEAR, peak, hl, ss)[1:] == want[1:]
        assert R.chain_rule(t_0, 2 * peak, hl, ss)[::2] == want[::2]
        assert R.chain_rule(t_0, peak, 2 * hl, ss)[:2] == want[:2]


def _one(a0, ts, bursts, t):
    r = R.planes(np.array([[[a0]]], dtype=np.float64), np.array([[[ts]]], dtype=np.float64),
                 bursts, t)
    return float(r["S"][0, 0]), [float(v) for v in r["D"][:, 0, 0]], \
        [float(v) for v in r["absD"][:, 0, 0]]


def test_hand_worked_cases(tmp_path):
    # one red cell, one red burst: every number from the formulas with math.exp (the hand formulas
    # are float64: up to ten roundings and exp's ulp, 2e-15; the helper works in long double)
    a0, ts, t = -2.0, 0.3, 1.2
    t0, amp, sg = 1.0, 3.0, 0.5
    k = 1.0 / (2.0 * sg ** 2)
    dd = (t - ts) - t0
    G = math.exp(-dd * dd * k)
    chi = 1.0 + amp * G
    S, D, aD = _one(a0, ts, ([(t0, amp, sg)], []), t)
    np.testing.assert_allclose(S, 2.0 * chi ** 2, rtol=2e-15)
    want = [2.0 * 2 * chi * amp * G * 2 * k * dd, 2.0 * 2 * chi * G, 2.0 * 2 * chi * amp * G * -dd * dd]
    np.testing.assert_allclose(D, want, rtol=2e-15)
    np.testing.assert_allclose(aD, np.abs(want), rtol=2e-15)
    assert D[0] < 0 < D[1] and D[2] < 0
    # the same burst registered for the BLUE jet: the red cell is untouched by it
    S, D, _ = _one(a0, ts, ([], [(t0, amp, sg)]), t)
    assert S == 2.0 and D == [0.0, 0.0, 0.0]
    # a NaN launch time in a jet with bursts: the term is dropped from every sum ...
    S, D, aD = _one(a0, math.nan, ([(t0, amp, sg)], []), t)
    assert S == 0.0 and D == [0.0] * 3 and aD == [0.0] * 3
    # ... in a jet without bursts chi = 1: |a0| in S, nothing in any derivative
    S, D, _ = _one(a0, math.nan, ([], [(t0, amp, sg)]), t)
    assert S == 2.0 and D == [0.0] * 3
    # NaN a0
    S, D, _ = _one(math.nan, ts, ([(t0, amp, sg)], [(t0, amp, sg)]), t)
    assert S == 0.0 and D == [0.0] * 6
    # a Gaussian far below 2^-1021 is an exact zero, not a denormal
    S, D, _ = _one(a0, ts, ([(t0 + 60.0, amp, sg)], []), t)
    assert S == 2.0 and D == [0.0] * 3
    # a negative amplitude: chi < 1, the amp_rel plane keeps the sign of chi
    S, D, _ = _one(a0, ts, ([(t0, -0.5, sg)], []), t)
    assert S < 2.0 and D[1] > 0 and D[0] > 0
    # two cells of one sightline, one per jet; plane order: the red jet's bursts first
    r = R.planes(np.array([[[-2.0], [3.0]]]), np.array([[[0.3], [0.1]]]),
                 ([(t0, amp, sg)], [(0.9, 1.5, 0.4)]), t)
    S1, D1, _ = _one(-2.0, 0.3, ([(t0, amp, sg)], []), t)
    S2, D2, _ = _one(3.0, 0.1, ([], [(0.9, 1.5, 0.4)]), t)
    np.testing.assert_allclose(float(r["S"][0, 0]), S1 + S2, rtol=2e-15)
    np.testing.assert_allclose(r["D"][:, 0, 0].astype(np.float64), D1 + D2, rtol=2e-15)

    # the model's parameter order: ejections R, B, B, RB register as events 1..5 = R, B, B, R, B;
    # kernel planes run over the red jet's bursts first (events 1, 4), then the blue jet's (2, 3, 5)
    from rajepy_amd import classes, logger
    p = copy.deepcopy(U.load_golden("cfg1_example")[2])
    p["ejection"] = U.example_bursts_params()
    jm = classes.JetModel(p, log=logger.Log(str(tmp_path / "m.log"), verbose=False))
    assert [e["which"] for e in jm.ejections.values()] == ["R", "B", "B", "R", "B"]
    slots = jm._ejection_slots()
    assert [k for k, _ in slots] == [0, 6, 9, 3, 12]
    for (k, chain), ej in zip(slots, jm.ejections.values()):
        want = classes.ejection_chain_rule(ej["t_0"], ej["peak_jml"], ej["half_life"],
                                           jm.ss_jml(ej["which"]))
        assert chain == want[1]
        # ... and that conversion is the one the model hands to the kernels
        j = "RB".index(ej["which"])
        i = (k // 3) - (len(jm._bursts["R"]) if j else 0)
        t0_, amp_, sg_ = jm._bursts["RB"[j]][i]
        np.testing.assert_allclose((t0_, amp_, 1.0 / (2.0 * sg_ ** 2)), want[0], rtol=1e-15)


@pytest.mark.parametrize("shape", R.COVER_SHAPES)
def test_reference_planes_are_not_vacuous(shape):
    """What tests/test_gpu_ff_grad.py asks of its references: every plane exceeds 1e-6 of its own
    maximum on at least 40 % of all sightlines (a jet owns half of them in the synthetic set)."""
    a0, ts = R.synth_a0_ts(shape, R.SEED, "halves")
    bursts = U.example_burst_lists()
    for t in R.EPOCHS_YR:
        ref = R.planes(a0, ts, bursts, t * YEAR)
        cov = [R.coverage(pl) for pl in ref["D"]]
        assert min(cov) >= R.MIN_COVER, (shape, t, cov)
