"""Generator of tests/golden/k4_times.npz: launch times of jet cells at 50 digits.

    python tests/golden/make_k4_times_golden.py          (needs mpmath; about a minute)

For every case of CASES the geometry comes from oracle.rt_oracle.OracleJet in float64 (the clamped
axial distance rc = _r_clamped(|rr|), the cylindrical radius ww, the jet mask).  On a deterministic
sample of jet cells the flow time from r_0 to (rc, ww) -- the formula oracle/rt_oracle.py:t_rw
restates in float64 with scipy's hyp2f1 -- is evaluated with mpmath at 50 digits from those float64
inputs and rounded to float64 seconds.  Nothing else is stored: parameters, indices, numbers.

Per case `<name>` the file holds
    <name>/params   the model parameters handed to OracleJet, JSON
    <name>/shape    (n_x, n_y, n_z)
    <name>/idx      flat indices of the sampled cells (C order), ascending
    <name>/A, a, b  the 2F1 argument -A per cell and its parameters (float64)
    <name>/ts       reference launch times [s]
    <name>/ts_f64   the oracle's own float64 t_rw * YEAR on the same cells
and once `table_hash` (sha256 of the case table) and `families` / `tags` per case in `cases` (JSON).
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import rt_oracle as orc  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "k4_times.npz")
MAX_CELLS = 300
DPS = 50

# geometry presets: (inc, pa, rotation, (n_x, n_y, n_z)).  Axis-aligned jets run along z.
TILT_A = dict(inc=60.0, pa=25.0, rotation="CW", shape=(24, 64, 56))
TILT_B = dict(inc=35.0, pa=-40.0, rotation="CCW", shape=(28, 96, 24))
ALIGNED = dict(inc=90.0, pa=0.0, rotation="CCW", shape=(24, 24, 96))


def _case(name, family, eps, q_v, qd_v, geo, tags=(), **over):
    c = dict(name=name, family=family, eps=eps, q_v=q_v, qd_v=qd_v, tags=sorted(tags),
             inc=geo["inc"], pa=geo["pa"], rotation=geo["rotation"], shape=list(geo["shape"]),
             c_size=0.5, w_0=3.0, r_0=1.3, opang=30.0, R_1=0.3, R_2=0.75)
    c.update(over)
    return c


def _near(k, d):
    """q_v for eps = 0.5 with a - b = -(1 - q_v)/eps = -k + d."""
    return 1.0 - 0.5 * (k - d)


X, REF = "crossover", "may_refuse"
CASES = [
    # typical b
    _case("typ_tilted", "typical", 0.6, -0.1, -0.4, TILT_A, [X]),
    _case("typ_qd2", "typical", 2.0 / 3.0, -0.5, 2.0, TILT_B, [X]),
    _case("typ_eps025", "typical", 0.25, 0.1, 1.0, ALIGNED, [X]),
    _case("typ_eps79", "typical", 7.0 / 9.0, 0.0, 0.7, TILT_A, [X]),
    _case("typ_negb", "typical", 1.5, 0.2, -1.5, TILT_B, [X], w_0=1.5),
    # large b
    _case("big_b13", "large_b", 1.0 / 9.0, -0.3, 1.3, TILT_A, [X]),
    _case("big_b13_aligned", "large_b", 1.0 / 9.0, -0.3, 1.3, ALIGNED, [X]),
    _case("big_b20", "large_b", 1.0 / 9.0, -1.1, 1.35, TILT_B, [X]),
    _case("big_aneg", "large_b", 1.0 / 9.0, -0.3, -1.72, TILT_A, [X]),
    _case("big_b60", "large_b", 1.0 / 60.5, 0.0, 0.3, TILT_B, [X], opang=3.0),
    _case("big_b150", "large_b", 0.0066, 0.025, 2.5, TILT_A, [X], opang=1.5),
    _case("big_b180", "huge_b", 0.0055, 0.02, 1.5, ALIGNED, [X, REF], opang=1.5),
] + [
    _case("near1_d%g" % d, "near_degenerate", 0.5, _near(1, d), 1.0,
          ALIGNED if d in (1e-4, 2e-6) else TILT_A, [REF] if d <= 1e-5 else [])
    for d in (1e-2, 1e-4, 1e-5, 2e-6, 5e-7)
] + [
    _case("near3_d%g" % d, "near_degenerate", 0.5, _near(3, d), 1.0,
          ALIGNED if d in (1e-2, 1e-5) else TILT_B, [REF] if d <= 1e-5 else [])
    for d in (1e-2, 1e-4, 1e-5, 2e-6, 5e-7)
] + [
    # exactly degenerate: q_v = 0, eps = 1/2 -> a - b = -2.  Always refused; the host fallback
    _case("degenerate", "degenerate", 0.5, 0.0, 1.0, TILT_A, ["host"]),
    # a a non-positive integer: K2 = 0, the series terminate
    _case("aint_m1", "a_integer", 0.6, -0.1, -1.0, TILT_B),
    _case("aint_m2", "a_integer", 1.0 / 3.0, 0.2, -2.0, ALIGNED),
    # closed form, q^d_v = 0
    _case("closed_m15", "closed_form", 0.6, -1.5, 0.0, TILT_A),
    _case("closed_m03", "closed_form", 1.0 / 9.0, -0.3, 0.0, ALIGNED),
    _case("closed_p05", "closed_form", 2.0 / 3.0, 0.5, 0.0, TILT_B),
    _case("closed_p09", "closed_form", 0.6, 0.9, 0.0, TILT_A),
]


def table_hash():
    return hashlib.sha256(json.dumps(CASES, sort_keys=True).encode()).hexdigest()


def case_params(c):
    """The parameter dictionary OracleJet takes (no bursts: the launch times do not depend on them)."""
    nx, ny, nz = c["shape"]
    return {
        "target": {"name": c["name"], "dist": 140.0, "v_lsr": -3.5, "M_star": 0.8,
                   "R_1": c["R_1"], "R_2": c["R_2"]},
        "grid": {"n_x": nx, "n_y": ny, "n_z": nz, "l_z": None, "c_size": c["c_size"]},
        "geometry": {"epsilon": c["eps"], "opang": c["opang"], "w_0": c["w_0"], "r_0": c["r_0"],
                     "inc": c["inc"], "pa": c["pa"], "rotation": c["rotation"]},
        "power_laws": {"q_v": c["q_v"], "q_T": -0.05, "q_x": -0.2, "q^d_n": -0.5, "q^d_T": -0.1,
                       "q^d_v": c["qd_v"], "q^d_x": 0.2},
        "properties": {"v_0": 200.0, "x_0": 0.2, "T_0": 8000.0, "mu": 1.3, "mlr_bj": 1e-8,
                       "mlr_rj": 7.5e-9},
        "ejection": {"t_0": [], "hl": [], "chi": [], "which": []},
    }


def case_geometry(c):
    """(jet, rc, ww, mask, A, a, b): float64 geometry of a case, flat arrays over the grid."""
    p = case_params(c)
    for k in p["ejection"]:
        p["ejection"][k] = np.array(p["ejection"][k])
    jet = orc.OracleJet(p)
    g, t = jet.params["geometry"], jet.params["target"]
    rc = jet._r_clamped(np.abs(jet.rr)).ravel()
    ww = jet.ww.ravel()
    mask = np.isfinite(jet.fill_factor).ravel()
    rad = rc + g["mod_r_0"] - g["r_0"]
    with np.errstate(all="ignore"):
        wr = g["w_0"] * (rad / g["mod_r_0"]) ** g["epsilon"]
        A = (wr / ww) * t["R_1"] / (t["R_2"] - t["R_1"])
    a = c["qd_v"]
    b = (1. - c["q_v"] + c["eps"] * c["qd_v"]) / c["eps"]
    return jet, rc, ww, mask, A, a, b


def sample_cells(A, rc, r_0, mask, limit=MAX_CELLS):
    """Deterministic sample of jet cells: around A = 1 from both sides, both ends of A, the cells
    closest to r_0, the rest evenly strided over the mask."""
    cells = np.flatnonzero(mask)
    Am = A[cells]
    order = np.argsort(Am, kind="stable")
    above = order[Am[order] > 1.0]
    below = order[Am[order] <= 1.0]
    pick = [cells[above[:40]], cells[below[::-1][:40]], cells[order[::-1][:20]], cells[order[:20]],
            cells[np.argsort(rc[cells] - r_0, kind="stable")[:20]]]
    got = np.unique(np.concatenate(pick))
    rest = np.setdiff1d(cells, got)
    room = limit - got.size
    if room > 0 and rest.size:
        got = np.union1d(got, rest[np.linspace(0, rest.size - 1, min(room, rest.size)).astype(int)])
    return got


def ref_times(rc, ww, params, dps=DPS):
    """Flow time [s] from r_0 to (rc, ww) [au, float64] at `dps` digits, rounded to float64: the
    definite integral whose antiderivative is
        const rad^(1 - q_v) (r_eff / R_1)^-q^d_v (1 + A)^q^d_v 2F1(q^d_v, b; b + 1; -A)."""
    import mpmath as mp
    out = np.empty(len(rc))
    with mp.workdps(dps):
        f = mp.mpf
        au = f(orc.AU)
        g, t = params["geometry"], params["target"]
        w_0, r_0, mr0 = f(g["w_0"]) * au, f(g["r_0"]) * au, f(g["mod_r_0"]) * au
        eps = f(g["epsilon"])
        v_0 = f(params["properties"]["v_0"]) * f(1e3)
        r_1, r_2 = f(t["R_1"]) * au, f(t["R_2"]) * au
        q_v, q_vd = f(params["power_laws"]["q_v"]), f(params["power_laws"]["q^d_v"])
        const = mr0 ** q_v / (v_0 * (1 - q_v + eps * q_vd))
        b = (1 - q_v + eps * q_vd) / eps

        def indef(r_, w_):
            rad = r_ + mr0 - r_0
            p1 = rad ** (1 - q_v)
            if w_ == 0:
                return const * p1 * (1 + q_vd / (1 - q_v))
            w_r = w_0 * (rad / mr0) ** eps
            big_a = r_1 * w_r / (w_ * (r_2 - r_1))
            p2 = ((r_1 + (r_2 - r_1) * w_ / w_r) / r_1) ** -q_vd
            p3 = (big_a + 1) ** q_vd
            p4 = mp.hyp2f1(q_vd, b, b + 1, -big_a) if q_vd != 0 else f(1)
            return const * p1 * p2 * p3 * p4

        for i, (r, w) in enumerate(zip(rc, ww)):
            r_, w_ = f(float(r)) * au, f(float(w)) * au
            out[i] = float(mp.re(indef(r_, w_) - indef(r_0, w_)))
    return out


def build_case(c, with_ref=True):
    jet, rc, ww, mask, A, a, b = case_geometry(c)
    idx = sample_cells(A, rc, c["r_0"], mask, MAX_CELLS if "crossover" in c["tags"] else 160)
    if "crossover" in c["tags"]:
        Ai = A[idx]
        for lo, hi in ((0.0, 1.0), (1.0, 1.5), (1.5, 10.0)):
            n = int(((Ai > lo) & (Ai <= hi)).sum())
            assert n >= 20, (c["name"], "sampled cells with %g < A <= %g" % (lo, hi), n)
    assert idx.size <= MAX_CELLS and mask.sum() >= 1500, (c["name"], idx.size, int(mask.sum()))
    with np.errstate(all="ignore"):
        f64 = (orc.t_rw(rc[idx], ww[idx], jet.params) * orc.YEAR)
    out = {"params": json.dumps(case_params(c)), "shape": np.array(c["shape"]), "idx": idx.astype(np.int32),
           "A": A[idx], "a": np.float64(a), "b": np.float64(b), "ts_f64": f64}
    if with_ref:
        ts = ref_times(rc[idx], ww[idx], jet.params)
        assert np.isfinite(ts).all(), (c["name"], "50-digit value not finite")
        out["ts"] = ts
    return out, int(mask.sum())


def main():
    blob = {"table_hash": table_hash(),
            "cases": json.dumps([{k: c[k] for k in ("name", "family", "tags")} for c in CASES])}
    for c in CASES:
        out, n_mask = build_case(c)
        for k, v in out.items():
            blob[c["name"] + "/" + k] = v
        dev = np.abs(out["ts_f64"] - out["ts"]) / np.maximum(np.abs(out["ts"]), 1e-300)
        print("%-18s a %6.3f b %9.4f  mask %6d  sample %3d  A %.3g..%.3g  oracle dev %.1e"
              % (c["name"], out["a"], out["b"], n_mask, out["idx"].size, out["A"].min(),
                 out["A"].max(), np.nanmax(dev)))
    np.savez_compressed(OUT, **blob)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
