"""float64 NumPy reference of the RRL formal solution (rjp_rrl_formal, K6), shared by
tests/test_rrl_formal_reference_cpu.py (which pins it against the oracle) and
tests/test_gpu_rrl_formal.py (which holds the kernel to it).  Tests only."""
import numpy as np


def _clean(c_cells, l_cells, temp, hnu_k):
    """NaN optical depths are dropped (as nansum drops them); B = 1 / expm1(h nu / k T) of the cells
    that count, 0 (not NaN) for the others."""
    c = np.where(np.isnan(c_cells), 0.0, c_cells)
    l = np.where(np.isnan(l_cells), 0.0, l_cells)
    live = (c != 0.0) | (l != 0.0)
    with np.errstate(all="ignore"):
        B = 1.0 / np.expm1(np.asarray(hnu_k)[:, None, None, None] / temp[None])
    return c, l, np.where(live, B, 0.0)


def np_rrl_formal(c_cells, l_cells, temp, hnu_k, csrc):
    """c_cells, l_cells [F, nx, ny, nz]: per-cell continuum and line optical depths; temp
    [nx, ny, nz]; observer at iy = 0.  The recurrence of the issue: never forms I_tot - I_cont.
    -> [F, nx, nz], NaN where no cell of the sightline has T > 0."""
    c, l, B = _clean(c_cells, l_cells, temp, hnu_k)
    F, nx, ny, nz = c.shape
    I = np.zeros((F, nx, nz))
    D = np.zeros((F, nx, nz))
    Th = np.ones((F, nx, nz))
    for iy in range(ny):
        ci, li, Bi = c[:, :, iy], l[:, :, iy], B[:, :, iy]
        e_c = np.exp(-ci)
        om_l = -np.expm1(-li)
        u = -np.expm1(-(ci + li))
        I += Bi * (e_c * om_l * Th - u * D)
        D = e_c * (D + (Th - D) * om_l)
        Th = Th * e_c
    out = np.asarray(csrc)[:, None, None] * I
    out[:, ~np.any(temp > 0.0, axis=1)] = np.nan
    return out


def np_rrl_formal_chains(c_cells, l_cells, temp, hnu_k, csrc):
    """The same quantity as the difference of two formal solutions, I_tot - I_cont."""
    c, l, B = _clean(c_cells, l_cells, temp, hnu_k)

    def chain(dt):
        csum = np.cumsum(dt, axis=2)
        front = np.concatenate([np.zeros_like(csum[:, :, :1]), csum[:, :, :-1]], axis=2)
        return np.sum(B * -np.expm1(-dt) * np.exp(-front), axis=2)

    out = np.asarray(csrc)[:, None, None] * (chain(c + l) - chain(c))
    out[:, ~np.any(temp > 0.0, axis=1)] = np.nan
    return out


def within(got, ref, r):
    """|got - ref| <= r |ref| + r max_p |ref[f]| per channel, identical NaN patterns; -> the worst
    error in units of the bound."""
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    worst = 0.0
    for f in range(ref.shape[0]):
        ok = ~np.isnan(ref[f])
        if not ok.any():
            continue
        bound = r * np.abs(ref[f][ok]) + r * np.max(np.abs(ref[f][ok]))
        err = np.abs(got[f][ok] - ref[f][ok])
        if np.max(bound) == 0.0:
            assert np.all(err == 0.0)
            continue
        worst = max(worst, float(np.max(err / np.where(bound > 0, bound, 1.0))))
    return worst
