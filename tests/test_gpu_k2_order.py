"""K2's cube kernel (ff_maps_acc_kernel, ff_scan.hip) stores channel after channel: within a
channel, tau and flux of pixel group after pixel group.  The order of the stores is free; the
values are not: every voxel is what the map formulas give (classes.py:1395-1397, 1473-1475,
1519-1521; the tolerances of test_k2_per_lane_flux_accumulators_every_launch_shape), the cubes do
not depend on whether the totals are asked for, and a voxel does not depend on the launch shape --
the first 4096 pixels of a large map equal, bit for bit, a call on those pixels alone (the
small-map kernel).  These properties held before the order was changed as well: the module pins
them, on shapes the other K2 tests do not take (a partly live fourth pixel group, a 10-channel
last slice, two epochs)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NCHAN, NEP = 250, 2               # 15 slices of 16 channels + one of 10; two epochs


@pytest.fixture(scope="module")
def eng():
    from rajepy_amd.engine import RTEngine
    e = RTEngine(0)
    yield e
    e.close()


def _bits(a, b):
    import torch
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


# 65276 = 2 x (31 x 1024 + 894): 16-byte lanes, four pixel groups per lane, a last workgroup whose
# fourth group is partly live; 65277: the same with scalar lanes
@pytest.mark.parametrize("npix", [65276, 65277])
def test_k2_store_order_keeps_every_value(eng, npix):
    import torch
    rng = np.random.default_rng(npix)
    A = rng.uniform(1e-3, 3e3, (NEP, npix)) * 10.0 ** rng.uniform(-8, 2, (NEP, npix))
    T = rng.uniform(5e3, 2e4, npix)
    T[rng.random(npix) < 0.01] = np.nan                       # empty sightlines
    A[:, np.isnan(T)] = 0.0
    assert np.isnan(T[:4096]).any()
    ctau = 10.0 ** rng.uniform(-6, 1, NCHAN)
    cflux = 10.0 ** rng.uniform(-12, -8, NCHAN)
    dA, dT = torch.from_numpy(A).to(eng.device), torch.from_numpy(T).to(eng.device)
    tau, flux, ftot = eng.ff_maps(dA, dT, ctau, cflux)
    t2, f2, _ = eng.ff_maps(dA, dT, ctau, cflux, want_ftot=False)
    ts, fs, ftot_s = eng.ff_maps(dA[:, :4096].contiguous(), dT[:4096].contiguous(), ctau, cflux)
    eng.synchronize()
    want_tau = ctau[None, :, None] * A[:, None, :]
    want_flux = cflux[None, :, None] * (T[None, None, :] * -np.expm1(-want_tau))
    np.testing.assert_allclose(tau.cpu().numpy(), want_tau, rtol=1e-14)
    got_f = flux.cpu().numpy()
    assert np.array_equal(np.isnan(got_f), np.isnan(want_flux))
    np.testing.assert_allclose(got_f, want_flux, rtol=1e-13)
    np.testing.assert_allclose(ftot.cpu().numpy(), np.nansum(want_flux, axis=2), rtol=1e-12)
    np.testing.assert_allclose(ftot_s.cpu().numpy(), np.nansum(want_flux[:, :, :4096], axis=2),
                               rtol=1e-12)
    # with and without the totals
    assert _bits(tau, t2) and _bits(flux, f2)
    # the large map's kernel against the small map's, voxel by voxel
    assert _bits(tau[:, :, :4096], ts) and _bits(flux[:, :, :4096], fs)
