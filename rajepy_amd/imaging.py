"""The imaging chain -- the reference's simobserve -> tclean -> imfit, on the device -- as one unit:
the host-side conventions (scales, beams, antenna lists, observing plans, fit results), the result
types and the `Imager`, which takes flux maps or visibilities as device tensors through the K10-K16
wrappers of an `RTEngine`.  `JetModel` is a front to it.  `engine` re-exports the host helpers
(`engine.image_scales`, `engine.fit_beam`, ...), `classes` the result types; this imports neither.
"""
import collections
import os
import re

import numpy as np

from . import _constants as con


def vis_scales(freqs, csize_au, dist_pc):
    """su[f], sv[f] of `RTEngine.vis` / rjp_vis for baselines (u, v) in METRES, as measurement sets
    store them -- the one place that holds the sky convention:
      * V(u, v) = sum_p I_p exp(-2 pi i (u l_p + v m_p)), (l, m) the direction cosines towards
        East (RA) and North (Dec), u and v in wavelengths = metres * nu / c;
      * the phase centre is the map centre, pixel ((nx-1)/2, (nz-1)/2): CRPIX of `save_fits`;
      * one cell subtends cell = arctan(csize au / (dist pc)) radians (the square root of
        `solid_angle`); the FITS header `save_fits` writes has CDELT1 < 0 -- RA decreases with
        ix -- and CDELT2 > 0, so l = -cell (ix - (nx-1)/2), m = +cell (iz - (nz-1)/2):
        su = -cell nu / c,  sv = +cell nu / c   [cycles per cell per metre]."""
    freqs = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    cell = np.arctan((csize_au * con.au) / (dist_pc * con.parsec))
    return -cell * freqs / con.c, cell * freqs / con.c


def image_scales(freqs, cell_rad):
    """su[f], sv[f] of an image grid whose cells subtend `cell_rad` radians, for baselines in
    METRES, under the sky convention of `vis_scales` (phase centre = grid centre, RA decreasing
    with ix): su = -cell nu / c, sv = +cell nu / c.  `vis_scales` is the special case
    cell = arctan(csize au / dist).  For `RTEngine.vis_adjoint` (any imaging grid) and
    `RTEngine.vis`."""
    freqs = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    cell = float(cell_rad)
    return -cell * freqs / con.c, cell * freqs / con.c


# -- synthetic observations (K16): the host side ------------------------------------------------
SIDEREAL_DAY_S = 86164.0905        # the hour angle of a fixed direction advances one turn in this
WGS84_A, WGS84_F = 6378137.0, 1. / 298.257223563

AntennaConfig = collections.namedtuple("AntennaConfig", ["names", "xyz", "diameters", "observatory"])
Geodetic = collections.namedtuple("Geodetic", ["lat_deg", "lon_deg", "up", "lat0_deg", "lon0_deg",
                                               "up0"])


def read_antenna_config(path):
    """An antenna list in the format CASA simobserve reads -> `AntennaConfig` (names [A], xyz
    [A, 3] in metres, diameters [A] in metres, observatory).  `#` lines form the header and carry
    `observatory=` and `coordsys=`; every other non-blank line is `x y z diameter name`.  Only
    `coordsys=XYZ` (geocentric ITRF positions) is read: `UTM` and `LOC` lists, which need a datum
    or a site position, raise ValueError naming the system, as does a malformed line."""
    obs, coordsys, names, xyz, diam = None, None, [], [], []
    with open(path, "rt") as f:
        for no, line in enumerate(f, 1):
            text = line.strip()
            if not text:
                continue
            if text.startswith("#"):
                for key, val in re.findall(r"(\w+)\s*=\s*(\S+)", text[1:]):
                    if key.lower() == "observatory":
                        obs = val
                    elif key.lower() == "coordsys":
                        coordsys = val.upper()
                continue
            cols = text.split()
            if len(cols) < 5:
                raise ValueError("%s:%d: expected `x y z diameter name`, found %d columns"
                                 % (path, no, len(cols)))
            try:
                vals = [float(c) for c in cols[:4]]
            except ValueError:
                raise ValueError("%s:%d: x, y, z and diameter must be numbers" % (path, no)) from None
            if not np.all(np.isfinite(vals)) or not vals[3] > 0.:
                raise ValueError("%s:%d: non-finite position or non-positive diameter" % (path, no))
            xyz.append(vals[:3])
            diam.append(vals[3])
            names.append(cols[4])
    if coordsys is None:
        raise ValueError("%s: no `# coordsys=` header line" % path)
    if not coordsys.startswith("XYZ"):
        raise ValueError("%s: coordsys=%s is not supported (geocentric XYZ lists only)"
                         % (path, coordsys))
    if len(names) < 2:
        raise ValueError("%s: fewer than two antennas" % path)
    if len(set(names)) != len(names):
        raise ValueError("%s: antenna names are not unique" % path)
    return AntennaConfig(names, np.array(xyz, dtype=np.float64), np.array(diam, dtype=np.float64),
                         obs)


def _geodetic_one(x, y, z):
    """WGS84 latitude, east longitude [rad] of geocentric (x, y, z) [m]: the fixed point of
    lat = atan2(z, p (1 - e^2 N / (N + h))), which contracts by ~e^2 per step."""
    e2 = WGS84_F * (2. - WGS84_F)
    p = np.hypot(x, y)
    lon = np.arctan2(y, x)
    lat = np.arctan2(z, p * (1. - e2))
    for _ in range(12):
        n = WGS84_A / np.sqrt(1. - e2 * np.sin(lat) ** 2)
        h = p / np.cos(lat) - n if abs(np.cos(lat)) > 1e-8 else abs(z) - n * (1. - e2)
        lat = np.arctan2(z, p * (1. - e2 * n / (n + h)))
    return lat, lon


def geodetic(xyz):
    """WGS84 geodetic latitude and EAST longitude [deg] and the unit local vertical (the ellipsoid
    normal, in the geocentric frame of `xyz`) of every antenna of `xyz` [A, 3] [m], and the same
    three of the mean position -> `Geodetic`.  The verticals are what `RTEngine.uv_tracks` takes
    as `up`; lat0 / lon0 place the array for `observing_plan` and the hour angle."""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    pts = np.vstack([xyz, xyz.mean(axis=0)[None, :]])
    ll = np.array([_geodetic_one(*p) for p in pts])
    lat, lon = ll[:, 0], ll[:, 1]
    up = np.stack([np.cos(lat) * np.cos(lon), np.cos(lat) * np.sin(lon), np.sin(lat)], axis=1)
    return Geodetic(np.degrees(lat[:-1]), np.degrees(lon[:-1]), up[:-1], float(np.degrees(lat[-1])),
                    float(np.degrees(lon[-1])), up[-1])


def observing_plan(dec_deg, lat_deg, t_obs_s, t_int_s, min_el_deg, hourangle_h=0.):
    """The integrations of `t_obs_s` seconds on a target at declination `dec_deg` from latitude
    `lat_deg` -> (local hour angles in TURNS [n], day of each [n]) -- the reference's rule for
    splitting an observation over days (classes.py:2510-2550), stated here:
      * `time_up` = 86400 s if the target is above `min_el_deg` at lower culmination, else
        int(7200 H) with H = arccos((sin el - sin lat sin dec) / (cos lat cos dec)) in hours;
        ValueError if the target never reaches the limit;
      * the days last [time_up] * (t_obs // time_up) and then the remainder WHEN IT IS NOT ZERO
        (the reference appends a day of length zero);
      * every day is centred on `hourangle_h` and holds max(1, floor(T / t_int)) integrations of
        `t_int_s`, placed symmetrically about the centre and taken at their mid-points;
      * the hour angle advances one turn per SIDEREAL_DAY_S.
    The reference's eight-scan split of the last day for east-west arrays is not made."""
    t_obs, t_int = float(t_obs_s), float(t_int_s)
    if not (t_obs > 0. and t_int > 0. and np.isfinite(t_obs) and np.isfinite(t_int)):
        raise ValueError("observing_plan: t_obs_s and t_int_s must be positive")
    dec, lat, el = np.radians(dec_deg), np.radians(lat_deg), np.radians(min_el_deg)
    low = np.arcsin(np.clip(np.sin(lat) * np.sin(dec) - np.cos(lat) * np.cos(dec), -1., 1.))
    if low > el:
        time_up = 86400
    else:
        den = np.cos(lat) * np.cos(dec)
        ch = (np.sin(el) - np.sin(lat) * np.sin(dec)) / den if den != 0. else np.inf
        if not ch <= 1.:
            raise ValueError("observing_plan: a target at declination %.3f deg never reaches an "
                             "elevation of %.3f deg from latitude %.3f deg"
                             % (dec_deg, min_el_deg, lat_deg))
        time_up = int(7200. * np.degrees(np.arccos(max(ch, -1.))) / 15.)
        if time_up < 1:
            raise ValueError("observing_plan: the target is above %.3f deg for less than a second "
                             "a day" % min_el_deg)
    days = [float(time_up)] * int(t_obs // time_up)
    rest = t_obs - (t_obs // time_up) * time_up
    if rest > 0.:
        days.append(rest)
    ha, day = [], []
    for d, T in enumerate(days):
        n = max(1, int(np.floor(T / t_int)))
        mid = (np.arange(n) + 0.5 - 0.5 * n) * t_int
        ha.append(float(hourangle_h) / 24. + mid / SIDEREAL_DAY_S)
        day.append(np.full(n, d, dtype=np.int64))
    return np.concatenate(ha), np.concatenate(day)


def thermal_sigma(sefd_jy, chanwidth_hz, t_int_s, n_pol=2, efficiency=1.):
    """The rms [Jy] of the real and of the imaginary part of ONE visibility -- one baseline, one
    channel of `chanwidth_hz`, one integration of `t_int_s`, `n_pol` polarisations averaged --
    of an array of identical antennas of system-equivalent flux density `sefd_jy`:
    SEFD / (efficiency sqrt(2 n_pol chanwidth t_int))."""
    sefd, dnu, t = (np.asarray(x, dtype=np.float64) for x in (sefd_jy, chanwidth_hz, t_int_s))
    if np.any(~(sefd >= 0.)) or np.any(~(dnu > 0.)) or np.any(~(t > 0.)) or n_pol < 1 or \
            not efficiency > 0.:
        raise ValueError("thermal_sigma: sefd_jy >= 0, chanwidth_hz, t_int_s, n_pol and "
                         "efficiency > 0")
    return sefd / (float(efficiency) * np.sqrt(2. * n_pol * dnu * t))


def image_rms(iw, sigma_k):
    """The thermal rms [Jy / beam] of a dirty image made with the imaging weights `iw` ([K], or
    [M, K] -> one value per map) from visibilities whose real and imaginary parts have the rms
    `sigma_k` (one number, [K], [M, 1] or [M, K]): sqrt(sum w'^2 sigma^2) / sum w'.  Flagged
    visibilities carry the weight 0 and drop out; a map without weights gives NaN."""
    w = np.atleast_2d(np.asarray(iw, dtype=np.float64))
    s = np.broadcast_to(np.asarray(sigma_k, dtype=np.float64), w.shape)
    live = w > 0.
    num = np.sqrt(np.sum(np.where(live, (w * s) ** 2, 0.), axis=1))
    with np.errstate(invalid="ignore", divide="ignore"):
        return num / np.sum(np.where(live, w, 0.), axis=1)


def antenna_config_path(directory, telescope, config):
    """The antenna list of (`telescope`, `config`) in `directory`, found by name without regard
    to case: `<tel>.<cfg>.cfg`, `<tel>_<cfg>.cfg`, or `<tel>.cfg` when the configuration is
    '0' (a telescope with one) -> its path, or None."""
    tel, cfg = str(telescope).lower(), str(config).lower()
    want = [tel + "." + cfg + ".cfg", tel + "_" + cfg + ".cfg"] + ([tel + ".cfg"] if cfg == "0" else [])
    try:
        have = {name.lower(): name for name in sorted(os.listdir(directory), reverse=True)}
    except OSError:
        return None
    for name in want:
        if name in have:
            return os.path.join(directory, have[name])
    return None


def observation_grid(max_baseline_m, freq_hz, extent_as):
    """(cell [arcsec], image side [cells]) the reference images a synthetic observation on
    (classes.py:2674-2678, 2753-2759): the cell is a quarter of 1 / (longest baseline in
    wavelengths), rounded to 1e-6 arcsec; the side is ceil(2 extent / cell) for a model that
    spans `extent_as`, and at least 500."""
    beam_as = np.degrees(1. / (float(max_baseline_m) * float(freq_hz) / con.c)) * 3600.
    cell_as = float("%.6f" % (beam_as / 4.))
    if not cell_as > 0.:
        raise ValueError("observation_grid: the cell rounds to 0 at 1e-6 arcsec")
    return cell_as, max(500, int(np.ceil(2. * float(extent_as) / cell_as)))


_FOUR_LN2 = 4. * np.log(2.)


def beam_quadratic(bmaj_as, bmin_as, bpa_deg, cell_rad):
    """(A, B, C) [cells^-2] of `RTEngine.restore` / rjp_restore for an elliptical Gaussian clean
    beam exp(-(A dx^2 + 2 B dx dz + C dz^2)) -- the one place that holds the convention:
      * `bmaj_as`, `bmin_as` [arcsec] are FWHM: along an axis of FWHM w the beam is
        exp(-4 ln2 s^2 / w^2);
      * `bpa_deg` is the position angle of the major axis, from North through East.  North is +z
        and East is DECREASING ix (RA decreases with ix: `vis_scales`), so the major axis points
        along (dx, dz) = (-sin bpa, cos bpa): with bpa = 0 it lies along z;
      * (dx, dz) are in cells of `cell_rad` radians."""
    cell_as = np.degrees(float(cell_rad)) * 3600.
    ka = _FOUR_LN2 / (float(bmaj_as) / cell_as) ** 2
    kb = _FOUR_LN2 / (float(bmin_as) / cell_as) ** 2
    s, c = np.sin(np.radians(float(bpa_deg))), np.cos(np.radians(float(bpa_deg)))
    return (float(ka * s * s + kb * c * c), float((kb - ka) * s * c),
            float(ka * c * c + kb * s * s))


def beam_from_quadratic(A, B, C, cell_rad):
    """The inverse of `beam_quadratic`: (bmaj_as, bmin_as, bpa_deg) of a positive definite
    (A, B, C) [cells^-2], bpa in (-90, 90]."""
    lam, vec = np.linalg.eigh(np.array([[A, B], [B, C]], dtype=np.float64))
    if not lam[0] > 0.:
        raise ValueError("beam: (A, B, C) is not positive definite")
    cell_as = np.degrees(float(cell_rad)) * 3600.
    ex, ez = vec[:, 0]                             # the major axis: the smaller eigenvalue
    bpa = np.degrees(np.arctan2(-ex, ez))
    bpa = bpa - 180. if bpa > 90. else bpa + 180. if bpa <= -90. else bpa
    return (float(np.sqrt(_FOUR_LN2 / lam[0]) * cell_as),
            float(np.sqrt(_FOUR_LN2 / lam[1]) * cell_as), float(bpa))


def fit_beam(patch):
    """(A, B, C) [cells^-2] of the Gaussian that fits the main lobe of a dirty beam: `patch` is a
    2-D array [odd, odd] around the beam's centre pixel; a linear least-squares fit of
    -ln(patch / centre) = A dx^2 + 2 B dx dz + C dz^2 over the pixels >= half the centre value
    that are connected to the centre (4-neighbours), as tclean fits its restoring beam."""
    b = np.asarray(patch, dtype=np.float64)
    if b.ndim != 2 or b.shape[0] % 2 == 0 or b.shape[1] % 2 == 0:
        raise ValueError("fit_beam: `patch` must be 2-D with odd sizes")
    cx, cz = (b.shape[0] - 1) // 2, (b.shape[1] - 1) // 2
    if not (np.isfinite(b[cx, cz]) and b[cx, cz] > 0.):
        raise ValueError("fit_beam: the centre of the beam must be positive")
    b = b / b[cx, cz]
    lobe = np.zeros(b.shape, dtype=bool)
    todo = [(cx, cz)]
    while todo:
        i, j = todo.pop()
        if 0 <= i < b.shape[0] and 0 <= j < b.shape[1] and not lobe[i, j] and b[i, j] >= 0.5:
            lobe[i, j] = True
            todo += [(i + 1, j), (i - 1, j), (i, j + 1), (i, j - 1)]
    ii, jj = np.nonzero(lobe)
    dx, dz = (ii - cx).astype(np.float64), (jj - cz).astype(np.float64)
    design = np.stack([dx * dx, 2. * dx * dz, dz * dz], axis=1)
    if np.linalg.matrix_rank(design) < 3:
        raise ValueError("fit_beam: the main lobe covers too few pixels (the beam is not resolved "
                         "by the cell)")
    sol = np.linalg.lstsq(design, -np.log(b[ii, jj]), rcond=None)[0]
    A, B, C = (float(x) for x in sol)
    if not (A > 0. and C > 0. and A * C > B * B):
        raise ValueError("fit_beam: the fitted form is not positive definite")
    return A, B, C


def gauss_start(img, nx, nz, beam_abc, box=None, mask=None):
    """The default start of `RTEngine.gaussfit` -> tensor [M, 6] beside `img`: per map the
    counting pixel (inside `box`, non-zero in `mask`, finite) of largest |I|, its value and
    position, and the clean beam's (A, B, C) -- a point source as the beam sees it.  `img`: a
    float64 tensor of M * nx * nz values; `beam_abc`: one (A, B, C) or one per map.  Plain torch,
    batched, nothing goes to the host.  A map without a counting pixel gets a NaN peak, which
    `gaussfit` reports as status 3.  (The reference's own estimate comes from the model's
    tau = 1 surface, classes.py:2718-2743; a caller may pass any start instead.)"""
    import torch
    nx, nz = int(nx), int(nz)
    t = img.reshape(-1, nx, nz)
    M = int(t.shape[0])
    ok = torch.zeros(nx, nz, dtype=torch.bool, device=t.device)
    i0, i1, j0, j1 = (0, nx - 1, 0, nz - 1) if box is None else (int(x) for x in np.ravel(box))
    ok[i0:i1 + 1, j0:j1 + 1] = True
    if mask is not None:
        if not isinstance(mask, torch.Tensor):
            mask = torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0))
        ok &= (mask != 0).to(t.device).reshape(nx, nz)
    ok = ok.unsqueeze(0) & torch.isfinite(t)
    mag = torch.where(ok, t.abs(), torch.full_like(t, -1.0)).reshape(M, -1)
    top, idx = mag.max(dim=1)
    val = t.reshape(M, -1).gather(1, idx.unsqueeze(1)).squeeze(1)
    val = torch.where(top >= 0, val, torch.full_like(val, float("nan")))
    abc = np.asarray(beam_abc, dtype=np.float64).reshape(-1, 3)
    if abc.shape[0] not in (1, M):
        raise ValueError("gauss_start: `beam_abc` must be one (A, B, C) or one per map (%d)" % M)
    abc = torch.from_numpy(np.array(np.broadcast_to(abc, (M, 3)))).to(t.device)
    pos = torch.stack([torch.div(idx, nz, rounding_mode="floor"), idx % nz], dim=1)
    return torch.cat([val.unsqueeze(1), pos.to(torch.float64), abc], dim=1).contiguous()


def gauss_results(theta, cov, chi2, npix, beam_abc, cell_rad, rms=None, shape=None, status=None):
    """What CASA imfit reports, from the outputs of `RTEngine.gaussfit` (host arrays; pure NumPy)
    -> one dict per map.  Conventions as in `beam_quadratic`; `beam_abc`: the clean beam, one
    (A, B, C) or one per map; `cell_rad`: the cell in radians.
      * 'peak' [Jy / beam] = S;  'I' = {'val': S sqrt(det Q_beam / det Q_fit), 'unit': 'Jy'}, the
        integrated flux (Q = [[A, B], [B, C]]);
      * 'x0', 'z0' [pixels]; with `shape` = (nx, nz) also 'east_as', 'north_as', the offsets from
        the map centre ((nx-1)/2, (nz-1)/2) in arcsec under the sky convention of `vis_scales`
        (East = DECREASING ix, North = +z);
      * 'maj_as', 'min_as', 'pa_deg': the fitted size (`beam_from_quadratic`);
      * 'deconvolved': {'maj_as', 'min_as', 'pa_deg'} of Sigma_src = (2 Q_fit)^-1 - (2 Q_beam)^-1,
        or None with 'point_source' True where that is not positive definite;
      * with `rms` [Jy / beam] (one number or one per map) the 1-sigma errors 'peak_err',
        'x0_err', 'z0_err', 'abc_err' and 'Ierr' = {'val', 'unit'} from the covariance
        rms^2 Omega_b (J^T J)^-1, Omega_b = pi / sqrt(det Q_beam) cells: the usual inflation for
        noise that is correlated over a beam; Ierr by first-order propagation through
        I(S, A, B, C).  This is a STATED APPROXIMATION, not the expressions of Condon (1997)
        that CASA uses.  Without `rms`: None;
      * 'chi2', 'npix', and 'status' where given.
    A map whose fit is not finite and positive definite (status 3) gets NaN / None entries."""
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, 6)
    M = theta.shape[0]
    cov = np.asarray(cov, dtype=np.float64).reshape(M, 21)
    chi2, npix = np.asarray(chi2, dtype=np.float64).reshape(M), np.asarray(npix).reshape(M)
    beam = np.broadcast_to(np.asarray(beam_abc, dtype=np.float64).reshape(-1, 3), (M, 3))
    rms_m = None if rms is None else np.broadcast_to(np.asarray(rms, dtype=np.float64), (M,))
    cell_as = np.degrees(float(cell_rad)) * 3600.
    nan = float("nan")
    out = []
    for m in range(M):
        S, x0, z0, A, B, C = (float(v) for v in theta[m])
        bA, bB, bC = (float(v) for v in beam[m])
        det, bdet = A * C - B * B, bA * bC - bB * bB
        d = {"peak": S, "x0": x0, "z0": z0, "chi2": float(chi2[m]), "npix": int(npix[m]),
             "I": {"val": nan, "unit": "Jy"}, "Ierr": {"val": None, "unit": "Jy"},
             "maj_as": nan, "min_as": nan, "pa_deg": nan, "deconvolved": None,
             "point_source": False, "peak_err": None, "x0_err": None, "z0_err": None,
             "abc_err": None}
        if status is not None:
            d["status"] = int(np.asarray(status).reshape(M)[m])
        if shape is not None:
            d["east_as"] = float(-(x0 - (int(shape[0]) - 1) / 2.) * cell_as)
            d["north_as"] = float((z0 - (int(shape[1]) - 1) / 2.) * cell_as)
        good = np.all(np.isfinite(theta[m])) and A > 0. and C > 0. and det > 0. and bdet > 0.
        if not good:
            out.append(d)
            continue
        flux = S * np.sqrt(bdet / det)
        d["I"]["val"] = float(flux)
        d["maj_as"], d["min_as"], d["pa_deg"] = beam_from_quadratic(A, B, C, cell_rad)
        # covariance matrices of the Gaussians: Sigma = (2 Q)^-1
        sig = (np.array([[C, -B], [-B, A]]) / (2. * det)
               - np.array([[bC, -bB], [-bB, bA]]) / (2. * bdet))
        sdet = sig[0, 0] * sig[1, 1] - sig[0, 1] * sig[1, 0]
        if sig[0, 0] > 0. and sig[1, 1] > 0. and sdet > 0.:
            q = np.array([[sig[1, 1], -sig[0, 1]], [-sig[0, 1], sig[0, 0]]]) / (2. * sdet)
            mj, mn, pa = beam_from_quadratic(q[0, 0], q[0, 1], q[1, 1], cell_rad)
            d["deconvolved"] = {"maj_as": mj, "min_as": mn, "pa_deg": pa}
        else:
            d["point_source"] = True
        if rms_m is not None and np.all(np.isfinite(cov[m])):
            N = np.zeros((6, 6))
            k = 0
            for i in range(6):
                for j in range(i, 6):
                    N[i, j] = N[j, i] = cov[m, k]
                    k += 1
            try:
                P = rms_m[m] ** 2 * (np.pi / np.sqrt(bdet)) * np.linalg.inv(N)
            except np.linalg.LinAlgError:
                P = None
            if P is not None and np.all(np.diag(P) >= 0.):
                sd = np.sqrt(np.diag(P))
                d["peak_err"], d["x0_err"], d["z0_err"] = float(sd[0]), float(sd[1]), float(sd[2])
                d["abc_err"] = (float(sd[3]), float(sd[4]), float(sd[5]))
                grad = np.array([flux / S if S != 0. else np.sqrt(bdet / det), 0., 0.,
                                 -flux * C / (2. * det), flux * B / det, -flux * A / (2. * det)])
                d["Ierr"]["val"] = float(np.sqrt(grad @ P @ grad))
        out.append(d)
    return out


# -- fits in the uv plane (K20): the host side ------------------------------------------------------
UVFIT_MAX_COMP = 2           # RJP_UVFIT_MAX_COMP
_FWHM_PER_SIGMA = float(np.sqrt(8. * np.log(2.)))


def uvfit_theta(flux, east_as, north_as, maj_as, min_as, pa_deg, cell_rad):
    """(F, x, z, sxx, sxz, szz) of `RTEngine.uvfit` / rjp_uvfit for one component, under the
    conventions of `vis_scales` and `beam_quadratic`: `flux` in the visibilities' unit; the offset
    from the phase centre (`east_as`, `north_as`) [arcsec] with East = DECREASING ix and North =
    +z, so x = -east / cell, z = north / cell; `maj_as`, `min_as` FWHM [arcsec] and `pa_deg` the
    position angle of the major axis from North through East: the major axis points along
    (dx, dz) = (-sin pa, cos pa), and Sigma = sig_maj^2 e e^T + sig_min^2 f f^T [cells^2] with
    sig = FWHM / sqrt(8 ln 2).  `maj_as` = 0 gives a point (Sigma = 0)."""
    cell_as = np.degrees(float(cell_rad)) * 3600.
    if not (float(maj_as) >= 0. and float(min_as) >= 0.):
        raise ValueError("uvfit_theta: maj_as and min_as must be >= 0")
    if float(maj_as) == 0.:
        return np.array([float(flux), -float(east_as) / cell_as, float(north_as) / cell_as,
                         0., 0., 0.])
    vM = (float(maj_as) / cell_as / _FWHM_PER_SIGMA) ** 2
    vm = (float(min_as) / cell_as / _FWHM_PER_SIGMA) ** 2
    s, c = np.sin(np.radians(float(pa_deg))), np.cos(np.radians(float(pa_deg)))
    return np.array([float(flux), -float(east_as) / cell_as, float(north_as) / cell_as,
                     vM * s * s + vm * c * c, (vm - vM) * s * c, vM * c * c + vm * s * s])


def uvfit_components(theta, cell_rad):
    """The inverse of `uvfit_theta` for one component (6 values) -> (flux, east_as, north_as,
    maj_as, min_as, pa_deg), pa in (-90, 90]; a Sigma that is zero gives maj = min = pa = 0; one
    that is not positive semi-definite raises ValueError."""
    F, x, z, sxx, sxz, szz = (float(t) for t in np.asarray(theta, dtype=np.float64).reshape(6))
    cell_as = np.degrees(float(cell_rad)) * 3600.
    if sxx == 0. and sxz == 0. and szz == 0.:
        return F, -x * cell_as, z * cell_as, 0., 0., 0.
    lam, vec = np.linalg.eigh(np.array([[sxx, sxz], [sxz, szz]], dtype=np.float64))
    if not lam[0] >= -1e-15 * abs(lam[1]):
        raise ValueError("uvfit_components: Sigma is not positive semi-definite")
    ex, ez = vec[:, 1]                              # the major axis: the larger eigenvalue
    pa = np.degrees(np.arctan2(-ex, ez))
    pa = pa - 180. if pa > 90. else pa + 180. if pa <= -90. else pa
    return (F, -x * cell_as, z * cell_as, float(np.sqrt(lam[1]) * _FWHM_PER_SIGMA * cell_as),
            float(np.sqrt(max(lam[0], 0.)) * _FWHM_PER_SIGMA * cell_as), float(pa))


def uvfit_theta_from_imfit(fit, cell_rad):
    """One component's (F, x, z, sxx, sxz, szz) from one dict of `gauss_results` made with
    `shape` (it then carries 'east_as' / 'north_as'): the integrated flux 'I', the centre, and
    the DECONVOLVED size -- or a point where the dict says 'point_source'.  `cell_rad`: the cell
    the uv fit works in (the scales it gets come from the same cell)."""
    if "east_as" not in fit or "north_as" not in fit:
        raise ValueError("uvfit_theta_from_imfit: the fit carries no sky offsets (gauss_results "
                         "needs `shape`)")
    dec = fit.get("deconvolved")
    if dec is None:
        return uvfit_theta(fit["I"]["val"], fit["east_as"], fit["north_as"], 0., 0., 0., cell_rad)
    return uvfit_theta(fit["I"]["val"], fit["east_as"], fit["north_as"], dec["maj_as"],
                       dec["min_as"], dec["pa_deg"], cell_rad)


def uvfit_start(vis, su, sv, u, v, weights=None):
    """A one-component start for `RTEngine.uvfit` -> tensor [M, 6] beside `vis`, in plain torch
    on the device, nothing going to the host.  With rho^2 = (su u)^2 + (sv v)^2 [cycles per cell,
    squared] and the counting visibilities (finite V, u, v, weight; weight > 0):
      * F: the zero-spacing value of the straight line (unweighted least squares) through
        (rho^2, ln |V|) of the n = max(1, K // 10) points of smallest rho that count and have
        |V| > 0 (the shortest baselines; their geometric-mean amplitude when they share one rho);
      * the centre is the phase centre, x = z = 0;
      * a circular size from the amplitude's fall-off, |V| = F exp(-2 pi^2 s rho^2): the
        least-squares slope through the origin of ln(F / |V|) against rho^2 over the counting
        visibilities with 0 < |V| < F, s = sum rho^2 ln(F / |V|) / (2 pi^2 sum rho^4), 0 when
        there is none; sxx = szz = s, sxz = 0.
    `vis`: complex128 [M, K] or float64 [M, K, 2]; `su`, `sv` [M]; `u`, `v` [K] device tensors;
    `weights`: None, [K] or [M, K].  A map without a counting visibility gets a NaN flux, which
    `uvfit` reports as status 3.  The sums are torch reductions: their order, and with it the last
    bits of the start, may follow the shape of the stack.  A two-component start is the caller's."""
    import torch
    V = vis if vis.dtype == torch.complex128 else torch.view_as_complex(vis.contiguous())
    M, K = int(V.shape[0]), int(V.shape[1])
    dev = V.device
    col = lambda s: torch.from_numpy(np.ascontiguousarray(s, dtype=np.float64).reshape(-1)) \
        .to(dev)[:, None]
    a, b = col(su) * u.reshape(1, K), col(sv) * v.reshape(1, K)
    rho2 = a * a + b * b
    ok = torch.isfinite(V.real) & torch.isfinite(V.imag) & torch.isfinite(rho2)
    if weights is not None:
        w = weights.reshape(-1, K)
        ok = ok & torch.isfinite(w) & (w > 0)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    amp = torch.where(ok, V.abs(), zero)
    key = torch.where(ok, rho2, torch.full_like(rho2, float("inf")))
    idx = key.topk(max(1, K // 10), dim=1, largest=False).indices
    x, amp_n = rho2.gather(1, idx), amp.gather(1, idx)
    sel = ok.gather(1, idx) & (amp_n > 0)
    near = sel.to(torch.float64)
    n_near = near.sum(dim=1)
    y = torch.where(sel, torch.log(torch.where(sel, amp_n, 1. + zero)), zero)
    x = torch.where(sel, x, zero)
    mx, my = x.sum(dim=1) / n_near, y.sum(dim=1) / n_near                  # (0 / 0 = NaN: no data)
    dx = (x - mx[:, None]) * near
    sxx = (dx * dx).sum(dim=1)
    slope = torch.where(sxx > 0, (dx * y).sum(dim=1) / torch.where(sxx > 0, sxx, 1. + sxx), zero)
    flux = torch.exp(my - slope * mx)
    live = ok & (amp > 0) & (amp < flux[:, None])
    y = torch.where(live, torch.log(flux[:, None] / torch.where(live, amp, flux[:, None])), zero)
    r2 = torch.where(live, rho2, zero)
    den = (r2 * r2).sum(dim=1)
    s = torch.where(den > 0, (r2 * y).sum(dim=1) / (2. * np.pi ** 2 * torch.where(den > 0, den, 1. + den)),
                    zero)
    z = torch.zeros_like(flux)
    return torch.stack([flux, z, z, s, z, s], dim=1).contiguous()


def uvfit_results(theta, cov, chi2, nvis, free, cell_rad, status=None, scale_errors=True):
    """What a uv-plane model fit reports, from the outputs of `RTEngine.uvfit` (host arrays; pure
    NumPy) -> one list of component dicts per map.  `free`: None (all free) or the P flags the fit
    ran with; `cell_rad`: the cell in radians.  Per component:
      * 'I' = {'val': F, 'unit': 'Jy'} and 'Ierr' = {'val', 'unit'}, as the reference stores them;
      * 'east_as', 'north_as' (`uvfit_theta`'s convention), 'maj_as', 'min_as', 'pa_deg' (FWHM,
        North through East), 'point_source' (Sigma = 0), 'theta' (the six raw parameters);
      * the 1-sigma errors 'Ierr', 'east_err_as', 'north_err_as', 'sigma_err' (of sxx, sxz, szz
        [cells^2]), 'maj_err_as', 'min_err_as', 'pa_err_deg' from C = (N_ff)^-1, N_ff the rows and
        columns of `cov` of the free parameters -- exact for weights 1 / sigma^2 -- the last three
        by first-order propagation through the eigen-decomposition of Sigma (None for a point or
        fixed sizes; 'pa_err_deg' None for a circle).  A fixed parameter has the error 0.  With
        `scale_errors` every error is multiplied by sqrt(reduced chi^2), as uvmodelfit does;
      * 'chi2', 'reduced_chi2' = chi^2 / (2 nvis - n_free) (NaN without a degree of freedom),
        'nvis', and 'status' where given.
    A map whose fit is not finite (status 3) gets NaN / None entries."""
    theta = np.asarray(theta, dtype=np.float64)
    theta = theta.reshape(-1, theta.shape[-1])
    M, P = theta.shape
    nc, T = P // 6, P * (P + 1) // 2
    if P != 6 * nc or not 1 <= nc <= UVFIT_MAX_COMP:
        raise ValueError("uvfit_results: `theta` must hold 6 values per component")
    cov = np.asarray(cov, dtype=np.float64).reshape(M, T)
    chi2, nvis = np.asarray(chi2, dtype=np.float64).reshape(M), np.asarray(nvis).reshape(M)
    fr = np.ones(P, dtype=bool) if free is None else (np.asarray(free).reshape(-1) != 0)
    if fr.size != P:
        raise ValueError("uvfit_results: `free` must hold %d flags" % P)
    n_free = int(fr.sum())
    cell_as = np.degrees(float(cell_rad)) * 3600.
    nan = float("nan")
    iu = np.triu_indices(P)
    out = []
    for m in range(M):
        dof = 2 * int(nvis[m]) - n_free
        red = float(chi2[m]) / dof if dof > 0 and np.isfinite(chi2[m]) else nan
        C = None
        if np.all(np.isfinite(cov[m])) and np.all(np.isfinite(theta[m])) and n_free > 0:
            N = np.zeros((P, P))
            N[iu] = cov[m]
            N = N + np.triu(N, 1).T
            try:
                Cf = np.linalg.inv(N[np.ix_(fr, fr)])
            except np.linalg.LinAlgError:
                Cf = None
            if Cf is not None and np.all(np.isfinite(Cf)) and np.all(np.diag(Cf) >= 0.):
                C = np.zeros((P, P))
                C[np.ix_(fr, fr)] = Cf
                if scale_errors:
                    C = C * red if np.isfinite(red) else None
        comps = []
        for c in range(nc):
            th = theta[m, 6 * c:6 * c + 6]
            d = {"I": {"val": nan, "unit": "Jy"}, "Ierr": {"val": None, "unit": "Jy"},
                 "east_as": nan, "north_as": nan, "maj_as": nan, "min_as": nan, "pa_deg": nan,
                 "point_source": False, "theta": th.copy(), "east_err_as": None,
                 "north_err_as": None, "sigma_err": None, "maj_err_as": None, "min_err_as": None,
                 "pa_err_deg": None, "chi2": float(chi2[m]), "reduced_chi2": red,
                 "nvis": int(nvis[m])}
            if status is not None:
                d["status"] = int(np.asarray(status).reshape(M)[m])
            comps.append(d)
            if not np.all(np.isfinite(th)):
                continue
            try:
                F, east, north, mj, mn, pa = uvfit_components(th, cell_rad)
            except ValueError:
                continue
            d["I"]["val"], d["east_as"], d["north_as"] = F, east, north
            d["maj_as"], d["min_as"], d["pa_deg"] = mj, mn, pa
            d["point_source"] = bool(th[3] == 0. and th[4] == 0. and th[5] == 0.)
            if C is None:
                continue
            Cc = C[6 * c:6 * c + 6, 6 * c:6 * c + 6]
            sd = np.sqrt(np.maximum(np.diag(Cc), 0.))
            d["Ierr"]["val"] = float(sd[0])
            d["east_err_as"], d["north_err_as"] = float(sd[1] * cell_as), float(sd[2] * cell_as)
            d["sigma_err"] = (float(sd[3]), float(sd[4]), float(sd[5]))
            if d["point_source"] or not fr[6 * c + 3:6 * c + 6].any():
                continue
            lam, vec = np.linalg.eigh(np.array([[th[3], th[4]], [th[4], th[5]]]))
            Cs = Cc[3:, 3:]
            k = _FWHM_PER_SIGMA * cell_as
            for name, l, e in (("maj_err_as", lam[1], vec[:, 1]), ("min_err_as", lam[0], vec[:, 0])):
                if l > 0.:
                    g = np.array([e[0] * e[0], 2. * e[0] * e[1], e[1] * e[1]])
                    d[name] = float(k / (2. * np.sqrt(l)) * np.sqrt(max(g @ Cs @ g, 0.)))
            if lam[1] > lam[0]:
                e, f = vec[:, 1], vec[:, 0]
                g = np.array([f[0] * e[0], f[0] * e[1] + f[1] * e[0], f[1] * e[1]]) / (lam[1] - lam[0])
                d["pa_err_deg"] = float(np.degrees(np.sqrt(max(g @ Cs @ g, 0.))))
        out.append(comps)
    return out


# -- K25: robust statistics and the automatic clean mask ----------------------------------------------
MAD_TO_SIGMA = 1.4826            # sigma of a normal distribution = 1.4826 x its MAD
# tclean's usemask = 'auto-multithresh' defaults, where the step exists here; `nsigma` is the stop of
# a minor run at nsigma x the update's robust sigma (0: off)
AUTOMASK_DEFAULTS = dict(sidelobe_threshold=3.0, noise_threshold=5.0, low_noise_threshold=1.5,
                         min_beam_frac=0.3, grow_iterations=75, connectivity=1, nsigma=0.0)


def automask_options(automask):
    """None (or False) -> None; True -> the defaults (`AUTOMASK_DEFAULTS`); a dict -> the defaults
    with its entries, validated: an unknown key, a threshold, fraction or `nsigma` that is negative
    or not finite, a `grow_iterations` that is no integer (< 0 = until stable) or a `connectivity`
    other than 1 or 2 raise ValueError."""
    if automask is None or automask is False:
        return None
    if automask is True:
        automask = {}
    if not isinstance(automask, dict):
        raise ValueError("automask: None, True or a dict of options (%s)"
                         % ", ".join(sorted(AUTOMASK_DEFAULTS)))
    unknown = sorted(set(automask) - set(AUTOMASK_DEFAULTS))
    if unknown:
        raise ValueError("automask: unknown option(s) %s (known: %s)"
                         % (", ".join(map(str, unknown)), ", ".join(sorted(AUTOMASK_DEFAULTS))))
    out = dict(AUTOMASK_DEFAULTS)
    out.update(automask)
    for k in ("sidelobe_threshold", "noise_threshold", "low_noise_threshold", "min_beam_frac", "nsigma"):
        v = out[k]
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or \
                not np.isfinite(v) or v < 0:
            raise ValueError("automask: `%s` must be a finite number >= 0" % k)
        out[k] = float(v)
    g = out["grow_iterations"]
    if isinstance(g, bool) or not isinstance(g, (int, np.integer)):
        raise ValueError("automask: `grow_iterations` must be an integer (< 0: until stable)")
    out["grow_iterations"] = int(g)
    if isinstance(out["connectivity"], bool) or out["connectivity"] not in (1, 2):
        raise ValueError("automask: `connectivity` must be 1 (four neighbours) or 2 (eight)")
    out["connectivity"] = int(out["connectivity"])
    return out


def image_stats_results(stats):
    """`RTEngine.image_stats`' [M, 8] (tensor or array) -> one dict per map, named as imstat names
    them: `npts`, `min`, `max`, `median` (the LOWER median), `medabsdevmed`, `sigma_robust`
    (1.4826 x MAD), `sum`, `mean`, `rms` (sqrt(sumsq / npts)) and `sigma` (the standard deviation
    from sum and sumsq, npts - 1 in the denominator; 0 for one point).  No point: NaN but for npts,
    sum = 0."""
    st = stats.cpu().numpy() if hasattr(stats, "cpu") else np.asarray(stats, dtype=np.float64)
    out = []
    for count, _, lo, hi, med, mad, s, q in st.reshape(-1, 8):
        n = int(count)
        d = dict(npts=n, min=float(lo), max=float(hi), median=float(med), medabsdevmed=float(mad),
                 sigma_robust=MAD_TO_SIGMA * float(mad), sum=float(s), mean=np.nan, rms=np.nan,
                 sigma=np.nan)
        if n:
            d["mean"] = float(s) / n
            d["rms"] = float(np.sqrt(float(q) / n))
            d["sigma"] = float(np.sqrt(max(0., (float(q) - float(s) * float(s) / n) / (n - 1)))) \
                if n > 1 else 0.
        out.append(d)
    return out


def automask_step(eng, R, prev, user_mask, sidelobe, abc, opts, shape=None):
    """One update of the automatic clean masks of a stack of residuals -> (masks uint8 device tensor
    [M, ni nj], info: one dict per map).  `R`: float64 device tensor [M, ni, nj], or [M, ni nj] with
    `shape` = (ni, nj); `prev`: the masks so far, [M, ni nj] on the device (None: empty);
    `user_mask`: None or a device tensor [ni nj] that bounds the automatic mask; `sidelobe` [M]:
    the beams' sidelobe levels; `abc` [M][3]: the clean beams' quadratic forms; `opts`: what
    `automask_options` returns.  Four engine calls (`image_stats` twice, `label_regions`,
    `mask_grow`) and torch comparisons; the formulas are evaluated in float64 on the host, in this
    order, from the numbers the device returned:
      noise   median and MAD of the finite pixels OUTSIDE prev[m] (none: of all finite pixels);
              sigma = 1.4826 * mad;  peak = the largest finite R[m], signed
      t_noise = median + noise_threshold * sigma;  t_side = sidelobe_threshold * sidelobe[m] * peak
      T = max(t_side, t_noise);  T_low = min(T, median + low_noise_threshold * sigma)
      seed = finite & (R > T) & user_mask;  constraint = finite & (R > T_low) & user_mask
      min_pixels = max(1, ceil(min_beam_frac * Omega_b)), Omega_b = pi / sqrt(A C - B^2) pixels;
              a region of the seed (`connectivity`) stays when its area >= min_pixels
      grown = `mask_grow`(kept, constraint, grow_iterations);  mask = prev | grown
    info[m]: `median`, `sigma`, `peak`, `T`, `T_low`, `n_regions`, `n_kept`, `n_seed`, `n_mask`."""
    import torch
    if shape is None:
        if R.dim() != 3:
            raise ValueError("automask_step: `R` must be [M, ni, nj], or [M, ni nj] with `shape`")
        shape = (int(R.shape[1]), int(R.shape[2]))
    ni, nj = int(shape[0]), int(shape[1])
    R = R.reshape(-1, ni * nj)
    M = int(R.shape[0])
    if prev is None:
        prev = torch.zeros(M, ni * nj, dtype=torch.uint8, device=R.device)
    prev = (prev.reshape(M, ni * nj) != 0)
    st_all = eng.image_stats(R, ni, nj).cpu().numpy()
    st_out = eng.image_stats(R, ni, nj, mask=prev.to(torch.uint8), inside=False).cpu().numpy()
    T, T_low, noise, min_pix = np.zeros(M), np.zeros(M), [], np.zeros(M, dtype=np.int64)
    for m in range(M):
        st = st_out[m] if st_out[m, 0] > 0 else st_all[m]
        median, sigma, peak = float(st[4]), MAD_TO_SIGMA * float(st[5]), float(st_all[m, 3])
        t_noise = median + opts["noise_threshold"] * sigma
        t_side = opts["sidelobe_threshold"] * float(sidelobe[m]) * peak
        T[m] = max(t_side, t_noise)
        T_low[m] = min(T[m], median + opts["low_noise_threshold"] * sigma)
        A, B, C = (float(v) for v in abc[m])
        omega = np.pi / np.sqrt(A * C - B * B)
        min_pix[m] = max(1, int(np.ceil(opts["min_beam_frac"] * omega)))
        noise.append((median, sigma, peak))
    ok = torch.isfinite(R)
    if user_mask is not None:
        ok = ok & (user_mask.reshape(1, ni * nj) != 0)
    dev = R.device
    seed = ok & (R > torch.from_numpy(T).to(dev)[:, None])
    con = ok & (R > torch.from_numpy(T_low).to(dev)[:, None])
    label, area, nreg = eng.label_regions(seed, ni, nj, opts["connectivity"])
    big = area >= torch.from_numpy(min_pix).to(device=dev, dtype=torch.int32)[:, None]
    kept = seed & big
    root = label == torch.arange(1, ni * nj + 1, dtype=torch.int32, device=dev)[None, :]
    grown = eng.mask_grow(kept, con, ni, nj, opts["grow_iterations"], opts["connectivity"])
    masks = (prev | (grown != 0)).to(torch.uint8)
    counts = torch.stack([nreg.to(torch.int64), (root & big).sum(dim=1), seed.sum(dim=1),
                          masks.sum(dim=1, dtype=torch.int64)], dim=1).cpu().numpy()
    info = [dict(median=noise[m][0], sigma=noise[m][1], peak=noise[m][2], T=float(T[m]),
                 T_low=float(T_low[m]), n_regions=int(counts[m, 0]), n_kept=int(counts[m, 1]),
                 n_seed=int(counts[m, 2]), n_mask=int(counts[m, 3])) for m in range(M)]
    return masks, info


# -- result types -----------------------------------------------------------------------------------
# what `JetModel.clean_image_ff` / `clean_image_rrl` return
class CleanResult(collections.namedtuple(
        "CleanResult", ["image", "residual", "model", "components", "beam", "peak_residual"])):
    """The six products of a CLEAN as a tuple, and `imfit`: None, or with the `imfit` keyword one
    dict per map (`engine.gauss_results`) -- an attribute beside the tuple, so that code which
    unpacks the six products keeps working.  `_replace` carries `imfit` over (and takes it as a
    keyword); `_make`, which builds from the six values alone, leaves it None.
    `major`, handled the same way: None, or with `major_cycles` >= 1 one dict per map -- `runs` (a
    list of dicts `start`, `n`, `peak`, `threshold`: where the run's components begin in the map's
    list, how many it kept, the masked peak it started from and the threshold it ran to),
    `sidelobe` and `vis_residual` (complex [K], or [F K] with `mfs`: V minus the list's
    visibilities, what the residual is the image of).
    `taylor`, handled the same way: None, or with `nterms` > 1 one dict per output map -- `tt`,
    `residual_tt`, `model_tt` (each (n_t, ni, nj): the restored Taylor images, the raw Taylor
    residual planes and the delta models), `alpha` (tt1 / tt0 where tt0 > `alpha_cut_jy`, NaN
    elsewhere), `beta` (tt2 / tt0 - alpha (alpha - 1) / 2; None below three terms),
    `alpha_cut_jy`, `reffreq_hz`, `hessian` and `hinv` (n_t, n_t).
    `automask`, handled the same way: None, or with the `automask` keyword one dict per map --
    `mask` (bool (ni, nj): the final automatic mask) and `runs` (one dict per update, what
    `automask_step` reports: `median`, `sigma`, `peak`, `T`, `T_low`, `n_regions`, `n_kept`,
    `n_seed`, `n_mask`; and `start`, the length of the map's component list at that update)."""

    def __new__(cls, *args, imfit=None, major=None, taylor=None, automask=None, **kw):
        self = super().__new__(cls, *args, **kw)
        self.imfit = imfit
        self.major = major
        self.taylor = taylor
        self.automask = automask
        return self

    imfit = None
    major = None
    taylor = None
    automask = None

    def _replace(self, **kw):
        imfit = kw.pop("imfit", self.imfit)
        major = kw.pop("major", self.major)
        taylor = kw.pop("taylor", self.taylor)
        automask = kw.pop("automask", self.automask)
        out = super()._replace(**kw)
        out.imfit = imfit
        out.major = major
        out.taylor = taylor
        out.automask = automask
        return out


# what `JetModel.uv_tracks` returns: device tensors u_m, v_m, w_m [n_t * n_bl] (visibility
# k = t n_bl + b), host arrays ha_h, day [n_t] and ant1, ant2 [n_bl], and the longest baseline
UVTracks = collections.namedtuple("UVTracks", ["u_m", "v_m", "w_m", "ha_h", "day", "ant1", "ant2",
                                               "max_baseline_m"])
# what `JetModel.observe_ff` / `observe_rrl` return
Observation = collections.namedtuple("Observation", ["tracks", "vis_clean", "vis", "sigma",
                                                     "image_rms", "clean"])


class Weighting(collections.namedtuple("Weighting", ["scheme", "robust", "weights"])):
    """An imaging-weight scheme as ONE value for the `weights` of `JetModel.dirty_image_ff`, whose
    parameter list is fixed: `scheme` None / "natural" / "uniform" / "briggs", `robust` (Briggs
    only) and the data `weights` [K] the scheme starts from (None = all ones).  The other imaging
    methods take `weighting=` and `robust=` beside their `weights`."""
    __slots__ = ()

    def __new__(cls, scheme="briggs", robust=0.5, weights=None):
        return super().__new__(cls, scheme, robust, weights)


def _split_weights(weights):
    """The `weights` of `dirty_image_ff` -> the data weights, the scheme and its robustness: a
    `Weighting` carries all three, anything else is data weights, naturally weighted."""
    weighting, robust = None, 0.5
    if isinstance(weights, Weighting):
        weights, weighting, robust = weights.weights, weights.scheme, weights.robust
    _weighting_mode(weighting)
    return weights, weighting, robust


def _weighting_mode(weighting):
    """None for natural weights (None or "natural": no kernel, the path as it was), else the mode
    of `RTEngine.uv_weights`."""
    if weighting is None or weighting == "natural":
        return None
    if weighting not in ("uniform", "briggs"):
        raise ValueError("imaging weights: `weighting` must be None, 'natural', 'uniform' or "
                         "'briggs'")
    return weighting


def _col(eng, s):
    import torch
    return torch.from_numpy(np.ascontiguousarray(s, dtype=np.float64)).to(eng.device)[:, None]


def _mfs_points(eng, u_d, v_d, su, sv, w_d):
    """The F K points of F channels as ONE visibility set, channel by channel: the baselines in
    cycles per cell (to be used with the scales [1.0]) and the data weights repeated."""
    return ((_col(eng, su) * u_d[None, :]).reshape(-1), (_col(eng, sv) * v_d[None, :]).reshape(-1),
            w_d.repeat(len(su)) if w_d is not None else None)


def _imaging_weights(eng, u_d, v_d, su, sv, w_d, ni, nj, mode, robust, mfs):
    """The imaging weights of one chunk of channels from ONE `RTEngine.uv_weights` call on the
    ni x nj image grid -> device tensor [F, K], a density per channel; `mfs`: [1, F K], one
    density over all F K points in cycles per cell (scale 1), as `_dirty_images` images them."""
    if mfs:
        u_d, v_d, w_d = _mfs_points(eng, u_d, v_d, su, sv, w_d)
        su = sv = [1.0]
    return eng.uv_weights(u_d, v_d, su, sv, ni, nj, w=w_d, mode=mode, robust=robust)


# -- multi-scale CLEAN: the scale kernels and their biases (host) ------------------------------------
def scale_kernel(s):
    """The kernel of the scale `s` [image pixels, as tclean takes `scales`] -> float64 array
    (2 h + 1, 2 h + 1), h = ceil(s) - 1, of unit sum: the truncated paraboloid 1 - (r / s)^2 for
    r < s, 0 beyond; s <= 0 is the delta [[1.0]].  (CASA multiplies the paraboloid by a
    prolate-spheroidal taper; this kernel does not: DESIGN section 7.)"""
    s = float(s)
    if not np.isfinite(s):
        raise ValueError("scale_kernel: the scale must be finite")
    if s <= 0.:
        return np.ones((1, 1))
    h = int(np.ceil(s)) - 1
    d = np.arange(-h, h + 1, dtype=np.float64)
    r2 = d[:, None] ** 2 + d[None, :] ** 2
    k = np.where(r2 < s * s, 1. - r2 / (s * s), 0.)
    return np.ascontiguousarray(k / k.sum())


def scale_biases(scales):
    """The bias of each scale of `scales` [pixels], 1 - 0.6 s / s_max (Cornwell 2008, eq. 21:
    large scales are held back) -> float64 array; 1 for a single scale (or no scale above 0)."""
    sc = np.atleast_1d(np.asarray(scales, dtype=np.float64))
    if sc.size == 0 or not np.all(np.isfinite(sc)):
        raise ValueError("scale_biases: `scales` must be a non-empty list of finite sizes")
    sc = np.maximum(sc, 0.)
    smax = sc.max()
    if sc.size == 1 or smax == 0.:
        return np.ones(sc.size)
    return 1. - 0.6 * sc / smax


def _scale_planes(scales, scale_bias):
    """The `scales=` / `scale_bias=` keywords of a multi-scale CLEAN -> (the scale of every plane
    [pixels], the bias of every plane, h_max): plane 0 is ALWAYS the delta scale -- bias 1 if 0 is
    among `scales`, else 0 (the raw residual is updated but never picked) --, the non-zero scales
    follow, ascending and without repeats.  `scale_bias`: None (`scale_biases` of the planes) or
    one bias per plane in that order."""
    sc = np.atleast_1d(np.asarray(scales, dtype=np.float64)).reshape(-1)
    if sc.size == 0 or not np.all(np.isfinite(sc)):
        raise ValueError("clean: `scales` must be a non-empty list of finite sizes in pixels")
    planes = np.concatenate([[0.], np.unique(sc[sc > 0.])])
    if scale_bias is None:
        bias = scale_biases(planes)
    else:
        bias = np.asarray(scale_bias, dtype=np.float64).reshape(-1).copy()
        if bias.size != planes.size or not np.all(np.isfinite(bias) & (bias >= 0.)):
            raise ValueError("clean: `scale_bias` must be one finite bias >= 0 per plane (%d: the "
                             "delta scale, then the other scales ascending)" % planes.size)
    if not np.any(sc <= 0.):
        bias[0] = 0.
    if not np.any(bias > 0.):
        raise ValueError("clean: every scale has bias 0")
    return planes, bias, int(np.ceil(planes.max())) - 1 if planes.max() > 0. else 0


def _major_options(major_cycles, cyclefactor, cycleniter, min_psf_fraction, max_psf_fraction):
    """The major-cycle keywords of a CLEAN, checked -> None (`major_cycles` = 0: minor cycles
    only) or a dict of them."""
    try:
        n, cf = int(major_cycles), float(cyclefactor)
        cn = None if cycleniter is None else int(cycleniter)
        lo, hi = float(min_psf_fraction), float(max_psf_fraction)
    except (TypeError, ValueError):
        raise ValueError("clean: major_cycles, cyclefactor, cycleniter, min_psf_fraction and "
                         "max_psf_fraction must be numbers") from None
    if n != major_cycles or n < 0:
        raise ValueError("clean: `major_cycles` must be an integer >= 0")
    if not (np.isfinite(cf) and cf > 0.):
        raise ValueError("clean: `cyclefactor` must be finite and > 0")
    if cn is not None and (cn != cycleniter or cn < 1):
        raise ValueError("clean: `cycleniter` must be None or an integer >= 1")
    if not 0. <= lo <= hi <= 1.:
        raise ValueError("clean: 0 <= min_psf_fraction <= max_psf_fraction <= 1")
    if n == 0:
        return None
    return dict(major_cycles=n, cyclefactor=cf, cycleniter=cn, min_psf_fraction=lo,
                max_psf_fraction=hi)


# ---- multi-term MFS (K19) ----------------------------------------------------------------------------
MTMFS_MAX_NT = 4             # RJP_MTMFS_MAX_NT
# The largest condition number of the Taylor Hessian that `taylor_hessian_inverse` accepts.  The
# principal solution a = Hinv R loses a factor cond(H) of the planes' accuracy: at 1e10 the
# coefficients of a noise-free model still hold about six digits in double precision, and any
# thermal noise is amplified by the same factor -- beyond it the band is too narrow for `nterms`.
TAYLOR_COND_MAX = 1e10


def taylor_weights(freqs, reffreq_hz, n):
    """The Taylor weights of the channels `freqs` [Hz] about `reffreq_hz` -> float64 array [n, F]:
    row q is w_f^q, w_f = (nu_f - nu_0) / nu_0 (one subtraction, one division).  Row 0 is exactly
    1, row q is row q - 1 times w (one rounding each)."""
    f = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    nu0, n = float(reffreq_hz), int(n)
    if n < 1 or f.ndim != 1 or not (np.isfinite(nu0) and nu0 > 0.) or not np.all(np.isfinite(f)):
        raise ValueError("taylor_weights: n >= 1, finite `freqs` and a finite `reffreq_hz` > 0")
    w = (f - nu0) / nu0
    out = np.ones((n, f.size))
    for q in range(1, n):
        out[q] = out[q - 1] * w
    return out


def taylor_hessian_inverse(centres):
    """The Hessian of a multi-term MFS minor cycle and its inverse from the centre values of the
    spectral beams, `centres` [2 n_t - 1] = B_0 .. B_{2 n_t - 2} at the centre pixel -> (H, Hinv),
    float64 [n_t, n_t]: H[t][q] = centres[t + q] (a Hankel matrix, symmetric), Hinv its inverse,
    symmetrised.  ValueError when H is not positive definite (a band of fewer distinct frequencies
    than terms makes it singular) or its 2-norm condition number exceeds `TAYLOR_COND_MAX`: the
    band is too narrow for that many terms."""
    c = np.asarray(centres, dtype=np.float64).reshape(-1)
    if c.size < 1 or c.size % 2 == 0 or not np.all(np.isfinite(c)):
        raise ValueError("taylor_hessian_inverse: `centres` must be 2 n_t - 1 finite numbers")
    n = (c.size + 1) // 2
    H = np.array([[c[t + q] for q in range(n)] for t in range(n)])
    try:
        np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        raise ValueError("mtmfs: the Taylor Hessian is not positive definite (fewer distinct "
                         "frequencies than terms, or beams that are not those of one band)") from None
    cond = float(np.linalg.cond(H))
    if not cond <= TAYLOR_COND_MAX:
        raise ValueError("mtmfs: the Taylor Hessian's condition number %.3g exceeds %.3g: the band "
                         "is too narrow for nterms = %d" % (cond, TAYLOR_COND_MAX, n))
    Hinv = np.linalg.inv(H)
    return H, 0.5 * (Hinv + Hinv.T)


def _taylor_options(nterms, reffreq_hz, alpha_cut_jy, freqs, mfs, scales, major):
    """`nterms`, `reffreq_hz`, `alpha_cut_jy` of `clean_image_*` -> None for one term, else a dict
    (n_t, reffreq_hz, alpha_cut_jy, tw: `taylor_weights` with 2 n_t - 1 rows)."""
    try:
        n = int(nterms)
    except (TypeError, ValueError):
        raise ValueError("clean: `nterms` must be an integer from 1 to %d" % MTMFS_MAX_NT) from None
    if n != nterms or not 1 <= n <= MTMFS_MAX_NT:
        raise ValueError("clean: `nterms` must be an integer from 1 to %d" % MTMFS_MAX_NT)
    if n == 1:
        return None
    if not mfs:
        raise ValueError("clean: `nterms` > 1 needs `mfs=True` (the Taylor terms are those of one "
                         "image of the whole band)")
    if scales is not None:
        raise ValueError("clean: `nterms` > 1 with `scales` (multi-scale multi-term) is not built")
    if major is not None:
        raise ValueError("clean: `nterms` > 1 with `major_cycles` >= 1 is not built")
    f = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    if np.unique(f).size < n:
        raise ValueError("clean: `nterms` = %d needs at least that many distinct frequencies" % n)
    nu0 = 0.5 * (f.min() + f.max()) if reffreq_hz is None else float(reffreq_hz)
    if not (np.isfinite(nu0) and nu0 > 0.):
        raise ValueError("clean: `reffreq_hz` must be None or a finite frequency > 0")
    cut = None if alpha_cut_jy is None else float(alpha_cut_jy)
    if cut is not None and not np.isfinite(cut):
        raise ValueError("clean: `alpha_cut_jy` must be None or a finite number")
    return dict(n_t=n, reffreq_hz=nu0, alpha_cut_jy=cut, tw=taylor_weights(f, nu0, 2 * n - 1))


class Imager:
    """Visibilities, images, synthetic observations and Gaussian fits of the flux maps of an
    nx x nz grid of `csize_au` cells at `dist_pc`, through `engine` (an `RTEngine`).  Maps and
    visibilities are device tensors; `stack_bytes`: the most one engine call of a chunk loop takes."""
    BEAM_PATCH = 33          # side of the central patch of the dirty beam that `fit_beam` sees

    def __init__(self, engine, nx, nz, csize_au, dist_pc, stack_bytes):
        self.engine, self.nx, self.nz = engine, nx, nz
        self.csize_au, self.dist_pc, self.stack_bytes = csize_au, dist_pc, int(stack_bytes)

    def model_vis(self, maps, freqs, u, v):
        """`RTEngine.vis` of the flux maps [F, nx * nz] at (`u`, `v`) [m] -> complex device [F, K]."""
        su, sv = vis_scales(freqs, self.csize_au, self.dist_pc)
        return self.engine.vis(maps, self.nx, self.nz, su, sv, u, v)

    def _unit_vis(self, F, K):
        """Visibilities that are all 1 (what a dirty beam is the image of) -> complex [F, K]."""
        import torch
        return torch.ones(F, K, dtype=torch.complex128, device=self.engine.device)

    # ------------------------------------------------------------------ dirty images ----
    def _image_grid(self, shape, cell_as):
        """(ni, nj, cell [rad]) of an imaging grid: the model's own by default."""
        ni, nj = (self.nx, self.nz) if shape is None else (int(shape[0]), int(shape[1]))
        if ni < 1 or nj < 1:
            raise ValueError("dirty image: `shape` must be two positive sizes")
        if cell_as is None:
            cell = np.arctan((self.csize_au * con.au) / (self.dist_pc * con.parsec))
        else:
            cell = np.radians(float(cell_as) / 3600.)
            if not (np.isfinite(cell) and cell > 0.):
                raise ValueError("dirty image: `cell_as` must be a positive number of arcseconds")
        return ni, nj, float(cell)

    def _dirty_images(self, V, u_d, v_d, freqs, weights, shape, cell_as, mfs, device=False,
                      weighting=None, robust=0.5, iw=None):
        """Dirty images [Jy / beam] of the visibilities `V` (complex device tensor [F, K]) at the
        baselines (`u_d`, `v_d`) [m] -> host array (F, ni, nj), or (1, ni, nj) with `mfs`;
        `device=True`: the same numbers as a device tensor [F or 1, ni * nj] (for `_clean_images`).
        `RTEngine.vis_adjoint` on chunks of channels whose images stay under `stack_bytes`
        (K10's `_vis_chunk` rule on the imaging grid), divided by the sum of the weights of the
        baselines that are not flagged; nothing but the images leaves the device, chunk by chunk.
        `weighting` "uniform" / "briggs" (with `robust`): the imaging weights of every chunk come
        from ONE `RTEngine.uv_weights` call on this image's grid, a density per channel (one over
        all F K points with `mfs`), are multiplied into V on the device and the image is divided
        by the channel's own sum of them; the chunks then also keep the [F, K] weights under
        `stack_bytes`.  `iw`: those weights already made ([F, K], or [1, F K] with `mfs`: what
        `_clean_images` shares between the image and the larger beam grid)."""
        import torch
        eng = self.engine
        ni, nj, cell = self._image_grid(shape, cell_as)
        su, sv = image_scales(freqs, cell)
        F, K = int(V.shape[0]), int(V.shape[1])
        w_d = eng._device_f64(weights) if weights is not None else None
        if w_d is not None and w_d.numel() != K:
            raise ValueError("dirty image: `weights` must have one entry per baseline (%d)" % K)
        mode = _weighting_mode(weighting)
        weighted = mode is not None or iw is not None
        # what a chunk is.  Natural weights are the engine's `w`, and every image is divided by their
        # sum over the unflagged baselines; imaging weights go into V, each image's own sum divides.
        step = self.stack_bytes // (ni * nj * 8)
        if weighted:
            step = min(step, self.stack_bytes // (K * 8))
        else:
            good = torch.isfinite(u_d) & torch.isfinite(v_d)
            if w_d is not None:
                good = good & torch.isfinite(w_d)
            wsum = (torch.where(good, w_d, torch.zeros_like(w_d)).sum() if w_d is not None
                    else good.sum().to(torch.float64))
        if mfs:
            # one chunk of one image: one visibility set of F K points, baselines in cycles per
            # cell, scale 1
            V, step = V.reshape(1, F * K), 1
            u_d, v_d, w_d = _mfs_points(eng, u_d, v_d, su, sv, w_d)
            su = sv = [1.0]
            if not weighted:
                wsum = wsum * F
        n, step = int(V.shape[0]), max(1, step)
        out = [] if device else np.zeros((n, ni, nj))
        for f0 in range(0, n, step):
            sl = slice(f0, f0 + step)
            vis = V[sl]
            if weighted:
                wc = iw[sl] if iw is not None else _imaging_weights(
                    eng, u_d, v_d, su[sl], sv[sl], w_d, ni, nj, mode, robust, False)
                vis = vis * wc
                # (a full reduction with `mfs`, row sums without: two reductions, kept apart)
                wsum = wc.sum() if mfs else wc.sum(dim=1)[:, None]
                del wc
            img = eng.vis_adjoint(vis.contiguous(), ni, nj, su[sl], sv[sl], u_d, v_d,
                                  None if weighted else w_d) / wsum
            del vis
            if device:
                out.append(img)
            else:
                out[sl] = img.cpu().numpy().reshape(-1, ni, nj)
            del img
        return torch.cat(out, dim=0) if device else out

    def imaging_weights(self, u_m, v_m, freq, weights=None, shape=None, cell_as=None,
                        weighting="briggs", robust=0.5, mfs=False):
        """See `JetModel.imaging_weights`."""
        import torch
        eng = self.engine
        freqs = np.atleast_1d(np.asarray(freq, dtype=np.float64))
        mode = _weighting_mode(weighting)     # (refuses an unknown scheme before any work)
        ni, nj, cell = self._image_grid(shape, cell_as)
        su, sv = image_scales(freqs, cell)
        u_d, v_d = eng._device_f64(u_m), eng._device_f64(v_m)
        F, K = len(freqs), int(u_d.numel())
        w_d = eng._device_f64(weights) if weights is not None else None
        if v_d.numel() != K or (w_d is not None and w_d.numel() != K):
            raise ValueError("imaging weights: u, v and weights must have one entry per baseline")
        w1 = w_d if w_d is not None else torch.ones(K, dtype=torch.float64, device=eng.device)
        names = ("sum_w", "sum_w2", "f2", "counted", "out_of_range", "shift")
        if mode is None:
            ok = torch.isfinite(u_d) & torch.isfinite(v_d) & torch.isfinite(w1) & (w1 >= 0)
            row = torch.where(ok, w1, torch.zeros_like(w1)).cpu().numpy()
            n = 1 if mfs else F
            st = {k: np.zeros(n) for k in names}
            st["sum_w"][:] = row.sum() * (F if mfs else 1)
            st["counted"][:] = np.count_nonzero(ok.cpu().numpy()) * (F if mfs else 1)
            st["sum_wout"], st["noise_factor"] = st["sum_w"].copy(), np.ones(n)
            return np.tile(row, (F, 1)), st
        out, stats, extra = np.zeros((F, K)), [], []
        step = F if mfs else max(1, self.stack_bytes // (K * 8))
        for f0 in range(0, F, step):
            sl = slice(f0, f0 + step)
            iw = _imaging_weights(eng, u_d, v_d, su[sl], sv[sl], w_d, ni, nj, mode, robust, mfs)
            wd = w1.repeat(F)[None, :] if mfs else w1[None, :]
            live = (iw > 0) & (wd > 0)
            ratio = torch.where(live, iw * iw / torch.where(live, wd, torch.ones_like(wd)),
                                torch.zeros_like(iw))
            extra.append(torch.stack([iw.sum(dim=1), ratio.sum(dim=1),
                                      torch.where(live, wd.expand_as(iw), torch.zeros_like(iw))
                                      .sum(dim=1)], dim=1).cpu().numpy())
            stats.append(eng.last_uv_weight_stats.cpu().numpy())
            out[sl] = iw.cpu().numpy().reshape(-1, K)
            del iw
        stats, extra = np.concatenate(stats, axis=0), np.concatenate(extra, axis=0)
        st = {k: stats[:, i].copy() for i, k in enumerate(names)}
        st["sum_wout"] = extra[:, 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            st["noise_factor"] = np.sqrt(extra[:, 1] * extra[:, 2]) / extra[:, 0]
        return out, st

    # ------------------------------------------------------------------ CLEAN ----
    def _clean_mask(self, mask, ni, nj):
        """None, a box (i0, i1, j0, j1) of inclusive pixel corners (as the reference hands
        tclean a box) or a boolean array (ni, nj) -> None or a bool array (ni, nj)."""
        if mask is None:
            return None
        m = np.asarray(mask)
        if m.ndim == 1 and m.size == 4:
            i0, i1, j0, j1 = (int(x) for x in m)
            if not (0 <= i0 <= i1 < ni and 0 <= j0 <= j1 < nj):
                raise ValueError("clean: the box (i0, i1, j0, j1) must lie inside the image")
            out = np.zeros((ni, nj), dtype=bool)
            out[i0:i1 + 1, j0:j1 + 1] = True
            return out
        if m.shape != (ni, nj):
            raise ValueError("clean: `mask` must be None, a box (i0, i1, j0, j1) or an array of "
                             "the image's shape (%d, %d)" % (ni, nj))
        return m != 0

    def _clean_images(self, V, u_d, v_d, freqs, weights, shape, cell_as, mfs, niter, gain,
                      threshold_jy, mask, beam, psf_shape, imfit=None, weighting=None, robust=0.5,
                      automask=None, scales=None, scale_bias=None, nterms=1, reffreq_hz=None,
                      alpha_cut_jy=None,
                      major_cycles=0, cyclefactor=1.5, cycleniter=None,
                      min_psf_fraction=0.05, max_psf_fraction=0.8):
        """Hogbom CLEAN of the dirty images of `V` (see `JetModel.clean_image_ff`), in chunks of
        channels whose dirty images AND beams stay under `stack_bytes`.  Per chunk, on the device:
        `_dirty_images` of V and of unit visibilities (the beams, on the `psf_shape` grid),
        `RTEngine.clean`, `RTEngine.restore`; only the central patch of each beam goes to the
        host before the end (for `fit_beam`).  With `weighting` "uniform" / "briggs" the chunk's
        imaging weights are computed ONCE, on the image's grid (never the larger beam grid), and
        image and beam share them; the chunks then also keep the [F, K] weights under
        `stack_bytes`.
        `scales` (pixels, with `scale_bias`: `_scale_planes`): multi-scale CLEAN instead, per
        chunk `_msclean_chunk` -- `RTEngine.convolve2d`, `RTEngine.msclean` -- and the chunks
        count the n_s planes and the n_s (n_s + 1) / 2 cross beams; the threshold is then one of
        the SCORE, bias x component flux.
        `major_cycles` >= 1 (with `cyclefactor`, `cycleniter`, `min_psf_fraction`,
        `max_psf_fraction`): per chunk `_major_chunk` -- minor runs alternating with residuals
        recomputed from the visibilities -- and `CleanResult.major`; 0 is the path as it was.
        `nterms` > 1 (with `mfs`; `reffreq_hz`, `alpha_cut_jy`): multi-term MFS CLEAN, the one
        chunk through `_mtmfs_chunk` -- n_t Taylor dirty images and 2 n_t - 1 spectral beams with
        the chunk's weights, `RTEngine.mtmfs` -- and `CleanResult.taylor`; 1 is the path as it
        was.
        `automask` (`automask_options`; not with `scales` or `nterms` > 1): every map is cleaned
        under a mask of its own that `automask_step` makes from its residual, inside `mask` -- once
        from the dirty image without major cycles, at the top of every run with them (`_major_chunk`
        with `am`) -- one `RTEngine.clean` call per map (`_clean_per_map`), and
        `CleanResult.automask`; None makes no new call: the path as it was."""
        import torch
        eng = self.engine
        mj = _major_options(major_cycles, cyclefactor, cycleniter, min_psf_fraction,
                            max_psf_fraction)
        ty = _taylor_options(nterms, reffreq_hz, alpha_cut_jy, freqs, mfs, scales, mj)
        am = automask_options(automask)
        if am is not None and (scales is not None or ty is not None):
            raise ValueError("clean: `automask` goes with Hogbom CLEAN only, not with `scales` or "
                             "`nterms` > 1")
        ni, nj, cell = self._image_grid(shape, cell_as)
        pi_, pj = (2 * ni - 1, 2 * nj - 1) if psf_shape is None else (int(psf_shape[0]),
                                                                      int(psf_shape[1]))
        if pi_ < 1 or pj < 1 or pi_ % 2 == 0 or pj % 2 == 0:
            raise ValueError("clean: `psf_shape` must be two odd positive sizes")
        niter = int(niter)
        # (one threshold, or one per image: what `_observe` derives from each image's own rms)
        thr = np.asarray(threshold_jy, dtype=np.float64).reshape(-1)
        if niter < 1 or not (0. < float(gain) <= 1.) or not np.all(thr >= 0.) or \
                thr.size not in (1, 1 if mfs else int(V.shape[0])):
            raise ValueError("clean: niter >= 1, 0 < gain <= 1 and threshold_jy >= 0")
        mk = self._clean_mask(mask, ni, nj)
        F, K = int(V.shape[0]), int(V.shape[1])
        n_out = 1 if mfs else F
        ones = self._unit_vis(F, K)
        fit_opts = self._imfit_options(imfit, mask, ni, nj)
        res = CleanResult(image=np.zeros((n_out, ni, nj)), residual=np.zeros((n_out, ni, nj)),
                          model=np.zeros((n_out, ni, nj)), components=[], beam=[],
                          peak_residual=np.zeros(n_out), imfit=None if fit_opts is None else [],
                          major=None if mj is None else [], taylor=None if ty is None else [],
                          automask=None if am is None else [])
        step = F if mfs else max(1, self.stack_bytes // ((ni * nj * 3 + pi_ * pj) * 8))
        ms = None
        if scales is not None:
            planes, bias, hmax = _scale_planes(scales, scale_bias)
            n_s = len(planes)
            mk = np.ones((ni, nj), dtype=bool) if mk is None else mk.copy()
            if hmax > 0:
                # a component nearer than h_max to the border would lose part of its scale kernel
                mk[:hmax], mk[ni - hmax:], mk[:, :hmax], mk[:, nj - hmax:] = False, False, False, False
            if not mk.any():
                raise ValueError("clean: no pixel of the mask lies at least %d pixels (the largest "
                                 "scale's half width) from the border" % hmax)
            ms = dict(planes=planes, bias=bias, hmax=hmax, mask=torch.from_numpy(mk).to(eng.device),
                      ker=[torch.from_numpy(scale_kernel(s)).to(eng.device) for s in planes])
            if not mfs:
                step = max(1, self.stack_bytes // (
                    (ni * nj * (2 * n_s + 1) + n_s * (n_s + 1) // 2 * pi_ * pj) * 8))
        if mj is not None and not mfs:
            # what `_major_chunk` holds per map beside the above: a run's planes and the re-imaged
            # residual, the packed lists, V_res and (with scales) G
            n_p = 1 if ms is None else len(ms["planes"])
            extra = ni * nj * (n_p + 1) + 2 * niter + 2 * K * (1 + (0 if ms is None else n_p))
            per = (ni * nj * 3 + pi_ * pj) if ms is None else \
                (ni * nj * (2 * n_p + 1) + n_p * (n_p + 1) // 2 * pi_ * pj)
            step = max(1, self.stack_bytes // ((per + extra) * 8))
        hi, hj = min(self.BEAM_PATCH, pi_) // 2, min(self.BEAM_PATCH, pj) // 2
        mode = _weighting_mode(weighting)
        if mode is not None:
            w_d = eng._device_f64(weights) if weights is not None else None
            if w_d is not None and w_d.numel() != K:
                raise ValueError("dirty image: `weights` must have one entry per baseline (%d)" % K)
            if not mfs:
                step = max(1, min(step, self.stack_bytes // (K * 8)))
        for f0 in range(0, F, step):
            sl = slice(f0, f0 + step)
            iw = None
            if mode is not None:
                isu, isv = image_scales(freqs[sl], cell)
                iw = _imaging_weights(eng, u_d, v_d, isu, isv, w_d, ni, nj, mode, robust, mfs)
            dirty = self._dirty_images(V[sl], u_d, v_d, freqs[sl], weights, (ni, nj), cell_as,
                                       mfs, device=True, iw=iw)
            grow = 0 if ms is None else 4 * ms["hmax"]
            psf = self._dirty_images(ones[sl], u_d, v_d, freqs[sl], weights,
                                     (pi_ + grow, pj + grow), cell_as, mfs, device=True, iw=iw)
            M = int(dirty.shape[0])
            if grow:
                # (the clean beam is fitted to, and the cross beams cropped to, the `psf_shape` window)
                big, g = psf, grow // 2
                psf = big.reshape(M, pi_ + grow, pj + grow)[:, g:g + pi_, g:g + pj].reshape(
                    M, pi_ * pj).contiguous()
            spsf = centres = None
            if ty is not None:
                # B_0 is `psf` itself; the centres of all the spectral beams travel with the patch
                spsf = self._taylor_stack(ones[sl], psf, ty["tw"], u_d, v_d, freqs[sl], weights,
                                          (pi_, pj), cell_as, iw)
            if beam is None or ty is not None:
                ci, cj = (pi_ - 1) // 2, (pj - 1) // 2
                patch = (psf if spsf is None else spsf).reshape(M, -1, pi_, pj)[
                    :, :, ci - hi:ci + hi + 1, cj - hj:cj + hj + 1].cpu().numpy()
                centres = patch[:, :, hi, hj]
            if beam is None:
                abc = [fit_beam(p[0]) for p in patch]
            else:
                abc = [beam_quadratic(beam[0], beam[1], beam[2], cell)] * M
            thr_c = float(thr[0]) if thr.size == 1 else thr[f0:f0 + M]
            cscale = None
            if mj is not None:
                dirty, model, image, cpix, cscale, cflux, ncomp, peak, info = self._major_chunk(
                    V[sl], u_d, v_d, freqs[sl], weights, ni, nj, cell, cell_as, mfs, iw, dirty,
                    psf if not grow else big, psf, pi_, pj, ms, abc, mk, niter, gain, thr_c, mj,
                    # (named only when set: without it the call is, argument for argument, the one
                    # it was, also for a stand-in with the earlier parameter list)
                    **({} if am is None else dict(am=am)))
                if am is not None:
                    res.automask.extend(i.pop("automask") for i in info)
                res.major.extend(info)
            elif am is not None:
                # one mask per map from its dirty image, then one minor run
                side = self._sidelobe_levels(psf, abc, M, pi_, pj)
                um = torch.from_numpy(mk).to(eng.device).reshape(-1) if mk is not None else None
                masks, upd = automask_step(eng, dirty, None, um, side, abc, am, shape=(ni, nj))
                t = np.array(np.broadcast_to(np.asarray(thr_c, dtype=np.float64).reshape(-1), (M,)))
                if am["nsigma"] > 0.:
                    t = np.maximum(t, am["nsigma"] * np.array([u["sigma"] for u in upd]))
                model = torch.zeros_like(dirty)
                live = np.array([u["n_mask"] > 0 for u in upd])
                cpix, cflux, ncomp = self._clean_per_map(dirty, psf, ni, nj, pi_, pj, niter, gain, t,
                                                         masks, live, model=model)
                image = eng.restore(cpix, cflux, ncomp, abc, ni, nj, add=dirty)
                inside = (masks != 0) & torch.isfinite(dirty)
                peak = torch.where(inside, dirty.abs(), torch.zeros_like(dirty)).amax(dim=1)
                hm = (masks != 0).cpu().numpy().reshape(M, ni, nj)
                res.automask.extend(dict(mask=hm[m].copy(), runs=[dict(upd[m], start=0)])
                                    for m in range(M))
            elif ty is not None:
                planes = self._taylor_stack(V[sl], dirty, ty["tw"][:ty["n_t"]], u_d, v_d, freqs[sl],
                                            weights, (ni, nj), cell_as, iw)
                dirty, model, image, cpix, cflux, ncomp, peak, info = self._mtmfs_chunk(
                    planes, spsf, centres, ni, nj, pi_, pj, ty, abc, mk, niter, gain, thr_c)
                res.taylor.extend(info)
                del planes, spsf
            elif ms is None:
                model = torch.zeros_like(dirty)
                cpix, cflux, ncomp, peak = eng.clean(dirty, ni, nj, psf, pi_, pj, niter, gain, thr_c,
                                                     mask=mk, model=model)
                image = eng.restore(cpix, cflux, ncomp, abc, ni, nj, add=dirty)
            else:
                dirty, model, image, cpix, cscale, cflux, ncomp, peak = self._msclean_chunk(
                    dirty, psf if not grow else big, ni, nj, pi_, pj, ms, abc, niter, gain, thr_c)
            o = slice(f0, f0 + M)
            if fit_opts is not None:
                res.imfit.extend(self._imfit_images(image, ni, nj, abc, cell, fit_opts, o))
            res.image[o] = image.cpu().numpy().reshape(M, ni, nj)
            res.residual[o] = dirty.cpu().numpy().reshape(M, ni, nj)
            res.model[o] = model.cpu().numpy().reshape(M, ni, nj)
            res.peak_residual[o] = peak.cpu().numpy()
            hp, hf, hn = cpix.cpu().numpy(), cflux.cpu().numpy(), ncomp.cpu().numpy()
            hs = cscale.cpu().numpy() if cscale is not None else None
            for m in range(M):
                n = int(hn[m])
                # (multi-term: hf is [M, niter, n_t], the rows are (ix, iz, c_0 .. c_{n_t - 1}))
                cols = [hp[m, :n] // nj, hp[m, :n] % nj] + \
                    ([hf[m, :n]] if hf.ndim == 2 else [hf[m, :n, t] for t in range(hf.shape[2])])
                if hs is not None:
                    cols.append(ms["planes"][hs[m, :n]])          # (ix, iz, flux, scale [pixels])
                res.components.append(np.stack(cols, axis=1).astype(np.float64)
                                      .reshape(n, len(cols)))
                res.beam.append(beam_from_quadratic(*abc[m], cell))
            del dirty, psf, model, image, cpix, cflux, ncomp, peak, iw
        return res

    def _taylor_stack(self, V, first, tw, u_d, v_d, freqs, weights, shape, cell_as, iw):
        """The `mfs` images of `V` [F, K] times each row of `tw` [n, F] on the grid `shape` -> device
        [1, n, ni * nj].  Row 0 of `tw` is 1: that image is `first` [1, ni * nj], made before with
        the same arguments; the others go through `_dirty_images` with the same weights `iw` (or
        the same natural weights) and hence the same normaliser."""
        import torch
        out = [first]
        for q in range(1, len(tw)):
            wq = torch.from_numpy(np.ascontiguousarray(tw[q])).to(self.engine.device)
            out.append(self._dirty_images(V * wq[:, None], u_d, v_d, freqs, weights, shape, cell_as,
                                          True, device=True, iw=iw))
        return torch.stack(out, dim=1).contiguous()

    def _mtmfs_chunk(self, planes, spsf, centres, ni, nj, pi_, pj, ty, abc, mk, niter, gain, thr):
        """Multi-term MFS CLEAN of one chunk: `planes` [M, n_t, ni * nj] the Taylor dirty images,
        `spsf` [M, 2 n_t - 1, pi_ * pj] the spectral beams, `centres` [M, 2 n_t - 1] their centre
        values on the host -> (raw R_0, tt0 delta model, tt0 image [M, ni * nj], cpix, ccoef
        [M, niter, n_t], ncomp, peak [M] = the final max |a_0|, info: per map the dict of
        `CleanResult.taylor`), all but `info` on the device.  tt[t] = `restore` of (cpix,
        ccoef[..., t]) plus term t of the principal solution of the final residual planes,
        sum_q Hinv[t][q] R_q; alpha = tt1 / tt0 where tt0 > the cut (None: 0.1 of the largest tt0),
        NaN elsewhere; beta = tt2 / tt0 - alpha (alpha - 1) / 2 with three terms or more."""
        import torch
        eng = self.engine
        M, n_t = int(planes.shape[0]), ty["n_t"]
        hs = [taylor_hessian_inverse(c) for c in centres]
        hinv = np.stack([h[1] for h in hs])
        model = torch.zeros_like(planes)
        cpix, ccoef, ncomp, peak = eng.mtmfs(planes, n_t, ni, nj, spsf, pi_, pj, hinv, niter, gain,
                                             thr, mask=mk, model=model)
        hd = torch.from_numpy(hinv).to(eng.device)
        tt = []
        for t in range(n_t):
            ps = hd[:, t, 0, None] * planes[:, 0]
            for q in range(1, n_t):
                ps = ps + hd[:, t, q, None] * planes[:, q]
            tt.append(eng.restore(cpix, ccoef[:, :, t].contiguous(), ncomp, abc, ni, nj, add=ps))
        h_tt = torch.stack(tt, dim=1).cpu().numpy().reshape(M, n_t, ni, nj)
        h_res = planes.cpu().numpy().reshape(M, n_t, ni, nj)
        h_mod = model.cpu().numpy().reshape(M, n_t, ni, nj)
        info = []
        for m in range(M):
            tt0 = h_tt[m, 0]
            cut = ty["alpha_cut_jy"]
            if cut is None:
                top = np.nanmax(tt0) if np.isfinite(tt0).any() else np.nan
                cut = 0.1 * float(top)
            with np.errstate(divide="ignore", invalid="ignore"):
                ok = tt0 > cut
                alpha = np.where(ok, h_tt[m, 1] / tt0, np.nan)
                beta = np.where(ok, h_tt[m, 2] / tt0 - alpha * (alpha - 1.) / 2., np.nan) \
                    if n_t >= 3 else None
            info.append(dict(tt=h_tt[m], residual_tt=h_res[m], model_tt=h_mod[m], alpha=alpha,
                             beta=beta, alpha_cut_jy=float(cut), reffreq_hz=ty["reffreq_hz"],
                             hessian=hs[m][0], hinv=hs[m][1]))
        return (planes[:, 0].contiguous(), model[:, 0].contiguous(), tt[0], cpix, ccoef, ncomp, peak,
                info)

    def _sidelobe_levels(self, psf, abc, M, pi_, pj):
        """sidelobe[m] of `_major_chunk`'s docstring for the beam windows `psf` [M, pi_ * pj] and
        the clean beams' forms `abc` -> host array [M]."""
        import torch
        eng = self.engine
        q = torch.from_numpy(np.asarray(abc, dtype=np.float64).reshape(M, 3)).to(eng.device)
        dx = (torch.arange(pi_, dtype=torch.float64, device=eng.device) - (pi_ - 1) // 2)[None, :, None]
        dz = (torch.arange(pj, dtype=torch.float64, device=eng.device) - (pj - 1) // 2)[None, None, :]
        form = q[:, 0, None, None] * dx * dx + 2. * q[:, 1, None, None] * dx * dz + \
            q[:, 2, None, None] * dz * dz
        win = psf.reshape(M, pi_, pj).abs()
        return torch.where(form >= _FOUR_LN2, win, torch.zeros_like(win)).amax(dim=(1, 2)).cpu().numpy()

    def _major_chunk(self, V, u_d, v_d, freqs, weights, ni, nj, cell, cell_as, mfs, iw, dirty, beam,
                     psf, pi_, pj, ms, abc, mk, niter, gain, thr, mj, am=None):
        """CLEAN with major cycles of one chunk: N = mj["major_cycles"] minor runs at most, the
        residual recomputed from the visibilities after every one -> (residual, model, image
        [M, ni * nj], cpix, cscale (None without scales), cflux [M, niter], ncomp, peak_residual
        [M], info: per map the dict of `CleanResult.major`), all but `info` on the device.
        `dirty` [M, ni * nj] and `psf` [M, pi_ * pj] are the chunk's dirty images and beam windows,
        `beam` what `_msclean_chunk` takes (multi-scale) and `iw` the chunk's imaging weights: all
        made once.  sidelobe[m] = max |psf| over the window's pixels with A dx^2 + 2 B dx dz +
        C dz^2 >= 4 ln 2 of the clean beam's form -- outside twice its half-power ellipse; this
        project's definition, not CASA's -- 0 when there is no such pixel.  Run r = 1 .. N:
        peak[m] = the masked max of what the minor cycle compares (|R|; the score with scales); a
        map with no iteration left or peak <= thr is finished, and the loop ends when every map
        is; the run's threshold is thr[m] on run N, before it max(thr[m], clip(cyclefactor
        sidelobe[m], min_psf_fraction, max_psf_fraction) peak[m]), and the largest finite double
        for a finished map; it runs min(cycleniter or niter, max_m left[m]) iterations and a map
        keeps the first left[m] of what it finds (the picks are sequential: what n_iter = left[m]
        would have found), appended to its packed list.  Then V_res = V - the visibilities of the
        WHOLE list (`RTEngine.vis_components` on the original V, never on the previous V_res) and
        the residual is `_dirty_images` of V_res with the dirty image's weights; with scales the
        planes are its convolutions.  The products are functions of the final list and the data:
        the last residual, `RTEngine.components_image` (and the scale kernels), `restore` plus the
        residual, its masked max."""
        import torch
        eng = self.engine
        M, F, K = int(dirty.shape[0]), int(V.shape[0]), int(V.shape[1])
        su, sv = image_scales(freqs, cell)
        if mfs:
            cu, cv, _ = _mfs_points(eng, u_d, v_d, su, sv, None)
            su = sv = [1.0]
            V0 = V.reshape(1, F * K).contiguous()
        else:
            cu, cv, V0 = u_d, v_d, V.contiguous()
        side = self._sidelobe_levels(psf, abc, M, pi_, pj)
        n_s, G, cscale_all = 1, None, None
        if ms is None:
            dmask = torch.from_numpy(mk).to(eng.device).reshape(1, -1) if mk is not None else None
        else:
            n_s, hmax, dmask = len(ms["planes"]), ms["hmax"], ms["mask"].reshape(1, -1)
            conv, xpsf, weight = self._ms_setup(beam, M, pi_, pj, ms)
            wd = torch.from_numpy(np.ascontiguousarray(weight)).to(eng.device)
            # G[m, s, k]: the transform of scale s's kernel, zero-padded and centred on one odd side
            gs = 2 * hmax + 1
            kers = torch.zeros(n_s, gs, gs, dtype=torch.float64, device=eng.device)
            for k, kk in enumerate(ms["ker"]):
                h = (int(kk.shape[0]) - 1) // 2
                kers[k, hmax - h:hmax + h + 1, hmax - h:hmax + h + 1] = kk
            G = eng.vis(kers.reshape(n_s, gs * gs).repeat(M, 1).contiguous(), gs, gs,
                        np.repeat(su, n_s), np.repeat(sv, n_s), cu, cv).reshape(M, n_s, -1).contiguous()
            cscale_all = torch.zeros(M, niter, dtype=torch.int32, device=eng.device)
        cpix_all = torch.zeros(M, niter, dtype=torch.int32, device=eng.device)
        cflux_all = torch.zeros(M, niter, dtype=torch.float64, device=eng.device)
        thr = np.array(np.broadcast_to(np.asarray(thr, dtype=np.float64).reshape(-1), (M,)))
        left, n_all = np.full(M, niter, dtype=np.int64), np.zeros(M, dtype=np.int64)
        runs = [[] for _ in range(M)]
        frac = np.clip(mj["cyclefactor"] * side, mj["min_psf_fraction"], mj["max_psf_fraction"])
        N, R, Vres = mj["major_cycles"], dirty, V0

        def masked(x):
            ok = torch.isfinite(x) if dmask is None else dmask & torch.isfinite(x)
            return torch.where(ok, x.abs(), torch.zeros_like(x)).amax(dim=1)

        def count():
            return torch.from_numpy(n_all.astype(np.int32)).to(eng.device)

        am_runs, am_sigma, um = [[] for _ in range(M)], np.zeros(M), None
        if am is not None:
            # the automatic masks, one per map, inside the user's; empty before the first update
            um = dmask
            dmask = torch.zeros(M, ni * nj, dtype=torch.bool, device=eng.device)
        for r in range(1, N + 1):
            if am is not None:
                masks, upd = automask_step(eng, R, dmask, um, side, abc, am, shape=(ni, nj))
                dmask = masks != 0
                for m in range(M):
                    am_runs[m].append(dict(upd[m], start=int(n_all[m])))
                    am_sigma[m] = upd[m]["sigma"]
            if ms is None:
                planes = R.clone()
                peak = masked(planes).cpu().numpy()
            else:
                planes = torch.stack([conv(R, ni, nj, l) for l in range(n_s)], dim=1).contiguous()
                # the score, weight[k] |R_k[p]|, over the planes that may be picked
                peak = torch.stack([masked(planes[:, l] * wd[:, l, None]) for l in range(n_s)],
                                   dim=1).amax(dim=1).cpu().numpy()
            active = (left > 0) & (peak > thr)
            if am is not None:
                # (a map whose mask is empty is finished for this run)
                active &= np.array([u["n_mask"] > 0 for u in upd])
            if not active.any():
                break
            t = thr if r == N else np.maximum(thr, frac * peak)
            if am is not None and am["nsigma"] > 0.:
                t = np.maximum(t, am["nsigma"] * am_sigma)
            t = np.where(active, t, np.finfo(np.float64).max)
            n_r = int(min(mj["cycleniter"] or niter, left.max()))
            if am is not None:
                cp, cf, nc = self._clean_per_map(planes, psf, ni, nj, pi_, pj, n_r, gain, t, dmask,
                                                 active)
            elif ms is None:
                cp, cf, nc, _ = eng.clean(planes, ni, nj, psf, pi_, pj, n_r, gain, t, mask=mk)
            else:
                cp, cs, cf, nc, _ = eng.msclean(planes, n_s, ni, nj, xpsf, pi_, pj, weight, n_r,
                                                gain, t, mask=ms["mask"])
            take = np.where(active, np.minimum(nc.cpu().numpy(), left), 0)
            # one masked scatter: slot j < take[m] of the run goes to slot n_all[m] + j of the list
            j = torch.arange(n_r, device=eng.device)[None, :]
            sel = j < torch.from_numpy(take).to(eng.device)[:, None]
            row = torch.arange(M, device=eng.device)[:, None].expand(M, n_r)[sel]
            dst = (torch.from_numpy(n_all).to(eng.device)[:, None] + j)[sel]
            cpix_all[row, dst] = cp[sel]
            cflux_all[row, dst] = cf[sel]
            if ms is not None:
                cscale_all[row, dst] = cs[sel]
            for m in np.nonzero(active)[0]:
                runs[m].append(dict(start=int(n_all[m]), n=int(take[m]), peak=float(peak[m]),
                                    threshold=float(t[m])))
            n_all += take
            left -= take
            del planes, cp, cf, nc, sel, row, dst
            Vres = eng.vis_components(cpix_all, cflux_all, count(), ni, nj, su, sv, cu, cv,
                                      cscale=cscale_all, n_s=n_s, gvis=G, vis_in=V0, sign=-1)
            R = self._dirty_images(Vres.reshape(F, K) if mfs else Vres, u_d, v_d, freqs, weights,
                                   (ni, nj), cell_as, mfs, device=True, iw=iw)
        ncomp = count()
        model = eng.components_image(cpix_all, cflux_all, ncomp, ni, nj, cscale=cscale_all, n_s=n_s)
        if ms is None:
            model = model.reshape(M, ni * nj)
            image = eng.restore(cpix_all, cflux_all, ncomp, abc, ni, nj, add=R)
            peak = masked(R)
        else:
            model, image, peak = self._ms_products(R, model, cpix_all, cscale_all, cflux_all, ncomp,
                                                   abc, ni, nj, ms, conv)
        hv = Vres.cpu().numpy()
        info = [dict(runs=runs[m], sidelobe=float(side[m]), vis_residual=hv[m].copy())
                for m in range(M)]
        if am is not None:
            hm = dmask.cpu().numpy().reshape(M, ni, nj)
            for m in range(M):
                # (`_clean_images` moves this entry to `CleanResult.automask`)
                info[m]["automask"] = dict(mask=hm[m].copy(), runs=am_runs[m])
        return R, model, image, cpix_all, cscale_all, cflux_all, ncomp, peak, info

    def _clean_per_map(self, planes, psf, ni, nj, pi_, pj, n_iter, gain, thr, masks, active,
                       model=None):
        """`RTEngine.clean` of a stack whose maps have masks of their own: rjp_clean takes one mask
        for all maps, so this is ONE call per map of `active`, in place on that map's row of
        `planes` (and `model`), with its row of `masks` [M, ni nj] and its threshold -> (cpix
        [M, n_iter] int32, cflux [M, n_iter], ncomp [M] int32) on the device, zero for the maps
        that did not run.  M times as many launches as one call on the stack; with `mfs` M = 1."""
        import torch
        eng = self.engine
        M = int(planes.shape[0])
        cpix = torch.zeros(M, n_iter, dtype=torch.int32, device=eng.device)
        cflux = torch.zeros(M, n_iter, dtype=torch.float64, device=eng.device)
        ncomp = torch.zeros(M, dtype=torch.int32, device=eng.device)
        slot = torch.arange(n_iter, device=eng.device)
        for m in np.nonzero(active)[0]:
            m = int(m)
            cp, cf, nc, _ = eng.clean(planes[m:m + 1], ni, nj, psf[m:m + 1], pi_, pj, n_iter, gain,
                                      float(thr[m]), mask=masks[m],
                                      model=None if model is None else model[m:m + 1])
            # (the slots at and beyond nc are not written by `clean`: they stay zero here; nothing
            # is read back, so the calls of a run queue up behind each other)
            found = slot < nc[0]
            cpix[m] = torch.where(found, cp[0], torch.zeros_like(cp[0]))
            cflux[m] = torch.where(found, cf[0], torch.zeros_like(cf[0]))
            ncomp[m] = nc[0]
        return cpix, cflux, ncomp

    def _msclean_chunk(self, dirty, beam, ni, nj, pi_, pj, ms, abc, niter, gain, thr):
        """Multi-scale CLEAN of one chunk's dirty images [M, ni * nj] -> (raw residual, model,
        image [M, ni * nj], cpix, cscale, cflux, ncomp, peak_residual), all on the device.
        `beam` [M, (pi_ + 4 h_max)(pj + 4 h_max)]: the dirty beams on the enlarged grid, so that
        the cross beams X[k][l] = m_k * m_l * B, cropped to the centre (pi_, pj) window, are exact
        in the window and not truncated at its edge.  Planes R_l = m_l * D; weight[m][k] =
        bias_k / X_kk(centre), which makes the score the component's flux times the bias (CASA's
        normalisation); model = sum_k m_k * (delta model k); image = raw residual + sum_k m_k *
        restore(components of scale k).  `peak_residual`: the masked max of the raw plane."""
        import torch
        eng = self.engine
        n_s = len(ms["planes"])
        conv, xpsf, weight = self._ms_setup(beam, int(dirty.shape[0]), pi_, pj, ms)
        res = torch.stack([conv(dirty, ni, nj, l) for l in range(n_s)], dim=1).contiguous()
        model = torch.zeros_like(res)
        cpix, cscale, cflux, ncomp, _ = eng.msclean(res, n_s, ni, nj, xpsf, pi_, pj, weight, niter,
                                                    gain, thr, mask=ms["mask"], model=model)
        del xpsf
        raw = res[:, 0].contiguous()
        total, image, peak = self._ms_products(raw, model, cpix, cscale, cflux, ncomp, abc, ni, nj,
                                               ms, conv)
        return raw, total, image, cpix, cscale, cflux, ncomp, peak

    def _ms_setup(self, beam, M, pi_, pj, ms):
        """What a multi-scale chunk makes once from its dirty beams (`_msclean_chunk`) -> (conv: the
        convolution with scale k's kernel, the cross beams [M, n_s (n_s + 1) / 2, pi_ * pj], the
        weights [M, n_s] on the host)."""
        import torch
        eng = self.engine
        planes, ker, hmax = ms["planes"], ms["ker"], ms["hmax"]
        n_s = len(planes)
        bi, bj = pi_ + 4 * hmax, pj + 4 * hmax

        def conv(x, nx, nz, k, add=None):
            # (the delta scale's kernel is [[1.0]]: the identity, nothing to launch)
            if ker[k].numel() == 1 and add is None:
                return x
            side = int(ker[k].shape[0])
            return eng.convolve2d(x, nx, nz, ker[k].reshape(-1), side, side, add=add)

        g = 2 * hmax
        single = [conv(beam, bi, bj, k) for k in range(n_s)]
        xpsf = torch.stack([conv(single[k], bi, bj, l).reshape(M, bi, bj)[:, g:g + pi_, g:g + pj]
                            for k in range(n_s) for l in range(k, n_s)], dim=1)
        xpsf = xpsf.reshape(M, -1, pi_ * pj).contiguous()
        del single
        centre = ((pi_ - 1) // 2) * pj + (pj - 1) // 2
        diag = [k * n_s - k * (k - 1) // 2 for k in range(n_s)]
        xkk = xpsf[:, diag, centre].cpu().numpy()                       # [M, n_s]: a few numbers
        with np.errstate(divide="ignore", invalid="ignore"):
            weight = np.where(ms["bias"][None, :] > 0., ms["bias"][None, :] / xkk, 0.)
        if not np.all(np.isfinite(weight) & (weight >= 0.)):
            raise ValueError("clean: a scale's beam X_kk is not positive at its centre")
        return conv, xpsf, weight

    def _ms_products(self, raw, model, cpix, cscale, cflux, ncomp, abc, ni, nj, ms, conv):
        """The products of a multi-scale chunk from its raw residual [M, ni * nj], the delta models
        [M, n_s, ni * nj] and the component list -> (model, image [M, ni * nj], peak_residual)."""
        import torch
        eng = self.engine
        total, image = model[:, 0].contiguous(), raw          # (plane 0 is the delta scale)
        for k in range(len(ms["planes"])):
            # K13 with the other scales' fluxes zeroed, then the scale's kernel, chained by `add`
            fk = torch.where(cscale == k, cflux, torch.zeros_like(cflux))
            if k == 0:
                image = eng.restore(cpix, fk, ncomp, abc, ni, nj, add=image)
                continue
            total = conv(model[:, k].contiguous(), ni, nj, k, add=total)
            image = conv(eng.restore(cpix, fk, ncomp, abc, ni, nj), ni, nj, k, add=image)
        ok = ms["mask"].reshape(1, -1) & torch.isfinite(raw)
        peak = torch.where(ok, raw.abs(), torch.zeros_like(raw)).amax(dim=1)
        return total, image, peak

    # ------------------------------------------------------------------ synthetic observations ----
    def uv_tracks(self, antennalist, dec_deg, t_obs_s, t_int_s, min_el_deg=None, hourangle_h=0.):
        """See `JetModel.uv_tracks`, which takes `dec_deg` from the model's target."""
        cfg = antennalist if isinstance(antennalist, AntennaConfig) else \
            read_antenna_config(antennalist)
        geo = geodetic(cfg.xyz)
        ha, day = observing_plan(dec_deg, geo.lat0_deg, t_obs_s, t_int_s,
                                 0. if min_el_deg is None else min_el_deg, hourangle_h)
        flags = dict(up=geo.up, min_el_rad=np.radians(min_el_deg)) if min_el_deg is not None else {}
        u, v, w = self.engine.uv_tracks(cfg.xyz, ha - geo.lon0_deg / 360., np.radians(dec_deg),
                                        **flags)
        a1, a2 = np.triu_indices(len(cfg.names), 1)
        bmax = float(np.sqrt(((cfg.xyz[a2] - cfg.xyz[a1]) ** 2).sum(axis=1)).max())
        return UVTracks(u.reshape(-1), v.reshape(-1), w.reshape(-1), ha * 24., day,
                        a1.astype(np.int32), a2.astype(np.int32), bmax)

    def _observe(self, maps, freqs, tracks, t_int_s, sigma_jy, sefd_jy, chanwidth_hz, seed,
                 nsigma, weights, shape, cell_as, mfs, niter, gain, threshold_jy, mask, beam,
                 psf_shape, imfit, weighting, robust, automask=None, scales=None, scale_bias=None,
                 nterms=1,
                 reffreq_hz=None, alpha_cut_jy=None, major_cycles=0,
                 cyclefactor=1.5, cycleniter=None, min_psf_fraction=0.05, max_psf_fraction=0.8):
        """`JetModel.observe_*` after the maps [F, nx * nz]: visibilities, noise, image rms, CLEAN."""
        F = len(freqs)
        if sigma_jy is not None and sefd_jy is not None:
            raise ValueError("observe: give `sigma_jy` or `sefd_jy`, not both")
        if sefd_jy is not None:
            if chanwidth_hz is None:
                raise ValueError("observe: `sefd_jy` needs `chanwidth_hz`")
            sigma_jy = thermal_sigma(sefd_jy, chanwidth_hz, t_int_s)
        sigma = np.asarray(0. if sigma_jy is None else sigma_jy, dtype=np.float64).reshape(-1)
        if sigma.size not in (1, F) or not np.all(np.isfinite(sigma) & (sigma >= 0.)):
            raise ValueError("observe: `sigma_jy` must be one finite rms >= 0 or one per channel")
        sigma = np.broadcast_to(sigma, (F,)).copy()
        if not (float(nsigma) >= 0.):
            raise ValueError("observe: `nsigma` must be >= 0")
        u_d, v_d = tracks.u_m, tracks.v_m
        V0 = self.model_vis(maps, freqs, u_d, v_d)
        noisy = bool(np.any(sigma > 0.))
        # (every visibility has its own counter k = t n_bl + b: an independent draw per day,
        # integration, baseline and channel)
        V = self.engine.vis_noise(V0, sigma, seed=seed) if noisy else V0
        rms = np.zeros(1 if mfs else F)
        if noisy:
            iw, _ = self.imaging_weights(u_d, v_d, freqs, weights=weights, shape=shape,
                                         cell_as=cell_as, weighting=weighting, robust=robust,
                                         mfs=mfs)
            rms = image_rms(iw.reshape(1, -1), np.repeat(sigma, iw.shape[1])) if mfs else \
                image_rms(iw, sigma[:, None])
            del iw
        thr = threshold_jy
        if float(nsigma) > 0.:
            thr = np.maximum(float(thr), float(nsigma) * np.where(np.isfinite(rms), rms, 0.))
        if imfit is not None and imfit is not False and noisy:
            imfit = {} if imfit is True else dict(imfit)
            if imfit.get("rms") is None:
                imfit["rms"] = rms
        res = self._clean_images(V, u_d, v_d, freqs, weights, shape, cell_as, mfs, niter, gain,
                                 thr, mask, beam, psf_shape, imfit, weighting=weighting,
                                 robust=robust, scales=scales, scale_bias=scale_bias,
                                 nterms=nterms, reffreq_hz=reffreq_hz, alpha_cut_jy=alpha_cut_jy,
                                 major_cycles=major_cycles, cyclefactor=cyclefactor,
                                 cycleniter=cycleniter, min_psf_fraction=min_psf_fraction,
                                 max_psf_fraction=max_psf_fraction,
                                 # (named only when set, as in `_clean_images`' call of `_major_chunk`)
                                 **({} if automask is None else dict(automask=automask)))
        v0 = V0.cpu().numpy()
        return Observation(tracks, v0, V.cpu().numpy() if noisy else v0.copy(), sigma, rms, res)

    # ------------------------------------------------------------------ imfit ----
    def _imfit_options(self, imfit, mask, ni, nj):
        """The `imfit` keyword of `clean_image_*` / `imfit` -> None or a dict (box, theta0,
        n_iter, rms); the default box is the bounding box of `mask` (as `_clean_mask` reads it)."""
        if imfit is None or imfit is False:
            return None
        opts = {} if imfit is True else dict(imfit)
        bad = set(opts) - {"box", "theta0", "n_iter", "rms"}
        if bad:
            raise ValueError("imfit: unknown option(s) %s" % sorted(bad))
        box = opts.get("box")
        if box is None:
            mk = self._clean_mask(mask, ni, nj)
            if mk is not None and mk.any():
                ii, jj = np.nonzero(mk)
                box = (int(ii.min()), int(ii.max()), int(jj.min()), int(jj.max()))
            else:
                box = (0, ni - 1, 0, nj - 1)
        box = tuple(int(x) for x in np.ravel(box))
        if len(box) != 4 or not (0 <= box[0] <= box[1] < ni and 0 <= box[2] <= box[3] < nj):
            raise ValueError("imfit: the box (i0, i1, j0, j1) must lie inside the image")
        return {"box": box, "theta0": opts.get("theta0"), "n_iter": int(opts.get("n_iter", 60)),
                "rms": opts.get("rms")}

    def _imfit_images(self, image, ni, nj, abc, cell, opts, sl=None):
        """One Gaussian per image of the device stack `image` [M, ni * nj] (`RTEngine.gaussfit`)
        -> list of M dicts (`gauss_results`).  `abc`: the clean beams, one per map; `sl`: the
        rows of a `theta0` / `rms` given per map that belong to this stack."""
        import torch

        def pick(a, w):
            # (a start or an rms per map: a host array or a tensor; else one for all)
            if a is None or sl is None:
                return a
            if isinstance(a, torch.Tensor):
                return a[sl] if a.dim() >= w else a
            return np.asarray(a)[sl] if np.ndim(a) >= w else a
        theta0 = pick(opts["theta0"], 2)
        if theta0 is None:
            theta0 = gauss_start(image, ni, nj, abc, box=opts["box"])
        fit = self.engine.gaussfit(image, ni, nj, theta0, box=opts["box"], n_iter=opts["n_iter"])
        host = {k: v.cpu().numpy() for k, v in fit.items()}
        rms = pick(opts["rms"], 1)
        if isinstance(rms, torch.Tensor):
            rms = rms.detach().cpu().numpy()
        return gauss_results(host["theta"], host["cov"], host["chi2"], host["npix"], abc, cell,
                             rms=rms, shape=(ni, nj), status=host["status"])

    def imfit(self, images, beam, cell_as=None, box=None, theta0=None, n_iter=60, rms=None):
        """See `JetModel.imfit`."""
        import torch
        eng = self.engine
        if isinstance(images, torch.Tensor):
            img = images.to(device=eng.device, dtype=torch.float64)
        else:
            img = torch.from_numpy(np.ascontiguousarray(images, dtype=np.float64)).to(eng.device)
        if img.dim() == 2:
            img = img.unsqueeze(0)
        if img.dim() != 3:
            raise ValueError("imfit: `images` must be (F, ni, nj) or (ni, nj)")
        M, ni, nj = (int(x) for x in img.shape)
        _, _, cell = self._image_grid((ni, nj), cell_as)
        beams = np.asarray(beam, dtype=np.float64).reshape(-1, 3)
        if beams.shape[0] not in (1, M):
            raise ValueError("imfit: `beam` must be one (bmaj_as, bmin_as, bpa_deg) or one per image")
        abc = [beam_quadratic(b[0], b[1], b[2], cell) for b in np.broadcast_to(beams, (M, 3))]
        opts = self._imfit_options({"box": box, "theta0": theta0, "n_iter": n_iter, "rms": rms},
                                   None, ni, nj)
        return self._imfit_images(img.reshape(M, ni * nj).contiguous(), ni, nj, abc, cell, opts)

    # ------------------------------------------------------------------ imstat, automask ----
    def _image_stack(self, who, images):
        """`images` (F, ni, nj) or (ni, nj), host or device -> (float64 device tensor [M, ni nj],
        M, ni, nj)."""
        import torch
        eng = self.engine
        if isinstance(images, torch.Tensor):
            img = images.to(device=eng.device, dtype=torch.float64)
        else:
            img = torch.from_numpy(np.ascontiguousarray(images, dtype=np.float64)).to(eng.device)
        if img.dim() == 2:
            img = img.unsqueeze(0)
        if img.dim() != 3:
            raise ValueError("%s: `images` must be (F, ni, nj) or (ni, nj)" % who)
        M, ni, nj = (int(x) for x in img.shape)
        return img.reshape(M, ni * nj).contiguous(), M, ni, nj

    def _mask_planes(self, who, name, mask, M, ni, nj, per_map=True):
        """None, or `mask` (ni, nj) -- with `per_map` also (M, ni, nj) -- host or device -> bool
        device tensor [1 or M, ni nj]."""
        import torch
        if mask is None:
            return None
        if not isinstance(mask, torch.Tensor):
            mask = torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0))
        mask = (mask != 0).to(self.engine.device)
        ok = [(ni, nj)] + ([(M, ni, nj)] if per_map else [])
        if tuple(mask.shape) not in ok:
            raise ValueError("%s: `%s` must have the shape %s" % (who, name, " or ".join(map(str, ok))))
        return mask.reshape(-1, ni * nj).contiguous()

    def imstat(self, images, mask=None, inside=True):
        """See `JetModel.imstat`."""
        img, M, ni, nj = self._image_stack("imstat", images)
        mk = self._mask_planes("imstat", "mask", mask, M, ni, nj)
        return image_stats_results(self.engine.image_stats(img, ni, nj, mask=mk, inside=inside))

    def automask(self, images, beam, sidelobe=0., mask=None, prev=None, options=None):
        """See `JetModel.automask`."""
        img, M, ni, nj = self._image_stack("automask", images)
        opts = automask_options(dict(options) if options else True)
        _, _, cell = self._image_grid((ni, nj), None)
        beams = np.asarray(beam, dtype=np.float64).reshape(-1, 3)
        if beams.shape[0] not in (1, M):
            raise ValueError("automask: `beam` must be one (bmaj_as, bmin_as, bpa_deg) or one per image")
        abc = [beam_quadratic(b[0], b[1], b[2], cell) for b in np.broadcast_to(beams, (M, 3))]
        side = np.asarray(sidelobe, dtype=np.float64).reshape(-1)
        if side.size not in (1, M):
            raise ValueError("automask: `sidelobe` must be one number or one per image")
        um = self._mask_planes("automask", "mask", mask, M, ni, nj, per_map=False)
        pv = self._mask_planes("automask", "prev", prev, M, ni, nj)
        if pv is not None and int(pv.shape[0]) != M:
            pv = pv.expand(M, ni * nj).contiguous()
        masks, info = automask_step(self.engine, img, pv, um, np.broadcast_to(side, (M,)), abc, opts,
                                    shape=(ni, nj))
        return (masks != 0).cpu().numpy().reshape(M, ni, nj), info

    # ------------------------------------------------------------------ uvmodelfit ----
    @staticmethod
    def _uvfit_options(comps, comptype, theta0, free):
        """(n_comp, the P free flags or None, the sizes to zero [P] bool) of the `comps`,
        `comptype` and `free` of `uvmodelfit`.  `comptype`: None (all Gaussians) or one of 'G' /
        'P' per component; a 'P' component is a point: its sizes start at 0 and stay fixed."""
        nc = int(comps)
        if nc != comps or not 1 <= nc <= UVFIT_MAX_COMP:
            raise ValueError("uvmodelfit: `comps` must be an integer from 1 to %d" % UVFIT_MAX_COMP)
        if theta0 is None and nc != 1:
            raise ValueError("uvmodelfit: a start for more than one component is the caller's "
                             "(`theta0`)")
        P = 6 * nc
        fr = None if free is None else (np.asarray(free).reshape(-1) != 0)
        if fr is not None and fr.size != P:
            raise ValueError("uvmodelfit: `free` must hold %d flags" % P)
        point = np.zeros(P, dtype=bool)
        if comptype is not None:
            kinds = [comptype] * nc if isinstance(comptype, str) else list(comptype)
            if len(kinds) != nc or any(k not in ("G", "P") for k in kinds):
                raise ValueError("uvmodelfit: `comptype` must be 'G' or 'P', one per component")
            for c, k in enumerate(kinds):
                point[6 * c + 3:6 * c + 6] = k == "P"
            if point.any():
                fr = (np.ones(P, dtype=bool) if fr is None else fr) & ~point
        if fr is not None and not fr.any():
            raise ValueError("uvmodelfit: at least one parameter must be free")
        return nc, fr, point

    def _uvfit_stack(self, V, su, sv, u_d, v_d, w_d, theta0, fr, point, n_iter, cell):
        """One `RTEngine.uvfit` call on the device stack `V` [M, K] -> (`uvfit_results` lists, the
        device outputs).  `theta0`: None (`uvfit_start`), or a start as `RTEngine.uvfit` takes it."""
        import torch
        eng = self.engine
        if theta0 is None:
            theta0 = uvfit_start(V, su, sv, u_d, v_d, w_d)
        elif not isinstance(theta0, torch.Tensor):
            theta0 = torch.from_numpy(np.ascontiguousarray(theta0, dtype=np.float64)).to(eng.device)
        if point.any():
            theta0 = theta0.clone()
            theta0[..., torch.from_numpy(point).to(theta0.device)] = 0.
        fit = eng.uvfit(V, su, sv, u_d, v_d, theta0, weights=w_d, free=fr, n_iter=n_iter)
        host = {k: t.cpu().numpy() for k, t in fit.items()}
        return uvfit_results(host["theta"], host["cov"], host["chi2"], host["nvis"], fr, cell,
                             status=host["status"]), fit

    def uvmodelfit(self, vis, u_m, v_m, freq, weights=None, cell_as=None, comps=1, comptype=None,
                   theta0=None, free=None, mfs=False, n_iter=60):
        """See `JetModel.uvmodelfit`."""
        import torch
        eng = self.engine
        freqs = np.atleast_1d(np.asarray(freq, dtype=np.float64))
        nc, fr, point = self._uvfit_options(comps, comptype, theta0, free)
        _, _, cell = self._image_grid(None, cell_as)
        if isinstance(vis, torch.Tensor):
            V = vis.to(device=eng.device)
            V = V if V.dtype == torch.complex128 else torch.view_as_complex(
                V.to(torch.float64).contiguous())
        else:
            V = torch.from_numpy(np.ascontiguousarray(vis, dtype=np.complex128)).to(eng.device)
        if V.dim() == 1:
            V = V.unsqueeze(0)
        F = len(freqs)
        if V.dim() != 2 or int(V.shape[0]) != F:
            raise ValueError("uvmodelfit: `vis` must be (F, K) with one row per frequency (%d)" % F)
        K = int(V.shape[1])
        u_d, v_d = eng._device_f64(u_m), eng._device_f64(v_m)
        if u_d.numel() != K or v_d.numel() != K:
            raise ValueError("uvmodelfit: u and v must have one entry per baseline (%d)" % K)
        w_d = eng._device_f64(weights) if weights is not None else None
        if w_d is not None and w_d.numel() not in (K, F * K):
            raise ValueError("uvmodelfit: `weights` must be [K] or [F, K] = [%d, %d]" % (F, K))
        su, sv = image_scales(freqs, cell)
        if mfs:
            # one map of F K points, baselines in cycles per cell, unit scales
            # (weights [K] are repeated per channel; [F, K] are already in that order)
            shared = w_d is not None and w_d.numel() == K
            u_d, v_d, w_rep = _mfs_points(eng, u_d, v_d, su, sv, w_d if shared else None)
            w_d = w_rep if shared else w_d
            V, su, sv = V.reshape(1, F * K), [1.0], [1.0]
        return self._uvfit_stack(V.contiguous(), su, sv, u_d, v_d, w_d, theta0, fr, point,
                                 int(n_iter), cell)[0]
