"""What tests/test_gpu_regions.py holds K25 (rjp_image_stats, rjp_label_regions, rjp_mask_grow) to
-- tests/regions_ref.py -- pinned on the CPU: hand-worked cases; a plain-Python emulation of the
device's radix select on every statistics case and of its tile union-find plus border merge on every
label case (each must equal the reference); planted mistakes, each caught by a named case; the
argument checks from plain C++; the ABI table; the automatic-mask convention of
rajepy_amd.imaging on a recording engine against the reference's restatement; the public surface."""
import ctypes
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from rajepy_amd import _lib, classes, imaging
from rajepy_amd import engine as E
from tests import regions_cases as RC
from tests import regions_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.float64(x).tobytes()


# ---- hand-worked cases ----------------------------------------------------------------------------------
def test_five_pixel_median_and_mad_by_hand():
    st = K.image_stats([7.0, -1.0, 3.0, 10.0, 2.0])
    # sorted: -1 2 3 7 10 -> rank 2 is 3; |x - 3| = 4 4 0 7 1 -> sorted 0 1 4 4 7 -> rank 2 is 4
    assert (st["count"], st["median"], st["mad"], st["min"], st["max"]) == (5.0, 3.0, 4.0, -1.0, 10.0)
    assert float(st["sum"]) == 21.0 and float(st["sumsq"]) == 163.0


def test_even_count_takes_the_lower_element():
    st = K.image_stats([4.0, 1.0, 3.0, 2.0])
    # rank (4 - 1) / 2 = 1 -> 2, never 2.5; |x - 2| = 2 1 1 0 -> sorted 0 1 1 2 -> rank 1 is 1
    assert (st["median"], st["mad"]) == (2.0, 1.0)
    st = K.image_stats([np.nan, 4.0, np.inf, 1.0, 3.0, 2.0, -np.inf], mask=[1, 1, 1, 1, 1, 0, 1], inside=True)
    assert (st["count"], st["n_nonfinite"], st["median"]) == (3.0, 3.0, 3.0)
    st = K.image_stats([-0.0, 0.0])
    assert bits(st["median"]) == bits(-0.0) and bits(st["min"]) == bits(-0.0) and bits(st["max"]) == bits(0.0)
    empty = K.image_stats([1.0, 2.0], mask=[0, 0])
    assert empty["count"] == 0 and np.isnan(empty["median"]) and np.isnan(empty["mad"]) and float(empty["sum"]) == 0


def test_three_by_three_labels_by_hand():
    mask = [1, 0, 1,
            0, 1, 0,
            1, 1, 0]
    lab, area, n = K.label_regions(mask, 3, 3, 1)
    # four neighbours: {0}, {2} and {4, 6, 7} (the centre, the pixel below it and that one's left neighbour)
    assert n == 3 and lab.tolist() == [1, 0, 3, 0, 5, 0, 5, 5, 0] and area.tolist() == [1, 0, 1, 0, 3, 0, 3, 3, 0]
    lab, area, n = K.label_regions(mask, 3, 3, 2)
    assert n == 1 and lab.tolist() == [1, 0, 1, 0, 1, 0, 1, 1, 0] and area.tolist() == [5, 0, 5, 0, 5, 0, 5, 5, 0]


def test_a_corridor_grown_by_two_by_hand():
    seed = [1, 0, 0, 0, 0, 0,
            0, 0, 0, 0, 0, 1]
    con = [1, 1, 1, 1, 1, 0,
           0, 0, 0, 0, 0, 0]
    # two steps along the corridor; the seed at (1, 5) lies outside the constraint and stays
    assert K.mask_grow(seed, con, 2, 6, 2, 1).astype(int).tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1]
    assert K.mask_grow(seed, con, 2, 6, 0, 1).astype(int).tolist() == seed
    assert K.mask_grow(seed, con, 2, 6, -1, 1).astype(int).tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1]
    # with eight neighbours (1, 5) reaches (0, 4) in one step
    assert K.mask_grow(seed, con, 2, 6, 1, 2).astype(int).tolist() == [1, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1]


# ---- the device's algorithms, emulated --------------------------------------------------------------------
def test_radix_select_equals_the_reference_on_every_statistics_case():
    n = 0
    for name, c in RC.stat_cases():
        for m in range(c["img"].shape[0]):
            mk = None if c["mask"] is None else c["mask"][m if c["mask"].shape[0] > 1 else 0]
            ref = K.image_stats(c["img"][m], mk, c["inside"])
            med, mad = K.emulate_stats(c["img"][m], mk, c["inside"])
            assert bits(med) == bits(ref["median"]) and bits(mad) == bits(ref["mad"]), (name, m)
            n += 1
    assert n > 80


def test_the_statistics_cases_cover_what_they_claim():
    cases = dict(RC.stat_cases())
    sizes = {c["nx"] * c["nz"] for c in cases.values()}
    assert {1, 2, 63, 64, 65, 255, 256, 257, 2048, 2049, 65793} <= sizes
    lo = K.image_stats(cases["zeros_lo-23x89"]["img"][0])
    hi = K.image_stats(cases["zeros_hi-23x89"]["img"][0])
    assert bits(lo["median"]) == bits(0.0) and bits(hi["median"]) == bits(-0.0)
    x = cases["ties-23x89"]["img"][0]
    r = (x.size - 1) // 2
    assert np.sort(x)[r - 5] == np.sort(x)[r + 5] == 1.0
    sub = cases["subnormal-16x16"]["img"][0]
    assert 0 < np.abs(sub).max() < 2.3e-308
    huge = np.abs(cases["huge-23x89"]["img"][0])
    assert huge.max() > 2.0 ** 500 and huge.min() < 2.0 ** -500
    assert cases["negative-5x13"]["img"].max() < 0
    assert K.image_stats(cases["normal-nothing-3maps"]["img"][0], cases["normal-nothing-3maps"]["mask"][0])["count"] == 0
    assert np.isnan(cases["normal-per_map_in-3maps"]["img"][1]).all()
    assert {c["nx"] * c["nz"] % 2 for c in cases.values()} == {0, 1}


def test_tile_union_find_equals_the_reference_on_every_label_case():
    for name, c in RC.label_cases():
        for conn in (1, 2):
            for m in range(c["mask"].shape[0]):
                ref = K.label_regions(c["mask"][m], c["nx"], c["nz"], conn)[0]
                assert np.array_equal(K.emulate_labels(c["mask"][m], c["nx"], c["nz"], conn), ref), (name, conn)


def test_the_label_cases_cover_what_they_claim():
    cases = dict(RC.label_cases())
    ser = cases["serpentine-130x65"]["mask"][0]
    lab, area, n = K.label_regions(ser, 130, 65, 1)
    assert n == 1 and int(ser.sum()) == 4290 and int(area.max()) == 4290
    chk = cases["checker-67x131"]["mask"][0]
    assert K.label_regions(chk, 67, 131, 1)[2] == int(chk.sum()) and K.label_regions(chk, 67, 131, 2)[2] == 1
    cor = cases["corner-67x131"]["mask"][0]
    assert K.label_regions(cor, 67, 131, 1)[2] == 2 and K.label_regions(cor, 67, 131, 2)[2] == 1
    u = cases["u-67x131"]["mask"][0].reshape(67, 131)
    assert K.label_regions(u, 67, 131, 1)[2] == 1 and K.label_regions(u[:, :K.TILE_Z], 67, K.TILE_Z, 1)[2] == 2
    # with the 16 x 64 tile the issue's 130 x 65 is 9 x 2 tiles (a border in z, no interior tile along z) and
    # 67 x 131 is 5 x 3; 130 x 131 is there so that the long chain and the dense random masks also meet 9 x 3
    tiles = {(nx, nz): (-(-nx // K.TILE_X), -(-nz // K.TILE_Z)) for nx, nz in RC.BIG}
    assert tiles == {(130, 65): (9, 2), (67, 131): (5, 3), (130, 131): (9, 3)}
    ser = cases["serpentine-130x131"]["mask"][0]
    assert K.label_regions(ser, 130, 131, 1)[2] == 1
    assert set(RC.GROW_SHAPES) == set(RC.LABEL_SHAPES), "the growth runs on the labels' shapes"


# ---- planted mistakes ---------------------------------------------------------------------------------------
def test_planted_mistakes_are_caught_by_named_cases():
    st = dict(RC.stat_cases())
    even = st["normal-16x16"]["img"][0]
    assert K.image_stats(even, upper=True)["median"] != K.image_stats(even)["median"], "upper median"
    neg = st["negative-5x13"]["img"][0]
    assert K.image_stats(neg, mad_of_abs=True)["mad"] != K.image_stats(neg)["mad"], "median of |x|"
    lc = dict(RC.label_cases())
    chk = lc["checker-17x65"]["mask"][0]
    assert not np.array_equal(K.label_regions(chk, 17, 65, 2)[0], K.label_regions(chk, 17, 65, 1)[0]), "8 for 4"
    rnd = lc["random0.59-130x65"]["mask"][0]
    assert not np.array_equal(K.label_regions(rnd, 130, 65, 1, first_found=True)[0],
                              K.label_regions(rnd, 130, 65, 1)[0]), "first-found labels"
    gc = dict(RC.grow_cases())
    cor = gc["corridor-67x131"]
    s, c = cor["seed"][0], cor["con"][0]
    ref = K.mask_grow(s, c, 67, 131, 75, 1)
    assert int(ref.sum()) == 76
    assert not np.array_equal(K.mask_grow(s, c, 67, 131, 75, 1, unconstrained=True), ref), "growth unconstrained"
    assert int(K.mask_grow(s, c, 67, 131, 75, 1, extra=1).sum()) == 77, "one step over"
    for it in (RC.H - 1, RC.H, RC.H + 1):
        assert int(K.mask_grow(s, c, 67, 131, it, 1).sum()) == it + 1
    rn = gc["random-67x131"]
    s, c = rn["seed"][0], rn["con"][0]
    assert ((s != 0) & (c == 0)).any()
    assert not np.array_equal(K.mask_grow(s, c, 67, 131, 3, 1, drop_outside=True),
                              K.mask_grow(s, c, 67, 131, 3, 1)), "seed outside the constraint dropped"


def test_reconstruction_by_regions_equals_dilation_until_stable():
    """The rule rjp_mask_grow uses for n_iter < 0 -- keep the constraint regions that hold a seed or
    a neighbour of one -- against binary_dilation(iterations=0, mask=...)."""
    rng = np.random.default_rng(5)
    for k in range(300):
        nx, nz, conn = int(rng.integers(1, 24)), int(rng.integers(1, 24)), 1 + k % 2
        c = rng.random(nx * nz) < rng.choice([0.3, 0.6, 0.9])
        s = rng.random(nx * nz) < 0.05
        lab = K.label_regions(c, nx, nz, conn)[0]
        near = K.mask_grow(s, np.ones(nx * nz), nx, nz, 1, conn)
        kept = np.unique(lab[near & c])
        got = s | (np.isin(lab, kept) & c)
        assert np.array_equal(got, K.mask_grow(s, c, nx, nz, -1, conn)), k


# ---- the argument checks and the ABI ------------------------------------------------------------------------
def test_checks_from_plain_cpp(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "rjp_args_regions_cases"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rajepy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rjp_args_regions_cases.cpp"), "-o", str(exe)], check=True)
    got = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        case, status, msg = line.split("\t")
        got[case] = (int(status), msg)
    want = {"stats_null": ["stats NULL d_img", "stats NULL d_stats", "stats NULL beats sizes"],
            "stats_size": ["stats n_maps 0", "stats nx -1", "stats sizes beat n_mask"],
            "stats_maps": ["stats n_maps 65536"], "stats_nx": ["stats nx 1048561"],
            "stats_pix": ["stats 2^31 pixels"], "stats_nmask": ["stats n_mask 2", "stats n_mask 0"],
            "stats_wgs": ["stats 2^31 workgroups"],
            "label_null": ["label NULL d_mask_in", "label NULL d_label", "label NULL d_nreg"],
            "label_size": ["label nz 0"], "label_maps": ["label n_maps 65536"], "label_nx": ["label nx 1048561"],
            "label_pix": ["label 2^31 pixels beat n_mask"],
            "label_nmask": ["label n_mask beats connectivity", "label n_mask 4"],
            "label_conn": ["label connectivity 0", "label connectivity 3"],
            "grow_null": ["grow NULL d_seed", "grow NULL d_con"], "grow_size": ["grow n_maps 0"],
            "grow_maps": ["grow n_maps 65536"], "grow_nx": ["grow nx 1048561"],
            "grow_pix": ["grow 2^31 pixels beat connectivity"],
            "grow_nmask": ["grow n_mask 2", "grow n_mask beats connectivity"],
            "grow_conn": ["grow connectivity 4"]}
    seen = set()
    for key, cases in want.items():
        for case in cases:
            assert got[case] == (_lib.RJP_ERR_ARG, K.MESSAGES[key]), case
            seen.add(case)
    valid = {c for c in got if " valid" in c}
    assert len(valid) == 9 and all(got[c] == (0, "") for c in valid)
    assert seen | valid == set(got)


def test_abi_signatures():
    P, i32, i64, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_size_t
    for name in ("rjp_image_stats", "rjp_label_regions", "rjp_mask_grow"):
        assert _lib.SIGNATURES[name + "_workspace"] == (sz, [i32, i32, i32])
    assert _lib.SIGNATURES["rjp_image_stats"] == (i64, [P, P, i32, i32, i32, P, i32, i32, P, P, sz, P])
    assert _lib.SIGNATURES["rjp_label_regions"] == (i64, [P, P, i32, i32, i32, i32, i32, P, P, P, P, sz, P])
    assert _lib.SIGNATURES["rjp_mask_grow"] == (i64, [P, P, P, i32, i32, i32, i32, i32, i32, P, sz, P])
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    assert "int64_t rjp_image_stats(rjp_ctx* ctx, const double* d_img, int32_t n_maps, int32_t nx, int32_t nz," in hdr
    assert "int64_t rjp_label_regions(rjp_ctx* ctx, const uint8_t* d_mask_in, int32_t n_mask, int32_t n_maps," in hdr
    assert "int64_t rjp_mask_grow(rjp_ctx* ctx, uint8_t* d_seed, const uint8_t* d_con, int32_t n_mask," in hdr
    assert "#define RJP_GROW_HALO 8" in hdr and "#define RJP_VERSION 117" in hdr    # symbols added, none changed
    assert K.HALO == 8
    lib = _lib.load()
    assert lib.rjp_image_stats(None, None, 1, 1, 1, None, 0, 1, None, None, 0, None) == _lib.RJP_ERR_ARG
    assert lib.rjp_label_regions(None, None, 1, 1, 1, 1, 1, None, None, None, None, 0, None) == _lib.RJP_ERR_ARG
    assert lib.rjp_mask_grow(None, None, None, 1, 1, 1, 1, 1, 1, None, 0, None) == _lib.RJP_ERR_ARG
    for args in ((1, 1, 1), (3, 67, 131), (2, 273, 241)):
        assert lib.rjp_image_stats_workspace(*args) == K.stats_workspace(*args)
        assert lib.rjp_label_regions_workspace(*args) == K.label_workspace(*args)
        assert lib.rjp_mask_grow_workspace(*args) == K.grow_workspace(*args)
    for q in (lib.rjp_image_stats_workspace, lib.rjp_label_regions_workspace, lib.rjp_mask_grow_workspace):
        assert q(0, 1, 1) == 0 and q(1, 65536, 32768) == 0 and q(65536, 1, 1) == 0


# ---- the automatic-mask convention ---------------------------------------------------------------------------
def test_automask_options_defaults_and_every_rejection():
    want = dict(sidelobe_threshold=3.0, noise_threshold=5.0, low_noise_threshold=1.5, min_beam_frac=0.3,
                grow_iterations=75, connectivity=1, nsigma=0.0)
    assert imaging.automask_options(True) == want == imaging.AUTOMASK_DEFAULTS == K.DEFAULTS
    assert imaging.automask_options(None) is None and imaging.automask_options(False) is None
    assert imaging.automask_options({}) == want
    got = imaging.automask_options(dict(noise_threshold=4, grow_iterations=-1, connectivity=2, nsigma=3))
    assert got == dict(want, noise_threshold=4.0, grow_iterations=-1, connectivity=2, nsigma=3.0)
    assert isinstance(got["noise_threshold"], float) and imaging.AUTOMASK_DEFAULTS == want
    assert E.automask_options is imaging.automask_options and E.automask_step is imaging.automask_step
    assert E.image_stats_results is imaging.image_stats_results
    for bad in ("auto", 1, [], dict(threshold=1.0), dict(sidelobe_threshold=-1.0), dict(noise_threshold=np.nan),
                dict(low_noise_threshold=np.inf), dict(min_beam_frac="0.3"), dict(nsigma=-0.5),
                dict(noise_threshold=True), dict(grow_iterations=7.5), dict(grow_iterations=True),
                dict(connectivity=3), dict(connectivity=0), dict(connectivity=True)):
        with pytest.raises(ValueError):
            imaging.automask_options(bad)


def test_image_stats_results_names_the_numbers():
    st = np.array([[4., 1., -1., 5., 1., 2., 8., 34.], [0., 3., np.nan, np.nan, np.nan, np.nan, 0., 0.],
                   [1., 0., 2., 2., 2., 0., 2., 4.]])
    a, b, c = imaging.image_stats_results(st)
    assert (a["npts"], a["min"], a["max"], a["median"], a["medabsdevmed"], a["sum"]) == (4, -1., 5., 1., 2., 8.)
    assert a["sigma_robust"] == 1.4826 * 2. and a["mean"] == 2. and a["rms"] == np.sqrt(34. / 4.)
    assert a["sigma"] == np.sqrt((34. - 8. * 8. / 4.) / 3.)
    assert b["npts"] == 0 and np.isnan(b["mean"]) and np.isnan(b["rms"]) and np.isnan(b["median"]) and b["sum"] == 0.
    assert c["npts"] == 1 and c["sigma"] == 0. and c["mean"] == 2.


import torch  # noqa: E402

from tests import test_msclean_reference_cpu as MS  # noqa: E402


class _Regions(MS._RecordingEngine):
    """The three K25 calls answered by the reference on CPU tensors, every call recorded; `clean`
    records the mask and the threshold it is given and finds nothing."""

    def image_stats(self, img, nx, nz, mask=None, inside=True):
        self.calls.append(dict(kind="stats", masked=mask is not None, inside=inside))
        x = img.numpy().reshape(-1, nx * nz)
        out = np.zeros((x.shape[0], 8))
        for m in range(x.shape[0]):
            mk = None if mask is None else mask.numpy().reshape(-1, nx * nz)[m if mask.shape[0] > 1 else 0]
            r = K.image_stats(x[m], mk, inside)
            out[m] = [r["count"], r["n_nonfinite"], r["min"], r["max"], r["median"], r["mad"], float(r["sum"]),
                      float(r["sumsq"])]
        return torch.from_numpy(out)

    def label_regions(self, mask, nx, nz, connectivity=1):
        self.calls.append(dict(kind="label", connectivity=connectivity))
        mk = mask.numpy().reshape(-1, nx * nz)
        res = [K.label_regions(m, nx, nz, connectivity) for m in mk]
        return (torch.from_numpy(np.stack([r[0] for r in res])), torch.from_numpy(np.stack([r[1] for r in res])),
                torch.tensor([r[2] for r in res], dtype=torch.int32))

    def mask_grow(self, seed, constraint, nx, nz, n_iter, connectivity=1):
        self.calls.append(dict(kind="grow", n_iter=n_iter, connectivity=connectivity))
        s, c = seed.numpy().reshape(-1, nx * nz), constraint.numpy().reshape(-1, nx * nz)
        return torch.from_numpy(np.stack([K.mask_grow(s[m], c[m if c.shape[0] > 1 else 0], nx, nz, n_iter,
                                                      connectivity) for m in range(s.shape[0])]).astype(np.uint8))

    def clean(self, res, nx, nz, psf, px, pz, n_iter, gain, thresh, mask=None, model=None):
        out = super().clean(res, nx, nz, psf, px, pz, n_iter, gain, thresh, mask=mask, model=model)
        self.calls[-1].update(maps=int(res.shape[0]), thresh=thresh,
                              mask=None if mask is None else (mask != 0).numpy().reshape(nx, nz).copy())
        return out

    def vis_components(self, cpix, cflux, ncomp, nx, nz, su, sv, u, v, cscale=None, n_s=1, gvis=None, vis_in=None,
                       sign=1):
        self.calls.append(dict(kind="viscomp"))
        return vis_in.clone()

    def components_image(self, cpix, cflux, ncomp, nx, nz, cscale=None, n_s=1):
        self.calls.append(dict(kind="compimg"))
        return torch.zeros(cpix.shape[0], nx * nz, dtype=torch.float64)


def _sky(ni, nj, M, seed=3):
    """Noise, a bright blob, a faint one-pixel spike above the high threshold and some NaN pixels."""
    rng = np.random.default_rng(seed)
    R = rng.standard_normal((M, ni, nj)) * 0.01
    x, z = np.arange(ni)[:, None], np.arange(nj)[None, :]
    for m in range(M):
        R[m] += (1.0 + m) * np.exp(-((x - 12 - m) ** 2 + (z - 20) ** 2) / 8.0)
        R[m, 30, 5 + m] = 0.2
        R[m, 0, :3] = np.nan
    return R.reshape(M, ni * nj)


def test_automask_step_on_a_recording_engine_equals_the_restatement():
    ni, nj, M = 40, 37, 3
    R = _sky(ni, nj, M)
    abc = [imaging.beam_quadratic(0.5, 0.3, 20. + m, 0.1 * np.pi / 180. / 3600.) for m in range(M)]
    side = np.array([0.05, 0.1, 0.2])
    um = np.zeros((ni, nj), dtype=bool)
    um[2:38, 3:35] = True
    prev = np.zeros((M, ni * nj), dtype=bool)
    prev[1, :200] = True
    for custom in ({}, dict(connectivity=2, grow_iterations=-1, min_beam_frac=0.0, sidelobe_threshold=2.0),
                   dict(grow_iterations=3, noise_threshold=20.0)):
        opts = imaging.automask_options(custom)
        eng = _Regions()
        masks, info = imaging.automask_step(eng, torch.from_numpy(R), torch.from_numpy(prev), torch.from_numpy(um),
                                            side, abc, opts, shape=(ni, nj))
        assert [c["kind"] for c in eng.calls] == ["stats", "stats", "label", "grow"]
        assert eng.calls[1]["masked"] and eng.calls[1]["inside"] is False and not eng.calls[0]["masked"]
        assert eng.calls[3]["n_iter"] == opts["grow_iterations"]
        want, winfo = K.automask_step(R, prev, um, side, abc, opts, ni, nj)
        assert masks.dtype == torch.uint8 and np.array_equal(masks.numpy() != 0, want)
        for m in range(M):
            assert set(info[m]) == set(winfo[m])
            for k in winfo[m]:
                assert np.float64(info[m][k]).tobytes() == np.float64(winfo[m][k]).tobytes(), (m, k)
        assert all(i["n_kept"] >= 1 for i in info) and (masks.numpy()[1, :200] != 0).all()
    # the defaults prune the one-pixel spike: a region is found and dropped
    opts = imaging.automask_options(True)
    _, info = imaging.automask_step(_Regions(), torch.from_numpy(R), None, None, np.zeros(M), abc, opts,
                                    shape=(ni, nj))
    assert all(i["n_regions"] > i["n_kept"] >= 1 for i in info)
    # a map in which nothing is left outside the mask takes its noise from all finite pixels
    full = np.ones((M, ni * nj), dtype=bool)
    m2, i2 = imaging.automask_step(_Regions(), torch.from_numpy(R), torch.from_numpy(full), None, side, abc, opts,
                                   shape=(ni, nj))
    w2, wi2 = K.automask_step(R, full, None, side, abc, opts, ni, nj)
    assert i2[0]["sigma"] == wi2[0]["sigma"] > 0 and (m2.numpy() != 0).all()


def _model(nx, nz):
    m = MS._model(nx, nz)
    m._engine = _Regions()
    return m


KW = dict(shape=(15, 13), beam=(0.1, 0.1, 0.), niter=2)
AM = dict(sidelobe_threshold=0.0, noise_threshold=0.5, low_noise_threshold=0.1, min_beam_frac=0.0)


def test_clean_images_without_the_keyword_makes_no_new_call():
    m = _model(6, 4)
    res = m.clean_image_ff(MS.U_M, MS.V_M, MS.FREQS, **KW)
    assert MS.kinds(m) == ["adjoint", "adjoint", "clean", "restore"] and res.automask is None
    m2 = _model(6, 4)
    res2 = m2.clean_image_ff(MS.U_M, MS.V_M, MS.FREQS, automask=None, **KW)
    assert MS.kinds(m2) == MS.kinds(m) and res2.image.tobytes() == res.image.tobytes() and res2.automask is None
    assert m2.engine.calls[2]["maps"] == 2 and m2.engine.calls[2]["mask"] is None
    m3 = _model(6, 4)
    m3.clean_image_ff(MS.U_M, MS.V_M, MS.FREQS, major_cycles=2, threshold_jy=1e-3, **KW)
    assert not {"stats", "label", "grow"} & set(MS.kinds(m3))
    assert all(c["maps"] == 2 for c in m3.engine.calls if c["kind"] == "clean")


def test_clean_images_with_the_keyword_one_clean_per_map_and_one_update_per_run():
    m = _model(6, 4)
    res = m.clean_image_ff(MS.U_M, MS.V_M, MS.FREQS, automask=AM, mask=(1, 13, 1, 11), **KW)
    assert MS.kinds(m) == ["adjoint", "adjoint", "stats", "stats", "label", "grow", "clean", "clean", "restore"]
    cl = [c for c in m.engine.calls if c["kind"] == "clean"]
    assert all(c["maps"] == 1 for c in cl)
    box = np.zeros((15, 13), dtype=bool)
    box[1:14, 1:12] = True
    assert len(res.automask) == 2
    for k, a in enumerate(res.automask):
        assert a["mask"].dtype == bool and a["mask"].shape == (15, 13) and a["mask"].any()
        assert not (a["mask"] & ~box).any(), "the automatic mask left the user's"
        assert np.array_equal(cl[k]["mask"], a["mask"]) and len(a["runs"]) == 1
        assert a["runs"][0]["n_mask"] == int(a["mask"].sum())
    # nsigma: the run's threshold is at least nsigma x the update's sigma
    m1 = _model(6, 4)
    r1 = m1.clean_image_ff(MS.U_M, MS.V_M, MS.FREQS, automask=dict(AM, nsigma=2.0), threshold_jy=1e-9, **KW)
    cl = [c for c in m1.engine.calls if c["kind"] == "clean"]
    assert [c["thresh"] for c in cl] == [max(1e-9, 2.0 * a["runs"][0]["sigma"]) for a in r1.automask]
    # with major cycles: one update at the top of every run, one clean per active map
    m2 = _model(6, 4)
    r2 = m2.clean_image_ff(MS.U_M, MS.V_M, MS.FREQS, automask=AM, major_cycles=2, threshold_jy=1e-3, **KW)
    kinds = MS.kinds(m2)
    assert kinds.count("stats") == 4 and kinds.count("label") == 2 and kinds.count("grow") == 2
    assert kinds.count("clean") == 4 and all(c["maps"] == 1 for c in m2.engine.calls if c["kind"] == "clean")
    assert len(r2.automask) == 2 and all(len(a["runs"]) == 2 for a in r2.automask)
    assert all("automask" not in d for d in r2.major) and len(r2.major) == 2
    for a in r2.automask:
        assert a["runs"][0]["n_mask"] <= a["runs"][1]["n_mask"] == int(a["mask"].sum())
    # mfs: one map, one call
    m3 = _model(6, 4)
    m3.clean_image_ff(MS.U_M, MS.V_M, MS.FREQS, automask=AM, mfs=True, **KW)
    assert MS.kinds(m3).count("clean") == 1
    for bad in (dict(scales=[0, 3]), dict(nterms=2, mfs=True), dict(automask="yes")):
        with pytest.raises(ValueError):
            _model(6, 4).clean_image_ff(MS.U_M, MS.V_M, np.array([4e9, 5e9]), **dict(dict(KW, automask=True), **bad))


def test_public_surface():
    J = classes.JetModel
    for fn in (J.clean_image_ff, J.clean_image_rrl, J.observe_ff, J.observe_rrl, imaging.Imager._clean_images,
               imaging.Imager._observe):
        p = inspect.signature(fn).parameters
        assert "automask" in p and p["automask"].default is None, fn.__qualname__
        names = list(p)
        assert names[names.index("automask") - 1] == "robust" and names[names.index("automask") + 1] == "scales"
    ex = inspect.signature(classes.Pipeline.execute).parameters
    assert "automask" not in ex and list(ex)[-3:] == ["antenna_configs", "sefd_jy", "seed"]
    assert list(inspect.signature(J.imstat).parameters) == ["self", "images", "mask", "inside"]
    p = inspect.signature(J.automask)
    assert list(p.parameters) == ["self", "images", "beam", "sidelobe", "mask", "prev", "options"]
    assert p.parameters["options"].kind is inspect.Parameter.VAR_KEYWORD
    assert list(inspect.signature(E.RTEngine.image_stats).parameters) == ["self", "img", "nx", "nz", "mask", "inside"]
    assert list(inspect.signature(E.RTEngine.label_regions).parameters) == ["self", "mask", "nx", "nz", "connectivity"]
    assert list(inspect.signature(E.RTEngine.mask_grow).parameters) == ["self", "seed", "constraint", "nx", "nz",
                                                                        "n_iter", "connectivity"]
    R = imaging.CleanResult
    r = R(1, 2, 3, 4, 5, 6)
    assert r.automask is None and R.automask is None and len(r) == 6
    r = R(1, 2, 3, 4, 5, 6, automask=[{"mask": 0}], imfit=["f"])
    assert r.automask == [{"mask": 0}] and r._replace(image=9).automask == [{"mask": 0}]
    assert r._replace(automask=None).automask is None and r._replace(automask=None).imfit == ["f"]
    assert R._make(range(6)).automask is None

    class _M(J):
        def __init__(self):
            self._engine, self._nx, self._nz, self._csize = _Regions(), 6, 4, 0.5
            self._params = {"target": {"dist": 120.}}
    m = _M()
    img = _sky(40, 37, 2).reshape(2, 40, 37)
    st = m.imstat(img)
    assert len(st) == 2 and st[0]["npts"] == 40 * 37 - 3 and st[0]["median"] == K.image_stats(img[0])["median"]
    inner = np.zeros((40, 37), dtype=bool)
    inner[5:, :] = True
    assert m.imstat(img[0], mask=inner, inside=False)[0]["npts"] == 5 * 37 - 3
    masks, info = m.automask(img, (0.5, 0.3, 20.), sidelobe=0.1, mask=inner, noise_threshold=4.0, min_beam_frac=0.0)
    assert masks.shape == (2, 40, 37) and masks.dtype == bool and masks.any() and not masks[:, :5].any()
    assert len(info) == 2 and info[0]["n_kept"] >= 1
    with pytest.raises(ValueError):
        m.automask(img, (0.5, 0.3, 20.), threshold=1.0)
