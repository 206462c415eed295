"""tests/vis_components_ref.py, the reference rjp_vis_components (K18) and rjp_components_image are
held to on the device (tests/test_gpu_vis_components.py), pinned without a GPU: a delta at the centre,
K10's own reference on the list's image, a float64 emulation of the device's stated order inside
the derived bound and four planted mistakes outside it, the delta model against a sequential sum
and against the model a reference CLEAN builds; the argument checks driven from plain C++; the
header, the binding and the ABI version."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np

from rajepy_amd import _lib
from tests import clean_ref as C
from tests import vis_components_ref as R
from tests import vis_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble


def test_a_delta_at_the_centre_gives_its_flux():
    """On an odd grid the centre pixel has jx = jz = 0: V = f at every baseline, sign and `in`
    included; ncomp = 0 returns `in`; a non-finite baseline gives NaN there alone."""
    nx, nz = 7, 5
    p = np.array([(nx // 2) * nz + nz // 2], dtype=np.int32)
    f = np.array([0.75])
    a, b = np.array([0.0, 0.3, -8.0, np.nan]), np.array([0.0, -0.2, 3.5, 0.1])
    out, S = R.vis_components_ref(p, f, None, 1, nx, nz, a, b)
    assert np.all(out[:3] == 0.75) and np.isnan(complex(out[3]).real) and np.all(S == 0.75)
    vin = np.array([1 + 2j, -0.0 + 0j, 3j, 1.0])
    out, S = R.vis_components_ref(p, f, None, 1, nx, nz, a, b, vin=vin, sign=-1)
    assert np.all(out[:3] == vin[:3] - 0.75) and np.allclose(S, np.abs(vin) + 0.75)
    out, _ = R.vis_components_ref(p, f, None, 0, nx, nz, a[:3], b[:3], vin=vin[:3])
    assert np.all(out == vin[:3])


def test_agrees_with_k10s_reference_on_the_lists_image():
    """The list's visibilities are the transform of the list's delta image: tests/vis_ref.py on
    components_image_ref, both in long double."""
    rng = np.random.default_rng(3)
    for nx, nz in R.SHAPES:
        for n in (1, 65, 300):
            p, f, _ = R.random_list(rng, nx, nz, n)
            a, b = VR.random_points(rng, 17, 0.5)
            img = R.components_image_ref(p, f, None, n, nx, nz)[0].reshape(nx, nz)
            out, S = R.vis_components_ref(p, f, None, n, nx, nz, a, b)
            want = VR.vis_ref(img, a, b)
            # (the image sums duplicated pixels in float64 first: n u of sum |f|)
            assert np.all(np.abs(out - want).astype(np.float64) <= (n + 4) * R.U * S)


def _case(rng, nx, nz, n, n_s, K, amax):
    p, f, s = R.random_list(rng, nx, nz, n, n_s)
    a, b = VR.random_points(rng, K, amax)
    G = R.random_g(rng, n_s, K) if n_s > 1 else None
    vin = rng.standard_normal(K) + 1j * rng.standard_normal(K)
    return p, f, (s if n_s > 1 else None), a, b, G, vin


def test_the_emulated_order_lies_inside_the_bound_and_planted_mistakes_outside():
    rng = np.random.default_rng(11)
    worst = 0.0
    for (nx, nz), n, n_s, amax in (((5, 3), 65, 1, 0.5), ((67, 131), 300, 3, 0.5),
                                   ((67, 131), 1000, 1, 8.0), ((67, 131), 257, 3, 8.0)):
        K = 9
        p, f, s, a, b, G, vin = _case(rng, nx, nz, n, n_s, K, amax)
        ref, S = R.vis_components_ref(p, f, s, n, nx, nz, a, b, n_s, G, vin, -1)
        bnd = R.bound(a, b, nx, nz, n, n_s)
        emu = lambda **kw: R.vis_components_emulated(p, f, s, n, nx, nz, a, b, n_s, G, vin, -1, **kw)
        r = R.worst_ratio(emu(), ref, S, bnd)
        worst = max(worst, r)
        assert r <= 1.0, (nx, nz, n, n_s, r)
        # (the zero spacing sees no phase: the first three mistakes are judged off it)
        off = slice(1, None)
        for kw in (dict(centre_shift=0.5), dict(phase_sign=1.0), dict(phasor_dtype=np.float32)):
            r = R.worst_ratio(emu(**kw)[off], ref[off], S[off], bnd[off])
            assert r > 10.0, (kw, r)
        if n_s > 1:
            r = R.worst_ratio(emu(g_shift=1), ref, S, bnd)
            assert r > 10.0, ("G of the wrong scale", r)
    print("emulation: worst |got - ref| / bound = %.3f" % worst)
    assert worst > 1e-3, "the bound is not vacuous"


def test_components_that_add_nothing():
    """A NaN or infinite flux, a pixel outside [0, nx nz), a scale outside [0, n_s): dropped by the
    visibilities and by the image alike; ncomp is clamped into [0, stride]."""
    nx, nz, n_s = 5, 3, 2
    p = np.array([7, 7, -1, 15, 2, 3, 4], dtype=np.int32)
    f = np.array([1.0, np.nan, 2.0, 4.0, np.inf, 8.0, 16.0])
    s = np.array([0, 0, 0, 0, 1, 2, -1], dtype=np.int32)
    pv, fv, sv, idx = R.valid(p, f, s, 7, nx, nz, n_s)
    assert list(idx) == [0] and list(fv) == [1.0]
    img = R.components_image_ref(p, f, s, 7, nx, nz, n_s)
    assert img.sum() == 1.0 and img[0, 7] == 1.0
    assert R.clamp(-3, 7) == 0 and R.clamp(9, 7) == 7 and R.clamp(4, 7) == 4


def test_components_image_is_the_sequential_sum_and_a_cleans_model():
    rng = np.random.default_rng(5)
    nx, nz, n_s, n = 9, 7, 3, 400
    p, f, s = R.random_list(rng, nx, nz, n, n_s, dup_share=0.6)
    img = R.components_image_ref(p, f, s, n, nx, nz, n_s)
    for sc in range(n_s):
        for q in range(nx * nz):
            acc = 0.0
            for c in range(n):
                if p[c] == q and s[c] == sc:
                    acc += f[c]
            assert img[sc, q].tobytes() == np.float64(acc).tobytes()
    # order matters in float64, so "in list order" is a real statement
    assert not np.array_equal(img, R.components_image_ref(p[::-1], f[::-1], s[::-1], n, nx, nz, n_s))
    # the model a CLEAN adds up as it goes (model[p] += f from zeros) is this image
    B = C.random_beam(rng, 2 * nx - 1, 2 * nz - 1)
    D = C.random_image(rng, nx, nz, B)
    cp, cf, _ = C.hogbom(D, B, None, 1e-3, 0.3, 200, dtype=np.float64)
    model = np.zeros(nx * nz)
    for pc, fc in zip(cp, cf):
        model[pc] += fc
    assert len(cp) > 20 and len(set(cp.tolist())) < len(cp)
    assert np.array_equal(R.components_image_ref(cp, cf, None, len(cp), nx, nz)[0], model)


def test_grid_rules():
    assert R.workgroups(1, 1) == 1 and R.workgroups(1, 64) == 1 and R.workgroups(3, 65) == 6
    assert R.image_workgroups(1, 1, 1, 1) == 1 and R.image_workgroups(2, 3, 67, 131) == 6 * 35
    assert R.bound(0.0, 0.0, 1, 1, 0) == R.bound(0.0, 0.0, 1, 1, 256) < R.bound(0.0, 0.0, 1, 1, 257)


def test_abi_signatures_and_header():
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    P, i32, DP = ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_double)

    def names(fn):
        decl = re.search(r"int64_t %s\((.*?)\);" % fn, hdr, re.S).group(1)
        return [re.search(r"(\w+)$", p.strip()).group(1) for p in decl.split(",")]

    assert names("rjp_vis_components") == [
        "ctx", "d_cpix", "d_cscale", "d_cflux", "d_ncomp", "n_maps", "comp_stride", "n_s", "nx", "nz",
        "h_su", "h_sv", "d_u", "d_v", "n_vis", "d_gvis", "d_in", "sign", "d_out", "stream"]
    assert names("rjp_components_image") == [
        "ctx", "d_cpix", "d_cscale", "d_cflux", "d_ncomp", "n_maps", "comp_stride", "n_s", "nx", "nz",
        "d_out", "stream"]
    assert "#define RJP_VERSION 117" in hdr and _lib.RJP_VERSION == 117
    assert "casa/tasks.py:259-262" in hdr
    assert _lib.SIGNATURES["rjp_vis_components"] == (
        ctypes.c_int64, [P, P, P, P, P, i32, i32, i32, i32, i32, DP, DP, P, P, i32, P, P, i32, P, P])
    assert _lib.SIGNATURES["rjp_components_image"] == (
        ctypes.c_int64, [P, P, P, P, P, i32, i32, i32, i32, i32, P, P])
    lib = _lib.load()
    assert lib.rjp_version() == 117
    for name in ("rjp_vis_components", "rjp_components_image"):
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    mk = open(os.path.join(ROOT, "rajepy_amd", "csrc", "Makefile")).read()
    assert "$(OBJDIR)/vis_components.o" in mk
    # a NULL context is refused before anything else
    assert lib.rjp_vis_components(None, None, None, None, None, 1, 1, 1, 1, 1, None, None, None, None,
                                  1, None, None, 1, None, None) == _lib.RJP_ERR_ARG
    assert lib.rjp_components_image(None, None, None, None, None, 1, 1, 1, 1, 1, None,
                                    None) == _lib.RJP_ERR_ARG


def test_engine_methods():
    from rajepy_amd import engine as E
    p = inspect.signature(E.RTEngine.vis_components).parameters
    assert list(p) == ["self", "cpix", "cflux", "ncomp", "nx", "nz", "su", "sv", "u", "v", "cscale", "n_s",
                       "gvis", "vis_in", "sign", "out"]
    assert p["cscale"].default is None and p["n_s"].default == 1 and p["sign"].default == 1
    p = inspect.signature(E.RTEngine.components_image).parameters
    assert list(p) == ["self", "cpix", "cflux", "ncomp", "nx", "nz", "cscale", "n_s"]


def test_checks_from_plain_cpp(tmp_path):
    """check_vis_components and check_components_image compiled into a stand-alone program by plain
    g++ (tests/rjp_args_viscomp_cases.cpp): every refusal, status and message, in the order the
    checks make them -- the messages tests/test_gpu_vis_components.py sees from the library."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "rjp_args_viscomp_cases"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rajepy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rjp_args_viscomp_cases.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {}
    for line in out.splitlines():
        case, status, msg = line.split("\t")
        got[case] = (int(status), msg)
    want = {"null": ["NULL d_cpix", "NULL d_cflux", "NULL d_ncomp", "NULL h_su", "NULL h_sv", "NULL d_u",
                     "NULL d_v", "NULL d_out", "NULL beats sizes"],
            "sizes": ["n_maps 0", "comp_stride 0", "n_s 0", "nx 0", "nz -1", "n_vis 0", "sizes beat sign"],
            "sign": ["sign 0", "sign 2", "sign beats gvis"],
            "gvis": ["NULL d_gvis n_s 3", "gvis beats scales"],
            "scales": ["su nan", "sv inf", "scales beat the image size"],
            "npix": ["nx nz 2^31", "image size beats workgroups"],
            "wgs": ["workgroups"],
            "img_null": ["img NULL d_cpix", "img NULL d_cflux", "img NULL d_ncomp", "img NULL d_out",
                         "img NULL beats sizes"],
            "img_sizes": ["img n_maps 0", "img comp_stride -2", "img n_s 0", "img nx 0", "img nz 0",
                          "img sizes first"],
            "img_npix": ["img nx nz 2^31"],
            "img_wgs": ["img workgroups"]}
    seen = set()
    for key, cases in want.items():
        for case in cases:
            assert got[case] == (_lib.RJP_ERR_ARG, R.MSG[key]), case
            seen.add(case)
    valid = {c for c in got if c not in seen}
    assert valid == {"valid", "valid sign +1", "valid hogbom", "valid 1", "valid 63 x 2^25 workgroups",
                     "img valid", "img valid 1"}
    assert all(got[c] == (0, "") for c in valid)
