"""Host-side logic that needs no GPU: parameter handling, run tables, file names, the FITS
writer (byte-for-byte against the reference's astropy output), scalar maths, the ABI."""
import copy
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest

from rajepy_amd import _constants as con
from rajepy_amd import _lib, classes, fits, logger
from rajepy_amd.maths import geometry as mgeom, physics as mphys, rrls as mrrl
from rajepy_amd.miscellaneous import functions as miscf
from tests import gpu_util as U

GOLDEN = U.GOLDEN
ROOT = os.path.dirname(GOLDEN.rstrip(os.sep).rsplit(os.sep, 1)[0])


@pytest.fixture()
def rec():
    return json.load(open(os.path.join(GOLDEN, "pipeline_cfg1.json")))


def example_params():
    p = copy.deepcopy(U.load_golden("cfg1_example")[2])
    for k in ("mod_r_0",):
        p["geometry"].pop(k, None)
    for k in ("q_n", "q_tau"):
        p["power_laws"].pop(k, None)
    p["properties"].pop("n_0", None)
    return p


def make_model(tmp_path, params=None):
    log = logger.Log(str(tmp_path / "m.log"), verbose=False)
    return classes.JetModel(params or example_params(), log=log)


# ---- C-ABI ---------------------------------------------------------------------------
def test_abi_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    declared = set(re.findall(r"\b(rjp_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    lib = _lib.load()                       # raises if the .so or any symbol is missing
    # header, library and binding agree on the ABI version
    assert int(re.search(r"#define RJP_VERSION (\d+)", hdr).group(1)) == _lib.RJP_VERSION
    assert lib.rjp_version() == _lib.RJP_VERSION
    for name in declared:
        assert hasattr(lib, name)


_ABI_STRUCTS = {"rjp_fields": "Fields", "rjp_bursts": "Bursts", "rjp_line": "Line",
                "rjp_geometry": "Geometry"}


def _header_struct_members(hdr):
    """{struct name: [member names in declaration order]} parsed from include/rjprt.h."""
    out = {}
    for m in re.finditer(r"typedef struct (rjp_\w+) \{(.*?)\}\s*\1;", hdr, re.S):
        body = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
        names = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            # "const void* d_nd" / "int32_t nx, ny, nz" / "const double* t0[2]"
            first, *rest = decl.split(",")
            names.append(re.search(r"(\w+)\s*(\[\d+\])?$", first.strip()).group(1))
            names += [re.search(r"(\w+)", r).group(1) for r in rest]
        out[m.group(1)] = names
    return out


def _compiled_layouts(tmp_path):
    """sizeof / offsetof / member size of every struct of include/rjprt.h as the C++ compiler
    lays them out: a small program generated from the HEADER's member list, built with g++."""
    import shutil
    import subprocess
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    members = _header_struct_members(hdr)
    assert set(members) == set(_ABI_STRUCTS), members.keys()
    lines = ['#include <cstdio>', '#include <cstddef>', '#include "rjprt.h"', "int main() {",
             '  std::printf("{\\"version\\": %d", RJP_VERSION);']
    for st, names in members.items():
        lines.append('  std::printf(", \\"%s\\": {\\"sizeof\\": %%zu, \\"members\\": ["'
                     ', sizeof(%s));' % (st, st))
        for i, nm in enumerate(names):
            lines.append('  std::printf("%s[\\"%s\\", %%zu, %%zu]", offsetof(%s, %s), '
                         'sizeof(((%s*)0)->%s));' % (", " if i else "", nm, st, nm, st, nm))
        lines.append('  std::printf("]}");')
    lines += ['  std::printf("}\\n");', "  return 0;", "}"]
    src = tmp_path / "abi_layout.cpp"
    src.write_text("\n".join(lines))
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("hipcc")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "abi_layout"
    subprocess.run([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True)
    return json.loads(subprocess.run([str(exe)], check=True, capture_output=True,
                                     text=True).stdout)


def _ctypes_layout(cls):
    return [[n, getattr(cls, n).offset, getattr(cls, n).size] for n, _ in cls._fields_]


def test_abi_struct_layouts_match_header_as_compiled(tmp_path):
    """The ctypes structs of rajepy_amd/_lib.py against include/rjprt.h AS COMPILED: a C++
    program generated from the header's own member list prints sizeof / offsetof / member
    sizes; every member, in order, must sit where ctypes puts it (a member added to the header
    and not to the binding -- or the reverse -- fails here, not on the GPU)."""
    comp = _compiled_layouts(tmp_path)
    assert comp["version"] == _lib.RJP_VERSION
    for st, cname in _ABI_STRUCTS.items():
        cls = getattr(_lib, cname)
        assert comp[st]["sizeof"] == ctypes.sizeof(cls), st
        assert comp[st]["members"] == _ctypes_layout(cls), st


def test_last_scan_tiles_prototype_as_compiled_and_null_refusals(tmp_path):
    """rjp_last_scan_tiles as the C++ compiler reads include/rjprt.h -- a function pointer of the
    documented type takes its address -- against the binding's argtypes; and the refusals that need
    no context: a NULL context or a NULL count is RJP_ERR_ARG, nothing is written."""
    import shutil
    import subprocess
    src = tmp_path / "proto.cpp"
    src.write_text('#include "rjprt.h"\n'
                   "int (*const fp)(const rjp_ctx*, int32_t*, int32_t*, int32_t) = "
                   "&rjp_last_scan_tiles;\n"
                   "int (*const fq)(const rjp_ctx*, double*, int32_t*) = &rjp_last_scan_path;\n"
                   "int main() { return fp && fq ? 0 : 1; }\n")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("hipcc")
    assert cxx, "no C++ compiler"
    subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    str(src)], check=True)
    res, args = _lib.SIGNATURES["rjp_last_scan_tiles"]
    i32p = ctypes.POINTER(ctypes.c_int32)
    assert res is ctypes.c_int and args == [ctypes.c_void_p, i32p, i32p, ctypes.c_int32]
    hdr = open(os.path.join(ROOT, "include", "rjprt.h")).read()
    decl = hdr[:hdr.index("int rjp_last_scan_tiles(")]
    assert decl.rstrip().endswith("For tests. */")               # beside rjp_last_scan_path's wording
    lib = _lib.load()
    n = ctypes.c_int32(-5)
    buf = (ctypes.c_int32 * 5)(*([-7] * 5))
    assert lib.rjp_last_scan_tiles(None, ctypes.byref(n), buf, 1) == _lib.RJP_ERR_ARG
    assert n.value == -5 and list(buf) == [-7] * 5


def _integration_md_binding():
    """exec()s the ctypes stub printed in INTEGRATION.md (section B, `RaJePy/_rjprt.py`) with
    the CDLL call replaced by a recorder; returns (namespace, recorder)."""
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    blocks = re.findall(r"```python\n(.*?)```", md, re.S)
    stub = [b for b in blocks if "RaJePy/_rjprt.py" in b]
    assert len(stub) == 1

    class _Fn:
        argtypes = None
        restype = ctypes.c_int

    class _Recorder:
        def __init__(self):
            self.fns = {}

        def __getattr__(self, name):
            if name.startswith("rjp_"):
                return self.fns.setdefault(name, _Fn())
            raise AttributeError(name)

    rec = _Recorder()
    rec.fns["rjp_version"] = lambda: _lib.RJP_VERSION
    code = stub[0].replace('C.CDLL("librjprt.so")', "_RECORDER")
    assert "_RECORDER" in code
    ns = {"_RECORDER": rec}
    exec(compile(code, "INTEGRATION.md", "exec"), ns)
    return ns, rec


def test_integration_md_binding_matches_the_abi():
    """The reference-side stub a maintainer would paste from INTEGRATION.md is executed and
    compared with the binding the tests run through: struct members, types, offsets, sizes,
    the ABI version it asserts, and every prototype it declares."""
    ns, rec = _integration_md_binding()
    seen = 0
    for cname in _ABI_STRUCTS.values():
        if cname not in ns:
            continue
        seen += 1
        doc, ours = ns[cname], getattr(_lib, cname)
        assert ctypes.sizeof(doc) == ctypes.sizeof(ours), cname
        assert _ctypes_layout(doc) == _ctypes_layout(ours), cname
    assert seen >= 2 and "Fields" in ns and "Bursts" in ns
    declared = {k: v for k, v in rec.fns.items() if k != "rjp_version"}
    assert len(declared) >= 6

    def norm(t):
        # the stub's own Fields / Bursts classes are distinct Python types: compare by layout
        if hasattr(t, "_type_") and hasattr(t._type_, "_fields_"):
            return ("ptr", tuple(map(tuple, _ctypes_layout(t._type_))))
        return t
    for name, fn in declared.items():
        res, args = _lib.SIGNATURES[name]                   # KeyError: not an entry point
        if fn.argtypes is not None:
            assert [norm(a) for a in fn.argtypes] == [norm(a) for a in args], name
        assert fn.restype is res, name


def test_workspace_queries_are_host_arithmetic():
    """The workspace sizes are plain host arithmetic of the launcher's tiling rules (no GPU):
    one plane set per y-range, 2 E + 2 planes per set; tiles of >= 16 epochs are cut into 4x
    the y-ranges of the HBM-bound scans while their partial sums stay below 6 GiB."""
    lib = _lib.load()
    npix = 512 * 512
    # worst case over the lane widths the launcher may pick: 4 sightlines per lane (f32
    # storage) leave a quarter of the lanes, hence 16 y-ranges where 2-wide f64 lanes take 8
    one = lib.rjp_ff_scan_workspace(512, 4096, 512, 1)
    assert one == 16 * (2 * 1 + 2) * npix * 8 + 256
    eight = lib.rjp_ff_scan_workspace(512, 4096, 512, 8)
    assert eight == 16 * (2 * 8 + 2) * npix * 8 + 256
    tile32 = lib.rjp_ff_scan_workspace(512, 4096, 512, 32)
    assert tile32 == 32 * (2 * 32 + 2) * npix * 8 + 256            # 32 y-ranges of 128 rows
    assert lib.rjp_ff_scan_workspace(512, 4096, 512, 1000) == tile32   # tiles never exceed 32
    # 4x the sightlines: 32 ranges of a 32-epoch tile would need 17.7 GB -> halved until < 6 GiB
    big = lib.rjp_ff_scan_workspace(1024, 4096, 1024, 32)
    assert big == 16 * (2 * 16 + 2) * 4 * npix * 8 + 256           # its 16-epoch tiles decide
    # sweeps of >= 12 epochs may take the moment path: up to 1280 moments per sightline (+ on
    # maps of fewer than 4096 waves the chunk sums of the split contraction: 16 x 32 planes here)
    assert lib.rjp_ff_scan_workspace(64, 128, 64, 12) == (1280 + 16 * 32) * 64 * 64 * 8 + 256
    assert lib.rjp_ff_scan_workspace(512, 4096, 512, 12) >= 1280 * npix * 8 + 256
    assert lib.rjp_ff_scan_workspace(64, 128, 64, 11) < 1024 * 64 * 64 * 8
    assert lib.rjp_ff_scan_workspace(0, 4, 4, 1) == 0
    # round 5: the single-epoch table scan cuts mid-size maps into its OWN y-ranges
    # (until 512 workgroups exist, >= 64 rows each) -- 4 planes per range -- and the scan of the
    # five model fields keeps its table behind 8 x 4 planes: both inside the workspace now
    p2 = 256 * 256
    assert lib.rjp_ff_scan_workspace(256, 128, 256, 1) >= max(2 * 4 * p2 * 8, 32 * p2 * 8 + 73600)
    assert lib.rjp_ff_scan_workspace(256, 256, 256, 1) >= max(4 * 4 * p2 * 8, 32 * p2 * 8 + 73600)
    assert lib.rjp_ff_scan_workspace(100, 400, 700, 1) >= 32 * 70000 * 8 + 73600
    assert lib.rjp_ff_scan_workspace(64, 4096, 512, 1) >= 8 * 4 * 64 * 512 * 8     # an x-slab of cfg4
    assert lib.rjp_ff_maps_workspace(npix, 1, 256) > 0
    assert lib.rjp_ff_maps_workspace(0, 1, 1) == 0


def test_no_gpu_fails_loudly_not_silently():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from rajepy_amd.engine import RTEngine
    with pytest.raises(_lib.RjprtError):
        RTEngine(0)
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    assert lib.rjp_ctx_create(0, ctypes.byref(ctx)) < 0
    assert b"device" in lib.rjp_last_error(None).lower()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "rajepy_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".sh")):
                txt = open(os.path.join(dirpath, fn)).read()
                assert "oracle" not in txt.replace("# oracle", ""), fn


# ---- Pipeline epoch batching -----------------------------------------------------------
@pytest.mark.parametrize("n_times, n_freqs", [(100, 1), (33, 2), (5, 3)])
def test_pipeline_prefetches_each_epoch_once_in_chunks_of_32(tmp_path, n_times, n_freqs):
    """Pipeline.execute hands the epochs still to come to JetModel.prefetch_epochs 32 at a
    time -- one pass over HBM per chunk: ceil(N / 32) scans for N epochs, every epoch in
    exactly one chunk, in run order (the reference scans the grid once per run and channel,
    classes.py:2358-2453).  No GPU: the device calls are replaced by recorders."""
    jm = make_model(tmp_path)
    times = [round(0.05 * i, 4) for i in range(n_times)]
    freqs = [1e9 * (k + 1) for k in range(n_freqs)]
    pp = {"min_el": 20., "dcys": {"model_dcy": str(tmp_path / "run")},
          "continuum": {"times": np.array(times), "freqs": np.array(freqs),
                        "t_obs": np.array([1200] * n_freqs),
                        "tscps": np.array([("VLA", "A")] * n_freqs),
                        "t_ints": np.array([5] * n_freqs), "bws": np.array([1e8] * n_freqs),
                        "chanws": np.array([1e8] * n_freqs)},
          "rrls": {"times": None, "lines": np.array([]), "t_obs": np.array([]),
                   "tscps": np.array([]), "t_ints": np.array([]), "bws": np.array([]),
                   "chanws": np.array([])}}
    pl = classes.Pipeline(jm, pp, log=jm.log)
    chunks, served = [], []
    jm.prefetch_epochs = lambda ts: chunks.append([float(t) for t in ts])
    pl._radiative_transfer = lambda idx, run, clobber: served.append(float(jm.time))
    jm.save = lambda f: None
    pl.execute(simobserve=False, verbose=False, resume=False)
    assert len(served) == n_times * n_freqs
    assert len(chunks) == -(-n_times // 32)
    assert all(len(c) <= 32 for c in chunks)
    flat = [t for c in chunks for t in c]
    assert flat == [t * con.year for t in times]            # each epoch once, in run order
    # every run found its epoch in a chunk prefetched before it was served
    seen = set()
    it = iter(chunks)
    for t in served:
        if t not in seen:
            seen.update(next(it))
        assert t in seen


# ---- JetModel host behaviour ---------------------------------------------------------
def test_jetmodel_derived_params_and_str(tmp_path, rec):
    jm = make_model(tmp_path)
    ref = U.load_golden("cfg1_example")[1]["params"]
    assert (jm.nx, jm.ny, jm.nz) == (50, 400, 50)
    assert jm.params["geometry"]["mod_r_0"] == pytest.approx(ref["geometry"]["mod_r_0"], rel=1e-15)
    assert jm.params["power_laws"]["q_n"] == pytest.approx(ref["power_laws"]["q_n"], rel=1e-15)
    assert jm.params["power_laws"]["q_tau"] == pytest.approx(ref["power_laws"]["q_tau"], rel=1e-15)
    assert jm.params["properties"]["n_0"] == pytest.approx(ref["properties"]["n_0"], rel=1e-14)
    assert str(jm) == rec["jetmodel_str"]
    assert len(jm.ejections) == 5            # "RB" registers one burst per jet
    assert jm.gff_mode == _lib.RJP_GFF_SCALAR


@pytest.mark.parametrize("tag", ["cfg1_example", "tilted"])
def test_geometry_accessors_match_reference(tmp_path, tag):
    """rr / ww / pp / rreff grids (host side) against the reference's at the jet cells."""
    z, meta, p = U.load_golden(tag)
    p["geometry"].pop("mod_r_0", None)
    p["power_laws"].pop("q_n", None), p["power_laws"].pop("q_tau", None)
    p["properties"].pop("n_0", None)
    jm = make_model(tmp_path, p)
    idx = z["f_idx"]
    with np.errstate(all="ignore"):
        for name, key in (("rr", "rr"), ("ww", "ww"), ("pp", "pp"), ("rreff", "rreff")):
            got = getattr(jm, name).ravel()[idx]
            np.testing.assert_allclose(got, z["f_" + key], rtol=1e-12, atol=1e-12, err_msg=name)
    assert jm.xx.shape == (jm.nx, jm.ny, jm.nz) and jm.xs[0] == -jm.csize * (jm.nx // 2)
    assert np.array_equal(jm.zz[0, 0], jm.zs)


def test_jetmodel_errors(tmp_path):
    with pytest.raises(TypeError):
        classes.JetModel(42)
    with pytest.raises(FileNotFoundError):
        classes.JetModel(str(tmp_path / "missing.py"))
    jm = make_model(tmp_path)
    with pytest.raises(ValueError):
        jm._rrl_flux("H66a", 2.2e10, lte=False, contsub=True)
    with pytest.raises(ValueError):
        jm.save_fits(np.zeros((2, 2)), str(tmp_path / "x.fits"), "nonsense")


def test_param_file_surface(tmp_path):
    """A params FILE like the reference's example (no `n_0`, l_z set) loads; a broken one
    raises the validator's error."""
    src = tmp_path / "example-model-params.py"
    p = example_params()
    body = "import numpy as np\nparams = " + repr(
        {k: {kk: (vv.tolist() if isinstance(vv, np.ndarray) else vv) for kk, vv in v.items()}
         for k, v in p.items()})
    body = body.replace("'t_0': [", "'t_0': np.array([").replace("'hl': [", "'hl': np.array([")
    body = body.replace("'chi': [", "'chi': np.array([").replace("'which': [", "'which': np.array([")
    body = re.sub(r"(np\.array\(\[[^\]]*\])", r"\1)", body)
    src.write_text(body)
    (tmp_path / "log").mkdir()
    jm = classes.JetModel(str(src), log=logger.Log(str(tmp_path / "log" / "a.log"), verbose=False))
    assert (jm.nx, jm.ny, jm.nz) == (50, 400, 50)
    bad = tmp_path / "bad.py"
    bad.write_text(body.replace("'epsilon'", "'epsilonX'"))
    with pytest.raises(KeyError):
        classes.JetModel(str(bad))


def test_lz_overrides_grid_and_burstless_table(tmp_path):
    ref = json.load(open(os.path.join(GOLDEN, "scalars.json")))
    p = example_params()
    p["grid"]["l_z"] = 2.
    jm = make_model(tmp_path, p)
    assert [jm.nx, jm.ny, jm.nz] == ref["lz_grid_dims"] == [108, 110, 588]   # SURVEY finding 4
    p = example_params()
    p["ejection"] = {k: np.array([]) for k in ("t_0", "hl", "chi", "which")}
    jm = make_model(tmp_path, p)
    assert str(jm) == ref["jetmodel_str_no_bursts"]
    assert jm.ejections == {} and jm._rjp_bursts().n[0] == 0


def test_validators_return_exceptions():
    assert isinstance(miscf.check_model_params([]), TypeError)
    p = example_params()
    assert miscf.check_model_params(p) is None            # n_0 optional (documented leniency)
    q = copy.deepcopy(p)
    q["target"]["ra"] = "nonsense"
    assert isinstance(miscf.check_model_params(q), ValueError)
    q = copy.deepcopy(p)
    q["grid"]["n_x"] = 5.5
    assert isinstance(miscf.check_model_params(q), ValueError)
    q = copy.deepcopy(p)
    del q["ejection"]
    assert isinstance(miscf.check_model_params(q), KeyError)
    assert isinstance(miscf.check_pline_params({"min_el": 20.}), KeyError)


# ---- runs / pipeline table -------------------------------------------------------------
def pline_params(dcy):
    return {
        "min_el": 20., "dcys": {"model_dcy": dcy},
        "continuum": {"times": np.array([0., 1.]), "freqs": np.array([5.]) * 1e9,
                      "t_obs": np.array([1200]), "tscps": np.array([("VLA", "A")]),
                      "t_ints": np.array([5]), "bws": np.array([4e8]), "chanws": np.array([2e8])},
        "rrls": {"times": np.array([0.]), "lines": np.array(["H66a"]),
                 "t_obs": np.array([1200]), "tscps": np.array([("VLA", "A")]),
                 "t_ints": np.array([60]), "bws": np.array([4e5]), "chanws": np.array([1e5])},
    }


def test_pipeline_save_keeps_the_runs_where_they_are(tmp_path, monkeypatch):
    """A save without absolute_directories writes '~' for the home directory into the FILE
    (the reference's portable form) but leaves the pipeline's own runs and parameters alone:
    a run under the home directory still names its products by their real paths."""
    import pickle
    monkeypatch.setenv("HOME", str(tmp_path))
    dcy = str(tmp_path / "out")
    os.makedirs(dcy)
    log = logger.Log(os.path.join(dcy, "model.log"), verbose=False)
    jm = classes.JetModel(example_params(), log=log)
    pl = classes.Pipeline(jm, pline_params(dcy), log=log)
    before = [(r.dcy, r.fits_flux) for r in pl.runs]
    jm.save(pl.model_file)
    pl.save(pl.save_file)
    assert [(r.dcy, r.fits_flux) for r in pl.runs] == before
    assert all(p.startswith(dcy) for _, p in before)
    assert pl.params["dcys"]["model_dcy"] == dcy
    saved = pickle.load(open(pl.save_file, "rb"))
    assert all(r.dcy == "~/out" for r in saved["runs"])
    assert saved["params"]["dcys"]["model_dcy"] == "~/out"
    assert saved["model_file"] == "~/out/jetmodel.save"
    back = classes.Pipeline.load_pipeline(pl.save_file)
    assert [(r.dcy, r.fits_flux) for r in back.runs] == before


def test_pipeline_run_table_matches_reference(tmp_path, rec):
    dcy = str(tmp_path / "out")
    os.makedirs(dcy)
    log = logger.Log(os.path.join(dcy, "model.log"), verbose=False)
    jm = classes.JetModel(example_params(), log=log)
    pl = classes.Pipeline(jm, pline_params(dcy), log=log)
    assert len(pl.runs) == len(rec["runs"])
    for run, ref in zip(pl.runs, rec["runs"]):
        assert run.obs_type == ref["obs_type"] and run.year == ref["year"]
        assert run.day == ref["day"] and run.nchan == ref["nchan"]
        np.testing.assert_allclose(run.chan_freqs, ref["chan_freqs"], rtol=1e-15)
        assert os.path.relpath(run.rt_dcy, dcy) == ref["rt_dcy"]
        for kind in ("em", "tau", "flux"):
            assert os.path.relpath(getattr(run, "fits_" + kind), dcy) == ref["fits"][kind]["name"]
    ours = str(pl).replace("False", "True ")     # golden table was printed after completion
    assert [len(l) for l in ours.split("\n")] == [len(l) for l in rec["pipeline_str"].split("\n")]
    assert ours.split("\n")[:3] == rec["pipeline_str"].split("\n")[:3]
    with pytest.raises(TypeError):
        classes.Pipeline("not a model", pline_params(dcy))


def test_freq_str_and_scalars():
    s = json.load(open(os.path.join(GOLDEN, "scalars.json")))
    for f, ref in s["freq_str"].items():
        assert miscf.freq_str(float(f)) == ref
    assert mgeom.mod_r_0(25., 7. / 9., 1.) == pytest.approx(s["mod_r_0"], rel=1e-15)
    for line, ref in s["rrl_nu_0"].items():
        assert mrrl.rrl_nu_0(*mrrl.rrl_parser(line)) == pytest.approx(ref, rel=1e-15)
    assert mphys.doppler_shift(2.2364174326e10, 12.5) == pytest.approx(s["doppler_shift"], rel=1e-15)
    assert mphys.blackbody_nu(2.2e10, 9e3) == pytest.approx(s["blackbody_nu"], rel=1e-14)
    assert mrrl.deltanu_g(2.2364e10, 1e4, "H") == pytest.approx(s["deltanu_g"], rel=1e-14)
    assert mrrl.deltanu_l(1e6, 66, 1) == pytest.approx(s["deltanu_l"], rel=1e-14)
    g = np.load(os.path.join(GOLDEN, "gff.npz"))
    for i, nu in enumerate(g["nus"]):
        for j, t in enumerate(g["temps"]):
            assert mphys.gff(nu, t) == pytest.approx(g["gff"][i, j], rel=1e-13)


def test_mlr_roundtrip_like_reference_tests():
    """The reference's two passing tests (test/test_physics.py:15-57) check mlr_from_n_0 /
    n_0_from_mlr against numerical quadrature over a (q^d_n, q^d_v) grid; restated here
    as the analytic pair against the same integral."""
    from scipy.integrate import quad
    from rajepy_amd import _constants as con
    v_0, w_0, mu, R_1, R_2, n_0 = 150., 1., 1.3, .25, 2.5, 3e8
    for q_nd in np.linspace(-2., 0.5, 5):
        for q_vd in np.linspace(-2., 0.5, 5):
            def integrand(w):
                reff = R_1 + (R_2 - R_1) * w / w_0
                return 2 * np.pi * w * (reff / R_1) ** (q_nd + q_vd)
            integ = quad(integrand, 0, w_0)[0] * con.au ** 2
            ref = (integ * mu * mphys.atomic_mass('H') * n_0 * 1e6 * v_0 * 1e3
                   / con.MSOL * con.year)
            got = mphys.mlr_from_n_0(n_0, v_0, w_0, mu, q_nd, q_vd, R_1, R_2)
            assert got == pytest.approx(ref, rel=1e-3)
            assert mphys.n_0_from_mlr(got, v_0, w_0, mu, q_nd, q_vd, R_1, R_2) == \
                pytest.approx(n_0, rel=1e-9)


# ---- FITS writer -------------------------------------------------------------------------
def test_fits_float_format():
    assert fits.format_float(25.5) == "25.5"
    assert fits.format_float(2000.) == "2000.0"
    assert fits.format_float(67.89198899999998) == "67.89198899999998"
    assert fits.format_float(-1.157407407407407e-06) == "-1.1574074074074E-06"
    assert fits.format_float(5e9) == "5000000000.0"
    assert fits.format_float(22364174326.22781) == "22364174326.22781"


def test_fits_products_byte_identical_to_reference(tmp_path, rec):
    """Feed the reference's own map data through JetModel.save_fits: header cards and the
    whole file (sha256) must equal what astropy wrote for the reference."""
    arr = np.load(os.path.join(GOLDEN, "pipeline_cfg1.npz"))
    jm = make_model(tmp_path)
    kinds = {"em": "em", "tau": "tau", "flux": "flux"}
    for i, run in enumerate(rec["runs"]):
        jm.time = run["year"] * 31536000.0
        for kind, image_type in kinds.items():
            data = arr["run%d_%s" % (i, kind)]
            out = str(tmp_path / ("r%d_%s.fits" % (i, kind)))
            jm.save_fits(data, out, image_type, np.array(run["chan_freqs"]))
            got_data, cards = fits.read(out)
            assert cards == run["fits"][kind]["cards"], (i, kind)
            assert np.array_equal(got_data, data, equal_nan=True)
            raw = open(out, "rb").read()
            assert len(raw) == run["fits"][kind]["nbytes"]
            assert hashlib.sha256(raw).hexdigest() == run["fits"][kind]["sha256"], (i, kind)


def test_reorder_axes():
    a = np.arange(2 * 3 * 4).reshape(2, 3, 4)          # (F, n_x, n_z)
    r = miscf.reorder_axes(a, ra_axis=1, dec_axis=2, axis3=0, axis3_type='freq')
    assert r.shape == (2, 4, 3) and r[1, 2, 1] == a[1, 1, 2]
    b = np.arange(12).reshape(3, 4)
    assert np.array_equal(miscf.reorder_axes(b, ra_axis=0, dec_axis=1), b.T)


def test_logger_format(tmp_path):
    log = logger.Log(str(tmp_path / "x.log"), verbose=False)
    log.add_entry("INFO", "hello\nworld")
    log.add_entry("WARNING", "again", timestamp=False)
    lines = open(log.filename).read().split("\n")
    assert re.match(r"^\d{2}[A-Z]+\d{4}-\d{2}:\d{2}:\d{2}:: INFO   : hello$", lines[0])
    assert lines[1].endswith("world") and lines[1].startswith(" " * 10)
    assert lines[2].strip() == ": again"
    with pytest.raises(TypeError):
        log.add_entry("DEBUG", "x")


def test_graft_entry_build_compiles_and_binds():
    """The driver's build check: __graft_entry__.build() must compile the library in-tree and
    bind every symbol (no GPU needed)."""
    import __graft_entry__ as g
    g.build()


def test_any_number_of_bursts_and_lower_case_jet_names(tmp_path):
    """The reference registers every row of params["ejection"] (classes.py:245-264) and takes
    `which` in either case (which.upper(), classes.py:450-455): no cap on the burst count."""
    p = example_params()
    n = 11
    p["ejection"] = {"t_0": np.linspace(0.1, 3., n), "hl": np.full(n, 0.2),
                     "chi": np.full(n, 2.0), "which": np.array(["RB"] * n)}
    jm = make_model(tmp_path, p)
    assert len(jm._bursts['R']) == n and len(jm._bursts['B']) == n
    jm.add_ejection_event(1.0 * con.year, 3. * jm.ss_jml('R'), 0.1 * con.year, which='r')
    jm.add_ejection_event(1.0 * con.year, 3. * jm.ss_jml('B'), 0.1 * con.year, which='b')
    assert len(jm._bursts['R']) == n + 1 and len(jm._bursts['B']) == n + 1
    assert jm.ejections[str(2 * n + 1)]['which'] == 'R'
    with pytest.raises(ValueError):
        jm.add_ejection_event(0., 1., 1., which='x')
    b = jm._rjp_bursts()                     # ctypes struct: counts + host pointers
    assert b.n[0] == n + 1 and b.n[1] == n + 1
    assert b.t0[0][n] == 1.0 * con.year and b.amp_rel[1][n] == pytest.approx(2.0)
    # mdot(t) closure of the host mirror follows the same chain (classes.py:442-448)
    t = 1.0 * con.year
    want = jm.ss_jml('R') * (1. + sum(a * np.exp(-(t - t0) ** 2. / (2. * s ** 2.))
                                      for t0, a, s in jm._bursts['R']))
    assert jm.jml_t('R')(t) == pytest.approx(want, rel=1e-14)


def test_reynolds86_analytic_fluxes_match_the_reference(tmp_path):
    """tau_r, r_tau1, approx_flux_expected_r86, flux_expected_r86
    (maths/physics.py:93-374) against values recorded from the imported reference
    (tests/golden/r86.json, written by make_golden.py) for config 1 at three frequencies,
    both lobes, with and without y_min.  Tolerance 1e-10 (mpmath 1.3.0 here vs the
    reference's 1.2.1 for the incomplete gamma function of negative order)."""
    gold = json.load(open(os.path.join(GOLDEN, "r86.json")))
    jm = make_model(tmp_path)
    freqs = gold["freqs"]
    for which in ("R", "B"):
        assert jm.ss_jml(which) == pytest.approx(gold["ss_jml"][which], rel=1e-14)
        got = [mphys.approx_flux_expected_r86(jm, f, which) for f in freqs]
        np.testing.assert_allclose(got, gold["approx_" + which], rtol=1e-10)
        got = [mphys.flux_expected_r86(jm, f, which, gold["y_max_arcsec"]) for f in freqs]
        np.testing.assert_allclose(got, gold["exact_" + which], rtol=1e-10)
        got = [mphys.flux_expected_r86(jm, f, which, gold["y_max_arcsec"], 0.05) for f in freqs]
        np.testing.assert_allclose(got, gold["exact_ymin_" + which], rtol=1e-10)
    np.testing.assert_allclose(mphys.approx_flux_expected_r86(jm, list(freqs), "B"),
                               gold["approx_array_B"], rtol=1e-10)
    g, pl, pr = jm.params["geometry"], jm.params["power_laws"], jm.params["properties"]
    args = (g["r_0"], g["w_0"], pr["n_0"], pr["x_0"], pr["T_0"])
    tail = (g["inc"], g["epsilon"], pl["q_n"], pl["q_x"], pl["q_T"], g["opang"])
    np.testing.assert_allclose([mphys.r_tau1(*args, f, *tail) for f in freqs],
                               gold["r_tau1_au"], rtol=1e-10)
    np.testing.assert_allclose([mphys.r_tau1(*args, f, *tail, dist=jm.params["target"]["dist"])
                                for f in freqs], gold["r_tau1_arcsec"], rtol=1e-10)
    np.testing.assert_allclose([[mphys.tau_r(r, *args, f, *tail) for r in (1., 5., 40.)]
                                for f in freqs], gold["tau_r"], rtol=1e-10)
    # disc-wind density prescription: the reference looks up properties["mlr"], which
    # today's params files do not carry -> KeyError there (recorded) and here
    assert gold["tilted_raises"].startswith("KeyError")
    from tests.test_gpu_model import tilted_params
    tj = make_model(tmp_path, tilted_params())
    with pytest.raises(KeyError, match="mlr"):
        mphys.flux_expected_r86(tj, 5e9, "B", 1.0)
    with pytest.raises(KeyError, match="mlr"):
        mphys.approx_flux_expected_r86(tj, 5e9, "B")


def test_sgpr_table_load_checker_sees_a_reader_before_the_wait():
    """tools/check_sgpr_tables.py (run by `build.sh --report`): a copy or spill of the registers
    an in-flight s_load_dwordx16 will fill, before the s_waitcnt that covers it, is reported."""
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "check_sgpr_tables", os.path.join(ROOT, "tools", "check_sgpr_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    good = """_ZN3rjp4kernE:
	s_load_dwordx16 s[36:51], s[2:3], 0x0
	v_fma_f64 v[0:1], v[2:3], v[4:5], v[6:7]
	v_writelane_b32 v9, s60, 3
	s_waitcnt lgkmcnt(0)
	v_fma_f64 v[0:1], v[2:3], s[36:37], v[6:7]
	s_endpgm
"""
    bad, n = mod.check(good, "t")
    assert n == 1 and bad == []
    for culprit in ("v_writelane_b32 v9, s40, 3", "s_mov_b64 s[70:71], s[50:51]",
                    "v_fma_f64 v[0:1], v[2:3], s[36:37], v[6:7]"):
        text = good.replace("	v_writelane_b32 v9, s60, 3", "	" + culprit)
        bad, _ = mod.check(text, "t")
        assert len(bad) == 1 and bad[0][3] == culprit, (culprit, bad)
    # a wait for another counter does not count
    text = good.replace("s_waitcnt lgkmcnt(0)", "s_waitcnt vmcnt(0)\n	v_writelane_b32 v9, s41, 1\n	s_waitcnt lgkmcnt(0)")
    assert len(mod.check(text, "t")[0]) == 1


def test_burst_gaussian_polynomial_meets_its_documented_bound():
    """K1's direct scans evaluate 2^f, |f| <= 1/2, by the degree-8 polynomial whose
    coefficients sit in rjp_device.h (RJP_EXP2_D8 .. D1): the header documents 1.1e-12
    relative before rounding -- the float64 Horner chain the kernel runs must stay inside it
    (and the degree-10 one of the recurrence anchors inside 1e-15)."""
    hdr = open(os.path.join(ROOT, "rajepy_amd", "csrc", "rjp_device.h")).read()
    f = np.linspace(-0.5, 0.5, 400001)

    def horner(prefix, deg):
        c = [float(re.search(r"#define %s%d ([-+0-9.eE]+)" % (prefix, k), hdr).group(1))
             for k in range(deg, 0, -1)]
        p = np.full_like(f, c[0])
        for ck in c[1:]:
            p = p * f + ck
        return p * f + 1.0

    ref = np.exp2(f)
    assert np.max(np.abs(horner("RJP_EXP2_D", 8) / ref - 1.0)) < 1.2e-12
    assert np.max(np.abs(horner("RJP_EXP2_C", 10) / ref - 1.0)) < 1e-15


def test_pure_argument_checks_from_plain_cpp(tmp_path):
    """rajepy_amd/csrc/rjp_args.h -- the argument checks that are pure functions of the caller's
    structs -- compiled into a stand-alone program by plain g++ (tests/rjp_args_cases.cpp: no HIP,
    hand-built structs).  Every refusal it prints must be, status and message, what the library
    gave for the same case on the GPU (tests/golden/abi_refusals.json); the calls it marks valid
    pass; the chain-rule table of the sensitivity calls holds (2 amp inv2s2, 1, -amp) per burst,
    behind a leading 1 for rjp_ff_grad."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "rjp_args_cases"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I",
                    os.path.join(ROOT, "rajepy_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rjp_args_cases.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    golden = json.load(open(os.path.join(GOLDEN, "abi_refusals.json")))
    refusals, valid, scales = set(), 0, {}
    for line in out.splitlines():
        entry, case, *rest = line.split("\t")
        if entry == "scale":
            scales.setdefault(case, []).append([float(v) for v in rest])
        elif case == "valid":
            assert rest == ["0", ""], line
            valid += 1
        else:
            assert [int(rest[0]), rest[1]] == golden[entry][case], line
            refusals.add(entry)
    # (one entry point per check and flag combination the program drives)
    assert refusals == {"rjp_compact_fields", "rjp_y_bounds", "rjp_rrl_scan", "rjp_tavg",
                        "rjp_ff_formal_sweep", "rjp_ff_grad", "rjp_ff_formal_grad",
                        "rjp_lt_count", "rjp_srt_count"} and valid > 0
    per_burst = {0: [2.0 * 2.0 * 1e-14, 1.0, -2.0], 1: [2.0 * 1.0 * 1e-14, 1.0, -1.0]}
    for who, lead in (("rjp_ff_grad", [1.0]), ("rjp_ff_formal_grad", [])):
        assert scales[who] == [lead + per_burst[0] + per_burst[1],
                               lead + per_burst[0] * 8 + per_burst[1] * 8], who
