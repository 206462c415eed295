"""The case table of tests/test_gpu_refusals.py and tools/record_abi_refusals.py: for every
int-returning entry point of include/rjprt.h that takes arguments beyond the context, ONE valid
call on a synthetic 8 x 16 x 16 grid (f64, tau layout; an f32 twin where a check needs one) and
the refusals of that call.  A case names the arguments it changes -- one argument per case (a
struct counts as one argument), two in the cases whose name starts with "2:", which record which
refusal wins.  Every non-NULL pointer is a real allocation of the size the valid call needs:
should a case ever be accepted, the kernel it starts stays inside its buffers.

    ENTRIES: name -> (valid(env) -> {argument: value} in the prototype's order, [(case, change)])

`change(args)` edits the dict `valid` returned (fresh for every case).  The expected (status,
message) pairs are tests/golden/abi_refusals.json, recorded from the library before its entry
points were consolidated."""
import ctypes as C

from rajepy_amd import _lib
from rajepy_amd.engine import RJP_F32, RJP_F64, RJP_GFF_SCALAR, make_bursts

SHAPE = (8, 16, 16)
SEED = 20240611
YEAR = 31557600.0
LT_K = SRT_K = 4
BAD_MODE = 5


class Env:
    """The allocations the valid calls need, made once."""

    def __init__(self, eng):
        import torch
        from rajepy_amd.maths import rrls
        from oracle import rt_oracle as orc
        from tests import gpu_util as U
        self.eng, self.lib = eng, eng.lib
        kw = dict(csize_au=0.5, with_vy=True)
        self.f64 = eng.synth_fields(SHAPE, SEED, 1, RJP_F64, tau_mode=RJP_GFF_SCALAR, **kw)
        self.f32 = eng.synth_fields(SHAPE, SEED, 1, RJP_F32, **kw)
        assert self.f64.a0 is not None and self.f64.em0 is not None and self.f32.em0 is not None
        assert eng.launch_time_range(self.f64) is not None
        free = eng.srt_min_free
        eng.srt_min_free = 0.0
        self.lt, self.srt = eng.build_lt(self.f64, LT_K), eng.build_sorted(self.f64, SRT_K)
        eng.srt_min_free = free
        assert self.srt is not None and self.srt["mom"] is not None
        self.f64.lt = self.f64.srt = None          # (the buffers stay; no scan here reads them)
        self.N = self.f64.ncells
        self.P = self.f64.npix
        self.out = [torch.empty(1 << 16, dtype=torch.float64, device=eng.device) for _ in range(8)]
        self.i32 = [torch.empty(1 << 12, dtype=torch.int32, device=eng.device) for _ in range(2)]
        self.i32[0].zero_()                        # (a y-range pair: rjp_occupied_cells)
        self.i32[1].fill_(SHAPE[1])
        self.i64 = torch.empty(64, dtype=torch.int64, device=eng.device)
        self.work = torch.empty(1 << 22, dtype=torch.uint8, device=eng.device)
        self.work2 = torch.empty(1 << 22, dtype=torch.uint8, device=eng.device)
        self.red = torch.zeros(self.N, dtype=torch.uint8, device=eng.device)
        self.line = _lib.Line(**rrls.line_constants("H66a"))
        self.nu = _lib.dbl_array([self.line.nu_rest * (1.0 - 1e-5), self.line.nu_rest])
        self.tab = [_lib.dbl_array([1e-30 * (k + 1), 2e-30 * (k + 1)]) for k in range(4)]
        self.epochs = _lib.dbl_array([1.0 * YEAR, 1.25 * YEAR])
        self.nan = _lib.dbl_array([1.0 * YEAR, float("nan")])
        p = U.load_golden("cfg1_example")[2]
        p["grid"].update(n_x=SHAPE[0], n_y=SHAPE[1], n_z=SHAPE[2])
        self.params = orc.OracleJet(p).params

    def fields(self):
        return self.f64.struct()

    def geometry(self):
        from rajepy_amd.classes import geometry_struct
        return geometry_struct(self.params, *SHAPE)

    def new_bursts(self, red=1, blue=1):
        return make_bursts([(1.0 * YEAR, 2.0, 0.2 * YEAR)] * red,
                           [(1.5 * YEAR, 1.0, 0.3 * YEAR)] * blue)

    def need(self, nbytes):
        """A workspace size the library names: the shared workspace holds it."""
        assert 0 < nbytes <= self.work.numel(), nbytes
        return nbytes


def ptr(t):
    return t.data_ptr() if t is not None else None


# ---- changes ---------------------------------------------------------------------------------
def arg(**kw):
    return lambda a: a.update(kw)


def mem(name, **kw):
    def change(a):
        for k, v in kw.items():
            setattr(a[name], k, v)
    return change


def elem(name, member, index, value):
    """a[name].member[index] = value (the arrays inside rjp_bursts)"""
    def change(a):
        getattr(a[name], member)[index] = value
    return change


def both(*changes):
    def change(a):
        for c in changes:
            c(a)
    return change


def f32_twin(a):
    a["fields"] = a["_env"].f32.struct()


def ylo_only(a):
    a["fields"].d_ylo = ptr(a["_env"].i32[0])


def less(name):
    return lambda a: a.update({name: a[name] - 1})


NULL_DP = C.POINTER(C.c_double)()


def fields_cases(need_vy=False, compact_ok=False):
    """check_fields' refusals as an entry point with these flags reaches them"""
    c = [("fields NULL", arg(fields=None)),
         ("fields.dtype", mem("fields", dtype=3)),
         ("fields.nx = 0", mem("fields", nx=0)),
         ("fields.nz < 0", mem("fields", nz=-4)),
         ("fields.a0_mode", mem("fields", a0_mode=7)),
         ("fields.csize_au = 0", mem("fields", csize_au=0.0)),
         ("fields.d_ylo alone", ylo_only)]
    if compact_ok:
        c += [("compact without d_temp", mem("fields", d_a0=None, d_temp=None)),
              ("no complete layout", mem("fields", d_a0=None, d_em0=None, d_pf=None))]
    else:
        c += [("fields.d_xi NULL", mem("fields", d_xi=None))]
    if need_vy:
        c += [("fields.d_vy NULL", mem("fields", d_vy=None))]
    return c


def bursts_cases():
    """check_bursts' refusals"""
    return [("bursts.n < 0", elem("bursts", "n", 1, -1)),
            ("bursts.n too large", elem("bursts", "n", 0, (1 << 20) + 1)),
            ("bursts.amp_rel NULL", elem("bursts", "amp_rel", 0, NULL_DP)),
            ("bursts without fields.d_ts", mem("fields", d_ts=None))]


def layout_cases(kmax, ny_limit=False):
    """check_lt / check_srt (`ny_limit`: the layout holds y in 16 bits)"""
    more = [("fields.ny = 65536", mem("fields", ny=65536))] if ny_limit else []
    return more + [("fields NULL", arg(fields=None)),
            ("f32 fields", f32_twin),
            ("fields.d_a0 NULL", mem("fields", d_a0=None)),
            ("fields.d_ts NULL", mem("fields", d_ts=None)),
            ("fields.ny = 0", mem("fields", ny=0)),
            ("K = 0", arg(K=0)),
            ("K above the limit", arg(K=kmax + 1)),
            ("no launch-time range", mem("fields", ts_lo=0.0, ts_hi=0.0)),
            ("ts_hi < ts_lo", mem("fields", ts_lo=2.0, ts_hi=1.0)),
            ("ts_hi infinite", mem("fields", ts_hi=float("inf"))),
            ("2: f32 fields, K = 0", both(f32_twin, arg(K=0))),
            ("2: K = 0, no launch-time range", both(arg(K=0), mem("fields", ts_lo=0.0, ts_hi=0.0)))]


ENTRIES = {}


def entry(name, cases):
    def deco(valid):
        ENTRIES[name] = (valid, cases)
        return valid
    return deco


# ---- contexts and plain fields ------------------------------------------------------------------
@entry("rjp_ctx_create", [("out NULL", arg(out=None)), ("device = -1", arg(device=-1)),
                          ("device out of range", arg(device=1 << 20)),
                          ("2: device = -1, out NULL", arg(device=-1, out=None))])
def _(e):
    return dict(device=e.eng.device_index, out=C.c_void_p())


@entry("rjp_pack_field", [("d_src NULL", arg(d_src=None)), ("d_dst NULL", arg(d_dst=None)),
                          ("n = 0", arg(n=0)), ("dtype", arg(dtype=2)),
                          ("2: n = 0, dtype", arg(n=0, dtype=2))])
def _(e):
    return dict(ctx=e.eng.ctx, d_src=ptr(e.out[0]), d_den=ptr(e.out[1]), d_red=ptr(e.red),
                d_dst=ptr(e.out[2]), n=e.N, dtype=RJP_F64)


@entry("rjp_compact_fields", fields_cases() + [
    ("d_em0 NULL", arg(d_em0=None)), ("d_n_bad NULL", arg(d_n_bad=None)),
    ("2: fields NULL, d_em0 NULL", arg(fields=None, d_em0=None))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), d_em0=ptr(e.out[0]), d_n_bad=ptr(e.i64))


@entry("rjp_tau_field", fields_cases(compact_ok=True) + [
    ("gff_mode", arg(gff_mode=BAD_MODE)), ("f32 fields", f32_twin),
    ("fields.d_em0 NULL", mem("fields", d_em0=None)), ("d_a0 NULL", arg(d_a0=None)),
    ("2: gff_mode, d_a0 NULL", arg(gff_mode=BAD_MODE, d_a0=None)),
    ("2: fields.dtype, gff_mode", both(mem("fields", dtype=3), arg(gff_mode=BAD_MODE)))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), gff_mode=RJP_GFF_SCALAR, d_a0=ptr(e.out[0]))


@entry("rjp_unmask_launch_times", [
    ("fields NULL", arg(fields=None)), ("fields.d_ts NULL", mem("fields", d_ts=None)),
    ("d_ts_out NULL", arg(d_ts_out=None)), ("fields.dtype", mem("fields", dtype=3)),
    ("fields.ny = 0", mem("fields", ny=0)), ("jet", arg(jet=2)),
    ("no flag field", mem("fields", d_a0=None, d_em0=None, d_nd=None)),
    ("2: fields.dtype, jet", both(mem("fields", dtype=3), arg(jet=2))),
    ("2: d_ts_out NULL, jet", arg(d_ts_out=None, jet=-1))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), jet=0, d_ts_out=ptr(e.out[0]))


@entry("rjp_field_range", [("d_field NULL", arg(d_field=None)),
                           ("d_partials NULL", arg(d_partials=None)), ("n = 0", arg(n=0)),
                           ("dtype", arg(dtype=0)), ("2: n < 0, dtype", arg(n=-1, dtype=0))])
def _(e):
    assert 2 * _lib.RJP_RANGE_BLOCKS <= e.out[0].numel()
    return dict(ctx=e.eng.ctx, d_field=ptr(e.f64.ts), n=e.N, dtype=RJP_F64,
                d_partials=ptr(e.out[0]))


@entry("rjp_tavg", [
    ("fields NULL", arg(fields=None)), ("fields.d_temp NULL", mem("fields", d_temp=None)),
    ("fields.dtype", mem("fields", dtype=3)), ("fields.nx = 0", mem("fields", nx=0)),
    ("fields.d_ylo alone", ylo_only), ("d_tavg NULL", arg(d_tavg=None)),
    ("d_work NULL", arg(d_work=None)), ("workspace one byte short", less("work_bytes")),
    ("2: fields.dtype, d_tavg NULL", both(mem("fields", dtype=3), arg(d_tavg=None))),
    ("2: d_work NULL, work_bytes = 0", arg(d_work=None, work_bytes=0))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), d_tavg=ptr(e.out[0]), d_work=ptr(e.work),
                work_bytes=e.need(e.lib.rjp_ff_scan_workspace(*SHAPE, 1)))


@entry("rjp_y_bounds", fields_cases(compact_ok=True) + [
    ("d_ylo NULL", arg(d_ylo=None)), ("d_yhi NULL", arg(d_yhi=None)),
    ("2: fields NULL, d_ylo NULL", arg(fields=None, d_ylo=None))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), d_ylo=ptr(e.i32[0]), d_yhi=ptr(e.i32[1]))


@entry("rjp_occupied_cells", [("d_ylo NULL", arg(d_ylo=None)), ("d_yhi NULL", arg(d_yhi=None)),
                              ("h_count NULL", arg(h_count=None)), ("n_pix = 0", arg(n_pix=0))])
def _(e):
    return dict(ctx=e.eng.ctx, d_ylo=ptr(e.i32[0]), d_yhi=ptr(e.i32[1]), n_pix=e.P,
                h_count=C.c_int64())


# ---- K1 / K2 -----------------------------------------------------------------------------------
def scan_args(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), bursts=e.new_bursts(), h_epochs_s=e.epochs,
                n_epochs=1, gff_mode=RJP_GFF_SCALAR, d_sumA=ptr(e.out[0]), d_em=ptr(e.out[1]),
                d_tavg=ptr(e.out[2]), d_work=ptr(e.work),
                work_bytes=e.need(e.lib.rjp_ff_scan_workspace(*SHAPE, 1)))


SCAN_CASES = [("gff_mode", arg(gff_mode=BAD_MODE))] + \
    fields_cases(compact_ok=True) + bursts_cases() + [
    ("h_epochs_s NULL", arg(h_epochs_s=None)), ("n_epochs = 0", arg(n_epochs=0)),
    ("d_sumA NULL", arg(d_sumA=None)), ("d_work NULL", arg(d_work=None)),
    ("tau layout only, d_tavg", mem("fields", d_temp=None)),
    ("tau layout only, d_em", mem("fields", d_em0=None, d_nd=None)),
    ("workspace one byte short", less("work_bytes")),
    ("2: gff_mode, fields NULL", arg(gff_mode=BAD_MODE, fields=None)),
    ("2: fields NULL, h_epochs_s NULL", arg(fields=None, h_epochs_s=None)),
    ("2: bursts.n < 0, n_epochs = 0", both(elem("bursts", "n", 0, -1), arg(n_epochs=0))),
    ("2: d_sumA NULL, workspace short", both(arg(d_sumA=None), less("work_bytes")))]


entry("rjp_ff_scan", SCAN_CASES)(scan_args)


@entry("rjp_time_ff_scan", [
    ("reps = 0", arg(reps=0)), ("ms_avg NULL", arg(ms_avg=None)),
    ("gff_mode", arg(gff_mode=BAD_MODE)), ("fields NULL", arg(fields=None)),
    ("d_sumA NULL", arg(d_sumA=None)), ("workspace one byte short", less("work_bytes")),
    ("2: ctx NULL, reps = 0", arg(ctx=None, reps=0)),
    ("2: reps = 0, fields NULL", arg(reps=0, fields=None))])
def _(e):
    a = scan_args(e)
    a["_tail"] = dict(reps=2, ms_avg=C.c_double())
    return a


def maps_args(e):
    return dict(ctx=e.eng.ctx, d_sumA=ptr(e.out[0]), d_tavg=ptr(e.out[1]), n_pix=e.P, n_epochs=2,
                h_ctau=e.tab[0], h_cflux=e.tab[1], n_chan=2, d_tau=ptr(e.out[2]),
                d_flux=ptr(e.out[3]), d_ftot=ptr(e.out[4]), d_work=ptr(e.work2),
                work_bytes=e.need(e.lib.rjp_ff_maps_workspace(e.P, 2, 2)))


entry("rjp_ff_maps", [
    ("d_sumA NULL", arg(d_sumA=None)), ("d_tavg NULL", arg(d_tavg=None)),
    ("h_ctau NULL", arg(h_ctau=None)), ("h_cflux NULL", arg(h_cflux=None)),
    ("n_pix = 0", arg(n_pix=0)), ("n_epochs = 0", arg(n_epochs=0)), ("n_chan = 0", arg(n_chan=0)),
    ("d_work NULL", arg(d_work=None)), ("workspace one byte short", less("work_bytes")),
    ("2: h_ctau NULL, n_chan = 0", arg(h_ctau=None, n_chan=0)),
    ("2: n_pix = 0, d_work NULL", arg(n_pix=0, d_work=None))])(maps_args)


@entry("rjp_ff_step", [
    ("fields NULL", arg(fields=None)), ("d_tavg NULL", arg(d_tavg=None)),
    ("h_cflux NULL", arg(h_cflux=None)), ("n_chan = 0", arg(n_chan=0)),
    ("fields.nx = 0", mem("fields", nx=0)), ("n_epochs = 0", arg(n_epochs=0)),
    ("d_work_maps NULL", arg(d_work_maps=None)),
    ("map workspace one byte short", less("work_maps_bytes")),
    ("gff_mode", arg(gff_mode=BAD_MODE)), ("fields.dtype", mem("fields", dtype=3)),
    ("fields.ny = 0", mem("fields", ny=0)), ("bursts.n < 0", elem("bursts", "n", 1, -1)),
    ("h_epochs_s NULL", arg(h_epochs_s=None)), ("d_sumA NULL", arg(d_sumA=None)),
    ("tau layout only, d_em", mem("fields", d_em0=None, d_nd=None)),
    ("workspace one byte short", less("work_bytes")),
    ("2: gff_mode, n_chan = 0", arg(gff_mode=BAD_MODE, n_chan=0)),
    ("2: d_work_maps NULL, d_sumA NULL", arg(d_work_maps=None, d_sumA=None)),
    ("2: fields.dtype, d_tavg NULL", both(mem("fields", dtype=3), arg(d_tavg=None)))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), bursts=e.new_bursts(), h_epochs_s=e.epochs,
                n_epochs=1, gff_mode=RJP_GFF_SCALAR, d_tavg=ptr(e.out[5]), h_ctau=e.tab[0],
                h_cflux=e.tab[1], n_chan=2, d_sumA=ptr(e.out[0]), d_em=ptr(e.out[1]),
                d_tau=ptr(e.out[2]), d_flux=ptr(e.out[3]), d_ftot=ptr(e.out[4]),
                d_work=ptr(e.work),
                work_bytes=e.need(e.lib.rjp_ff_scan_workspace(*SHAPE, 1)),
                d_work_maps=ptr(e.work2),
                work_maps_bytes=e.need(e.lib.rjp_ff_maps_workspace(e.P, 1, 2)))


# ---- diagnostics ---------------------------------------------------------------------------------
@entry("rjp_last_scan_path", [("ctx NULL", arg(ctx=None))])
def _(e):
    return dict(ctx=e.eng.ctx, worst_rel_err=C.c_double(), moment_shape=(C.c_int32 * 2)(),
                _status_only=True, _no_stream=True)


@entry("rjp_last_scan_tiles", [("ctx NULL", arg(ctx=None)), ("n_tiles NULL", arg(n_tiles=None)),
                               ("cap < 0", arg(cap=-1)), ("tiles NULL", arg(tiles=None)),
                               ("cap = 0 after a tiled scan", arg(cap=0))])
def _(e):
    return dict(ctx=e.eng.ctx, n_tiles=C.c_int32(), tiles=(C.c_int32 * 320)(), cap=64,
                _status_only=True, _no_stream=True)


@entry("rjp_last_maps_launch", [("ctx NULL", arg(ctx=None))])
def _(e):
    return dict(ctx=e.eng.ctx, out=(C.c_int32 * 6)(), _status_only=True, _no_stream=True)


@entry("rjp_last_srt_bins", [("contracted NULL", arg(contracted=None)),
                             ("read NULL", arg(read=None))])
def _(e):
    return dict(ctx=e.eng.ctx, contracted=C.c_int64(), read=C.c_int64(), _no_stream=True)


# ---- the launch-time layouts ---------------------------------------------------------------------
@entry("rjp_lt_count", layout_cases(80, True) + [
    ("d_rowoff NULL", arg(d_rowoff=None)), ("h_total_rows NULL", arg(h_total_rows=None))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), K=LT_K, d_rowoff=ptr(e.lt["rowoff"]),
                h_total_rows=C.c_int64())


@entry("rjp_lt_fill", layout_cases(80, True) + [
    ("d_rowoff NULL", arg(d_rowoff=None)), ("d_cells NULL", arg(d_cells=None)),
    ("d_aux NULL", arg(d_aux=None))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), K=LT_K, d_rowoff=ptr(e.lt["rowoff"]),
                d_cells=ptr(e.lt["cells"]), d_aux=ptr(e.lt["aux"]))


@entry("rjp_srt_count", layout_cases(32) + [
    ("d_start NULL", arg(d_start=None)), ("d_rowbase NULL", arg(d_rowbase=None)),
    ("h_hist NULL", arg(h_hist=None)), ("h_total_rows NULL", arg(h_total_rows=None))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), K=SRT_K, d_start=ptr(e.srt["start"]),
                d_rowbase=ptr(e.srt["rowbase"]), h_hist=(C.c_int64 * (2 * SRT_K))(),
                h_total_rows=C.c_int64())


@entry("rjp_srt_fill", layout_cases(32) + [
    ("d_start NULL", arg(d_start=None)), ("d_rowbase NULL", arg(d_rowbase=None)),
    ("d_cells NULL", arg(d_cells=None)), ("d_cum NULL", arg(d_cum=None)),
    ("d_aux NULL", arg(d_aux=None))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), K=SRT_K, d_start=ptr(e.srt["start"]),
                d_rowbase=ptr(e.srt["rowbase"]), d_cells=ptr(e.srt["cells"]),
                d_cum=ptr(e.srt["cum"]), d_aux=ptr(e.srt["aux"]))


@entry("rjp_srt_moments", layout_cases(32) + [
    ("N", arg(N=18)), ("d_start NULL", arg(d_start=None)), ("d_rowbase NULL", arg(d_rowbase=None)),
    ("d_cells NULL", arg(d_cells=None)), ("d_mom NULL", arg(d_mom=None)),
    ("2: N, d_mom NULL", arg(N=0, d_mom=None))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), K=SRT_K, N=e.srt["N"],
                d_start=ptr(e.srt["start"]), d_rowbase=ptr(e.srt["rowbase"]),
                d_cells=ptr(e.srt["cells"]), d_mom=ptr(e.srt["mom"]))


# ---- per-cell depths, formal solutions, sensitivities --------------------------------------------
@entry("rjp_rrl_scan", fields_cases(need_vy=True) + bursts_cases() + [
    ("line NULL", arg(line=None)), ("h_nu NULL", arg(h_nu=None)), ("n_chan = 0", arg(n_chan=0)),
    ("d_tau_rrl NULL", arg(d_tau_rrl=None)),
    ("2: fields.d_vy NULL, line NULL", both(mem("fields", d_vy=None), arg(line=None))),
    ("2: bursts.n < 0, h_nu NULL", both(elem("bursts", "n", 0, -1), arg(h_nu=None)))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), bursts=e.new_bursts(), time_s=1.2 * YEAR,
                line=e.line, h_nu=e.nu, n_chan=2, d_tau_rrl=ptr(e.out[0]))


@entry("rjp_rrl_cells", fields_cases(need_vy=True) + bursts_cases() + [
    ("line NULL", arg(line=None)), ("h_nu NULL", arg(h_nu=None)), ("n_chan = 0", arg(n_chan=0)),
    ("d_tau_cells NULL", arg(d_tau_cells=None)),
    ("2: fields NULL, n_chan = 0", arg(fields=None, n_chan=0))])
def _(e):
    assert 2 * e.N <= e.out[0].numel()
    return dict(ctx=e.eng.ctx, fields=e.fields(), bursts=e.new_bursts(), time_s=1.2 * YEAR,
                line=e.line, h_nu=e.nu, n_chan=2, d_tau_cells=ptr(e.out[0]))


@entry("rjp_ff_cells", fields_cases() + bursts_cases() + [
    ("h_ctau NULL", arg(h_ctau=None)), ("n_chan = 0", arg(n_chan=0)),
    ("d_tau_cells NULL", arg(d_tau_cells=None)), ("gff_mode", arg(gff_mode=BAD_MODE)),
    ("2: gff_mode, h_ctau NULL", arg(gff_mode=BAD_MODE, h_ctau=None)),
    ("2: gff_mode, fields NULL", arg(gff_mode=BAD_MODE, fields=None))])
def _(e):
    assert 2 * e.N <= e.out[0].numel()
    return dict(ctx=e.eng.ctx, fields=e.fields(), bursts=e.new_bursts(), time_s=1.2 * YEAR,
                gff_mode=RJP_GFF_SCALAR, h_ctau=e.tab[0], n_chan=2, d_tau_cells=ptr(e.out[0]))


@entry("rjp_ff_formal", [("gff_mode", arg(gff_mode=BAD_MODE))] +
       fields_cases(compact_ok=True) + bursts_cases() + [
    ("fields.d_temp NULL", mem("fields", d_temp=None)),
    ("h_ctau NULL", arg(h_ctau=None)), ("h_csrc NULL", arg(h_csrc=None)),
    ("n_chan = 0", arg(n_chan=0)), ("d_out NULL", arg(d_out=None)),
    ("2: gff_mode, fields NULL", arg(gff_mode=BAD_MODE, fields=None)),
    ("2: fields.d_temp NULL, d_out NULL", both(mem("fields", d_temp=None), arg(d_out=None)))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), bursts=e.new_bursts(), time_s=1.2 * YEAR,
                gff_mode=RJP_GFF_SCALAR, h_ctau=e.tab[0], h_csrc=e.tab[1], n_chan=2,
                d_out=ptr(e.out[0]))


@entry("rjp_ff_formal_sweep", [("gff_mode", arg(gff_mode=BAD_MODE))] +
       fields_cases(compact_ok=True) + bursts_cases() + [
    ("fields.d_temp NULL", mem("fields", d_temp=None)),
    ("h_epochs_s NULL", arg(h_epochs_s=None)), ("n_epochs = 0", arg(n_epochs=0)),
    ("non-finite epoch", lambda a: a.update(h_epochs_s=a["_env"].nan)),
    ("h_csrc NULL", arg(h_csrc=None)), ("n_chan = 0", arg(n_chan=0)),
    ("n_epochs * n_chan", arg(n_chan=1 << 30)),
    ("d_work NULL", arg(d_work=None)), ("workspace one byte short", less("work_bytes")),
    ("2: both outputs NULL", arg(d_out=None, d_ftot=None)),
    ("2: n_epochs = 0, n_chan = 0", arg(n_epochs=0, n_chan=0)),
    ("2: non-finite epoch, h_ctau NULL",
     lambda a: a.update(h_epochs_s=a["_env"].nan, h_ctau=None))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), bursts=e.new_bursts(), h_epochs_s=e.epochs,
                n_epochs=2, gff_mode=RJP_GFF_SCALAR, h_ctau=e.tab[0], h_csrc=e.tab[1], n_chan=2,
                d_out=ptr(e.out[0]), d_ftot=ptr(e.out[1]), d_work=ptr(e.work),
                work_bytes=e.need(e.lib.rjp_ff_formal_sweep_workspace(*SHAPE, 2, 2)))


def nan_burst(a):
    b = a["_env"].new_bursts()
    b.inv2s2[1][0] = float("nan")
    a["bursts"] = b


GRAD_BURSTS = [
    ("bursts NULL", arg(bursts=None)), ("no burst", lambda a: a.update(bursts=make_bursts([], []))),
    ("bursts.n < 0", elem("bursts", "n", 1, -1)),
    ("bursts.amp_rel NULL", elem("bursts", "amp_rel", 0, NULL_DP)),
    ("nine bursts in a jet", lambda a: a.update(bursts=a["_env"].new_bursts(9, 1))),
    ("non-finite burst parameter", nan_burst),
    ("h_epochs_s NULL", arg(h_epochs_s=None)), ("n_epochs = 0", arg(n_epochs=0)),
    ("non-finite epoch", lambda a: a.update(h_epochs_s=a["_env"].nan)),
    ("2: nine bursts, n_epochs = 0",
     lambda a: a.update(bursts=a["_env"].new_bursts(1, 9), n_epochs=0)),
    ("2: non-finite epoch and burst parameter",
     both(nan_burst, lambda a: a.update(h_epochs_s=a["_env"].nan)))]


@entry("rjp_ff_grad", [
    ("gff_mode", arg(gff_mode=BAD_MODE)), ("fields NULL", arg(fields=None)),
    ("f32 fields", f32_twin), ("fields.d_a0 NULL", mem("fields", d_a0=None)),
    ("a0 built for the other mode", mem("fields", a0_mode=1)),
    ("fields.nx = 0", mem("fields", nx=0)), ("fields.csize_au = 0", mem("fields", csize_au=0.0)),
    ("fields.d_ylo alone", ylo_only), ("fields.d_ts NULL", mem("fields", d_ts=None))] +
    GRAD_BURSTS + [
    ("2: all four outputs NULL", lambda a: a.update(d_sumA=None, d_dsumA=None, d_ftot=None,
                                                    d_dftot=None)),
    ("d_tavg NULL", arg(d_tavg=None)), ("h_cflux NULL", arg(h_cflux=None)),
    ("n_chan = 0", arg(n_chan=0)), ("d_work NULL", arg(d_work=None)),
    ("workspace one byte short", less("work_bytes")),
    ("2: gff_mode, fields NULL", arg(gff_mode=BAD_MODE, fields=None)),
    ("2: fields.d_ts NULL, bursts NULL", both(mem("fields", d_ts=None), arg(bursts=None)))])
def _(e):
    assert 2 * 6 * e.P <= e.out[1].numel()
    return dict(ctx=e.eng.ctx, fields=e.fields(), bursts=e.new_bursts(), h_epochs_s=e.epochs,
                n_epochs=2, gff_mode=RJP_GFF_SCALAR, d_tavg=ptr(e.out[5]), h_ctau=e.tab[0],
                h_cflux=e.tab[1], n_chan=2, d_sumA=ptr(e.out[0]), d_dsumA=ptr(e.out[1]),
                d_ftot=ptr(e.out[2]), d_dftot=ptr(e.out[3]), d_work=ptr(e.work),
                work_bytes=e.need(e.lib.rjp_ff_grad_workspace(*SHAPE, 2, 6, 2)))


@entry("rjp_ff_formal_grad", [
    ("gff_mode", arg(gff_mode=BAD_MODE)), ("fields NULL", arg(fields=None)),
    ("f32 fields", f32_twin), ("fields.a0_mode", mem("fields", a0_mode=7)),
    ("fields.nx = 0", mem("fields", nx=0)), ("fields.csize_au = 0", mem("fields", csize_au=0.0)),
    ("fields.d_ylo alone", ylo_only),
    ("compact without d_temp", mem("fields", d_a0=None, d_temp=None)),
    ("no complete layout", mem("fields", d_a0=None, d_em0=None, d_pf=None)),
    ("fields.d_temp NULL", mem("fields", d_temp=None)),
    ("fields.d_ts NULL", mem("fields", d_ts=None))] + GRAD_BURSTS + [
    ("h_ctau NULL", arg(h_ctau=None)), ("n_chan = 0", arg(n_chan=0)),
    ("2: all three outputs NULL", arg(d_ftot=None, d_dftot=None, d_dout=None)),
    ("n_epochs * n_chan * n_par", arg(n_chan=1 << 30)),
    ("d_work NULL", arg(d_work=None)), ("workspace one byte short", less("work_bytes")),
    ("2: fields.d_ts NULL, no burst",
     both(mem("fields", d_ts=None), lambda a: a.update(bursts=make_bursts([], [])))),
    ("2: non-finite burst parameter, h_csrc NULL", both(nan_burst, arg(h_csrc=None)))])
def _(e):
    assert 2 * 2 * 6 * e.P <= e.out[2].numel()
    return dict(ctx=e.eng.ctx, fields=e.fields(), bursts=e.new_bursts(), h_epochs_s=e.epochs,
                n_epochs=2, gff_mode=RJP_GFF_SCALAR, h_ctau=e.tab[0], h_csrc=e.tab[1], n_chan=2,
                d_ftot=ptr(e.out[0]), d_dftot=ptr(e.out[1]), d_dout=ptr(e.out[2]),
                d_work=ptr(e.work),
                work_bytes=e.need(e.lib.rjp_ff_formal_grad_workspace(*SHAPE, 2, 6, 2)))


VIS_NX = 200          # two row tiles: the valid call needs its workspace


@entry("rjp_vis", [
    ("d_maps NULL", arg(d_maps=None)), ("h_sv NULL", arg(h_sv=None)), ("d_u NULL", arg(d_u=None)),
    ("d_vis NULL", arg(d_vis=None)), ("n_maps = 0", arg(n_maps=0)), ("nz = 0", arg(nz=0)),
    ("n_vis = 0", arg(n_vis=0)),
    ("non-finite h_su", lambda a: a.update(h_su=_lib.dbl_array([1e-3, float("inf")]))),
    ("n_vis = 2^31 - 1", arg(n_vis=(1 << 31) - 1)),
    ("d_work NULL", arg(d_work=None)), ("workspace one byte short", less("work_bytes")),
    ("2: d_v NULL, n_vis = 0", arg(d_v=None, n_vis=0)),
    ("2: nx and n_vis = 2^31 - 1", arg(nx=(1 << 31) - 1, n_vis=(1 << 31) - 1)),
    ("2: non-finite h_su, n_vis = 2^31 - 1",
     lambda a: a.update(h_su=_lib.dbl_array([1e-3, float("inf")]), n_vis=(1 << 31) - 1))])
def _(e):
    assert 2 * VIS_NX * 4 <= e.out[0].numel()
    return dict(ctx=e.eng.ctx, d_maps=ptr(e.out[0]), n_maps=2, nx=VIS_NX, nz=4,
                h_su=_lib.dbl_array([1e-3, 2e-3]), h_sv=_lib.dbl_array([1e-3, -2e-3]),
                d_u=ptr(e.out[1]), d_v=ptr(e.out[2]), n_vis=3, d_vis=ptr(e.out[3]),
                d_work=ptr(e.work),
                work_bytes=e.need(e.lib.rjp_vis_workspace(2, VIS_NX, 4, 3)))


@entry("rjp_rrl_formal", [("gff_mode", arg(gff_mode=BAD_MODE))] +
       fields_cases(need_vy=True) + bursts_cases() + [
    ("line NULL", arg(line=None)), ("h_nu NULL", arg(h_nu=None)),
    ("h_hnu_k NULL", arg(h_hnu_k=None)), ("n_chan = 0", arg(n_chan=0)),
    ("d_out NULL", arg(d_out=None)),
    ("2: gff_mode, fields NULL", arg(gff_mode=BAD_MODE, fields=None)),
    ("2: fields.d_vy NULL, d_out NULL", both(mem("fields", d_vy=None), arg(d_out=None)))])
def _(e):
    return dict(ctx=e.eng.ctx, fields=e.fields(), bursts=e.new_bursts(), time_s=1.2 * YEAR,
                gff_mode=RJP_GFF_SCALAR, line=e.line, h_nu=e.nu, h_ctau=e.tab[0],
                h_csrc=e.tab[1], h_hnu_k=e.tab[2], n_chan=2, d_add=ptr(e.out[1]),
                d_out=ptr(e.out[0]))


@entry("rjp_rrl_maps", [
    ("d_tau_rrl NULL", arg(d_tau_rrl=None)), ("d_tavg NULL", arg(d_tavg=None)),
    ("h_hnu_k NULL", arg(h_hnu_k=None)), ("n_pix = 0", arg(n_pix=0)), ("n_chan = 0", arg(n_chan=0)),
    ("d_work NULL", arg(d_work=None)), ("workspace one byte short", less("work_bytes")),
    ("2: d_tau_ff NULL, n_pix = 0", arg(d_tau_ff=None, n_pix=0))])
def _(e):
    return dict(ctx=e.eng.ctx, d_tau_rrl=ptr(e.out[0]), d_tau_ff=ptr(e.out[1]),
                d_tavg=ptr(e.out[2]), d_flux_ff=ptr(e.out[3]), n_pix=e.P, h_cflux_rrl=e.tab[0],
                h_hnu_k=e.tab[2], n_chan=2, d_flux=ptr(e.out[4]), d_ftot=ptr(e.out[5]),
                d_work=ptr(e.work2),
                work_bytes=e.need(e.lib.rjp_ff_maps_workspace(e.P, 1, 2)))


# ---- producers -----------------------------------------------------------------------------------
def degenerate(a):
    """a - b = -(1 - q_v) / epsilon = -1: the connection formula's logarithmic case"""
    g = a["geometry"]
    g.qd_v = 0.5
    g.q_v = 1.0 - g.epsilon


@entry("rjp_build_fields", [
    ("geometry NULL", arg(geometry=None)), ("dtype", arg(dtype=16)),
    ("geometry.ny = 0", mem("geometry", ny=0)), ("geometry.csize = 0", mem("geometry", csize=0.0)),
    ("geometry.epsilon = 0", mem("geometry", epsilon=0.0)),
    ("geometry.mod_r_0 = 0", mem("geometry", mod_r_0=0.0)),
    ("d_a0 in f32 storage", arg(dtype=RJP_F32)), ("a0_mode", arg(a0_mode=BAD_MODE)),
    ("x-slab outside the grid", mem("geometry", ix0=4, nx_total=8)),
    ("geometry.ix0 < 0", mem("geometry", ix0=-1)),
    ("degenerate 2F1", degenerate),
    ("2: dtype, geometry NULL", arg(dtype=16, geometry=None)),
    ("2: geometry.epsilon = 0, a0_mode", both(mem("geometry", epsilon=0.0), arg(a0_mode=BAD_MODE))),
    ("2: degenerate 2F1, x-slab outside the grid",
     both(degenerate, mem("geometry", ix0=4, nx_total=8)))])
def _(e):
    o = [ptr(t) for t in e.out]
    return dict(ctx=e.eng.ctx, geometry=e.geometry(), dtype=RJP_F64, d_nd=o[0], d_xi=o[1],
                d_temp=o[2], d_pf=o[3], d_ts=o[4], d_vy=o[5], d_ff_raw=None, d_areas_raw=None,
                d_vx_raw=None, d_vz_raw=None, d_em0=o[6], d_a0=o[7],
                a0_mode=RJP_GFF_SCALAR)


@entry("rjp_synth_fields", [
    ("n = 0", arg(n=0)), ("nz = 0", arg(nz=0)), ("cell0 < 0", arg(cell0=-1)),
    ("dtype", arg(dtype=16)), ("d_a0 in f32 storage", arg(dtype=RJP_F32)),
    ("a0_mode", arg(a0_mode=BAD_MODE)), ("2: n = 0, dtype", arg(n=0, dtype=16))])
def _(e):
    o = [ptr(t) for t in e.out]
    return dict(ctx=e.eng.ctx, seed=SEED, temp_mode=0, nz=SHAPE[2], cell0=0, n=e.N,
                dtype=RJP_F64, d_nd=o[0], d_xi=o[1], d_temp=o[2], d_pf=o[3], d_ts=o[4],
                d_vy=o[5], d_em0=None, d_a0=o[6], a0_mode=RJP_GFF_SCALAR)


# ---- the runner ----------------------------------------------------------------------------------
def call(env, name, change=None):
    """One call of `name`: the valid arguments, `change` applied -> (status, message | None).
    The message is what rjp_last_error gives for the context THE CALL was handed (the
    context-less slot for a NULL context), None for the entry points that set none."""
    valid, _ = ENTRIES[name]
    a = valid(env)
    tail = a.pop("_tail", {})
    status_only = a.pop("_status_only", False)
    stream = () if a.pop("_no_stream", False) or name == "rjp_ctx_create" else (env.eng._stream(),)
    a["_env"] = env
    a.update(tail)                     # (arguments behind the stream: rjp_time_ff_scan)
    if change is not None:
        change(a)
    del a["_env"]
    vals = [v for k, v in a.items() if k not in tail] + list(stream) + [a[k] for k in tail]
    status = getattr(env.lib, name)(*vals)
    if name == "rjp_ctx_create" and status == _lib.RJP_OK:
        env.lib.rjp_ctx_destroy(a["out"])
    if status_only or status == _lib.RJP_OK:
        return int(status), None
    msg = env.lib.rjp_last_error(a.get("ctx"))
    return int(status), msg.decode() if msg is not None else None


def cases(name):
    """[(case name, change)] of an entry point: the NULL context first where it takes one"""
    valid, table = ENTRIES[name]
    names = [c for c, _ in table]
    assert len(set(names)) == len(names), name
    if name == "rjp_ctx_create" or "ctx NULL" in names:
        return list(table)
    return [("ctx NULL", arg(ctx=None))] + list(table)
