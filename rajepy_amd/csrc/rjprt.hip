// librjprt.so -- C-ABI entry points (include/rjprt.h) over the gfx950 kernels.
// The kernels live in their own translation units (ff_scan*.hip, fields.hip, rrl_scan.hip;
// csrc/Makefile builds them in parallel); rjp_host.h declares their launch wrappers.
// The argument checks that are pure functions of the caller's structs live in rjp_args.h.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rjp_args.h"
#include "rjp_host.h"

struct rjp_ctx {
  int device = -1;
  std::string err;
  // small per-call tables (channel coefficients, frequencies): a ring of pinned host
  // staging buffers + device copies, grown on demand; the copies are ordered on the
  // caller's stream and a slot is overwritten only after its readers have finished.  A call
  // whose tables equal a slot's content (a sweep over epochs at a fixed channel list) reuses
  // the device copy: no host-to-device copy between the scan and the map stage.
  rjp::MomPlan mom;               // last moment-path request (its tables are reused)
  rjp::ChiPlan chi;               // the burst-factor table of the last single-epoch scan
  rjp::TabRing tabs;              // its table slots and the side stream that fills them
  int last_path = 0;              // 0 = epoch tiles, 1 = LDS moments, 2 = launch-time-ordered layout
  int last_layout = 0;            // 0 = grid order, 1 = launch-time-bucketed layout (rjp_last_scan_layout)
  bool last_srt_mom = false;      // the last scan contracted bins from the layout's moments
  // (e0, et, uniform, nsplit, vec) of every epoch tile the last scan launched (rjp_last_scan_tiles);
  // empty after a scan on another path
  std::vector<int32_t> last_tiles;
  // (kernel, VEC, KP, blocks, nparts, fchunk) of the last map stage (rjp_last_maps_launch);
  // kernel -1 before the first
  int32_t last_maps[6] = {-1, 0, 0, 0, 0, 0};
  static constexpr int kSlots = 8;
  struct Slot {
    double* h = nullptr;
    double* d = nullptr;
    size_t cap = 0;               // doubles
    size_t used = 0;              // doubles of valid content (0 = none)
    hipStream_t up_stream = nullptr;   // stream the content was uploaded on
    bool side_seen = false;       // the table ring's side stream is ordered behind the upload
    bool fresh = false;           // uploaded by the call in progress
    bool hot = false;             // read by calls whose end no record of free_ev covers
    hipEvent_t free_ev = nullptr; // recorded after the last kernel that reads `d`
  } slot[kSlots];
  int next_slot = 0;
  int cur_slot = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // Launch-time range guard (include/rjprt.h): one int in pinned, device-visible host memory.
  // Kernels that bin or tabulate by launch time store 1 into it when they meet a finite launch
  // time outside rjp_fields.ts_lo / ts_hi (and poison that sightline's sums with NaN); the next
  // entry point of the context reports it.  `range_ok`: the ranges rjp_ff_scan has already
  // checked against their launch-time field with a pass of its own (most recent first).
  int* guard = nullptr;
  unsigned long long* d_count = nullptr;      // device word of rjp_occupied_cells
  unsigned long long* d_srt_hist = nullptr;   // RJP_SRT_MAX_K * 2 counters of rjp_srt_count
  // (contracted, read, residual) bins of rjp_last_srt_bins / rjp_last_srt_resid and the fallback
  // cells of rjp_last_srt_fallbacks: kSrtDiagWords words per group of 64 sightlines, written
  // by the group's wave with plain stores (ff_scan_hybrid_kernel); grown when a scan has more
  // groups than it holds.  `srt_diag_groups`: the groups the last such scan wrote.
  unsigned long long* d_srt_diag = nullptr;
  int64_t srt_diag_cap = 0, srt_diag_groups = 0;
  struct RangeKey {
    const void* d_ts = nullptr;
    int64_t n = 0;
    int dtype = 0;
    double lo = 0.0, hi = 0.0;
  } range_ok[4];
};

static std::string g_create_err;

static int fail(rjp_ctx* ctx, int code, const char* what, hipError_t e = hipSuccess) {
  std::string m = what;
  if (e != hipSuccess) {
    m += ": ";
    m += hipGetErrorString(e);
  }
  if (ctx) ctx->err = m; else g_create_err = m;
  return code;
}

#define RJP_HIP(ctx, call)                                              \
  do {                                                                  \
    hipError_t _e = (call);                                             \
    if (_e != hipSuccess) return fail((ctx), RJP_ERR_HIP, #call, _e);   \
  } while (0)

static const char* const kGuardMsg =
    "an earlier scan of this context met finite launch times outside fields.ts_lo / ts_hi: the "
    "sums of those sightlines were set to NaN (pass what rjp_field_range returns for d_ts, or "
    "zeros)";

// Reads and clears the range guard; true: it was raised.  `void_ranges`: what raised it was an
// earlier, asynchronous scan, so the ranges check_ts_range has passed are void with it.
static bool take_guard(rjp_ctx* ctx, bool void_ranges) {
  if (*(volatile int*)ctx->guard == 0) return false;
  *(volatile int*)ctx->guard = 0;
  if (void_ranges)
    for (auto& k : ctx->range_ok) k = rjp_ctx::RangeKey();
  return true;
}

static int bind(rjp_ctx* ctx) {
  if (!ctx) return fail(nullptr, RJP_ERR_ARG, "null context");
  hipError_t e = hipSetDevice(ctx->device);
  if (e != hipSuccess) return fail(ctx, RJP_ERR_HIP, "hipSetDevice", e);
  // the range guard is sticky until reported once (a kernel of an earlier, asynchronous call
  // raised it; whatever this call would enqueue is refused)
  if (ctx->guard && take_guard(ctx, true)) return fail(ctx, RJP_ERR_ARG, kGuardMsg);
  return RJP_OK;
}

// A scan is about to bin / tabulate by launch time on the strength of fields.ts_lo / ts_hi: a
// range this context has not seen with this launch-time field is CHECKED first -- one pass over
// d_ts (8 B/cell: 1.3 ms for 1.07e9 cells) and one stream synchronisation, once per model -- so
// that a wrong range is refused by the very call that passes it, before anything else is
// enqueued.  (Later content changes under the same pointer are caught by the kernels' guard.)
static int check_ts_range(rjp_ctx* ctx, const rjp_fields* f, hipStream_t st) {
  const int64_t n = (int64_t)f->nx * f->ny * f->nz;
  for (const auto& k : ctx->range_ok)
    if (k.d_ts == f->d_ts && k.n == n && k.dtype == f->dtype && k.lo == f->ts_lo && k.hi == f->ts_hi)
      return RJP_OK;
  RJP_HIP(ctx, rjp::range_check_launch(f->d_ts, n, f->dtype, f->ts_lo, f->ts_hi, ctx->guard, st));
  RJP_HIP(ctx, hipStreamSynchronize(st));
  if (take_guard(ctx, false))
    return fail(ctx, RJP_ERR_ARG,
                "fields.ts_lo / ts_hi do not contain every finite launch time of fields.d_ts "
                "(pass what rjp_field_range returns for it, or zeros); nothing was enqueued");
  for (int i = 3; i > 0; --i) ctx->range_ok[i] = ctx->range_ok[i - 1];
  ctx->range_ok[0].d_ts = f->d_ts; ctx->range_ok[0].n = n; ctx->range_ok[0].dtype = f->dtype;
  ctx->range_ok[0].lo = f->ts_lo; ctx->range_ok[0].hi = f->ts_hi;
  return RJP_OK;
}

// Stage small host tables into one slot of the context's table ring and return device
// pointers (the first half of staged(), which records the slot's release event).
static int stage_tables(rjp_ctx* ctx, hipStream_t st, const double* const* src,
                        const size_t* len, int ntab, double** dev_out) {
  size_t tot = 0;
  for (int i = 0; i < ntab; ++i) tot += len[i];
  for (int k = 0; k < rjp_ctx::kSlots; ++k) {
    rjp_ctx::Slot& c = ctx->slot[k];
    if (c.used != tot || c.up_stream != st || tot == 0) continue;
    size_t off = 0;
    bool same = true;
    for (int i = 0; i < ntab && same; ++i) {
      same = memcmp(c.h + off, src[i], len[i] * sizeof(double)) == 0;
      off += len[i];
    }
    if (!same) continue;
    off = 0;
    for (int i = 0; i < ntab; ++i) { dev_out[i] = c.d + off; off += len[i]; }
    c.fresh = false;
    ctx->cur_slot = k;
    return RJP_OK;
  }
  // the next slot of the ring that is not hot (a hot slot's readers are covered by no record: it
  // is kept, its content is in use call after call); all hot: the device is drained once
  int pick = -1;
  for (int k = 0; k < rjp_ctx::kSlots && pick < 0; ++k)
    if (!ctx->slot[(ctx->next_slot + k) % rjp_ctx::kSlots].hot) pick = (ctx->next_slot + k) % rjp_ctx::kSlots;
  if (pick < 0) {
    RJP_HIP(ctx, hipDeviceSynchronize());
    for (auto& c : ctx->slot) c.hot = false;
    pick = ctx->next_slot;
  }
  rjp_ctx::Slot& sl = ctx->slot[pick];
  ctx->cur_slot = pick;
  ctx->next_slot = (pick + 1) % rjp_ctx::kSlots;
  RJP_HIP(ctx, hipEventSynchronize(sl.free_ev));     // no-op unless its readers still run
  sl.used = 0;
  if (tot > sl.cap) {
    if (sl.h) RJP_HIP(ctx, hipHostFree(sl.h));
    if (sl.d) RJP_HIP(ctx, hipFree(sl.d));
    sl.h = nullptr; sl.d = nullptr; sl.cap = 0;
    const size_t cap = tot < 4096 ? 4096 : tot * 2;
    RJP_HIP(ctx, hipHostMalloc((void**)&sl.h, cap * sizeof(double), hipHostMallocDefault));
    RJP_HIP(ctx, hipMalloc((void**)&sl.d, cap * sizeof(double)));
    sl.cap = cap;
  }
  size_t off = 0;
  for (int i = 0; i < ntab; ++i) {
    if (len[i]) memcpy(sl.h + off, src[i], len[i] * sizeof(double));
    dev_out[i] = sl.d + off;
    off += len[i];
  }
  RJP_HIP(ctx, hipMemcpyAsync(sl.d, sl.h, tot * sizeof(double), hipMemcpyHostToDevice, st));
  sl.used = tot;
  sl.up_stream = st;
  sl.side_seen = false;
  sl.fresh = true;
  return RJP_OK;
}

// A small host table of a call
struct Tab {
  const double* p;
  size_t n;       // doubles
};
constexpr int kMaxTabs = 5;
constexpr int kMaxScale = 1 + 6 * RJP_SGPR_BURSTS;   // the chain-rule table of a sensitivity call

// A call that reads small host tables on the device: stages up to kMaxTabs of them (a slot
// whose content on this stream equals them is reused without an upload), runs
// `launch(dev, d_ext)` -> hipError_t with their device copies in the order given, and records
// the slot's release event on EVERY path -- after a failed launch too, since the slot's upload
// (and anything enqueued before the failure) may still be in flight when the ring comes round to
// it again.  An event record holds the stream up for about 6 us between two kernels, so a call
// that REUSED a slot records nothing unless `release` asks for it (chi_table_scan's, whose table
// ring borrows the event): the slot is marked hot instead, and the ring passes hot slots over
// (stage_tables).  `bursts`: the parameters of a single-epoch call's bursts beyond RJP_SGPR_BURSTS
// travel as one more table, `d_ext` (nullptr when no jet has that many; always so without
// `bursts`).  No heap allocation unless there are such bursts.
template <class Launch>
static int staged(rjp_ctx* ctx, hipStream_t st, const char* what, const rjp_bursts* bursts,
                  std::initializer_list<Tab> tabs, Launch&& launch, bool release = false) {
  const double* src[kMaxTabs];
  size_t len[kMaxTabs];
  double* dev[kMaxTabs];
  int n = 0;
  if (tabs.size() + (bursts ? 1 : 0) > (size_t)kMaxTabs)   // (a slip in this file, no caller's)
    return fail(ctx, RJP_ERR_ARG, "staged: more tables than one call stages");
  for (const Tab& t : tabs) { src[n] = t.p; len[n++] = t.n; }
  // host image of the overflow-burst table (parameters only)
  std::vector<double> ext(bursts_ext_doubles(bursts), 0.0);
  if (!ext.empty()) {
    bursts_fill_ext(bursts, ext.data());
    src[n] = ext.data();
    len[n++] = ext.size();
  }
  if (int r = stage_tables(ctx, st, src, len, n, dev)) return r;
  const hipError_t e = launch(dev, ext.empty() ? nullptr : dev[n - 1]);
  rjp_ctx::Slot& sl = ctx->slot[ctx->cur_slot];
  hipError_t rel = hipSuccess;
  if (sl.fresh || release) {
    rel = hipEventRecord(sl.free_ev, st);
    sl.hot = false;
  } else {
    sl.hot = true;
  }
  if (e != hipSuccess) return fail(ctx, RJP_ERR_HIP, what, e);
  if (rel != hipSuccess)
    return fail(ctx, RJP_ERR_HIP, "hipEventRecord(ctx->slot[ctx->cur_slot].free_ev, st)", rel);
  return RJP_OK;
}

using rjp_args::mode_ok;

// rjp_args.h's checks with their message routed into fail()
template <class Check>
static int checked(rjp_ctx* ctx, Check&& check) {
  std::string m;
  const int r = check(m);
  return r ? fail(ctx, r, m.c_str()) : RJP_OK;
}

static int check_fields(rjp_ctx* ctx, const rjp_fields* f, bool need_vy, bool compact_ok = false,
                        int tau_mode = -1) {
  return checked(ctx, [&](std::string& m) {
    return rjp_args::check_fields(f, need_vy, compact_ok, tau_mode, m);
  });
}

static int check_bursts(rjp_ctx* ctx, const rjp_bursts* b, const rjp_fields* f) {
  return checked(ctx, [&](std::string& m) { return rjp_args::check_bursts(b, f, m); });
}

static int check_grid(rjp_ctx* ctx, const rjp_fields* f, bool y_pair) {
  return checked(ctx, [&](std::string& m) { return rjp_args::check_grid(f, y_pair, m); });
}

extern "C" {

int rjp_version(void) { return RJP_VERSION; }

int rjp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int rjp_ctx_create(int device, rjp_ctx** out) {
  if (!out) return fail(nullptr, RJP_ERR_ARG, "out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(nullptr, RJP_ERR_NODEVICE, "no HIP device visible", e);
  if (device < 0 || device >= n) return fail(nullptr, RJP_ERR_ARG, "device index out of range");
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) return fail(nullptr, RJP_ERR_HIP, "hipGetDeviceProperties", e);
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    std::string m = std::string("librjprt is built for gfx950 only; device is ") + prop.gcnArchName;
    return fail(nullptr, RJP_ERR_NODEVICE, m.c_str());
  }
  e = hipSetDevice(device);
  if (e != hipSuccess) return fail(nullptr, RJP_ERR_HIP, "hipSetDevice", e);
  rjp_ctx* c = new rjp_ctx();
  c->device = device;
  bool ok = hipEventCreate(&c->ev0) == hipSuccess && hipEventCreate(&c->ev1) == hipSuccess;
  for (int i = 0; ok && i < rjp_ctx::kSlots; ++i)
    ok = hipEventCreateWithFlags(&c->slot[i].free_ev, hipEventDisableTiming) == hipSuccess;
  ok = ok && hipHostMalloc((void**)&c->guard, sizeof(int), hipHostMallocDefault) == hipSuccess;
  if (!ok) {
    if (c->guard) (void)hipHostFree(c->guard);
    delete c;
    return fail(nullptr, RJP_ERR_HIP, "hipEventCreate / hipHostMalloc failed");
  }
  *c->guard = 0;
  rjp::tab_ring_create(c->tabs);
  *out = c;
  return RJP_OK;
}

int rjp_ctx_destroy(rjp_ctx* ctx) {
  if (!ctx) return RJP_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  for (auto& sl : ctx->slot) {
    if (sl.h) (void)hipHostFree(sl.h);
    if (sl.d) (void)hipFree(sl.d);
    if (sl.free_ev) (void)hipEventDestroy(sl.free_ev);
  }
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->guard) (void)hipHostFree(ctx->guard);
  if (ctx->d_count) (void)hipFree(ctx->d_count);
  if (ctx->d_srt_hist) (void)hipFree(ctx->d_srt_hist);
  if (ctx->d_srt_diag) (void)hipFree(ctx->d_srt_diag);
  rjp::tab_ring_destroy(ctx->tabs);
  rjp::moments_release(ctx->mom);
  delete ctx;
  return RJP_OK;
}

const char* rjp_last_error(const rjp_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_create_err.c_str();
}

int rjp_pack_field(rjp_ctx* ctx, const double* d_src, const double* d_den,
                   const uint8_t* d_red, void* d_dst, int64_t n, int dtype, void* stream) {
  if (int r = bind(ctx)) return r;
  if (!d_src || !d_dst || n <= 0) return fail(ctx, RJP_ERR_ARG, "rjp_pack_field: bad pointers/size");
  if (dtype != RJP_F32 && dtype != RJP_F64) return fail(ctx, RJP_ERR_ARG, "bad dtype tag");
  RJP_HIP(ctx, rjp::pack_field_launch(d_src, d_den, d_red, d_dst, n, dtype, (hipStream_t)stream));
  return RJP_OK;
}

int rjp_compact_fields(rjp_ctx* ctx, const rjp_fields* fields, void* d_em0, int64_t* d_n_bad,
                       void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = check_fields(ctx, fields, false)) return r;
  if (!d_em0 || !d_n_bad) return fail(ctx, RJP_ERR_ARG, "rjp_compact_fields: NULL output");
  RJP_HIP(ctx, rjp::compact_fields_launch(fields, d_em0, d_n_bad, (hipStream_t)stream));
  return RJP_OK;
}

int rjp_tau_field(rjp_ctx* ctx, const rjp_fields* fields, int32_t gff_mode, void* d_a0,
                  void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = check_fields(ctx, fields, false, true)) return r;
  if (!mode_ok(gff_mode)) return fail(ctx, RJP_ERR_ARG, "bad gff_mode");
  if (fields->dtype != RJP_F64 || !fields->d_em0)
    return fail(ctx, RJP_ERR_ARG, "rjp_tau_field: needs RJP_F64 storage with the compact field "
                                  "d_em0 attached");
  if (!d_a0) return fail(ctx, RJP_ERR_ARG, "rjp_tau_field: NULL output");
  RJP_HIP(ctx, rjp::tau_field_launch(fields, gff_mode, d_a0, (hipStream_t)stream));
  return RJP_OK;
}

int rjp_unmask_launch_times(rjp_ctx* ctx, const rjp_fields* fields, int32_t jet, void* d_ts_out,
                            void* stream) {
  if (int r = bind(ctx)) return r;
  if (!fields || !fields->d_ts || !d_ts_out)
    return fail(ctx, RJP_ERR_ARG, "rjp_unmask_launch_times: fields.d_ts / d_ts_out is NULL");
  if (int r = check_grid(ctx, fields, false)) return r;
  if (jet != 0 && jet != 1) return fail(ctx, RJP_ERR_ARG, "jet must be 0 (red) or 1 (blue)");
  if (!fields->d_a0 && !fields->d_em0 && !fields->d_nd)
    return fail(ctx, RJP_ERR_ARG, "rjp_unmask_launch_times: needs a field that carries the jet "
                                  "flag (d_a0, d_em0 or d_nd)");
  RJP_HIP(ctx, rjp::unmask_ts_launch(fields, jet, d_ts_out, (hipStream_t)stream));
  return RJP_OK;
}

int rjp_field_range(rjp_ctx* ctx, const void* d_field, int64_t n, int dtype, double* d_partials,
                    void* stream) {
  if (int r = bind(ctx)) return r;
  if (!d_field || !d_partials || n <= 0) return fail(ctx, RJP_ERR_ARG, "rjp_field_range: bad pointers/size");
  if (dtype != RJP_F32 && dtype != RJP_F64) return fail(ctx, RJP_ERR_ARG, "bad dtype tag");
  RJP_HIP(ctx, rjp::field_range_launch(d_field, n, dtype, d_partials, (hipStream_t)stream));
  return RJP_OK;
}

int rjp_tavg(rjp_ctx* ctx, const rjp_fields* fields, double* d_tavg, void* d_work,
             size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (!fields || !fields->d_temp) return fail(ctx, RJP_ERR_ARG, "rjp_tavg: fields.d_temp is NULL");
  if (int r = check_grid(ctx, fields, true)) return r;
  if (!d_tavg || !d_work) return fail(ctx, RJP_ERR_ARG, "rjp_tavg: d_tavg / d_work is NULL");
  if (work_bytes < rjp::ff_scan_workspace_bytes(fields->nx, fields->ny, fields->nz, 1))
    return fail(ctx, RJP_ERR_WORKSPACE, "rjp_tavg: workspace smaller than rjp_ff_scan_workspace(.., 1)");
  RJP_HIP(ctx, rjp::tavg_launch(fields, d_tavg, (double*)d_work, (hipStream_t)stream));
  return RJP_OK;
}

int rjp_y_bounds(rjp_ctx* ctx, const rjp_fields* fields, int32_t* d_ylo, int32_t* d_yhi,
                 void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = check_fields(ctx, fields, false, true)) return r;
  if (!d_ylo || !d_yhi) return fail(ctx, RJP_ERR_ARG, "rjp_y_bounds: NULL output");
  RJP_HIP(ctx, rjp::y_bounds_launch(fields, d_ylo, d_yhi, (hipStream_t)stream));
  return RJP_OK;
}

size_t rjp_ff_scan_workspace(int32_t nx, int32_t ny, int32_t nz, int32_t n_epochs) {
  if (nx <= 0 || ny <= 0 || nz <= 0) return 0;
  return rjp::ff_scan_workspace_bytes(nx, ny, nz, n_epochs);
}

int rjp_occupied_cells(rjp_ctx* ctx, const int32_t* d_ylo, const int32_t* d_yhi, int64_t n_pix,
                       int64_t* h_count, void* stream) {
  if (int r = bind(ctx)) return r;
  if (!d_ylo || !d_yhi || !h_count || n_pix <= 0)
    return fail(ctx, RJP_ERR_ARG, "rjp_occupied_cells: NULL argument or n_pix <= 0");
  hipStream_t st = (hipStream_t)stream;
  if (!ctx->d_count) RJP_HIP(ctx, hipMalloc((void**)&ctx->d_count, sizeof(unsigned long long)));
  RJP_HIP(ctx, hipMemsetAsync(ctx->d_count, 0, sizeof(unsigned long long), st));
  RJP_HIP(ctx, rjp::occupied_launch(d_ylo, d_yhi, n_pix, ctx->d_count, st));
  unsigned long long v = 0;
  RJP_HIP(ctx, hipMemcpyAsync(&v, ctx->d_count, sizeof(v), hipMemcpyDeviceToHost, st));
  RJP_HIP(ctx, hipStreamSynchronize(st));
  *h_count = (int64_t)v;
  return RJP_OK;
}

// (the body of rjp_ff_scan; also the first half of rjp_ff_step)
static int ff_scan_impl(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                        const double* h_epochs_s, int32_t n_epochs, int32_t gff_mode,
                        double* d_sumA, double* d_em, double* d_tavg, void* d_work,
                        size_t work_bytes, void* stream) {
  if (!mode_ok(gff_mode)) return fail(ctx, RJP_ERR_ARG, "bad gff_mode");
  if (int r = check_fields(ctx, fields, false, true, gff_mode)) return r;
  if (int r = check_bursts(ctx, bursts, fields)) return r;
  if (!h_epochs_s || n_epochs < 1) return fail(ctx, RJP_ERR_ARG, "need >= 1 epoch");
  if (!d_sumA || !d_work) return fail(ctx, RJP_ERR_ARG, "d_sumA / d_work is NULL");
  // check_fields accepted the call on the strength of ONE complete layout; the layout the scan
  // really takes depends on what is asked for (d_em moves a tau-only field set to the compact
  // or wide kernels): every pointer THAT layout dereferences must be there
  switch (rjp::scan_layout(fields, gff_mode, d_em != nullptr)) {
    case rjp::LAY_TAU:
      if (d_tavg && !fields->d_temp)
        return fail(ctx, RJP_ERR_ARG, "rjp_ff_scan: fields hold the tau layout only; d_tavg needs "
                                      "fields.d_temp");
      break;
    case rjp::LAY_CMP:
      if (!fields->d_temp)
        return fail(ctx, RJP_ERR_ARG, "rjp_ff_scan: the compact layout needs fields.d_temp");
      break;
    default:
      if (!fields->d_nd || !fields->d_xi || !fields->d_temp || !fields->d_pf)
        return fail(ctx, RJP_ERR_ARG,
                    d_em ? "rjp_ff_scan: d_em needs fields.d_em0 or the complete wide set "
                           "(nd, xi, temp, pf); these fields hold the tau layout only"
                         : "rjp_ff_scan: fields nd/xi/temp/pf must be device pointers");
  }
  if (work_bytes < rjp::ff_scan_workspace_bytes(fields->nx, fields->ny, fields->nz, n_epochs))
    return fail(ctx, RJP_ERR_WORKSPACE, "rjp_ff_scan: workspace smaller than rjp_ff_scan_workspace()");
  hipStream_t st = (hipStream_t)stream;
  ctx->last_layout = 0;
  ctx->last_srt_mom = false;
  ctx->last_tiles.clear();
  // epoch sweeps by launch-time moments (ff_moments.hip) when the caller provided the launch-time
  // range and the host-side accuracy check of the expansion passes
  const int mr = rjp::moments_plan(fields, bursts, h_epochs_s, n_epochs, gff_mode, d_em != nullptr,
                                   work_bytes, ctx->mom);
  if (mr) {
    if (int r = check_ts_range(ctx, fields, st)) return r;
  }
  if (mr == 2) {
    // a new (bursts, epochs) request: its coefficient tables are built and checked on the device
    const auto t0 = std::chrono::steady_clock::now();
    if (int r = staged(ctx, st, "moments_build", nullptr,
                       {{ctx->mom.stage.data(), ctx->mom.stage.size()}},
                       [&](double* const* d, const double*) {
                         return rjp::moments_build(ctx->mom, d[0], st);
                       }))
      return r;
    ctx->mom.build_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  if (mr && ctx->mom.ok) {
    if (d_tavg) {
      if (!fields->d_temp)
        return fail(ctx, RJP_ERR_ARG, "rjp_ff_scan: d_tavg on the tau layout needs fields.d_temp");
      RJP_HIP(ctx, rjp::tavg_launch(fields, d_tavg, (double*)d_work, st));
    }
    ctx->last_path = ctx->mom.path;
    if (ctx->mom.path == 2) {
      RJP_HIP(ctx, rjp::lt_run(fields, ctx->mom, n_epochs, d_sumA, (double*)d_work, work_bytes, st));
      return RJP_OK;
    }
    // the moment maps of a0 are model state (they depend on the launch-time bins and on which
    // jets have bursts, not on the epochs or the burst parameters): a caller-kept cache of the
    // selected shape replaces the pass over the grid; an empty or differently shaped one is
    // filled by this call
    double* mbuf = (double*)d_work;
    bool cached = false;
    if (fields->d_mom_cache && !d_em) {
      mbuf = fields->d_mom_cache;
      cached = fields->mom_cache_K == ctx->mom.K && fields->mom_cache_N == ctx->mom.N;
    }
    if (cached) ctx->last_path = 4;
    // (the chunk sums of a small map's split contraction: behind the moment maps' room in the
    // workspace -- moments_plan has checked that the workspace holds both)
    const int64_t npix_ = (int64_t)fields->nx * fields->nz;
    double* part = nullptr;
    if (rjp::moments_scan_workspace_bytes(npix_) > rjp::moments_workspace_bytes(npix_) &&
        work_bytes >= rjp::moments_scan_workspace_bytes(npix_))
      part = (double*)((char*)d_work + rjp::moments_workspace_bytes(npix_));
    hipError_t e = rjp::moments_run(fields, ctx->mom, n_epochs, d_sumA, mbuf, part, st,
                                    (const double*)fields->d_a0, 1.0, ctx->guard, cached);
    if (e == hipSuccess && d_em) {
      // the emission measure of every epoch: the same pass and tables with em0 as the weight
      // (em = sum (n x)^2 * csize*au/pc * pf, classes.py:1116-1118)
      const double em_scale = fields->csize_au * 149597870700.0 / 3.085677581491367e+16;
      e = rjp::moments_run(fields, ctx->mom, n_epochs, d_em, (double*)d_work, part, st,
                           (const double*)fields->d_em0, em_scale, ctx->guard);
    }
    if (e != hipSuccess) return fail(ctx, RJP_ERR_HIP, "moments_run", e);
    return RJP_OK;
  }
  if (rjp::chi_table_plan(fields, bursts, h_epochs_s, n_epochs, gff_mode, d_em != nullptr,
                          work_bytes, ctx->chi) &&
      (d_tavg == nullptr || ctx->chi.wide)) {      // (T_avg with the scan: the wide kernel only)
    // single epoch on the tau layout: the burst factor from a table in LDS (ff_scan_tab.hip)
    if (int r = check_ts_range(ctx, fields, st)) return r;
    ctx->last_path = 3;
    // ... reading only the launch-time bins inside the bursts' support when the caller attached
    // the bucketed layout and the epoch leaves enough of it out
    rjp::SrtPlan sp;
    const bool srt = !ctx->chi.wide && !d_em && rjp::srt_plan(fields, bursts, h_epochs_s[0], sp);
    ctx->last_layout = srt ? 1 : 0;
    if (srt && sp.N > 0) {
      // the bin counters of rjp_last_srt_bins, a pair per group: every pair is stored by the scan
      // itself, so nothing is zeroed.  Growing it (a larger map than any before on this context)
      // costs a hipFree, which synchronises the whole device and so also waits for a scan that
      // still writes the old buffer: accepted for a diagnostic, it happens once per map size
      const int64_t groups = ((int64_t)fields->nx * fields->nz + 63) / 64;
      if (groups > ctx->srt_diag_cap) {
        if (ctx->d_srt_diag) RJP_HIP(ctx, hipFree(ctx->d_srt_diag));
        ctx->d_srt_diag = nullptr;
        ctx->srt_diag_cap = 0;
        RJP_HIP(ctx, hipMalloc((void**)&ctx->d_srt_diag,
                               (size_t)groups * rjp::kSrtDiagWords * sizeof(unsigned long long)));
        ctx->srt_diag_cap = groups;
      }
      ctx->srt_diag_groups = groups;
      sp.diag = ctx->d_srt_diag;
      ctx->last_srt_mom = true;
    }
    return staged(ctx, st, "chi_table_scan", nullptr,
                  {{ctx->chi.stage.data(), ctx->chi.stage.size()}},
                  [&](double* const* d, const double*) {
                    bool fresh = !ctx->slot[ctx->cur_slot].side_seen;
                    const hipError_t e = rjp::chi_table_scan(
                        fields, ctx->chi, d[0], h_epochs_s[0], gff_mode, d_sumA, d_em, d_tavg,
                        (double*)d_work, work_bytes, ctx->guard, st, srt ? &sp : nullptr,
                        &ctx->tabs, &fresh, ctx->slot[ctx->cur_slot].free_ev);
                    ctx->slot[ctx->cur_slot].side_seen = !fresh;
                    return e;
                  }, true);
  }
  ctx->last_path = 0;
  rjp::ScanPlan plan;
  rjp::ff_scan_plan(fields, bursts, h_epochs_s, n_epochs, gff_mode, d_em != nullptr, plan);
  for (const rjp::ScanTile& tl : plan.tiles) {
    // (tiles of >= 16 epochs run one sightline per lane: ff_scan_run)
    const int32_t row[5] = {tl.e0, tl.et, tl.un.on, tl.nsplit, tl.et < 16 ? plan.vec : 1};
    ctx->last_tiles.insert(ctx->last_tiles.end(), row, row + 5);
  }
  auto run = [&](const double* d_ext) {
    return rjp::ff_scan_run(fields, bursts, plan, d_ext, h_epochs_s, n_epochs, gff_mode, d_sumA,
                            d_em, d_tavg, (double*)d_work, st);
  };
  // (the plan's own overflow table: the bursts' parameters and the tiles' constants in one)
  if (!plan.ext.empty())
    return staged(ctx, st, "ff_scan_run", nullptr, {{plan.ext.data(), plan.ext.size()}},
                  [&](double* const* d, const double*) { return run(d[0]); });
  const hipError_t e = run(nullptr);
  if (e != hipSuccess) return fail(ctx, RJP_ERR_HIP, "ff_scan_run", e);
  return RJP_OK;
}

int rjp_ff_scan(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                const double* h_epochs_s, int32_t n_epochs, int32_t gff_mode, double* d_sumA,
                double* d_em, double* d_tavg, void* d_work, size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  return ff_scan_impl(ctx, fields, bursts, h_epochs_s, n_epochs, gff_mode, d_sumA, d_em, d_tavg,
                      d_work, work_bytes, stream);
}

int rjp_range_guard(rjp_ctx* ctx) {
  if (!ctx || !ctx->guard) return RJP_ERR_ARG;
  if (!take_guard(ctx, true)) return 0;
  ctx->err = kGuardMsg;
  return 1;
}

int rjp_last_scan_path(const rjp_ctx* ctx, double* worst_rel_err, int32_t* moment_shape) {
  if (!ctx) return RJP_ERR_ARG;
  const bool mom = ctx->last_path == 1 || ctx->last_path == 2 || ctx->last_path == 4;
  if (worst_rel_err) *worst_rel_err = mom ? ctx->mom.worst : ctx->last_path == 3 ? 2e-13 : 0.0;
  if (moment_shape) {
    // (path 3: the table's intervals per jet and its polynomial degree + 1)
    moment_shape[0] = mom ? ctx->mom.K : ctx->last_path == 3 ? ctx->chi.ni : 0;
    moment_shape[1] = mom ? ctx->mom.N : ctx->last_path == 3 ? 8 : 0;
  }
  return ctx->last_path;
}

int rjp_last_scan_tiles(const rjp_ctx* ctx, int32_t* n_tiles, int32_t* tiles, int32_t cap) {
  if (!ctx || !n_tiles || cap < 0 || (cap > 0 && !tiles)) return RJP_ERR_ARG;
  const int32_t n = (int32_t)(ctx->last_tiles.size() / 5);
  *n_tiles = n;
  if (n > cap) return RJP_ERR_ARG;
  for (size_t i = 0; i < ctx->last_tiles.size(); ++i) tiles[i] = ctx->last_tiles[i];
  return RJP_OK;
}

int rjp_last_scan_layout(const rjp_ctx* ctx) { return ctx ? ctx->last_layout : RJP_ERR_ARG; }

int rjp_last_maps_launch(const rjp_ctx* ctx, int32_t out[6]) {
  if (!ctx || !out) return RJP_ERR_ARG;
  for (int i = 0; i < 6; ++i) out[i] = ctx->last_maps[i];
  return RJP_OK;
}

int rjp_last_srt_bins(rjp_ctx* ctx, int64_t* contracted, int64_t* read) {
  if (int r = bind(ctx)) return r;
  if (!contracted || !read) return fail(ctx, RJP_ERR_ARG, "rjp_last_srt_bins: NULL output");
  *contracted = *read = 0;
  if (!ctx->last_srt_mom) return RJP_OK;
  std::vector<unsigned long long> h((size_t)ctx->srt_diag_groups * rjp::kSrtDiagWords);
  RJP_HIP(ctx, hipDeviceSynchronize());
  RJP_HIP(ctx, hipMemcpy(h.data(), ctx->d_srt_diag, h.size() * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost));
  int64_t con = 0, rd = 0;
  for (size_t g = 0; g < h.size(); g += rjp::kSrtDiagWords) {
    con += (int64_t)h[g];
    rd += (int64_t)h[g + 1];
  }
  *contracted = con;
  *read = rd;
  return RJP_OK;
}

double rjp_last_table_build_ms(const rjp_ctx* ctx) { return ctx ? ctx->mom.build_ms : 0.0; }

size_t rjp_moment_cache_bytes(int32_t nx, int32_t nz) {
  if (nx <= 0 || nz <= 0) return 0;
  return rjp::moments_workspace_bytes((int64_t)nx * nz);
}

size_t rjp_lt_rowoff_entries(int32_t nx, int32_t nz, int32_t K) {
  if (nx <= 0 || nz <= 0 || K < 1 || K > RJP_LT_MAX_K) return 0;
  return rjp::lt_rowoff_entries(nx, nz, K);
}

static int check_lt(rjp_ctx* ctx, const rjp_fields* f, int32_t K) {
  return checked(ctx, [&](std::string& m) {
    return rjp_args::check_layout(f, K, "launch-time-ordered layout", RJP_LT_MAX_K, 65536, m);
  });
}

int rjp_lt_count(rjp_ctx* ctx, const rjp_fields* fields, int32_t K, int32_t* d_rowoff,
                 int64_t* h_total_rows, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = check_lt(ctx, fields, K)) return r;
  if (!d_rowoff || !h_total_rows) return fail(ctx, RJP_ERR_ARG, "rjp_lt_count: NULL output");
  hipStream_t st = (hipStream_t)stream;
  RJP_HIP(ctx, rjp::lt_count_launch(fields, K, d_rowoff, ctx->guard, st));
  int32_t total = 0;
  const size_t n = rjp::lt_rowoff_entries(fields->nx, fields->nz, K);
  RJP_HIP(ctx, hipMemcpyAsync(&total, d_rowoff + (n - 1), sizeof(int32_t), hipMemcpyDeviceToHost, st));
  RJP_HIP(ctx, hipStreamSynchronize(st));
  if (take_guard(ctx, false))
    return fail(ctx, RJP_ERR_ARG, "rjp_lt_count: fields.ts_lo / ts_hi do not contain every launch "
                                  "time of the cells the layout keeps (rjp_field_range)");
  if (total < 0) return fail(ctx, RJP_ERR_ARG, "rjp_lt_count: more than 2^31 rows");
  *h_total_rows = total;
  return RJP_OK;
}

int rjp_lt_fill(rjp_ctx* ctx, const rjp_fields* fields, int32_t K, const int32_t* d_rowoff,
                void* d_cells, double* d_aux, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = check_lt(ctx, fields, K)) return r;
  if (!d_rowoff || !d_cells || !d_aux) return fail(ctx, RJP_ERR_ARG, "rjp_lt_fill: NULL argument");
  RJP_HIP(ctx, rjp::lt_fill_launch(fields, K, d_rowoff, d_cells, d_aux, (hipStream_t)stream));
  return RJP_OK;
}

size_t rjp_srt_index_entries(int32_t nx, int32_t nz, int32_t K) {
  if (nx <= 0 || nz <= 0 || K < 1 || K > RJP_SRT_MAX_K) return 0;
  return rjp::srt_index_entries(nx, nz, K);
}

static int check_srt(rjp_ctx* ctx, const rjp_fields* f, int32_t K) {
  return checked(ctx, [&](std::string& m) {
    return rjp_args::check_layout(f, K, "launch-time-bucketed layout", RJP_SRT_MAX_K, 0, m);
  });
}

int rjp_srt_count(rjp_ctx* ctx, const rjp_fields* fields, int32_t K, int32_t* d_start,
                  int64_t* d_rowbase, int64_t* h_hist, int64_t* h_total_rows, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = check_srt(ctx, fields, K)) return r;
  if (!d_start || !d_rowbase || !h_hist || !h_total_rows)
    return fail(ctx, RJP_ERR_ARG, "rjp_srt_count: NULL output");
  hipStream_t st = (hipStream_t)stream;
  if (!ctx->d_srt_hist)
    RJP_HIP(ctx, hipMalloc((void**)&ctx->d_srt_hist, 2 * RJP_SRT_MAX_K * sizeof(unsigned long long)));
  RJP_HIP(ctx, rjp::srt_count_launch(fields, K, d_start, d_rowbase, ctx->d_srt_hist, ctx->guard, st));
  const int64_t G = ((int64_t)fields->nx * fields->nz + 63) / 64;
  int64_t total = 0;
  unsigned long long hist[2 * RJP_SRT_MAX_K];
  RJP_HIP(ctx, hipMemcpyAsync(&total, d_rowbase + G, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  RJP_HIP(ctx, hipMemcpyAsync(hist, ctx->d_srt_hist, 2 * K * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, st));
  RJP_HIP(ctx, hipStreamSynchronize(st));
  if (take_guard(ctx, false))
    return fail(ctx, RJP_ERR_ARG, "rjp_srt_count: fields.ts_lo / ts_hi do not contain every launch "
                                  "time of the cells the layout keeps (rjp_field_range)");
  for (int q = 0; q < 2 * K; ++q) h_hist[q] = (int64_t)hist[q];
  *h_total_rows = total;
  return RJP_OK;
}

int rjp_srt_fill(rjp_ctx* ctx, const rjp_fields* fields, int32_t K, const int32_t* d_start,
                 const int64_t* d_rowbase, void* d_cells, double* d_cum, double* d_aux,
                 void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = check_srt(ctx, fields, K)) return r;
  if (!d_start || !d_rowbase || !d_cells || !d_cum || !d_aux)
    return fail(ctx, RJP_ERR_ARG, "rjp_srt_fill: NULL argument");
  RJP_HIP(ctx, rjp::srt_fill_launch(fields, K, d_start, d_rowbase, d_cells, d_cum, d_aux,
                                    (hipStream_t)stream));
  return RJP_OK;
}

size_t rjp_srt_moment_entries(int32_t nx, int32_t nz, int32_t K, int32_t N) {
  if (nx <= 0 || nz <= 0 || K < 1 || K > RJP_SRT_MAX_K || !rjp::srt_moment_order_ok(N)) return 0;
  return rjp::srt_moment_entries(nx, nz, K, N);
}

int rjp_srt_moments(rjp_ctx* ctx, const rjp_fields* fields, int32_t K, int32_t N,
                    const int32_t* d_start, const int64_t* d_rowbase, const void* d_cells,
                    double* d_mom, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = check_srt(ctx, fields, K)) return r;
  if (!rjp::srt_moment_order_ok(N))
    return fail(ctx, RJP_ERR_ARG, "rjp_srt_moments: N must be 16, 20 or 24");
  if (!d_start || !d_rowbase || !d_cells || !d_mom)
    return fail(ctx, RJP_ERR_ARG, "rjp_srt_moments: NULL argument");
  RJP_HIP(ctx, rjp::srt_moments_launch(fields, K, N, d_start, d_rowbase, d_cells, d_mom,
                                       (hipStream_t)stream));
  return RJP_OK;
}

size_t rjp_srt_packed_rows(int32_t nx, int32_t nz, int64_t total_rows) {
  if (nx <= 0 || nz <= 0 || total_rows < 0) return 0;
  return (size_t)rjp::srt_packed_rows(total_rows, ((int64_t)nx * nz + 63) / 64);
}

int64_t rjp_srt_pack(rjp_ctx* ctx, const rjp_fields* fields, int32_t K, const int32_t* d_start,
                     const int64_t* d_rowbase, const void* d_cells, void* d_pts, void* d_pw,
                     void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = check_srt(ctx, fields, K)) return r;
  if (!d_start || !d_rowbase || !d_cells || !d_pts || !d_pw)
    return fail(ctx, RJP_ERR_ARG, "rjp_srt_pack: NULL argument");
  if (((uintptr_t)d_pts % 16) != 0 || ((uintptr_t)d_pw % 16) != 0)
    return fail(ctx, RJP_ERR_ARG, "rjp_srt_pack: d_pts and d_pw must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  // (the out-of-range flag: the context's device word, as rjp_occupied_cells uses it)
  if (!ctx->d_count) RJP_HIP(ctx, hipMalloc((void**)&ctx->d_count, sizeof(unsigned long long)));
  RJP_HIP(ctx, hipMemsetAsync(ctx->d_count, 0, sizeof(unsigned long long), st));
  RJP_HIP(ctx, rjp::srt_pack_launch(fields, K, d_start, d_rowbase, d_cells, d_pts, d_pw,
                                    reinterpret_cast<int*>(ctx->d_count), st));
  unsigned long long flag = 0;
  RJP_HIP(ctx, hipMemcpyAsync(&flag, ctx->d_count, sizeof(flag), hipMemcpyDeviceToHost, st));
  RJP_HIP(ctx, hipStreamSynchronize(st));
  return flag ? 2 : 1;
}

// word `slot` of every group's counters of the last scan, summed
static int64_t srt_diag_sum(rjp_ctx* ctx, int slot) {
  if (int r = bind(ctx)) return r;
  if (!ctx->last_srt_mom) return 0;
  std::vector<unsigned long long> h((size_t)ctx->srt_diag_groups * rjp::kSrtDiagWords);
  RJP_HIP(ctx, hipDeviceSynchronize());
  RJP_HIP(ctx, hipMemcpy(h.data(), ctx->d_srt_diag, h.size() * sizeof(unsigned long long),
                         hipMemcpyDeviceToHost));
  int64_t n = 0;
  for (size_t g = slot; g < h.size(); g += rjp::kSrtDiagWords) n += (int64_t)h[g];
  return n;
}

int64_t rjp_last_srt_resid(rjp_ctx* ctx) { return srt_diag_sum(ctx, 2); }

int64_t rjp_last_srt_fallbacks(rjp_ctx* ctx) { return srt_diag_sum(ctx, 3); }

int64_t rjp_srt_codes(rjp_ctx* ctx, const rjp_fields* fields, int32_t K, const int32_t* d_start,
                      const int64_t* d_rowbase, const void* d_cells, void* d_pc, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_srt_codes(fields, K, RJP_SRT_MAX_K, d_start, d_rowbase, d_cells, d_pc, m);
      }))
    return r;
  RJP_HIP(ctx, rjp::srt_codes_launch(fields, K, d_start, d_rowbase, d_cells, d_pc,
                                     (hipStream_t)stream));
  return 1;
}

int rjp_time_ff_scan(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                     const double* h_epochs_s, int32_t n_epochs, int32_t gff_mode,
                     double* d_sumA, double* d_em, double* d_tavg, void* d_work,
                     size_t work_bytes, void* stream, int32_t reps, double* ms_avg) {
  if (!ms_avg || reps < 1) return fail(ctx, RJP_ERR_ARG, "rjp_time_ff_scan: bad reps/ms_avg");
  if (int r = bind(ctx)) return r;
  hipStream_t st = (hipStream_t)stream;
  RJP_HIP(ctx, hipEventRecord(ctx->ev0, st));
  for (int i = 0; i < reps; ++i) {
    int r = ff_scan_impl(ctx, fields, bursts, h_epochs_s, n_epochs, gff_mode, d_sumA, d_em,
                         d_tavg, d_work, work_bytes, stream);
    if (r != RJP_OK) return r;
  }
  RJP_HIP(ctx, hipEventRecord(ctx->ev1, st));
  RJP_HIP(ctx, hipEventSynchronize(ctx->ev1));
  float ms = 0.f;
  RJP_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
  *ms_avg = (double)ms / reps;
  return RJP_OK;
}

size_t rjp_ff_maps_workspace(int64_t n_pix, int32_t n_epochs, int32_t n_chan) {
  if (n_pix <= 0 || n_epochs <= 0 || n_chan <= 0) return 0;
  return rjp::ff_maps_workspace_bytes(n_pix, n_epochs, n_chan);
}

static int ff_maps_impl(rjp_ctx* ctx, const double* d_sumA, const double* d_tavg, int64_t n_pix,
                        int32_t n_epochs, const double* h_ctau, const double* h_cflux,
                        int32_t n_chan, double* d_tau, double* d_flux, double* d_ftot,
                        void* d_work, size_t work_bytes, void* stream) {
  if (!d_sumA || !d_tavg || !h_ctau || !h_cflux)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_maps: NULL input");
  if (n_pix <= 0 || n_epochs <= 0 || n_chan <= 0)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_maps: sizes must be positive");
  if (d_ftot && (!d_work || work_bytes < rjp::ff_maps_workspace_bytes(n_pix, n_epochs, n_chan)))
    return fail(ctx, RJP_ERR_WORKSPACE, "rjp_ff_maps: workspace smaller than rjp_ff_maps_workspace()");
  hipStream_t st = (hipStream_t)stream;
  const size_t F = (size_t)n_chan;
  return staged(ctx, st, "ff_maps_launch", nullptr, {{h_ctau, F}, {h_cflux, F}},
                [&](double* const* d, const double*) {
                  return rjp::ff_maps_launch(d_sumA, d_tavg, n_pix, n_epochs, d[0], d[1], n_chan,
                                             d_tau, d_flux, d_ftot, (double*)d_work, st,
                                             ctx->last_maps);
                });
}

int rjp_ff_maps(rjp_ctx* ctx, const double* d_sumA, const double* d_tavg, int64_t n_pix,
                int32_t n_epochs, const double* h_ctau, const double* h_cflux, int32_t n_chan,
                double* d_tau, double* d_flux, double* d_ftot, void* d_work, size_t work_bytes,
                void* stream) {
  if (int r = bind(ctx)) return r;
  return ff_maps_impl(ctx, d_sumA, d_tavg, n_pix, n_epochs, h_ctau, h_cflux, n_chan, d_tau, d_flux,
                      d_ftot, d_work, work_bytes, stream);
}

int rjp_ff_step(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                const double* h_epochs_s, int32_t n_epochs, int32_t gff_mode,
                const double* d_tavg, const double* h_ctau, const double* h_cflux, int32_t n_chan,
                double* d_sumA, double* d_em, double* d_tau, double* d_flux, double* d_ftot,
                void* d_work, size_t work_bytes, void* d_work_maps, size_t work_maps_bytes,
                void* stream) {
  if (int r = bind(ctx)) return r;
  // every argument of the map stage is checked BEFORE the scan is enqueued: a step either runs
  // whole or not at all
  if (!fields) return fail(ctx, RJP_ERR_ARG, "fields is NULL");
  if (!d_tavg || !h_ctau || !h_cflux || n_chan < 1)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_step: NULL d_tavg / channel table or n_chan < 1");
  if (fields->nx <= 0 || fields->nz <= 0 || n_epochs < 1)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_step: bad grid or n_epochs < 1");
  const int64_t n_pix = (int64_t)fields->nx * fields->nz;
  if (d_ftot && (!d_work_maps ||
                 work_maps_bytes < rjp::ff_maps_workspace_bytes(n_pix, n_epochs, n_chan)))
    return fail(ctx, RJP_ERR_WORKSPACE, "rjp_ff_step: d_work_maps smaller than rjp_ff_maps_workspace()");
  if (int r = ff_scan_impl(ctx, fields, bursts, h_epochs_s, n_epochs, gff_mode, d_sumA, d_em,
                           nullptr, d_work, work_bytes, stream))
    return r;
  return ff_maps_impl(ctx, d_sumA, d_tavg, n_pix, n_epochs, h_ctau, h_cflux, n_chan, d_tau, d_flux,
                      d_ftot, d_work_maps, work_maps_bytes, stream);
}

int rjp_rrl_scan(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                 double time_s, const rjp_line* line, const double* h_nu, int32_t n_chan,
                 double* d_tau_rrl, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = check_fields(ctx, fields, true)) return r;
  if (int r = check_bursts(ctx, bursts, fields)) return r;
  if (!line || !h_nu || n_chan < 1 || !d_tau_rrl)
    return fail(ctx, RJP_ERR_ARG, "rjp_rrl_scan: NULL line / nu / output or n_chan < 1");
  hipStream_t st = (hipStream_t)stream;
  return staged(ctx, st, "rrl_scan_launch", bursts, {{h_nu, (size_t)n_chan}},
                [&](double* const* d, const double* d_ext) {
                  return rjp::rrl_scan_launch(fields, bursts, d_ext, time_s, line, h_nu, d[0],
                                              n_chan, d_tau_rrl, st);
                });
}

int rjp_ff_cells(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts, double time_s,
                 int32_t gff_mode, const double* h_ctau, int32_t n_chan, double* d_tau_cells,
                 void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = check_fields(ctx, fields, false)) return r;
  if (int r = check_bursts(ctx, bursts, fields)) return r;
  if (!h_ctau || n_chan < 1 || !d_tau_cells)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_cells: NULL table / output or n_chan < 1");
  if (!mode_ok(gff_mode)) return fail(ctx, RJP_ERR_ARG, "bad gff_mode");
  hipStream_t st = (hipStream_t)stream;
  return staged(ctx, st, "ff_cells_launch", bursts, {{h_ctau, (size_t)n_chan}},
                [&](double* const* d, const double* d_ext) {
                  return rjp::ff_cells_launch(fields, bursts, d_ext, time_s, gff_mode, d[0],
                                              n_chan, d_tau_cells, st);
                });
}

int rjp_ff_formal(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                  double time_s, int32_t gff_mode, const double* h_ctau, const double* h_csrc,
                  int32_t n_chan, double* d_out, void* stream) {
  if (int r = bind(ctx)) return r;
  if (!mode_ok(gff_mode)) return fail(ctx, RJP_ERR_ARG, "bad gff_mode");
  if (int r = check_fields(ctx, fields, false, true, gff_mode)) return r;
  if (!fields->d_temp)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_formal: fields.d_temp must be a device pointer");
  if (int r = check_bursts(ctx, bursts, fields)) return r;
  if (!h_ctau || !h_csrc || n_chan < 1 || !d_out)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_formal: NULL table / output or n_chan < 1");
  hipStream_t st = (hipStream_t)stream;
  const size_t F = (size_t)n_chan;
  return staged(ctx, st, "ff_formal_launch", bursts, {{h_ctau, F}, {h_csrc, F}},
                [&](double* const* d, const double* d_ext) {
                  return rjp::ff_formal_launch(fields, bursts, d_ext, time_s, gff_mode, d[0], d[1],
                                               n_chan, d_out, st);
                });
}

size_t rjp_ff_formal_sweep_workspace(int32_t nx, int32_t ny, int32_t nz, int32_t n_epochs,
                                     int32_t n_chan) {
  if (nx <= 0 || ny <= 0 || nz <= 0 || n_epochs <= 0 || n_chan <= 0) return 0;
  return rjp::ff_formal_sweep_workspace_bytes(nx, nz, n_epochs, n_chan);
}

int rjp_ff_formal_sweep(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                        const double* h_epochs_s, int32_t n_epochs, int32_t gff_mode,
                        const double* h_ctau, const double* h_csrc, int32_t n_chan,
                        double* d_out, double* d_ftot, void* d_work, size_t work_bytes,
                        void* stream) {
  if (int r = bind(ctx)) return r;
  if (!mode_ok(gff_mode)) return fail(ctx, RJP_ERR_ARG, "bad gff_mode");
  if (int r = check_fields(ctx, fields, false, true, gff_mode)) return r;
  if (!fields->d_temp)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_formal_sweep: fields.d_temp must be a device pointer");
  if (int r = check_bursts(ctx, bursts, fields)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_epochs(h_epochs_s, n_epochs, true, "rjp_ff_formal_sweep", m);
      }))
    return r;
  if (!h_ctau || !h_csrc || n_chan < 1)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_formal_sweep: NULL table or n_chan < 1");
  if (!d_out && !d_ftot)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_formal_sweep: both outputs are NULL");
  if ((int64_t)n_epochs * n_chan > INT32_MAX)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_formal_sweep: n_epochs * n_chan exceeds 2^31 - 1");
  if (d_ftot && (!d_work || work_bytes < rjp::ff_formal_sweep_workspace_bytes(
                                             fields->nx, fields->nz, n_epochs, n_chan)))
    return fail(ctx, RJP_ERR_WORKSPACE,
                "rjp_ff_formal_sweep: workspace smaller than rjp_ff_formal_sweep_workspace()");
  hipStream_t st = (hipStream_t)stream;
  const size_t F = (size_t)n_chan;
  return staged(ctx, st, "ff_formal_sweep_launch", bursts,
                {{h_ctau, F}, {h_csrc, F}, {h_epochs_s, (size_t)n_epochs}},
                [&](double* const* d, const double* d_ext) {
                  return rjp::ff_formal_sweep_launch(fields, bursts, d_ext, d[2], n_epochs,
                                                     gff_mode, d[0], d[1], n_chan, d_out, d_ftot,
                                                     (double*)d_work, st);
                });
}

size_t rjp_ff_grad_workspace(int32_t nx, int32_t ny, int32_t nz, int32_t n_epochs,
                             int32_t n_par, int32_t n_chan) {
  if (nx <= 0 || ny <= 0 || nz <= 0 || n_epochs <= 0 || n_par <= 0 || n_chan < 0) return 0;
  return rjp::ff_grad_workspace_bytes(nx, ny, nz, n_epochs, n_par, n_chan);
}

int rjp_ff_grad(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                const double* h_epochs_s, int32_t n_epochs, int32_t gff_mode,
                const double* d_tavg, const double* h_ctau, const double* h_cflux, int32_t n_chan,
                double* d_sumA, double* d_dsumA, double* d_ftot, double* d_dftot,
                void* d_work, size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (!mode_ok(gff_mode)) return fail(ctx, RJP_ERR_ARG, "bad gff_mode");
  if (!fields) return fail(ctx, RJP_ERR_ARG, "fields is NULL");
  if (fields->dtype != RJP_F64 || !fields->d_a0 || fields->a0_mode != gff_mode)
    return fail(ctx, RJP_ERR_ARG,
                "rjp_ff_grad: needs RJP_F64 fields with the tau layout (d_a0) built for gff_mode");
  if (int r = check_fields(ctx, fields, false, false, gff_mode)) return r;
  if (!fields->d_ts) return fail(ctx, RJP_ERR_ARG, "rjp_ff_grad: fields.d_ts required");
  double scale[kMaxScale];          // 1, then the chain-rule constant of every parameter
  int n_scale = 0;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_grad_bursts(bursts, fields, h_epochs_s, n_epochs, RJP_SGPR_BURSTS,
                                           true, "rjp_ff_grad", scale, &n_scale, m);
      }))
    return r;
  const int npar = n_scale - 1;
  if (!d_sumA && !d_dsumA && !d_ftot && !d_dftot)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_grad: all four outputs are NULL");
  const bool totals = d_ftot || d_dftot;
  if (totals && (!d_tavg || !h_ctau || !h_cflux || n_chan < 1))
    return fail(ctx, RJP_ERR_ARG,
                "rjp_ff_grad: d_ftot / d_dftot need d_tavg, the channel tables and n_chan >= 1");
  const int nch = totals ? n_chan : 0;
  if (!d_work || work_bytes < rjp::ff_grad_workspace_bytes(fields->nx, fields->ny, fields->nz,
                                                           n_epochs, npar, nch))
    return fail(ctx, RJP_ERR_WORKSPACE, "rjp_ff_grad: workspace smaller than rjp_ff_grad_workspace()");
  hipStream_t st = (hipStream_t)stream;
  return staged(ctx, st, "ff_grad_run", nullptr,
                {{scale, (size_t)n_scale}, {h_ctau, (size_t)nch}, {h_cflux, (size_t)nch}},
                [&](double* const* d, const double*) {
                  return rjp::ff_grad_run(fields, bursts, h_epochs_s, n_epochs, d[0], d_tavg, d[1],
                                          d[2], nch, d_sumA, d_dsumA, d_ftot, d_dftot,
                                          (double*)d_work, work_bytes, st);
                });
}

size_t rjp_ff_formal_grad_workspace(int32_t nx, int32_t ny, int32_t nz, int32_t n_epochs,
                                    int32_t n_par, int32_t n_chan) {
  if (nx <= 0 || ny <= 0 || nz <= 0 || n_epochs <= 0 || n_par <= 0 || n_chan <= 0) return 0;
  return rjp::ff_formal_grad_workspace_bytes(nx, nz, n_epochs, n_par, n_chan);
}

int rjp_ff_formal_grad(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                       const double* h_epochs_s, int32_t n_epochs, int32_t gff_mode,
                       const double* h_ctau, const double* h_csrc, int32_t n_chan,
                       double* d_ftot, double* d_dftot, double* d_dout,
                       void* d_work, size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (!mode_ok(gff_mode)) return fail(ctx, RJP_ERR_ARG, "bad gff_mode");
  if (!fields) return fail(ctx, RJP_ERR_ARG, "fields is NULL");
  if (fields->dtype != RJP_F64)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_formal_grad: needs RJP_F64 fields");
  if (int r = check_fields(ctx, fields, false, true, gff_mode)) return r;
  if (!fields->d_temp || !fields->d_ts)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_formal_grad: fields.d_temp and fields.d_ts required");
  double scale[kMaxScale];          // the chain-rule constant of every parameter
  int npar = 0;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_grad_bursts(bursts, fields, h_epochs_s, n_epochs, RJP_SGPR_BURSTS,
                                           false, "rjp_ff_formal_grad", scale, &npar, m);
      }))
    return r;
  if (!h_ctau || !h_csrc || n_chan < 1)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_formal_grad: NULL table or n_chan < 1");
  if (!d_ftot && !d_dftot && !d_dout)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_formal_grad: all three outputs are NULL");
  if ((int64_t)n_epochs * n_chan * npar > INT32_MAX)
    return fail(ctx, RJP_ERR_ARG, "rjp_ff_formal_grad: n_epochs * n_chan * n_par exceeds 2^31 - 1");
  if ((d_ftot || d_dftot) &&
      (!d_work || work_bytes < rjp::ff_formal_grad_workspace_bytes(fields->nx, fields->nz, n_epochs,
                                                                   npar, n_chan)))
    return fail(ctx, RJP_ERR_WORKSPACE,
                "rjp_ff_formal_grad: workspace smaller than rjp_ff_formal_grad_workspace()");
  hipStream_t st = (hipStream_t)stream;
  const size_t F = (size_t)n_chan;
  return staged(ctx, st, "ff_formal_grad_launch", nullptr,
                {{h_ctau, F}, {h_csrc, F}, {h_epochs_s, (size_t)n_epochs}, {scale, (size_t)npar}},
                [&](double* const* d, const double*) {
                  return rjp::ff_formal_grad_launch(fields, bursts, d[2], n_epochs, gff_mode, d[0],
                                                    d[1], n_chan, d[3], d_ftot, d_dftot, d_dout,
                                                    (double*)d_work, st);
                });
}

size_t rjp_vis_workspace(int32_t n_maps, int32_t nx, int32_t nz, int32_t n_vis) {
  if (n_maps <= 0 || nx <= 0 || nz <= 0 || n_vis <= 0) return 0;
  return rjp::vis_workspace_bytes(n_maps, nx, nz, n_vis);
}

int rjp_vis(rjp_ctx* ctx, const double* d_maps, int32_t n_maps, int32_t nx, int32_t nz,
            const double* h_su, const double* h_sv, const double* d_u, const double* d_v,
            int32_t n_vis, double* d_vis, void* d_work, size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (!d_maps || !h_su || !h_sv || !d_u || !d_v || !d_vis)
    return fail(ctx, RJP_ERR_ARG, "rjp_vis: NULL maps, scales, baselines or output");
  if (n_maps < 1 || nx < 1 || nz < 1 || n_vis < 1)
    return fail(ctx, RJP_ERR_ARG, "rjp_vis: n_maps, nx, nz and n_vis must be positive");
  for (int m = 0; m < n_maps; ++m)
    if (!std::isfinite(h_su[m]) || !std::isfinite(h_sv[m]))
      return fail(ctx, RJP_ERR_ARG, "rjp_vis: non-finite h_su / h_sv");
  if (!rjp::vis_grid_ok(n_maps, nx, n_vis))
    return fail(ctx, RJP_ERR_ARG, "rjp_vis: more than 2^31 - 1 tiles");
  const size_t need = rjp::vis_workspace_bytes(n_maps, nx, nz, n_vis);
  if (need == 0) return fail(ctx, RJP_ERR_ARG, "rjp_vis: the workspace size overflows");
  if (!d_work || work_bytes < need)
    return fail(ctx, RJP_ERR_WORKSPACE, "rjp_vis: workspace smaller than rjp_vis_workspace()");
  hipStream_t st = (hipStream_t)stream;
  return staged(ctx, st, "vis_launch", nullptr, {{h_su, (size_t)n_maps}, {h_sv, (size_t)n_maps}},
                [&](double* const* d, const double*) {
                  return rjp::vis_launch(d_maps, n_maps, nx, nz, d[0], d[1], d_u, d_v, n_vis,
                                         d_vis, (double*)d_work, st);
                });
}

size_t rjp_vis_adjoint_workspace(int32_t n_maps, int32_t nx, int32_t nz, int32_t n_vis) {
  if (n_maps <= 0 || nx <= 0 || nz <= 0 || n_vis <= 0) return 0;
  return rjp::vis_adjoint_workspace_bytes(n_maps, nx, nz, n_vis);
}

int64_t rjp_vis_adjoint(rjp_ctx* ctx, const double* d_vis, int32_t n_maps, int32_t n_vis,
                        const double* h_su, const double* h_sv, const double* d_u,
                        const double* d_v, const double* d_w, int32_t nx, int32_t nz,
                        double* d_img, void* d_work, size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_vis_adjoint(d_vis, n_maps, n_vis, h_su, h_sv, d_u, d_v, nx, nz,
                                           d_img, m);
      }))
    return r;
  const rjp::VisAdjointTiling t = rjp::vis_adjoint_tiling(n_maps, nx, nz, n_vis);
  if (t.workgroups > (int64_t)INT32_MAX)
    return fail(ctx, RJP_ERR_ARG, "rjp_vis_adjoint: more than 2^31 - 1 workgroups");
  const size_t need = rjp::vis_adjoint_workspace_bytes(n_maps, nx, nz, n_vis);
  if (need == 0) return fail(ctx, RJP_ERR_ARG, "rjp_vis_adjoint: the workspace size overflows");
  if (!d_work || work_bytes < need)
    return fail(ctx, RJP_ERR_WORKSPACE,
                "rjp_vis_adjoint: workspace smaller than rjp_vis_adjoint_workspace()");
  hipStream_t st = (hipStream_t)stream;
  const int r = staged(ctx, st, "vis_adjoint_launch", nullptr,
                       {{h_su, (size_t)n_maps}, {h_sv, (size_t)n_maps}},
                       [&](double* const* d, const double*) {
                         return rjp::vis_adjoint_launch(d_vis, n_maps, n_vis, d[0], d[1], d_u, d_v,
                                                        d_w, nx, nz, d_img, (double*)d_work, st);
                       });
  return r ? r : t.workgroups;
}

size_t rjp_clean_workspace(int32_t n_maps, int32_t nx, int32_t nz) {
  if (n_maps <= 0 || nx <= 0 || nz <= 0) return 0;
  return rjp::clean_workspace_bytes(n_maps, nx, nz);
}

int64_t rjp_clean(rjp_ctx* ctx, double* d_res, int32_t n_maps, int32_t nx, int32_t nz,
                  const double* d_psf, int32_t n_psf, int32_t px, int32_t pz,
                  const uint8_t* d_mask, const double* h_thresh, double gain, int32_t n_iter,
                  int32_t* d_cpix, double* d_cflux, int32_t* d_ncomp, double* d_model,
                  double* d_peak, void* d_work, size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_clean(d_res, n_maps, nx, nz, d_psf, n_psf, px, pz, h_thresh, gain,
                                     n_iter, d_cpix, d_cflux, d_ncomp, m);
      }))
    return r;
  const rjp::CleanTiling t = rjp::clean_tiling(n_maps, nx, nz);
  if (t.workgroups > (int64_t)INT32_MAX)
    return fail(ctx, RJP_ERR_ARG, "rjp_clean: more than 2^31 - 1 workgroups");
  const size_t need = rjp::clean_workspace_bytes(n_maps, nx, nz);
  if (!d_work || work_bytes < need)
    return fail(ctx, RJP_ERR_WORKSPACE, "rjp_clean: workspace smaller than rjp_clean_workspace()");
  hipStream_t st = (hipStream_t)stream;
  const int r = staged(ctx, st, "clean_launch", nullptr, {{h_thresh, (size_t)n_maps}},
                       [&](double* const* d, const double*) {
                         return rjp::clean_launch(d_res, n_maps, nx, nz, d_psf, n_psf, px, pz,
                                                  d_mask, d[0], gain, n_iter, d_cpix, d_cflux,
                                                  d_ncomp, d_model, d_peak, d_work, st);
                       });
  return r ? r : t.workgroups;
}

int64_t rjp_restore(rjp_ctx* ctx, const int32_t* d_cpix, const double* d_cflux,
                    const int32_t* d_ncomp, int32_t n_maps, int32_t comp_stride,
                    const double* h_beam, const double* d_add, int32_t nx, int32_t nz,
                    double* d_out, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_restore(d_cpix, d_cflux, d_ncomp, n_maps, comp_stride, h_beam, nx,
                                       nz, d_out, m);
      }))
    return r;
  const int64_t wgs = rjp::restore_workgroups(n_maps, nx, nz);
  if (wgs > (int64_t)INT32_MAX)
    return fail(ctx, RJP_ERR_ARG, "rjp_restore: more than 2^31 - 1 workgroups");
  hipStream_t st = (hipStream_t)stream;
  const int r = staged(ctx, st, "restore_launch", nullptr, {{h_beam, 3 * (size_t)n_maps}},
                       [&](double* const* d, const double*) {
                         return rjp::restore_launch(d_cpix, d_cflux, d_ncomp, n_maps, comp_stride,
                                                    d[0], d_add, nx, nz, d_out, st);
                       });
  return r ? r : wgs;
}

int64_t rjp_convolve2d(rjp_ctx* ctx, const double* d_in, int32_t n_maps, int32_t nx, int32_t nz,
                       const double* d_ker, int32_t n_ker, int32_t kx, int32_t kz,
                       const double* d_add, double* d_out, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_convolve2d(d_in, n_maps, nx, nz, d_ker, n_ker, kx, kz, d_out, m);
      }))
    return r;
  const rjp::ConvTiling t = rjp::conv_tiling(n_maps, nx, nz);
  if (t.workgroups > (int64_t)INT32_MAX || rjp::conv_chunk_rows(kx, kz) < 1)   // (check_convolve2d's)
    return fail(ctx, RJP_ERR_ARG, "rjp_convolve2d: more than 2^31 - 1 workgroups");
  const hipError_t e = rjp::convolve2d_launch(d_in, n_maps, nx, nz, d_ker, n_ker, kx, kz, d_add,
                                              d_out, (hipStream_t)stream);
  if (e != hipSuccess) return fail(ctx, RJP_ERR_HIP, "convolve2d_launch", e);
  return t.workgroups;
}

size_t rjp_msclean_workspace(int32_t n_maps, int32_t n_s, int32_t nx, int32_t nz) {
  if (n_maps <= 0 || n_s <= 0 || nx <= 0 || nz <= 0) return 0;
  return rjp::msclean_workspace_bytes(n_maps, n_s, nx, nz);
}

int64_t rjp_msclean(rjp_ctx* ctx, double* d_res, int32_t n_maps, int32_t n_s, int32_t nx,
                    int32_t nz, const double* d_xpsf, int32_t n_psf, int32_t px, int32_t pz,
                    const double* h_weight, const uint8_t* d_mask, const double* h_thresh,
                    double gain, int32_t n_iter, int32_t* d_cpix, int32_t* d_cscale,
                    double* d_cflux, int32_t* d_ncomp, double* d_model, double* d_peak,
                    void* d_work, size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_msclean(d_res, n_maps, n_s, nx, nz, d_xpsf, n_psf, px, pz, h_weight,
                                       h_thresh, gain, n_iter, d_cpix, d_cscale, d_cflux, d_ncomp,
                                       m);
      }))
    return r;
  const rjp::MsCleanTiling t = rjp::msclean_tiling(n_maps, n_s, nx, nz);
  if (t.workgroups > (int64_t)INT32_MAX)
    return fail(ctx, RJP_ERR_ARG, "rjp_msclean: more than 2^31 - 1 workgroups");
  const size_t need = rjp::msclean_workspace_bytes(n_maps, n_s, nx, nz);
  if (!d_work || need == 0 || work_bytes < need)
    return fail(ctx, RJP_ERR_WORKSPACE,
                "rjp_msclean: workspace smaller than rjp_msclean_workspace()");
  hipStream_t st = (hipStream_t)stream;
  const int r = staged(ctx, st, "msclean_launch", nullptr,
                       {{h_weight, (size_t)n_maps * (size_t)n_s}, {h_thresh, (size_t)n_maps}},
                       [&](double* const* d, const double*) {
                         return rjp::msclean_launch(d_res, n_maps, n_s, nx, nz, d_xpsf, n_psf, px,
                                                    pz, d[0], d_mask, d[1], gain, n_iter, d_cpix,
                                                    d_cscale, d_cflux, d_ncomp, d_model, d_peak,
                                                    d_work, st);
                       });
  return r ? r : t.workgroups;
}

size_t rjp_mtmfs_workspace(int32_t n_maps, int32_t n_t, int32_t nx, int32_t nz) {
  if (n_maps <= 0 || n_t <= 0 || n_t > RJP_MTMFS_MAX_NT || nx <= 0 || nz <= 0) return 0;
  return rjp::mtmfs_workspace_bytes(n_maps, n_t, nx, nz);
}

int64_t rjp_mtmfs(rjp_ctx* ctx, double* d_res, int32_t n_maps, int32_t n_t, int32_t nx, int32_t nz,
                  const double* d_spsf, int32_t n_psf, int32_t px, int32_t pz,
                  const double* h_hinv, const uint8_t* d_mask, const double* h_thresh, double gain,
                  int32_t n_iter, int32_t* d_cpix, double* d_ccoef, int32_t* d_ncomp,
                  double* d_model, double* d_peak, void* d_work, size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_mtmfs(d_res, n_maps, n_t, nx, nz, d_spsf, n_psf, px, pz, h_hinv,
                                     h_thresh, gain, n_iter, d_cpix, d_ccoef, d_ncomp, m);
      }))
    return r;
  const rjp::MtmfsTiling t = rjp::mtmfs_tiling(n_maps, nx, nz);
  if (t.workgroups > (int64_t)INT32_MAX)
    return fail(ctx, RJP_ERR_ARG, "rjp_mtmfs: more than 2^31 - 1 workgroups");
  const size_t need = rjp::mtmfs_workspace_bytes(n_maps, n_t, nx, nz);
  if (!d_work || need == 0 || work_bytes < need)
    return fail(ctx, RJP_ERR_WORKSPACE, "rjp_mtmfs: workspace smaller than rjp_mtmfs_workspace()");
  hipStream_t st = (hipStream_t)stream;
  const int r = staged(ctx, st, "mtmfs_launch", nullptr,
                       {{h_hinv, (size_t)n_maps * (size_t)n_t * (size_t)n_t},
                        {h_thresh, (size_t)n_maps}},
                       [&](double* const* d, const double*) {
                         return rjp::mtmfs_launch(d_res, n_maps, n_t, nx, nz, d_spsf, n_psf, px, pz,
                                                  d[0], d_mask, d[1], gain, n_iter, d_cpix, d_ccoef,
                                                  d_ncomp, d_model, d_peak, d_work, st);
                       });
  return r ? r : t.workgroups;
}

int64_t rjp_vis_components(rjp_ctx* ctx, const int32_t* d_cpix, const int32_t* d_cscale,
                           const double* d_cflux, const int32_t* d_ncomp, int32_t n_maps,
                           int32_t comp_stride, int32_t n_s, int32_t nx, int32_t nz,
                           const double* h_su, const double* h_sv, const double* d_u,
                           const double* d_v, int32_t n_vis, const double* d_gvis,
                           const double* d_in, int32_t sign, double* d_out, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_vis_components(d_cpix, d_cflux, d_ncomp, n_maps, comp_stride, n_s, nx,
                                              nz, h_su, h_sv, d_u, d_v, n_vis, d_gvis, sign, d_out,
                                              m);
      }))
    return r;
  hipStream_t st = (hipStream_t)stream;
  const int r = staged(ctx, st, "vis_components_launch", nullptr,
                       {{h_su, (size_t)n_maps}, {h_sv, (size_t)n_maps}},
                       [&](double* const* d, const double*) {
                         return rjp::vis_components_launch(d_cpix, d_cscale, d_cflux, d_ncomp,
                                                           n_maps, comp_stride, n_s, nx, nz, d[0],
                                                           d[1], d_u, d_v, n_vis, d_gvis, d_in, sign,
                                                           d_out, st);
                       });
  return r ? r : rjp::vis_components_workgroups(n_maps, n_vis);
}

int64_t rjp_components_image(rjp_ctx* ctx, const int32_t* d_cpix, const int32_t* d_cscale,
                             const double* d_cflux, const int32_t* d_ncomp, int32_t n_maps,
                             int32_t comp_stride, int32_t n_s, int32_t nx, int32_t nz,
                             double* d_out, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_components_image(d_cpix, d_cflux, d_ncomp, n_maps, comp_stride, n_s,
                                                nx, nz, d_out, m);
      }))
    return r;
  const hipError_t e = rjp::components_image_launch(d_cpix, d_cscale, d_cflux, d_ncomp, n_maps,
                                                    comp_stride, n_s, nx, nz, d_out,
                                                    (hipStream_t)stream);
  if (e != hipSuccess) return fail(ctx, RJP_ERR_HIP, "components_image_launch", e);
  return rjp::components_image_workgroups(n_maps, n_s, nx, nz);
}

size_t rjp_gaussfit_workspace(int32_t n_maps, int32_t box_pixels) {
  if (n_maps <= 0 || box_pixels <= 0) return 0;
  return rjp::gaussfit_workspace_bytes(n_maps, box_pixels);
}

int64_t rjp_gaussfit(rjp_ctx* ctx, const double* d_img, int32_t n_maps, int32_t nx, int32_t nz,
                     const int32_t* h_box, const uint8_t* d_mask, double* d_theta, double lambda0,
                     double xtol, int32_t n_iter, double* d_chi2, double* d_cov, int32_t* d_npix,
                     int32_t* d_niter, int32_t* d_status, double* d_trace, void* d_work,
                     size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_gaussfit(d_img, n_maps, nx, nz, h_box, d_theta, lambda0, xtol,
                                        n_iter, d_chi2, d_cov, d_npix, d_niter, d_status, m);
      }))
    return r;
  const int64_t nbox = (int64_t)(h_box[1] - h_box[0] + 1) * (h_box[3] - h_box[2] + 1);
  const rjp::LmTiling t = rjp::gaussfit_tiling(n_maps, nbox);
  if (t.workgroups > (int64_t)INT32_MAX)
    return fail(ctx, RJP_ERR_ARG, "rjp_gaussfit: more than 2^31 - 1 workgroups");
  const size_t need = rjp::gaussfit_workspace_bytes(n_maps, nbox);
  if (!d_work || work_bytes < need)
    return fail(ctx, RJP_ERR_WORKSPACE,
                "rjp_gaussfit: workspace smaller than rjp_gaussfit_workspace()");
  RJP_HIP(ctx, rjp::gaussfit_launch(d_img, n_maps, nx, nz, h_box, d_mask, d_theta, lambda0, xtol,
                                    n_iter, d_chi2, d_cov, d_npix, d_niter, d_status, d_trace,
                                    d_work, (hipStream_t)stream));
  return t.workgroups;
}

size_t rjp_uvfit_workspace(int32_t n_maps, int32_t n_vis, int32_t n_comp) {
  if (n_maps <= 0 || n_vis <= 0 || n_comp < 1 || n_comp > RJP_UVFIT_MAX_COMP) return 0;
  return rjp::uvfit_workspace_bytes(n_maps, n_vis, n_comp);
}

int64_t rjp_uvfit(rjp_ctx* ctx, const double* d_vis, int32_t n_maps, int32_t n_vis,
                  const double* h_su, const double* h_sv, const double* d_u, const double* d_v,
                  const double* d_w, int32_t w_maps, int32_t n_comp, const uint8_t* h_free,
                  double* d_theta, double lambda0, double xtol, int32_t n_iter, double* d_chi2,
                  double* d_cov, int32_t* d_nvis, int32_t* d_niter, int32_t* d_status,
                  double* d_trace, void* d_work, size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_uvfit(d_vis, n_maps, n_vis, h_su, h_sv, d_u, d_v, d_w, w_maps,
                                     n_comp, h_free, d_theta, lambda0, xtol, n_iter, d_chi2, d_cov,
                                     d_nvis, d_niter, d_status, m);
      }))
    return r;
  const rjp::LmTiling t = rjp::uvfit_tiling(n_maps, n_vis);
  const size_t need = rjp::uvfit_workspace_bytes(n_maps, n_vis, n_comp);
  if (!d_work || work_bytes < need)
    return fail(ctx, RJP_ERR_WORKSPACE, "rjp_uvfit: workspace smaller than rjp_uvfit_workspace()");
  unsigned free_bits = 0;
  for (int i = 0; i < 6 * n_comp; ++i)
    if (!h_free || h_free[i]) free_bits |= 1u << i;
  hipStream_t st = (hipStream_t)stream;
  const int r = staged(ctx, st, "uvfit_launch", nullptr,
                       {{h_su, (size_t)n_maps}, {h_sv, (size_t)n_maps}},
                       [&](double* const* d, const double*) {
                         return rjp::uvfit_launch(d_vis, n_maps, n_vis, d[0], d[1], d_u, d_v, d_w,
                                                  w_maps, n_comp, free_bits, d_theta, lambda0, xtol,
                                                  n_iter, d_chi2, d_cov, d_nvis, d_niter, d_status,
                                                  d_trace, d_work, st);
                       });
  return r ? r : t.workgroups;
}

int64_t rjp_cube_moments(rjp_ctx* ctx, const double* d_cube, int64_t n_pix, int32_t n_chan,
                         const double* h_x, const double* h_dx, double x_ref, double clip,
                         const uint8_t* d_mask, double* d_mom, int32_t* d_ipeak, int32_t* d_count,
                         void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_cube_moments(d_cube, n_pix, n_chan, h_x, h_dx, x_ref, clip, d_mom,
                                            m);
      }))
    return r;
  hipStream_t st = (hipStream_t)stream;
  const size_t F = (size_t)n_chan;
  const int r = staged(ctx, st, "cube_moments_launch", nullptr, {{h_x, F}, {h_dx, F}},
                       [&](double* const* d, const double*) {
                         return rjp::cube_moments_launch(d_cube, n_pix, n_chan, d[0], d[1], x_ref,
                                                         clip, d_mask, d_mom, d_ipeak, d_count, st);
                       });
  return r ? r : rjp::specfit_workgroups(n_pix);
}

int64_t rjp_specfit(rjp_ctx* ctx, const double* d_cube, int64_t n_pix, int32_t n_chan,
                    const double* h_x, double x_ref, const double* h_w, const uint8_t* d_mask,
                    int32_t n_comp, const uint8_t* h_free, double* d_theta, double lambda0,
                    double xtol, int32_t n_iter, double* d_chi2, double* d_cov, int32_t* d_nchan,
                    int32_t* d_niter, int32_t* d_status, double* d_trace, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_specfit(d_cube, n_pix, n_chan, h_x, x_ref, h_w, n_comp, h_free,
                                       d_theta, lambda0, xtol, n_iter, d_chi2, d_cov, d_nchan,
                                       d_niter, d_status, m);
      }))
    return r;
  unsigned free_bits = 0;
  for (int i = 0; i < 3 * n_comp + 2; ++i)
    if (!h_free || h_free[i]) free_bits |= 1u << i;
  hipStream_t st = (hipStream_t)stream;
  const size_t F = (size_t)n_chan;
  const int r = staged(ctx, st, "specfit_launch", nullptr, {{h_x, F}, {h_w ? h_w : h_x, h_w ? F : 0}},
                       [&](double* const* d, const double*) {
                         return rjp::specfit_launch(d_cube, n_pix, n_chan, d[0],
                                                    h_w ? d[1] : nullptr, x_ref, d_mask, n_comp,
                                                    free_bits, d_theta, lambda0, xtol, n_iter,
                                                    d_chi2, d_cov, d_nchan, d_niter, d_status,
                                                    d_trace, st);
                       });
  return r ? r : rjp::specfit_workgroups(n_pix);
}

int64_t rjp_voigtfit(rjp_ctx* ctx, const double* d_cube, int64_t n_pix, int32_t n_chan,
                     const double* h_x, double x_ref, const double* h_w, const uint8_t* d_mask,
                     int32_t n_comp, const uint8_t* h_free, double* d_theta, double lambda0,
                     double xtol, int32_t n_iter, double* d_chi2, double* d_cov, int32_t* d_nchan,
                     int32_t* d_niter, int32_t* d_status, double* d_trace, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_voigtfit(d_cube, n_pix, n_chan, h_x, x_ref, h_w, n_comp, h_free,
                                        d_theta, lambda0, xtol, n_iter, d_chi2, d_cov, d_nchan,
                                        d_niter, d_status, m);
      }))
    return r;
  unsigned free_bits = 0;
  for (int i = 0; i < 4 * n_comp + 2; ++i)
    if (!h_free || h_free[i]) free_bits |= 1u << i;
  hipStream_t st = (hipStream_t)stream;
  const size_t F = (size_t)n_chan;
  const int r = staged(ctx, st, "voigtfit_launch", nullptr, {{h_x, F}, {h_w ? h_w : h_x, h_w ? F : 0}},
                       [&](double* const* d, const double*) {
                         return rjp::voigtfit_launch(d_cube, n_pix, n_chan, d[0],
                                                     h_w ? d[1] : nullptr, x_ref, d_mask, n_comp,
                                                     free_bits, d_theta, lambda0, xtol, n_iter,
                                                     d_chi2, d_cov, d_nchan, d_niter, d_status,
                                                     d_trace, st);
                       });
  return r ? r : rjp::specfit_workgroups(n_pix);
}

int64_t rjp_gain_apply(rjp_ctx* ctx, const double* d_vis, int32_t n_maps, int32_t n_t,
                       int32_t n_ant, const double* d_gains, int32_t g_maps, const int32_t* h_sol,
                       int32_t n_sol, int32_t mode, double* d_out, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_gain_apply(d_vis, n_maps, n_t, n_ant, d_gains, g_maps, h_sol, n_sol,
                                          mode, d_out, m);
      }))
    return r;
  std::vector<double> sol(h_sol, h_sol + n_t);
  hipStream_t st = (hipStream_t)stream;
  const int r = staged(ctx, st, "gain_apply_launch", nullptr, {{sol.data(), sol.size()}},
                       [&](double* const* d, const double*) {
                         return rjp::gain_apply_launch(d_vis, n_maps, n_t, n_ant, d_gains, g_maps,
                                                       n_sol, d[0], mode, d_out, st);
                       });
  return r ? r : rjp::gain_apply_workgroups(n_maps, n_t, n_ant);
}

size_t rjp_gaincal_workspace(int32_t n_maps, int32_t n_sol, int32_t n_ant) {
  if (n_maps <= 0 || n_sol <= 0 || n_ant < 2 || n_ant > RJP_GAINCAL_MAX_ANT) return 0;
  return rjp::gaincal_workspace_bytes(n_maps, n_sol, n_ant);
}

int64_t rjp_gaincal(rjp_ctx* ctx, const double* d_vis, int32_t n_maps, int32_t n_t, int32_t n_ant,
                    const double* d_model, int32_t model_maps, const double* d_w, int32_t w_maps,
                    const int32_t* h_sol, int32_t n_sol, int32_t mode, int32_t refant,
                    int32_t min_bl, double tol, int32_t n_iter, double* d_gains, double* d_chi2,
                    int32_t* d_nvis, int32_t* d_niter, int32_t* d_status, uint8_t* d_live,
                    double* d_trace, void* d_work, size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_gaincal(d_vis, n_maps, n_t, n_ant, d_model, model_maps, d_w, w_maps,
                                       h_sol, n_sol, mode, refant, min_bl, tol, n_iter, d_gains,
                                       d_chi2, d_nvis, d_niter, d_status, d_live, m);
      }))
    return r;
  if (!d_work || work_bytes < rjp::gaincal_workspace_bytes(n_maps, n_sol, n_ant))
    return fail(ctx, RJP_ERR_WORKSPACE,
                "rjp_gaincal: workspace smaller than rjp_gaincal_workspace()");
  // the first integration of every interval, and n_t
  std::vector<double> t0((size_t)n_sol + 1, (double)n_t);
  for (int t = n_t - 1; t >= 0; --t) t0[h_sol[t]] = (double)t;
  hipStream_t st = (hipStream_t)stream;
  const int r = staged(ctx, st, "gaincal_launch", nullptr, {{t0.data(), t0.size()}},
                       [&](double* const* d, const double*) {
                         return rjp::gaincal_launch(d_vis, d_model, model_maps, d_w, w_maps, n_maps,
                                                    n_t, n_ant, n_sol, d[0], mode, refant, min_bl,
                                                    tol, n_iter, d_gains, d_chi2, d_nvis, d_niter,
                                                    d_status, d_live, d_trace, d_work, st);
                       });
  return r ? r : rjp::gaincal_workgroups(n_maps, n_sol, n_ant);
}

size_t rjp_normal_eq_workspace(int64_t n_rows, int32_t n_vis, int32_t n_sel) {
  if (n_rows < 1 || n_vis < 1 || n_sel < 0 || n_sel > RJP_NORMAL_EQ_MAX_SEL ||
      n_rows > ((int64_t)INT32_MAX * 512) / n_vis)
    return 0;
  return rjp::normal_eq_workspace_bytes(n_rows, n_vis, n_sel);
}

int64_t rjp_normal_eq(rjp_ctx* ctx, const double* d_data, const double* d_model,
                      const double* d_dmodel, int64_t n_rows, int32_t n_vis, int32_t n_part,
                      int32_t n_par, const int32_t* h_sel, int32_t n_sel, const double* d_w,
                      int64_t w_rows, double* d_out, int64_t* d_count, void* d_work,
                      size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_normal_eq(d_data, d_model, d_dmodel, n_rows, n_vis, n_part, n_par,
                                         h_sel, n_sel, d_w, w_rows, d_out, d_count, m);
      }))
    return r;
  if (!d_work || work_bytes < rjp::normal_eq_workspace_bytes(n_rows, n_vis, n_sel))
    return fail(ctx, RJP_ERR_WORKSPACE,
                "rjp_normal_eq: workspace smaller than rjp_normal_eq_workspace()");
  RJP_HIP(ctx, rjp::normal_eq_launch(d_data, d_model, d_dmodel, n_rows, n_vis, n_part, n_par, h_sel,
                                     n_sel, d_w, w_rows, d_out, d_count, d_work,
                                     (hipStream_t)stream));
  return rjp::normal_eq_tiles(n_rows, n_vis);
}

static bool region_sizes_ok(int32_t n_maps, int32_t nx, int32_t nz) {
  std::string m;
  return rjp_args::check_region_sizes("", n_maps, nx, nz, m) == RJP_OK;
}

size_t rjp_image_stats_workspace(int32_t n_maps, int32_t nx, int32_t nz) {
  return region_sizes_ok(n_maps, nx, nz) ? rjp::image_stats_workspace_bytes(n_maps, nx, nz) : 0;
}

int64_t rjp_image_stats(rjp_ctx* ctx, const double* d_img, int32_t n_maps, int32_t nx, int32_t nz,
                        const uint8_t* d_mask, int32_t n_mask, int32_t sense, double* d_stats,
                        void* d_work, size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_image_stats(d_img, n_maps, nx, nz, d_mask, n_mask, d_stats, m);
      }))
    return r;
  if (!d_work || work_bytes < rjp::image_stats_workspace_bytes(n_maps, nx, nz))
    return fail(ctx, RJP_ERR_WORKSPACE,
                "rjp_image_stats: workspace smaller than rjp_image_stats_workspace()");
  if ((uintptr_t)d_work & 7)
    return fail(ctx, RJP_ERR_WORKSPACE, "rjp_image_stats: d_work is not 8-byte aligned");
  RJP_HIP(ctx, rjp::image_stats_launch(d_img, n_maps, nx, nz, d_mask, d_mask ? n_mask : 1, sense,
                                       d_stats, d_work, (hipStream_t)stream));
  return rjp::image_stats_workgroups(n_maps, nx, nz);
}

size_t rjp_label_regions_workspace(int32_t n_maps, int32_t nx, int32_t nz) {
  return region_sizes_ok(n_maps, nx, nz) ? rjp::label_regions_workspace_bytes(n_maps, nx, nz) : 0;
}

int64_t rjp_label_regions(rjp_ctx* ctx, const uint8_t* d_mask_in, int32_t n_mask, int32_t n_maps,
                          int32_t nx, int32_t nz, int32_t connectivity, int32_t* d_label,
                          int32_t* d_area, int32_t* d_nreg, void* d_work, size_t work_bytes,
                          void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_label_regions(d_mask_in, n_mask, n_maps, nx, nz, connectivity,
                                             d_label, d_nreg, m);
      }))
    return r;
  if (!d_work || work_bytes < rjp::label_regions_workspace_bytes(n_maps, nx, nz))
    return fail(ctx, RJP_ERR_WORKSPACE,
                "rjp_label_regions: workspace smaller than rjp_label_regions_workspace()");
  if ((uintptr_t)d_work & 7)
    return fail(ctx, RJP_ERR_WORKSPACE, "rjp_label_regions: d_work is not 8-byte aligned");
  RJP_HIP(ctx, rjp::label_regions_launch(d_mask_in, n_mask, n_maps, nx, nz, connectivity, d_label,
                                         d_area, d_nreg, d_work, (hipStream_t)stream));
  return rjp::regions_workgroups(n_maps, nx, nz);
}

size_t rjp_mask_grow_workspace(int32_t n_maps, int32_t nx, int32_t nz) {
  return region_sizes_ok(n_maps, nx, nz) ? rjp::mask_grow_workspace_bytes(n_maps, nx, nz) : 0;
}

int64_t rjp_mask_grow(rjp_ctx* ctx, uint8_t* d_seed, const uint8_t* d_con, int32_t n_mask,
                      int32_t n_maps, int32_t nx, int32_t nz, int32_t n_iter, int32_t connectivity,
                      void* d_work, size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_mask_grow(d_seed, d_con, n_mask, n_maps, nx, nz, connectivity, m);
      }))
    return r;
  if (!d_work || work_bytes < rjp::mask_grow_workspace_bytes(n_maps, nx, nz))
    return fail(ctx, RJP_ERR_WORKSPACE,
                "rjp_mask_grow: workspace smaller than rjp_mask_grow_workspace()");
  if ((uintptr_t)d_work & 7)
    return fail(ctx, RJP_ERR_WORKSPACE, "rjp_mask_grow: d_work is not 8-byte aligned");
  RJP_HIP(ctx, rjp::mask_grow_launch(d_seed, d_con, n_mask, n_maps, nx, nz, n_iter, connectivity,
                                     d_work, (hipStream_t)stream));
  return rjp::regions_workgroups(n_maps, nx, nz);
}

size_t rjp_uv_weights_workspace(int32_t n_maps, int32_t nx, int32_t nz, int32_t n_vis) {
  if (n_maps <= 0 || nx <= 0 || nz <= 0 || n_vis <= 0) return 0;
  return rjp::uv_weights_workspace_bytes(n_maps, nx, nz, n_vis);
}

int64_t rjp_uv_weights(rjp_ctx* ctx, int32_t n_maps, int32_t n_vis, const double* h_su,
                       const double* h_sv, const double* d_u, const double* d_v, const double* d_w,
                       int32_t nx, int32_t nz, int32_t mode, double robust, double* d_wout,
                       double* d_stats, double* d_density, void* d_work, size_t work_bytes,
                       void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_uv_weights(n_maps, n_vis, h_su, h_sv, d_u, d_v, nx, nz, mode, robust,
                                          d_wout, m);
      }))
    return r;
  const rjp::UvWeightTiling t = rjp::uv_weights_tiling(n_maps, nx, nz, n_vis);
  if (t.cells > (int64_t)INT32_MAX)
    return fail(ctx, RJP_ERR_ARG, "rjp_uv_weights: more than 2^31 - 1 density cells");
  if (t.workgroups > (int64_t)INT32_MAX || t.square_workgroups > (int64_t)INT32_MAX)
    return fail(ctx, RJP_ERR_ARG, "rjp_uv_weights: more than 2^31 - 1 workgroups");
  const size_t need = rjp::uv_weights_workspace_bytes(n_maps, nx, nz, n_vis);
  if (need == 0) return fail(ctx, RJP_ERR_ARG, "rjp_uv_weights: the workspace size overflows");
  if (!d_work || work_bytes < need)
    return fail(ctx, RJP_ERR_WORKSPACE,
                "rjp_uv_weights: workspace smaller than rjp_uv_weights_workspace()");
  double c2 = 0.0;
  if (mode == 2) {
    const double f = 5.0 * std::pow(10.0, -robust);
    c2 = f * f;
  }
  hipStream_t st = (hipStream_t)stream;
  const int r = staged(ctx, st, "uv_weights_launch", nullptr,
                       {{h_su, (size_t)n_maps}, {h_sv, (size_t)n_maps}},
                       [&](double* const* d, const double*) {
                         return rjp::uv_weights_launch(n_maps, n_vis, d[0], d[1], d_u, d_v, d_w, nx,
                                                       nz, mode, c2, d_wout, d_stats, d_density,
                                                       d_work, st);
                       });
  return r ? r : t.workgroups;
}

int64_t rjp_uv_tracks(rjp_ctx* ctx, const double* h_xyz, int32_t n_ant, const double* h_gha,
                      int32_t n_t, double sin_dec, double cos_dec, const double* h_up,
                      double sin_min_el, double* d_u, double* d_v, double* d_w, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_uv_tracks(h_xyz, n_ant, h_gha, n_t, sin_dec, cos_dec, d_u, d_v, m);
      }))
    return r;
  const int64_t wgs = rjp::uv_tracks_workgroups(n_ant, n_t);
  hipStream_t st = (hipStream_t)stream;
  const size_t A = 3 * (size_t)n_ant;
  const int r = staged(ctx, st, "uv_tracks_launch", nullptr,
                       {{h_xyz, A}, {h_gha, (size_t)n_t}, {h_up ? h_up : h_xyz, h_up ? A : 0}},
                       [&](double* const* d, const double*) {
                         return rjp::uv_tracks_launch(d[0], n_ant, d[1], n_t, sin_dec, cos_dec,
                                                      h_up ? d[2] : nullptr, sin_min_el, d_u, d_v,
                                                      d_w, st);
                       });
  return r ? r : wgs;
}

int64_t rjp_vis_noise(rjp_ctx* ctx, const double* d_vis, int32_t n_maps, int32_t n_vis,
                      const double* h_sigma, const double* d_s, uint64_t seed, int64_t k0,
                      int32_t m0, double* d_out, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp_args::check_vis_noise(d_vis, n_maps, n_vis, h_sigma, k0, m0, d_out, m);
      }))
    return r;
  const int64_t wgs = rjp::vis_noise_workgroups(n_maps, n_vis);
  if (wgs > (int64_t)INT32_MAX)
    return fail(ctx, RJP_ERR_ARG, "rjp_vis_noise: more than 2^31 - 1 workgroups");
  hipStream_t st = (hipStream_t)stream;
  const int r = staged(ctx, st, "vis_noise_launch", nullptr, {{h_sigma, (size_t)n_maps}},
                       [&](double* const* d, const double*) {
                         return rjp::vis_noise_launch(d_vis, n_maps, n_vis, d[0], d_s, seed, k0,
                                                      m0, d_out, st);
                       });
  return r ? r : wgs;
}

int rjp_rrl_formal(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                   double time_s, int32_t gff_mode, const rjp_line* line, const double* h_nu,
                   const double* h_ctau, const double* h_csrc, const double* h_hnu_k,
                   int32_t n_chan, const double* d_add, double* d_out, void* stream) {
  if (int r = bind(ctx)) return r;
  if (!mode_ok(gff_mode)) return fail(ctx, RJP_ERR_ARG, "bad gff_mode");
  // the wide fields only: nd, xi, temp, pf, vy (and ts with bursts)
  if (int r = check_fields(ctx, fields, true)) return r;
  if (int r = check_bursts(ctx, bursts, fields)) return r;
  if (!line || !h_nu || !h_ctau || !h_csrc || !h_hnu_k || n_chan < 1 || !d_out)
    return fail(ctx, RJP_ERR_ARG, "rjp_rrl_formal: NULL line / table / output or n_chan < 1");
  hipStream_t st = (hipStream_t)stream;
  const size_t F = (size_t)n_chan;
  return staged(ctx, st, "rrl_formal_launch", bursts,
                {{h_nu, F}, {h_ctau, F}, {h_csrc, F}, {h_hnu_k, F}},
                [&](double* const* d, const double* d_ext) {
                  return rjp::rrl_formal_launch(fields, bursts, d_ext, time_s, gff_mode, line,
                                                h_nu, d[0], d[1], d[2], d[3], n_chan, d_add, d_out,
                                                st);
                });
}

int rjp_rrl_cells(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                  double time_s, const rjp_line* line, const double* h_nu, int32_t n_chan,
                  double* d_tau_cells, void* stream) {
  if (int r = bind(ctx)) return r;
  if (int r = check_fields(ctx, fields, true)) return r;
  if (int r = check_bursts(ctx, bursts, fields)) return r;
  if (!line || !h_nu || n_chan < 1 || !d_tau_cells)
    return fail(ctx, RJP_ERR_ARG, "rjp_rrl_cells: NULL line / nu / output or n_chan < 1");
  hipStream_t st = (hipStream_t)stream;
  return staged(ctx, st, "rrl_cells_launch", bursts, {{h_nu, (size_t)n_chan}},
                [&](double* const* d, const double* d_ext) {
                  return rjp::rrl_cells_launch(fields, bursts, d_ext, time_s, line, h_nu, d[0],
                                               n_chan, d_tau_cells, st);
                });
}

int rjp_rrl_maps(rjp_ctx* ctx, const double* d_tau_rrl, const double* d_tau_ff,
                 const double* d_tavg, const double* d_flux_ff, int64_t n_pix,
                 const double* h_cflux_rrl, const double* h_hnu_k, int32_t n_chan,
                 double* d_flux, double* d_ftot, void* d_work, size_t work_bytes, void* stream) {
  if (int r = bind(ctx)) return r;
  if (!d_tau_rrl || !d_tau_ff || !d_tavg || !h_cflux_rrl || !h_hnu_k)
    return fail(ctx, RJP_ERR_ARG, "rjp_rrl_maps: NULL input");
  if (n_pix <= 0 || n_chan <= 0) return fail(ctx, RJP_ERR_ARG, "rjp_rrl_maps: sizes must be positive");
  if (d_ftot && (!d_work || work_bytes < rjp::ff_maps_workspace_bytes(n_pix, 1, n_chan)))
    return fail(ctx, RJP_ERR_WORKSPACE, "rjp_rrl_maps: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const size_t F = (size_t)n_chan;
  return staged(ctx, st, "rrl_maps_launch", nullptr, {{h_cflux_rrl, F}, {h_hnu_k, F}},
                [&](double* const* d, const double*) {
                  return rjp::rrl_maps_launch(d_tau_rrl, d_tau_ff, d_tavg, d_flux_ff, n_pix, d[0],
                                              d[1], n_chan, d_flux, d_ftot, (double*)d_work, st);
                });
}

int rjp_build_fields(rjp_ctx* ctx, const rjp_geometry* gm, int dtype, void* d_nd, void* d_xi,
                     void* d_temp, void* d_pf, void* d_ts, void* d_vy, double* d_ff_raw,
                     double* d_areas_raw, double* d_vx_raw, double* d_vz_raw, void* d_em0,
                     void* d_a0, int32_t a0_mode, void* stream) {
  if (int r = bind(ctx)) return r;
  if (!gm) return fail(ctx, RJP_ERR_ARG, "geometry is NULL");
  if (dtype != RJP_F32 && dtype != RJP_F64) return fail(ctx, RJP_ERR_ARG, "bad dtype tag");
  if (gm->nx <= 0 || gm->ny <= 0 || gm->nz <= 0 || !(gm->csize > 0))
    return fail(ctx, RJP_ERR_ARG, "bad grid in geometry");
  if (gm->epsilon == 0.0 || gm->mod_r_0 == 0.0)
    return fail(ctx, RJP_ERR_ARG, "rjp_build_fields: epsilon = 0 / mod_r_0 = 0 (a cylindrical jet, "
                                  "for which the reference scales rho = |r| / r_0) is not "
                                  "implemented: every field would be inf or NaN");
  if ((d_em0 || d_a0) && dtype != RJP_F64)
    return fail(ctx, RJP_ERR_ARG, "rjp_build_fields: d_em0 / d_a0 are written for RJP_F64 storage "
                                  "only (float storage goes through rjp_compact_fields' range check)");
  if (d_a0 && !mode_ok(a0_mode)) return fail(ctx, RJP_ERR_ARG, "rjp_build_fields: bad a0_mode");
  rjp::GeomDev g;
  if (int r = checked(ctx, [&](std::string& m) {
        return rjp::geometry_to_dev(gm, d_ts != nullptr, g, m);
      }))
    return r;
  RJP_HIP(ctx, rjp::build_fields_launch(g, dtype, d_nd, d_xi, d_temp, d_pf, d_ts, d_vy, d_ff_raw,
                                        d_areas_raw, d_vx_raw, d_vz_raw, d_em0, d_a0, (int)a0_mode,
                                        (hipStream_t)stream));
  return RJP_OK;
}

int rjp_synth_fields(rjp_ctx* ctx, uint64_t seed, int32_t temp_mode, int32_t nz, int64_t cell0,
                     int64_t n, int dtype, void* d_nd, void* d_xi, void* d_temp, void* d_pf,
                     void* d_ts, void* d_vy, void* d_em0, void* d_a0, int32_t a0_mode,
                     void* stream) {
  if (int r = bind(ctx)) return r;
  if (n <= 0 || nz <= 0 || cell0 < 0) return fail(ctx, RJP_ERR_ARG, "rjp_synth_fields: bad range");
  if (dtype != RJP_F32 && dtype != RJP_F64) return fail(ctx, RJP_ERR_ARG, "bad dtype tag");
  if ((d_em0 || d_a0) && dtype != RJP_F64)
    return fail(ctx, RJP_ERR_ARG, "rjp_synth_fields: d_em0 / d_a0 are written for RJP_F64 storage only");
  if (d_a0 && !mode_ok(a0_mode)) return fail(ctx, RJP_ERR_ARG, "rjp_synth_fields: bad a0_mode");
  RJP_HIP(ctx, rjp::synth_launch(seed, temp_mode, nz, cell0, n, dtype, d_nd, d_xi, d_temp, d_pf,
                                 d_ts, d_vy, d_em0, d_a0, (int)a0_mode, (hipStream_t)stream));
  return RJP_OK;
}

}  // extern "C"
