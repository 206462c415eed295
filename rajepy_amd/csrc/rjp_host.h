// Host-side interface between the translation units of librjprt (rjprt.hip = the C-ABI,
// ff_scan.hip, ff_scan_inst.hip x 5, fields.hip, rrl_scan.hip, rrl_formal.hip, ff_grad.hip,
// ff_formal_sweep.hip, ff_formal_grad.hip, vis.hip, vis_adjoint.hip, clean.hip, imfit.hip, uv_weight.hip, observe.hip, ...): launch
// wrappers and the small structs they exchange.  Nothing here is exported; the library's surface is include/rjprt.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "rjp_device.h"

namespace rjp {

// ---- ff_scan.hip --------------------------------------------------------------------------
// The epoch tiling of one scan, decided on the host before anything is enqueued, so that the
// constants of bursts beyond RJP_SGPR_BURSTS (parameters + one q per tile) and the step tables
// of the uniform-epoch tiles can travel to the device in ONE small table:
// ext = [params: 6 * next][tile 0: q (2 * next), step table (2 * nbt * 16 or 0)][tile 1 ...] ...
struct ScanTile {
  int e0, et;
  UnifDev un;          // un.qext / un.atab are patched to the device table by ff_scan_run
  size_t q_off, a_off; // offsets of the tile's q and step table in ScanPlan::ext
  int nsplit, ylen;    // y-ranges of this tile's launch
};
struct ScanPlan {
  bool bursts = false;
  int vec = 1, next = 0;
  std::vector<ScanTile> tiles;
  std::vector<double> ext;       // host image of the overflow table (empty without overflow)
};

// which fields a scan kernel streams (scan_layout)
enum : int {
  LAY_WIDE = 0,            // nd, xi, temp, pf, ts
  LAY_CMP = 1,             // em0, temp, ts
  LAY_TAU = 2              // a0, ts (+ em0 with emission-measure maps); no T_avg sums
};

int ff_scan_vec(const rjp_fields* fl);
int scan_layout(const rjp_fields* fl, int mode, bool want_em);
bool tile_dma_ok(const rjp_fields* fl);
size_t ff_scan_workspace_bytes(int nx, int ny, int nz, int n_epochs);
void ff_scan_plan(const rjp_fields* fl, const rjp_bursts* hb, const double* epochs, int n_epochs,
                  int mode, bool want_em, ScanPlan& pl);
hipError_t ff_scan_run(const rjp_fields* fl, const rjp_bursts* hb, const ScanPlan& pl,
                       const double* d_ext, const double* epochs, int n_epochs, int mode,
                       double* sumA, double* em, double* tavg, double* ws, hipStream_t st);
hipError_t tavg_launch(const rjp_fields* fl, double* tavg, double* ws, hipStream_t st);
hipError_t y_bounds_launch(const rjp_fields* fl, int32_t* ylo, int32_t* yhi, hipStream_t st);
hipError_t occupied_launch(const int32_t* ylo, const int32_t* yhi, int64_t npix,
                           unsigned long long* d_count, hipStream_t st);
hipError_t ff_cells_launch(const rjp_fields* fl, const rjp_bursts* hb, const double* d_ext,
                           double time_s, int mode, const double* d_ctau, int nchan, double* out,
                           hipStream_t st);
// ff_formal.hip: the formal solution along the line of sight (K5), out[F * P]
hipError_t ff_formal_launch(const rjp_fields* fl, const rjp_bursts* hb, const double* d_ext,
                            double time_s, int mode, const double* d_ctau, const double* d_csrc,
                            int nchan, double* out, hipStream_t st);
// ff_formal_sweep.hip: K5's maps at E epochs and their totals from one pass (K8), out[E * F * P]
// and / or ftot[E * F]; `part` (ff_formal_sweep_workspace_bytes) only with ftot
size_t ff_formal_sweep_workspace_bytes(int nx, int nz, int n_epochs, int n_chan);
hipError_t ff_formal_sweep_launch(const rjp_fields* fl, const rjp_bursts* hb, const double* d_ext,
                                  const double* d_epochs, int n_epochs, int mode,
                                  const double* d_ctau, const double* d_csrc, int nchan,
                                  double* out, double* ftot, double* part, hipStream_t st);
size_t ff_maps_workspace_bytes(int64_t npix, int n_epochs, int n_chan);
hipError_t ff_maps_launch(const double* sumA, const double* tavg, int64_t npix, int n_epochs,
                          const double* d_ctau, const double* d_cflux, int n_chan, double* tau,
                          double* flux, double* ftot, double* part, hipStream_t st,
                          int32_t* info = nullptr);
// out[row] = sum of part[row * nblk .. + nblk) in a fixed order
hipError_t sum_partials_launch(const double* part, int rows, int nblk, double* out,
                               hipStream_t st);

// fixed-order reduction of the y-range partials of one tile (ff_reduce_kernel)
hipError_t ff_reduce_launch(const double* ws, int nsplit, int et, int64_t npix, int e0,
                            double em_scale, double* sumA, double* em, double* tavg,
                            hipStream_t st);

// ---- ff_scan_tab.hip: single-epoch tau-layout scan with the burst factor from an LDS table -----
struct ChiPlan {
  bool ok = false;
  bool wide = false;              // the scan reads the five model fields, not the tau layout
  int ni = 0, n[2] = {0, 0};
  double lo = 0.0, inv_h = 0.0;
  std::vector<double> stage;      // Vandermonde inverse, nodes, burst parameters
  mutable bool attr_set = false;  // the kernels' dynamic-LDS limit was raised on this context's device
};
size_t chi_table_workspace_bytes(int64_t npix, int ny);
bool chi_table_plan(const rjp_fields* fl, const rjp_bursts* hb, const double* epochs, int n_epochs,
                    int mode, bool want_em, size_t work_bytes, ChiPlan& cp);
// the bins a single-epoch scan reads from the launch-time-bucketed layout: per jet [b0, b1) (the
// bins that meet the jet's bursts' support at the epoch; empty for a jet without bursts)
constexpr int kSrtDiagWords = 4;  // words per group in SrtPlan::diag
struct SrtPlan {
  int b0[2] = {0, 0}, b1[2] = {0, 0};
  int hb[2] = {0, 0};             // the jet has bursts
  double share = 0.0;             // the map's cells in those bins / all cells in the layout
  // Chebyshev moments of the layout attached (rjp_fields.d_srt_mom): their order N, else 0.  The
  // bins in the support whose chi^2 the degree-(N-1) interpolant matches are contracted from them
  unsigned long long* diag = nullptr;   // (contracted, read, residual) bin and fallback-cell counters of the scan, four per group, or null
  int N = 0;
  // the packed state is attached (rjp_fields.d_srt_pts / d_srt_pw): bins that fail check (b) alone
  // may be taken as table-residual bins (ff_scan_tab.hip)
  bool packed = false;
  // ... and with it its launch-time codes (rjp_fields.d_srt_pc): the residual stream reads 6 bytes
  // per cell, not 10
  bool codes = false;
};
// false: no layout attached, or too large a share of it would be read (the grid order is as fast)
bool srt_plan(const rjp_fields* fl, const rjp_bursts* hb, double t_epoch, SrtPlan& sp);
// Tables ahead of the scan: chi_table_kernel and srt_coef_kernel depend on host arguments and the
// staged burst table only, so a context builds them on a side stream of its own, into one of
// kSlots table slots, while the caller's stream still runs what was enqueued before.  The slots
// are ordered by stream events alone: `ready` (side stream, behind the table kernels; the
// caller's stream waits for it in front of the scan) and `readers_done` (caller's stream, behind
// the scan; the side stream waits for it before the slot is written again).  An event record
// costs the stream it is made on about 6 us between two kernels (profiles/README.md, r19), so
// `readers_done` is no event of the ring's own: it is the event the CALLER records behind the
// scan anyway (`release_ev`, the release event of the staged burst table), borrowed.  Recorded
// again by a later scan it only orders the side stream behind that later scan.
struct TabRing {
  static constexpr int kSlots = 4;
  hipStream_t side = nullptr;     // non-blocking; null: the tables stay on the caller's stream
  void* mem = nullptr;            // one allocation for every slot
  struct Slot {
    double* tab = nullptr;        // [2][kChiMaxNI][kChiStride]
    double* W = nullptr;          // [2 RJP_SRT_MAX_K][kSrtMaxN]
    int* ok = nullptr;            // [2 RJP_SRT_MAX_K]
    float* E = nullptr;           // [2][kChiMaxNI][kErrStride]: the table's own error, per piece
    hipEvent_t ready = nullptr;
    hipEvent_t readers_done = nullptr;   // borrowed: the release_ev of the slot's last scan
    hipEvent_t uploaded = nullptr;   // caller's stream, behind a fresh upload of the burst table
  } slot[kSlots];
  int next = 0;
};
// (a ring that could not be created is left without a side stream: the scans then keep the
// single-stream order)
void tab_ring_create(TabRing& r);
void tab_ring_destroy(TabRing& r);
// `stage_fresh`: the side stream has not yet been ordered behind the upload of `d_stage`; cleared
// once it has been.  `release_ev`: the event the caller records on `st` when this returns, on
// every path (null: the tables stay on the caller's stream)
hipError_t chi_table_scan(const rjp_fields* fl, const ChiPlan& cp, const double* d_stage,
                          double t_epoch, int mode, double* sumA, double* em, double* tavg,
                          double* ws, size_t work_bytes, int* d_guard, hipStream_t st,
                          const SrtPlan* sp = nullptr, TabRing* ring = nullptr,
                          bool* stage_fresh = nullptr, hipEvent_t release_ev = nullptr);

// ---- ff_moments.hip: epoch sweeps by launch-time moments --------------------------------------
#define RJP_MOM_MAX_IDX 1280      /* 2 jets x K bins x N Chebyshev moments <= this (160 KB of LDS
                                    for 16 sightlines); the (K, N) shapes: ff_moments.hip */
#define RJP_MOM_TILE 32          /* epochs per pass of the contraction */
#define RJP_MOM_MIN_EPOCHS 12    /* below: the epoch tiles are faster */
#define RJP_MOM_TOL 1e-11        /* worst relative error of the expansion the host accepts */
#define RJP_MOM_MAX_CAND 12     /* (bins, order) shapes tried in one table build */
#define RJP_MOM_NMAX 32         /* highest Chebyshev order of any shape */
struct MomCand {
  int K, N;
  int path;                      // 1 = LDS moments, 2 = launch-time-ordered layout
  size_t w_off;                  // doubles: this shape's tables in MomPlan::d_W
  size_t tab_off;                // doubles: its nodes x[N] and DCT matrix cs[N][N] in MomPlan::stage
};
struct MomPlan {
  bool ok = false;
  int path = 0;                  // 1 = LDS moments + contraction, 2 = launch-time-ordered layout
  double s0 = 0.0, inv_h = 0.0, worst = 0.0;
  int has_bursts[2] = {0, 0};
  int nchunk = 0;
  int K = 0, N = 0;              // the shape in use
  const double* d_Wsel = nullptr;   // its tables, [chunk][2 * K * N][TILE], on the device
  // device / pinned state of the table builder (owned; moments_release frees it)
  double* d_W = nullptr;
  size_t capW = 0;               // doubles
  unsigned long long* d_err = nullptr;
  unsigned long long* h_err = nullptr;
  // one table build: the staged host table (bursts, epochs, nodes + DCT matrices) and shapes
  std::vector<double> stage;
  std::vector<MomCand> cands;
  size_t w_total = 0, off_bursts[2] = {0, 0}, off_epochs = 0;
  double build_ms = 0.0;         // host wall time of the last table build (incl. its one sync)
  // the request the tables were built for (a sweep repeated with the same epochs reuses them)
  int key_E = -1, key_n[2] = {0, 0}, key_ltK = -1;
  bool key_ok = false;
  double key_lo = 0.0, key_hi = 0.0;
  std::vector<double> key_epochs, key_bursts;
  mutable bool attr_set[3] = {false, false, false};   // dynamic-LDS limit raised, per LDS shape
};
size_t moments_workspace_bytes(int64_t npix);
size_t moments_scan_workspace_bytes(int64_t npix);
// 0 = this scan keeps the epoch tiles, 1 = moment path with the tables already on the device,
// 2 = moment path after moments_build() (mp.stage has to be staged first)
int moments_plan(const rjp_fields* fl, const rjp_bursts* hb, const double* epochs, int n_epochs,
                 int mode, bool want_em, size_t work_bytes, MomPlan& mp);
// builds and checks the tables of every candidate shape on the device (one launch, one 64-byte
// copy back, ONE stream synchronisation) and selects the cheapest shape that passes; mp.ok says
// whether one did.  `d_stage` = device copy of mp.stage.
hipError_t moments_build(MomPlan& mp, const double* d_stage, hipStream_t st);
void moments_release(MomPlan& mp);
hipError_t moments_run(const rjp_fields* fl, const MomPlan& mp, int n_epochs,
                       double* sumA, double* ws, double* part, hipStream_t st,
                       const double* weights, double scale, int* d_guard, bool skip_pass = false);
// launch-time-ordered layout (ff_lt.hip)
#define RJP_LT_MAX_K 80
#define RJP_LT_MAX_EPOCHS 32     /* one fused pass serves one contraction tile */
size_t lt_rowoff_entries(int nx, int nz, int K);
hipError_t lt_count_launch(const rjp_fields* fl, int K, int32_t* d_rowoff, int* d_guard,
                           hipStream_t st);
hipError_t lt_fill_launch(const rjp_fields* fl, int K, const int32_t* d_rowoff, void* d_cells,
                          double* d_aux, hipStream_t st);
hipError_t lt_run(const rjp_fields* fl, const MomPlan& mp, int n_epochs, double* sumA, double* ws,
                  size_t work_bytes, hipStream_t st);
// launch-time-bucketed layout for single-epoch scans (ff_lt.hip; its scan: ff_scan_tab.hip)
#define RJP_SRT_MAX_K 32         /* the fill pass keeps 12 bytes per (lane, key) in LDS: 48 KiB */
size_t srt_index_entries(int nx, int nz, int K);
hipError_t srt_count_launch(const rjp_fields* fl, int K, int32_t* d_start, int64_t* d_rowbase,
                            unsigned long long* d_hist, int* d_guard, hipStream_t st);
hipError_t srt_fill_launch(const rjp_fields* fl, int K, const int32_t* d_start,
                           const int64_t* d_rowbase, void* d_cells, double* d_cum, double* d_aux,
                           hipStream_t st);
// orders of the layout's Chebyshev moments (rjp_fields.srt_N) the kernels are instantiated for
inline bool srt_moment_order_ok(int N) { return N == 16 || N == 20 || N == 24; }
size_t srt_moment_entries(int nx, int nz, int K, int N);
hipError_t srt_moments_launch(const rjp_fields* fl, int K, int N, const int32_t* d_start,
                              const int64_t* d_rowbase, const void* d_cells, double* d_mom,
                              hipStream_t st);
// the packed state of the layout (rjp_fields.d_srt_pts / d_srt_pw): rows of group g start at
// srt_packed_row(d_srt_rowbase[g], g), a multiple of 8 that leaves every group its rows rounded
// up to 8; srt_packed_rows(total, G) rows hold every group
__host__ __device__ inline int64_t srt_packed_row(int64_t rowbase, int64_t g) { return ((rowbase + 7) & ~(int64_t)7) + 8 * g; }
inline int64_t srt_packed_rows(int64_t total_rows, int64_t groups) { return srt_packed_row(total_rows, groups); }
hipError_t srt_pack_launch(const rjp_fields* fl, int K, const int32_t* d_start,
                           const int64_t* d_rowbase, const void* d_cells, void* d_pts, void* d_pw,
                           int* d_flag, hipStream_t st);
// the launch-time codes of the packed state (rjp_fields.d_srt_pc, ff_lt.hip): 4 bytes per cell in
// the packed state's rows, code = floor((ts - ts_lo) * srt_code_scale), saturating at 2^32 - 1
inline double srt_code_scale(const rjp_fields* fl) {
  const double span = fl->ts_hi - fl->ts_lo;
  return span > 0.0 ? 4294967296.0 / span : 0.0;
}
hipError_t srt_codes_launch(const rjp_fields* fl, int K, const int32_t* d_start,
                            const int64_t* d_rowbase, const void* d_cells, void* d_pc,
                            hipStream_t st);
hipError_t field_range_launch(const void* d_field, int64_t n, int dtype, double* d_part,
                              hipStream_t st);
hipError_t range_check_launch(const void* d_field, int64_t n, int dtype, double lo, double hi,
                              int* d_flag, hipStream_t st);

// ---- ff_grad.hip: sensitivities to the burst parameters (K7) -----------------------------------
size_t ff_grad_workspace_bytes(int nx, int ny, int nz, int n_epochs, int npar, int nchan);
// d_scale[1 + npar]: 1, then per parameter the constant its plane is multiplied with (2 amp inv2s2
// for t0, 1 for amp_rel, -amp for inv2s2); d_tavg / d_ctau / d_cflux only with ftot or dftot
hipError_t ff_grad_run(const rjp_fields* fl, const rjp_bursts* hb, const double* epochs,
                       int n_epochs, const double* d_scale, const double* d_tavg,
                       const double* d_ctau, const double* d_cflux, int nchan, double* sumA,
                       double* dsumA, double* ftot, double* dftot, double* ws, size_t work_bytes,
                       hipStream_t st);

// ---- ff_formal_grad.hip: sensitivities of K8's light curves to the burst parameters (K9) -------
size_t ff_formal_grad_workspace_bytes(int nx, int nz, int n_epochs, int n_par, int n_chan);
// d_scale[npar]: the constant each parameter's plane is multiplied with (2 amp inv2s2 for t0, 1
// for amp_rel, -amp for inv2s2); `work` (ff_formal_grad_workspace_bytes) with ftot or dftot
hipError_t ff_formal_grad_launch(const rjp_fields* fl, const rjp_bursts* hb,
                                 const double* d_epochs, int n_epochs, int mode,
                                 const double* d_ctau, const double* d_csrc, int nchan,
                                 const double* d_scale, double* ftot, double* dftot, double* dout,
                                 double* work, hipStream_t st);

// ---- vis.hip: visibilities of a stack of maps at given (u, v) points (K10) ----------------------
// rows per thread of K10's and K11's tiles of 16 row groups -- the two tile alike: (nx + 1) / 2
// rows would idle in a 128-row tile below this
static inline int vis_rows_per_thread(int nx) { return nx > 64 ? 8 : 4; }
// out[m][c] = sum over r < n, in that order, of part[(m n + r) per + c] (K10's row tiles, K11's
// k-splits); one launch
hipError_t partial_combine_launch(const double* part, int n_maps, int n, int64_t per, double* out,
                                  hipStream_t st);
size_t vis_workspace_bytes(int n_maps, int nx, int nz, int n_vis);
// false: more workgroups than one launch takes
bool vis_grid_ok(int n_maps, int nx, int n_vis);
// d_su / d_sv[n_maps]: device copies of the scales; `part` (vis_workspace_bytes) holds the row
// tiles' partial sums when nx spans more than one tile
hipError_t vis_launch(const double* maps, int n_maps, int nx, int nz, const double* d_su,
                      const double* d_sv, const double* u, const double* v, int n_vis, double* vis,
                      double* part, hipStream_t st);

// ---- vis_adjoint.hip: dirty images from visibilities, the transpose of K10 (K11) ----------------
struct VisAdjointTiling {
  int row_tiles, col_tiles;     // of 128 (nx > 64) or 64 rows x 128 columns
  int k_splits;                 // ranges of visibilities over workgroups ...
  int64_t k_per_split;          // ... of this many each, a multiple of 16 (may pass 2^31 - 1)
  int64_t workgroups;           // n_maps x row_tiles x col_tiles x k_splits; INT64_MAX: too many
};
VisAdjointTiling vis_adjoint_tiling(int n_maps, int nx, int nz, int n_vis);
// >= 16; 0: does not fit a size_t
size_t vis_adjoint_workspace_bytes(int n_maps, int nx, int nz, int n_vis);
// d_su / d_sv[n_maps]: device copies of the scales; `w` may be nullptr (all ones); `part`
// (vis_adjoint_workspace_bytes) holds the k-splits' partial images when there are any
hipError_t vis_adjoint_launch(const double* vis, int n_maps, int n_vis, const double* d_su,
                              const double* d_sv, const double* u, const double* v, const double* w,
                              int nx, int nz, double* img, double* part, hipStream_t st);

// ---- clean.hip: Hogbom CLEAN on a stack of images (K12) and the restored image (K13) -------------
struct CleanTiling {
  int64_t tiles;                // of 1024 consecutive pixels, per map
  int64_t workgroups;           // n_maps x tiles: the grid of every iteration's launch
};
CleanTiling clean_tiling(int n_maps, int nx, int nz);
// >= 16; 0: does not fit a size_t
size_t clean_workspace_bytes(int n_maps, int nx, int nz);
// d_thresh[n_maps]: device copy of the thresholds; `mask`, `model`, `peak` may be nullptr;
// 1 + n_iter (+ 1 with `peak`) launches, no host synchronisation
hipError_t clean_launch(double* res, int n_maps, int nx, int nz, const double* psf, int n_psf,
                        int px, int pz, const uint8_t* mask, const double* d_thresh, double gain,
                        int n_iter, int32_t* cpix, double* cflux, int32_t* ncomp, double* model,
                        double* peak, void* work, hipStream_t st);
int64_t restore_workgroups(int n_maps, int nx, int nz);
// d_beam[n_maps][3]: device copy of the quadratic forms; `add` may be nullptr
hipError_t restore_launch(const int32_t* cpix, const double* cflux, const int32_t* ncomp,
                          int n_maps, int comp_stride, const double* d_beam, const double* add,
                          int nx, int nz, double* out, hipStream_t st);

// ---- convolve.hip: direct 2-D convolution of a stack of images (rjp_convolve2d) -------------------
struct ConvTiling {
  int64_t tiles_x, tiles_z;     // of 16 rows x 64 columns of the output
  int64_t workgroups;           // n_maps x tiles_x x tiles_z: the grid
};
ConvTiling conv_tiling(int n_maps, int nx, int nz);
// kernel rows per LDS chunk (>= 1 for kz <= RJP_CONV_MAX_K)
int conv_chunk_rows(int kx, int kz);
// `add` may be nullptr; one launch
hipError_t convolve2d_launch(const double* in, int n_maps, int nx, int nz, const double* ker,
                             int n_ker, int kx, int kz, const double* add, double* out,
                             hipStream_t st);

// ---- msclean.hip: multi-scale CLEAN on a stack of maps of n_s planes each (K17) ------------------
struct MsCleanTiling {
  int64_t tiles;                // of 1024 consecutive pixels, per plane
  int64_t workgroups;           // n_maps x n_s x tiles: the grid of every iteration's launch
                                // (INT64_MAX: beyond int64)
};
MsCleanTiling msclean_tiling(int n_maps, int n_s, int nx, int nz);
// >= 16; 0: does not fit a size_t
size_t msclean_workspace_bytes(int n_maps, int n_s, int nx, int nz);
// d_weight[n_maps][n_s], d_thresh[n_maps]: device copies; `mask`, `model`, `peak` may be nullptr;
// 1 + n_iter (+ 1 with `peak`) launches, no host synchronisation
hipError_t msclean_launch(double* res, int n_maps, int n_s, int nx, int nz, const double* xpsf,
                          int n_psf, int px, int pz, const double* d_weight, const uint8_t* mask,
                          const double* d_thresh, double gain, int n_iter, int32_t* cpix,
                          int32_t* cscale, double* cflux, int32_t* ncomp, double* model,
                          double* peak, void* work, hipStream_t st);

// ---- mtmfs.hip: multi-term MFS CLEAN on a stack of maps of n_t Taylor planes each (K19) ------------
struct MtmfsTiling {
  int64_t tiles;                // of 1024 consecutive pixels, per map (a workgroup holds all planes)
  int64_t workgroups;           // n_maps x tiles: the grid of every iteration's launch
};
MtmfsTiling mtmfs_tiling(int n_maps, int nx, int nz);
// >= 16; 0: does not fit a size_t
size_t mtmfs_workspace_bytes(int n_maps, int n_t, int nx, int nz);
// d_hinv[n_maps][n_t][n_t], d_thresh[n_maps]: device copies; `mask`, `model`, `peak` may be nullptr;
// 1 <= n_t <= RJP_MTMFS_MAX_NT; 1 + n_iter (+ 1 with `peak`) launches, no host synchronisation
hipError_t mtmfs_launch(double* res, int n_maps, int n_t, int nx, int nz, const double* spsf,
                        int n_psf, int px, int pz, const double* d_hinv, const uint8_t* mask,
                        const double* d_thresh, double gain, int n_iter, int32_t* cpix,
                        double* ccoef, int32_t* ncomp, double* model, double* peak, void* work,
                        hipStream_t st);

// ---- vis_components.hip: visibilities (K18) and the delta model image of a component list ---------
int64_t vis_components_workgroups(int n_maps, int n_vis);            // n_maps x ceil(n_vis / 64)
int64_t components_image_workgroups(int n_maps, int n_s, int nx, int nz);
// d_su / d_sv[n_maps]: device copies of the scales; `cscale`, `gvis`, `in` may be nullptr; `out` may
// be `in`; one launch
hipError_t vis_components_launch(const int32_t* cpix, const int32_t* cscale, const double* cflux,
                                 const int32_t* ncomp, int n_maps, int comp_stride, int n_s, int nx,
                                 int nz, const double* d_su, const double* d_sv, const double* u,
                                 const double* v, int n_vis, const double* gvis, const double* in,
                                 int sign, double* out, hipStream_t st);
// `cscale` may be nullptr; one launch
hipError_t components_image_launch(const int32_t* cpix, const int32_t* cscale, const double* cflux,
                                   const int32_t* ncomp, int n_maps, int comp_stride, int n_s,
                                   int nx, int nz, double* out, hipStream_t st);

// ---- lm_common.h: what the Levenberg-Marquardt fits share; the tiling of K14 and K20 -------------
struct LmTiling {
  int64_t tiles;                // of 1024 consecutive items (pixels of the box, visibilities), per map
  int64_t workgroups;           // n_maps x tiles: the grid of every iteration's launch
};

// ---- imfit.hip: Levenberg-Marquardt fits of one elliptical Gaussian per map (K14) ----------------
LmTiling gaussfit_tiling(int n_maps, int64_t box_pixels);
// 0: does not fit a size_t
size_t gaussfit_workspace_bytes(int n_maps, int64_t box_pixels);
// `box`: HOST (i0, i1, j0, j1); `mask`, `trace` may be nullptr; n_iter + 1 launches, no host
// synchronisation
hipError_t gaussfit_launch(const double* img, int n_maps, int nx, int nz, const int32_t* box,
                           const uint8_t* mask, double* theta, double lambda0, double xtol,
                           int n_iter, double* chi2, double* cov, int32_t* npix, int32_t* niter,
                           int32_t* status, double* trace, void* work, hipStream_t st);

// ---- uvfit.hip: Levenberg-Marquardt fits of point / Gaussian components to visibilities (K20) ----
LmTiling uvfit_tiling(int n_maps, int64_t n_vis);
// n_comp 1 or 2; 0: does not fit a size_t
size_t uvfit_workspace_bytes(int n_maps, int64_t n_vis, int n_comp);
// d_su / d_sv[n_maps]: device copies of the scales; `free_bits`: bit i set = parameter i is fitted;
// `w`, `trace` may be nullptr; n_comp 1 or 2; n_iter + 1 launches, no host synchronisation
hipError_t uvfit_launch(const double* vis, int n_maps, int n_vis, const double* d_su,
                        const double* d_sv, const double* u, const double* v, const double* w,
                        int w_maps, int n_comp, unsigned free_bits, double* theta, double lambda0,
                        double xtol, int n_iter, double* chi2, double* cov, int32_t* nvis,
                        int32_t* niter, int32_t* status, double* trace, void* work,
                        hipStream_t st);

// ---- specfit.hip: moment maps and per-sightline Gaussian fits of a line cube (K21) ---------------
// workgroups of 64 pixels, one lane per pixel: the grid of both launches
int64_t specfit_workgroups(int64_t n_pix);
// d_x, d_dx [n_chan]: device copies of the tables; `mask`, `ipeak`, `count` may be nullptr
hipError_t cube_moments_launch(const double* cube, int64_t n_pix, int n_chan, const double* d_x,
                               const double* d_dx, double x_ref, double clip, const uint8_t* mask,
                               double* mom, int32_t* ipeak, int32_t* count, hipStream_t st);
// d_w (nullptr: all ones), `mask`, `trace` may be nullptr; n_comp 1 or 2; `free_bits`: bit i set =
// parameter i is fitted; ONE launch, no host synchronisation
hipError_t specfit_launch(const double* cube, int64_t n_pix, int n_chan, const double* d_x,
                          const double* d_w, double x_ref, const uint8_t* mask, int n_comp,
                          unsigned free_bits, double* theta, double lambda0, double xtol,
                          int n_iter, double* chi2, double* cov, int32_t* nchan, int32_t* niter,
                          int32_t* status, double* trace, hipStream_t st);

// ---- voigtfit.hip: per-sightline Voigt fits of a line cube (K24) ---------------------------------
// specfit_launch's arguments and grid (specfit_workgroups); `free_bits` over the 4 n_comp + 2
// parameters (F, x0, s, g per component, b0, b1)
hipError_t voigtfit_launch(const double* cube, int64_t n_pix, int n_chan, const double* d_x,
                           const double* d_w, double x_ref, const uint8_t* mask, int n_comp,
                           unsigned free_bits, double* theta, double lambda0, double xtol,
                           int n_iter, double* chi2, double* cov, int32_t* nchan, int32_t* niter,
                           int32_t* status, double* trace, hipStream_t st);

// ---- gaincal.hip: antenna-based complex gains (K22) ----------------------------------------------
// one thread per visibility, workgroups of 256
int64_t gain_apply_workgroups(int n_maps, int n_t, int n_ant);
// accumulate (256 (m, s, pq) each) + one solve and one residual workgroup per (m, s)
int64_t gaincal_workgroups(int n_maps, int n_sol, int n_ant);
size_t gaincal_workspace_bytes(int n_maps, int n_sol, int n_ant);
// d_sol [n_t]: the interval of every integration, as doubles; `out` may be `vis`
hipError_t gain_apply_launch(const double* vis, int n_maps, int n_t, int n_ant, const double* gains,
                             int g_maps, int n_sol, const double* d_sol, int mode, double* out,
                             hipStream_t st);
// d_t0 [n_sol + 1]: the first integration of every interval and n_t, as doubles; `w`, `trace` may
// be nullptr; three launches, no host synchronisation
hipError_t gaincal_launch(const double* vis, const double* model, int model_maps, const double* w,
                          int w_maps, int n_maps, int n_t, int n_ant, int n_sol, const double* d_t0,
                          int mode, int refant, int min_bl, double tol, int n_iter, double* gains,
                          double* chi2, int32_t* nvis, int32_t* niter, int32_t* status,
                          uint8_t* live, double* trace, void* work, hipStream_t st);

// ---- normal_eq.hip: normal equations from data, model and derivative stacks (K23) ---------------
// tiles of 512 consecutive flattened samples = the workgroups of the first launch
int64_t normal_eq_tiles(int64_t n_rows, int n_vis);
size_t normal_eq_workspace_bytes(int64_t n_rows, int n_vis, int n_sel);
// `dmodel`, `h_sel` may be nullptr with n_sel = 0, `w` may be nullptr; two launches, no host
// synchronisation (h_sel travels as a kernel argument)
hipError_t normal_eq_launch(const double* data, const double* model, const double* dmodel,
                            int64_t n_rows, int n_vis, int n_part, int n_par, const int32_t* h_sel,
                            int n_sel, const double* w, int64_t w_rows, double* out, int64_t* count,
                            void* work, hipStream_t st);

// ---- regions.hip: robust image statistics, connected components, constrained growth (K25) -------
// n_maps x tiles of 2048 consecutive pixels: the grid of the statistics' tile launches
int64_t image_stats_workgroups(int n_maps, int nx, int nz);
// n_maps x tiles of 16 x 64 pixels: the grid of the labelling's and the growth's tile launches
int64_t regions_workgroups(int n_maps, int nx, int nz);
size_t image_stats_workspace_bytes(int n_maps, int nx, int nz);
size_t label_regions_workspace_bytes(int n_maps, int nx, int nz);
size_t mask_grow_workspace_bytes(int n_maps, int nx, int nz);
// `mask` may be nullptr; 26 launches, no host synchronisation
hipError_t image_stats_launch(const double* img, int n_maps, int nx, int nz, const uint8_t* mask,
                              int n_mask, int sense, double* stats, void* work, hipStream_t st);
// `area` may be nullptr; up to three memsets and four launches, no host synchronisation.  The first
// int32 of `work` is the cap flag (0 = no loop ran into its cap)
hipError_t label_regions_launch(const uint8_t* mask, int n_mask, int n_maps, int nx, int nz,
                                int conn, int32_t* label, int32_t* area, int32_t* nreg, void* work,
                                hipStream_t st);
// n_iter > 0: ceil(n_iter / RJP_GROW_HALO) launches; < 0: the labelling's launches and two more; the
// cap flag as above
hipError_t mask_grow_launch(uint8_t* seed, const uint8_t* con, int n_mask, int n_maps, int nx,
                            int nz, int n_iter, int conn, void* work, hipStream_t st);

// ---- uv_weight.hip: uniform and Briggs imaging weights from the (u, v) density (K15) -------------
struct UvWeightTiling {
  int64_t cells;                // (2 (nx / 2) + 1)(2 (nz / 2) + 1), per map (INT64_MAX: beyond int64)
  int64_t workgroups;           // n_maps x ceil(n_vis / 256): the grid of the scatter launch
  int64_t square_workgroups;    // n_maps x tiles of 1024 cells: the grid of the sum of W^2
};
UvWeightTiling uv_weights_tiling(int n_maps, int nx, int nz, int n_vis);
// 0: does not fit a size_t
size_t uv_weights_workspace_bytes(int n_maps, int nx, int nz, int n_vis);
// `c2` = (5 10^-robust)^2 (mode 2); `w`, `stats`, `density` may be nullptr; one memset and five
// launches, no host synchronisation
hipError_t uv_weights_launch(int n_maps, int n_vis, const double* d_su, const double* d_sv,
                             const double* u, const double* v, const double* w, int nx, int nz,
                             int mode, double c2, double* wout, double* stats, double* density,
                             void* work, hipStream_t st);

// ---- observe.hip: (u, v, w) tracks of an array and thermal noise on visibilities (K16) ------------
// n_t x ceil(n_bl / 256), n_bl = n_ant (n_ant - 1) / 2
int64_t uv_tracks_workgroups(int n_ant, int n_t);
// d_xyz[n_ant][3], d_gha[n_t], d_up[n_ant][3] (or nullptr): device copies of the host tables; `w`
// may be nullptr; one launch
hipError_t uv_tracks_launch(const double* d_xyz, int n_ant, const double* d_gha, int n_t,
                            double sin_dec, double cos_dec, const double* d_up, double sin_min_el,
                            double* u, double* v, double* w, hipStream_t st);
// n_maps x ceil(n_vis / 256)
int64_t vis_noise_workgroups(int n_maps, int n_vis);
// d_sigma[n_maps]: device copy of the rms per map; `s` may be nullptr; `out` may be `vis`; one launch
hipError_t vis_noise_launch(const double* vis, int n_maps, int n_vis, const double* d_sigma,
                            const double* s, uint64_t seed, int64_t k0, int m0, double* out,
                            hipStream_t st);

// ---- ff_scan_inst.hip: one slice of the K1 kernel family per translation unit -------------
#define RJP_SCAN_SLICE_ARGS                                                                  \
  const rjp_fields *fl, const BurstsDev &b, bool bursts, const double *t, const UnifDev &un, \
      int et, int nsplit, int ylen, double *ws, bool want_em, hipStream_t st
hipError_t scan_f64_tau(int vec, RJP_SCAN_SLICE_ARGS);
hipError_t scan_f64_cmp_scalar(int vec, RJP_SCAN_SLICE_ARGS);
hipError_t scan_f64_cmp_plaw(int vec, RJP_SCAN_SLICE_ARGS);
hipError_t scan_f64_wide(int vec, const rjp_fields* fl, const BurstsDev& b, bool bursts, int mode,
                         const double* t, const UnifDev& un, int et, int nsplit, int ylen,
                         double* ws, bool want_em, hipStream_t st);
hipError_t scan_f32(int vec, int lay, const rjp_fields* fl, const BurstsDev& b, bool bursts,
                    int mode, const double* t, const UnifDev& un, int et, int nsplit, int ylen,
                    double* ws, bool want_em, hipStream_t st);

// ---- fields.hip ---------------------------------------------------------------------------
// K4's two 2F1 series (hyp_series): no series may need more than kHypMaxTerms terms, and a term
// below kHypStop of the sum ends one.  hyp_plan (host) only hands the device a model for which
// both hold, with the same summation in double.
constexpr int kHypMaxTerms = 400;
constexpr double kHypStop = 1e-17;

struct GeomDev {
  int nx, ny, nz, ccw;
  int ix0, nx_total;              // x-slab: rows [ix0, ix0+nx) of an nx_total-wide grid
  double cs;
  double ca, sa, cb, sb;          // derotation: alpha = inc - 90 (about x), beta = pa (about y)
  double ca2, sa2, cb2, sb2;      // velocity rotation: alpha = 90 - inc, beta = -pa
  double w_0, r_0, mr0, eps, R_1, R_2;
  double gm;                      // G * M_star * MSOL [SI]
  double v_lsr;
  double n_0, x_0, T_0, v_0;
  double q_n, q_x, q_T, q_v, qd_n, qd_x, qd_T, qd_v;
  double rb_frac;
  double ts_const, ts_pow, ts_base;   // ts = ts_const * (rad^ts_pow - ts_base)  [q^d_v == 0]
  int ts_mode;                        // 0 = skip, 1 = closed form (q^d_v = 0), 2 = with 2F1
  // q^d_v != 0 (maths/geometry.py:150-178): a = q^d_v, b = (1 - q_v + eps q^d_v)/eps,
  // hypergeometric connection coefficients K1 = b/(b-a), K2 = Gamma(b+1)Gamma(a-b)/Gamma(a);
  // hy_switch: the Pfaff series serves A <= hy_switch, the connection formula A > hy_switch
  // (chosen per model by hyp_plan, fields.hip; +inf = the Pfaff series alone)
  double hy_a, hy_b, hy_k1, hy_k2, hy_axis, hy_switch;
  double r1_m, r2_m, w0_m, mr0_m, r0_m;
};

// K4's host half: rjp_geometry -> GeomDev, with the plan of the 2F1 when the launch times are
// asked for (`want_ts`).  RJP_OK, or the status and message rjp_build_fields reports.
int geometry_to_dev(const rjp_geometry* gm, bool want_ts, GeomDev& g, std::string& err);
hipError_t pack_field_launch(const double* src, const double* den, const uint8_t* red, void* dst,
                             int64_t n, int dtype, hipStream_t st);
hipError_t compact_fields_launch(const rjp_fields* fl, void* d_em0, int64_t* d_n_bad,
                                 hipStream_t st);
hipError_t tau_field_launch(const rjp_fields* fl, int gff_mode, void* d_a0, hipStream_t st);
hipError_t unmask_ts_launch(const rjp_fields* fl, int jet, void* d_out, hipStream_t st);
hipError_t synth_launch(uint64_t seed, int temp_mode, int nz, int64_t cell0, int64_t n, int dtype,
                        void* nd, void* xi, void* temp, void* pf, void* ts, void* vy, void* em0,
                        void* a0, int a0_mode, hipStream_t st);
hipError_t build_fields_launch(const GeomDev& g, int dtype, void* nd, void* xi, void* temp,
                               void* pf, void* ts, void* vy, double* ff_raw, double* areas_raw,
                               double* vx_raw, double* vz_raw, void* em0, void* a0, int a0_mode,
                               hipStream_t st);

// ---- rrl_scan.hip -------------------------------------------------------------------------
hipError_t rrl_scan_launch(const rjp_fields* fl, const rjp_bursts* hb, const double* d_ext,
                           double time_s, const rjp_line* line, const double* h_nu,
                           const double* d_nu, int nchan, double* tau, hipStream_t st);
hipError_t rrl_cells_launch(const rjp_fields* fl, const rjp_bursts* hb, const double* d_ext,
                            double time_s, const rjp_line* line, const double* h_nu,
                            const double* d_nu, int nchan, double* out, hipStream_t st);
hipError_t rrl_maps_launch(const double* tau_rrl, const double* tau_ff, const double* tavg,
                           const double* flux_ff, int64_t npix, const double* d_cflux,
                           const double* d_hnu_k, int nchan, double* flux, double* ftot,
                           double* part, hipStream_t st);

// rrl_formal.hip: the line intensity by the formal solution along the line of sight (K6), out[F * P]
hipError_t rrl_formal_launch(const rjp_fields* fl, const rjp_bursts* hb, const double* d_ext,
                             double time_s, int mode, const rjp_line* line, const double* h_nu,
                             const double* d_nu, const double* d_ctau, const double* d_csrc,
                             const double* d_hnu_k, int nchan, const double* d_add, double* out,
                             hipStream_t st);

}  // namespace rjp
