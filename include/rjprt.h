/* rjprt.h -- C-ABI of librjprt.so, the MI355X (gfx950) line-of-sight radiative-transfer core
 * behind RaJePy's JetModel.
 *
 * The reference (SimonP2207/RaJePy) has no FFI: its hot path is reached only through Python
 * methods of `JetModel` (classes.py:1101-1541).  Each entry point below names the reference
 * method(s) whose NumPy body it replaces; `rajepy_amd/_lib.py` is the ctypes binding and
 * INTEGRATION.md shows the stub a RaJePy maintainer would add.
 *
 * Conventions
 *  - every function returns an int status: 0 = RJP_OK, negative = error; the message for the
 *    last error of a context is `rjp_last_error(ctx)`.  No exceptions, no exit().
 *  - all array arguments named `d_*` are CALLER-OWNED DEVICE pointers (e.g.
 *    torch.Tensor.data_ptr()); the library never frees or retains them.  Arguments named
 *    `h_*` are host pointers to small per-channel / per-epoch tables (copied on the stream).
 *  - work is enqueued on the caller's `stream` (a hipStream_t passed as void*; NULL = the
 *    default stream) and is asynchronous; the caller synchronises.
 *  - a context is bound to one device and is not thread-safe: one context per rank.
 *  - grids are C-contiguous (n_x, n_y, n_z), line of sight = axis 1 (classes.py:46,
 *    363-367); maps are (n_x, n_z) row-major, P = n_x*n_z pixels.
 */
#ifndef RJPRT_H
#define RJPRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RJP_VERSION 117          /* 0.1.17 */
#define RJP_RANGE_BLOCKS 2048    /* partial (min, max) pairs rjp_field_range writes */
#define RJP_MAX_EPOCH_TILE 32    /* most epochs evaluated per grid pass: 32 uniformly spaced ones (with or without d_em), 16 when only 16-31 are left, else tiles of 8, 4, 2, 1 */

enum rjp_status {
  RJP_OK = 0,
  RJP_ERR_ARG = -1,        /* bad argument (null pointer, shape, dtype tag ...) */
  RJP_ERR_HIP = -2,        /* a HIP runtime call failed */
  RJP_ERR_NODEVICE = -3,   /* no usable gfx950 device */
  RJP_ERR_WORKSPACE = -4,  /* workspace too small */
  RJP_ERR_DEGENERATE = -5  /* rjp_build_fields: the launch-time integral's 2F1 is a logarithmic
                              case (or too close to one) for the device series; nothing was enqueued --
                              the caller evaluates `ts` itself (scipy hyp2f1, as the reference
                              does, maths/geometry.py:166-171) and uploads it */
};

enum rjp_dtype { RJP_F32 = 4, RJP_F64 = 8 };   /* storage width of the 3-D fields */

enum rjp_gff_mode {
  RJP_GFF_SCALAR = 0,      /* q_T == 0: one Gaunt factor per channel (classes.py:1388-1389) */
  RJP_GFF_POWERLAW = 1     /* 11.95 T^0.15 nu^-0.1 per cell        (classes.py:1393, 1426) */
};

typedef struct rjp_ctx rjp_ctx;

/* Device-resident model state: the five (continuum) / six (RRL) per-cell fields of
 * SURVEY.md 8(d).  Layout produced by rjp_pack_field / rjp_build_fields:
 *   nd   |value| = steady-state number density `_nd` [cm^-3] (classes.py:889-897);
 *        SIGN BIT = 1 where the cell belongs to the red jet (rr < 0, classes.py:866, 895)
 *   xi   ionisation fraction (classes.py:910-936)
 *   temp temperature [K] (classes.py:942-969)
 *   pf   path-length factor fill_factor / areas (classes.py:1118, 1185, 1396-1397)
 *   ts   launch time `_ts` [s] (classes.py:847-853); may be NULL when there are no bursts
 *   vy   line-of-sight velocity vel[1] [km/s] (classes.py:1093); RRL only, else NULL
 * NaN marks "outside the jet" exactly as in the reference. */
typedef struct rjp_fields {
  const void* d_nd;
  const void* d_xi;
  const void* d_temp;
  const void* d_pf;
  const void* d_ts;
  const void* d_vy;
  int32_t nx, ny, nz;
  int32_t dtype;            /* enum rjp_dtype */
  double csize_au;          /* cell size [au] */
  /* Optional per-sightline occupied y-range [d_ylo[p], d_yhi[p]) from rjp_y_bounds() (both
   * NULL = scan every row).  Real jets fill a few per cent of the grid; rows outside the
   * range hold only cells that cannot contribute (NaN density / T <= 0) and are skipped. */
  const int32_t* d_ylo;
  const int32_t* d_yhi;
  /* Optional compact scan layout, written by rjp_compact_fields() in the storage dtype:
   * d_em0[cell] = (|nd| * xi)^2 * pf, the emission-measure density of the steady-state jet
   * [cm^-6] -- the only combination of nd, xi and pf that emission_measure / optical_depth_ff
   * use (classes.py:1116-1118, 1395-1397) -- with the red-jet flag of nd in its SIGN BIT.
   * The free-free scan then streams 3 fields (em0, temp, ts = 24 B/cell in f64) instead of 5
   * (40 B/cell) and, for f64 storage, returns bit-identical maps (f32 storage rounds the
   * product once more, 6e-8).  When non-NULL, rjp_ff_scan and rjp_y_bounds
   * read d_em0 and ignore d_nd / d_xi / d_pf (which may then be NULL for those two calls);
   * the RRL and collapse=False entry points always read the wide fields. */
  const void* d_em0;
  /* Optional tau scan layout (RJP_F64 storage only), written by rjp_tau_field() or by the
   * producers: d_a0[cell] = em0 * T^-1.5 (a0_mode = RJP_GFF_SCALAR) or em0 * T^-1.35
   * (RJP_GFF_POWERLAW) -- every factor of a cell's free-free optical depth that depends on
   * neither frequency nor epoch (classes.py:1395-1397; the temperature grid is static,
   * classes.py:942-969) -- formed exactly as the scan forms it from em0 and temp, red-jet flag
   * in the SIGN BIT.  When non-NULL and a0_mode equals the gff_mode of the call, rjp_ff_scan
   * streams d_a0 and d_ts = 16 B/cell (plus d_em0, 24 B/cell, only when d_em is asked for) and
   * never reads d_temp; maps are bit-identical to the compact and wide layouts'.  T_avg, which
   * depends on neither frequency nor epoch either (classes.py:1471-1472), then comes from
   * rjp_tavg() once per model (a d_tavg passed to rjp_ff_scan is served by that pass). */
  const void* d_a0;
  int32_t a0_mode;          /* enum rjp_gff_mode d_a0 was built for */
  int32_t reserved_;        /* 0 */
  /* Optional: the range of the finite launch times, [ts_lo, ts_hi] in seconds (rjp_field_range;
   * both 0 = not provided).  With it, a tau-layout scan of >= 12 epochs (with EM maps: when
   * d_em0 is attached -- a second pass takes the moments of em0) may take the MOMENT path: sum_y a0 chi(t_e - ts)^2 is a convolution of the sightline's launch-time
   * distribution with chi^2, so ONE pass over the grid accumulates per-sightline Chebyshev
   * moments of a0 over K launch-time bins of order N -- (K, N) one of (80, 8), (53, 12), (39, 16),
   * the cheapest the host's accuracy check accepts -- and any number of epochs, uniformly spaced or
   * not, becomes a small contraction.  The expansion is checked against chi^2 for the call's bursts and
   * epochs (on the device) and the path is used only when every coefficient table is good to 1e-11
   * relative AND a cost model says it is the faster one (long, densely filled sightlines; else
   * the epoch tiles run, as before); sums are reproducible to rounding, not bit
   * for bit (LDS atomics).  The range must contain every finite launch time of d_ts: pass what
   * rjp_field_range returned for it, or zeros.
   * LAUNCH-TIME RANGE GUARD (ABI 109).  The paths below clamp a launch time into their bins /
   * table, so a range that misses some would give silently wrong maps -- the reference has no
   * such failure mode (classes.py:844-845 evaluates every cell).  Therefore: (1) the first
   * rjp_ff_scan / rjp_ff_step that uses a (d_ts, ts_lo, ts_hi) this context has not seen checks
   * it with one pass over d_ts and ONE stream synchronisation (1.3 ms for 1.07e9 cells, once per
   * model) and returns RJP_ERR_ARG with nothing enqueued when a finite launch time lies outside;
   * rjp_lt_count does the same inside its counting pass; (2) every kernel that bins or tabulates
   * by launch time watches the times it reads: a sightline that meets a finite one outside the
   * range gets NaN sums (never a clamped, plausible-looking value) and the context's guard flag is
   * raised -- the next entry point called on the context returns RJP_ERR_ARG once and enqueues
   * nothing; rjp_range_guard() queries and clears the flag after a synchronisation.
   * The same range lets SINGLE-epoch scans of large f64 maps (>= 32768 sightlines, >= 64 rows; the
   * tau layout or the five model fields) take the burst factor chi(t - ts) from a table in LDS
   * instead of evaluating the Gaussians per cell: piecewise polynomials of degree 7 over the
   * times since launch that can occur, built on the device in front of the scan, bound 2e-13 on
   * chi^2 (bursts with a negative amplitude or a table that would not fit 72 KB keep the
   * Gaussians); maps equal to the Gaussian scan's to rounding (rjp_last_scan_path = 3). */
  double ts_lo, ts_hi;
  /* Optional hint for the choice between the epoch tiles and the moment path: the number of
   * cells inside the occupied y-ranges, sum_p max(0, d_yhi[p] - d_ylo[p]) (0 = unknown: all
   * n_x n_y n_z cells are assumed to matter).  The tiles' cost scales with it, the moment
   * path's per-sightline costs (2 K N doubles of moments, <= 10 KiB, written and read back) do not: a sparse jet
   * keeps the tiles.  A negative value skips the cost model (tests: the moment path on grids it
   * would not pay for). */
  int64_t occupied_cells;
  /* Optional launch-time-ordered layout of (a0, ts) for epoch sweeps, built once per model by
   * rjp_lt_count() + rjp_lt_fill() (all three NULL / 0 = absent).  Every group of 64 consecutive
   * sightlines is bucketed by (jet, launch-time bin): d_lt_cells holds (|a0|, ts) pairs,
   * [(d_lt_rowoff[g * 2 lt_K + q] + r) * 64 + lane], the rows of one (group, bin) contiguous and
   * padded to the largest count among the group's sightlines (in chunks of 4 rows).  A wave then
   * walks the bins of its group with every lane in the SAME bin: the Chebyshev moments of a bin
   * live in registers and are contracted with the bin's coefficient rows at its end -- no LDS
   * atomics, no moment maps in HBM, sums in a fixed order (bit-reproducible for one layout).
   * rjp_ff_scan takes it for tau-layout scans of RJP_MOM_MIN.. 32 epochs without EM maps when
   * the coefficient tables pass the accuracy check at some order <= 32.  It belongs to the d_a0,
   * d_ts, ts_lo, ts_hi it was built from: rebuild after any of them changes. */
  const void* d_lt_cells;
  const int32_t* d_lt_rowoff;
  const double* d_lt_aux;
  int32_t lt_K;             /* launch-time bins per jet the layout was built with */
  int32_t reserved2_;       /* 0 */
  /* Optional cache of the launch-time moment maps of a0 (NULL = none): rjp_moment_cache_bytes()
   * bytes of device memory the CALLER keeps with the model.  The moments depend on the fields,
   * on ts_lo / ts_hi, on the (bins, order) shape and on WHICH jets have bursts -- not on the
   * epochs, not on the burst parameters -- so every further sweep of the model (other epochs,
   * other bursts, e.g. a fit of burst parameters) needs only the contraction.  A sweep that
   * takes the LDS moment path without EM maps writes its moment maps here instead of into the
   * workspace; when mom_cache_K / mom_cache_N equal the shape that sweep selects, the pass over
   * the grid is SKIPPED (rjp_last_scan_path returns 4).  The caller sets mom_cache_K / _N to the
   * shape rjp_last_scan_path reported after a call that filled the buffer, and back to 0
   * whenever d_a0, d_ts (their contents, not only the pointers), the range or the set of jets
   * with bursts changes.  The cache is VOID after a range-guard report (rjp_range_guard() == 1,
   * or an entry point that returns RJP_ERR_ARG with the guard's message): a pass that filled it
   * since the last clean report may have written the NaN sums of the sightlines concerned, so
   * the caller sets mom_cache_K / _N back to 0 then as well. */
  double* d_mom_cache;
  int32_t mom_cache_K, mom_cache_N;
  /* Optional launch-time-bucketed layout of (a0, ts) for SINGLE-epoch scans, built once per model
   * by rjp_srt_count() + rjp_srt_fill() (all NULL / 0 = absent).  Every group of 64 consecutive
   * sightlines g holds each lane's OWN cells sorted by key q = jet * srt_K + bin (srt_K bins per
   * jet over [ts_lo, ts_hi]):
   *   d_srt_cells[(d_srt_rowbase[g] + r) * 64 + lane] = (|a0|, ts)     16 bytes
   * where the cells of key q of sightline p are rows [d_srt_start[q * P + p], d_srt_start[(q + 1)
   * * P + p]) (d_srt_start[2 srt_K * P + p] = the sightline's length); lanes are padded at the END
   * only, up to the group's longest lane (d_srt_rowbase[g + 1] - d_srt_rowbase[g] rows).
   * d_srt_cum[q * P + p] = the sum of |a0| over the sightline's cells of the keys below q (2 srt_K
   * + 1 entries per sightline, like d_srt_start); d_srt_aux = 3 P doubles as d_lt_aux (NaN
   * launch times per jet, infinite weights); h_srt_hist = HOST array of 2 srt_K cell counts per
   * key over the whole map.  Cells with a0 == 0 or NaN, infinite a0 or a NaN launch time are not
   * in the layout (the aux sums stand for them, so the maps keep nansum's semantics).
   * Outside the bursts' support chi(t - ts) == 1 (to 1e-17), so a single-epoch scan on the table
   * path reads only the rows of the bins in the support of each jet at that epoch and adds the
   * |a0| sums of the other bins: the bytes read depend on the epoch.  rjp_ff_scan / rjp_ff_step
   * take it when the table path applies (single epoch, no d_em, no d_tavg) and at most 90 % of
   * the cells (h_srt_hist) fall into those bins, else they scan a0 / ts in grid order;
   * rjp_last_scan_layout() says which.  It belongs to the d_a0, d_ts, ts_lo, ts_hi it was built
   * from: rebuild after any of them changes.
   * Optional with it (NULL / 0 = absent: every bin of the support is read): the layout's Chebyshev
   * moments, built by rjp_srt_moments() from the layout alone,
   *   d_srt_mom[(q * (srt_N - 1) + n - 1) * P + p] = sum |a0| T_n(x),  n = 1 .. srt_N - 1,
   * over the cells of key q of sightline p, x = 2 (w - bin) - 1 in [-1, 1] with w = (ts - ts_lo)
   * srt_K / (ts_hi - ts_lo) (the layout's bins, clamping included; M_0 is the d_srt_cum step).
   * Per call, a small kernel interpolates chi^2 on every bin of the support at srt_N Chebyshev
   * nodes and accepts the bin when the interpolant matches, at 4 srt_N points across it, both the
   * exact chi^2 and the table's to 2e-14 relative; the scan then contracts an accepted bin from
   * its moments instead of reading its cells (16 bytes each) wherever (srt_N - 1) x 8 bytes per
   * sightline are fewer bytes for the group; of those planes it reads the first m - 1 only, m the
   * number of coefficients that matter on the bin (the dropped tail is below 5e-15 of its
   * smallest chi^2 and the truncated interpolant passes the same checks).  The planes are read as
   * 16-byte pairs of sightlines: d_srt_mom must be 16-byte aligned and P even, else the scan
   * fails.  rjp_last_srt_bins() counts both kinds.
   * The moments belong to the layout: rebuild them with it.
   * Optional with the moments (both NULL = absent): the layout's PACKED state, built by
   * rjp_srt_pack() from the finished layout -- the same rows in the same (row, lane) arrangement
   * at 10 bytes per cell.  With r0 = ((d_srt_rowbase[g] + 7) & ~7) + 8 g the first packed row of
   * group g (every group's rows are rounded up to 8; rjp_srt_packed_rows() rows in all) and r a row
   * of the group:
   *   d_srt_pts[((r0 + r) / 2) * 64 + lane] = (ts[r], ts[r + 1])         16 bytes, r even
   *   d_srt_pw [((r0 + r) / 8) * 64 + lane] = weights of rows r .. r + 7  16 bytes, 16 bits each
   * A weight is |a0| >= 0 rounded to nearest even to the upper 16 bits below the sign of a float
   * (8 exponent bits, 8 mantissa bits: relative error <= 2^-9); rows past a lane's length and the
   * padding hold weight 0.  A bin whose interpolant matches the exact chi^2 but not the table's is
   * then tested with the table's own error added, E_i(xi) = table^2 - chi^2 fitted per table piece
   * by a polynomial of degree 8 (f32): where that matches the table to the same 2e-14 at the same
   * points, the scan contracts the bin from its moments and adds sum |a0| E(ts) over the bin's
   * cells from the packed state -- that term is <= ~2.2e-13 of the bin's sum, so 8 bits of the
   * weight do (4.3e-16), while the launch time, which picks the table piece, stays exact -- wherever
   * 6 bytes x the longest lane run exceed (srt_N - 1) x 8 bytes.  Such a bin counts as read in
   * rjp_last_srt_bins(); rjp_last_srt_resid() counts them.  Not taken when the chi table and the
   * error table (128 bytes per piece and jet) exceed 80 KiB of LDS.  Both pointers 16-byte aligned.
   * The packed state belongs to the layout's cells: rebuild it whenever they change.
   * Optional with the packed state (NULL = absent): its launch-time CODES, built by
   * rjp_srt_codes() from the finished layout, 4 bytes per cell in the packed state's rows:
   *   d_srt_pc [((r0 + r) / 4) * 64 + lane] = codes of rows r .. r + 3    16 bytes, r % 4 == 0
   *   code = min(floor((ts - ts_lo) * 2^32 / (ts_hi - ts_lo)), 2^32 - 1) as a uint32, in f64 as
   * written: ts_lo gives 0, the code is monotone in ts and saturates; rows past a lane's length
   * and the padding hold 0.  With q = (ts_hi - ts_lo) 2^-32 a code c < 2^32 - 1 stands for the
   * launch times ts_lo + (c - 2^-18) q <= ts < ts_lo + (c + 1 + 2^-18) q (the 2^-18 covers the
   * f64 roundings of the encoding), 2^32 - 1 for everything from ts_lo + (2^32 - 1 - 2^-18) q on.
   * With the codes the residual stream reads 6 bytes per cell: the table piece and xi of a cell
   * come from its code, except where the code's interval, widened to a margin of 2 q per side plus
   * the roundings of both evaluations, reaches a piece boundary, or the code is saturated -- such a
   * cell (about 4 q x pieces per unit of launch time of them) is re-read from its 16-byte entry of
   * d_srt_cells and evaluated as without the codes, so every cell gets the piece its exact launch
   * time picks; inside a piece xi moves by <= ~1.2e-7 and the cell's term by < 2e-18 of itself.
   * rjp_last_srt_fallbacks() counts the re-read cells.  d_srt_pts is then not read at all: it is
   * the stream of a scan WITHOUT the codes.  16-byte aligned (and d_srt_cells with it), else the
   * scan reads d_srt_pts.  The codes belong to the layout's cells and to ts_lo / ts_hi. */
  const void* d_srt_cells;
  const int32_t* d_srt_start;
  const double* d_srt_cum;
  const int64_t* d_srt_rowbase;
  const double* d_srt_aux;
  const int64_t* h_srt_hist;
  const double* d_srt_mom;
  int32_t srt_K;            /* launch-time bins per jet, 1..32 */
  int32_t srt_N;            /* order of d_srt_mom: 16, 20 or 24 (0 = no moments) */
  const void* d_srt_pts;    /* packed launch times, pairs of rows (rjp_srt_pack) */
  const void* d_srt_pw;     /* packed 16-bit weights, eight rows per 16 bytes */
  const void* d_srt_pc;     /* launch-time codes, four rows per 16 bytes (rjp_srt_codes) */
} rjp_fields;

/* Ejection bursts (classes.py:399-463): mdot(t)/mdot_ss = 1 + sum_b amp_rel_b *
 * exp(-(t - t0_b)^2 * inv2s2_b); index 0 = red jet, 1 = blue jet.  ANY number of bursts per
 * jet, as in the reference (classes.py:245-264 registers every row of params["ejection"]):
 * the arrays are HOST pointers to n[j] doubles each (may be NULL when n[j] == 0), read
 * during the call.  The first eight bursts of a jet travel to the kernels as scalar
 * arguments, the rest in a small device table the library stages on the stream. */
typedef struct rjp_bursts {
  int32_t n[2];
  const double* t0[2];        /* [s] */
  const double* amp_rel[2];   /* (peak_jml - ss_jml) / ss_jml */
  const double* inv2s2[2];    /* 1 / (2 sigma^2) [s^-2] */
} rjp_bursts;

/* One radio recombination line, host-side scalars of maths/rrls.py (LTE path). */
typedef struct rjp_line {
  double nu_rest;      /* rrl_nu_0 [Hz] (rrls.py:14-29) */
  double kG;           /* deltanu_g / (nu0 sqrt(T)) = sqrt(4 ln2 2k/(m c^2)) (rrls.py:116-118) */
  double kL;           /* deltanu_l / n_e = 8.2 (n/100)^4.5 (1 + 2.25 dn/n) (rrls.py:101) */
  double kappa0;       /* 1.0991132675738456e-17 n^2 f_n1n2 * n_i/n_e (rrls.py:383-389, 73-83) */
  double en_over_k;    /* Z^2 E_n / k_cgs [K] (rrls.py:386) */
  double h_over_k;     /* h_cgs / k_cgs [K/Hz] (rrls.py:387) */
} rjp_line;

int rjp_version(void);
int rjp_device_count(void);
int rjp_ctx_create(int device, rjp_ctx** out);
int rjp_ctx_destroy(rjp_ctx* ctx);
const char* rjp_last_error(const rjp_ctx* ctx);   /* ctx may be NULL: last create error */

/* ---- field upload layout -------------------------------------------------------------- */

/* d_dst[i] = (dtype)d_src[i]; with d_red != NULL additionally sets the sign bit where
 * d_red[i] != 0 (and clears it elsewhere) -> the packed `nd` field; with d_den != NULL
 * stores d_src[i]/d_den[i] -> the `pf` field from fill_factor and areas. */
int rjp_pack_field(rjp_ctx* ctx, const double* d_src, const double* d_den,
                   const uint8_t* d_red, void* d_dst, int64_t n, int dtype, void* stream);

/* Builds the compact scan field (see rjp_fields.d_em0) from the wide fields nd, xi, pf in one
 * pass over all n_x*n_y*n_z cells, in the fields' storage dtype.  *d_n_bad (a device int64,
 * zeroed by the call) receives the number of cells the field cannot represent: a NEGATIVE
 * path factor (its sign would collide with the jet flag; fill_factor / areas never produce
 * one, classes.py:657-669, 763-764) or, for RJP_F32, a product outside the float range.
 * When it is non-zero the field is unusable and the caller keeps scanning the wide layout. */
int rjp_compact_fields(rjp_ctx* ctx, const rjp_fields* fields, void* d_em0,
                       int64_t* d_n_bad, void* stream);

/* Builds the tau scan field (see rjp_fields.d_a0) for `gff_mode` from fields->d_em0 and
 * fields->d_temp in one pass over all cells.  RJP_F64 storage with the compact field attached
 * (a model that has to stay on the wide layout -- negative path factors -- has no tau layout). */
int rjp_tau_field(rjp_ctx* ctx, const rjp_fields* fields, int32_t gff_mode, void* d_a0,
                  void* stream);

/* Launch times for the free-free scan of a model that has bursts in ONE jet only.  The
 * reference's burst Gaussians carry a NaN launch time into the cell's density, which nansum
 * then drops -- but a jet without any registered burst has the constant steady-state mass-loss
 * rate whatever the launch time (classes.py:232-233, 442-448, 866-875): its cells keep chi = 1.
 * rjp_ff_scan masks EVERY cell with a NaN launch time once bursts are present (a per-cell jet
 * test there cost the single-epoch scan 2.7 %), so such a model scans the copy written here:
 * d_ts_out[i] = fields->ts_lo (0 when no range is given: any finite value gives chi = 1 there;
 * this one lies inside the declared range, which the range guard holds the copy to as well) where
 * d_ts[i] is NaN and the cell belongs to `jet` (0 = red, 1 = blue: the one WITHOUT bursts; the flag
 * is read from the sign bit of d_a0, d_em0 or d_nd), d_ts[i] elsewhere.
 * (rjp_rrl_scan and the collapse=False entry points apply the rule themselves.) */
int rjp_unmask_launch_times(rjp_ctx* ctx, const rjp_fields* fields, int32_t jet, void* d_ts_out,
                            void* stream);

/* Per-block (min, max) of the finite entries of a field of n elements (NaN ignored):
 * d_partials[2 b], d_partials[2 b + 1], b < RJP_RANGE_BLOCKS (+inf / -inf for a block without a
 * finite entry); the caller finishes the reduction on the host.  Used once per model for
 * rjp_fields.ts_lo / ts_hi. */
int rjp_field_range(rjp_ctx* ctx, const void* d_field, int64_t n, int dtype, double* d_partials,
                    void* stream);

/* T_avg map of the model: d_tavg[p] = nanmean_y(T where T > 0) [K], NaN on empty sightlines
 * (classes.py:1471-1472, 1484-1485, 1254-1256).  One pass over fields->d_temp (the only field
 * read; d_ylo / d_yhi are honoured), bit-identical to the map a single-epoch rjp_ff_scan
 * derives.  d_work: at least rjp_ff_scan_workspace(nx, ny, nz, 1) bytes. */
int rjp_tavg(rjp_ctx* ctx, const rjp_fields* fields, double* d_tavg, void* d_work,
             size_t work_bytes, void* stream);

/* Per-sightline occupied y-range of a packed field set: d_ylo[p] = first row, d_yhi[p] = one
 * past the last row whose cell can contribute to any product of the path, i.e. T > 0 (counts
 * in the nanmean of intensity_ff, classes.py:1471) or n, x and ff/areas all non-NaN (emission
 * measure, classes.py:1116-1118); empty sightlines get [ny, 0).  One pass over 2 (compact layout) or 4 fields,
 * amortised over every later scan of the same model. */
int rjp_y_bounds(rjp_ctx* ctx, const rjp_fields* fields, int32_t* d_ylo, int32_t* d_yhi,
                 void* stream);

/* sum_p max(0, d_yhi[p] - d_ylo[p]) -> *h_count: the cells inside the occupied y-ranges, i.e.
 * rjp_fields.occupied_cells (one small launch, an 8-byte copy back; synchronises the stream). */
int rjp_occupied_cells(rjp_ctx* ctx, const int32_t* d_ylo, const int32_t* d_yhi, int64_t n_pix,
                       int64_t* h_count, void* stream);

/* ---- K1: free-free / emission-measure scan -------------------------------------------
 * Replaces the y-reductions of JetModel.emission_measure (classes.py:1116-1120),
 * .optical_depth_ff (1375-1432) and the nanmean of .intensity_ff (1471-1472, 1484-1485),
 * with number_density = _nd * chi_xyz (classes.py:861-875) evaluated in registers for
 * each of E epochs.  One pass over the grid per tile of up to RJP_MAX_EPOCH_TILE epochs.
 *   d_sumA [E*P]  sum_y T^-1.5 (n x)^2 pf          (RJP_GFF_SCALAR)
 *                 sum_y T^-1.35 (n x)^2 pf         (RJP_GFF_POWERLAW)   [cm^-6 K^-1.5|-1.35]
 *   d_em   [E*P]  emission measure [pc cm^-6]      (may be NULL)
 *   d_tavg [P]    nanmean_y(T where T > 0) [K], NaN on empty sightlines (may be NULL; on the
 *                 tau layout it costs a separate pass over d_temp: ask once, see rjp_tavg)
 * h_epochs_s: model times [s] (JetModel.time), E >= 1.
 * d_work: scratch of at least rjp_ff_scan_workspace() bytes.  (A single-epoch scan that takes the
 * burst factor from a table may build that table, and the bin coefficients of the bucketed
 * layout, in memory the context owns instead of in d_work -- on a stream of the context's own,
 * ordered against `stream` by events, while `stream` still runs earlier work.  The size asked for
 * here does not depend on that.) */
size_t rjp_ff_scan_workspace(int32_t nx, int32_t ny, int32_t nz, int32_t n_epochs);
int rjp_ff_scan(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                const double* h_epochs_s, int32_t n_epochs, int32_t gff_mode,
                double* d_sumA, double* d_em, double* d_tavg,
                void* d_work, size_t work_bytes, void* stream);

/* Launch-time range guard (see rjp_fields.ts_lo): 1 = a kernel of this context has met a finite
 * launch time outside fields.ts_lo / ts_hi since the last query (the sums of those sightlines are
 * NaN); the flag is cleared.  0 = none.  Meaningful after the caller has synchronised the stream
 * the scans ran on. */
int rjp_range_guard(rjp_ctx* ctx);

/* Which path the last rjp_ff_scan of this context took: 0 = epoch tiles, 1 = launch-time moments
 * in LDS + contraction, 2 = launch-time moments on the launch-time-ordered layout, 3 = the
 * single-epoch tau-layout scan with the burst factor from a table in LDS, 4 = contraction of the
 * caller's cached moment maps (rjp_fields.d_mom_cache: no pass over the grid) (and, if
 * non-NULL: in *worst_rel_err the worst relative error of the moment expansion measured for
 * that call, in moment_shape[0..1] the (bins, order) shape it chose; zeros for the tiles).
 * For tests and the bench line. */
int rjp_last_scan_path(const rjp_ctx* ctx, double* worst_rel_err, int32_t* moment_shape);

/* Which epoch tiles the last rjp_ff_scan / rjp_ff_step of this context launched: *n_tiles tiles,
 * and in tiles[5 * k .. 5 * k + 4] for tile k: its first epoch e0, its epochs et, whether it ran
 * the uniform-spacing recurrence (1) or evaluated every epoch directly (0), its y-ranges nsplit
 * and the sightlines per lane it was dispatched with (1 for et >= 16).  Zero tiles after a scan
 * on any other path (moments, cached moments, bucketed layout, table) and before the first scan.
 * `tiles` holds room for `cap` tiles; with more tiles than that only *n_tiles is written and
 * RJP_ERR_ARG returned.  Host-only: it synchronises and enqueues nothing.  For tests. */
int rjp_last_scan_tiles(const rjp_ctx* ctx, int32_t* n_tiles, int32_t* tiles, int32_t cap);

/* Which layout of (a0, ts) the last rjp_ff_scan / rjp_ff_step of this context read: 0 = the grid
 * order (every cell of the occupied y-ranges), 1 = the launch-time-bucketed layout of
 * rjp_fields.d_srt_cells (only the bins inside the bursts' support; rjp_last_scan_path then
 * reports 3: chi still comes from the table).  For tests and the bench line. */
int rjp_last_scan_layout(const rjp_ctx* ctx);

/* (jet, bin) decisions of the last rjp_ff_scan / rjp_ff_step of this context on the bucketed
 * layout with moments attached, summed over the groups of 64 sightlines that hold the jet: in
 * *contracted the bins taken from rjp_fields.d_srt_mom, in *read the bins of the support read cell
 * by cell (both 0 after a scan without moments).  SYNCHRONISES the device.  For tests. */
int rjp_last_srt_bins(rjp_ctx* ctx, int64_t* contracted, int64_t* read);

/* Host wall time [ms] the last table build of this context took (the coefficient tables of the
 * moment paths are built and checked on the device when the bursts or epochs of a sweep change:
 * one small launch and ONE stream synchronisation inside that rjp_ff_scan; a repeated request
 * reuses them).  0 before the first build. */
double rjp_last_table_build_ms(const rjp_ctx* ctx);

/* Bytes of rjp_fields.d_mom_cache for an n_x x n_z map (1280 doubles per sightline). */
size_t rjp_moment_cache_bytes(int32_t nx, int32_t nz);

/* ---- launch-time-ordered layout (rjp_fields.d_lt_*) -------------------------------------
 * Two calls, because the size of the padded layout is known only after counting:
 *   rjp_lt_rowoff_entries(nx, nz, K)  entries (int32) of d_rowoff: ceil(nx nz / 64) * 2 K + 1
 *   rjp_lt_count   counts the cells of every (group, jet, bin), pads each to the group's largest
 *                  count, writes the exclusive prefix d_rowoff and returns the total number of
 *                  rows in *h_total_rows (synchronises the stream);
 *   rjp_lt_fill    writes d_cells (total_rows * 64 * 16 bytes) and d_aux (3 * nx * nz doubles:
 *                  per sightline the sums of |a0| over red / blue cells with a NaN launch time --
 *                  added when that jet has no burst, classes.py:232-233 -- and an "infinite
 *                  term" flag).
 * Needs RJP_F64 fields with d_a0, d_ts and ts_lo / ts_hi; 1 <= K <= 80, n_y < 65536.  Cells with
 * a0 == 0 or NaN are dropped (nansum).  Cost: two passes over a0 and ts plus 16-byte scattered
 * writes (~50 ms for 1.07e9 cells): worth it for a model that is swept many times. */
size_t rjp_lt_rowoff_entries(int32_t nx, int32_t nz, int32_t K);
int rjp_lt_count(rjp_ctx* ctx, const rjp_fields* fields, int32_t K, int32_t* d_rowoff,
                 int64_t* h_total_rows, void* stream);
int rjp_lt_fill(rjp_ctx* ctx, const rjp_fields* fields, int32_t K, const int32_t* d_rowoff,
                void* d_cells, double* d_aux, void* stream);

/* ---- launch-time-bucketed layout (rjp_fields.d_srt_*) ------------------------------------
 * Two calls, because the size of the layout is known only after counting:
 *   rjp_srt_index_entries(nx, nz, K)  entries of d_start (int32) and of d_cum (double) each:
 *                  (2 K + 1) nx nz; d_rowbase holds ceil(nx nz / 64) + 1 int64
 *   rjp_srt_count  counts every sightline's cells per (jet, bin), writes d_start (the lane-local
 *                  start rows) and d_rowbase (the groups' first rows), fills h_hist[2 K] (host)
 *                  and returns the total number of rows in *h_total_rows (synchronises the
 *                  stream; checks the launch-time range as rjp_lt_count does);
 *   rjp_srt_fill   writes d_cells (total_rows * 64 * 16 bytes), d_cum and d_aux (3 nx nz doubles).
 * Needs RJP_F64 fields with d_a0, d_ts and ts_lo / ts_hi; 1 <= K <= 32.  Cost: two passes over a0
 * and ts plus 16-byte scattered writes, once per model; memory ~1.03 x the bytes of a0 + ts. */
size_t rjp_srt_index_entries(int32_t nx, int32_t nz, int32_t K);
int rjp_srt_count(rjp_ctx* ctx, const rjp_fields* fields, int32_t K, int32_t* d_start,
                  int64_t* d_rowbase, int64_t* h_hist, int64_t* h_total_rows, void* stream);
int rjp_srt_fill(rjp_ctx* ctx, const rjp_fields* fields, int32_t K, const int32_t* d_start,
                 const int64_t* d_rowbase, void* d_cells, double* d_cum, double* d_aux,
                 void* stream);
/* The layout's Chebyshev moments (rjp_fields.d_srt_mom): rjp_srt_moment_entries(nx, nz, K, N) =
 * 2 K (N - 1) nx nz doubles (0 for an N other than 16, 20, 24 or a bad K), written by
 * rjp_srt_moments from a layout rjp_srt_fill has built with the same fields and K.  One pass over
 * the layout's rows (~1.03 x the bytes of a0 + ts), f64 sums in a fixed order. */
size_t rjp_srt_moment_entries(int32_t nx, int32_t nz, int32_t K, int32_t N);
int rjp_srt_moments(rjp_ctx* ctx, const rjp_fields* fields, int32_t K, int32_t N,
                    const int32_t* d_start, const int64_t* d_rowbase, const void* d_cells,
                    double* d_mom, void* stream);
/* The layout's packed state (rjp_fields.d_srt_pts / d_srt_pw): rjp_srt_packed_rows(nx, nz,
 * total_rows) rows R (a multiple of 8; 0 for a bad shape), d_pts = R * 64 * 8 bytes, d_pw = R * 64 *
 * 2 bytes, both 16-byte aligned, written by rjp_srt_pack from a layout rjp_srt_fill has built with
 * the same fields and K: one coalesced pass over the layout's rows.  Returns 1 when every weight
 * fits the 16-bit format, 2 when some finite non-zero weight lies below 2^-126 or would round to
 * 2^128 and beyond -- it would be flushed or saturated and its residual lost: do NOT attach the
 * state then -- or a negative rjp_status: a bad K or fields, a NULL or misaligned pointer.
 * Synchronises the stream. */
size_t rjp_srt_packed_rows(int32_t nx, int32_t nz, int64_t total_rows);
int64_t rjp_srt_pack(rjp_ctx* ctx, const rjp_fields* fields, int32_t K, const int32_t* d_start,
                     const int64_t* d_rowbase, const void* d_cells, void* d_pts, void* d_pw,
                     void* stream);
/* The launch-time codes of the packed state (rjp_fields.d_srt_pc): d_pc = R * 64 * 4 bytes for
 * the R rows of rjp_srt_packed_rows(), 16-byte aligned, written from a layout rjp_srt_fill has
 * built with the same fields (ts_lo / ts_hi included) and K: one coalesced pass over the layout's
 * rows.  Returns 1, or a negative rjp_status: a bad K or fields, no launch-time range in the
 * fields, a NULL pointer, d_cells or d_pc not 16-byte aligned.  Does not synchronise. */
int64_t rjp_srt_codes(rjp_ctx* ctx, const rjp_fields* fields, int32_t K, const int32_t* d_start,
                      const int64_t* d_rowbase, const void* d_cells, void* d_pc, void* stream);
/* The table-residual (group, jet, bin) triples of the last scan (a subset of rjp_last_srt_bins'
 * *read), or a negative rjp_status.  SYNCHRONISES the device.  For tests. */
int64_t rjp_last_srt_resid(rjp_ctx* ctx);
/* The cells of the last scan's residual stream that fell back from their launch-time code to
 * their entry of d_srt_cells (0 for a scan without the codes), or a negative rjp_status.
 * SYNCHRONISES the device.  For tests. */
int64_t rjp_last_srt_fallbacks(rjp_ctx* ctx);

/* ---- K2: per-channel map stage --------------------------------------------------------
 * Replaces the map-level arithmetic of optical_depth_ff / intensity_ff / flux_ff
 * (classes.py:1395-1397, 1473-1475, 1519-1521):
 *   tau[e,f,p]  = h_ctau[f] * sumA[e,p]
 *   flux[e,f,p] = h_cflux[f] * tavg[p] * (1 - exp(-tau))      [Jy/pixel]
 *   ftot[e,f]   = nansum_p flux[e,f,p]
 * h_ctau[f]  = 0.018 nu^-2 gff(nu,T_0) csize au 100      (scalar mode)
 *            = 0.018 nu^-2 11.95 nu^-0.1 csize au 100    (power-law mode)
 * h_cflux[f] = 2 nu^2 k / c^2 * arctan(csize au / (dist pc))^2 / 1e-26
 * NaN rule: a NaN in tavg[p] (an empty sightline) or in sumA[e,p] (a sightline the launch-time
 * range guard poisoned, or a NaN of the caller's own sums) gives flux = NaN, and the pixel adds
 * nothing to ftot; tau is h_ctau * sumA either way (NaN for a NaN sum).  A NaN sum is never turned
 * into the finite flux h_cflux * tavg of an optically thick sightline.  sumA = +inf gives
 * tau = +inf and flux = h_cflux * tavg; sumA = 0 gives +0.0 in both.  h_ctau must be finite.
 * Any of d_tau / d_flux / d_ftot may be NULL.  d_work >= rjp_ff_maps_workspace(). */
size_t rjp_ff_maps_workspace(int64_t n_pix, int32_t n_epochs, int32_t n_chan);
int rjp_ff_maps(rjp_ctx* ctx, const double* d_sumA, const double* d_tavg, int64_t n_pix,
                int32_t n_epochs, const double* h_ctau, const double* h_cflux, int32_t n_chan,
                double* d_tau, double* d_flux, double* d_ftot,
                void* d_work, size_t work_bytes, void* stream);

/* What the last rjp_ff_maps / rjp_ff_step of this context launched for its map stage:
 *   out[0]  the kernel: 0 = the small-map kernel (a lane per VEC pixels, a wave reduction per
 *           channel), 1 = the cube kernel with per-lane flux accumulators, 2 = totals only (no
 *           cube was asked for); -1 before the first map stage of the context
 *   out[1]  VEC, the pixels per lane and load: 2 when n_pix is even and d_sumA, d_tavg, d_tau and
 *           d_flux are all 16-byte aligned, else 1
 *   out[2]  KP, the pixel groups a lane walks (1 or 4; 4 for totals only)
 *   out[3]  the workgroups along the pixel axis (gridDim.x)
 *   out[4]  the partial sums per (epoch, channel) handed to the fixed-order reduction; 0 when no
 *           d_ftot was asked for
 *   out[5]  the channels per workgroup (gridDim.z slices the channel axis)
 * RJP_ERR_ARG for a NULL argument.  Host-only: it synchronises and enqueues nothing.  For tests. */
int rjp_last_maps_launch(const rjp_ctx* ctx, int32_t out[6]);

/* ---- K1 + K2 from ONE call ----------------------------------------------------------------
 * rjp_ff_scan followed by rjp_ff_maps on the same stream, for callers whose step is shorter than
 * two round trips through their FFI (an x-slab of a sharded grid: 0.3 ms per step at 64 x 4096 x
 * 512; a 256 x 1024 x 256 model: 0.2 ms): what JetModel.optical_depth_ff / flux_ff ask per epoch
 * (classes.py:1375-1432, 1466-1541).  Arguments as for the two calls; d_tavg is the model's T_avg
 * map (rjp_tavg: INPUT here, the scan derives none); d_em, d_tau, d_flux, d_ftot may be NULL.
 * Every argument of both stages is validated before anything is enqueued.  d_work >=
 * rjp_ff_scan_workspace(), d_work_maps >= rjp_ff_maps_workspace() (two buffers: the scan of the
 * next step may overlap this step's map stage on another stream). */
int rjp_ff_step(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                const double* h_epochs_s, int32_t n_epochs, int32_t gff_mode,
                const double* d_tavg, const double* h_ctau, const double* h_cflux, int32_t n_chan,
                double* d_sumA, double* d_em, double* d_tau, double* d_flux, double* d_ftot,
                void* d_work, size_t work_bytes, void* d_work_maps, size_t work_maps_bytes,
                void* stream);

/* ---- K3: recombination-line scan ------------------------------------------------------
 * Replaces JetModel.optical_depth_rrl (classes.py:1159-1214): per cell Doppler-shifted rest
 * frequency, thermal + Stark widths, Voigt profile Re w(z) (rrls.py:350-354), LTE kappa_L
 * (rrls.py:383-389), summed along y for every channel.
 *   d_tau_rrl [F*P]
 * One epoch per call (time_s). */
int rjp_rrl_scan(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                 double time_s, const rjp_line* line, const double* h_nu, int32_t n_chan,
                 double* d_tau_rrl, void* stream);

/* collapse=False forms (classes.py:1382-1383, 1176-1177): the 3-D per-cell optical depths,
 * d_tau_cells[f * N + cell], NaN outside the jet as in the reference.  h_ctau as for
 * rjp_ff_maps.  Not used by Pipeline; N*F*8 bytes of output. */
int rjp_ff_cells(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                 double time_s, int32_t gff_mode, const double* h_ctau, int32_t n_chan,
                 double* d_tau_cells, void* stream);
int rjp_rrl_cells(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                  double time_s, const rjp_line* line, const double* h_nu, int32_t n_chan,
                  double* d_tau_cells, void* stream);

/* ---- K5: free-free intensity by the formal solution along the line of sight ----------------
 * The reference's intensity_ff / flux_ff (classes.py:1466-1541) are isothermal:
 * S = c[f] T_avg (1 - e^-tau) with T_avg = nanmean_y(T > 0), exact only where T is constant along
 * the sightline.  This entry point sums the emission of every cell attenuated by the cells in
 * front of it:
 *   d_out[f * P + p] = h_csrc[f] * sum_i T_i (1 - e^-dtau_i) exp(-sum_{j in front of i} dtau_j)
 *   dtau_i = h_ctau[f] |a0_i| chi_i^2
 * with a0 (= (n x)^2 pf T^-1.5 | T^-1.35 for gff_mode) and the burst factor chi(time_s - ts)
 * exactly as the tau scans form them (rjp_ff_scan; the tau, compact and wide layouts are all
 * accepted and give bit-identical f64 maps; d_temp is always read).  h_ctau as for rjp_ff_maps;
 * h_csrc[f] is the Rayleigh-Jeans source factor per kelvin: h_cflux of rjp_ff_maps for Jy/pixel,
 * 2 nu^2 k / c^2 for W m^-2 Hz^-1 sr^-1.
 * OBSERVER SIDE: the iy = 0 end of axis 1 -- the reference's Doppler shift is nu0 (1 - v/c)
 * (physics.py:557-558), so gas with vel[1] > 0 recedes and lies at larger iy.
 * A cell contributes exactly when its term enters the nansum of the tau scans; d_out is NaN
 * exactly where T_avg is (no cell of the sightline has T > 0).  With a constant T the sum
 * telescopes to T (1 - e^-tau): the reference's maps are the isothermal special case.
 * d_ylo / d_yhi are honoured; the launch-time range (ts_lo / ts_hi) is not used.  One epoch per
 * call; every argument is validated before anything is enqueued (RJP_ERR_ARG otherwise). */
int rjp_ff_formal(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                  double time_s, int32_t gff_mode, const double* h_ctau, const double* h_csrc,
                  int32_t n_chan, double* d_out, void* stream);

/* ---- K8: light curves and map sweeps by the formal solution ------------------------------------
 * The reference's light curves loop over `time` and sum a flux_ff map per epoch (Pipeline results,
 * classes.py:2461-2467, with the isothermal maps of classes.py:1466-1541); with rjp_ff_formal that
 * is one call, one [F, P] map and one host-side nansum per epoch.  This entry point walks the
 * fields ONCE for all epochs:
 *   d_out [(e * F + f) * P + p]   rjp_ff_formal's map at time h_epochs_s[e]          (or NULL)
 *   d_ftot[e * F + f]             nansum_p of that map: a pixel whose sightline has no T > 0 is
 *                                 NaN in the map and adds nothing                     (or NULL)
 * The burst factor is evaluated once per (cell, epoch) whatever the number of channels; with d_out
 * NULL no map touches memory.  Every map equals rjp_ff_formal's at that epoch BIT FOR BIT on the
 * same fields (tau, compact or wide layout, RJP_F32 or RJP_F64, any number of bursts or none): the
 * two kernels share the code that forms b and each (sightline, epoch, channel) value is one
 * sequential chain.  The totals are summed in a fixed order without floating-point atomics: a
 * repeated call, or a call with d_out NULL, gives the same bits.  Epochs need not be sorted, evenly
 * spaced or distinct.  h_ctau / h_csrc, the observer side, d_ylo / d_yhi: as rjp_ff_formal; the
 * launch-time range, the layouts ordered by launch time and the moment cache are not used.
 * d_work (rjp_ff_formal_sweep_workspace bytes; 0 from it = a bad argument) is needed with d_ftot
 * only.  Every argument is validated before anything is enqueued: RJP_ERR_ARG for a bad gff_mode,
 * NULL tables, n_epochs < 1, n_chan < 1, a non-finite epoch, both outputs NULL, or bursts without
 * d_ts; RJP_ERR_WORKSPACE for a d_work smaller than rjp_ff_formal_sweep_workspace(). */
size_t rjp_ff_formal_sweep_workspace(int32_t nx, int32_t ny, int32_t nz, int32_t n_epochs,
                                     int32_t n_chan);
int rjp_ff_formal_sweep(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                        const double* h_epochs_s, int32_t n_epochs, int32_t gff_mode,
                        const double* h_ctau, const double* h_csrc, int32_t n_chan,
                        double* d_out, double* d_ftot, void* d_work, size_t work_bytes,
                        void* stream);

/* ---- K7: sensitivities of the light curves to the ejection-burst parameters --------------------
 * Generalises the burst factor of number_density (classes.py:861-875), the y-reduction of
 * optical_depth_ff (classes.py:1395-1432) and the flux sum of flux_ff (classes.py:1519-1521) to
 * their derivatives with respect to the members of rjp_bursts.  For the bursts b of a cell's jet,
 * with d = t_e - ts, G_b = exp(-(d - t0_b)^2 inv2s2_b) and chi = 1 + sum_b amp_rel_b G_b:
 *   S[e, p]           = sum_y |a0| chi^2                            (what rjp_ff_scan returns)
 *   dS/dt0_b          = sum_y |a0| 2 chi amp_rel_b G_b 2 inv2s2_b (d - t0_b)
 *   dS/damp_rel_b     = sum_y |a0| 2 chi G_b
 *   dS/dinv2s2_b      = sum_y |a0| 2 chi amp_rel_b G_b (-(d - t0_b)^2)
 * (sums over the cells of burst b's jet only), from ONE pass over (d_a0, d_ts) per tile of up to
 * four epochs, and
 *   F[e, f]           = sum_p h_cflux[f] tavg[p] (1 - exp(-h_ctau[f] S[e, p]))
 *   dF[e, f]/dtheta_k = sum_p h_cflux[f] tavg[p] h_ctau[f] exp(-h_ctau[f] S[e, p]) dS[e, p]/dtheta_k
 * (h_ctau / h_cflux as for rjp_ff_maps; F with the arithmetic of its d_ftot).
 * n_par = 3 (n[0] + n[1]); parameter k = 3 b + c, where b counts the red jet's bursts first and
 * then the blue jet's, and c = 0: t0 [s], 1: amp_rel, 2: inv2s2 [s^-2].
 * Outputs (device, any may be NULL, not all four):
 *   d_sumA [E * P]                        S
 *   d_dsumA[(e * n_par + k) * P + p]      dS/dtheta_k
 *   d_ftot [E * F]                        F
 *   d_dftot[(e * F + f) * n_par + k]      dF/dtheta_k
 * With d_dsumA NULL the derivative maps live in the workspace one epoch tile at a time.
 * Semantics: nansum as rjp_ff_scan (a NaN d_a0, or a NaN launch time in a jet that has bursts,
 * drops the cell; a NaN tavg drops the pixel from the totals); the cells of a jet WITHOUT bursts
 * have chi = 1 whatever their launch time (classes.py:232-233) -- they add |a0| to S and nothing to
 * any derivative; the call applies that rule itself, d_ts is the model's own field (no
 * rjp_unmask_launch_times copy).  A Gaussian below 2^-1021 counts as zero.  Negative amplitudes are
 * fine.  Sums in a fixed order: bit-reproducible.  d_ylo / d_yhi are honoured; ts_lo / ts_hi, the
 * layouts and the moment cache are not used.
 * Needs RJP_F64 fields with d_a0 (a0_mode == gff_mode) and d_ts; d_tavg, h_ctau, h_cflux and
 * n_chan >= 1 only when d_ftot or d_dftot is asked for.  RJP_ERR_ARG, with nothing enqueued, for:
 * no burst at all, more than 8 bursts in a jet, a non-finite epoch or burst parameter, all four
 * outputs NULL, a wrong dtype or layout; RJP_ERR_WORKSPACE for d_work smaller than
 * rjp_ff_grad_workspace() (n_chan = 0 there: no totals).  Every argument is validated before the
 * first launch. */
size_t rjp_ff_grad_workspace(int32_t nx, int32_t ny, int32_t nz, int32_t n_epochs,
                             int32_t n_par, int32_t n_chan);
int rjp_ff_grad(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                const double* h_epochs_s, int32_t n_epochs, int32_t gff_mode,
                const double* d_tavg, const double* h_ctau, const double* h_cflux, int32_t n_chan,
                double* d_sumA, double* d_dsumA, double* d_ftot, double* d_dftot,
                void* d_work, size_t work_bytes, void* stream);

/* ---- K9: sensitivities of the formal-solution light curves to the burst parameters -------------
 * rjp_ff_grad differentiates the isothermal light curves; this entry point differentiates
 * rjp_ff_formal_sweep's.  For one sightline, cells i from the observer side back, c = h_ctau[f]:
 *   b_i = |a0_i| chi_i^2   dtau_i = c b_i   om_i = 1 - e^-dtau_i   Theta_i = exp(-sum_{j<i} dtau_j)
 *   I              = sum_i T_i om_i Theta_i                              (rjp_ff_formal's pixel)
 *   g_ik           = db_i/dtheta_k, K7's three terms, non-zero only for the bursts of cell i's jet:
 *                    |a0| 2 chi amp G 2 inv2s2 (d - t0),  |a0| 2 chi G,  |a0| 2 chi amp G (-(d - t0)^2)
 *   D_ik           = sum_{j<i} g_jk
 *   dI/dtheta_k    = sum_i c T_i Theta_i [ e^-dtau_i g_ik - om_i D_ik ]
 * -- a cell's own emission rises with its opacity, and what lies behind it is hidden: the two terms
 * have opposite signs.  ONE walk of the fields serves all epochs (lanes over epochs, as K8); the
 * parameters are spread over workgroups in blocks of whole bursts.
 * n_par = 3 (n[0] + n[1]); parameter k = 3 b + c exactly as in rjp_ff_grad: b counts the red jet's
 * bursts first, then the blue jet's; c = 0: t0 [s], 1: amp_rel, 2: inv2s2 [s^-2].
 * Outputs (device, any may be NULL, not all three):
 *   d_ftot [e * F + f]                        rjp_ff_formal_sweep's d_ftot, BIT FOR BIT
 *   d_dftot[(e * F + f) * n_par + k]          nansum_p of the derivative map
 *   d_dout [((e * F + f) * n_par + k) * P + p] h_csrc[f] dI/dtheta_k: NaN exactly where
 *                                             rjp_ff_formal's map is NaN (no T > 0 on the sightline;
 *                                             such a pixel adds nothing to a total); an exact zero
 *                                             where no cell of burst k's jet lies on the sightline
 * Semantics as K8 and K7: a NaN a0, or a NaN launch time in a jet that has bursts, drops the cell;
 * the cells of a jet WITHOUT bursts have chi = 1 whatever their launch time -- g = 0 there, and
 * they still attenuate (the call applies the rule itself, d_ts is the model's own field); a
 * Gaussian below 2^-1021 counts as zero in g; negative amplitudes are fine.  Sums in a fixed order
 * without floating-point atomics: a repeated call, or a call with other outputs NULL, gives the
 * same bits.  d_ylo / d_yhi are honoured; any RJP_F64 layout (tau, compact, wide).
 * RJP_ERR_ARG, nothing enqueued and no output touched, for: a bad gff_mode, no burst at all, more
 * than 8 bursts in a jet, a non-finite epoch or burst parameter, all three outputs NULL, NULL
 * tables, n_epochs < 1, n_chan < 1, n_epochs * n_chan * n_par > 2^31 - 1, RJP_F32 fields, fields
 * without d_ts or d_temp; RJP_ERR_WORKSPACE for d_work smaller than rjp_ff_formal_grad_workspace()
 * (which is 0 for a non-positive argument). */
size_t rjp_ff_formal_grad_workspace(int32_t nx, int32_t ny, int32_t nz, int32_t n_epochs,
                                    int32_t n_par, int32_t n_chan);
int rjp_ff_formal_grad(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                       const double* h_epochs_s, int32_t n_epochs, int32_t gff_mode,
                       const double* h_ctau, const double* h_csrc, int32_t n_chan,
                       double* d_ftot, double* d_dftot, double* d_dout,
                       void* d_work, size_t work_bytes, void* stream);

/* Map stage of intensity_rrl / flux_rrl (classes.py:1280-1282, 1339-1343;
 * rrls.py:444-449; physics.py:571-574):
 *   I_L = B_nu(tavg) exp(-tau_ff) (1 - exp(-tau_rrl)) 1e-3 ; S = I_L * omega / 1e-26
 *   flux[f,p] = S (+ flux_ff[f,p] when d_flux_ff != NULL, i.e. contsub=False)
 * h_cflux_rrl[f] = omega/1e-26 * 1e-3 * 2 h_cgs nu^3 / c_cgs^2 ; h_hnu_k[f] = h nu / k.
 * The Planck factor is 1 / expm1(h nu / k tavg), good to a few ulp; the original's
 * 1 / (exp() - 1) loses 5 to 6 digits at radio frequencies, so the two differ by up to ~5e-11
 * at 1 GHz.  NaN pixels (tavg, or flux_ff where given) stay NaN in d_flux and add nothing to
 * d_ftot; d_flux may be NULL (totals only), d_ftot may be NULL (d_work then unused). */
int rjp_rrl_maps(rjp_ctx* ctx, const double* d_tau_rrl, const double* d_tau_ff,
                 const double* d_tavg, const double* d_flux_ff, int64_t n_pix,
                 const double* h_cflux_rrl, const double* h_hnu_k, int32_t n_chan,
                 double* d_flux, double* d_ftot, void* d_work, size_t work_bytes,
                 void* stream);

/* ---- K6: recombination-line intensity by the formal solution along the line of sight --------
 * The reference's intensity_rrl / flux_rrl (classes.py:1280-1282, 1339-1343; rrls.py:444-449;
 * physics.py:571-574; rjp_rrl_maps here) are isothermal: I_L = B_nu(T_avg) e^-tau_ff
 * (1 - e^-tau_rrl), exact only where T is constant along the sightline and never negative.  This
 * entry point walks every sightline front to back (observer at the iy = 0 end of axis 1, as
 * rjp_ff_formal) with, per cell i and channel f,
 *   c_i = h_ctau[f] b_i     the free-free optical depth, b_i as rjp_ff_formal forms it from the
 *                           wide fields ((|nd| xi)^2 pf T^-1.5 | T^-1.35, times chi^2),
 *   l_i                     the line optical depth, exactly the term rjp_rrl_scan sums and
 *                           rjp_rrl_cells writes (classes.py:1159-1214; rrls.py:350-354, 383-389),
 *   B_i = 1 / expm1(h_hnu_k[f] / T_i)                                  (physics.py:571-574),
 *   I_tot  = sum_i B_i (1 - e^-(c_i + l_i)) exp(-sum_{j < i} (c_j + l_j)),  I_cont: the same, l = 0,
 *   d_out[f * P + p] = h_csrc[f] (I_tot - I_cont)  (+ d_add[f * P + p] when d_add != NULL),
 * the difference accumulated without cancellation.  With a constant T it
 * telescopes to B e^-tau_ff (1 - e^-tau_rrl): the reference's maps are the isothermal special case;
 * with a temperature gradient a pixel can be negative (line absorption against hotter gas behind).
 * h_nu: the channel frequencies [Hz]; h_ctau as for rjp_ff_maps; h_csrc / h_hnu_k as rjp_rrl_maps'
 * h_cflux_rrl / h_hnu_k (divide h_csrc by omega / 1e-26 for intensity).  d_add: typically
 * rjp_ff_formal's flux, for the line-plus-continuum product (contsub=False).
 * A cell contributes its c_i exactly when rjp_ff_formal counts it and its l_i exactly when
 * rjp_rrl_scan does; d_out is NaN exactly where T_avg is.  Reads the wide fields only (d_nd, d_xi,
 * d_temp, d_pf, d_vy; d_ts with bursts), RJP_F32 or RJP_F64; d_ylo / d_yhi are honoured.  One epoch
 * per call; every argument is validated before anything is enqueued (RJP_ERR_ARG otherwise). */
int rjp_rrl_formal(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                   double time_s, int32_t gff_mode, const rjp_line* line, const double* h_nu,
                   const double* h_ctau, const double* h_csrc, const double* h_hnu_k,
                   int32_t n_chan, const double* d_add, double* d_out, void* stream);

/* ---- K10: model visibilities of a stack of maps at given (u, v) points --------------------------
 * An interferometer samples the Fourier transform of the sky; the reference reaches that plane only
 * through FITS files and CASA simobserve, outside this library.  This entry
 * point evaluates the transform of any stack of maps directly at the baselines the caller gives --
 * a direct sum, no gridding, no FFT:
 *   V[m, k] = sum_{ix, iz} I[m, ix nz + iz] exp(-2 pi i (a (ix - (nx-1)/2) + b (iz - (nz-1)/2)))
 *             a = h_su[m] d_u[k],  b = h_sv[m] d_v[k]                      (cycles per cell)
 *   d_maps [n_maps * P]      float64 maps in the library's pixel order p = ix nz + iz: the fluxes of
 *                            the ff / rrl map stages and formal solutions, or K9's d_dout (the
 *                            transform is linear: derivative maps give dV/dtheta)
 *   h_su, h_sv [n_maps]      HOST: cycles per cell per unit of d_u / d_v, signs included -- the ABI
 *                            carries no sky convention (every channel has its own scale)
 *   d_u, d_v [n_vis]         the baselines, in the unit the scales are per
 *   d_vis [n_maps][n_vis][2] (re, im)
 * A NaN pixel adds nothing (the nansum rule of every total here; the maps are NaN off the jet); a map
 * that is NaN everywhere gives exact zeros.  A non-finite d_u[k] or d_v[k] makes visibility k NaN
 * (in every map) and no other.  The sums run in a fixed order without floating-point atomics: a
 * repeated call gives the same bits.
 * ARGUMENT RANGE: every phase a (ix - (nx-1)/2), b (iz - (nz-1)/2) is formed as one double product
 * and reduced to a quarter turn; that needs |a| nx / 2 and |b| nz / 2 below 2^29 cycles (beyond, the
 * result is meaningless, not refused: the baselines live on the device).  The product's rounding
 * costs 2 pi (|a| nx / 2 + |b| nz / 2) 2^-53 of sum |I|: 1e-16 per cycle across the map.
 * Everything else is validated before anything is enqueued, and no output is touched on a refusal:
 * RJP_ERR_ARG for a NULL pointer, n_maps, nx, nz or n_vis < 1, a non-finite h_su / h_sv, or more
 * than 2^31 - 1 tiles (n_maps x ceil(nx / 128) x ceil(n_vis / 64)); RJP_ERR_WORKSPACE for a d_work
 * smaller than the workspace query (16 bytes per map, visibility and tile of 128 x-rows; 0 from it
 * = a bad argument). */
size_t rjp_vis_workspace(int32_t n_maps, int32_t nx, int32_t nz, int32_t n_vis);
int rjp_vis(rjp_ctx* ctx, const double* d_maps, int32_t n_maps, int32_t nx, int32_t nz,
            const double* h_su, const double* h_sv, const double* d_u, const double* d_v,
            int32_t n_vis, double* d_vis, void* d_work, size_t work_bytes, void* stream);

/* ---- K11: dirty images from visibilities, the transpose of K10 ------------------------------------
 * The reference goes from the uv-plane back to the sky only outside itself: CASA tclean transforms
 * the simulated visibilities into the dirty image that imfit then measures (classes.py:2770-2782);
 * nothing inside RaJePy does it.  This entry point evaluates that image directly -- a direct sum, no
 * gridding, no FFT -- for a stack of n_maps visibility sets on the same n_vis baselines:
 *   D[m, ix nz + iz] = sum_k w[k] Re( V[m, k] exp(+2 pi i (a (ix - (nx-1)/2) + b (iz - (nz-1)/2))) )
 *                      a = h_su[m] d_u[k],  b = h_sv[m] d_v[k]              (cycles per cell)
 *   d_vis [n_maps][n_vis][2] (re, im), the layout rjp_vis writes
 *   h_su, h_sv [n_maps]      HOST: cycles per cell per unit of d_u / d_v, signs included; no sky
 *                            convention here either
 *   d_u, d_v [n_vis]         the baselines;  d_w [n_vis] the weights, NULL = all ones
 *   nx, nz                   the OUTPUT grid, pixel order p = ix nz + iz, centre ((nx-1)/2, (nz-1)/2):
 *                            with the scales it need not be the grid the visibilities came from
 *   d_img [n_maps * nx * nz] float64, NOT normalised (divide by sum w for Jy per beam)
 * With the same scales and grid, D is exactly the real transpose of rjp_vis:
 * sum_k w_k Re(conj(Y_k) V_k) = sum_p I_p D_p for V = rjp_vis of I and D = this call on Y.
 * FLAGS: visibility k of map m adds nothing when any of Re V[m,k], Im V[m,k], w[k], d_u[k], d_v[k]
 * is non-finite (the nansum rule; rjp_vis writes NaN for a non-finite baseline, so the chain flags
 * consistently); a map whose visibilities are all flagged gives exact zeros.  The sums run in a
 * fixed order without floating-point atomics: a repeated call gives the same bits.
 * ARGUMENT RANGE: as rjp_vis -- one double product per phase, |a| nx / 2 and |b| nz / 2 below 2^29
 * cycles; the product's rounding costs 2 pi (|a| nx / 2 + |b| nz / 2) 2^-53 of sum_k |w_k| |V_k|
 * per pixel, the sum over k about 2 n_vis 2^-53 more.
 * RETURNS the number of workgroups (output tiles) it enqueued, > 0 -- n_maps x row tiles (128 rows,
 * 64 for nx <= 64) x column tiles (128) x k-splits (fewer than 256 tiles: the visibilities are split
 * over workgroups, at least 64 each, and the partial images summed in split order) -- or a negative
 * RJP_ERR_*: the one entry point whose return value is not a bare status.  Everything is validated
 * before anything is enqueued, and no output or workspace byte is touched on a refusal: RJP_ERR_ARG
 * for a NULL ctx, d_vis, h_su, h_sv, d_u, d_v or d_img, n_maps, n_vis, nx or nz < 1, a non-finite
 * h_su / h_sv, or more than 2^31 - 1 workgroups; RJP_ERR_WORKSPACE for a d_work smaller than the
 * workspace query (8 bytes per map, k-split and pixel, 16 without a split; 0 from it = a bad
 * argument). */
size_t rjp_vis_adjoint_workspace(int32_t n_maps, int32_t nx, int32_t nz, int32_t n_vis);
int64_t rjp_vis_adjoint(rjp_ctx* ctx, const double* d_vis, int32_t n_maps, int32_t n_vis,
                        const double* h_su, const double* h_sv, const double* d_u, const double* d_v,
                        const double* d_w, int32_t nx, int32_t nz, double* d_img,
                        void* d_work, size_t work_bytes, void* stream);

/* ---- K12: Hogbom CLEAN minor cycles on a stack of images -------------------------------------------
 * The reference deconvolves outside itself: CASA tclean(niter=500) on the simulated measurement set
 * (classes.py:2770-2808).  This entry point runs the minor cycles of Hogbom's CLEAN on the dirty
 * images and beams that rjp_vis_adjoint leaves on the device, one fused launch per iteration for the
 * whole stack and nothing going to the host until the end:
 *   d_res [n_maps][nx nz]    the dirty images on entry, the residuals on exit (IN PLACE), pixel order
 *                            p = ix nz + iz
 *   d_psf [n_psf][px pz]     the beams; n_psf = n_maps, or 1 for one beam shared by all maps; px and
 *                            pz ODD, the centre ((px-1)/2, (pz-1)/2) is a pixel.  px = 2 nx - 1,
 *                            pz = 2 nz - 1 is full Hogbom, a smaller beam subtracts only inside its
 *                            window.  Used as given, nothing is normalised (rjp_vis_adjoint of unit
 *                            visibilities on an odd grid, over the sum of the weights, is 1 at the
 *                            centre)
 *   d_mask [nx nz]           uint8, non-zero = the pixel may hold a component; NULL = all pixels; one
 *                            mask for all maps
 *   h_thresh [n_maps]        HOST: each >= 0 and finite;  gain in (0, 1];  n_iter >= 1
 *   d_cpix, d_cflux [n_maps][n_iter], d_ncomp [n_maps]   the components, in the order found
 *   d_model [n_maps][nx nz]  (optional) ADDED to, not overwritten: zero it first
 *   d_peak [n_maps]          (optional) the final masked max |R|, 0 when no pixel qualifies
 * Iteration t of map m: among the pixels that are unmasked and hold a finite R[p], p* is the one with
 * the largest |R[p]|, the lowest p on a tie.  With no such pixel, or |R[p*]| <= h_thresh[m], the map
 * is finished and nothing of it changes any more.  Otherwise f = gain R[p*]; (p*, f) goes to slot t
 * of the map's row of d_cpix / d_cflux, d_model[m][p*] += f, and
 *   R[q] = fma(-f, B[q - p* + centre], R[q])   for every q whose beam index lies inside the beam
 * (one rounding per update).  d_ncomp[m] is the number of components; slots at and beyond it are not
 * written.  A non-finite pixel of R is never picked and is left as it is.  A second call on the
 * residuals (same model) continues the same clean.  Fixed reduction and update order, no atomics: a
 * repeated call on the same input gives the same bits in every output.
 * The workspace holds the per-tile partial maxima (tiles of 1024 consecutive pixels), double
 * buffered: 2 x 12 bytes per map and tile, rounded up to 16.  1 + n_iter (+ 1 with d_peak) launches
 * are enqueued back to back without a host synchronisation.
 * RETURNS, like rjp_vis_adjoint, the number of workgroups of one iteration's launch, > 0 --
 * n_maps x ceil(nx nz / 1024) -- or a negative RJP_ERR_*.  Everything is validated before anything
 * is enqueued, and no output or workspace byte is touched on a refusal: RJP_ERR_ARG for a NULL ctx,
 * d_res, d_psf, h_thresh, d_cpix, d_cflux or d_ncomp; n_maps, nx, nz, px or pz < 1; an even px or
 * pz; an n_psf that is neither 1 nor n_maps; nx nz > 2^31 - 1; a gain outside (0, 1]; n_iter < 1; a
 * negative or non-finite threshold; more than 2^31 - 1 workgroups.  RJP_ERR_WORKSPACE for a d_work
 * smaller than the workspace query (0 from it = a bad argument). */
size_t rjp_clean_workspace(int32_t n_maps, int32_t nx, int32_t nz);
int64_t rjp_clean(rjp_ctx* ctx, double* d_res, int32_t n_maps, int32_t nx, int32_t nz,
                  const double* d_psf, int32_t n_psf, int32_t px, int32_t pz,
                  const uint8_t* d_mask, const double* h_thresh, double gain, int32_t n_iter,
                  int32_t* d_cpix, double* d_cflux, int32_t* d_ncomp, double* d_model,
                  double* d_peak, void* d_work, size_t work_bytes, void* stream);

/* ---- K13: clean components convolved with the clean beam, plus the residual ------------------------
 *   out[m][q] = add[m][q] + sum_{c < ncomp[m]} f_c exp(-(A dx^2 + 2 B dx dz + C dz^2))
 * (dx, dz) the offset of pixel q from component c in cells; (A, B, C) = h_beam[m] in cells^-2 (HOST,
 * [n_maps][3]), a positive definite form: A > 0, C > 0, A C > B^2.  d_cpix / d_cflux / d_ncomp as
 * rjp_clean writes them, rows comp_stride apart (d_ncomp[m] is clamped into [0, comp_stride]);
 * d_add [n_maps][nx nz] the residuals, or NULL; d_out [n_maps][nx nz].  The component fluxes are in
 * Jy when the dirty beam peaks at 1, so the result is Jy per clean beam with no further scale.
 * The sum runs in list order (one fma per term, exp at < 1e-14 relative); a term whose exponent lies
 * below -700 adds an exact zero; the residual is added last.  The same bits on every call.
 * RETURNS the number of workgroups enqueued, > 0 -- n_maps x ceil(nx nz / 256) -- or a negative
 * RJP_ERR_*; nothing is enqueued or touched on a refusal: RJP_ERR_ARG for a NULL ctx, d_cpix, d_cflux,
 * d_ncomp, h_beam or d_out; n_maps, comp_stride, nx or nz < 1; nx nz > 2^31 - 1; a beam that is not
 * finite and positive definite; more than 2^31 - 1 workgroups. */
int64_t rjp_restore(rjp_ctx* ctx, const int32_t* d_cpix, const double* d_cflux,
                    const int32_t* d_ncomp, int32_t n_maps, int32_t comp_stride,
                    const double* h_beam, const double* d_add, int32_t nx, int32_t nz,
                    double* d_out, void* stream);

/* ---- A direct 2-D convolution of a stack of images -------------------------------------------------
 *   out[m][i, j] = add[m][i, j] + sum_{a, b} ker[kappa][a, b] in[m][i - (a - ca), j - (b - cb)]
 * a true convolution (the index is flipped; not a correlation), pixel order p = i nz + j:
 *   d_in, d_add, d_out [n_maps][nx nz]   d_add may be NULL (= 0); d_out must not alias d_in
 *   d_ker [n_ker][kx kz]                 n_ker = n_maps (kappa = m), or 1 for one kernel shared by
 *                                        all maps; kx and kz ODD, at most RJP_CONV_MAX_K, the centre
 *                                        (ca, cb) = ((kx-1)/2, (kz-1)/2)
 * d_in counts as zero outside the image (those terms are taken, as products with 0).  f64
 * throughout, one fma per term, the terms in kernel order -- a outer, b inner, both ascending --
 * and d_add is the accumulator's start: the bits are a function of the inputs alone, and a NaN or
 * infinite pixel propagates by IEEE arithmetic (0 NaN = NaN) to every output its kernel reaches.
 * A workgroup owns RJP_CONV_TILE_X x RJP_CONV_TILE_Z output pixels and stages its input tile plus
 * halo through 64 KiB of LDS, a chunk of kernel rows at a time; RJP_CONV_MAX_K is the widest kernel
 * for which one kernel row plus the tile and its halo fit.
 * RETURNS the number of workgroups enqueued, > 0 -- n_maps x ceil(nx / 16) x ceil(nz / 64) -- or a
 * negative RJP_ERR_*; nothing is enqueued or touched on a refusal: RJP_ERR_ARG for a NULL ctx, d_in,
 * d_ker or d_out; n_maps, nx, nz, kx or kz < 1; an even kx or kz; kx or kz > RJP_CONV_MAX_K; an
 * n_ker that is neither 1 nor n_maps; nx nz > 2^31 - 1; more than 2^31 - 1 workgroups. */
#define RJP_CONV_MAX_K 255
#define RJP_CONV_TILE_X 16
#define RJP_CONV_TILE_Z 64
int64_t rjp_convolve2d(rjp_ctx* ctx, const double* d_in, int32_t n_maps, int32_t nx, int32_t nz,
                       const double* d_ker, int32_t n_ker, int32_t kx, int32_t kz,
                       const double* d_add, double* d_out, void* stream);

/* ---- K17: multi-scale CLEAN minor cycles on a stack of maps ----------------------------------------
 * CASA tclean(deconvolver='multiscale', scales=[...]) is what the reference's Tclean task offers for
 * resolved sources (casa/tasks.py:243-244).  This entry point generalises K12 from one residual
 * plane per map to n_s planes; it is scale-agnostic, the caller prepares planes and cross beams:
 *   d_res [n_maps][n_s][nx nz]   the dirty image convolved with each scale kernel on entry, the
 *                                residual planes on exit (IN PLACE)
 *   d_xpsf [n_psf][n_s (n_s + 1) / 2][px pz]   the cross beams X[k][l], k <= l (the beam convolved
 *                                with scale k and scale l), as a packed upper triangle in row order:
 *                                plane k n_s - k (k - 1) / 2 + (l - k); X[l][k] is the same plane;
 *                                px and pz ODD; n_psf = n_maps, or 1 for one set shared by all maps
 *   h_weight [n_maps][n_s]       HOST: finite and >= 0; 0 = the plane is updated but never picked
 *   d_mask [nx nz]               as K12: one mask for every plane and map; NULL = all pixels
 *   h_thresh [n_maps], gain, n_iter   as K12
 *   d_cpix, d_cscale [n_maps][n_iter] int32, d_cflux [n_maps][n_iter], d_ncomp [n_maps]
 *   d_model [n_maps][n_s][nx nz] (optional) ADDED to: the delta model of each scale
 *   d_peak [n_maps]              (optional) the final best score, 0 when no pixel qualifies
 * Iteration t of map m: among the planes with weight > 0 and the pixels that are unmasked and hold a
 * finite R_k[p], the score is s = weight[k] |R_k[p]| (one rounding).  The largest s is taken, on a tie
 * the lower k, then the lower p.  With no candidate, or s* <= h_thresh[m], the map is finished and
 * nothing of it changes any more.  Otherwise f = (gain R_k*[p*]) / X[k*][k*][centre] (one product,
 * one division, both correctly rounded); (p*, k*, f) goes to slot t, d_model[m][k*][p*] += f, and for
 * EVERY plane l
 *   R_l[q] = fma(-f, X[k*][l][q - p* + centre], R_l[q])   for every q inside the beam window.
 * A map whose X[k][k][centre] is zero or not finite for some k of weight > 0 is finished from the
 * start: d_ncomp[m] = 0, d_peak[m] = 0.  Slots at and beyond d_ncomp[m] are not written; a non-finite
 * pixel is never picked and is left as it is; a second call on the planes continues the same clean.
 * One launch per iteration for the whole stack, grid = tiles x planes x maps, per-tile partial maxima
 * in a double-buffered workspace (2 x 12 bytes per map, plane and tile of 1024 pixels, rounded up to
 * 16), no atomics, every reduction in a fixed order: a repeated call gives the same bits.  With
 * n_s = 1, weight 1 and a beam whose centre is exactly 1.0 every output equals rjp_clean's bit for bit.
 * RETURNS the number of workgroups of one iteration's launch, > 0 -- n_maps x n_s x
 * ceil(nx nz / 1024) -- or a negative RJP_ERR_*.  Everything is validated before anything is
 * enqueued, and no output or workspace byte is touched on a refusal: RJP_ERR_ARG for K12's refusals
 * (with d_xpsf for d_psf), a NULL h_weight or d_cscale, n_s < 1, a negative or non-finite weight,
 * more than 2^31 - 1 workgroups.  RJP_ERR_WORKSPACE for a d_work smaller than the workspace query
 * (0 from it = a bad argument, or a size that overflows). */
size_t rjp_msclean_workspace(int32_t n_maps, int32_t n_s, int32_t nx, int32_t nz);
int64_t rjp_msclean(rjp_ctx* ctx, double* d_res, int32_t n_maps, int32_t n_s, int32_t nx,
                    int32_t nz, const double* d_xpsf, int32_t n_psf, int32_t px, int32_t pz,
                    const double* h_weight, const uint8_t* d_mask, const double* h_thresh,
                    double gain, int32_t n_iter, int32_t* d_cpix, int32_t* d_cscale,
                    double* d_cflux, int32_t* d_ncomp, double* d_model, double* d_peak,
                    void* d_work, size_t work_bytes, void* stream);

/* ---- K19: multi-term MFS CLEAN minor cycles on a stack of maps -- spectral-index maps --------------
 * CASA tclean(deconvolver='mtmfs', nterms=2) is what the reference's Tclean task offers for a band
 * (`nterms` beside `deconvolver` and `scales`: casa/tasks.py:243-246).  Sault & Wieringa 1994 /
 * Rau & Cornwell 2011 at a single scale: the sky is I(nu) = sum_t I_t w^t, w = (nu - nu_0) / nu_0,
 * and the minor cycle works on n_t Taylor residual planes coupled through a small Hessian.  The entry
 * point is agnostic of frequencies, like rjp_msclean: the caller prepares planes, beams and Hinv.
 *   d_res [n_maps][n_t][nx nz]   the Taylor residual planes R_t (the dirty image of the visibilities
 *                                times w^t), updated IN PLACE
 *   d_spsf [n_psf][2 n_t - 1][px pz]   the spectral beams B_q (the beam of unit visibilities times
 *                                w^q); px and pz ODD; n_psf = n_maps, or 1 for one set for all maps
 *   h_hinv [n_maps][n_t][n_t]    HOST: the inverse of the Hessian H[t][q] = B_{t+q}(centre), every
 *                                entry finite; used as given, row by row (no symmetry is assumed)
 *   d_mask [nx nz], h_thresh [n_maps], gain, n_iter   as K12
 *   d_cpix [n_maps][n_iter] int32, d_ccoef [n_maps][n_iter][n_t], d_ncomp [n_maps]
 *   d_model [n_maps][n_t][nx nz] (optional) ADDED to: the delta model of each Taylor term
 *   d_peak [n_maps]              (optional) the final masked max |a_0|, 0 when no pixel qualifies
 * ARITHMETIC.  At a pixel p, term q of the principal solution is
 *   a_q = Hinv[q][0] R_0[p]  (one product),  then a_q = fma(Hinv[q][t], R_t[p], a_q), t = 1 .. n_t - 1.
 * Iteration i of map m: among the pixels that are unmasked and finite in ALL n_t planes, p* is the one
 * with the largest |a_0(p)|, the lowest p on a tie.  With no such pixel, or |a_0(p*)| <= h_thresh[m],
 * the map is finished and nothing of it changes any more.  Otherwise c_q = gain a_q(p*) (one product)
 * for every q; (p*, c_0 .. c_{n_t-1}) goes to slot i, d_model[m][t][p*] += c_t, and for every plane t
 *   r = R_t[x];  r = fma(-c_q, B_{t+q}[x - p* + centre], r)  for q = 0 .. n_t - 1 ascending;  R_t[x] = r
 * for every x whose beam index lies inside the beam: n_t roundings per update.  A pixel that is
 * non-finite in plane t is never a candidate; it is left as it is in that plane and updated normally
 * in the others.  Slots at and beyond d_ncomp[m] are not written.  A second call on the planes
 * continues the same clean.  No atomics, every reduction in a fixed order: a repeated call gives the
 * same bits.  With n_t = 1, Hinv = 1.0 and a beam whose centre is exactly 1.0 every output equals
 * rjp_clean's bit for bit.
 * One launch per iteration for the whole stack, grid = tiles x maps; one workgroup holds all n_t
 * planes of its tile of 1024 pixels.  A tile's partial carries the pixel and the n_t plane values at
 * it, double buffered: 2 x (8 n_t + 4) bytes per map and tile, rounded up to 16.
 * RETURNS the number of workgroups of one iteration's launch, > 0 -- n_maps x ceil(nx nz / 1024) --
 * or a negative RJP_ERR_*.  Everything is validated before anything is enqueued, and no output or
 * workspace byte is touched on a refusal: RJP_ERR_ARG for K12's refusals (with d_spsf for d_psf), a
 * NULL h_hinv or d_ccoef, n_t outside 1 .. RJP_MTMFS_MAX_NT, a non-finite h_hinv entry, more than
 * 2^31 - 1 workgroups.  RJP_ERR_WORKSPACE for a d_work smaller than the workspace query (0 from it =
 * a bad argument, or a size that overflows). */
#define RJP_MTMFS_MAX_NT 4
size_t rjp_mtmfs_workspace(int32_t n_maps, int32_t n_t, int32_t nx, int32_t nz);
int64_t rjp_mtmfs(rjp_ctx* ctx, double* d_res, int32_t n_maps, int32_t n_t, int32_t nx, int32_t nz,
                  const double* d_spsf, int32_t n_psf, int32_t px, int32_t pz,
                  const double* h_hinv, const uint8_t* d_mask, const double* h_thresh, double gain,
                  int32_t n_iter, int32_t* d_cpix, double* d_ccoef, int32_t* d_ncomp,
                  double* d_model, double* d_peak, void* d_work, size_t work_bytes, void* stream);

/* ---- K18: the visibilities of a list of clean components -- the forward step of a major cycle -------
 * CASA tclean alternates minor cycles in the image plane with major cycles that recompute the residual
 * from the visibilities; the reference's Tclean task carries the controls (cycleniter, cyclefactor,
 * minpsffraction, maxpsffraction: casa/tasks.py:259-262).  The forward step of a major cycle is the
 * model's visibilities.  From a component list they cost n_comp x n_vis phasors, where rjp_vis on the
 * dense model image costs nx nz x n_vis multiply-adds:
 *   out[m,k] = in[m,k] + sign sum_s G[m,s,k] sum_{c < ncomp[m], cscale[m,c] = s}
 *              f_c exp(-2 pi i (a (ix_c - (nx-1)/2) + b (iz_c - (nz-1)/2)))
 *              a = h_su[m] d_u[k],  b = h_sv[m] d_v[k],  p_c = ix_c nz + iz_c
 *   d_cpix, d_cflux [n_maps][comp_stride], d_ncomp [n_maps]   as rjp_clean / rjp_msclean write them,
 *                            rows comp_stride apart (d_ncomp[m] is clamped into [0, comp_stride])
 *   d_cscale [n_maps][comp_stride]   (optional) the scale of each component; NULL = all of scale 0
 *   n_s                      the number of scales;  nx, nz the grid the pixels index
 *   h_su, h_sv [n_maps]      HOST, d_u, d_v [n_vis]: as rjp_vis
 *   d_gvis [n_maps][n_s][n_vis][2]   (optional) G, the transform of each scale's kernel at each
 *                            visibility: rjp_vis of the kernel images, zero-padded and centred on one
 *                            odd side.  NULL = G = 1, the Hogbom case, and needs n_s = 1.  The entry
 *                            point is scale-agnostic, like rjp_msclean
 *   d_in [n_maps][n_vis][2]  (optional) NULL = 0;  d_out [n_maps][n_vis][2] may be d_in (in place)
 *   sign                     +1 or -1, applied to the flux (exact): -1 forms V - model
 * Every phase is ONE double product per factor, a (ix - (nx-1)/2) and b (iz - (nz-1)/2), reduced and
 * evaluated by the library's sine / cosine of an argument in turns, exactly as rjp_vis forms its
 * phasors (its ARGUMENT RANGE holds here too); no recurrence, no float.  The sums run in a fixed
 * order without atomics -- per (map, visibility): the scales ascending; inside a scale four slices
 * of the list, slice w = the components c with (c mod 256) / 64 = w, each in list order, one fma
 * per term and part; G multiplies each slice's sum of a scale once (two fmas per part); the four
 * slices are added in slice order and `in` last -- so a repeated call gives the same bits.
 * A component adds nothing if its flux is not finite, its pixel lies outside [0, nx nz) or its scale
 * outside [0, n_s).  A non-finite d_u[k] or d_v[k] makes visibility k NaN in every map and touches no
 * other visibility.  A non-finite in[m,k] stays non-finite (it is a flag: rjp_vis_adjoint skips it).
 * A map with ncomp = 0 copies `in` bit for bit, -0.0 included.  One launch, 64 visibilities of one
 * map per workgroup, no workspace.
 * RETURNS the number of workgroups enqueued, > 0 -- n_maps x ceil(n_vis / 64) -- or a negative
 * RJP_ERR_*; nothing is enqueued or touched on a refusal: RJP_ERR_ARG for a NULL ctx, d_cpix, d_cflux,
 * d_ncomp, h_su, h_sv, d_u, d_v or d_out; n_maps, comp_stride, n_s, nx, nz or n_vis < 1; a sign
 * other than +1 / -1; a NULL d_gvis with n_s != 1; a non-finite h_su / h_sv; nx nz > 2^31 - 1; more
 * than 2^31 - 1 workgroups.
 *
 * rjp_components_image: the delta model of the same list, one plane per scale,
 *   out[m][s][q] = sum_{c < ncomp[m]: p_c = q, cscale[m,c] = s} f_c      in list order, from +0.0
 * -- rjp_restore with a delta beam; d_out [n_maps][n_s][nx nz] is overwritten.  The component rules
 * are those above.  The model image is thereby a function of the list alone, without atomics, and
 * equals bit for bit what rjp_clean and rjp_msclean add into a zeroed d_model.
 * RETURNS the number of workgroups enqueued, > 0 -- n_maps x n_s x ceil(nx nz / 256) -- or a negative
 * RJP_ERR_*; nothing is enqueued or touched on a refusal: RJP_ERR_ARG for a NULL ctx, d_cpix, d_cflux,
 * d_ncomp or d_out; n_maps, comp_stride, n_s, nx or nz < 1; nx nz > 2^31 - 1; more than 2^31 - 1
 * workgroups. */
int64_t rjp_vis_components(rjp_ctx* ctx, const int32_t* d_cpix, const int32_t* d_cscale,
                           const double* d_cflux, const int32_t* d_ncomp, int32_t n_maps,
                           int32_t comp_stride, int32_t n_s, int32_t nx, int32_t nz,
                           const double* h_su, const double* h_sv, const double* d_u,
                           const double* d_v, int32_t n_vis, const double* d_gvis,
                           const double* d_in, int32_t sign, double* d_out, void* stream);
int64_t rjp_components_image(rjp_ctx* ctx, const int32_t* d_cpix, const int32_t* d_cscale,
                             const double* d_cflux, const int32_t* d_ncomp, int32_t n_maps,
                             int32_t comp_stride, int32_t n_s, int32_t nx, int32_t nz,
                             double* d_out, void* stream);

/* ---- K14: Gaussian fits of a stack of images (imfit) ----------------------------------------------
 * The reference measures its synthetic images outside itself: CASA imfit on the restored image
 * (classes.py:2790-2840).  This entry point fits one elliptical Gaussian per map by
 * Levenberg-Marquardt, one fused launch per iteration for the whole stack and nothing going to the
 * host until the end:
 *   G(ix, iz) = S exp(-(A dx^2 + 2 B dx dz + C dz^2)),  dx = ix - x0, dz = iz - z0,
 * theta = (S, x0, z0, A, B, C): peak [the image's unit, may be negative], centre [pixels], and the
 * quadratic form in cells^-2 (A > 0, C > 0, A C > B^2), no offset.  exp to < 1e-14 relative, an exact
 * 0 below an exponent of -700.
 *   d_img [n_maps][nx nz]    the images (READ ONLY), pixel order p = ix nz + iz
 *   h_box [4]                HOST: (i0, i1, j0, j1), inclusive corners of the fitting box
 *   d_mask [nx nz]           uint8, non-zero = the pixel counts; NULL = all; one mask for all maps
 *   d_theta [n_maps][6]      the start on entry, the fit on exit (IN PLACE)
 *   lambda0, xtol            finite and > 0;  n_iter >= 1
 *   d_chi2 [n_maps], d_cov [n_maps][21], d_npix, d_niter, d_status [n_maps] (int32)
 *   d_trace [n_maps][n_iter][9]   (optional) per iteration (chi^2 of the trial, the lambda that
 *                            proposed it, accepted 0 / 1, the trial's six parameters); rows at and
 *                            beyond d_niter[m] are not written
 * A pixel counts when it lies in the box, is non-zero in the mask and finite in the image.  With
 * r = I - G and J = dG / dtheta over the counting pixels: chi^2 = sum r^2, N = J^T J, g = J^T r.
 * Iteration t = 1, 2, ... evaluates one trial (the first: the start, with chi^2_cur = +inf) and
 * decides, in this order:
 *   1. accept iff the trial is positive definite, its chi^2 is finite and < chi^2_cur; on accept
 *      theta_cur, chi^2_cur, N, g become the trial's and lambda <- max(lambda / 10, 1e-12) (accepting
 *      the start leaves lambda0); on reject lambda <- 10 lambda;
 *   2. chi^2_cur = 0 -> status 1.  Else delta from (N + lambda diag N) delta = g by a 6 x 6
 *      Cholesky; a pivot that is not > 0 counts as a reject (lambda <- 10 lambda, again);
 *      lambda > 1e12 -> status 2 (stalled);
 *   3. max_i |delta_i| / s_i <= xtol, s = (max(|S|, 1e-300), 1, 1, A + C, A + C, A + C) -> status 1 (converged;
 *      tested on every proposed step); n_iter trials done -> status 0; else the next trial is
 *      theta_cur + delta.
 * status 3 (degenerate): a start that is not finite and positive definite, a first chi^2 that is
 * not finite, or fewer than 6 counting pixels; d_status[m] = 3 and NOTHING else of that map is
 * written.  Otherwise d_theta / d_chi2 are theta_cur / chi^2_cur, d_cov the packed upper triangle
 * (row by row) of N at theta_cur, NOT inverted, d_npix the counting pixels, d_niter the trials
 * evaluated.  Calling again with the returned d_theta continues the fit (lambda starts over).
 * Tiles of 1024 consecutive pixels of the box in the box's row-major order; every sum in a fixed
 * order, no atomics: a repeated call gives the same bits in every output.  The workspace holds the
 * 29 partial sums per tile and 48 doubles of state per map, both double buffered.  n_iter + 1
 * launches are enqueued back to back without a host synchronisation.
 * RETURNS, like rjp_clean, the number of workgroups of one iteration's launch, > 0 --
 * n_maps x ceil(box pixels / 1024) -- or a negative RJP_ERR_*.  Everything is validated before
 * anything is enqueued, and no output or workspace byte is touched on a refusal: RJP_ERR_ARG for a
 * NULL ctx, d_img, h_box, d_theta, d_chi2, d_cov, d_npix, d_niter or d_status; n_maps, nx or nz < 1;
 * nx nz > 2^31 - 1; a box outside the image or with i1 < i0 or j1 < j0; lambda0 or xtol not finite
 * and positive; n_iter < 1; more than 2^31 - 1 workgroups.  RJP_ERR_WORKSPACE for a d_work smaller
 * than the workspace query (0 from it = a bad argument). */
size_t rjp_gaussfit_workspace(int32_t n_maps, int32_t box_pixels);
int64_t rjp_gaussfit(rjp_ctx* ctx, const double* d_img, int32_t n_maps, int32_t nx, int32_t nz,
                     const int32_t* h_box, const uint8_t* d_mask, double* d_theta, double lambda0,
                     double xtol, int32_t n_iter, double* d_chi2, double* d_cov, int32_t* d_npix,
                     int32_t* d_niter, int32_t* d_status, double* d_trace, void* d_work,
                     size_t work_bytes, void* stream);

/* ---- K15: uniform and Briggs imaging weights from the (u, v) density -------------------------------
 * The reference weights its visibilities outside itself: CASA tclean(weighting='briggs', robust=0.5)
 * (classes.py:2775-2776).  CASA is not at hand, so this comment IS the definition; parity with
 * CASA is not claimed.  Per map m on an imaging grid of nx x nz cells, hx = nx / 2, hz = nz / 2
 * (integer division), for n_vis visibilities shared by all maps:
 *   gu = rint((h_su[m] d_u[k]) nx),  gv = rint((h_sv[m] d_v[k]) nz)   float64 products in this order,
 *                            ties to even: the Fourier plane binned at 1 / (nx cell)
 *   FLAGGED: d_u[k], d_v[k] or d_w[k] not finite, or d_w[k] < 0 (d_w = NULL: all ones)
 *   IN RANGE: |gu| <= hx and |gv| <= hz, compared in double: a symmetric grid of
 *                            (2 hx + 1)(2 hz + 1) cells that holds the mirror of each of its cells
 *   COUNTED = not flagged and in range; every other visibility adds nothing and gets the weight 0
 *   W(c) = S(c) + S(-c), S(c) the sum of the counted weights in cell c (Hermitian gridding: the origin
 *                            cell counts its visibilities twice), summed in FIXED POINT:
 *                            w_max = the largest counted weight of the call (any map), w_max < 2^e
 *                            (frexp), L = ceil(log2(2 n_vis)), s = 62 - e - L, q_k = (int64) rint(w_k 2^s),
 *                            W(c) = (double)(sum q) 2^-s with one correctly rounded conversion; the
 *                            total of a map stays below 2^62.  w_max = 0: s = 0 and all outputs 0
 *   mode 1, uniform:         w'_k = w_k / W(c_k)   (0 where W(c_k) = 0: weights below 2^-s-1 only)
 *   mode 2, Briggs (Briggs 1995, casacore's "norm" form): f2 = (5 10^-robust)^2 (2 sum_k w_k) /
 *                            sum_c W(c)^2, k over the map's counted visibilities with sum_k w_k =
 *                            (sum q) 2^-s, c over all cells;  w'_k = w_k / fma(f2, W(c_k), 1)
 *   d_wout [n_maps][n_vis]   the weights
 *   d_stats [n_maps][6]      (optional) sum_k w_k (exact), sum_c W^2, f2 (0 in mode 1), the counted
 *                            visibilities, the unflagged ones out of range, s
 *   d_density [n_maps][(2 hx + 1)(2 hz + 1)]   (optional) W(c) at (gu + hx)(2 hz + 1) + (gv + hz)
 * The integer sums have no order, sum_c W^2 is a float64 sum in a fixed order (tiles of 1024 cells
 * in tile order) and there are no floating-point atomics: a repeated call gives the same bits, a
 * permutation of the visibilities permutes the weights and changes nothing else, and replacing any
 * (u, v) by (-u, -v) changes nothing.  A map without a counted visibility gets zeros and f2 = 0.
 * One memset (the density and the counters) and five launches for the whole stack, no host
 * synchronisation.
 * RETURNS, like rjp_vis_adjoint, the number of workgroups of the scatter launch, > 0 -- n_maps x
 * ceil(n_vis / 256) -- or a negative RJP_ERR_*.  Everything is validated before anything is enqueued,
 * and no output or workspace byte is touched on a refusal: RJP_ERR_ARG for a NULL ctx, h_su, h_sv,
 * d_u, d_v or d_wout; n_maps, n_vis, nx or nz < 1; a non-finite h_su / h_sv; a mode other than 1 or
 * 2; in mode 2 a robust that is not finite or outside [-2, 2]; more than 2^31 - 1 density cells per
 * map or workgroups in a launch.  RJP_ERR_WORKSPACE for a d_work smaller than the workspace query
 * (256 bytes, 32 per map, 8 per tile of 1024 cells and 8 per cell; 0 from it = a bad argument or
 * a grid of more than 2^31 - 1 cells). */
size_t rjp_uv_weights_workspace(int32_t n_maps, int32_t nx, int32_t nz, int32_t n_vis);
int64_t rjp_uv_weights(rjp_ctx* ctx, int32_t n_maps, int32_t n_vis, const double* h_su,
                       const double* h_sv, const double* d_u, const double* d_v, const double* d_w,
                       int32_t nx, int32_t nz, int32_t mode, double robust, double* d_wout,
                       double* d_stats, double* d_density, void* d_work, size_t work_bytes,
                       void* stream);

/* ---- K16: synthetic observations -- (u, v, w) tracks of an array and thermal noise ---------------
 * The reference observes its models outside itself: CASA simobserve (classes.py:2490-2650).  CASA is
 * not at hand, so this comment IS the definition; parity with simobserve is not claimed.
 *
 * TRACKS.  Earth-rotation synthesis of n_ant antennas over n_t integrations:
 *   h_xyz [n_ant][3]   geocentric (ITRF) antenna positions [m]
 *   h_gha [n_t]        Greenwich hour angle of the phase centre per integration, in TURNS; it is
 *                      reduced exactly, g = gha - rint(gha), and G = 2 pi g is evaluated by the
 *                      library's sine / cosine of an argument in turns (truncation < 2e-14 / 1e-15)
 *   sin_dec, cos_dec   of the phase centre's declination
 *   h_up [n_ant][3]    (optional) unit local verticals;  sin_min_el: sine of the elevation limit
 *   d_u, d_v, d_w [n_t][n_bl]   [m]; d_w may be NULL.  n_bl = n_ant (n_ant - 1) / 2, the pairs (i < j)
 *                      in i-major order -- (0,1), (0,2), ..., (1,2), ... -- with b = xyz_j - xyz_i:
 *   u =          sinG bx +         cosG by
 *   v = -sin_dec cosG bx + sin_dec sinG by + cos_dec bz
 *   w =  cos_dec cosG bx - cos_dec sinG by + sin_dec bz
 * The source direction in the ITRF frame is s = (cos_dec cosG, -cos_dec sinG, sin_dec).
 * FLAGS: with h_up, antenna i is below the limit at integration t when up_i . s(t) < sin_min_el
 * (float64; a NaN limit flags nothing); a baseline with either antenna below it gets u = v = w = NaN
 * -- the flag the chain honours: rjp_vis writes a NaN visibility there, rjp_vis_adjoint and
 * rjp_uv_weights drop it.  A non-finite h_gha[t] flags the whole integration t.  The ABI carries no
 * geography beyond this: no dates, no longitude (GHA = local hour angle - east longitude is the
 * caller's).  One launch, one thread per (t, baseline), no atomics: the same bits on every call.
 * RETURNS the number of workgroups of the launch, > 0 -- n_t x ceil(n_bl / 256) -- or a negative
 * RJP_ERR_*.  Everything is validated before anything is enqueued, and no output byte is touched on
 * a refusal: RJP_ERR_ARG for a NULL ctx, h_xyz, h_gha, d_u or d_v; n_ant < 2; n_t < 1; a non-finite
 * h_xyz, sin_dec or cos_dec; |sin_dec^2 + cos_dec^2 - 1| > 1e-12; n_t n_bl > 2^31 - 1.
 *
 * NOISE.  Thermal noise that is a pure function of (seed, map, visibility), on the
 * [n_maps][n_vis][2] layout (re, im) of rjp_vis's output:
 *   d_out[m][k] = d_vis[m][k] + h_sigma[m] s_k (g1 + i g2),   s_k = d_s[k] (d_s = NULL: all ones)
 * d_out may be d_vis (in place).  (g1, g2) come from ONE block of Philox4x32-10 (Salmon et al. 2011;
 * multipliers D2511F53 / CD9E8D57, Weyl constants 9E3779B9 / BB67AE85):
 *   key     = (low, high 32 bits of seed)
 *   counter = (low 32 bits of k0 + k, high 32 bits of k0 + k, m0 + m, 0)
 * k0 (int64) and m0 (int32) are the offsets of this call's chunk inside the whole data set, so that
 * chunked calls reproduce the unchunked bits.  The output words x0 .. x3 give
 *   n1 = (x0 << 20) | (x1 >> 12)  (52 bits),  u1 = (2 n1 + 1) 2^-53,  u2 likewise from x2, x3
 * -- exact in float64 and strictly inside (0, 1) -- and Box-Muller
 *   r = sqrt(-2 log(u1)),  g1 = r cos(2 pi u2),  g2 = r sin(2 pi u2)
 * with the same sine / cosine of an argument in turns; the real part is fma((sigma s_k) r, cos, Re V),
 * the imaginary part likewise with the sine.  A map whose h_sigma[m] is 0 is copied bit for bit
 * (V + 0 g would turn -0.0 into +0.0).  NaN visibilities stay NaN.  A non-finite d_s[k] makes
 * visibility k NaN in EVERY map, those with sigma = 0 included (it flags the visibility).  No
 * atomics and no dependence on the launch shape: a repeated call, a call split into chunks with
 * k0 / m0, and in place against out of place all give identical bits.  One launch.
 * RETURNS the number of workgroups of the launch, > 0 -- n_maps x ceil(n_vis / 256) -- or a negative
 * RJP_ERR_*, validated like the tracks: RJP_ERR_ARG for a NULL ctx, d_vis, h_sigma or d_out; n_maps
 * or n_vis < 1; a negative or non-finite h_sigma; k0 < 0 or k0 + n_vis > 2^63 - 1; m0 < 0 or
 * m0 + n_maps > 2^31 - 1; more than 2^31 - 1 workgroups. */
int64_t rjp_uv_tracks(rjp_ctx* ctx, const double* h_xyz, int32_t n_ant, const double* h_gha,
                      int32_t n_t, double sin_dec, double cos_dec, const double* h_up,
                      double sin_min_el, double* d_u, double* d_v, double* d_w, void* stream);
int64_t rjp_vis_noise(rjp_ctx* ctx, const double* d_vis, int32_t n_maps, int32_t n_vis,
                      const double* h_sigma, const double* d_s, uint64_t seed, int64_t k0,
                      int32_t m0, double* d_out, void* stream);

/* ---- K20: point and Gaussian components fitted to visibilities (uvmodelfit) -----------------------
 * Radio astronomers measure barely resolved sources in the uv plane (CASA uvmodelfit, difmap
 * modelfit): the data are independent, the weights thermal, no beam enters and a point source is an
 * ordinary point of the parameter space.  CASA is not at hand, so this comment IS the definition;
 * parity with uvmodelfit is not claimed.  This entry point fits n_comp components per map by
 * Levenberg-Marquardt, one fused launch per iteration for the whole stack and nothing going to the
 * host until the end.  For map m and visibility k, in float64,
 *   a = h_su[m] * d_u[k],  b = h_sv[m] * d_v[k]      cycles per cell (the convention of rjp_vis;
 *                                                     the ABI carries no sky convention)
 * and per component c with theta_c = (F, x, z, sxx, sxz, szz) -- flux [the visibilities' unit],
 * offset from the phase centre [cells; ix - (nx - 1) / 2, iz - (nz - 1) / 2 of rjp_vis] and the
 * sky-plane covariance [cells^2]; a point source is sxx = sxz = szz = 0 --
 *   ph = fma(a, x, b * z)                             phase in turns, |ph| < 2^30; sine and cosine
 *                                                     of 2 pi ph to < 2e-14 / 1e-15 absolute
 *   q  = fma(sxx, a * a, fma(2 sxz, a * b, szz * (b * b)))
 *   e  = q * -19.739208802178716                      (-2 pi^2; one rounding)
 *   E  = exp(e) to < 1e-14 relative, an exact 0 for e < -700
 *   M[m][k] = sum_c (F E) (cos - i sin)               = sum_c F exp(-2 pi^2 q) exp(-2 pi i ph),
 *                                                     added in component order
 * This is the transform of K14's S exp(-(A dx^2 + 2 B dx dz + C dz^2)) with Sigma = (2 Q)^-1 and
 * F = S pi / sqrt(det Q).
 *   d_vis [n_maps][n_vis][2]  the data (READ ONLY), (re, im) as rjp_vis writes them
 *   d_u, d_v [n_vis];  h_su, h_sv [n_maps]  HOST, finite
 *   d_w                       NULL (all ones) or [w_maps][n_vis], w_maps 1 (shared) or n_maps
 *   n_comp                    1 .. RJP_UVFIT_MAX_COMP;  P = 6 n_comp parameters per map
 *   h_free [n_comp][6]        HOST uint8, non-zero = the parameter is fitted; one pattern for all
 *                             maps; NULL = all free; at least one must be free
 *   d_theta [n_maps][P]       the start on entry, the fit on exit (IN PLACE)
 *   lambda0, xtol             finite and > 0;  n_iter >= 1
 *   d_chi2 [n_maps], d_cov [n_maps][P (P + 1) / 2], d_nvis, d_niter, d_status [n_maps] (int32)
 *   d_trace [n_maps][n_iter][3 + P]   (optional) per iteration (chi^2 of the trial, the lambda that
 *                             proposed it, accepted 0 / 1, the trial's P parameters); rows at and
 *                             beyond d_niter[m] are not written
 * Visibility k of map m counts when Re V, Im V, u, v and w are finite and w > 0.  With r = V - M and
 * J = dM / dtheta over the counting visibilities:
 *   chi^2 = sum w |r|^2,  N = Re(J^H W J),  g = Re(J^H W r).
 * A fixed parameter keeps its start value: its row and column of N are replaced by the identity's
 * and its g by 0, so that its step is exactly 0.  This is how a point component is fitted (sizes
 * fixed at 0) and how a position is held.
 * Iteration t = 1, 2, ... evaluates one trial (the first: the start, with chi^2_cur = +inf) and
 * decides, in this order:
 *   1. accept iff every component of the trial is positive SEMI-definite (sxx >= 0, szz >= 0,
 *      sxx szz >= sxz^2), its chi^2 is finite and < chi^2_cur; on accept theta_cur, chi^2_cur, N, g
 *      become the trial's and lambda <- max(lambda / 10, 1e-12) (accepting the start leaves
 *      lambda0); on reject lambda <- 10 lambda;
 *   2. chi^2_cur = 0 -> status 1.  Else delta from (N + lambda diag N) delta = g by a P x P
 *      Cholesky; a pivot that is not > 0 counts as a reject (lambda <- 10 lambda, again);
 *      lambda > 1e12 -> status 2 (stalled);
 *   3. max_i |delta_i| / s_i <= xtol, s = (max(|F|, 1e-300), 1, 1, t, t, t) with t = max(sxx + szz, 1)
 *      per component -> status 1 (converged; tested on every proposed step); n_iter trials done ->
 *      status 0; else the next trial is theta_cur + delta.
 * status 3 (degenerate): a start that is not finite or not positive semi-definite, a first chi^2
 * that is not finite, or 2 x (counting visibilities) < the number of free parameters; d_status[m] =
 * 3 and NOTHING else of that map is written.  Otherwise d_theta / d_chi2 are theta_cur / chi^2_cur,
 * d_cov the packed upper triangle (row by row) of N at theta_cur with the identity's rows for fixed
 * parameters, NOT inverted, d_nvis the counting visibilities, d_niter the trials evaluated.  Calling
 * again with the returned d_theta continues the fit (lambda starts over).
 * Tiles of 1024 consecutive visibilities; every sum in a fixed order, no atomics: a repeated call
 * gives the same bits in every output.  The workspace holds 1 + P (P + 1) / 2 + P + 1 partial sums
 * per tile (29, 92) and 48 / 120 doubles of state per map, both double buffered.  n_iter + 1
 * launches are enqueued back to back without a host synchronisation.
 * RETURNS, like the K14 entry point, the number of workgroups of one iteration's launch, > 0 --
 * n_maps x ceil(n_vis / 1024) -- or a negative RJP_ERR_*.  Everything is validated before anything
 * is enqueued, and no output or workspace byte is touched on a refusal: RJP_ERR_ARG for a NULL ctx,
 * d_vis, h_su, h_sv, d_u, d_v, d_theta, d_chi2, d_cov, d_nvis, d_niter or d_status; n_maps or
 * n_vis < 1; n_comp outside 1 .. RJP_UVFIT_MAX_COMP; with d_w a w_maps that is neither 1 nor n_maps;
 * a non-finite h_su / h_sv; no free parameter; lambda0 or xtol not finite and positive; n_iter < 1;
 * more than 2^31 - 1 workgroups.  RJP_ERR_WORKSPACE for a d_work smaller than the workspace query
 * (0 from it = a bad argument). */
#define RJP_UVFIT_MAX_COMP 2
size_t rjp_uvfit_workspace(int32_t n_maps, int32_t n_vis, int32_t n_comp);
int64_t rjp_uvfit(rjp_ctx* ctx, const double* d_vis, int32_t n_maps, int32_t n_vis,
                  const double* h_su, const double* h_sv, const double* d_u, const double* d_v,
                  const double* d_w, int32_t w_maps, int32_t n_comp, const uint8_t* h_free,
                  double* d_theta, double lambda0, double xtol, int32_t n_iter, double* d_chi2,
                  double* d_cov, int32_t* d_nvis, int32_t* d_niter, int32_t* d_status,
                  double* d_trace, void* d_work, size_t work_bytes, void* stream);

/* ---- K21: moment maps and per-sightline line fits of a cube (immoments, specfit) -----------------
 * What an astronomer wants of a recombination-line cube: the integrated line flux, the velocity
 * field, the line width, and a line profile fitted per sightline (CASA immoments and specfit, the
 * third fitting task after imfit = K14 and uvmodelfit = K20).  CASA is not at hand, so this
 * comment IS the definition; parity is not claimed.  Shared by both entry points:
 *   d_cube [n_chan][n_pix]    float64 channel planes (READ ONLY): the memory of a (F, nx, nz)
 *                             stack; 8-byte alignment suffices (an odd n_pix puts every other
 *                             plane 8 bytes off a 16-byte boundary)
 *   h_x [n_chan]              HOST, the spectral axis: finite, any unit, any order, need not be
 *                             uniform;  x_ref: a finite origin (the mid-channel, say)
 *   n_chan                    1 .. RJP_SPECFIT_MAX_CHAN
 *   d_mask [n_pix]            (optional) uint8, non-zero = the pixel is live; a masked pixel is a
 *                             pixel without counted channels
 * One lane per pixel walks the channels in ascending order; every sum is a chain in channel order
 * (from +0.0), no atomics, no cross-lane reduction, no workspace: the bits of a pixel's outputs are
 * a function of its spectrum and the tables alone -- not of n_pix, of where the pixel lies or of its
 * neighbours -- and the same on every call.
 * BOTH RETURN the number of workgroups enqueued, ceil(n_pix / 64) > 0, or a negative RJP_ERR_*.
 * Everything is validated before anything is enqueued, and no output byte is touched on a refusal.
 *
 * rjp_cube_moments.  h_dx [n_chan] HOST, finite and >= 0: the channel widths; clip finite, >= 0.
 * Channel c of pixel p counts when y = d_cube[c][p] is finite and |y| >= clip.  Pass 1 over the
 * counted channels:
 *   m0 = fma(y, dx_c, m0);  s1 = fma(y * dx_c, x_c - x_ref, s1);  the count;
 *   the peak = the largest y, on a tie the lowest channel (y > peak, from -inf), ipeak its channel
 * then m1 = x_ref + s1 / m0, and pass 2 (same launch, same lane, same channels):
 *   s2 = fma(y * dx_c, (x_c - m1) * (x_c - m1), s2);  m2 = sqrt(s2 / m0), NaN for s2 / m0 < 0
 *   (emission and absorption mixed).
 * No counted channel (a masked pixel included) or m0 == 0: m0 = +0.0, m1 = m2 = peak = NaN,
 * ipeak = -1.
 *   d_mom [4][n_pix]          m0, m1, m2, peak
 *   d_ipeak, d_count [n_pix]  int32, either may be NULL
 * RJP_ERR_ARG for a NULL ctx, d_cube, h_x, h_dx or d_mom; n_pix or n_chan < 1; n_chan above the
 * limit; a non-finite h_x; an h_dx that is negative or not finite; a non-finite x_ref; a clip that
 * is negative or not finite; more than 2^31 - 1 workgroups.
 *
 * rjp_specfit.  Per pixel, n_comp Gaussians plus a linear baseline,
 *   y(x) = sum_c A_c exp(-(x - x0_c)^2 / (2 s_c^2)) + b0 + b1 (x - x_ref),
 * P = 3 n_comp + 2 parameters, theta = (A_0, x0_0, s_0, [A_1, x0_1, s_1,] b0, b1).  Per counted
 * channel and component, in float64:
 *   d = x_c - x0;  z = d / s (the one division of a channel);  e = -0.5 * (z * z)
 *   E = exp(e) to < 1e-14 relative, an exact 0 for e < -700;  the component is A * E
 *   model = the components added in order, then + fma(b1, x_c - x_ref, b0)
 *   Jacobian: dA = E;  dx0 = ((A * E) * z) * r, r = 1 / s rounded once per trial;
 *             ds = dx0 * z;  db0 = 1;  db1 = x_c - x_ref
 *   h_w [n_chan]              HOST weights (1 / sigma_c^2; 0 = ignore the channel), finite and
 *                             >= 0; NULL = all ones
 *   n_comp                    1 .. RJP_SPECFIT_MAX_COMP
 *   h_free [P]                HOST uint8, non-zero = the parameter is fitted; one pattern for all
 *                             pixels; NULL = all free; at least one must be free.  b0 = b1 = 0
 *                             held: the fit of a continuum-subtracted cube
 *   d_theta [P][n_pix]        parameter planes: the start on entry, the fit on exit (IN PLACE)
 *   lambda0, xtol             finite and > 0;  n_iter >= 1
 *   d_chi2 [n_pix], d_cov [P (P + 1) / 2][n_pix], d_nchan, d_niter, d_status [n_pix] (int32)
 *   d_trace [n_pix][n_iter][3 + P]   (optional) per iteration (chi^2 of the trial, the lambda that
 *                             proposed it, accepted 0 / 1, the trial's P parameters); rows at and
 *                             beyond d_niter[p] are not written
 * Channel c counts when y is finite and w_c > 0.  With r = y - model over the counted channels,
 *   chi^2 = sum w r^2,  N = J^T W J,  g = J^T W r,
 * accumulated per channel as fma(w * r, r, .), fma(w * J_i, J_j, .) (i <= j) and fma(w * J_i, r, .).
 * A fixed parameter keeps its start value: its row and column of N are replaced by the identity's
 * and its g by 0, so that its step is exactly 0.
 * The iteration is rjp_uvfit's (K20), word for word: iteration t = 1, 2, ... evaluates one trial
 * (the first: the start, with chi^2_cur = +inf) and decides, in this order:
 *   1. accept iff every s_c of the trial is finite and > 0, its chi^2 is finite and < chi^2_cur; on
 *      accept theta_cur, chi^2_cur, N, g become the trial's and lambda <- max(lambda / 10, 1e-12)
 *      (accepting the start leaves lambda0); on reject lambda <- 10 lambda;
 *   2. chi^2_cur = 0 -> status 1.  Else delta from (N + lambda diag N) delta = g by a P x P
 *      Cholesky; a pivot that is not > 0 counts as a reject (lambda <- 10 lambda, again);
 *      lambda > 1e12 -> status 2 (stalled);
 *   3. max_i |delta_i| / s_i <= xtol, s = (max(|A|, 1e-300), max(s, 1e-300), max(s, 1e-300)) per
 *      component and max(|b0|, 1e-300), max(|b1|, 1e-300), at theta_cur -> status 1 (converged;
 *      tested on every proposed step); n_iter trials done -> status 0; else the next trial is
 *      theta_cur + delta.
 * status 3 (degenerate): a masked pixel, a start that is not finite or has an s_c <= 0, a first
 * chi^2 that is not finite, or fewer counted channels than free parameters; d_status[p] = 3 and
 * NOTHING else of that pixel is written.  Otherwise d_theta / d_chi2 are theta_cur / chi^2_cur,
 * d_cov the packed upper triangle (row by row) of N at theta_cur with the identity's rows for fixed
 * parameters, NOT inverted, d_nchan the counted channels, d_niter the trials evaluated.  Calling
 * again with the returned d_theta continues the fit (lambda starts over).
 * The whole fit of a pixel runs in ONE launch: a lane re-reads its spectrum once per trial, keeps
 * chi^2, N and g in registers, and idles once finished; a wave leaves with its last lane.
 * RJP_ERR_ARG for a NULL ctx, d_cube, h_x, d_theta, d_chi2, d_cov, d_nchan, d_niter or d_status;
 * n_pix or n_chan < 1; n_chan above the limit; n_comp outside 1 .. RJP_SPECFIT_MAX_COMP; a
 * non-finite h_x or x_ref; an h_w that is negative or not finite; no free parameter; lambda0 or
 * xtol not finite and positive; n_iter < 1; more than 2^31 - 1 workgroups. */
#define RJP_SPECFIT_MAX_CHAN 4096
#define RJP_SPECFIT_MAX_COMP 2
int64_t rjp_cube_moments(rjp_ctx* ctx, const double* d_cube, int64_t n_pix, int32_t n_chan,
                         const double* h_x, const double* h_dx, double x_ref, double clip,
                         const uint8_t* d_mask, double* d_mom, int32_t* d_ipeak, int32_t* d_count,
                         void* stream);
int64_t rjp_specfit(rjp_ctx* ctx, const double* d_cube, int64_t n_pix, int32_t n_chan,
                    const double* h_x, double x_ref, const double* h_w, const uint8_t* d_mask,
                    int32_t n_comp, const uint8_t* h_free, double* d_theta, double lambda0,
                    double xtol, int32_t n_iter, double* d_chi2, double* d_cov, int32_t* d_nchan,
                    int32_t* d_niter, int32_t* d_status, double* d_trace, void* stream);

/* ---- K22: antenna-based complex gains (corrupt, gaincal, applycal) ------------------------------
 * The one corruption that dominates real centimetre-wave data, and the step that removes it: per
 * antenna and per solution interval a complex gain, D_pq = g_p conj(g_q) M_pq.  (CASA simobserve's
 * `corrupt`, gaincal and applycal; CASA is not at hand: THIS COMMENT IS THE DEFINITION, no parity
 * is claimed.)
 *
 * Layouts.  Visibilities [n_maps][n_t][n_bl][2] (Re, Im) as rjp_vis writes them for the n_t n_bl
 * points of rjp_uv_tracks: n_bl = n_ant (n_ant - 1) / 2 pairs (p < q), p-major ((0,1), (0,2), ...,
 * (1,2), ...).  Gains [g_maps][n_sol][n_ant][2].  h_sol [n_t] (HOST, int32): the solution interval
 * of every integration, h_sol[0] = 0, rising in steps of 0 or 1, n_sol = h_sol[n_t - 1] + 1 -- every
 * interval is a non-empty contiguous range of integrations.  2 <= n_ant <= RJP_GAINCAL_MAX_ANT.
 *
 * rjp_gain_apply.  One launch, one thread per visibility, no atomics.  With g_p = (pr, pi), g_q =
 * (qr, qi) of the visibility's interval (map 0's when g_maps = 1) and V = (vr, vi):
 *   cr = fma(pr, qr, pi qi)       ci = fma(pi, qr, -(pr qi))                  (c = g_p conj g_q)
 *   mode 0 (corrupt)   out = (fma(cr, vr, -(ci vi)), fma(cr, vi, ci vr))      (c V)
 *   mode 1 (correct)   n2 = fma(cr, cr, ci ci)
 *                      out = (fma(vr, cr, vi ci) / n2, fma(vi, cr, -(vr ci)) / n2)   (V conj c / |c|^2)
 * d_out may be d_vis.  A NaN gain or a NaN visibility gives a NaN visibility: the flag that
 * rjp_vis_adjoint, rjp_uv_weights and rjp_uvfit honour.  Returns the workgroups of its launch.
 *
 * rjp_gaincal.  StefCal (Salvini & Wijnholds 2014) for every (map m, interval s) at once.
 *   d_model [model_maps][n_t][n_bl][2], model_maps 1 or n_maps; d_w NULL (all ones) or
 *   [w_maps][n_t][n_bl], w_maps 1 or n_maps; d_gains [n_maps][n_sol][n_ant][2] IN PLACE.
 * A visibility (m, t, pq) COUNTS when Re D, Im D, Re M, Im M and w are finite, w > 0 and
 * m2 = fma(Mr, Mr, Mi Mi) > 0.
 * 1. Accumulate (the pass over the data).  Per (m, s, pq), over the counting integrations of the
 *    interval in ascending t, from 0:
 *      Ar = fma(w, fma(Dr, Mr, Di Mi), Ar)   Ai = fma(w, fma(Di, Mr, -(Dr Mi)), Ai)   (w D conj M)
 *      B  = fma(w, m2, B)                    n_pq += 1
 *    and A_qp = conj(A_pq), B_qp = B_pq.  They go to the workspace: [n_maps n_sol][3][n_bl]
 *    doubles (Re A, Im A, B), then [n_maps n_sol][n_ant][2] doubles (the start gains of the
 *    solutions that were solved), then [n_maps n_sol][n_bl] int32 (n_pq).
 * 2. Live antennas.  All antennas start live.  In a sweep every live antenna p counts its partners
 *    q != p that are live and have B_pq > 0, by the flags as they stood BEFORE the sweep; all with
 *    fewer than min_bl leave together; sweeps repeat until one removes nothing.  (The set is the
 *    largest one in which every member has min_bl such partners; no other order reaches another.)
 *    Fewer than 3 live antennas (mode 0, amplitude and phase) or 2 (mode 1, phase only), or a live
 *    antenna whose start gain is not finite or is (0, 0): status 3 -- every gain of that solution
 *    becomes NaN, d_nvis and d_status are written, NOTHING else of that solution is.
 * 3. Iterate.  For k = 1, 2, ... and every live p, over the live q != p in ascending q as FOUR
 *    chains, q mod 4 = 0, 1, 2, 3, each from 0, combined (c0 + c1) + (c2 + c3) -- an order that
 *    depends on n_ant and the live set alone.  With A_pq = (ar, ai), g_q = (qr, qi):
 *      nr = fma(qr, ar, nr); nr = fma(-qi, ai, nr); ni = fma(qr, ai, ni); ni = fma(qi, ar, ni)
 *      mode 0:  dn = fma(fma(qr, qr, qi qi), B_pq, dn)
 *      div = dn (mode 0) or sqrt(fma(nr, nr, ni ni)) (mode 1);   h = (nr / div, ni / div)
 *      g' = h for odd k, (0.5 (hr + gr), 0.5 (hi + gi)) for even k.
 *    A div that is not finite and > 0, or an h that is not finite, at any live antenna: status 2,
 *    the gains stay at g, d_niter = k - 1.  Else g <- g', d_niter = k, and with |z| =
 *    sqrt(fma(zr, zr, zi zi)): max_p |g'_p - g_p| <= tol max_p |g'_p| gives status 1; k = n_iter
 *    gives status 0.  A second call continues from the gains of the first (k starts over).
 * 4. Reference antenna.  r = refant if it is live, else the lowest live antenna; a = |g_r|,
 *    (cr, ci) = (gr_r / a, -(gi_r / a)); every live gain becomes (fma(gr, cr, -(gi ci)), fma(gr, ci,
 *    gi cr)), Im g_r exactly +0.0; dead antennas get NaN.
 * 5. Residual.  d_chi2[m][s][0 / 1] = sum w |D - c M|^2 over the counting visibilities of the
 *    pairs with both antennas live, c = g_p conj g_q (cr, ci as in rjp_gain_apply) of the start
 *    gains (0) and of the gains as written (1).  Lane l of 256 takes the pairs pq = l, l + 256, ...
 *    in ascending order and of each the interval's integrations in ascending t, ONE chain from 0:
 *      er = Dr - fma(cr, Mr, -(ci Mi));  ei = Di - fma(cr, Mi, ci Mr)
 *      x = fma(w er, er, x);  x = fma(w ei, ei, x)
 *    then the 256 partials are folded by halves: x[l] += x[l + h] for h = 128, 64, ..., 1.
 * Outputs: d_nvis (the sum of n_pq over ALL pairs), d_niter, d_status [n_maps][n_sol] int32;
 * d_live [n_maps][n_sol][n_ant] uint8; optional d_trace [n_maps][n_sol][n_iter][n_ant][2]: the
 * gains after each step BEFORE referencing (NaN for a dead antenna); rows at and beyond d_niter are
 * not written.  No atomics, every sum in the order stated: a repeated call gives identical bits,
 * and the bits of a solution depend on its own interval's data alone, not on what else is in the
 * call.  Three launches (accumulate; one wave per (m, s), one lane per antenna, the triangle of
 * A and B in LDS and the whole iteration in one launch; residual), nothing on the host.
 * RJP_GAINCAL_MAX_ANT = 64: a triangle of 2016 x 24 B = 48 KiB fits static LDS.
 * Both return the workgroups they enqueued.  Everything is validated before anything is enqueued;
 * a refusal touches no output and no workspace byte.  RJP_ERR_ARG for a NULL ctx, d_vis, d_gains,
 * h_sol, d_out / d_model, d_chi2, d_nvis, d_niter, d_status, d_live; n_maps, n_t or n_sol < 1;
 * n_ant < 2 or above the cap; a malformed h_sol; g_maps / model_maps / w_maps neither 1 nor
 * n_maps; a mode other than 0 and 1; refant outside 0 .. n_ant - 1; min_bl < 1; tol not finite and
 * positive; n_iter < 1; more than 2^31 - 1 workgroups.  RJP_ERR_WORKSPACE for a d_work that is NULL
 * or smaller than rjp_gaincal_workspace() (0 for arguments it would refuse). */
#define RJP_GAINCAL_MAX_ANT 64
int64_t rjp_gain_apply(rjp_ctx* ctx, const double* d_vis, int32_t n_maps, int32_t n_t,
                       int32_t n_ant, const double* d_gains, int32_t g_maps, const int32_t* h_sol,
                       int32_t n_sol, int32_t mode, double* d_out, void* stream);
size_t rjp_gaincal_workspace(int32_t n_maps, int32_t n_sol, int32_t n_ant);
int64_t rjp_gaincal(rjp_ctx* ctx, const double* d_vis, int32_t n_maps, int32_t n_t, int32_t n_ant,
                    const double* d_model, int32_t model_maps, const double* d_w, int32_t w_maps,
                    const int32_t* h_sol, int32_t n_sol, int32_t mode, int32_t refant,
                    int32_t min_bl, double tol, int32_t n_iter, double* d_gains, double* d_chi2,
                    int32_t* d_nvis, int32_t* d_niter, int32_t* d_status, uint8_t* d_live,
                    double* d_trace, void* d_work, size_t work_bytes, void* stream);

/* ---- K23: normal equations from data, model and derivative stacks ---------------------------------
 * The reduction a least-squares fit of the MODEL'S OWN parameters needs: data, model and the
 * model's derivatives are stacks on the device (light curves and their Jacobian from
 * rjp_ff_grad / rjp_ff_formal_grad, visibilities from rjp_vis on flux and derivative maps); this
 * entry point reduces them to chi^2, the gradient and the Gauss-Newton matrix.  This comment IS
 * the definition.
 *   n_part                    2: complex samples stored (re, im) as rjp_vis writes them; 1: real
 *                             samples (a light curve, with n_vis = 1: d_ftot / d_dftot as they are)
 *   d_data, d_model           [n_rows][n_vis][n_part]   (READ ONLY)
 *   d_dmodel                  [n_rows][n_par][n_vis][n_part]: plane j of a row is d model / d theta_j
 *   h_sel [n_sel]             HOST, distinct indices in [0, n_par): the planes that take part, in
 *                             the order of the outputs; a plane that is not named is never read.
 *                             n_sel = 0: chi^2 and the count only (d_dmodel and h_sel may be NULL)
 *   d_w                       NULL (all ones) or [w_rows][n_vis], w_rows 1 (shared) or n_rows
 *   d_out [1 + P + P (P + 1) / 2], P = n_sel: chi^2, then g[P], then the packed upper triangle of N
 *                             row by row (the order of rjp_uvfit's d_cov);  d_count: one int64
 *   d_work                    8-byte aligned, like every double buffer
 * Sample (row, k) counts when every part of its datum and its weight are finite and w > 0.  With
 * r = data - model (one rounding per part) and J_p the selected plane p, over the counting samples
 *   chi^2 = sum w |r|^2,   g_p = sum w Re(conj(J_p) r),   N_pq = sum w Re(conj(J_p) J_q),
 * *d_count their number.  A sample that does not count adds nothing, whatever its model or
 * derivatives hold; a counting sample with a non-finite model or derivative propagates by IEEE
 * rules (into the entries that touch it, and no others).
 * The order of every sum.  With column P standing for r, every entry is G[p][q], p <= q <= P.  A
 * tile is 512 consecutive flattened samples s = row n_vis + k; sample i of a tile belongs to slice
 * i mod 16.  A slice starts at +0 and takes its counting samples in increasing i, part 0 then part
 * 1, each as one fused multiply-add G[p][q] <- fma(a_p, w a_q, G[p][q]) with w a_q rounded once
 * (the weight on the column with the higher index).  The 16 slices are added in slice order, ((s0 +
 * s1) + s2) + ..., into the tile's partial; a second launch adds the partials in tile order,
 * starting from tile 0's.  No atomics: a repeated call gives the same bits, and the value of a sum
 * depends on the inputs and these two constants, not on n_sel, n_par or the device.
 * RETURNS the workgroups of the first launch, ceil(n_rows n_vis / 512) > 0, or a negative
 * RJP_ERR_*.  Everything is validated before anything is enqueued, and no output or workspace byte
 * is touched on a refusal: RJP_ERR_ARG for a NULL ctx, d_data, d_model, d_out or d_count; n_rows or
 * n_vis < 1; n_part not 1 or 2; n_sel outside 0 .. RJP_NORMAL_EQ_MAX_SEL; n_sel > 0 with a NULL
 * d_dmodel or h_sel; n_par < n_sel; an index outside [0, n_par); a repeated index; with d_w a w_rows
 * that is neither 1 nor n_rows; more than 2^31 - 1 workgroups.  RJP_ERR_WORKSPACE for a d_work that
 * is NULL or smaller than the workspace query (n_tiles x (1 + P + P (P + 1) / 2 + 1) x 8 bytes; 0
 * from it = a bad argument). */
#define RJP_NORMAL_EQ_MAX_SEL 48          /* 3 x (8 + 8) bursts: what K9 allows */
size_t rjp_normal_eq_workspace(int64_t n_rows, int32_t n_vis, int32_t n_sel);
int64_t rjp_normal_eq(rjp_ctx* ctx, const double* d_data, const double* d_model,
                      const double* d_dmodel, int64_t n_rows, int32_t n_vis, int32_t n_part,
                      int32_t n_par, const int32_t* h_sel, int32_t n_sel, const double* d_w,
                      int64_t w_rows, double* d_out, int64_t* d_count, void* d_work,
                      size_t work_bytes, void* stream);

/* ---- K24: per-sightline Voigt fits of a line cube ---------------------------------------------------
 * rjp_specfit (K21) fits Gaussians; the model's own lines (K3, K6) are Voigt profiles, a thermal
 * Doppler core with pressure-broadened Lorentz wings, and an observer wants T from the Doppler width
 * and n_e from the Lorentz width.  CASA is not at hand, so this comment IS the definition; parity is
 * not claimed.
 *
 * rjp_voigtfit.  Per pixel, n_comp area-normalised Voigt components plus a linear baseline,
 *   y(x) = sum_c F_c K(u_c, a_c) / (s_c sqrt(2 pi)) + b0 + b1 (x - x_ref),
 *   q_c = 1 / (sqrt(2) s_c),  u_c = (x - x0_c) q_c,  a_c = g_c q_c,  K + i L = w(u + i a),
 * w the Faddeeva function exp(-z^2) erfc(-i z).  P = 4 n_comp + 2 parameters,
 * theta = (F_0, x0_0, s_0, g_0, [F_1, x0_1, s_1, g_1,] b0, b1): s the Doppler dispersion, g the
 * Lorentz HWHM, both in the unit of the axis, F the component's integral over x (the area, not
 * K21's peak: in the Lorentz limit only peak x s is determined, the area stays well conditioned).
 * The derivatives are exact, from w' = -2 z w + 2 i / sqrt(pi).  Per trial and component, in float64:
 *   rs = 1 / s (the one reciprocal);  q = rs * 0.70710678118654752440;  a = g * q;
 *   cn = rs * 0.39894228040143267794
 * and per counted channel and component:
 *   u = (x_c - x0) * q;  (K, L) = w(u + i a) to |w_dev - w| <= 2.0e-15 |w| (both parts against the
 *       modulus; a = 0 included)
 *   Rw = -2 * fma(u, K, -(a * L));  Iw = fma(-2, fma(u, L, a * K), 2 / sqrt(pi))
 *   c = F * cn;  cq = c * q;  the component is c * K
 *   model = the components added in order, then + fma(b1, x_c - x_ref, b0)
 *   Jacobian: dF = K * cn;  dx0 = -(cq * Rw);  ds = -(c * rs) * fma(-a, Iw, fma(u, Rw, K));
 *             dg = -(cq * Iw);  db0 = 1;  db1 = x_c - x_ref
 * Everything else is rjp_specfit's, word for word (see there, and lm_common.h's iteration): d_cube,
 * h_x, x_ref, h_w, d_mask; the counted channels (y finite and w_c > 0); chi^2, N, g as fma chains in
 * channel order with the weight on the left factor, fma(w * r, r, .), fma(w * J_i, J_j, .) (i <= j),
 * fma(w * J_i, r, .); the fixed-parameter rule and h_free [P] (g held at 0: a Gaussian fit in area
 * form; s held at a known thermal width); the iteration and the statuses 0 - 3; d_theta [P][n_pix]
 * IN PLACE, d_chi2, d_cov [P (P + 1) / 2][n_pix] packed and NOT inverted, d_nchan, d_niter,
 * d_status, the optional d_trace [n_pix][n_iter][3 + P]; the whole fit of a pixel in ONE launch, one
 * lane per pixel, the bits of a pixel a function of its spectrum and the tables alone.  It differs in:
 *   feasible    every s_c finite and > 0 AND every g_c finite and >= 0 (a trial with a g < 0 is
 *               rejected)
 *   the scales  per component max(|F|, 1e-300) for F and max(s, g, 1e-300) for x0, s and g; max(|b0|,
 *               1e-300), max(|b1|, 1e-300)
 *   status 3    also for a start with a g_c < 0
 *   n_comp      1 .. RJP_VOIGTFIT_MAX_COMP; n_chan 1 .. RJP_SPECFIT_MAX_CHAN
 * RETURNS ceil(n_pix / 64) > 0 or a negative RJP_ERR_*; nothing is written on a refusal.
 * RJP_ERR_ARG: rjp_specfit's list with these limits. */
#define RJP_VOIGTFIT_MAX_COMP 2
int64_t rjp_voigtfit(rjp_ctx* ctx, const double* d_cube, int64_t n_pix, int32_t n_chan,
                     const double* h_x, double x_ref, const double* h_w, const uint8_t* d_mask,
                     int32_t n_comp, const uint8_t* h_free, double* d_theta, double lambda0,
                     double xtol, int32_t n_iter, double* d_chi2, double* d_cov, int32_t* d_nchan,
                     int32_t* d_niter, int32_t* d_status, double* d_trace, void* stream);

/* ---- K25: robust image statistics, connected components, constrained growth of a mask -------------
 * What an automatic clean mask (tclean's usemask = 'auto-multithresh') is made of, on stacks that are
 * already on the device.  Integer and order-statistic work: every output but two sums is a function
 * of the inputs alone, the same bits on every call.  CASA is not at hand, so this comment IS the
 * definition; parity is not claimed.
 * Common to the three: images and masks in the pixel order p = ix nz + iz (K12's); masks are uint8,
 * non-zero = set; n_mask is 1 (one mask for all maps) or n_maps, as n_psf is in K12; n_maps 1 ..
 * RJP_REGIONS_MAX_MAPS, nx 1 .. RJP_REGIONS_MAX_NX, nz >= 1, nx nz <= 2^31 - 1; d_work 8-byte
 * aligned.  No floating-point atomics anywhere; workgroups meet only in integer atomics and at launch
 * boundaries.  Everything is validated before anything is enqueued, and no output or workspace byte
 * is touched on a refusal: RJP_ERR_ARG for a NULL ctx or a NULL required pointer, sizes outside the
 * ranges above, an n_mask that is neither 1 nor n_maps, and what each call adds below;
 * RJP_ERR_WORKSPACE for a d_work that is NULL, smaller than the call's workspace query (0 from a
 * query = a bad argument) or not 8-byte aligned.
 *
 * rjp_image_stats.  Per map m, over its COUNTING pixels: pixel p counts when d_img[m][p] is finite
 * and, with a d_mask, (mask[p] != 0) == (sense != 0) -- sense 1 measures inside the mask, 0 outside
 * it; d_mask NULL: every finite pixel (n_mask and sense are then ignored).
 *   d_stats [n_maps][8]: count; n_nonfinite (the pixels the mask selects that are NaN or +-inf);
 *                        min; max; median; mad; sum; sumsq
 *   order      ascending IEEE total order on the finite values: numerical order, with -0.0 < +0.0
 *   median     the LOWER median: the element of rank (count - 1) / 2 (integer division, rank 0 the
 *              smallest).  No two values are averaged: it is an element of the input, no rounding.
 *   mad        the element of the same rank of fabs(x - median), one rounding per pixel (an
 *              overflowing difference is +inf and sorts last), formed on the fly from the median that
 *              the first stage left in d_stats: no host round trip, no temporary image.
 *   min, max   by the same order (so min of {-0.0, +0.0} is -0.0)
 *   count = 0  median = mad = min = max = NaN, sum = sumsq = +0.0
 *   sum, sumsq in a fixed order.  A tile is 2048 consecutive pixels of the map.  Lane t (0 .. 255) of
 *              a tile starts at +0 and takes the tile's counting pixels t, t + 256, t + 512, ... in
 *              that order, s <- s + x and q <- fma(x, x, q); the 256 lane values are folded by
 *              halving, v[t] <- v[t] + v[t + h] for h = 128, 64, ..., 1; the tiles are added in tile
 *              order starting from tile 0's value.
 * The selection is an exact radix select on the order-preserving 64-bit key of the double, six digits
 * of 11, 11, 11, 11, 11 and 9 bits from the top: per digit every workgroup counts its pixels in a
 * histogram in LDS and adds it to the map's histogram in the workspace (integer atomics both), then
 * one workgroup per map picks the bin that holds the rank.  26 launches, no host synchronisation.
 * RETURNS n_maps x ceil(nx nz / 2048) > 0 or a negative RJP_ERR_*.
 *
 * rjp_label_regions.  The connected components of the non-zero pixels of d_mask_in [n_mask][nx nz];
 * connectivity 1: the four edge neighbours, 2: the eight edge and corner neighbours (else
 * RJP_ERR_ARG).
 *   d_label [n_maps][nx nz] int32: 0 on background, otherwise 1 + the smallest pixel index p of the
 *                           pixel's region -- a function of the input alone, whatever order the
 *                           merges happen in
 *   d_area  [n_maps][nx nz] int32 or NULL: the pixel count of the region on each of its pixels, 0 on
 *                           background
 *   d_nreg  [n_maps] int32: the number of regions
 * Union-find per tile of 16 x 64 pixels in LDS, a merge of the tile borders in global memory with
 * atomic minima on the parents, a flatten pass, an area pass (an integer atomic add at the root, then
 * a gather).  Parents only ever decrease and are bounded below by 0, which ends every loop that
 * follows parents or retries a union; each such loop is also capped at nx nz iterations and, when a
 * cap is hit, sets the first int32 of d_work (0 otherwise; cleared by every call) instead of
 * spinning: the caller reads that word after the call and treats non-zero as an error.
 * RETURNS n_maps x ceil(nx / 16) x ceil(nz / 64) > 0 or a negative RJP_ERR_*.
 *
 * rjp_mask_grow.  Geodesic dilation IN PLACE on d_seed [n_maps][nx nz] under d_con [n_mask][nx nz].
 * One step is seed <- seed OR (dilate(seed) AND con), dilate by the neighbours of `connectivity`, the
 * outside of the image unset: scipy.ndimage.binary_dilation(seed, structure, iterations = n_iter,
 * mask = con).  A seed pixel outside the constraint stays.
 *   n_iter = 0   nothing is done: d_seed keeps its bytes
 *   n_iter > 0   exactly n_iter steps, ceil(n_iter / RJP_GROW_HALO) launches: a tile with a halo of
 *                RJP_GROW_HALO pixels is staged in LDS and advanced that many steps per launch, the
 *                last launch the remainder; the launches alternate between d_seed and a plane of the
 *                workspace.  On return every pixel of d_seed is 0 or 1.
 *   n_iter < 0   until stable (morphological reconstruction), not a loop of launches: d_con is
 *                labelled as by rjp_label_regions; a region is kept when one of its pixels is a seed
 *                or a neighbour of a seed (an integer flag at the root); d_seed <- 1 on the kept
 *                regions, its other bytes as they were.  A d_con that all maps share (n_mask =
 *                1) is labelled once.  The cap flag as above.
 * RETURNS n_maps x ceil(nx / 16) x ceil(nz / 64) > 0 or a negative RJP_ERR_*; RJP_ERR_ARG also for a
 * connectivity that is neither 1 nor 2. */
#define RJP_REGIONS_MAX_MAPS 65535
#define RJP_REGIONS_MAX_NX 1048560        /* 16 x 65535 */
#define RJP_GROW_HALO 8
size_t rjp_image_stats_workspace(int32_t n_maps, int32_t nx, int32_t nz);
int64_t rjp_image_stats(rjp_ctx* ctx, const double* d_img, int32_t n_maps, int32_t nx, int32_t nz,
                        const uint8_t* d_mask, int32_t n_mask, int32_t sense, double* d_stats,
                        void* d_work, size_t work_bytes, void* stream);
size_t rjp_label_regions_workspace(int32_t n_maps, int32_t nx, int32_t nz);
int64_t rjp_label_regions(rjp_ctx* ctx, const uint8_t* d_mask_in, int32_t n_mask, int32_t n_maps,
                          int32_t nx, int32_t nz, int32_t connectivity, int32_t* d_label,
                          int32_t* d_area, int32_t* d_nreg, void* d_work, size_t work_bytes,
                          void* stream);
size_t rjp_mask_grow_workspace(int32_t n_maps, int32_t nx, int32_t nz);
int64_t rjp_mask_grow(rjp_ctx* ctx, uint8_t* d_seed, const uint8_t* d_con, int32_t n_mask,
                      int32_t n_maps, int32_t nx, int32_t nz, int32_t n_iter, int32_t connectivity,
                      void* d_work, size_t work_bytes, void* stream);

/* ---- K4: geometry -> fields on the device --------------------------------------------
 * Replaces the lazily cached grids of JetModel (fill_factor/areas classes.py:657-669,
 * 763-764; grid_rwp 521-525; rreff 549-555; _nd 877-897; ion_fraction 915-934;
 * temperature 950-967; ts 847-853 with maths/geometry.py:150-178; vel[1] 1042-1093).
 * Writes the packed device layout directly. */
typedef struct rjp_geometry {
  int32_t nx, ny, nz;
  int32_t rotation_ccw;       /* 1 = "CCW", 0 = "CW" */
  double csize;               /* [au] */
  double inc, pa;             /* [deg] */
  double w_0, r_0, mod_r_0, epsilon;
  double R_1, R_2;            /* [au] */
  double M_star;              /* [Msol] */
  double v_lsr;               /* [km/s] */
  double n_0, x_0, T_0, v_0;  /* axis values at the base */
  double q_n, q_x, q_T, q_v;          /* power laws along r */
  double qd_n, qd_x, qd_T, qd_v;      /* power laws across the jet */
  double rb_frac;             /* mlr_rj / mlr_bj (classes.py:228-229, 895) */
  /* x-slab sharding: build rows [ix0, ix0 + nx) of a grid that is nx_total rows wide
   * (cell x-coordinate = csize * (ix0 + i_x - nx_total / 2)); nx_total = 0 means nx. */
  int32_t ix0, nx_total;
} rjp_geometry;

/* Any output may be NULL to skip it (d_vy / d_ts typically); d_ff_raw / d_areas_raw (float64, optional) receive
 * the un-packed fill factors / areas that JetModel.save pickles (classes.py:1704-1709);
 * d_vx_raw / d_vz_raw (float64, optional) the transverse components of JetModel.vel.
 * Launch times: closed form for q^d_v = 0, otherwise Gauss' 2F1(a, b; b+1; -A) of
 * maths/geometry.py:166-171 evaluated on the device (Pfaff series up to a switch point chosen
 * per model, the 1/z connection formula above it; narrow jets, b ~ 1/epsilon of several hundred,
 * included); RJP_ERR_DEGENERATE if d_ts != NULL and a-b or b is a non-positive integer
 * (logarithmic cases) or a-b is so close to one (about 1e-5 for a-b near -1, 1e-7 near -3) that
 * the connection formula would cancel below 1e-11.
 * RJP_ERR_ARG for epsilon = 0 / mod_r_0 = 0 (the reference's rho = |r|/r_0 branch is not built).
 * d_em0 (optional, RJP_F64 only): the compact scan field of rjp_fields.d_em0 written in the
 * same pass, bit-identical to what rjp_compact_fields derives from nd, xi, pf -- with d_nd,
 * d_xi, d_pf NULL a continuum-only model occupies 24 B/cell (12e9 cells per 288 GB GPU).
 * d_a0 (optional, RJP_F64 only): the tau scan field of rjp_fields.d_a0 for gff mode `a0_mode`,
 * bit-identical to rjp_tau_field's. */
int rjp_build_fields(rjp_ctx* ctx, const rjp_geometry* geom, int dtype,
                     void* d_nd, void* d_xi, void* d_temp, void* d_pf, void* d_ts,
                     void* d_vy, double* d_ff_raw, double* d_areas_raw,
                     double* d_vx_raw, double* d_vz_raw, void* d_em0, void* d_a0,
                     int32_t a0_mode, void* stream);

/* ---- measurement harness: synthetic dense fields ---------------------
 * Counter-based: u = splitmix64(seed ^ field_id<<60 ^ linear_cell_index) -> [0,1).
 *   n = 10^(5+2.5u), x = 0.05+0.45u, T = 1e4 (temp_mode 0) or 5e3+1.5e4u (temp_mode 1),
 *   pf = 0.5 w.p. 0.25 else 1, ts = 5u yr, red = i_z < n_z/2, vy = 6.2+60(u-0.5) km/s.
 * Generates cells [cell0, cell0+n) of the flattened grid so a host restatement can
 * regenerate any sub-block.  Any output may be NULL; d_em0 / d_a0 (optional, RJP_F64 only)
 * receive the compact and tau scan fields of the same cells, as for rjp_build_fields. */
int rjp_synth_fields(rjp_ctx* ctx, uint64_t seed, int32_t temp_mode, int32_t nz,
                     int64_t cell0, int64_t n, int dtype, void* d_nd, void* d_xi,
                     void* d_temp, void* d_pf, void* d_ts, void* d_vy, void* d_em0,
                     void* d_a0, int32_t a0_mode, void* stream);

/* Device-time probe used by bench.py: average duration [ms] of `reps` back-to-back
 * rjp_ff_scan launches measured with HIP events on `stream`. */
int rjp_time_ff_scan(rjp_ctx* ctx, const rjp_fields* fields, const rjp_bursts* bursts,
                     const double* h_epochs_s, int32_t n_epochs, int32_t gff_mode,
                     double* d_sumA, double* d_em, double* d_tavg, void* d_work,
                     size_t work_bytes, void* stream, int32_t reps, double* ms_avg);

#ifdef __cplusplus
}
#endif
#endif /* RJPRT_H */
