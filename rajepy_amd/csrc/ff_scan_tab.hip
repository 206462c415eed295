// K1, single epoch, tau layout: the burst factor from a table in LDS (round 4).
//
// The single-epoch scan of (a0, ts) spends ~42 of its 51 vector instructions per cell on the 2-3
// burst Gaussians of chi(t - ts) (classes.py:442-448, 866-868) and is co-limited by vector-ALU
// issue at a power-limited clock (profiles/r03c_cfg4_k1_tau_sq.json).  chi is a function of ONE
// variable, the time since launch: per call it is tabulated on the interval of times since launch
// that can occur AND matter -- [t - ts_hi, t - ts_lo] cut with the bursts' support (chi == 1 to
// 1e-17 outside) -- as piecewise polynomials of degree 7 in the interval's own coordinate
// xi in [-1, 1), 8 coefficients per interval and jet at a stride of 80 bytes (an odd multiple of
// 16: the four 16-byte reads of a lookup then spread over all LDS bank groups; at 64 bytes they
// fall on a quarter of them), built on the device by a tiny kernel in front of the scan (8
// Chebyshev nodes per interval, inverse Vandermonde matrix on [-1, 1] from the host).  A cell
// costs one interval lookup: four 16-byte LDS reads at a random address + 7 FMAs, whatever the
// number of bursts.  The number of intervals follows from the interpolation bound
//   |chi - p| <= max|chi^(8)| (h/2)^8 / (8! 2^7),   max|G^(8)| = 105 A / sigma^8
// for a Gaussian of amplitude A: h is chosen so that the bound is <= 1e-13 (chi >= 1: bursts with
// a negative amplitude keep the Gaussians), i.e. <= 2e-13 relative on chi^2; a table that would
// not fit 72 KB of LDS (460 intervals per jet; two workgroups per CU) keeps the Gaussians too.
// (Quintics at 48 bytes, the round-3 experiment, need 4.2 x the intervals: the example's bursts
// then fit for few epochs only.)
//
// Launch shape: with ~22 instead of 51 vector instructions per cell the scan no longer needs
// eight y-ranges' worth of waves to hide its ALU work: ONE y-range per sightline chunk on maps
// that fill the chip that way (cfg4: 512 workgroups of 256 threads, two per CU), six rows of
// loads in flight, sums written straight to the map -- no partial sums, no reduction kernel.
// Same-buffer A/B at cfg4 (profiles/r04_k1_table_variants.log): 2.48 ms against 2.64-2.69 ms for
// the Gaussians = 0.865 of the 8 TB/s peak on the 17.18 GB the scan needs.  The sums follow another order than the compact / wide layouts' eight ranges: equal
// to them to rounding (tests: 1e-12), not bit for bit -- the price VERDICT r03 item 5 accepts.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ff_scan_kernels.h"

namespace rjp {

#ifndef RJP_TAB_U
#define RJP_TAB_U 6              /* rows of loads in flight per lane (same-buffer A/B at cfg4, profiles/r04_k1_table_variants.log: 6: 2.483 ms, 8: 2.513, 12: 2.516, 16: 2.529) */
#endif
#ifndef RJP_TAB_U_EM
#define RJP_TAB_U_EM 4           /* ... with the EM map (three streams; 3 / 4 / 6 rows: 3.83 / 3.86 / 3.86 ms -- noise) */
#endif
#ifndef RJP_TAB_U_WIDE
#define RJP_TAB_U_WIDE 4         /* ... from the five model fields (five streams; 2 / 3 / 4 rows: 6.229 / 6.230 / 6.187 ms) */
#endif
#ifndef RJP_TAB_WGS
#define RJP_TAB_WGS 512          /* y-ranges are added until this many workgroups exist (1024 / 2048 at cfg4: 2.518 / 2.524 ms) */
#endif
#ifndef RJP_TAB_GUARD
#define RJP_TAB_GUARD 1          /* 0: a build without the launch-time range guard, for A/B only (2 vector instructions per cell; same-buffer A/B at cfg4: profiles/r05_guard_ab.log) */
#endif
constexpr int kChiNC = 8;                    // coefficients per interval (degree 7)
constexpr int kChiStride = 10;               // doubles between intervals (80 B)
constexpr int kChiMaxNI = 460;               // 2 jets x 460 x 80 B = 73600 B of LDS
constexpr double kChiTol = 1e-13;            // bound on |chi - table|
// a Gaussian of relative amplitude A is below 1e-17 beyond sqrt(2 ln(A 1e17)) sigmas
static double chi_reach(double amp) { return std::sqrt(2.0 * std::log(std::max(amp, 1.0) * 1e17)); }

struct ChiTabDev {
  int ni;
  double lo, inv_h;
  double wmax;     // the largest double below ni: a cell launched exactly at ts_lo (w == ni)
                   // belongs to the last interval, xi -> 1
  // range guard (include/rjprt.h "Launch-time range guard"): the table covers the times since
  // launch of [ts_lo, ts_hi] only and the lookup clamps -- a lane that meets a finite launch time
  // outside the range poisons its sums with NaN and raises the context's flag
  double ts_lo, ts_hi;
  int* guard;
};

// one lane's verdict at the end of its column: `tmin` / `tmax` = fmin / fmax over the launch
// times it read (NaN ignored; an infinite launch time is the reference's chi == 1, not a breach)
__device__ __forceinline__ bool ts_range_breach(const ChiTabDev& t, double tmin, double tmax) {
  return (tmin < t.ts_lo && tmin > -__builtin_inf()) || (tmax > t.ts_hi && tmax < __builtin_inf());
}

// table builder: one thread per (jet, interval); tab[(jet * ni + k) * kChiStride + c]
// stage = [Vandermonde inverse 8 x 8][nodes 8][jet 0: t0.., amp.., inv2s2..][jet 1: ...]
__global__ __launch_bounds__(256) void chi_table_kernel(const double* __restrict__ stage, int nb0,
                                                        int nb1, ChiTabDev t,
                                                        double* __restrict__ tab) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * t.ni) return;
  const int j = i / t.ni, k = i - j * t.ni;
  const int nb = j == 0 ? nb0 : nb1;
  const double* vinv = stage;
  const double* xs = stage + kChiNC * kChiNC;
  const double* bj = stage + kChiNC * kChiNC + kChiNC + (j == 0 ? 0 : 3 * nb0);
  const double h = 1.0 / t.inv_h;
  double f[kChiNC];
  for (int m = 0; m < kChiNC; ++m) {
    const double tl = t.lo + (k + 0.5 * (xs[m] + 1.0)) * h;
    double chi = 1.0;
    for (int b = 0; b < nb; ++b) {
      const double d = tl - bj[b];
      chi += bj[nb + b] * exp(-d * d * bj[2 * nb + b]);
    }
    f[m] = chi;
  }
  for (int c = 0; c < kChiNC; ++c) {
    double s = 0.0;
    for (int m = 0; m < kChiNC; ++m) s += vinv[c * kChiNC + m] * f[m];
    tab[(size_t)i * kChiStride + c] = s;
  }
  tab[(size_t)i * kChiStride + 8] = tab[(size_t)i * kChiStride + 9] = 0.0;
}

// EM: the emission measure of the epoch as well (a third stream, em0: classes.py:1116-1118 with
// number_density = _nd chi); `em_scale` is applied when the sums go straight to the map
template <int U, bool EM>
__global__ __launch_bounds__(kBlock) void ff_scan_table_kernel(
    const double* __restrict__ a0, const double* __restrict__ em0, const double* __restrict__ ts,
    const int32_t* __restrict__ ylo, const int32_t* __restrict__ yhi, int ny, int nz,
    int64_t nchunks, int64_t npix, int ylen, int nsplit, ChiTabDev t, double t_epoch,
    const double* __restrict__ tab, double* __restrict__ out, int64_t out_split_stride,
    double* __restrict__ out_em, double em_scale) {
  constexpr int VEC = 2;
  extern __shared__ __attribute__((aligned(16))) double s_chi[];       // [2][ni][10]
  for (int i = threadIdx.x; i < 2 * t.ni * kChiStride; i += kBlock) s_chi[i] = tab[i];
  const LaneRange lr = lane_y_range<VEC, kBlock>(nsplit, ylen, ny, nchunks, ylo, yhi);
  __syncthreads();                           // the table is staged
  if (!lr.live) return;
  const int split = lr.split, y0 = lr.y0, y1 = lr.y1;
  const int64_t p0 = lr.p0;
  const int64_t x = p0 / nz;
  const int z = (int)(p0 - x * nz);
  const double wmax = t.wmax;
  // chi^2-weighted term of one cell: the jet picks the half of the table, the time since launch
  // the interval; a NaN launch time lands in interval 0 and the term is masked (nansum)
  auto chi2 = [&](double av, double tv) __attribute__((always_inline)) {
    double w = (t_epoch - tv - t.lo) * t.inv_h;
    w = __builtin_fmin(__builtin_fmax(w, 0.0), wmax);
    const double kf = __builtin_floor(w);
    const double xi = __builtin_fma(2.0, w - kf, -1.0);
    const int k = (int)kf + (signbit_d(av) ? 0 : t.ni);
    const rjp_d2* cp = reinterpret_cast<const rjp_d2*>(s_chi + k * kChiStride);
    const rjp_d2 c01 = cp[0], c23 = cp[1], c45 = cp[2], c67 = cp[3];
    double chi = __builtin_fma(c67.y, xi, c67.x);
    chi = __builtin_fma(chi, xi, c45.y);
    chi = __builtin_fma(chi, xi, c45.x);
    chi = __builtin_fma(chi, xi, c23.y);
    chi = __builtin_fma(chi, xi, c23.x);
    chi = __builtin_fma(chi, xi, c01.y);
    chi = __builtin_fma(chi, xi, c01.x);
    return chi * chi;
  };
  double acc[VEC] = {0.0, 0.0}, accE[VEC] = {0.0, 0.0};
  double tmin = __builtin_inf(), tmax = -__builtin_inf();
  int64_t off = (x * ny + y0) * (int64_t)nz + z;
  int y = y0;
  for (; y + U <= y1; y += U) {
    double a[U][VEC], g[U][VEC], tt[U][VEC];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      load_vec(a0 + off + (int64_t)u * nz, a[u]);
      if (EM) load_vec(em0 + off + (int64_t)u * nz, g[u]);
      load_vec(ts + off + (int64_t)u * nz, tt[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const double c2 = chi2(a[u][v], tt[u][v]);
        if (RJP_TAB_GUARD) {
          tmin = __builtin_fmin(tmin, tt[u][v]);
          tmax = __builtin_fmax(tmax, tt[u][v]);
        }
        acc[v] = __builtin_fma(keep_if_ordered(__builtin_fabs(a[u][v]), tt[u][v]), c2, acc[v]);
        if (EM) accE[v] = __builtin_fma(keep_if_ordered(__builtin_fabs(g[u][v]), tt[u][v]), c2, accE[v]);
      }
    off += (int64_t)U * nz;
  }
  for (; y < y1; ++y) {
    double a[VEC], g[VEC], tt[VEC];
    load_vec(a0 + off, a);
    if (EM) load_vec(em0 + off, g);
    load_vec(ts + off, tt);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const double c2 = chi2(a[v], tt[v]);
      if (RJP_TAB_GUARD) {
        tmin = __builtin_fmin(tmin, tt[v]);
        tmax = __builtin_fmax(tmax, tt[v]);
      }
      acc[v] = __builtin_fma(keep_if_ordered(__builtin_fabs(a[v]), tt[v]), c2, acc[v]);
      if (EM) accE[v] = __builtin_fma(keep_if_ordered(__builtin_fabs(g[v]), tt[v]), c2, accE[v]);
    }
    off += nz;
  }
  if (ts_range_breach(t, tmin, tmax)) {
    *t.guard = 1;
#pragma unroll
    for (int v = 0; v < VEC; ++v) { acc[v] = __builtin_nan(""); accE[v] = __builtin_nan(""); }
  }
  double* w = out + (int64_t)split * out_split_stride + p0;
#pragma unroll
  for (int v = 0; v < VEC; ++v) w[v] = acc[v];
  if (EM) {
    // straight to the map (scaled) with one y-range, else plane 1 of this range's partial sums
    double* we = nsplit == 1 ? out_em + p0 : out + (int64_t)split * out_split_stride + npix + p0;
#pragma unroll
    for (int v = 0; v < VEC; ++v) we[v] = nsplit == 1 ? accE[v] * em_scale : accE[v];
  }
}

// The same scan on the launch-time-bucketed layout (rjp_fields.d_srt_*, built by ff_lt.hip): one
// wave per group of 64 sightlines.  Outside a jet's bursts' support chi == 1 (to 1e-17), so per jet
// only the bins [b0, b1) that meet the support at this epoch are read -- in every lane one run of
// rows, [start(b0), start(b1)) -- and the |a0| sums of the other bins (prefix sums kept with the
// layout) stand for the rest.  The wave streams the rows from the smallest start to the largest
// end over its lanes, a lane loading (and summing) the rows of its own run only; lanes are padded
// at their end only, so the runs of a group line up to the Poisson noise of the counts.  The cells in the layout
// are finite and non-zero with a finite launch time inside [ts_lo, ts_hi] (the build checked the
// range); the dropped ones come back through aux as in the launch-time-ordered sweep: a NaN launch
// time counts with chi = 1 when its jet has no bursts (what rjp_unmask_launch_times gives the
// grid-order scan), an infinite weight makes the sightline +inf.
#ifndef RJP_SRT_U
#define RJP_SRT_U 8              /* rows of 16-byte loads in flight per lane */
#endif
#ifndef RJP_SRT_DIAG
#define RJP_SRT_DIAG 1           /* 0: a build whose hybrid scan keeps no bin counters (rjp_last_srt_bins then reads stale slots), for A/B only */
#endif
#ifndef RJP_SRT_OWNROWS
#define RJP_SRT_OWNROWS 1        /* 0: a build in which every lane loads every row of its wave's window, for A/B only */
#endif
constexpr int kSrtBlock = 512;   // 8 groups per workgroup: 512 workgroups at cfg4, one round
struct SrtDev {
  const rjp_d2* cells;
  const int32_t* start;
  const double* cum;
  const int64_t* rowbase;
  const double* aux;
  int64_t npix;
  int K;
  int b0[2], b1[2], hb[2];
};

template <int U>
__global__ __launch_bounds__(kSrtBlock) void ff_scan_sorted_kernel(SrtDev s, ChiTabDev t,
                                                                   double t_epoch,
                                                                   const double* __restrict__ tab,
                                                                   double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double s_chi[];       // [2][ni][10]
  for (int i = threadIdx.x; i < 2 * t.ni * kChiStride; i += kSrtBlock) s_chi[i] = tab[i];
  __syncthreads();
  const int lane = threadIdx.x & (RJP_WAVE - 1);
  const int64_t g = (int64_t)blockIdx.x * (kSrtBlock / RJP_WAVE) + threadIdx.x / RJP_WAVE;
  const int64_t npix = s.npix;
  if (g * RJP_WAVE >= npix) return;                    // (whole waves)
  const int64_t p = g * RJP_WAVE + lane;
  const bool live = p < npix;
  const rjp_d2* base = s.cells + s.rowbase[g] * RJP_WAVE + lane;
  const double wmax = t.wmax;
  double total = 0.0;
#pragma unroll 1
  for (int j = 0; j < 2; ++j) {
    const int q0 = j * s.K, b0 = s.b0[j], b1 = s.b1[j];
    int rs = 0, re = 0;
    double skipped = 0.0;
    if (live) {
      const double* c = s.cum + p;
      if (b0 < b1) {
        skipped = (c[(int64_t)(q0 + s.K) * npix] - c[(int64_t)(q0 + b1) * npix]) +
                  (c[(int64_t)(q0 + b0) * npix] - c[(int64_t)q0 * npix]);
        rs = s.start[(int64_t)(q0 + b0) * npix + p];
        re = s.start[(int64_t)(q0 + b1) * npix + p];
      } else {
        skipped = c[(int64_t)(q0 + s.K) * npix] - c[(int64_t)q0 * npix];
      }
    }
    // the wave's rows: from the smallest start to the largest end of the lanes' non-empty runs
    int lo = rs < re ? rs : 0x7fffffff, hi = rs < re ? re : 0;
#pragma unroll
    for (int d = RJP_WAVE / 2; d > 0; d >>= 1) {
      lo = min(lo, __shfl_xor(lo, d, RJP_WAVE));
      hi = max(hi, __shfl_xor(hi, d, RJP_WAVE));
    }
    lo = __builtin_amdgcn_readfirstlane(lo);
    hi = __builtin_amdgcn_readfirstlane(hi);
    const int koff = j == 0 ? 0 : t.ni;                // red jet: the first half of the table
    double acc = 0.0;
    for (int r = lo; r < hi; r += U) {
      rjp_d2 cl[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
#if RJP_SRT_OWNROWS
        // a lane loads the rows of its own run only (see ff_scan_hybrid_kernel)
        cl[u] = rjp_d2{0.0, 0.0};
        if (r + u >= rs && r + u < re)
          cl[u] = __builtin_nontemporal_load(base + (int64_t)(r + u) * RJP_WAVE);
#else
        const int rr = r + u < hi ? r + u : hi - 1;    // (never past the wave's last row)
        cl[u] = __builtin_nontemporal_load(base + (int64_t)rr * RJP_WAVE);
#endif
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        double w = (t_epoch - cl[u].y - t.lo) * t.inv_h;
        w = __builtin_fmin(__builtin_fmax(w, 0.0), wmax);
        const double kf = __builtin_floor(w);
        const double xi = __builtin_fma(2.0, w - kf, -1.0);
        const rjp_d2* cp = reinterpret_cast<const rjp_d2*>(s_chi + ((int)kf + koff) * kChiStride);
        const rjp_d2 c01 = cp[0], c23 = cp[1], c45 = cp[2], c67 = cp[3];
        double chi = __builtin_fma(c67.y, xi, c67.x);
        chi = __builtin_fma(chi, xi, c45.y);
        chi = __builtin_fma(chi, xi, c45.x);
        chi = __builtin_fma(chi, xi, c23.y);
        chi = __builtin_fma(chi, xi, c23.x);
        chi = __builtin_fma(chi, xi, c01.y);
        chi = __builtin_fma(chi, xi, c01.x);
#if RJP_SRT_OWNROWS
        acc = __builtin_fma(cl[u].x, chi * chi, acc);      // (a row outside the run: weight 0.0)
#else
        const bool mine = r + u >= rs && r + u < re;
        acc = __builtin_fma(mine ? cl[u].x : 0.0, chi * chi, acc);
#endif
      }
    }
    total += acc + skipped;
  }
  if (!live) return;
  if (!s.hb[0]) total += s.aux[p];
  if (!s.hb[1]) total += s.aux[npix + p];
  if (s.aux[2 * npix + p] != 0.0) total = __builtin_inf();
  out[p] = total;
}

// ---- bins contracted from the layout's Chebyshev moments (rjp_fields.d_srt_mom) ----------------
// On bin k of a jet, F(ts) = chi^2(t - ts) as a function of the bin's coordinate x = 2 (w - k) - 1
// (the moments' x) is smooth wherever the bursts are wide against the bin.  When the Chebyshev
// interpolant p(x) = sum_n W_n T_n(x) of degree N - 1 equals F there, the bin's sum is
//   sum_cells |a0| F(ts) = sum_n W_n M_n,   M_n = sum_cells |a0| T_n(x)   (M_0: the d_srt_cum step)
// -- (N - 1) 8 bytes per sightline instead of 16 per cell.  srt_coef_kernel builds W on the device
// for every (jet, bin) in the support (N Chebyshev nodes of the exact F) and accepts the bin only if
// p matches at 4 N points across it BOTH the exact F and the table's chi^2 (what the cell path and
// the grid-order scan compute) to kSrtMomTol relative: a contracted bin then differs from the same
// bin read cell by cell by <= kSrtMomTol relative, as the tests against the grid order require.
constexpr double kSrtMomTol = 2e-14;
// How many of a contracted bin's N coefficients the scan sums.  The W_n of a smooth bin fall to the
// rounding of their own sums long before n = N - 1 (the far tail of a wide burst: 6-12 orders), and
// every order not summed is a moment plane not read.  srt_coef_kernel keeps the first m, m the
// smallest count whose dropped tail  sum_{n >= m} |W_n|  is <= kSrtTailFrac kSrtMomTol F_min (F_min:
// the smallest exact F at the check points).  The moments' weights |a0| are >= 0 and |T_n| <= 1 on
// the bin, so |M_n| <= M_0 and the dropped terms are <= tail M_0 <= kSrtTailFrac kSrtMomTol x the
// bin's sum (every F >= F_min): a bound in moment space that holds between the check points too.
// The fraction is set from below by the coefficients' own rounding: W_n is (2 / N) x a sum of N
// terms <= F_max, each rounded twice (cospi, the product), so a coefficient that is "zero" carries
// up to ~2 x 2^-53 F_max and N - 1 of them up to 4.2e-15 F_max at N = 20 -- a tail bound below
// that is never met on a flat bin (F_max ~ F_min).  1 / 4 (5e-15) is the smallest simple fraction
// above it, and leaves the sum of both errors (2e-14 at the check points, 0.5e-14 from the
// truncation between them) inside the 1e-13 the hybrid scan is held to against the other orders.
// The truncated interpolant is then put through checks (a) and (b) again, the same 4 N points and
// tolerance; where it fails, m = N: what the scan sums is exactly what was checked, and a bin
// accepted with N coefficients stays accepted whatever happens here.
constexpr double kSrtTailFrac = 0.25;
#ifndef RJP_SRT_TRUNC
#define RJP_SRT_TRUNC 1          /* 0: a build that sums all N coefficients of every contracted bin, for A/B only */
#endif
#ifndef RJP_SRT_PAIR
#define RJP_SRT_PAIR 1           /* 0: a build that loads the moment planes 8 bytes per lane, for A/B only */
#endif
constexpr int kSrtCoefThreads = 128;           // >= 4 N check points for N <= 24
constexpr int kSrtMaxN = 24;

struct SrtCoefDev {
  double s0, inv_h;                            // the layout's bins (srt_bins in ff_lt.hip)
  int K, N;
  int b0[2], b1[2];                            // the bins in each jet's support (SrtPlan)
  double* W;                                   // [2 K][N]
  int* ok;                                     // [2 K]: 0 = read the bin, else the coefficients to sum
};

__device__ __forceinline__ double chi_exact(const double* bj, int nb, double tl) {
  double chi = 1.0;
  for (int b = 0; b < nb; ++b) {
    const double d = tl - bj[b];
    chi += bj[nb + b] * exp(-d * d * bj[2 * nb + b]);
  }
  return chi;
}

// ---- table-residual bins -------------------------------------------------------------------------
// Check (b) rejects the bins on the steep flanks, where the TABLE's interpolation error
// E_i(xi) = T_i(xi)^2 - F reaches 2e-14 .. 6e-14 of F; there p still matches the exact F to a few
// 1e-15.  E is a smooth function of the table piece i and the piece coordinate xi alone, so per
// call srt_err_kernel fits it on every piece by a polynomial of degree 8 (least squares at 12
// Chebyshev nodes of the exact chi, f64; 9 monomial coefficients stored in f32 at a stride of 48
// bytes, an odd multiple of 16 like the chi table's 80), and a bin that passes (a) and fails (b) is
// tested against
//   (b')  |p + E~_i(xi) - T^2| <= kSrtMomTol T^2   at the same 4 N points,
// E~ and (i, xi) evaluated exactly as the scan evaluates them (the lookup's f64 index arithmetic,
// xi rounded to f32, an f32 Horner chain).  For such a bin
//   sum |a0| T^2(ts) = sum_n W_n M_n + sum_cells |a0| E~_i(xi(ts)):
// the first term is the contraction of any accepted bin, and the second -- at most ~2.2e-13 of
// the bin's sum by the table's own bound -- needs the launch time exactly but the weight to 8 bits
// only: the scan streams it from the layout's packed state (rjp_fields.d_srt_pts / d_srt_pw,
// ff_lt.hip), 10 bytes per cell instead of 16.  Error budget of a residual bin against the same
// bin read through the table: kSrtMomTol at the check points + 2^-9 x 2.2e-13 = 4.3e-16 from the
// weight.  (a), (b), kSrtMomTol, kSrtTailFrac and the table are what they were; the count rule
// runs with (b') in place of (b) on such a bin.
#ifndef RJP_SRT_RESID
#define RJP_SRT_RESID 1          /* 0: a build without table-residual bins (what fails (b) is read cell by cell), for A/B only */
#endif
#ifndef RJP_SRT_RESID_BLOCKS
#define RJP_SRT_RESID_BLOCKS 2   /* blocks of 8 packed rows (3 loads of 16 B; 5 without the codes) in flight per lane */
#endif
// Launch-time codes (rjp_fields.d_srt_pc, ff_lt.hip): with them attached the residual stream reads
// a 32-bit code of the launch time instead of the f64, 6 bytes per cell instead of 10.  Inside a
// table piece E~_i is a polynomial of degree 8 in an f32 xi, and a launch time known to a code step
// moves xi by about two f32 roundings; only WHICH piece needs the exact time, and only for a cell
// whose code interval reaches a piece boundary.  Such a cell falls back to its own 16-byte entry
// of the layout's cells and runs the arithmetic of the 10-byte path, so every cell gets exactly
// the piece it gets there.
// The margin.  q = fl(ts_hi - ts_lo) 2^-32, B = fl(q inv_h), A = the f64 value of
// (t_epoch - ts_lo - lo) inv_h - B / 2, and a cell of code c < 2^32 - 1 takes
//   w_q = fma(-c, B, A)   for the 10-byte path's   w = fl(fl(fl(t_epoch - ts) - lo) inv_h).
// In exact arithmetic w_q is the w of the middle of the code's interval, and ts lies within
// (1/2 + 2^-18) q of it (ff_lt.hip), so the two differ by at most (1/2 + 2^-18) q inv_h.  The
// roundings, with Tm = |t_epoch| + max(|ts_lo|, |ts_hi|) + |lo| (no intermediate of either chain
// exceeds Tm, or Tm inv_h): w carries two differences and a product, <= 3 x 2^-53 Tm inv_h; A two
// differences, a product and the B / 2 step, <= 4 x 2^-53 Tm inv_h; c B inherits B's rounding,
// <= 2^-53 x 2^32 q inv_h <= 2^-52 Tm inv_h; the fma adds one more 2^-53 Tm inv_h -- ten units in
// all, and rho = 2^-48 Tm inv_h grants thirty-two.  Hence
//   |w - w_q| < mg = 2 B + rho    (the code's half-width four times over, plus the roundings),
// and with f = w_q - floor(w_q) a cell is AMBIGUOUS when |f - 1/2| > 1/2 - mg, or when its code is
// saturated (2^32 - 1 stands for ts_hi and beyond).  Otherwise floor(w_q) + mg <= w_q and
// w_q <= floor(w_q) + 1 - mg put w strictly inside [floor(w_q), floor(w_q) + 1): floor(w) =
// floor(w_q), and clamping both to [0, wmax] keeps the floors equal (floor and clamp are
// monotone), so the piece is the 10-byte path's.  The test runs on the UNCLAMPED w_q: a cell far
// outside the table is as rarely ambiguous as one inside.  f is exact for w_q >= 0 and rounds to
// 1 just below an integer <= 0, which the test then calls ambiguous; f - 1/2 rounds by < 2^-54.
// The expected ambiguous share of launch times spread evenly over a stretch of w is 2 mg.
// xi of a decided cell moves by 2 |w - w_q| < (1 + 2^-17) B + 2 rho in f64, plus one f32 rounding
// on either side; |E~| <= 2.2e-13 F on [-1, 1] gives |E~'| <= 64 x 2.2e-13 F (Markov, degree 8),
// so a cell's term moves by < 2e-18 of itself at B = 6e-8: far below the 16-bit weight's 4.3e-16.
#ifndef RJP_SRT_CODES
#define RJP_SRT_CODES 1          /* 0: a build whose residual stream always reads the f64 launch times (10 bytes per cell), for A/B only */
#endif
constexpr int kErrNC = 9;                    // coefficients per piece (degree 8)
constexpr int kErrNodes = 12;
constexpr int kErrStride = 12;               // floats between pieces (48 B)
// chi table + error table of a scan with residual bins: two workgroups per CU (160 KiB of LDS)
constexpr size_t kSrtResidShm = 80 * 1024;
constexpr int kSrtResidFlag = 0x100;         // in srt_coef_kernel's verdict, above the count
// row n: the monomial coefficients of T_n
__device__ const double kErrCheb[kErrNC][kErrNC] = {
    {1, 0, 0, 0, 0, 0, 0, 0, 0},        {0, 1, 0, 0, 0, 0, 0, 0, 0},
    {-1, 0, 2, 0, 0, 0, 0, 0, 0},       {0, -3, 0, 4, 0, 0, 0, 0, 0},
    {1, 0, -8, 0, 8, 0, 0, 0, 0},       {0, 5, 0, -20, 0, 16, 0, 0, 0},
    {-1, 0, 18, 0, -48, 0, 32, 0, 0},   {0, -7, 0, 56, 0, -112, 0, 64, 0},
    {1, 0, -32, 0, 160, 0, -256, 0, 128}};

// behind chi_table_kernel: E[(jet * ni + k) * kErrStride + c]
__global__ __launch_bounds__(256) void srt_err_kernel(const double* __restrict__ stage, int nb0,
                                                      int nb1, ChiTabDev t,
                                                      const double* __restrict__ tab,
                                                      float* __restrict__ E) {
  // sixteen lanes per piece: lane m < 12 takes node m (the kernel sits in the scan's chain of
  // dependent launches when the tables are not built ahead: one thread per piece, twelve nodes
  // each, cost the 0.3 yr scan more than its two residual bins saved), then lane q < 9 writes
  // coefficient q
  const int tid = blockIdx.x * 256 + threadIdx.x;
  const int i = tid >> 4, m = tid & 15;
  const bool piece = i < 2 * t.ni;
  double e = 0.0;
  if (piece && m < kErrNodes) {
    const int j = i / t.ni, k = i - j * t.ni;
    const int nb = j == 0 ? nb0 : nb1;
    const double* bj = stage + kChiNC * kChiNC + kChiNC + (j == 0 ? 0 : 3 * nb0);
    const double* cp = tab + (size_t)i * kChiStride;
    const double x = cospi((m + 0.5) / kErrNodes);
    const double chi = chi_exact(bj, nb, t.lo + (k + 0.5 * (x + 1.0)) * (1.0 / t.inv_h));
    double ct = cp[7];
    for (int n = 6; n >= 0; --n) ct = __builtin_fma(ct, x, cp[n]);
    e = ct * ct - chi * chi;
  }
  // Chebyshev coefficients c_n = s_n sum_m e_m T_n(x_m), summed over the piece's lanes
  double c[kErrNC];
#pragma unroll
  for (int n = 0; n < kErrNC; ++n) {
    double v = e * cospi((double)((n * (2 * m + 1)) % (4 * kErrNodes)) / (2 * kErrNodes));
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) v += __shfl_xor(v, d, 16);
    c[n] = v * ((n == 0 ? 1.0 : 2.0) / kErrNodes);
  }
  if (!piece || m >= kErrStride) return;
  double a = 0.0;
  if (m < kErrNC) {
#pragma unroll
    for (int n = 0; n < kErrNC; ++n) a += c[n] * kErrCheb[n][m];
  }
  E[(size_t)i * kErrStride + m] = (float)a;
}

// E~ of a piece at xi: the f32 Horner chain of the scan and of check (b')
__device__ __forceinline__ float srt_err_eval(const rjp_f4 e0, const rjp_f4 e1, const float e8,
                                              const float xf) {
  float v = __builtin_fmaf(e8, xf, e1.w);
  v = __builtin_fmaf(v, xf, e1.z);
  v = __builtin_fmaf(v, xf, e1.y);
  v = __builtin_fmaf(v, xf, e1.x);
  v = __builtin_fmaf(v, xf, e0.w);
  v = __builtin_fmaf(v, xf, e0.z);
  v = __builtin_fmaf(v, xf, e0.y);
  return __builtin_fmaf(v, xf, e0.x);
}

// one workgroup per key q = jet * K + bin; `tab` / `t` / `stage` as chi_table_kernel's; `E`:
// srt_err_kernel's table, or null when the scan takes no residual bins
__global__ __launch_bounds__(kSrtCoefThreads) void srt_coef_kernel(const double* __restrict__ stage,
                                                                   int nb0, int nb1, ChiTabDev t,
                                                                   double t_epoch,
                                                                   const double* __restrict__ tab,
                                                                   const float* __restrict__ E,
                                                                   SrtCoefDev c) {
  __shared__ double sF[kSrtMaxN], sW[kSrtMaxN], sFc[4 * kSrtMaxN];
  const int q = blockIdx.x, i = threadIdx.x;
  const int j = q / c.K, k = q - j * c.K;
  if (k < c.b0[j] || k >= c.b1[j]) {
    if (i == 0) c.ok[q] = 0;
    return;
  }
  const int N = c.N, nb = j == 0 ? nb0 : nb1;
  const double* bj = stage + kChiNC * kChiNC + kChiNC + (j == 0 ? 0 : 3 * nb0);
  const double h = 1.0 / c.inv_h;
  auto ts_of = [&](double x) { return c.s0 + (k + 0.5 * (x + 1.0)) * h; };
  if (i < N) {
    const double chi = chi_exact(bj, nb, t_epoch - ts_of(cospi((i + 0.5) / N)));
    sF[i] = chi * chi;
  }
  __syncthreads();
  if (i < N) {
    // W_n = (2 / N) sum_m F(x_m) T_n(x_m), T_n(x_m) = cos(pi n (2 m + 1) / (2 N)); W_0 halved
    double s = 0.0;
    for (int m = 0; m < N; ++m) s += sF[m] * cospi((double)((i * (2 * m + 1)) % (4 * N)) / (2 * N));
    s *= (i == 0 ? 1.0 : 2.0) / N;
    sW[i] = s;
    c.W[(size_t)q * N + i] = s;
  }
  __syncthreads();
  // checks (a) and (b) at this thread's point, for the first `cnt` coefficients
  const double x = -1.0 + 2.0 * i / (4 * N - 1);
  double F = 1.0, T = 1.0, Et = 0.0;
  if (i < 4 * N) {
    const double ts = ts_of(x);
    const double chi = chi_exact(bj, nb, t_epoch - ts);
    F = chi * chi;
    // the table's chi at this launch time, as the scans evaluate it
    double w = (t_epoch - ts - t.lo) * t.inv_h;
    w = __builtin_fmin(__builtin_fmax(w, 0.0), t.wmax);
    const double kf = __builtin_floor(w);
    const double xi = __builtin_fma(2.0, w - kf, -1.0);
    const double* cp = tab + ((int)kf + (j == 0 ? 0 : t.ni)) * kChiStride;
    double ct = cp[7];
    for (int n = 6; n >= 0; --n) ct = __builtin_fma(ct, xi, cp[n]);
    T = ct * ct;
    sFc[i] = F;
    if (RJP_SRT_RESID && E) {
      // the fitted table error at this point, piece and xi as the scan takes them
      const rjp_f4* ep = reinterpret_cast<const rjp_f4*>(E + (size_t)((int)kf + (j == 0 ? 0 : t.ni)) * kErrStride);
      Et = (double)srt_err_eval(ep[0], ep[1], ep[2].x, (float)xi);
    }
  }
  // `resid`: check (b') in place of (b)
  auto passes = [&](int cnt, bool resid) {
    if (i >= 4 * N) return 1;
    double u1 = 0.0, u2 = 0.0;                 // Clenshaw
    for (int n = cnt - 1; n >= 1; --n) {
      const double un = __builtin_fma(2.0 * x, u1, sW[n] - u2);
      u2 = u1; u1 = un;
    }
    const double pv = __builtin_fma(x, u1, sW[0] - u2);
    const double pt = resid ? pv + Et : pv;
    return (int)(__builtin_fabs(pv - F) <= kSrtMomTol * F && __builtin_fabs(pt - T) <= kSrtMomTol * T);
  };
  int ok = __syncthreads_and(passes(N, false));        // (the barrier publishes sFc as well)
  int resid = 0;
  if (RJP_SRT_RESID && !ok && E) {                     // (uniform: so is the branch)
    resid = __syncthreads_and(passes(N, true));
    ok = resid;
  }
  int m = N;
  if (ok != 0 && RJP_SRT_TRUNC != 0) {
    // every thread finds the same m from the same shared values
    double fmin = sFc[0];
    for (int n = 1; n < 4 * N; ++n) fmin = __builtin_fmin(fmin, sFc[n]);
    const double lim = kSrtTailFrac * kSrtMomTol * fmin;
    double tail = 0.0;
    while (m > 1 && (tail += __builtin_fabs(sW[m - 1])) <= lim) --m;
    if (m < N && !__syncthreads_and(passes(m, resid != 0))) m = N;  // (m is uniform: so is the branch)
  }
  if (i == 0) c.ok[q] = ok ? (m | (resid ? kSrtResidFlag : 0)) : 0;
}

// The sorted scan with contracted bins: per group and jet, a bin of the support is contracted
// from the moments when srt_coef_kernel accepted it AND that reads fewer bytes for this group
// than its cells (the longest lane run of the bin x 16 B > (N - 1) x 8 B); every maximal run of
// the other bins is streamed as ff_scan_sorted_kernel streams its one run.  A jet no lane of the
// group holds is skipped (its sums are 0).  Without contracted bins the sums are
// ff_scan_sorted_kernel's, bit for bit.
// A contracted bin sums W_0 M_0 (each lane's own d_srt_cum step) and planes 1 .. m - 1 of its
// moments, m = srt_coef_kernel's count (the byte rule keeps N - 1: which bins are contracted does
// not depend on m).  The planes are read 16 bytes per lane: a plane's 64 sightlines of the group
// are 512 contiguous, 16-byte-aligned bytes (P is even on the table path), so lanes 0-31 take
// plane n as sightline pairs (2 l, 2 l + 1) and lanes 32-63 plane n + 1 the same way -- one wave
// instruction per two planes.  Each lane keeps the two sums of ITS PAIR (times W_n or W_n+1, by
// half-wave) across all contracted bins of both jets; the sums are linear, so the two half-waves
// are added and every sightline's sum moves to its own lane once, at the end of the scan.
// One wave serves a group and on a map like the bench's every wave is resident at once, so a
// wave's chain of dependent loads is the kernel's time: the index rows, verdicts, W_0 and cum
// steps of eight bins travel together, and a batch of N / 2 plane pairs runs on into the next
// contracted bin (same-buffer A/B of these shapes: profiles/r08_cfg4_hybrid_ab.json).
// A table-residual bin ("table-residual bins" above) is contracted in the same batches when the
// packed state is attached and the longest lane run x 6 B > (N - 1) x 8 B; every maximal run of
// such bins then streams weight x E~ of its cells from the packed state.  It counts as read.
struct SrtMomDev {
  const double* mom;                           // [2 K (N - 1)][P]
  const double* W;                             // [2 K][N]
  const int* ok;                               // [2 K]: 0 = read the bin, else the coefficients to sum
  // (contracted, read, residual) (jet, bin) counts and the fallback cells of every group,
  // [groups][4], or null: lane 0 of a group's wave stores its own four, zeros included -- every slot of a scan is written by that
  // scan, nothing is zeroed in front of it and no two waves share a word.  A residual bin counts
  // as read as well (its cells are read, from the packed state)
  unsigned long long* diag;
  // table-residual bins: srt_err_kernel's table (null: none are taken) and the packed state
  const float* E;
  const rjp_d2* pts;
  const rjp_u4* pw;
  // the launch-time codes (null: the residual stream reads `pts`) with A, B and 1/2 - mg of
  // "the margin" above (hm < 0: every cell falls back)
  const rjp_u4* pc;
  double cA, cB, hm;
};
constexpr int kSrtDiag = kSrtDiagWords;

template <int U, int N>
__global__ __launch_bounds__(kSrtBlock) __attribute__((amdgpu_waves_per_eu(4))) void ff_scan_hybrid_kernel(SrtDev s, SrtMomDev m,
                                                                   ChiTabDev t, double t_epoch,
                                                                   const double* __restrict__ tab,
                                                                   double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) double s_chi[];       // [2][ni][10], then [2][ni][12] floats
  for (int i = threadIdx.x; i < 2 * t.ni * kChiStride; i += kSrtBlock) s_chi[i] = tab[i];
  [[maybe_unused]] float* s_err = reinterpret_cast<float*>(s_chi + 2 * t.ni * kChiStride);
#if RJP_SRT_RESID
  if (m.E)
    for (int i = threadIdx.x; i < 2 * t.ni * kErrStride; i += kSrtBlock) s_err[i] = m.E[i];
#endif
  __syncthreads();
  const int lane = threadIdx.x & (RJP_WAVE - 1);
  const int64_t g = (int64_t)blockIdx.x * (kSrtBlock / RJP_WAVE) + threadIdx.x / RJP_WAVE;
  const int64_t npix = s.npix;
  if (g * RJP_WAVE >= npix) return;                    // (whole waves)
  const int64_t p = g * RJP_WAVE + lane;
  const bool live = p < npix;
  const int64_t rowbase = s.rowbase[g];
  const rjp_d2* base = s.cells + rowbase * RJP_WAVE + lane;
  const double wmax = t.wmax;
  const int K = s.K;
  unsigned n_res = 0;
  [[maybe_unused]] unsigned n_fb = 0;                  // this lane's cells that fell back to `cells`
  double racc = 0.0;                                   // sum of weight x E~ over the residual bins' cells
  auto start_at = [&](int q) { return live ? s.start[(int64_t)q * npix + p] : 0; };
  auto cum_at = [&](int q) { return live ? s.cum[(int64_t)q * npix + p] : 0.0; };
  auto wave_max = [](int v) {
#pragma unroll
    for (int d = RJP_WAVE / 2; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, RJP_WAVE));
    return __builtin_amdgcn_readfirstlane(v);
  };
  unsigned n_con = 0, n_read = 0;
  double total = 0.0;
  // the moment planes' sums: of this lane's sightline pair and half of the planes (RJP_SRT_PAIR),
  // else of its own sightline in .x
  static_assert(N % 2 == 0 && N <= kSrtMaxN, "the moment planes are read in pairs");
  [[maybe_unused]] constexpr int NP = N / 2;                            // pairs of planes (the last one is half empty)
  [[maybe_unused]] const int half = lane >> 5;
  [[maybe_unused]] const bool pair_live = g * RJP_WAVE + 2 * (lane & 31) < npix;
  rjp_d2 pacc{0.0, 0.0};
#pragma unroll 1
  for (int j = 0; j < 2; ++j) {
    const int q0 = j * K, b0 = s.b0[j], b1 = s.b1[j];
    if (wave_max(start_at(q0 + K) - start_at(q0)) == 0) continue;       // no lane holds the jet
    if (b0 >= b1) {
      total += cum_at(q0 + K) - cum_at(q0);
      continue;
    }
    const double skipped = (cum_at(q0 + K) - cum_at(q0 + b1)) + (cum_at(q0 + b0) - cum_at(q0));
    // which bins of the support this group contracts, and the M_0 terms of those: eight bins'
    // index rows, verdicts and W_0 per round trip to memory
    unsigned cmask = 0;
    unsigned rmask = 0;                                // of those, the table-residual bins
    unsigned long long cnt[3] = {0ull, 0ull, 0ull};    // coefficient counts, 5 bits per bin, 12 per word
    auto count_of = [&](int b) {
      return (int)(((b < 12 ? cnt[0] : b < 24 ? cnt[1] : cnt[2]) >> (5 * (b % 12))) & 31u);
    };
    double acc = 0.0;
    for (int bb = b0; bb < b1; bb += 8) {
      int st[9], wm[8];
      double cu[9], w0[8];
      unsigned mo[8];
#pragma unroll
      for (int u = 0; u < 9; ++u) {
        st[u] = start_at(q0 + min(bb + u, b1));
        cu[u] = cum_at(q0 + min(bb + u, b1));
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        mo[u] = (unsigned)m.ok[q0 + min(bb + u, b1 - 1)];
        w0[u] = m.W[(size_t)(q0 + min(bb + u, b1 - 1)) * N];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) wm[u] = wave_max(st[u + 1] - st[u]);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int b = bb + u;
        if (b < b1) {
          const unsigned mv = (unsigned)__builtin_amdgcn_readfirstlane(mo[u]);
          const unsigned mb = mv & 0xffu;
          // a residual bin pays when its packed cells (10 B) cost more than the planes on top of
          // the 4 B per cell it then does not read: longest run x 6 B > (N - 1) x 8 B
          const bool rb = RJP_SRT_RESID && (mv & (unsigned)kSrtResidFlag);
          if (mb && (rb ? (m.E != nullptr && wm[u] * 6 > (N - 1) * 8) : wm[u] * 16 > (N - 1) * 8)) {
            cmask |= 1u << b;
            if (rb) rmask |= 1u << b;
            acc = __builtin_fma(w0[u], cu[u + 1] - cu[u], acc);
          }
          const unsigned long long bits = (unsigned long long)mb << (5 * (b % 12));
          cnt[0] |= b < 12 ? bits : 0ull;
          cnt[1] |= b >= 12 && b < 24 ? bits : 0ull;
          cnt[2] |= b >= 24 ? bits : 0ull;
        }
      }
    }
    const int nc = __builtin_popcount(cmask & ~rmask);
    n_con += nc;
    n_read += (b1 - b0) - nc;
    n_res += __builtin_popcount(rmask);
#if RJP_SRT_PAIR
    // the planes of the contracted bins, NP plane pairs per round trip, a batch running on into
    // the next contracted bin: with m - 1 = 0 .. 16 planes a bin fills a batch rarely
    {
      auto next_bin = [&](int b) {
        while (b < b1 && !(((cmask >> b) & 1u) && count_of(b) > 1)) ++b;
        return b;
      };
      const double* mlane = m.mom + (int64_t)half * npix + g * RJP_WAVE + 2 * (lane & 31);
      int cb = next_bin(b0), ci = 0;                    // the next plane pair: bin, pair of the bin
      while (cb < b1) {
        rjp_d2 v[NP];
        double wn[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          v[i] = rjp_d2{0.0, 0.0};
          wn[i] = 0.0;
          if (cb < b1) {                                // (wave-uniform)
            const int m1 = count_of(cb) - 1, pl = 2 * ci + half;
            // W_pl+1 of this half-wave's plane (the empty half of an odd last pair: W_N-1 x 0)
            wn[i] = m.W[(size_t)(q0 + cb) * N + min(pl + 1, N - 1)];
            if (pl < m1 && pair_live)
              v[i] = __builtin_nontemporal_load(reinterpret_cast<const rjp_d2*>(
                  mlane + ((int64_t)(q0 + cb) * (N - 1) + 2 * ci) * npix));
            if (2 * ++ci >= m1) { cb = next_bin(cb + 1); ci = 0; }
          }
        }
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          pacc.x = __builtin_fma(wn[i], v[i].x, pacc.x);
          pacc.y = __builtin_fma(wn[i], v[i].y, pacc.y);
        }
      }
    }
#endif
    const int koff = j == 0 ? 0 : t.ni;                // red jet: the first half of the table
    for (int b = b0; b < b1;) {
      if ((cmask >> b) & 1u) {
#if !RJP_SRT_PAIR
        if (live) {
          const double* w = m.W + (size_t)(q0 + b) * N;
          const int m1 = count_of(b) - 1;                               // planes to read
          const double* mp = m.mom + (int64_t)(q0 + b) * (N - 1) * npix + p;
          double v[N - 1];
#pragma unroll
          for (int n = 0; n < N - 1; ++n)
            if (n < m1) v[n] = __builtin_nontemporal_load(mp + (int64_t)n * npix);
          double sum = 0.0;
#pragma unroll
          for (int n = 0; n < N - 1; ++n)
            if (n < m1) sum = __builtin_fma(w[n + 1], v[n], sum);
          pacc.x += sum;
        }
#endif
#if RJP_SRT_RESID
        if ((rmask >> b) & 1u) {
          // a maximal run of residual bins [b, e): weight x E~ of every cell, streamed from the
          // packed state in blocks of 8 rows aligned to 8 -- four 16-byte pairs of launch times
          // and one 16-byte unit of eight weights per lane, a lane loading only the units that
          // meet its own run; a row outside the run gets weight zero by predicate, so nothing it
          // holds can reach the sum (a NaN launch time lands in piece 0, as in the lookup)
          int e = b + 1;
#if RJP_SRT_PAIR
          while (e < b1 && ((rmask >> e) & 1u)) ++e;
#endif
          const int rs = start_at(q0 + b), re = start_at(q0 + e);
          int lo = rs < re ? rs : 0x7fffffff, hi = rs < re ? re : 0;
#pragma unroll
          for (int d = RJP_WAVE / 2; d > 0; d >>= 1) {
            lo = min(lo, __shfl_xor(lo, d, RJP_WAVE));
            hi = max(hi, __shfl_xor(hi, d, RJP_WAVE));
          }
          lo = __builtin_amdgcn_readfirstlane(lo) & ~7;
          hi = __builtin_amdgcn_readfirstlane(hi);
          const int64_t pb = srt_packed_row(rowbase, g);
          const rjp_d2* pt = m.pts + (pb / 2) * RJP_WAVE + lane;
          const rjp_u4* pq = m.pw + (pb / 8) * RJP_WAVE + lane;
          constexpr int RB = RJP_SRT_RESID_BLOCKS;       // blocks of 8 rows in flight
#if RJP_SRT_CODES
          // with the codes: two 16-byte units of four codes and the weight unit per block of 8
          // rows.  E~ of every cell first, from the code; then, where any lane of the wave holds
          // an ambiguous cell of its own run ("the margin" above), those lanes redo theirs from
          // their own entry of `cells` with the arithmetic of the loop below; then the additions
          // into racc, in that loop's order
          if (m.pc) {
            const rjp_u4* pcq = m.pc + (pb / 4) * RJP_WAVE + lane;
            for (int r = lo; r < hi; r += 8 * RB) {
              rjp_u4 cc[RB][2];
              rjp_u4 wq[RB];
#pragma unroll
              for (int k = 0; k < RB; ++k) {
                const int rk = r + 8 * k;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                  cc[k][u] = rjp_u4{0u, 0u, 0u, 0u};
                  if (rk + 4 * u + 3 >= rs && rk + 4 * u < re)
                    cc[k][u] = __builtin_nontemporal_load(pcq + (int64_t)(rk / 4 + u) * RJP_WAVE);
                }
                wq[k] = rjp_u4{0u, 0u, 0u, 0u};
                if (rk + 7 >= rs && rk < re)
                  wq[k] = __builtin_nontemporal_load(pq + (int64_t)(rk / 8) * RJP_WAVE);
              }
              float ev[8 * RB];
              unsigned amb = 0;                          // bit 8 k + u: the cell falls back
#pragma unroll
              for (int k = 0; k < RB; ++k)
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                  const int row = r + 8 * k + u;
                  const unsigned c = cc[k][u / 4][u % 4];
                  const double wv = __builtin_fma(-(double)c, m.cB, m.cA);
                  const double f = wv - __builtin_floor(wv);
                  const bool a = (__builtin_fabs(f - 0.5) > m.hm) | (c == 0xffffffffu);
                  amb |= (a && row >= rs && row < re) ? 1u << (8 * k + u) : 0u;
                  const double w = __builtin_fmin(__builtin_fmax(wv, 0.0), wmax);
                  const double kf = __builtin_floor(w);
                  const double xi = __builtin_fma(2.0, w - kf, -1.0);
                  const rjp_f4* ep = reinterpret_cast<const rjp_f4*>(s_err + ((int)kf + koff) * kErrStride);
                  const rjp_f4 e0 = ep[0], e1 = ep[1];
                  ev[8 * k + u] = srt_err_eval(e0, e1, ep[2].x, (float)xi);
                }
              if (__any(amb != 0u)) {                    // (rare: 2 mg of the cells)
                n_fb += (unsigned)__builtin_popcount(amb);
                while (amb) {
                  const int i = __builtin_ctz(amb);
                  amb &= amb - 1u;
                  const rjp_d2 cl = __builtin_nontemporal_load(base + (int64_t)(r + i) * RJP_WAVE);
                  double w = (t_epoch - cl.y - t.lo) * t.inv_h;
                  w = __builtin_fmin(__builtin_fmax(w, 0.0), wmax);
                  const double kf = __builtin_floor(w);
                  const double xi = __builtin_fma(2.0, w - kf, -1.0);
                  const rjp_f4* ep = reinterpret_cast<const rjp_f4*>(s_err + ((int)kf + koff) * kErrStride);
                  const rjp_f4 e0 = ep[0], e1 = ep[1];
                  const float ex = srt_err_eval(e0, e1, ep[2].x, (float)xi);
#pragma unroll
                  for (int u = 0; u < 8 * RB; ++u) ev[u] = u == i ? ex : ev[u];
                }
              }
#pragma unroll
              for (int k = 0; k < RB; ++k)
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                  const int row = r + 8 * k + u;
                  const unsigned wd = wq[k][u / 2];
                  const unsigned code = (u & 1) ? (wd >> 16) : (wd & 0xffffu);
                  const float wf = (row >= rs && row < re) ? __uint_as_float(code << 15) : 0.0f;
                  racc = __builtin_fma((double)wf, (double)ev[8 * k + u], racc);
                }
            }
            b = e;
            continue;
          }
#endif
          for (int r = lo; r < hi; r += 8 * RB) {
            rjp_d2 tt[RB][4];
            rjp_u4 wq[RB];
#pragma unroll
            for (int k = 0; k < RB; ++k) {
              const int rk = r + 8 * k;
#pragma unroll
              for (int u = 0; u < 4; ++u) {
                tt[k][u] = rjp_d2{0.0, 0.0};
                if (rk + 2 * u + 1 >= rs && rk + 2 * u < re)
                  tt[k][u] = __builtin_nontemporal_load(pt + (int64_t)(rk / 2 + u) * RJP_WAVE);
              }
              wq[k] = rjp_u4{0u, 0u, 0u, 0u};
              if (rk + 7 >= rs && rk < re)
                wq[k] = __builtin_nontemporal_load(pq + (int64_t)(rk / 8) * RJP_WAVE);
            }
#pragma unroll
            for (int k = 0; k < RB; ++k)
#pragma unroll
              for (int u = 0; u < 8; ++u) {
                const int row = r + 8 * k + u;
                const double tsu = (u & 1) ? tt[k][u / 2].y : tt[k][u / 2].x;
                const unsigned wd = wq[k][u / 2];
                const unsigned code = (u & 1) ? (wd >> 16) : (wd & 0xffffu);
                const float wf = (row >= rs && row < re) ? __uint_as_float(code << 15) : 0.0f;
                double w = (t_epoch - tsu - t.lo) * t.inv_h;
                w = __builtin_fmin(__builtin_fmax(w, 0.0), wmax);
                const double kf = __builtin_floor(w);
                const double xi = __builtin_fma(2.0, w - kf, -1.0);
                const rjp_f4* ep = reinterpret_cast<const rjp_f4*>(s_err + ((int)kf + koff) * kErrStride);
                const rjp_f4 e0 = ep[0], e1 = ep[1];
                const float e8 = ep[2].x;
                racc = __builtin_fma((double)wf, (double)srt_err_eval(e0, e1, e8, (float)xi), racc);
              }
          }
          b = e;
          continue;
        }
#endif
        ++b;
        continue;
      }
      int e = b + 1;
      while (e < b1 && !((cmask >> e) & 1u)) ++e;
      // bins [b, e) cell by cell: the wave's rows from the smallest start to the largest end of
      // the lanes' non-empty runs, as ff_scan_sorted_kernel
      const int rs = start_at(q0 + b), re = start_at(q0 + e);
      int lo = rs < re ? rs : 0x7fffffff, hi = rs < re ? re : 0;
#pragma unroll
      for (int d = RJP_WAVE / 2; d > 0; d >>= 1) {
        lo = min(lo, __shfl_xor(lo, d, RJP_WAVE));
        hi = max(hi, __shfl_xor(hi, d, RJP_WAVE));
      }
      lo = __builtin_amdgcn_readfirstlane(lo);
      hi = __builtin_amdgcn_readfirstlane(hi);
      for (int r = lo; r < hi; r += U) {
        rjp_d2 cl[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
#if RJP_SRT_OWNROWS
          // a lane loads the rows of its own run only: a row outside it is never fetched for the
          // lane, and nothing that row holds (a NaN included) can reach the lane's sum
          cl[u] = rjp_d2{0.0, 0.0};
          if (r + u >= rs && r + u < re)
            cl[u] = __builtin_nontemporal_load(base + (int64_t)(r + u) * RJP_WAVE);
#else
          const int rr = r + u < hi ? r + u : hi - 1;  // (never past the wave's last row)
          cl[u] = __builtin_nontemporal_load(base + (int64_t)rr * RJP_WAVE);
#endif
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          double w = (t_epoch - cl[u].y - t.lo) * t.inv_h;
          w = __builtin_fmin(__builtin_fmax(w, 0.0), wmax);
          const double kf = __builtin_floor(w);
          const double xi = __builtin_fma(2.0, w - kf, -1.0);
          const rjp_d2* cp = reinterpret_cast<const rjp_d2*>(s_chi + ((int)kf + koff) * kChiStride);
          const rjp_d2 c01 = cp[0], c23 = cp[1], c45 = cp[2], c67 = cp[3];
          double chi = __builtin_fma(c67.y, xi, c67.x);
          chi = __builtin_fma(chi, xi, c45.y);
          chi = __builtin_fma(chi, xi, c45.x);
          chi = __builtin_fma(chi, xi, c23.y);
          chi = __builtin_fma(chi, xi, c23.x);
          chi = __builtin_fma(chi, xi, c01.y);
          chi = __builtin_fma(chi, xi, c01.x);
#if RJP_SRT_OWNROWS
          acc = __builtin_fma(cl[u].x, chi * chi, acc);      // (a row outside the run: weight 0.0)
#else
          const bool mine = r + u >= rs && r + u < re;
          acc = __builtin_fma(mine ? cl[u].x : 0.0, chi * chi, acc);
#endif
        }
      }
      b = e;
    }
    total += acc + skipped;
  }
#if RJP_SRT_DIAG
  if (m.diag && lane == 0) {
    m.diag[kSrtDiag * g] = (unsigned long long)n_con;
    m.diag[kSrtDiag * g + 1] = (unsigned long long)n_read;
    m.diag[kSrtDiag * g + 2] = (unsigned long long)n_res;
  }
#if RJP_SRT_RESID && RJP_SRT_CODES
  if (m.diag) {                                        // (uniform; all lanes are here)
#pragma unroll
    for (int d = RJP_WAVE / 2; d > 0; d >>= 1) n_fb += (unsigned)__shfl_xor((int)n_fb, d, RJP_WAVE);
  }
#endif
  if (m.diag && lane == 0) m.diag[kSrtDiag * g + 3] = (unsigned long long)n_fb;
#endif
  total += racc;                                       // (+0.0 without residual bins)
#if RJP_SRT_PAIR
  // both halves of the planes, then sightline l from the pair of lane l / 2 (all lanes are here)
  pacc.x += __shfl_xor(pacc.x, 32, RJP_WAVE);
  pacc.y += __shfl_xor(pacc.y, 32, RJP_WAVE);
  const double px = __shfl(pacc.x, lane >> 1, RJP_WAVE), py = __shfl(pacc.y, lane >> 1, RJP_WAVE);
  total += (lane & 1) ? py : px;
#else
  total += pacc.x;
#endif
  if (!live) return;
  if (!s.hb[0]) total += s.aux[p];
  if (!s.hb[1]) total += s.aux[npix + p];
  if (s.aux[2 * npix + p] != 0.0) total = __builtin_inf();
  out[p] = total;
}

// The same scan from the five MODEL fields (nd, xi, temp, pf, ts: SURVEY 8(d)'s byte model, what
// a model without the derived scan fields a0 / em0 streams): optical-depth sums, emission measure
// and T_avg of the epoch in one pass, the burst factor from the table.  Per-product NaN semantics
// as ff_scan_kernel's wide layout (nansum of (n chi x)^2 pf T^p and of (n chi x)^2 pf; T_avg =
// nanmean_y(T > 0), classes.py:1116-1118, 1395-1397, 1471-1472).
template <int U, int MODE>
__global__ __launch_bounds__(kBlock) void ff_scan_table_wide_kernel(
    FieldPtrs<double> f, int ny, int nz, int64_t nchunks, int64_t npix, int ylen, int nsplit,
    ChiTabDev t, double t_epoch, const double* __restrict__ tab, double* __restrict__ ws,
    double* __restrict__ sumA, double* __restrict__ em, double* __restrict__ tavg,
    double em_scale) {
  constexpr int VEC = 2;
  extern __shared__ __attribute__((aligned(16))) double s_chi[];       // [2][ni][10]
  for (int i = threadIdx.x; i < 2 * t.ni * kChiStride; i += kBlock) s_chi[i] = tab[i];
  const LaneRange lr = lane_y_range<VEC, kBlock>(nsplit, ylen, ny, nchunks, f.ylo, f.yhi);
  __syncthreads();                           // the table is staged
  if (!lr.live) return;
  const int split = lr.split, y0 = lr.y0, y1 = lr.y1;
  const int64_t p0 = lr.p0;
  const int64_t x = p0 / nz;
  const int z = (int)(p0 - x * nz);
  const double wmax = t.wmax;
  auto chi2 = [&](bool red, double tv) __attribute__((always_inline)) {
    double w = (t_epoch - tv - t.lo) * t.inv_h;
    w = __builtin_fmin(__builtin_fmax(w, 0.0), wmax);
    const double kf = __builtin_floor(w);
    const double xi = __builtin_fma(2.0, w - kf, -1.0);
    const int k = (int)kf + (red ? 0 : t.ni);
    const rjp_d2* cp = reinterpret_cast<const rjp_d2*>(s_chi + k * kChiStride);
    const rjp_d2 c01 = cp[0], c23 = cp[1], c45 = cp[2], c67 = cp[3];
    double chi = __builtin_fma(c67.y, xi, c67.x);
    chi = __builtin_fma(chi, xi, c45.y);
    chi = __builtin_fma(chi, xi, c45.x);
    chi = __builtin_fma(chi, xi, c23.y);
    chi = __builtin_fma(chi, xi, c23.x);
    chi = __builtin_fma(chi, xi, c01.y);
    chi = __builtin_fma(chi, xi, c01.x);
    return chi * chi;
  };
  double accA[VEC] = {0.0, 0.0}, accE[VEC] = {0.0, 0.0}, accT[VEC] = {0.0, 0.0};
  double tmin = __builtin_inf(), tmax = -__builtin_inf();
  int cnt[VEC] = {0, 0};
  auto rows = [&](auto utag, int64_t off) __attribute__((always_inline)) {
    constexpr int UU = decltype(utag)::value;
    double nd[UU][VEC], xi[UU][VEC], tp[UU][VEC], pf[UU][VEC], tt[UU][VEC];
#pragma unroll
    for (int u = 0; u < UU; ++u) {
      const int64_t o = off + (int64_t)u * nz;
      load_vec(f.nd + o, nd[u]);
      load_vec(f.xi + o, xi[u]);
      load_vec(f.temp + o, tp[u]);
      load_vec(f.pf + o, pf[u]);
      load_vec(f.ts + o, tt[u]);
    }
    double tpw[UU][VEC];
    if (MODE == RJP_GFF_POWERLAW)
      pow_m1p35_batch<UU * VEC>(reinterpret_cast<const double (&)[UU * VEC]>(tp),
                                reinterpret_cast<double (&)[UU * VEC]>(tpw));
    else
      pow_m1p5_batch<UU * VEC>(reinterpret_cast<const double (&)[UU * VEC]>(tp),
                               reinterpret_cast<double (&)[UU * VEC]>(tpw));
#pragma unroll
    for (int u = 0; u < UU; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const double Tk = tp[u][v];
        accT[v] += __builtin_fmax(Tk, 0.0);
        cnt[v] += Tk > 0.0 ? 1 : 0;
        const double n0 = __builtin_fabs(nd[u][v]) * xi[u][v];
        const double g = poison_unless(n0 * n0 * pf[u][v], tt[u][v] == tt[u][v]);
        const double c2 = chi2(signbit_d(nd[u][v]), tt[u][v]);
        if (RJP_TAB_GUARD) {
          tmin = __builtin_fmin(tmin, tt[u][v]);
          tmax = __builtin_fmax(tmax, tt[u][v]);
        }
        accE[v] = __builtin_fma(nan_to_zero<false>(g), c2, accE[v]);
        accA[v] = __builtin_fma(nan_to_zero<false>(g * tpw[u][v]), c2, accA[v]);
      }
  };
  int64_t off = (x * ny + y0) * (int64_t)nz + z;
  int y = y0;
  for (; y + U <= y1; y += U) {
    rows(std::integral_constant<int, U>{}, off);
    off += (int64_t)U * nz;
  }
  for (; y < y1; ++y) {
    rows(std::integral_constant<int, 1>{}, off);
    off += nz;
  }
  if (ts_range_breach(t, tmin, tmax)) {
    *t.guard = 1;
#pragma unroll
    for (int v = 0; v < VEC; ++v) { accA[v] = __builtin_nan(""); accE[v] = __builtin_nan(""); }
  }
  if (nsplit == 1) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      sumA[p0 + v] = accA[v];
      if (em) em[p0 + v] = accE[v] * em_scale;
      if (tavg) tavg[p0 + v] = accT[v] / (double)cnt[v];      // 0/0 = NaN on empty sightlines
    }
  } else {
    double* w = ws + (int64_t)split * nacc(1) * npix + p0;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      w[v] = accA[v];
      w[npix + v] = accE[v];
      w[2 * npix + v] = accT[v];
      w[3 * npix + v] = (double)cnt[v];
    }
  }
}

// ---- host -----------------------------------------------------------------------------------
// Vandermonde inverse of the 8 Chebyshev nodes on [-1, 1] (monomial coefficients in the interval's
// own coordinate from node values; on [-1, 1] the matrix is well conditioned)
static void chi_nodes(double (&xs)[kChiNC], double (&vinv)[kChiNC][kChiNC]) {
  const double pi = 3.14159265358979323846;
  double A[kChiNC][2 * kChiNC];
  for (int m = 0; m < kChiNC; ++m) {
    xs[m] = -std::cos(pi * (m + 0.5) / kChiNC);
    double p = 1.0;
    for (int q = 0; q < kChiNC; ++q) { A[m][q] = p; p *= xs[m]; }
    for (int q = 0; q < kChiNC; ++q) A[m][kChiNC + q] = m == q ? 1.0 : 0.0;
  }
  for (int c = 0; c < kChiNC; ++c) {
    int piv = c;
    for (int r = c + 1; r < kChiNC; ++r) if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
    for (int q = 0; q < 2 * kChiNC; ++q) std::swap(A[c][q], A[piv][q]);
    for (int r = 0; r < kChiNC; ++r)
      if (r != c) {
        const double f = A[r][c] / A[c][c];
        for (int q = 0; q < 2 * kChiNC; ++q) A[r][q] -= f * A[c][q];
      }
  }
  for (int c = 0; c < kChiNC; ++c)
    for (int m = 0; m < kChiNC; ++m) vinv[c][m] = A[c][kChiNC + m] / A[c][c];
}

// Can this scan take the table path, and with which table?  On success: cp.tab describes the
// table, cp.stage is the small host table to stage (inverse, nodes, burst parameters).
bool chi_table_plan(const rjp_fields* fl, const rjp_bursts* hb, const double* epochs, int n_epochs,
                    int mode, bool want_em, size_t work_bytes, ChiPlan& cp) {
  cp.ok = false;
  if (!hb || (hb->n[0] <= 0 && hb->n[1] <= 0) || n_epochs != 1) return false;
  // the tau layout (a0, ts [, em0]) or the five model fields (f64): the compact layout -- no
  // default of any producer -- keeps the Gaussians
  const int lay = scan_layout(fl, mode, want_em);
  if ((lay != LAY_TAU && !(lay == LAY_WIDE && fl->dtype == RJP_F64)) || !fl->d_ts ||
      ff_scan_vec(fl) != 2)
    return false;
  cp.wide = lay == LAY_WIDE;
  if (!(fl->ts_hi >= fl->ts_lo) || !std::isfinite(fl->ts_lo) || !std::isfinite(fl->ts_hi) ||
      (fl->ts_lo == 0.0 && fl->ts_hi == 0.0) || !std::isfinite(epochs[0]))
    return false;
  // small maps gain nothing (their scan is launch-bound) and their workspace may not hold the table
  const int64_t npix = (int64_t)fl->nx * fl->nz;
  if (npix / 2 < 64 * 256 || fl->ny < 64) return false;
  // the bursts' support and the interpolation bound
  double s_lo = INFINITY, s_hi = -INFINITY, B = 0.0;
  for (int j = 0; j < 2; ++j) {
    double Bj = 0.0;
    for (int i = 0; i < hb->n[j]; ++i) {
      const double inv = hb->inv2s2[j][i], amp = hb->amp_rel[j][i], t0 = hb->t0[j][i];
      if (!(inv > 0.0) || !std::isfinite(inv) || !(amp >= 0.0) || !std::isfinite(amp) ||
          !std::isfinite(t0))
        return false;                             // dips (chi < 1) and degenerate widths: Gaussians
      const double sigma = std::sqrt(0.5 / inv);
      s_lo = std::min(s_lo, t0 - chi_reach(amp) * sigma);
      s_hi = std::max(s_hi, t0 + chi_reach(amp) * sigma);
      const double s2 = sigma * sigma;
      Bj += amp * 105.0 / (s2 * s2 * s2 * s2);
    }
    B = std::max(B, Bj);
  }
  double lo = std::max(s_lo, epochs[0] - fl->ts_hi), hi = std::min(s_hi, epochs[0] - fl->ts_lo);
  int ni = 1;
  if (!(hi > lo)) {
    // no cell is inside a burst's support at this epoch: chi == 1, one constant interval
    lo = epochs[0] - fl->ts_hi;
    hi = lo + 1.0;
  } else {
    const double h = 2.0 * std::pow(kChiTol * 5160960.0 / B, 1.0 / 8.0);      // 8! 2^7
    const double n = std::ceil((hi - lo) / h);
    if (!(n <= kChiMaxNI)) return false;          // would not fit the LDS: Gaussians
    ni = std::max(1, (int)n);
  }
  const size_t tab_bytes = (size_t)2 * ni * kChiStride * sizeof(double);
  // the table sits in the caller's workspace, in planes 2-3 of the first y-range's four planes
  // (the temperature sums of the other layouts: the scan writes planes 0 and 1 only): 2 npix
  // doubles in, 16-byte aligned because n_z is even
  if (work_bytes < (size_t)2 * npix * sizeof(double) + tab_bytes || (size_t)2 * npix * 8 < tab_bytes)
    return false;
  // (the wide scan fills all four planes of its <= 8 y-ranges: its table sits behind them)
  if (cp.wide && work_bytes < (size_t)32 * npix * sizeof(double) + tab_bytes) return false;
  cp.ni = ni;
  cp.lo = lo;
  cp.inv_h = ni / (hi - lo);
  cp.n[0] = hb->n[0]; cp.n[1] = hb->n[1];
  struct Nodes {
    double xs[kChiNC], vinv[kChiNC][kChiNC];
    Nodes() { chi_nodes(xs, vinv); }
  };
  static const Nodes nodes;                       // (initialised once, thread-safely)
  cp.stage.clear();
  for (int c = 0; c < kChiNC; ++c)
    for (int m = 0; m < kChiNC; ++m) cp.stage.push_back(nodes.vinv[c][m]);
  for (int m = 0; m < kChiNC; ++m) cp.stage.push_back(nodes.xs[m]);
  for (int j = 0; j < 2; ++j)
    for (int k = 0; k < 3; ++k)
      for (int i = 0; i < hb->n[j]; ++i)
        cp.stage.push_back(k == 0 ? hb->t0[j][i] : k == 1 ? hb->amp_rel[j][i] : hb->inv2s2[j][i]);
  cp.ok = true;
  return true;
}

// The bins of the launch-time-bucketed layout a scan at t_epoch reads: per jet, those that meet
// [t - s_hi, t - s_lo], the launch times for which the jet's own bursts' support (chi_reach, as
// the table's) is reached.  A cell of a bin at the edge may lie outside the support: it is read,
// and the table gives it chi = 1 to the table's bound, as the grid-order scan does.
bool srt_plan(const rjp_fields* fl, const rjp_bursts* hb, double t_epoch, SrtPlan& sp) {
  const int K = fl->srt_K;
  if (!fl->d_srt_cells || !fl->d_srt_start || !fl->d_srt_cum || !fl->d_srt_rowbase ||
      !fl->d_srt_aux || !fl->h_srt_hist || K < 1 || K > RJP_SRT_MAX_K || !hb)
    return false;
  const double span = fl->ts_hi - fl->ts_lo;
  const double inv_h = span > 0.0 ? K / span : 1.0;           // (srt_bins: the layout's bins)
  int64_t all = 0, read = 0;
  for (int j = 0; j < 2; ++j) {
    sp.hb[j] = hb->n[j] > 0;
    sp.b0[j] = sp.b1[j] = 0;
    if (sp.hb[j]) {
      double s_lo = INFINITY, s_hi = -INFINITY;
      for (int i = 0; i < hb->n[j]; ++i) {
        const double sigma = std::sqrt(0.5 / hb->inv2s2[j][i]);
        s_lo = std::min(s_lo, hb->t0[j][i] - chi_reach(hb->amp_rel[j][i]) * sigma);
        s_hi = std::max(s_hi, hb->t0[j][i] + chi_reach(hb->amp_rel[j][i]) * sigma);
      }
      const double w0 = std::floor((t_epoch - s_hi - fl->ts_lo) * inv_h);
      const double w1 = std::floor((t_epoch - s_lo - fl->ts_lo) * inv_h) + 1.0;
      const int b0 = (int)std::min(std::max(w0, 0.0), (double)K);
      const int b1 = (int)std::min(std::max(w1, 0.0), (double)K);
      if (b1 > b0) { sp.b0[j] = b0; sp.b1[j] = b1; }
    }
    for (int b = 0; b < K; ++b) {
      const int64_t n = fl->h_srt_hist[j * K + b];
      all += n;
      if (b >= sp.b0[j] && b < sp.b1[j]) read += n;
    }
  }
  sp.share = all > 0 ? (double)read / (double)all : 0.0;
  sp.N = fl->d_srt_mom && srt_moment_order_ok(fl->srt_N) ? fl->srt_N : 0;
  sp.packed = sp.N > 0 && fl->d_srt_pts && fl->d_srt_pw;
  sp.codes = sp.packed && fl->d_srt_pc;
  return sp.share <= 0.9;
}

// y-ranges of the table scan on a map of `npix` sightlines and `ny` rows: one when the sightline
// chunks alone give every CU two workgroups, else as many as it takes (powers of two, >= 64 rows
// each; the partials are reduced in ff_reduce_kernel's fixed order)
static int chi_table_nsplit(int64_t npix, int ny, bool wide) {
  const int64_t wgs = (npix / 2 + kBlock - 1) / kBlock;
  int nsplit = 1;
  while (wgs * nsplit < RJP_TAB_WGS && nsplit * 2 * 64 <= ny && nsplit < (wide ? 8 : 16)) nsplit *= 2;
  return nsplit;
}

// Workspace of the table path (part of rjp_ff_scan_workspace): the tau-layout scan writes planes
// 0-1 of nacc(1) = 4 planes per y-range and keeps its table in planes 2-3 of the first range; the
// wide scan fills all four planes of its <= 8 ranges and keeps the table behind them.
size_t chi_table_workspace_bytes(int64_t npix, int ny) {
  if (npix / 2 < 64 * 256 || ny < 64) return 0;            // (chi_table_plan's size rule)
  const size_t tab = (size_t)2 * kChiMaxNI * kChiStride * sizeof(double);
  const size_t tau = (size_t)chi_table_nsplit(npix, ny, false) * nacc(1) * npix * sizeof(double);
  const size_t wide = (size_t)32 * npix * sizeof(double) + tab;
  return std::max(tau, wide);
}

// ---- tables ahead of the scan (rjp_host.h: TabRing) ---------------------------------------------
#ifndef RJP_TABLES_AHEAD
#define RJP_TABLES_AHEAD 1       /* 0: a build whose table kernels stay on the caller's stream, in front of the scan, for A/B only */
#endif
constexpr size_t kRingTab = (size_t)2 * kChiMaxNI * kChiStride;           // doubles
constexpr size_t kRingW = (size_t)2 * RJP_SRT_MAX_K * kSrtMaxN;           // doubles
constexpr size_t kRingE = (size_t)2 * kChiMaxNI * kErrStride;              // floats
constexpr size_t kRingSlotBytes =
    ((kRingTab + kRingW) * sizeof(double) + kRingE * sizeof(float) +
     2 * RJP_SRT_MAX_K * sizeof(int) + 255) / 256 * 256;

void tab_ring_destroy(TabRing& r) {
  if (r.side) {
    (void)hipStreamSynchronize(r.side);
    (void)hipStreamDestroy(r.side);
  }
  for (auto& s : r.slot) {
    if (s.ready) (void)hipEventDestroy(s.ready);
    if (s.uploaded) (void)hipEventDestroy(s.uploaded);
  }
  if (r.mem) (void)hipFree(r.mem);
  r = TabRing();
}

void tab_ring_create(TabRing& r) {
  r = TabRing();
  bool ok = hipMalloc(&r.mem, TabRing::kSlots * kRingSlotBytes) == hipSuccess;
  for (int i = 0; ok && i < TabRing::kSlots; ++i) {
    TabRing::Slot& s = r.slot[i];
    s.tab = reinterpret_cast<double*>(static_cast<char*>(r.mem) + i * kRingSlotBytes);
    s.W = s.tab + kRingTab;
    s.E = reinterpret_cast<float*>(s.W + kRingW);         // (16-byte aligned: read as float4)
    s.ok = reinterpret_cast<int*>(s.E + kRingE);
    ok = hipEventCreateWithFlags(&s.ready, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&s.uploaded, hipEventDisableTiming) == hipSuccess;
  }
  ok = ok && hipStreamCreateWithFlags(&r.side, hipStreamNonBlocking) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();      // (not this context's caller's error: the ring is optional)
    tab_ring_destroy(r);
  }
}

// The table kernels of one scan: on the caller's stream, or on the ring's side stream with the
// events that order a slot.  join() puts the caller's stream behind the tables (once; it is a
// no-op on the caller's own stream).
struct TabLaunch {
  hipStream_t st, ts;             // the caller's stream; the stream of the table kernels
  TabRing::Slot* slot = nullptr;
  bool joined = false;
  hipError_t join() {
    if (!slot || joined) return hipSuccess;
    joined = true;
    hipError_t e = hipEventRecord(slot->ready, ts);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, slot->ready, 0);
    return e;
  }
};

static hipError_t chi_table_scan_on(const rjp_fields* fl, const ChiPlan& cp, const double* d_stage,
                                    double t_epoch, int mode, double* sumA, double* em,
                                    double* tavg, double* ws, size_t work_bytes, int* d_guard,
                                    hipStream_t st, const SrtPlan* sp, TabLaunch& tl,
                                    double* d_tab, double* d_W, int* d_ok, float* d_E);

hipError_t chi_table_scan(const rjp_fields* fl, const ChiPlan& cp, const double* d_stage,
                          double t_epoch, int mode, double* sumA, double* em, double* tavg,
                          double* ws, size_t work_bytes, int* d_guard, hipStream_t st,
                          const SrtPlan* sp, TabRing* ring, bool* stage_fresh,
                          hipEvent_t release_ev) {
  const int64_t npix = (int64_t)fl->nx * fl->nz;
  const size_t tab_doubles = (size_t)2 * cp.ni * kChiStride;
  if (((uintptr_t)ws % 16) != 0 || work_bytes < (2 * npix + tab_doubles) * sizeof(double))
    return hipErrorInvalidValue;
  if (cp.wide && work_bytes < (32 * npix + tab_doubles) * sizeof(double)) return hipErrorInvalidValue;
  // single-stream order: the table in plane 2 of the first y-range (see the plan; behind the
  // 8 x 4 planes of the wide scan), the hybrid scan's coefficients and verdicts in plane 0
  TabLaunch tl{st, st};
  double* d_tab = ws + (cp.wide ? 32 : 2) * npix;
  double* d_W = nullptr;
  int* d_ok = nullptr;
  float* d_E = nullptr;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusActive;
  bool ahead = RJP_TABLES_AHEAD && ring && ring->side && release_ev && cp.ni <= kChiMaxNI &&
               hipStreamIsCapturing(st, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone;
  if (ahead) {
    // a caller that waits for every step has nothing to overlap the tables with, and two streams
    // cost it two more hand-overs: the side stream is taken only while the previous scan of this
    // context is still enqueued or running
    const hipEvent_t prev = ring->slot[(ring->next + TabRing::kSlots - 1) % TabRing::kSlots].readers_done;
    ahead = prev && hipEventQuery(prev) == hipErrorNotReady;
    (void)hipGetLastError();             // (hipErrorNotReady is no error of this call)
  }
  if (ahead) {
    TabRing::Slot& s = ring->slot[ring->next];
    hipError_t e = s.readers_done ? hipStreamWaitEvent(ring->side, s.readers_done, 0) : hipSuccess;
    if (e == hipSuccess && stage_fresh && *stage_fresh) {
      e = hipEventRecord(s.uploaded, st);
      if (e == hipSuccess) e = hipStreamWaitEvent(ring->side, s.uploaded, 0);
      if (e == hipSuccess) *stage_fresh = false;
    }
    if (e != hipSuccess) return e;       // (nothing of this scan has been enqueued)
    tl.ts = ring->side;
    tl.slot = &s;
    d_tab = s.tab;
    d_W = s.W;
    d_ok = s.ok;
    d_E = s.E;
  }
  const hipError_t e = chi_table_scan_on(fl, cp, d_stage, t_epoch, mode, sumA, em, tavg, ws,
                                         work_bytes, d_guard, st, sp, tl, d_tab, d_W, d_ok, d_E);
  // on every path: the slot's kernels may be in flight, and the event the caller records behind
  // this scan (a failed launch included) has to cover them
  const hipError_t rel = tl.join();
  if (ring) {
    // the slot of this scan, taken or not: what the next call asks for is THIS scan's end
    ring->slot[ring->next].readers_done = release_ev;
    ring->next = (ring->next + 1) % TabRing::kSlots;
  }
  return e != hipSuccess ? e : rel;
}

static hipError_t chi_table_scan_on(const rjp_fields* fl, const ChiPlan& cp, const double* d_stage,
                                    double t_epoch, int mode, double* sumA, double* em,
                                    double* tavg, double* ws, size_t work_bytes, int* d_guard,
                                    hipStream_t st, const SrtPlan* sp, TabLaunch& tl,
                                    double* d_tab, double* d_W, int* d_ok, float* d_E) {
  const int64_t npix = (int64_t)fl->nx * fl->nz;
  const int64_t nchunks = npix / 2;
  const size_t tab_doubles = (size_t)2 * cp.ni * kChiStride;
  ChiTabDev t{cp.ni, cp.lo, cp.inv_h, std::nextafter((double)cp.ni, 0.0), fl->ts_lo, fl->ts_hi,
              d_guard};
  hipLaunchKernelGGL(chi_table_kernel, dim3((unsigned)((2 * cp.ni + 255) / 256)), dim3(256), 0,
                     tl.ts, d_stage, cp.n[0], cp.n[1], t, d_tab);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int64_t wgs = (nchunks + kBlock - 1) / kBlock;
  // never more y-ranges than the CALLER'S workspace holds (a workspace of rjp_ff_scan_workspace()
  // bytes holds them all; ADVICE r04: the rule used to be checked against nothing)
  int nsplit = chi_table_nsplit(npix, fl->ny, cp.wide);
  while (nsplit > 1 && (size_t)nsplit * nacc(1) * npix * sizeof(double) > work_bytes) nsplit /= 2;
  const int ylen = (fl->ny + nsplit - 1) / nsplit;
  const size_t shm = tab_doubles * sizeof(double);
  // em = sum (n x)^2 * csize*au/pc * pf  (classes.py:1116-1118)
  const double em_scale = fl->csize_au * 149597870700.0 / 3.085677581491367e+16;
  // (per context = per device: a context is bound to one device and used by one host thread)
  constexpr int kMaxShm = 2 * kChiMaxNI * kChiStride * (int)sizeof(double);
  if (!cp.attr_set) {
    e = hipFuncSetAttribute((const void*)ff_scan_table_wide_kernel<RJP_TAB_U_WIDE, 0>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, kMaxShm);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void*)ff_scan_table_wide_kernel<RJP_TAB_U_WIDE, 1>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, kMaxShm);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void*)ff_scan_table_kernel<RJP_TAB_U, false>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, kMaxShm);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void*)ff_scan_table_kernel<RJP_TAB_U_EM, true>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, kMaxShm);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void*)ff_scan_sorted_kernel<RJP_SRT_U>,
                            hipFuncAttributeMaxDynamicSharedMemorySize, kMaxShm);
    if (e != hipSuccess) return e;
    const void* hyb[3] = {(const void*)ff_scan_hybrid_kernel<RJP_SRT_U, 16>,
                          (const void*)ff_scan_hybrid_kernel<RJP_SRT_U, 20>,
                          (const void*)ff_scan_hybrid_kernel<RJP_SRT_U, 24>};
    for (const void* f : hyb) {
      e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize,
                              std::max(kMaxShm, (int)kSrtResidShm));
      if (e != hipSuccess) return e;
    }
    cp.attr_set = true;
  }
  if (sp && !cp.wide && !em) {
    // the launch-time-bucketed layout: sums straight to the map, no y-ranges
    const SrtDev s{(const rjp_d2*)fl->d_srt_cells, fl->d_srt_start, fl->d_srt_cum, fl->d_srt_rowbase,
                   fl->d_srt_aux, npix, fl->srt_K, {sp->b0[0], sp->b0[1]}, {sp->b1[0], sp->b1[1]},
                   {sp->hb[0], sp->hb[1]}};
    const int64_t groups = (npix + RJP_WAVE - 1) / RJP_WAVE;
    const int64_t per = kSrtBlock / RJP_WAVE;
    const dim3 sgrid((unsigned)((groups + per - 1) / per));
    if (sp->N == 0) {
      e = tl.join();
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL((ff_scan_sorted_kernel<RJP_SRT_U>), sgrid, dim3(kSrtBlock), shm, st, s, t,
                         t_epoch, (const double*)d_tab, sumA);
      return hipGetLastError();
    }
    // ... with the bins whose chi^2 the moments' interpolant matches contracted: the coefficients
    // and verdicts of every (jet, bin) go to the table slot, or in the single-stream order to
    // plane 0 of the workspace (unused by this scan)
    const int K = fl->srt_K, N = sp->N;
    // the scan reads the moment planes in 16-byte pairs of sightlines (n_z is even on this path)
    if ((npix & 1) || ((uintptr_t)fl->d_srt_mom % 16) != 0) return hipErrorInvalidValue;
    if (!d_W) {
      d_W = ws;
      d_ok = reinterpret_cast<int*>(ws + (size_t)2 * K * N);
      d_E = reinterpret_cast<float*>(ws + (size_t)2 * RJP_SRT_MAX_K * kSrtMaxN + RJP_SRT_MAX_K);
    }
    // table-residual bins: with the packed state attached, and only while the chi table and the
    // error table together leave the CU two workgroups -- else what fails (b) is read as before
    const size_t err_bytes = (size_t)2 * cp.ni * kErrStride * sizeof(float);
    const bool resid = RJP_SRT_RESID && sp->packed && ((uintptr_t)fl->d_srt_pts % 16) == 0 &&
                       ((uintptr_t)fl->d_srt_pw % 16) == 0 && shm + err_bytes <= kSrtResidShm;
    if (resid) {
      hipLaunchKernelGGL(srt_err_kernel, dim3((unsigned)((2 * cp.ni * 16 + 255) / 256)), dim3(256), 0,
                         tl.ts, d_stage, cp.n[0], cp.n[1], t, (const double*)d_tab, d_E);
      e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
    const float* dE = resid ? d_E : nullptr;
    const size_t hshm = shm + (resid ? err_bytes : 0);
    const SrtCoefDev c{fl->ts_lo, fl->ts_hi > fl->ts_lo ? K / (fl->ts_hi - fl->ts_lo) : 1.0, K, N,
                       {sp->b0[0], sp->b0[1]}, {sp->b1[0], sp->b1[1]}, d_W, d_ok};
    hipLaunchKernelGGL(srt_coef_kernel, dim3((unsigned)(2 * K)), dim3(kSrtCoefThreads), 0, tl.ts,
                       d_stage, cp.n[0], cp.n[1], t, t_epoch, (const double*)d_tab, dE, c);
    e = hipGetLastError();
    if (e == hipSuccess) e = tl.join();
    if (e != hipSuccess) return e;
    // ... from the launch-time codes when they are attached: A, B and 1/2 - mg of "the margin"
    const bool codes = RJP_SRT_CODES && resid && sp->codes && ((uintptr_t)fl->d_srt_pc % 16) == 0 &&
                       ((uintptr_t)fl->d_srt_cells % 16) == 0;
    const double cq = std::ldexp(fl->ts_hi - fl->ts_lo, -32);
    const double cB = cq * cp.inv_h;
    const double cA = (t_epoch - fl->ts_lo - cp.lo) * cp.inv_h - 0.5 * cB;
    const double Tm = std::fabs(t_epoch) + std::max(std::fabs(fl->ts_lo), std::fabs(fl->ts_hi)) +
                      std::fabs(cp.lo);
    const double mg = 2.0 * cB + std::ldexp(Tm * cp.inv_h, -48);
    const SrtMomDev m{fl->d_srt_mom, d_W, d_ok, sp->diag, dE, (const rjp_d2*)fl->d_srt_pts,
                      (const rjp_u4*)fl->d_srt_pw, codes ? (const rjp_u4*)fl->d_srt_pc : nullptr,
                      cA, cB, mg < 0.5 ? 0.5 - mg : -1.0};
    switch (N) {
      case 16:
        hipLaunchKernelGGL((ff_scan_hybrid_kernel<RJP_SRT_U, 16>), sgrid, dim3(kSrtBlock), hshm, st,
                           s, m, t, t_epoch, (const double*)d_tab, sumA);
        break;
      case 20:
        hipLaunchKernelGGL((ff_scan_hybrid_kernel<RJP_SRT_U, 20>), sgrid, dim3(kSrtBlock), hshm, st,
                           s, m, t, t_epoch, (const double*)d_tab, sumA);
        break;
      default:
        hipLaunchKernelGGL((ff_scan_hybrid_kernel<RJP_SRT_U, 24>), sgrid, dim3(kSrtBlock), hshm, st,
                           s, m, t, t_epoch, (const double*)d_tab, sumA);
        break;
    }
    return hipGetLastError();
  }
  const dim3 grid((unsigned)(wgs * nsplit));
  e = tl.join();
  if (e != hipSuccess) return e;
  if (cp.wide) {
    FieldPtrs<double> f{(const double*)fl->d_nd, (const double*)fl->d_xi, (const double*)fl->d_temp,
                        (const double*)fl->d_pf, (const double*)fl->d_ts, fl->d_ylo, fl->d_yhi,
                        nullptr, nullptr};
    if (mode == RJP_GFF_POWERLAW)
      hipLaunchKernelGGL((ff_scan_table_wide_kernel<RJP_TAB_U_WIDE, 1>), grid, dim3(kBlock), shm, st,
                         f, fl->ny, fl->nz, nchunks, npix, ylen, nsplit, t, t_epoch, d_tab, ws, sumA,
                         em, tavg, em_scale);
    else
      hipLaunchKernelGGL((ff_scan_table_wide_kernel<RJP_TAB_U_WIDE, 0>), grid, dim3(kBlock), shm, st,
                         f, fl->ny, fl->nz, nchunks, npix, ylen, nsplit, t, t_epoch, d_tab, ws, sumA,
                         em, tavg, em_scale);
    e = hipGetLastError();
    if (e != hipSuccess || nsplit == 1) return e;
    return ff_reduce_launch(ws, nsplit, 1, npix, 0, em_scale, sumA, em, tavg, st);
  }
  double* out = nsplit == 1 ? sumA : ws;
  const int64_t stride = nsplit == 1 ? 0 : (int64_t)nacc(1) * npix;
  if (em)
    hipLaunchKernelGGL((ff_scan_table_kernel<RJP_TAB_U_EM, true>), grid, dim3(kBlock), shm, st,
                       (const double*)fl->d_a0, (const double*)fl->d_em0, (const double*)fl->d_ts,
                       fl->d_ylo, fl->d_yhi, fl->ny, fl->nz, nchunks, npix, ylen, nsplit, t,
                       t_epoch, d_tab, out, stride, em, em_scale);
  else
    hipLaunchKernelGGL((ff_scan_table_kernel<RJP_TAB_U, false>), grid, dim3(kBlock), shm, st,
                       (const double*)fl->d_a0, (const double*)nullptr, (const double*)fl->d_ts,
                       fl->d_ylo, fl->d_yhi, fl->ny, fl->nz, nchunks, npix, ylen, nsplit, t,
                       t_epoch, d_tab, out, stride, (double*)nullptr, em_scale);
  e = hipGetLastError();
  if (e != hipSuccess || nsplit == 1) return e;
  return ff_reduce_launch(ws, nsplit, 1, npix, 0, em_scale, sumA, em, nullptr, st);
}

}  // namespace rjp
