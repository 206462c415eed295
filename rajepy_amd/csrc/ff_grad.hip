// K7: sensitivities of the free-free optical-depth sums and light curves to the burst parameters.
//
// The scans return S[e, p] = sum_y |a0| chi^2 with chi = 1 + sum_b amp_b G_b,
// G_b = exp(-(d - t0_b)^2 kappa_b), d = t_e - ts, over the bursts of the cell's jet
// (classes.py:861-875, 1395-1432).  A fit of (t0, amp_rel, inv2s2) needs the derivatives as well,
// and they are sums over the very Gaussians the scan evaluates:
//   dS/dt0_b      = sum_y |a0| 2 chi amp_b G_b 2 kappa_b (d - t0_b)
//   dS/damp_rel_b = sum_y |a0| 2 chi G_b
//   dS/dinv2s2_b  = sum_y |a0| 2 chi amp_b G_b (-(d - t0_b)^2)
// over the cells of burst b's jet.  ff_grad_kernel makes ONE pass over the tau layout (a0 with the
// jet flag in its sign bit, ts) per tile of epochs and keeps S and the three sums of every burst of
// BOTH jets in registers (a sightline may hold cells of either jet).  The per-burst constants
// 2 amp kappa and -amp are applied once per plane by the reduction of the y-range partials, so the
// loop accumulates g = 2 |a0| chi G, g (d - t0) and g (d - t0)^2: five FP64 instructions per
// (cell, epoch, burst) behind the Gaussian.  Lanes are adjacent along z as in K1; the y-range is
// split over workgroups on small maps and the partial planes are summed in a fixed order: no
// floating-point atomics, results reproducible bit for bit.
//
// Semantics: nansum as in the scans (a NaN a0, or a NaN launch time in a jet that has bursts,
// drops the cell); a jet WITHOUT bursts has chi = 1 whatever the launch time (classes.py:232-233):
// its cells add |a0| to S and nothing else -- the kernel applies that rule per jet itself, no
// patched launch-time copy is needed.  A Gaussian below 2^-1021 (the smallest the scans' exp2
// forms) counts as exactly zero.  a0 finite or NaN; negative amplitudes are fine.
//
// ff_grad_totals_kernel turns one tile's planes into the light curves and their Jacobian,
//   F[e, f]          = sum_p cflux[f] tavg[p] (1 - exp(-ctau[f] S[e, p]))          (classes.py:1519-1521)
//   dF[e, f]/dtheta_k = sum_p cflux[f] tavg[p] ctau[f] exp(-ctau[f] S[e, p]) dS[e, p]/dtheta_k,
// the weight once per (pixel, channel), n_par FMAs behind it, per-wave partials summed in a
// fixed order by ff_grad_sum_kernel.
#include <algorithm>

#include "ff_scan_kernels.h"

namespace rjp {

// ---- the pass over the grid ------------------------------------------------------------------
template <int ET>
struct GradEpochs {
  double t[ET];
};

// per-lane accumulators of one sightline and epoch: S and, per burst slot of either jet,
// sum g, sum g dd, sum g dd^2
template <int NBS>
struct GradAcc {
  double s;
  double g[2][NBS], g1[2][NBS], g2[2][NBS];
};

constexpr int kGradU = 2;        // y-rows of loads in flight per lane (the pass is FP64-bound)

// One cell at one epoch, straight-line code for NACT burst slots (a slot beyond the jet's count has
// amp = 0: it leaves chi alone and its sums are never written out).  MIXED = false: every lane of
// the wave sits in jet JET (parameters are wave-uniform, SGPR operands); MIXED = true: the wave
// straddles, parameters selected per lane and the terms added to the lane's own jet (the other
// jet's accumulators get an exact zero).
template <int NBS, int NACT, bool MIXED, int JET>
__device__ __forceinline__ void grad_cell(const BurstsDev& b, double w, double d, bool red,
                                          GradAcc<NBS>& acc) {
  static_assert(NACT <= NBS, "active slots");
  double G[NACT > 0 ? NACT : 1], dd[NACT > 0 ? NACT : 1];
  double chi = 1.0;
#pragma unroll
  for (int i = 0; i < NACT; ++i) {
    const double t0 = MIXED ? (red ? b.t0[0][i] : b.t0[1][i]) : b.t0[JET][i];
    const double k2 = MIXED ? (red ? b.k2[0][i] : b.k2[1][i]) : b.k2[JET][i];
    const double amp = MIXED ? (red ? b.amp_rel[0][i] : b.amp_rel[1][i]) : b.amp_rel[JET][i];
    dd[i] = d - t0;
    const double ga = gauss2<false>(d, t0, k2);
    G[i] = (dd[i] * dd[i]) * k2 < -1021.0 ? 0.0 : ga;
    chi = __builtin_fma(amp, G[i], chi);
  }
  acc.s = __builtin_fma(w, chi * chi, acc.s);
  const double f = (w + w) * chi;
#pragma unroll
  for (int i = 0; i < NACT; ++i) {
    const double g = f * G[i];
    const double h = g * dd[i];
    const double q = h * dd[i];
    if (MIXED) {
      acc.g[0][i] += red ? g : 0.0;
      acc.g1[0][i] += red ? h : 0.0;
      acc.g2[0][i] += red ? q : 0.0;
      acc.g[1][i] += red ? 0.0 : g;
      acc.g1[1][i] += red ? 0.0 : h;
      acc.g2[1][i] += red ? 0.0 : q;
    } else {
      acc.g[JET][i] += g;
      acc.g1[JET][i] += h;
      acc.g2[JET][i] += q;
    }
  }
}

// U rows x VEC sightlines of one lane at the ET epochs of the tile, on one code path
template <int NBS, int ET, int VEC, int U, int NACT, bool MIXED, int JET>
__device__ __forceinline__ void grad_batch(const double (&a)[U][VEC], const double (&ts)[U][VEC],
                                           const BurstsDev& b, const GradEpochs<ET>& ep,
                                           GradAcc<NBS> (&acc)[ET][VEC]) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const bool red = MIXED ? signbit_d(a[u][v]) : JET == 0;
      const bool has = MIXED ? (red ? b.n[0] : b.n[1]) > 0 : NACT > 0;
      const double am = fabs(a[u][v]);
      const double tl = ts[u][v];
      // nansum: a NaN a0 drops the cell; so does a NaN launch time, but only in a jet that has
      // bursts (chi = 1 otherwise).  A dropped cell gets weight 0 and a finite launch time, so
      // that every term it forms is an exact zero.
      const bool tnan = !(tl == tl);
      const double w = (am == am && !(has && tnan)) ? am : 0.0;
      const double tsafe = tnan ? 0.0 : tl;
#pragma unroll
      for (int e = 0; e < ET; ++e)
        grad_cell<NBS, NACT, MIXED, JET>(b, w, ep.t[e] - tsafe, red, acc[e][v]);
    }
}

// a wave inside jet JET: the variant for the slots that jet's bursts fill (wave-uniform choice)
template <int NBS, int ET, int VEC, int U, int JET>
__device__ __forceinline__ void grad_batch_jet(const double (&a)[U][VEC],
                                               const double (&ts)[U][VEC], const BurstsDev& b,
                                               const GradEpochs<ET>& ep,
                                               GradAcc<NBS> (&acc)[ET][VEC]) {
  const int n = b.n[JET];
  if (n == 0) return grad_batch<NBS, ET, VEC, U, 0, false, JET>(a, ts, b, ep, acc);
  if (NBS == 1 || n == 1) return grad_batch<NBS, ET, VEC, U, 1, false, JET>(a, ts, b, ep, acc);
  if constexpr (NBS >= 2) {
    if (NBS == 2 || n == 2) return grad_batch<NBS, ET, VEC, U, 2, false, JET>(a, ts, b, ep, acc);
  }
  if constexpr (NBS >= 4) {
    if (NBS == 4 || n <= 4) return grad_batch<NBS, ET, VEC, U, 4, false, JET>(a, ts, b, ep, acc);
  }
  if constexpr (NBS >= 8) return grad_batch<NBS, ET, VEC, U, 8, false, JET>(a, ts, b, ep, acc);
}

template <int NBS, int ET, int VEC, int U>
__device__ __forceinline__ void grad_rows(const double* __restrict__ a0p,
                                          const double* __restrict__ tsp, int64_t off,
                                          int64_t stride, const BurstsDev& b,
                                          const GradEpochs<ET>& ep, GradAcc<NBS> (&acc)[ET][VEC]) {
  double a[U][VEC], ts[U][VEC];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    load_vec(a0p + off + u * stride, a[u]);
    load_vec(tsp + off + u * stride, ts[u]);
  }
  // which jets the wave's cells of this batch belong to (bit 31 of a0's high dword = red): a wave
  // inside one jet reads that jet's parameters wave-uniformly, as chi_batch does
  uint32_t wor = 0u, wand = 0xffffffffu;
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      // (a NaN cell -- outside the jet -- carries no jet: it must not make the wave straddle)
      const bool live = a[u][v] == a[u][v];
      wor |= live ? hi_dword(a[u][v]) : 0u;
      wand &= live ? hi_dword(a[u][v]) : 0xffffffffu;
    }
  const bool wave_red = __builtin_amdgcn_ballot_w64((int)wor < 0) != 0;
  const bool wave_blue = __builtin_amdgcn_ballot_w64((int)wand >= 0) != 0;
  if (wave_red && wave_blue) grad_batch<NBS, ET, VEC, U, NBS, true, 0>(a, ts, b, ep, acc);
  else if (wave_red) grad_batch_jet<NBS, ET, VEC, U, 0>(a, ts, b, ep, acc);
  else grad_batch_jet<NBS, ET, VEC, U, 1>(a, ts, b, ep, acc);
}

// Partial planes of one tile: ws[split][e * (1 + npar) + q][pixel], q = 0: S, q = 1 + 3 b + c for
// burst b (the red jet's first, then the blue jet's) and c = 0 t0, 1 amp_rel, 2 inv2s2 -- still
// without the per-burst constants (grad_reduce_kernel applies them).
template <int NBS, int ET, int VEC>
__global__ __launch_bounds__(kBlock) void ff_grad_kernel(
    const double* __restrict__ a0p, const double* __restrict__ tsp,
    const int32_t* __restrict__ ylo, const int32_t* __restrict__ yhi, int ny, int nz,
    int64_t nchunks, int64_t npix, int ylen, int nsplit, BurstsDev b, GradEpochs<ET> ep,
    double* __restrict__ ws) {
  const LaneRange lr = lane_y_range<VEC, kBlock>(nsplit, ylen, ny, nchunks, ylo, yhi);
  if (!lr.live) return;
  const int split = lr.split, y0 = lr.y0, y1 = lr.y1;
  const int64_t p0 = lr.p0;
  const int64_t x = p0 / nz;
  const int z = (int)(p0 - x * nz);

  GradAcc<NBS> acc[ET][VEC];
#pragma unroll
  for (int e = 0; e < ET; ++e)
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      acc[e][v].s = 0.0;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < NBS; ++i) acc[e][v].g[j][i] = acc[e][v].g1[j][i] = acc[e][v].g2[j][i] = 0.0;
    }

  int64_t off = (x * ny + y0) * (int64_t)nz + z;
  const int64_t stride = nz;
  int y = y0;
  for (; y + kGradU <= y1; y += kGradU) {
    grad_rows<NBS, ET, VEC, kGradU>(a0p, tsp, off, stride, b, ep, acc);
    off += kGradU * stride;
  }
  for (; y < y1; ++y) {
    grad_rows<NBS, ET, VEC, 1>(a0p, tsp, off, stride, b, ep, acc);
    off += stride;
  }

  const int npar = 3 * (b.n[0] + b.n[1]);
  double* w = ws + (int64_t)split * ET * (1 + npar) * npix + p0;
#pragma unroll
  for (int e = 0; e < ET; ++e) {
    double* we = w + (int64_t)e * (1 + npar) * npix;
#pragma unroll
    for (int v = 0; v < VEC; ++v) we[v] = acc[e][v].s;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < NBS; ++i) {
        if (i < b.n[j]) {
          const int k = 3 * ((j ? b.n[0] : 0) + i);
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            we[(int64_t)(1 + k) * npix + v] = acc[e][v].g1[j][i];
            we[(int64_t)(2 + k) * npix + v] = acc[e][v].g[j][i];
            we[(int64_t)(3 + k) * npix + v] = acc[e][v].g2[j][i];
          }
        }
      }
  }
}

// Fixed-order reduction over the y-ranges of one tile; applies the per-burst constants
// (scale[q], scale[0] = 1) and writes the tile's planes tb[e * (1 + npar) + q][pixel] for the
// totals stage and, where asked for, the caller's maps of epochs [e0, e0 + et).
__global__ __launch_bounds__(kBlock) void grad_reduce_kernel(
    const double* __restrict__ ws, int nsplit, int et, int npar, int64_t npix, int e0,
    const double* __restrict__ scale, double* __restrict__ tb, double* __restrict__ sumA,
    double* __restrict__ dsumA) {
  const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (p >= npix) return;
  const int nq = 1 + npar;
  for (int r = 0; r < et * nq; ++r) {
    double a = 0.0;
    for (int s = 0; s < nsplit; ++s) a += ws[((int64_t)s * et * nq + r) * npix + p];
    const int e = r / nq, q = r - e * nq;
    a *= scale[q];
    tb[(int64_t)r * npix + p] = a;
    if (q == 0) {
      if (sumA) sumA[(int64_t)(e0 + e) * npix + p] = a;
    } else if (dsumA) {
      dsumA[((int64_t)(e0 + e) * npar + (q - 1)) * npix + p] = a;
    }
  }
}

// ---- the light curves and their Jacobian -------------------------------------------------------
// One thread per pixel (kGradKP groups per thread), FC channels x up to KMAX parameters of
// accumulators in registers: FC * KMAX = 48.  Per (pixel, channel): 1 - e^-tau exactly as
// ff_ftot_kernel forms it, the weight cflux tavg ctau e^-tau once, then one FMA per parameter.
// part[((e * nchan + f) * (1 + npar) + q) * nparts + slot], q = 0: F, q = 1 + k: dF/dtheta_k.
constexpr int kGradKP = 4;

// e^x = m 2^k for -1400 <= x <= 0 (smaller x counts as -1400), m in [0.7, 1.42]: exp_any's
// reduction and polynomial without the final ldexp.  A thick pixel's weight e^-tau may lie below
// the smallest double while its product with a derivative sum of 1e25 does not, and the totals are
// judged relative to their own size: the caller keeps the power of two apart.
__device__ __forceinline__ double exp_split(double x, int& k) {
  const double L2E = 1.4426950408889634074;
  const double LN2_HI = 6.93147180369123816490e-01;
  const double LN2_LO = 1.90821492927058770002e-10;
  x = fmax(x, -1400.0);
  const double kd = __builtin_rint(x * L2E);
  double r = __builtin_fma(-kd, LN2_HI, x);
  r = __builtin_fma(-kd, LN2_LO, r);
  double p = RJP_EXP_C10;
  p = __builtin_fma(p, r, RJP_EXP_C9);
  p = __builtin_fma(p, r, RJP_EXP_C8);
  p = __builtin_fma(p, r, RJP_EXP_C7);
  p = __builtin_fma(p, r, RJP_EXP_C6);
  p = __builtin_fma(p, r, RJP_EXP_C5);
  p = __builtin_fma(p, r, RJP_EXP_C4);
  p = __builtin_fma(p, r, RJP_EXP_C3);
  p = __builtin_fma(p, r, 0.5);
  p = __builtin_fma(p, r, 1.0);
  p = __builtin_fma(p, r, 1.0);
  k = (int)kd;
  return p;
}

template <int KMAX>
__global__ __launch_bounds__(kBlock) void ff_grad_totals_kernel(
    const double* __restrict__ tb, const double* __restrict__ tavg, int64_t npix, int npar,
    const double* __restrict__ ctau, const double* __restrict__ cflux, int nchan, int e0,
    double* __restrict__ part, int nparts) {
  constexpr int FC = 48 / KMAX;
  const int e = blockIdx.y;
  const int f0 = blockIdx.z * FC;
  const int nf = min(nchan - f0, FC);
  const int nq = 1 + npar;
  const double* __restrict__ te = tb + (int64_t)e * nq * npix;
  double accF[FC], acc[FC][KMAX];
#pragma unroll
  for (int j = 0; j < FC; ++j) {
    accF[j] = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[j][k] = 0.0;
  }
#pragma unroll 1
  for (int g = 0; g < kGradKP; ++g) {
    const int64_t p = ((int64_t)blockIdx.x * kGradKP + g) * kBlock + threadIdx.x;
    if (p >= npix) continue;
    const double A = te[p];
    double ta = tavg[p];
    ta = ta == ta ? ta : 0.0;          // nansum: an empty sightline adds zero to every total
    double dS[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) dS[k] = k < npar ? te[(int64_t)(1 + k) * npix + p] : 0.0;
#pragma unroll
    for (int j = 0; j < FC; ++j) {
      if (j < nf) {
        const double ct = ctau[f0 + j], cf = cflux[f0 + j];
        const double tau = ct * A;
        accF[j] = __builtin_fma(cf * ta, one_minus_exp_neg(tau), accF[j]);
        // weight = cf ta ct e^-tau = wm 2^kw.  Below 2^-512 half of the power of two goes to the
        // derivative sums instead, so that neither factor underflows where the product does not
        int kw;
        const double wm = (cf * ta) * (ct * exp_split(-tau, kw));
        const bool deep = kw < -512;
        const double wgt = __builtin_ldexp(wm, deep ? kw + 512 : kw);
        const double ds = deep ? 0x1p-512 : 1.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < npar) acc[j][k] = __builtin_fma(wgt, dS[k] * ds, acc[j][k]);
      }
    }
  }
  const int slot = blockIdx.x * (kBlock / RJP_WAVE) + threadIdx.x / RJP_WAVE;
  const bool lead = (threadIdx.x & (RJP_WAVE - 1)) == 0;
#pragma unroll
  for (int j = 0; j < FC; ++j) {
    if (j < nf) {
      double* row = part + ((int64_t)((e0 + e) * nchan + f0 + j) * nq) * nparts + slot;
      double a = accF[j];
#pragma unroll
      for (int d = RJP_WAVE / 2; d > 0; d >>= 1) a += __shfl_down(a, d, RJP_WAVE);
      if (lead) row[0] = a;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if (k < npar) {
          double v = acc[j][k];
#pragma unroll
          for (int d = RJP_WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d, RJP_WAVE);
          if (lead) row[(int64_t)(1 + k) * nparts] = v;
        }
      }
    }
  }
}

// sums the per-wave partials of one (epoch, channel, q) in a fixed order (as sum_partials_kernel)
// into ftot[e * nchan + f] (q = 0) or dftot[(e * nchan + f) * npar + q - 1]
__global__ __launch_bounds__(kBlock) void ff_grad_sum_kernel(const double* __restrict__ part,
                                                             int nparts, int npar,
                                                             double* __restrict__ ftot,
                                                             double* __restrict__ dftot) {
  const int64_t row = blockIdx.x;
  const int nq = 1 + npar;
  const int64_t ef = row / nq;
  const int q = (int)(row - ef * nq);
  double* dst = q == 0 ? (ftot ? ftot + ef : nullptr) : (dftot ? dftot + ef * npar + (q - 1) : nullptr);
  if (!dst) return;                     // (uniform over the workgroup)
  double v = 0.0;
  for (int i = threadIdx.x; i < nparts; i += kBlock) v += part[row * nparts + i];
  __shared__ double red[kBlock / RJP_WAVE];
#pragma unroll
  for (int d = RJP_WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d, RJP_WAVE);
  if ((threadIdx.x & (RJP_WAVE - 1)) == 0) red[threadIdx.x / RJP_WAVE] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int w = 0; w < kBlock / RJP_WAVE; ++w) tot += red[w];
    *dst = tot;
  }
}

// ---- host ---------------------------------------------------------------------------------------
// burst slots per jet the kernels are instantiated for, and the largest epoch tile whose
// accumulators (ET * VEC * (1 + 6 NBS) doubles per lane) stay in registers
static int grad_slots(int nmax) { return nmax <= 1 ? 1 : nmax <= 2 ? 2 : nmax <= 4 ? 4 : 8; }
static int grad_tile_max(int nbs) { return nbs <= 2 ? 4 : nbs == 4 ? 2 : 1; }
// two sightlines per lane (16-byte loads) where the budget admits them beside the tile
static bool grad_vec2_fits(int nbs, int et) { return 2 * et * (1 + 6 * nbs) <= 56; }

static int grad_ysplit(int64_t nchunks, int ny) {
  const int64_t waves = (nchunks + RJP_WAVE - 1) / RJP_WAVE;
  int64_t s = (2048 + waves - 1) / waves;
  const int64_t smax = std::max(1, ny / 8);
  if (s > smax) s = smax;
  return (int)(s < 1 ? 1 : s);
}

static int64_t grad_nparts(int64_t npix) {
  const int64_t nb = (npix + (int64_t)kBlock * kGradKP - 1) / ((int64_t)kBlock * kGradKP);
  return nb * (kBlock / RJP_WAVE);
}

// doubles of the three workspace areas for a tile of `et` epochs
struct GradLayout {
  size_t part, tile, tot;
  size_t bytes() const { return (part + tile + tot) * sizeof(double) + 256; }
};
static GradLayout grad_layout(int64_t npix, int ny, int et, int nsplit, int n_epochs, int npar,
                              int nchan) {
  (void)ny;
  GradLayout L;
  L.tile = (size_t)et * (1 + npar) * npix;
  L.part = L.tile * (size_t)nsplit;
  L.tot = nchan > 0 ? (size_t)n_epochs * nchan * (1 + npar) * grad_nparts(npix) : 0;
  return L;
}

size_t ff_grad_workspace_bytes(int nx, int ny, int nz, int n_epochs, int npar, int nchan) {
  const int64_t npix = (int64_t)nx * nz;
  // the tile depends on the larger jet's burst count, of which only the sum is known here: the
  // largest tile any split of npar / 3 bursts over the two jets can take
  const int nb = npar / 3;
  const int etmax = std::min(n_epochs, nb > 8 ? 1 : nb > 4 ? 2 : 4);
  const int split = std::max(grad_ysplit(npix, ny), grad_ysplit(std::max<int64_t>(1, npix / 2), ny));
  return grad_layout(npix, ny, etmax, split, n_epochs, npar, nchan).bytes();
}

template <int NBS, int ET, int VEC>
static hipError_t grad_launch_t(const rjp_fields* fl, const BurstsDev& b, const double* t,
                                int nsplit, int ylen, double* ws, hipStream_t st) {
  const int64_t npix = (int64_t)fl->nx * fl->nz;
  const int64_t nchunks = npix / VEC;
  GradEpochs<ET> ep;
  for (int e = 0; e < ET; ++e) ep.t[e] = t[e];
  const unsigned nblk = (unsigned)((nchunks + kBlock - 1) / kBlock) * (unsigned)nsplit;
  hipLaunchKernelGGL((ff_grad_kernel<NBS, ET, VEC>), dim3(nblk), dim3(kBlock), 0, st,
                     (const double*)fl->d_a0, (const double*)fl->d_ts, fl->d_ylo, fl->d_yhi,
                     fl->ny, fl->nz, nchunks, npix, ylen, nsplit, b, ep, ws);
  return hipGetLastError();
}

template <int NBS>
static hipError_t grad_launch_nbs(int et, int vec, const rjp_fields* fl, const BurstsDev& b,
                                  const double* t, int nsplit, int ylen, double* ws,
                                  hipStream_t st) {
#define RJP_GRAD_CASE(E_, V_)                                                         \
  if constexpr (E_ <= (NBS <= 2 ? 4 : NBS == 4 ? 2 : 1) &&                            \
                (V_ == 1 || 2 * E_ * (1 + 6 * NBS) <= 56))                            \
    if (et == E_ && vec == V_) return grad_launch_t<NBS, E_, V_>(fl, b, t, nsplit, ylen, ws, st);
  RJP_GRAD_CASE(1, 1) RJP_GRAD_CASE(2, 1) RJP_GRAD_CASE(4, 1)
  RJP_GRAD_CASE(1, 2) RJP_GRAD_CASE(2, 2) RJP_GRAD_CASE(4, 2)
#undef RJP_GRAD_CASE
  return hipErrorInvalidValue;
}

hipError_t ff_grad_run(const rjp_fields* fl, const rjp_bursts* hb, const double* epochs,
                       int n_epochs, const double* d_scale, const double* d_tavg,
                       const double* d_ctau, const double* d_cflux, int nchan, double* sumA,
                       double* dsumA, double* ftot, double* dftot, double* ws, size_t work_bytes,
                       hipStream_t st) {
  BurstsDev b;
  bursts_to_dev(hb, b);
  const int npar = 3 * (b.n[0] + b.n[1]);
  const int nbs = grad_slots(std::max(b.n[0], b.n[1]));
  const int64_t npix = (int64_t)fl->nx * fl->nz;
  const bool totals = ftot || dftot;
  const bool vec2_ok = ff_scan_vec(fl) == 2;
  const int64_t nparts = grad_nparts(npix);
  int e0 = 0;
  while (e0 < n_epochs) {
    int et = grad_tile_max(nbs);
    while (et > n_epochs - e0) et /= 2;
    const int vec = vec2_ok && grad_vec2_fits(nbs, et) ? 2 : 1;
    const int nsplit = grad_ysplit(npix / vec, fl->ny);
    const int ylen = (fl->ny + nsplit - 1) / nsplit;
    const GradLayout L = grad_layout(npix, fl->ny, et, nsplit, n_epochs, npar, totals ? nchan : 0);
    if (L.bytes() > work_bytes) return hipErrorInvalidValue;     // (rjp_ff_grad checked the bound)
    double* tpart = ws;                    // (first: the same place for every tile)
    double* part = ws + L.tot;
    double* tile = part + L.part;
    hipError_t err;
    switch (nbs) {
      case 1: err = grad_launch_nbs<1>(et, vec, fl, b, epochs + e0, nsplit, ylen, part, st); break;
      case 2: err = grad_launch_nbs<2>(et, vec, fl, b, epochs + e0, nsplit, ylen, part, st); break;
      case 4: err = grad_launch_nbs<4>(et, vec, fl, b, epochs + e0, nsplit, ylen, part, st); break;
      default: err = grad_launch_nbs<8>(et, vec, fl, b, epochs + e0, nsplit, ylen, part, st); break;
    }
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(grad_reduce_kernel, dim3((unsigned)((npix + kBlock - 1) / kBlock)),
                       dim3(kBlock), 0, st, part, nsplit, et, npar, npix, e0, d_scale, tile, sumA,
                       dsumA);
    if ((err = hipGetLastError()) != hipSuccess) return err;
    if (totals) {
      const int kmax = npar <= 6 ? 6 : npar <= 12 ? 12 : npar <= 24 ? 24 : 48;
      const int fc = 48 / kmax;
      const dim3 g((unsigned)(nparts / (kBlock / RJP_WAVE)), (unsigned)et,
                   (unsigned)((nchan + fc - 1) / fc));
#define RJP_GRAD_TOT(K_)                                                                          \
  hipLaunchKernelGGL(ff_grad_totals_kernel<K_>, g, dim3(kBlock), 0, st, tile, d_tavg, npix, npar, \
                     d_ctau, d_cflux, nchan, e0, tpart, (int)nparts)
      if (kmax == 6) RJP_GRAD_TOT(6);
      else if (kmax == 12) RJP_GRAD_TOT(12);
      else if (kmax == 24) RJP_GRAD_TOT(24);
      else RJP_GRAD_TOT(48);
#undef RJP_GRAD_TOT
      if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    e0 += et;
  }
  if (totals) {
    hipLaunchKernelGGL(ff_grad_sum_kernel, dim3((unsigned)(n_epochs * nchan * (1 + npar))),
                       dim3(kBlock), 0, st, ws, (int)nparts, npar, ftot, dftot);
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace rjp
