// K9: sensitivities of the formal-solution light curves (K8, ff_formal_sweep.hip) to the burst
// parameters, exact, from the walk that forms the light curves themselves.
//
// One sightline, cells i front to back, one channel with c = ctau[f]:
//   b_i = |a0_i| chi_i^2,  dtau_i = c b_i,  om_i = 1 - e^-dtau_i,  Theta_i = exp(-sum_{j<i} dtau_j)
//   I = sum_i T_i om_i Theta_i                                                         (K5 / K8)
//   g_ik = db_i/dtheta_k (K7's three terms per burst of cell i's jet),  D_ik = sum_{j<i} g_jk
//   dI/dtheta_k = sum_i c T_i Theta_i [ e^-dtau_i g_ik - om_i D_ik ]
// -- raising a cell's opacity adds its own emission and hides what lies behind it.  Per cell:
//   dI_k += c T Theta (e^-dtau g_k - om D_k),  D_k += g_k,  then K8's update of I and Theta.
// The recurrence is linear in g, so K7's trick carries over: the walk accumulates with
// g = 2 |a0| chi G, g (d - t0) and g (d - t0)^2 and the per-burst constants (2 amp inv2s2, 1, -amp)
// are applied once per plane behind it.
//
// Layout: K8's (ff_formal.h) -- 16 z-adjacent sightlines of one x-row per workgroup, slabs of 16
// y-rows staged in LDS (signed a, T, ts), lanes over EPOCHS in blocks of 64 (four sightlines per
// thread; the cell, hence its jet, is wave-uniform) or 16 (one sightline per thread, four per
// wave), K8's tail rule.  Per lane the state is D_k (once per parameter, shared by the channels),
// dI[f][k], and K8's I / Theta -- too much for 48 parameters, so PARAMETERS GO TO WORKGROUPS in
// blocks of NB whole bursts of ONE jet (gridDim.y = channel blocks x burst blocks), as K8's
// channels beyond its register block do; a block's workgroups repeat chi and om.  Cells of the
// other jet have g = 0 for the block and still attenuate through om D.
// b, om, I and Theta come from the functions K5 and K8 call, chi from the same Gaussians in the
// same order as chi_jet, so the F totals (burst block 0, through K8's tile stage) equal K8's bit
// for bit.  The derivative keeps an attenuation of its own, the running PRODUCT of e^-dtau_i (one
// FMA beside om): K8's Theta (1 - om) loses Theta's relative accuracy behind a thick cell (om
// rounds to 1), which I does not notice and a derivative judged against its own terms would.
// Totals: K8's scheme, one partial per (epoch, channel, parameter, workgroup) in a fixed order,
// NaN pixels add nothing, sum_partials_launch finishes.  No floating-point atomics.  A call that
// asks for the F totals alone is K8's launch.
#include "ff_formal.h"

namespace rjp {

// The burst block of a workgroup: bursts [lo, lo + cnt) of jet `jet`; k0 = its first parameter.
struct GradBlock {
  int jet, lo, cnt, k0;
};
template <int NB>
__host__ __device__ __forceinline__ int grad_blocks(const int (&n)[2]) {
  return (n[0] + NB - 1) / NB + (n[1] + NB - 1) / NB;
}
template <int NB>
__device__ __forceinline__ GradBlock grad_block(const BurstsDev& bd, int blk) {
  const int nb0 = (bd.n[0] + NB - 1) / NB;
  GradBlock g;
  g.jet = blk < nb0 ? 0 : 1;
  g.lo = (g.jet ? blk - nb0 : blk) * NB;
  const int left = bd.n[g.jet] - g.lo;
  g.cnt = left < NB ? left : NB;
  g.k0 = 3 * ((g.jet ? bd.n[0] : 0) + g.lo);
  return g;
}

// per (sightline of the thread): the walk's state
template <int FC, int NB>
struct FormalGradAcc {
  double I[FC], Th[FC];            // K8's
  double At[FC];                   // prod e^-dtau: the derivative's attenuation
  double D[3][NB];                 // sum over the cells in front of g (d - t0), g, g (d - t0)^2
  double dI[FC][3][NB];
};

template <int LAY, int LE, int FC, int NB>
__global__ __launch_bounds__(kFB, 2) void ff_formal_grad_kernel(
    FormalFields<double> f, int nx, int ny, int nz, int mode, BurstsDev bd,
    const double* __restrict__ epochs, int e_lo, int e_hi, const double* __restrict__ ctau,
    const double* __restrict__ csrc, int nchan, const double* __restrict__ scale,
    double* __restrict__ fpart, double* __restrict__ dout, double* __restrict__ dpart) {
  using TL = FormalTile<LE>;
  constexpr int ZT = TL::ZT, YC = TL::YC, NZP = TL::NZP;
  static_assert(ZT % TL::G == 0 && ZT == 16, "tile/group mismatch");

  __shared__ rjp_d2 s_at[kFB];      // (signed a, T) of the slab's cells, [row * ZT + sightline]
  __shared__ double s_ts[kFB];      // their launch times
  __shared__ double s_x[LE * ZT];   // one plane's pixel values of the tile, [epoch lane][sightline]
  __shared__ int s_hot[ZT];         // the sightline has a cell with T > 0

  const FormalPlace<LE> pl(nz);
  const int x = pl.x, z0 = pl.z0, cy = pl.cy, cz = pl.cz, cb = pl.cb;
  const int tid = threadIdx.x;
  const int el = tid % LE;
  const int e_blk = e_lo + (int)blockIdx.z * LE;
  const int ei = e_blk + el;
  const double te = ei < e_hi ? epochs[ei] : 0.0;    // (a dead lane walks epoch 0 s and stores nothing)
  const int ncb = (nchan + FC - 1) / FC;
  const int bblk = (int)blockIdx.y / ncb;
  const int f0 = ((int)blockIdx.y - bblk * ncb) * FC;
  const int nf = nchan - f0 < FC ? nchan - f0 : FC;
  const GradBlock gb = grad_block<NB>(bd, bblk);
  const int npar = 3 * (bd.n[0] + bd.n[1]);
  double ct[FC];
#pragma unroll
  for (int k = 0; k < FC; ++k) ct[k] = k < nf ? ctau[f0 + k] : 0.0;

  if (tid < ZT) s_hot[tid] = 0;
  __syncthreads();
  int ya, ye;
  tile_y_range<ZT>(f.ylo, f.yhi, x, z0, nz, ny, ya, ye);

  FormalGradAcc<FC, NB> acc[NZP];
#pragma unroll
  for (int j = 0; j < NZP; ++j) {
#pragma unroll
    for (int k = 0; k < FC; ++k) {
      acc[j].I[k] = 0.0;
      acc[j].Th[k] = 1.0;
      acc[j].At[k] = 1.0;
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int t = 0; t < NB; ++t) acc[j].dI[k][c][t] = 0.0;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int t = 0; t < NB; ++t) acc[j].D[c][t] = 0.0;
  }

  for (int yb = ya; yb < ye; yb += YC) {
    // ---- phase 1: signed a, T and ts of one cell per thread ----------------------------------
    {
      rjp_d2 v;
      double ts;
      formal_stage_cell<double, LAY>(f, x, yb + cy, z0 + cz, ye, ny, nz, mode, &s_hot[cz], v, ts);
      s_at[tid] = v;
      s_ts[tid] = ts;
    }
    __syncthreads();

    // ---- phase 2: lanes over epochs, rows front to back ---------------------------------------
#pragma unroll 1
    for (int r = 0; r < YC; ++r) {
#pragma unroll
      for (int j = 0; j < NZP; ++j) {
        const int ci = r * ZT + cb + j;
        const rjp_d2 c = s_at[ci];
        if (!(c.x != 0.0)) continue;                  // a dead cell (wave-uniform for LE = 64)
        const double tsv = s_ts[ci];
        bool red;
        if constexpr (LE >= RJP_WAVE) red = (int)__builtin_amdgcn_readfirstlane(hi_dword(c.x)) < 0;
        else red = signbit_d(c.x);
        // nansum: a NaN a drops the cell; so does a NaN launch time, but only in a jet that has
        // bursts (chi = 1 otherwise).  A dropped cell gets weight 0 and a finite launch time, so
        // that every term it forms is an exact zero -- b = 0 as formal_live makes it.
        const bool tnan = !(tsv == tsv);
        const bool has = (red ? bd.n[0] : bd.n[1]) > 0;
        const double am = fabs(c.x);
        const double w = (am == am && !(has && tnan)) ? am : 0.0;
        const double tl = te - (tnan ? 0.0 : tsv);
        // chi as chi_jet adds it up (the same Gaussians in the same order); the block's own
        // Gaussians are kept, a Gaussian below 2^-1021 an exact zero in the derivative terms
        const bool mine = (red ? 0 : 1) == gb.jet;
        double chi = 1.0;
        double G[NB], dd[NB];
#pragma unroll
        for (int t = 0; t < NB; ++t) G[t] = dd[t] = 0.0;
        if (mine) {
          const int J = gb.jet;
          for (int i = 0; i < gb.lo; ++i)
            chi = __builtin_fma(bd.amp_rel[J][i], gauss2<false>(tl, bd.t0[J][i], bd.k2[J][i]), chi);
#pragma unroll
          for (int t = 0; t < NB; ++t) {
            if (t < gb.cnt) {
              const double t0 = bd.t0[J][gb.lo + t], k2 = bd.k2[J][gb.lo + t];
              dd[t] = tl - t0;
              const double ga = gauss2<false>(tl, t0, k2);
              chi = __builtin_fma(bd.amp_rel[J][gb.lo + t], ga, chi);
              G[t] = (dd[t] * dd[t]) * k2 < -1021.0 ? 0.0 : ga;
            }
          }
          for (int i = gb.lo + gb.cnt; i < bd.n[J]; ++i)
            chi = __builtin_fma(bd.amp_rel[J][i], gauss2<false>(tl, bd.t0[J][i], bd.k2[J][i]), chi);
        } else {
          chi = chi_jet(bd, 1 - gb.jet, tl);
        }
        const double b = formal_live(formal_weigh(w, chi));
        const double tk = formal_temp(b, c.y);
        const double f2 = (w + w) * chi;
        double g[3][NB];
#pragma unroll
        for (int t = 0; t < NB; ++t) {
          g[1][t] = f2 * G[t];
          g[0][t] = g[1][t] * dd[t];
          g[2][t] = g[0][t] * dd[t];
        }
        FormalGradAcc<FC, NB>& a = acc[j];
#pragma unroll
        for (int k = 0; k < FC; ++k) {
          if (k < nf) {
            double ex;
            const double om = one_minus_exp_neg(ct[k] * b, ex);
            const double wgt = (ct[k] * tk) * a.At[k];
            const double wa = wgt * ex, wb = -(wgt * om);
#pragma unroll
            for (int t = 0; t < NB; ++t) {
              if (t < gb.cnt) {
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                  double v = __builtin_fma(wb, a.D[q][t], a.dI[k][q][t]);
                  if (LE < RJP_WAVE || mine) v = __builtin_fma(wa, g[q][t], v);
                  a.dI[k][q][t] = v;
                }
              }
            }
            a.At[k] *= ex;
            formal_update(tk, om, a.I[k], a.Th[k]);
          }
        }
        if (LE < RJP_WAVE || mine) {
#pragma unroll
          for (int t = 0; t < NB; ++t)
#pragma unroll
            for (int q = 0; q < 3; ++q) a.D[q][t] += g[q][t];
        }
      }
    }
    __syncthreads();
  }

  // ---- the tile's planes and its share of the totals, one plane at a time ---------------------
  const int ne = e_hi - e_blk < LE ? e_hi - e_blk : LE;        // live epochs of this workgroup
  const int64_t npix = (int64_t)nx * nz;
  const int64_t nwg = gridDim.x;
#pragma unroll
  for (int k = 0; k < FC; ++k) {
    if (k < nf) {
      const double cs = csrc[f0 + k];
      const int64_t pl0 = (int64_t)e_blk * nchan + f0 + k;        // (epoch, channel) of the first lane
      if (fpart && bblk == 0) {
#pragma unroll
        for (int j = 0; j < NZP; ++j)
          s_x[el * ZT + cb + j] = formal_out(z0 + cb + j < nz && s_hot[cb + j], cs, acc[j].I[k]);
        __syncthreads();
        formal_tile_emit(s_x, ne, z0, nz, nullptr, 0, fpart + pl0 * nwg + blockIdx.x,
                         (int64_t)nchan * nwg);
      }
#pragma unroll
      for (int t = 0; t < NB; ++t) {
        if (t < gb.cnt) {
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const int kp = gb.k0 + 3 * t + q;
            const double sc = cs * scale[kp];
#pragma unroll
            for (int j = 0; j < NZP; ++j)
              s_x[el * ZT + cb + j] =
                  formal_out(z0 + cb + j < nz && s_hot[cb + j], sc, acc[j].dI[k][q][t]);
            __syncthreads();
            const int64_t pk = pl0 * npar + kp;
            formal_tile_emit(s_x, ne, z0, nz,
                             dout ? dout + pk * npix + (int64_t)x * nz + z0 : nullptr,
                             (int64_t)nchan * npar * npix,
                             dpart ? dpart + pk * nwg + blockIdx.x : nullptr,
                             (int64_t)nchan * npar * nwg);
          }
        }
      }
    }
  }
}

size_t ff_formal_grad_workspace_bytes(int nx, int nz, int n_epochs, int n_par, int n_chan) {
  // one partial per (epoch, channel, F or parameter, workgroup of 16 sightlines)
  const size_t nwg = (size_t)nx * (size_t)((nz + 15) / 16);
  return nwg * (size_t)n_epochs * (size_t)n_chan * (size_t)(n_par + 1) * sizeof(double) + 256;
}

namespace {

struct GradArgs {
  const rjp_fields* fl;
  int mode;
  BurstsDev b;
  const double* epochs;
  int n_epochs;
  const double *ctau, *csrc;
  int nchan;
  const double* scale;
  double *fpart, *dout, *dpart;
  hipStream_t st;
};

template <int LAY, int LE, int FC, int NB>
hipError_t fgrad_launch_t(const FormalFields<double>& f, const GradArgs& a, int e_lo, int e_hi) {
  const int ntz = (a.fl->nz + FormalTile<LE>::ZT - 1) / FormalTile<LE>::ZT;
  const dim3 grid((unsigned)((int64_t)a.fl->nx * ntz),
                  (unsigned)(((a.nchan + FC - 1) / FC) * grad_blocks<NB>(a.b.n)),
                  (unsigned)((e_hi - e_lo + LE - 1) / LE));
  hipLaunchKernelGGL((ff_formal_grad_kernel<LAY, LE, FC, NB>), grid, dim3(kFB), 0, a.st, f,
                     a.fl->nx, a.fl->ny, a.fl->nz, a.mode, a.b, a.epochs, e_lo, e_hi, a.ctau,
                     a.csrc, a.nchan, a.scale, a.fpart, a.dout, a.dpart);
  return hipGetLastError();
}

// The (channel block, burst block) per lane layout: the largest whose state stays in registers
// (DESIGN.md section 3, K9).  16 lanes, one sightline per thread: 1 x 8 (1 x 4 where no jet has
// more than four bursts), 2 x 4, 4 x 2.  64 lanes, four sightlines per thread: 1 x 2 (1 x 1 with
// one burst per jet at most), 2 x 1.
template <int LAY, int LE>
hipError_t fgrad_launch_blk(const FormalFields<double>& f, const GradArgs& a, int e_lo, int e_hi) {
  const int nmax = a.b.n[0] > a.b.n[1] ? a.b.n[0] : a.b.n[1];
  if constexpr (LE == 16) {
    if (a.nchan == 1)
      return nmax <= 4 ? fgrad_launch_t<LAY, LE, 1, 4>(f, a, e_lo, e_hi)
                       : fgrad_launch_t<LAY, LE, 1, 8>(f, a, e_lo, e_hi);
    if (a.nchan == 2) return fgrad_launch_t<LAY, LE, 2, 4>(f, a, e_lo, e_hi);
    return fgrad_launch_t<LAY, LE, 4, 2>(f, a, e_lo, e_hi);
  } else {
    if (a.nchan == 1)
      return nmax <= 1 ? fgrad_launch_t<LAY, LE, 1, 1>(f, a, e_lo, e_hi)
                       : fgrad_launch_t<LAY, LE, 1, 2>(f, a, e_lo, e_hi);
    return fgrad_launch_t<LAY, LE, 2, 1>(f, a, e_lo, e_hi);
  }
}

template <int LAY>
hipError_t fgrad_launch_le(const FormalFields<double>& f, const GradArgs& a) {
  const int n64 = formal_epochs64(a.n_epochs);
  if (n64 > 0) {
    const hipError_t e = fgrad_launch_blk<LAY, 64>(f, a, 0, n64);
    if (e != hipSuccess) return e;
  }
  if (n64 < a.n_epochs) return fgrad_launch_blk<LAY, 16>(f, a, n64, a.n_epochs);
  return hipSuccess;
}

}  // namespace

hipError_t ff_formal_grad_launch(const rjp_fields* fl, const rjp_bursts* hb,
                                 const double* d_epochs, int n_epochs, int mode,
                                 const double* d_ctau, const double* d_csrc, int nchan,
                                 const double* d_scale, double* ftot, double* dftot, double* dout,
                                 double* work, hipStream_t st) {
  if (fl->dtype != RJP_F64 || !fl->d_ts) return hipErrorInvalidValue;
  // the totals alone are K8's call (at most 8 bursts per jet: no overflow table)
  if (!dftot && !dout)
    return ff_formal_sweep_launch(fl, hb, nullptr, d_epochs, n_epochs, mode, d_ctau, d_csrc, nchan,
                                  nullptr, ftot, work, st);
  GradArgs a{fl, mode, {}, d_epochs, n_epochs, d_ctau, d_csrc, nchan, d_scale, nullptr, dout,
             nullptr, st};
  if (!bursts_to_dev(hb, a.b)) return hipErrorInvalidValue;
  const int npar = 3 * (a.b.n[0] + a.b.n[1]);
  const int nwg = fl->nx * ((fl->nz + 15) / 16);
  // work: [E * F][nwg] for F, then [E * F * npar][nwg]
  if (ftot) a.fpart = work;
  if (dftot) a.dpart = work + (size_t)n_epochs * nchan * nwg;
  hipError_t e = formal_dispatch(fl, mode, fl->d_ts, [&](const auto& f, auto lay) {
    using T = typename std::decay_t<decltype(f)>::value_type;
    if constexpr (std::is_same<T, double>::value) return fgrad_launch_le<decltype(lay)::value>(f, a);
    else return hipErrorInvalidValue;
  });
  if (e != hipSuccess) return e;
  if (ftot && (e = sum_partials_launch(a.fpart, n_epochs * nchan, nwg, ftot, st)) != hipSuccess)
    return e;
  if (dftot) return sum_partials_launch(a.dpart, n_epochs * nchan * npar, nwg, dftot, st);
  return hipSuccess;
}

}  // namespace rjp
