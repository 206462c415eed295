// K5: free-free intensity by the formal solution of the transfer equation along the line of sight.
//
// The reference's map stage is isothermal: S = c_S[f] T_avg (1 - e^-tau) with T_avg the nanmean of
// the sightline's T > 0 (classes.py:1466-1475; K2 here), exact only where T is constant along the
// sightline.  This kernel sums the emission of every cell attenuated by the cells in front of it:
//   out[f, p] = csrc[f] sum_i T_i (1 - e^-dtau_i) exp(-sum_{j in front of i} dtau_j),
//   dtau_i = ctau[f] b_i,  b_i = |a0_i| chi_i^2
// with a0 and chi exactly as the tau scans form them (tau, compact and wide layouts give the same
// b bit for bit in f64) and the observer at the iy = 0 end of axis 1: the reference's Doppler shift
// is nu0 (1 - v/c) (physics.py:557-558), so gas with vel[1] > 0 recedes, i.e. lies behind.  With a
// constant T the sum telescopes to T (1 - e^-tau): the isothermal maps are a special case.  A cell
// contributes exactly when its term enters the tau scans' nansum (b == 0 / NaN: skipped); the
// output is NaN exactly where T_avg is (no cell of the sightline has T > 0).
//
// A 256-thread workgroup owns ZT z-adjacent sightlines of one x-row and a block of LF channels
// (lanes over channels, G = 256 / LF sightline groups; FormalTile / FormalPlace in ff_formal.h,
// which K8 shares together with the recurrence and the rules for dead cells and empty sightlines):
//   phase 1  one thread per cell of a slab of YC y-rows: b and T to LDS;
//   phase 2  every lane walks the slab's rows in increasing iy for its NZP sightlines:
//            om = 1 - e^(-ctau b), I += T om Theta, Theta -= Theta om (two FMAs), with b and T
//            LDS broadcasts.  A row whose cells are all dead is skipped (wave-uniform for LF >= 64).
// Compute-bound (vector FP64): ~26 instructions per (cell, channel) update, 21 of them in
// one_minus_exp_neg (relative error < 4e-15 for every tau); HBM traffic is 3 fields per cell
// (a0, temp, ts on the tau layout) once per channel block.
#include "ff_formal.h"

namespace rjp {

template <typename T, int LAY, int LF, bool BURSTS>
__global__ __launch_bounds__(kFB, RJP_FORMAL_WAVES) void ff_formal_kernel(
    FormalFields<T> f, int nx, int ny, int nz, int mode, BurstsDev bd, double time_s,
    const double* __restrict__ ctau, const double* __restrict__ csrc, int nchan,
    double* __restrict__ out) {
  using TL = FormalTile<LF>;
  constexpr int ZT = TL::ZT, YC = TL::YC, NZP = TL::NZP;
  static_assert(ZT % TL::G == 0, "tile/group mismatch");

  __shared__ rjp_d2 s_bt[kFB];      // (b, T) of the slab's cells, [row * ZT + sightline]
  __shared__ int s_hot[ZT];         // the sightline has a cell with T > 0 (T_avg is not NaN)

  const FormalPlace<LF> pl(nz);
  const int x = pl.x, z0 = pl.z0, cy = pl.cy, cz = pl.cz, cb = pl.cb;
  const int tid = threadIdx.x;
  const int fi = (int)blockIdx.y * LF + tid % LF;
  const bool chan_live = fi < nchan;
  const double ct = chan_live ? ctau[fi] : 0.0;     // dead lanes: dtau = 0, om = 0 exactly

  if (tid < ZT) s_hot[tid] = 0;
  __syncthreads();
  int ya, ye;
  tile_y_range<ZT>(f.ylo, f.yhi, x, z0, nz, ny, ya, ye);

  double I[NZP], Th[NZP];
#pragma unroll
  for (int j = 0; j < NZP; ++j) { I[j] = 0.0; Th[j] = 1.0; }

  for (int yb = ya; yb < ye; yb += YC) {
    // ---- phase 1: b and T of one cell per thread ------------------------------------------
    {
      const int yy = yb + cy, zz = z0 + cz;
      double bb = 0.0, tk = 0.0;
      if (yy < ye && zz < nz) {
        const int64_t o = ((int64_t)x * ny + yy) * nz + zz;
        const double Tk = (double)f.temp[o];
        if (Tk > 0.0) s_hot[cz] = 1;                  // (every writer stores the same value)
        bb = formal_b<T, LAY, BURSTS>(f, o, mode, bd, time_s, Tk);
        tk = formal_temp(bb, Tk);
      }
      rjp_d2 v;
      v.x = bb;
      v.y = tk;
      s_bt[tid] = v;
    }
    __syncthreads();

    // ---- phase 2: lanes over channels, rows front to back -----------------------------------
#pragma unroll 2
    for (int r = 0; r < YC; ++r) {
      rjp_d2 c[NZP];
      bool any = false;
#pragma unroll
      for (int j = 0; j < NZP; ++j) {
        c[j] = s_bt[r * ZT + cb + j];
        any |= c[j].x != 0.0;
      }
      if (!any) continue;
#pragma unroll
      for (int j = 0; j < NZP; ++j) {
        formal_update(c[j].y, one_minus_exp_neg(ct * c[j].x), I[j], Th[j]);
      }
    }
    __syncthreads();
  }

  if (chan_live) {
    const double cs = csrc[fi];
    const int64_t base = (int64_t)fi * nx * nz + (int64_t)x * nz + z0 + cb;
#pragma unroll
    for (int j = 0; j < NZP; ++j)
      if (z0 + cb + j < nz) out[base + j] = formal_out(s_hot[cb + j], cs, I[j]);
  }
}

template <typename T, int LAY, int LF>
static hipError_t formal_launch_t(const FormalFields<T>& f, const rjp_fields* fl, int mode,
                                  const BurstsDev& b, bool bursts, double time_s,
                                  const double* ctau, const double* csrc, int nchan, double* out,
                                  hipStream_t st) {
  const int ntz = (fl->nz + FormalTile<LF>::ZT - 1) / FormalTile<LF>::ZT;
  const dim3 grid((unsigned)((int64_t)fl->nx * ntz), (unsigned)((nchan + LF - 1) / LF));
  if (bursts)
    hipLaunchKernelGGL((ff_formal_kernel<T, LAY, LF, true>), grid, dim3(kFB), 0, st, f, fl->nx,
                       fl->ny, fl->nz, mode, b, time_s, ctau, csrc, nchan, out);
  else
    hipLaunchKernelGGL((ff_formal_kernel<T, LAY, LF, false>), grid, dim3(kFB), 0, st, f, fl->nx,
                       fl->ny, fl->nz, mode, b, time_s, ctau, csrc, nchan, out);
  return hipGetLastError();
}

// channel lanes: the narrowest layout that holds every channel up to 32 channels; blocks of 64
// lanes up to 128 channels, of 256 beyond
template <typename T, int LAY>
static hipError_t formal_launch_lf(const FormalFields<T>& f, const rjp_fields* fl, int mode,
                                   const BurstsDev& b, bool bursts, double time_s,
                                   const double* ctau, const double* csrc, int nchan, double* out,
                                   hipStream_t st) {
  if (nchan > 128) return formal_launch_t<T, LAY, 256>(f, fl, mode, b, bursts, time_s, ctau, csrc, nchan, out, st);
  if (nchan > 32) return formal_launch_t<T, LAY, 64>(f, fl, mode, b, bursts, time_s, ctau, csrc, nchan, out, st);
  if (nchan > 16) return formal_launch_t<T, LAY, 32>(f, fl, mode, b, bursts, time_s, ctau, csrc, nchan, out, st);
  return formal_launch_t<T, LAY, 16>(f, fl, mode, b, bursts, time_s, ctau, csrc, nchan, out, st);
}

hipError_t ff_formal_launch(const rjp_fields* fl, const rjp_bursts* hb, const double* d_ext,
                            double time_s, int mode, const double* d_ctau, const double* d_csrc,
                            int nchan, double* out, hipStream_t st) {
  BurstsDev b;
  const bool bursts = bursts_to_dev(hb, b, d_ext);
  if (bursts && !fl->d_ts) return hipErrorInvalidValue;
  return formal_dispatch(fl, mode, fl->d_ts, [&](const auto& f, auto lay) {
    using T = typename std::decay_t<decltype(f)>::value_type;
    return formal_launch_lf<T, decltype(lay)::value>(f, fl, mode, b, bursts, time_s, d_ctau,
                                                     d_csrc, nchan, out, st);
  });
}

}  // namespace rjp
