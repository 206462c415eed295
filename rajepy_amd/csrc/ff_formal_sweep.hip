// K8: epoch sweeps of the formal solution along the line of sight -- the maps of K5 (ff_formal.hip)
// at E epochs and their per-channel totals (light curves) from ONE pass over the fields.
//
//   out[e, f, p] = csrc[f] sum_i T_i (1 - e^-dtau_i) exp(-sum_{j in front of i} dtau_j),
//   dtau_i = ctau[f] b_i(e),  b_i(e) = |a0_i| chi_i(t_e - ts_i)^2,     ftot[e, f] = nansum_p out
//
// The tile and walk of ff_formal.h (FormalTile, FormalPlace, tile_y_range) with the lane axis
// turned from channels to EPOCHS (light curves have 1-8 channels and tens to hundreds of epochs):
// a 256-thread workgroup owns ZT = 16 z-adjacent
// sightlines of one x-row, LE epochs (lanes; G = 256 / LE sightline groups, NZP = 16 / G sightlines
// per thread) and a register block of FC channels.
//   phase 1  one thread per cell of a slab of YC y-rows stages what does not depend on the epoch:
//            the signed a (|a0| as formal_a forms it for the layout, jet flag in the sign), T, ts;
//   phase 2  every lane walks the slab's rows in increasing iy for its sightlines: per cell
//            b = a chi^2(t_e - ts) ONCE, then for each channel of the block formal_update:
//            om = 1 - e^(-ctau b), I += T om Theta, Theta -= Theta om.
// LE = 64: the lanes of a wave look at the same cell (LDS broadcast), so the cell's jet is
// wave-uniform -- the burst parameters are scalar operands (chi_jet) and a dead cell (a == 0) is
// skipped by the whole wave.  LE = 16: four sightlines per wave, chi_cell's per-lane select.
// chi is evaluated once per (cell, epoch) however many channels there are; channels beyond FC go
// to further workgroups (gridDim.y), which repeat it.  Epochs: blocks of 64 lanes, the tail by
// blocks of 16 unless it fills more than three of them -- the only dead lanes are the last
// block's.
// b, the recurrence, the dead-cell rule and the output rule are the functions K5 calls
// (ff_formal.h: formal_a / formal_weigh / formal_live, formal_update, formal_temp, formal_out):
// each (sightline, epoch, channel) value is one sequential chain that no layout reorders, so every
// map equals rjp_ff_formal's at that epoch bit for bit.
// Totals: the tile's values pass through LDS ([epoch][sightline]); one thread per epoch adds its 16
// sightlines in a fixed order (NaN pixels add nothing, as nansum) to one partial per (epoch,
// channel, workgroup), and sum_partials_launch finishes.  No floating-point atomics.  The same
// transpose makes the map stores 128-byte runs along z.
#include "ff_formal.h"

namespace rjp {

template <typename T, int LAY, int LE, int FC>
__global__ __launch_bounds__(kFB, RJP_FORMAL_WAVES) void ff_formal_sweep_kernel(
    FormalFields<T> f, int nx, int ny, int nz, int mode, BurstsDev bd,
    const double* __restrict__ epochs, int e_lo, int e_hi,
    const double* __restrict__ ctau, const double* __restrict__ csrc, int nchan,
    double* __restrict__ out, double* __restrict__ part) {
  using TL = FormalTile<LE>;
  constexpr int ZT = TL::ZT, YC = TL::YC, NZP = TL::NZP;
  static_assert(ZT % TL::G == 0 && ZT == 16, "tile/group mismatch");

  __shared__ rjp_d2 s_at[kFB];      // (signed a, T) of the slab's cells, [row * ZT + sightline]
  __shared__ double s_ts[kFB];      // their launch times
  __shared__ double s_x[LE * ZT];   // one channel's pixel values of the tile, [epoch lane][sightline]
  __shared__ int s_hot[ZT];         // the sightline has a cell with T > 0 (T_avg is not NaN)

  const FormalPlace<LE> pl(nz);
  const int x = pl.x, z0 = pl.z0, cy = pl.cy, cz = pl.cz, cb = pl.cb;
  const int tid = threadIdx.x;
  const int el = tid % LE;
  const int e_blk = e_lo + (int)blockIdx.z * LE;     // first epoch of this workgroup
  const int ei = e_blk + el;
  const double te = ei < e_hi ? epochs[ei] : 0.0;    // (a dead lane walks epoch 0 s and stores nothing)
  const int f0 = (int)blockIdx.y * FC;
  const int nf = nchan - f0 < FC ? nchan - f0 : FC;  // live channels of the block (workgroup-uniform)
  double ct[FC];
#pragma unroll
  for (int k = 0; k < FC; ++k) ct[k] = k < nf ? ctau[f0 + k] : 0.0;

  if (tid < ZT) s_hot[tid] = 0;
  __syncthreads();
  int ya, ye;
  tile_y_range<ZT>(f.ylo, f.yhi, x, z0, nz, ny, ya, ye);

  double I[NZP][FC], Th[NZP][FC];
#pragma unroll
  for (int j = 0; j < NZP; ++j)
#pragma unroll
    for (int k = 0; k < FC; ++k) { I[j][k] = 0.0; Th[j][k] = 1.0; }

  for (int yb = ya; yb < ye; yb += YC) {
    // ---- phase 1: signed a, T and ts of one cell per thread ----------------------------------
    {
      rjp_d2 v;
      double ts;
      formal_stage_cell<T, LAY>(f, x, yb + cy, z0 + cz, ye, ny, nz, mode, &s_hot[cz], v, ts);
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
        const double tl = te - s_ts[ci];
        double chi;
        if constexpr (LE >= RJP_WAVE) {
          const int jet = (int)__builtin_amdgcn_readfirstlane(hi_dword(c.x)) < 0 ? 0 : 1;
          chi = chi_jet(bd, jet, tl);
        } else {
          chi = chi_cell(bd, signbit_d(c.x), tl);
        }
        const double b = formal_live(formal_weigh(fabs(c.x), chi));
        const double tk = formal_temp(b, c.y);
#pragma unroll
        for (int k = 0; k < FC; ++k) {
          if (k < nf) formal_update(tk, one_minus_exp_neg(ct[k] * b), I[j][k], Th[j][k]);
        }
      }
    }
    __syncthreads();
  }

  // ---- the tile's maps and its share of the totals, one channel at a time -----------------------
  const int ne = e_hi - e_blk < LE ? e_hi - e_blk : LE;        // live epochs of this workgroup
  const int64_t npix = (int64_t)nx * nz;
#pragma unroll
  for (int k = 0; k < FC; ++k) {
    if (k < nf) {
      const double cs = csrc[f0 + k];
#pragma unroll
      for (int j = 0; j < NZP; ++j)
        s_x[el * ZT + cb + j] = formal_out(z0 + cb + j < nz && s_hot[cb + j], cs, I[j][k]);
      __syncthreads();
      const int64_t pl0 = (int64_t)e_blk * nchan + f0 + k;        // the plane of the first epoch
      formal_tile_emit(s_x, ne, z0, nz, out ? out + pl0 * npix + (int64_t)x * nz + z0 : nullptr,
                       (int64_t)nchan * npix, part ? part + pl0 * gridDim.x + blockIdx.x : nullptr,
                       (int64_t)nchan * gridDim.x);
    }
  }
}

size_t ff_formal_sweep_workspace_bytes(int nx, int nz, int n_epochs, int n_chan) {
  // one partial per (epoch, channel, workgroup of 16 sightlines)
  const size_t nwg = (size_t)nx * (size_t)((nz + 15) / 16);
  return nwg * (size_t)n_epochs * (size_t)n_chan * sizeof(double) + 256;
}

namespace {

struct SweepArgs {
  const rjp_fields* fl;
  int mode;
  BurstsDev b;
  const double* epochs;
  int n_epochs;
  const double *ctau, *csrc;
  int nchan;
  double *out, *part;
  hipStream_t st;
};

template <typename T, int LAY, int LE, int FC>
hipError_t sweep_launch_t(const FormalFields<T>& f, const SweepArgs& a, int e_lo, int e_hi) {
  const int ntz = (a.fl->nz + FormalTile<LE>::ZT - 1) / FormalTile<LE>::ZT;
  const dim3 grid((unsigned)((int64_t)a.fl->nx * ntz), (unsigned)((a.nchan + FC - 1) / FC),
                  (unsigned)((e_hi - e_lo + LE - 1) / LE));
  hipLaunchKernelGGL((ff_formal_sweep_kernel<T, LAY, LE, FC>), grid, dim3(kFB), 0, a.st, f,
                     a.fl->nx, a.fl->ny, a.fl->nz, a.mode, a.b, a.epochs, e_lo, e_hi, a.ctau,
                     a.csrc, a.nchan, a.out, a.part);
  return hipGetLastError();
}

// channel block: every channel in registers up to 2 channels, blocks of 4 beyond
template <typename T, int LAY, int LE>
hipError_t sweep_launch_fc(const FormalFields<T>& f, const SweepArgs& a, int e_lo, int e_hi) {
  if (a.nchan == 1) return sweep_launch_t<T, LAY, LE, 1>(f, a, e_lo, e_hi);
  if (a.nchan == 2) return sweep_launch_t<T, LAY, LE, 2>(f, a, e_lo, e_hi);
  return sweep_launch_t<T, LAY, LE, 4>(f, a, e_lo, e_hi);
}

// epoch lanes: blocks of 64 while they are full; a tail of up to 48 epochs by blocks of 16
template <typename T, int LAY>
hipError_t sweep_launch_le(const FormalFields<T>& f, const SweepArgs& a) {
  const int n64 = formal_epochs64(a.n_epochs);
  if (n64 > 0) {
    const hipError_t e = sweep_launch_fc<T, LAY, 64>(f, a, 0, n64);
    if (e != hipSuccess) return e;
  }
  if (n64 < a.n_epochs) return sweep_launch_fc<T, LAY, 16>(f, a, n64, a.n_epochs);
  return hipSuccess;
}

}  // namespace

hipError_t ff_formal_sweep_launch(const rjp_fields* fl, const rjp_bursts* hb, const double* d_ext,
                                  const double* d_epochs, int n_epochs, int mode,
                                  const double* d_ctau, const double* d_csrc, int nchan,
                                  double* out, double* ftot, double* part, hipStream_t st) {
  SweepArgs a{fl, mode, {}, d_epochs, n_epochs, d_ctau, d_csrc, nchan, out, ftot ? part : nullptr, st};
  const bool bursts = bursts_to_dev(hb, a.b, d_ext);
  if (bursts && !fl->d_ts) return hipErrorInvalidValue;
  const void* ts = bursts ? fl->d_ts : nullptr;
  const hipError_t e = formal_dispatch(fl, mode, ts, [&](const auto& f, auto lay) {
    using T = typename std::decay_t<decltype(f)>::value_type;
    return sweep_launch_le<T, decltype(lay)::value>(f, a);
  });
  if (e != hipSuccess || !ftot) return e;
  const int nwg = fl->nx * ((fl->nz + 15) / 16);
  return sum_partials_launch(part, n_epochs * nchan, nwg, ftot, st);
}

}  // namespace rjp
