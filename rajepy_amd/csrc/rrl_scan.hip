// K3: LTE radio-recombination-line optical-depth cube, and its map stage.
//
// The reference evaluates scipy.special.wofz over the WHOLE 3-D grid once per channel and
// recomputes every channel-independent per-cell quantity each time
// (classes.py:1159-1214; maths/rrls.py:350-354, 383-389).  Here a 256-thread workgroup owns a
// tile of z-adjacent sightlines of one x-row -- 8 sightlines for the 256-channel-lane layout,
// 16 for the 64- and 16-lane ones -- and a block of up to 256 channels:
//   phase 1  the 256 threads turn a slab of 256 cells (32 y x 8 z, or 16 y x 16 z) into
//            per-cell line constants (Doppler-shifted nu0, 1/(sigma sqrt2), Voigt y, LTE
//            prefactor, h/kT, pole-term constants) staged in LDS -- once per cell, not once
//            per channel -- and, for the layouts whose waves work on one cell at a time, into
//            one path code per (cell, wave): which of the Faddeeva paths below the whole wave
//            takes for that cell;
//   phase 2  lanes run over CHANNELS (folded about the block centre, so that a wave holds a
//            narrow |x| range): every lane reads the same cell's constants from LDS
//            (broadcast), branches on the wave's path code (a scalar), evaluates Re w(x+iy)
//            for its channel and accumulates tau in FP64; the per-(sightline, channel)
//            accumulators live in LDS, so the sightline loop is not unrolled (< 128 VGPRs,
//            4 waves per SIMD).  Cells outside the jet are skipped with a scalar branch.
// Compute-bound (vector FP64) by construction -- 102.5 VALU instructions per (cell, channel) on
// cfg3's fields (counted: profiles/r03e_cfg3_k3_sq.json), census in profiles/r03_k3_census.md; HBM traffic is 6 fields per cell, read
// once per block of 256 channels.
//
// Accuracy budget.  The wave-uniform paths (far-field series, plain lattice with or without the
// pole term, centred lattice) are designed for <= 1e-8 relative on Re w against
// scipy.special.wofz over their whole domain -- one order inside SURVEY.md section 7's 1e-7,
// three inside BASELINE.json's 1e-5 on the maps: lattice step h = 0.675 with 8 node pairs
// (3.5e-9, at x = 0 and y = pi/h, where the pole term ends), 6- and 4-term far-field series
// (4.1e-9 / 1.2e-9), pole term skipped where a rigorous bound puts it below 3e-8 Re w (measured
// <= 1.5e-9 on the plain lattice, <= 2.9e-9 on the centred one), centred lattice with 7 nodes a
// side (7.2e-10 with its pole term); tools/voigt_design.py restates each path in NumPy and prints
// this table.
// Rounds 1-2 held them to 1e-11 (h = 0.6, 10 pairs, 8/5 terms): 131 instead of ~102
// instructions.  The generic per-lane path (16-lane layout, collapse=False, irregular cells)
// keeps h = 0.6 / 10 pairs: core 1.3e-11 (worst at x = 0, y = pi/h, where its pole term ends; below
// 1e-11 elsewhere), far-field continued fraction 3e-10.  tests/test_k3_voigt_reference_cpu.py runs
// the tool and holds its figures to the ones stated here; tests/test_gpu_k3_evaluations.py holds the
// kernels to K3_RTOL_WAVE / K3_RTOL_LANE one evaluation at a time (measured: DESIGN.md section 3).
#include "rrl_voigt.h"

namespace rjp {

// collapse=False: the 3-D per-cell optical depths (classes.py:1176-1177, 1382-1383).  One
// thread per cell, serial over channels; out[f * ncell + cell].
template <typename T, bool BURSTS>
__global__ __launch_bounds__(kRB) void rrl_cells_kernel(RrlFields<T> f, int64_t ncell,
                                                        BurstsDev b, double time_s, LineDev ln,
                                                        const double* __restrict__ nu, int nchan,
                                                        double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kRB + threadIdx.x;
  if (i >= ncell) return;
  const CellLine c = cell_line<T, BURSTS, false>(f, i, b, time_s, ln);
  const double nan = __builtin_nan("");
  // a cell outside the jet is NaN in the reference's 3-D output (NaN fields propagate)
  const bool dead = !((double)f.nd[i] == (double)f.nd[i]) || !((double)f.xi[i] == (double)f.xi[i]) ||
                    !((double)f.temp[i] == (double)f.temp[i]) || !((double)f.pf[i] == (double)f.pf[i]) ||
                    !((double)f.vy[i] == (double)f.vy[i]);
  for (int k = 0; k < nchan; ++k) {
    double v = nan;
    if (!dead) v = c.C == 0.0 ? 0.0 : line_term<false>(c, nu[k], nu[k] - ln.nu_ref, ln.dnu_max, nullptr);
    out[(int64_t)k * ncell + i] = v;
  }
}

// LF = lanes along the channel axis (16, 64 or 256); G = kRB / LF sightline groups.
// Tile = ZT z-adjacent sightlines (8 for LF = 256, else 16), slab = 256 / ZT y-rows.
// The per-(sightline, channel) accumulators live in LDS, one slot per thread and sightline,
// so the sightline loop is NOT unrolled: one inlined copy of the Voigt code, < 128 VGPRs.
#ifndef RJP_K3_ZT256
#define RJP_K3_ZT256 8      /* sightlines per workgroup of the 256-channel-lane kernel */
#endif
template <int LF> struct RrlTile {
  static constexpr int ZT = LF == 256 ? RJP_K3_ZT256 : 16;
  static constexpr int YC = kRB / ZT;
  static constexpr int G = kRB / LF;
  static constexpr int NZP = ZT / G;        // sightlines per thread
};

#ifndef RJP_K3_WAVES
#define RJP_K3_WAVES 4      /* 128-VGPR budget: 4 waves per SIMD hide the LDS/constant waits (+8 %) */
#endif
template <typename T, int LF, bool BURSTS>
__global__ __launch_bounds__(kRB, RJP_K3_WAVES) void rrl_scan_kernel(
    RrlFields<T> f, int nx, int ny, int nz, BurstsDev b, double time_s, LineDev ln,
    const double* __restrict__ nu, int nchan, double* __restrict__ tau) {
  using TL = RrlTile<LF>;
  constexpr int ZT = TL::ZT, YC = TL::YC, NZP = TL::NZP;
  static_assert(ZT % TL::G == 0, "tile/group mismatch");

  __shared__ double s_nu0[kRB], s_is2[kRB], s_y[kRB], s_C[kRB], s_a[kRB], s_E0[kRB],
      s_q[kRB], s_cq[kRB];
  __shared__ double s_acc[NZP * kRB];
  // per-wave table of the centred Voigt lattice (kernels whose waves work on one cell)
  constexpr bool CEN = LF >= RJP_WAVE;
  __shared__ double s_tab[CEN ? kRB / RJP_WAVE : 1][RJP_WAVE];
  // path codes (one byte per wave of the channel block) and the waves' channel ranges
  constexpr int NWC = CEN ? LF / RJP_WAVE : 1;
  // one byte per (wave of the channel block, sightline of the tile, y-row of the slab), rows
  // adjacent: a wave fetches the codes of eight rows with ONE 8-byte read and two
  // readfirstlane, then shifts them out of an SGPR pair (it used to read, add an address and
  // readfirstlane per evaluation)
  static_assert(YC % 8 == 0, "eight codes per read");
  __shared__ __attribute__((aligned(8))) uint8_t s_cb[CEN ? NWC * ZT * YC : 8];
  __shared__ double s_ky[CEN ? kRB : 1];     // y h / pi of the wave-uniform lattice
  __shared__ double s_rng[NWC][4];

  const int ntz = (nz + ZT - 1) / ZT;
#ifndef RJP_K3_XCD
#define RJP_K3_XCD 1      /* 0: A/B build with the identity tile map */
#endif
  const unsigned bx = RJP_K3_XCD ? xcd_tile(blockIdx.x, gridDim.x) : blockIdx.x;
  const int x = (int)bx / ntz;
  const int z0 = ((int)bx - x * ntz) * ZT;
  const int tid = threadIdx.x;
  // 256 channel lanes: the four waves of a workgroup hold four BANDS of |x| (the folded channel
  // order below), i.e. paths of very different cost (line core: lattice + pole term, 113
  // instructions; outermost band: 37), and they meet at a barrier per slab.  Which wave takes
  // which band ROTATES WITH THE SIGHTLINE inside a slab (band = (wave + j) mod 4, j = the
  // sightline of the tile): every wave gets every band twice per slab, so the four waves reach
  // the barrier together instead of three of them waiting for the one that holds the line core.
  // A (sightline, band) pair still belongs to exactly one wave per slab: no atomics, the same
  // summation order.  The accumulators are LDS slots per CHANNEL already; the channel
  // frequencies go to LDS too.
#ifndef RJP_K3_ROT
#define RJP_K3_ROT 1
#endif
  constexpr bool ROT = LF == 256 && RJP_K3_ROT != 0;
  __shared__ double s_nu[ROT ? kRB : 1];
  const int g = tid / LF;
  const ChannelLane<LF> ch(nchan);               // (folded about the block centre)
  const int fl = ch.fl, fi = ch.fi;
  const bool chan_live = ch.live;
  const double nu_f0 = chan_live ? nu[fi] : ln.nu_ref;
  if constexpr (ROT) s_nu[tid] = nu_f0;          // (visible after the barrier of the range block)

#pragma unroll
  for (int j = 0; j < NZP; ++j) s_acc[j * kRB + tid] = 0.0;

  if constexpr (CEN) {
    wave_channel_range(ch, nu_f0, s_rng);
    __syncthreads();
  }

  const PoleTop ptop = pole_top();
  const int cy = tid / ZT, cz = tid % ZT;       // this thread's cell in the slab (phase 1)

  int ya, ye;
  tile_y_range<ZT>(f.ylo, f.yhi, x, z0, nz, ny, ya, ye);
  ya = (ya / YC) * YC;          // (K3's own: its slabs keep the boundaries of the full walk)

  // (a scalar: the path code must reach the branches below as a wave-uniform value)
  const int wave = (CEN && LF > RJP_WAVE) ? __builtin_amdgcn_readfirstlane(fl / RJP_WAVE) : 0;

  for (int yb = ya; yb < ye; yb += YC) {
    // ---- phase 1: per-cell line constants --------------------------------------------
    {
      const int yy = yb + cy, zz = z0 + cz;
      CellLine cl;
      if (yy < ny && zz < nz)
        cl = cell_line<T, BURSTS, (LF >= RJP_WAVE)>(f, ((int64_t)x * ny + yy) * nz + zz, b,
                                                    time_s, ln);
      const double C = cl.C, nu0 = cl.nu0, is2 = cl.is2, yv = cl.y, a = cl.a, E0 = cl.E0,
                   q = cl.q, cq = cl.cq;
      // wave-uniform kernels stage the derived forms in the same slots: s_C <- A, s_nu0 <- c1,
      // s_E0 <- B (the per-lane layouts keep the plain constants)
      s_C[tid] = CEN ? cl.A : C; s_nu0[tid] = CEN ? cl.c1 : nu0; s_is2[tid] = is2; s_y[tid] = yv;
      // (wave-uniform kernels: the bound cq is used up by path_code below for cells of the
      // plain lattice, y >= 0.03 -- their slot carries 2 q exp(y^2) for the pole term instead;
      // q < 0 marks y >= pi/h, where no pole term exists)
      // cells of the centred lattice, y < 0.03: q is needed as 2 q exp(y^2) / (1 + q) only
      const bool cen_cell = CEN && yv < kCenYMax;
      const double gq = q >= 0.0 ? 2.0 * q * exp(yv * yv) : 0.0;
      s_a[tid] = a; s_E0[tid] = CEN ? cl.B : E0; s_q[tid] = cen_cell ? gq / (1.0 + q) : q;
      s_cq[tid] = (CEN && !cen_cell) ? gq : cq;
      if constexpr (CEN) {
        s_ky[tid] = yv * (kHW / 3.14159265358979323846);
#pragma unroll
        for (int w = 0; w < NWC; ++w) {
          const double rg[4] = {s_rng[w][0], s_rng[w][1], s_rng[w][2], s_rng[w][3]};
          s_cb[(w * ZT + cz) * YC + cy] = (uint8_t)path_code(cl, rg, ln.dnu_max);
        }
      }
    }
    __syncthreads();

    // ---- phase 2: lanes over channels ------------------------------------------------
#pragma unroll 1
    for (int j = 0; j < NZP; ++j) {
      const int wq = ROT ? (wave + j) & 3 : wave;                          // this wave's band
      const int slot = ROT ? (wq << 6) | (tid & (RJP_WAVE - 1)) : tid;     // channel slot of this lane
      const double nu_f = ROT ? s_nu[slot] : nu_f0;
      const double dnu = nu_f - ln.nu_ref;
      double acc = s_acc[j * kRB + slot];
      if constexpr (CEN) {
        // the wave works on ONE cell per trip: its path was decided in phase 1
        CodeStream codes(s_cb + (wq * ZT + g * NZP + j) * YC);
#pragma unroll 1
        for (int r = 0; r < YC; ++r) {
          const int ci = r * ZT + g * NZP + j;
          const int pc = codes.next(r);
          if (pc == kPathSkip) continue;
          const int path = pc & 7;
          if (path == kPathGeneric) {
            // irregular constants or absurd |x| beside core lanes: per-lane generic code,
            // NaN terms dropped as numpy.nansum does
            static_assert(kCenYMax == 0.03, "generic path assumes the centred bound ends at 0.03");
            const int64_t o = ((int64_t)x * ny + (yb + r)) * nz + (z0 + g * NZP + j);
            const double term = line_term_generic<T, BURSTS>(f, o, b, time_s, ln, nu_f, dnu);
            if (term == term) acc += term;
            continue;
          }
          const double yv = s_y[ci];
          // Re w is even in x, and the lattice and its pole term are written in x^2 and in
          // cosines of angles odd in x: they take the SIGNED x (no |x| to materialise for the
          // inline-asm constant multiplies, which carry no source modifiers)
          const double xs = __builtin_fma(nu_f, s_is2[ci], s_nu0[ci]);            // s_nu0 holds c1
          const double ax = fabs(xs);
          const double V = voigt_wave_path(path, xs, ax, yv, &s_ky[ci], &s_q[ci], &s_cq[ci],
                                           s_tab[tid / RJP_WAVE], ptop);
          // C V (1 - exp(-h nu / kT)) with 1 - exp(...) = 1 - E0 exp(-a (nu - nu_ref)); to first
          // order in a dnu over the band (unless the path code says otherwise) that is
          // V (A + B dnu), A = C (1 - E0), B = C E0 a staged per cell: two fmas
          if (pc & kPathExpFlag) {
            const double a = s_a[ci];
            const double ce0 = s_E0[ci] / a;                  // C E0
            acc = __builtin_fma(V, (s_C[ci] + ce0) - ce0 * exp(-a * dnu), acc);
          } else {
            acc = __builtin_fma(V, __builtin_fma(s_E0[ci], dnu, s_C[ci]), acc);
          }
        }
      } else {
#pragma unroll 1
        for (int r = 0; r < YC; ++r) {
          const int ci = r * ZT + g * NZP + j;
          const double C = s_C[ci];
          if (C != 0.0) {
            CellLine cl;
            cl.C = C; cl.nu0 = s_nu0[ci]; cl.is2 = s_is2[ci]; cl.y = s_y[ci]; cl.a = s_a[ci];
            cl.E0 = s_E0[ci]; cl.q = s_q[ci]; cl.cq = s_cq[ci];
            const double term = line_term<false>(cl, nu_f, dnu, ln.dnu_max, nullptr);
            if (term == term) acc += term;
          }
        }
      }
      s_acc[j * kRB + slot] = acc;
    }
    __syncthreads();
  }

  if (chan_live) {
    const int64_t base = (int64_t)fi * nx * nz + (int64_t)x * nz + z0 + g * NZP;
#pragma unroll
    for (int j = 0; j < NZP; ++j)
      if (z0 + g * NZP + j < nz) tau[base + j] = s_acc[j * kRB + tid];
  }
}

// ---- map stage (intensity_rrl / flux_rrl at map level) ---------------------------------
__global__ __launch_bounds__(kRB) void rrl_maps_kernel(
    const double* __restrict__ tau_rrl, const double* __restrict__ tau_ff,
    const double* __restrict__ tavg, const double* __restrict__ flux_ff, int64_t npix,
    const double* __restrict__ cflux, const double* __restrict__ hnu_k, int nchan,
    double* __restrict__ flux, double* __restrict__ part) {
  const int64_t p = (int64_t)blockIdx.x * kRB + threadIdx.x;
  const int fch = blockIdx.y;
  const bool live = p < npix;
  const int64_t o = (int64_t)fch * npix + p;
  double s = 0.0;
  if (live) {
    // B_nu(T) ~ 1/(exp(h nu/kT) - 1)   (physics.py:571-574), through expm1 as in rrl_formal.hip:
    // h nu/kT is 2e-6 ... 1e-3 at radio frequencies, where exp() - 1 cancels 5 to 6 digits
    // (the original does; this stage differs from it by up to ~5e-11 there)
    const double bnu = 1.0 / expm1(hnu_k[fch] / tavg[p]);
    // rrls.py:445-447
    s = cflux[fch] * bnu * exp(-tau_ff[o]) * one_minus_exp_neg(tau_rrl[o]);
    if (flux_ff) s += flux_ff[o];
    if (flux) flux[o] = s;
  }
  if (part) {
    __shared__ double red[kRB / RJP_WAVE];
    double v = (live && s == s) ? s : 0.0;
#pragma unroll
    for (int d = RJP_WAVE / 2; d > 0; d >>= 1) v += __shfl_down(v, d, RJP_WAVE);
    if ((threadIdx.x & (RJP_WAVE - 1)) == 0) red[threadIdx.x / RJP_WAVE] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
      double tot = 0.0;
      for (int w = 0; w < kRB / RJP_WAVE; ++w) tot += red[w];
      part[(int64_t)fch * gridDim.x + blockIdx.x] = tot;
    }
  }
}

// ---- launch helpers ---------------------------------------------------------------------
template <typename T, int LF>
static hipError_t rrl_launch_t(const rjp_fields* fl, const BurstsDev& b, bool bursts,
                               double time_s, const LineDev& ln, const double* d_nu,
                               int nchan, double* tau, hipStream_t st) {
  RrlFields<T> f{(const T*)fl->d_nd, (const T*)fl->d_xi, (const T*)fl->d_temp,
                 (const T*)fl->d_pf, (const T*)fl->d_ts, (const T*)fl->d_vy, fl->d_ylo, fl->d_yhi};
  const int ntz = (fl->nz + RrlTile<LF>::ZT - 1) / RrlTile<LF>::ZT;
  dim3 grid((unsigned)(fl->nx * ntz), (unsigned)((nchan + LF - 1) / LF));
  if (bursts)
    hipLaunchKernelGGL((rrl_scan_kernel<T, LF, true>), grid, dim3(kRB), 0, st, f, fl->nx,
                       fl->ny, fl->nz, b, time_s, ln, d_nu, nchan, tau);
  else
    hipLaunchKernelGGL((rrl_scan_kernel<T, LF, false>), grid, dim3(kRB), 0, st, f, fl->nx,
                       fl->ny, fl->nz, b, time_s, ln, d_nu, nchan, tau);
  return hipGetLastError();
}

template <typename T>
static hipError_t rrl_launch_lf(const rjp_fields* fl, const BurstsDev& b, bool bursts,
                                double time_s, const LineDev& ln, const double* d_nu,
                                int nchan, double* tau, hipStream_t st) {
  // 65-128 channels: two blocks of the 64-lane layout (phase 1 runs twice: ~9 % more work) beat
  // one 256-lane block with half its lanes idle (a channel shard of a 256-channel cube on 2 ranks:
  // 338 -> see profiles/r05_cfg4_f64_tau2_bench.json rank_share.cfg3.channels)
  if (nchan > 128) return rrl_launch_t<T, 256>(fl, b, bursts, time_s, ln, d_nu, nchan, tau, st);
  if (nchan > 16) return rrl_launch_t<T, 64>(fl, b, bursts, time_s, ln, d_nu, nchan, tau, st);
  return rrl_launch_t<T, 16>(fl, b, bursts, time_s, ln, d_nu, nchan, tau, st);
}

hipError_t rrl_cells_launch(const rjp_fields* fl, const rjp_bursts* hb, const double* d_ext,
                            double time_s, const rjp_line* line, const double* h_nu,
                            const double* d_nu, int nchan, double* out, hipStream_t st) {
  BurstsDev b;
  const bool bursts = bursts_to_dev(hb, b, d_ext);
  if (bursts && !fl->d_ts) return hipErrorInvalidValue;
  LineDev ln;
  fill_line(fl, line, h_nu, nchan, ln);
  const int64_t n = (int64_t)fl->nx * fl->ny * fl->nz;
  const unsigned blocks = (unsigned)((n + kRB - 1) / kRB);
  auto go = [&](auto tag) {
    using T = decltype(tag);
    RrlFields<T> f{(const T*)fl->d_nd, (const T*)fl->d_xi, (const T*)fl->d_temp,
                   (const T*)fl->d_pf, (const T*)fl->d_ts, (const T*)fl->d_vy, nullptr, nullptr};
    if (bursts)
      hipLaunchKernelGGL((rrl_cells_kernel<T, true>), dim3(blocks), dim3(kRB), 0, st, f, n, b,
                         time_s, ln, d_nu, nchan, out);
    else
      hipLaunchKernelGGL((rrl_cells_kernel<T, false>), dim3(blocks), dim3(kRB), 0, st, f, n, b,
                         time_s, ln, d_nu, nchan, out);
  };
  if (fl->dtype == RJP_F64) go(double{}); else go(float{});
  return hipGetLastError();
}

hipError_t rrl_scan_launch(const rjp_fields* fl, const rjp_bursts* hb, const double* d_ext,
                           double time_s, const rjp_line* line, const double* h_nu,
                           const double* d_nu, int nchan, double* tau, hipStream_t st) {
  BurstsDev b;
  const bool bursts = bursts_to_dev(hb, b, d_ext);
  if (bursts && !fl->d_ts) return hipErrorInvalidValue;
  LineDev ln;
  fill_line(fl, line, h_nu, nchan, ln);
  if (fl->dtype == RJP_F64)
    return rrl_launch_lf<double>(fl, b, bursts, time_s, ln, d_nu, nchan, tau, st);
  return rrl_launch_lf<float>(fl, b, bursts, time_s, ln, d_nu, nchan, tau, st);
}

hipError_t rrl_maps_launch(const double* tau_rrl, const double* tau_ff, const double* tavg,
                           const double* flux_ff, int64_t npix, const double* d_cflux,
                           const double* d_hnu_k, int nchan, double* flux, double* ftot,
                           double* part, hipStream_t st) {
  const unsigned nblk = (unsigned)((npix + kRB - 1) / kRB);
  hipLaunchKernelGGL(rrl_maps_kernel, dim3(nblk, (unsigned)nchan), dim3(kRB), 0, st, tau_rrl,
                     tau_ff, tavg, flux_ff, npix, d_cflux, d_hnu_k, nchan, flux,
                     ftot ? part : nullptr);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return err;
  if (ftot) err = sum_partials_launch(part, nchan, (int)nblk, ftot, st);
  return err;
}

}  // namespace rjp
