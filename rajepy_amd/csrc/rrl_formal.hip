// K6: LTE recombination-line intensity by the formal solution of the transfer equation along the
// line of sight.
//
// The reference's line maps are isothermal: I_L = B_nu(T_avg) e^-tau_ff (1 - e^-tau_rrl) with T_avg
// the nanmean of the sightline's T > 0 (classes.py:1280-1282, 1339-1343; rrls.py:444-449; K3's map
// stage here), exact only where T is constant along the sightline, and never negative.  This
// kernel walks every sightline front to back (observer at the iy = 0 end of axis 1, as K5) with
// the continuum optical depth c_i = ctau[f] b_i of K5 (formal_b, ff_formal.h), the line optical
// depth l_i of K3 (cell_line and the Voigt paths, rrl_voigt.h) and B_i = 1 / expm1(hnu_k[f] / T_i):
//   out[f, p] = csrc[f] (I_tot - I_cont),
//   I_tot  = sum_i B_i (1 - e^-(c_i + l_i)) exp(-sum_{j < i} (c_j + l_j)),   I_cont: l == 0.
// The two chains are never formed and subtracted (tau_C reaches ~100 where the difference is
// 1e-10 of either): with Theta_C = exp(-sum c), D = Theta_C - Theta_tot >= 0 the line's emission
// and its absorption of what lies behind it accumulate directly,
//   e_c = e^-c, om_l = 1 - e^-l, u = 1 - e^-(c + l) = (1 - e_c) + e_c om_l
//   I += B (e_c om_l Theta_C - u D);  D = e_c (D + (Theta_C - D) om_l);  Theta_C *= e_c.
// e_c and 1 - e_c both come out of one_minus_exp_neg(c, e_c), each at its own relative accuracy.
// With a constant T the sum telescopes to B e^-tau_C (1 - e^-tau_L): the reference's product.
// A cell contributes its c exactly when K5 counts it (formal_b != 0) and its l exactly when K3
// does (CellLine::C != 0, i.e. path_code != kPathSkip); the output is NaN exactly where T_avg is
// (formal_out).
//
// Layout: a tile walked front to back like K5's (tile_y_range, rjp_device.h) with K3's channel
// loop, whose pieces both kernels take from rrl_voigt.h: the XCD tile map, the folded channel
// lanes, the waves' frequency ranges and the path-code stream.  A 256-thread
// workgroup owns ZT z-adjacent sightlines of one x-row and a block of LF channels;
//   phase 1  one thread per cell of a slab of YC y-rows: K3's line constants, b, the two constants
//            of the Planck expansion and one path code per (cell, wave) to LDS;
//   phase 2  a wave works on one cell per trip (LF >= 64), rows in increasing iy: Re w by the
//            wave-uniform path of the code, l = V (A + B dnu), the recurrence above.  I, Theta_C
//            and D live in LDS slots per (thread, sightline) between slabs.
// A lane keeps its channel for the whole walk (K3's rotation of the |x| bands over the waves is for
// unordered sums; measured here it bought nothing).  The wave-uniform layouts stage 128 cells per
// slab (256 lanes: 4 sightlines x 32 rows, 64 lanes: 16 x 8): three state slots per (thread,
// sightline) instead of K3's one, 38.6 KB of LDS, four workgroups per CU at 128 VGPRs.
// B_i costs no exp per update: expm1(x0 + d) = expm1(x0) + e^x0 (d + d^2/2 + ...) about
// x0 = h nu_ref / k T, d = (hnu_k[f] - h nu_ref / k) / T, to first order in d
//   B = T e^-x0 / (T (1 - e^-x0) + dh),   dh = hnu_k[f] - h nu_ref / k
// (two staged constants, one fma, one reciprocal); the dropped term is the one K3 drops from the
// stimulated-emission factor, and the same criterion (band_needs_exp -> kPathExpFlag) sends the
// wave to expm1 per lane.
// Compute-bound (vector FP64), as K3 and K5: 312 VALU lane-instructions per (cell, channel) counted
// at the cfg3 shape.
#include "ff_formal.h"
#include "rrl_voigt.h"

namespace rjp {

template <int LF> struct RrlFormalTile {
  static constexpr int ZT = LF == 256 ? 4 : 16;
  static constexpr int NC = LF >= RJP_WAVE ? 128 : kRB;     // cells per slab
  static constexpr int YC = NC / ZT;
  static constexpr int G = kRB / LF;
  static constexpr int NZP = ZT / G;        // sightlines per thread
};

// bit 4 of a cell's code: it has continuum opacity (b != 0); bits 0-3 are K3's path code
constexpr int kCodeCont = 16;

// one update of the recurrence; om_l = 1 - e^-l of the cell's line optical depth (exactly 0 for a
// cell without line opacity: the update is then the continuum's alone), c its continuum depth
__device__ __forceinline__ void formal_line_update(double Bp, double c, double om_l, double& I,
                                                   double& Th, double& D) {
  // e_c at its own relative accuracy: 1 - om_c is off by e^c 2^-53 of it, which a pixel behind a
  // thick front cell inherits whole (B e^-c (1 - e^-l): 1.7e-4 at c = 30)
  double e_c;
  const double om_c = one_minus_exp_neg(c, e_c);
  const double t = e_c * om_l;
  const double u = om_c + t;
  I = __builtin_fma(Bp, __builtin_fma(t, Th, -(u * D)), I);
  D = e_c * __builtin_fma(Th - D, om_l, D);
  Th *= e_c;
}

template <typename T, int LF, bool BURSTS>
__global__ __launch_bounds__(kRB, 4) void rrl_formal_kernel(
    RrlFields<T> f, int nx, int ny, int nz, int mode, BurstsDev b, double time_s, LineDev ln,
    const double* __restrict__ nu, const double* __restrict__ ctau,
    const double* __restrict__ csrc, const double* __restrict__ hnu_k, int nchan,
    const double* __restrict__ add, double* __restrict__ out) {
  using TL = RrlFormalTile<LF>;
  constexpr int ZT = TL::ZT, YC = TL::YC, NZP = TL::NZP, NC = TL::NC;
  static_assert(ZT % TL::G == 0, "tile/group mismatch");
  static_assert(NC <= kRB && NC % ZT == 0, "one thread per cell of a slab, whole rows");
  constexpr bool CEN = LF >= RJP_WAVE;       // the waves work on one cell at a time

  // per-cell constants of the slab, [row * ZT + sightline].  Wave-uniform layouts stage the forms
  // voigt_wave_path and the line factor A + B dnu read: s_C <- A, s_nu0 <- c1, s_E0 <- B,
  // s_q / s_cq as in K3, s_ky = y h / pi;
  // the per-lane layout keeps the plain constants, and s_ky carries h / kT.
  __shared__ double s_nu0[NC], s_is2[NC], s_y[NC], s_C[NC], s_E0[NC], s_q[NC], s_cq[NC],
      s_ky[NC];
  __shared__ double s_b[NC];                 // b of the continuum, 0 = none
  __shared__ double s_g0[NC], s_te[NC];      // T (1 - e^-x0), T e^-x0 (their sum is T)
  __shared__ double s_it[CEN ? 1 : NC];      // per-lane layout: 1 / T, the expansion's second order
  __shared__ double s_I[NZP * kRB], s_Th[NZP * kRB], s_D[NZP * kRB];
  __shared__ double s_tab[CEN ? kRB / RJP_WAVE : 1][RJP_WAVE];
  constexpr int NWC = CEN ? LF / RJP_WAVE : 1;
  static_assert(YC % 8 == 0, "eight codes per read");
  // wave-uniform layouts: one byte per (wave of the channel block, sightline, row), rows adjacent;
  // per-lane layout: one byte per cell (kPathExpFlag alone)
  __shared__ __attribute__((aligned(8))) uint8_t s_cb[CEN ? NWC * ZT * YC : NC];
  __shared__ double s_rng[NWC][4];
  __shared__ int s_hot[ZT];                  // the sightline has a cell with T > 0

  const int ntz = (nz + ZT - 1) / ZT;
  // z-neighbours, which share 128-byte lines, run on one XCD
  const unsigned bx = xcd_tile(blockIdx.x, gridDim.x);
  const int x = (int)bx / ntz;
  const int z0 = ((int)bx - x * ntz) * ZT;
  const int tid = threadIdx.x;
  const int g = tid / LF;
  const ChannelLane<LF> ch(nchan);               // (folded about the block centre)
  const int fl = ch.fl, fi = ch.fi;
  const bool chan_live = ch.live;
  const double hk_ref = ln.h_over_k * ln.nu_ref;
  const double nu_f0 = chan_live ? nu[fi] : ln.nu_ref;
  // dead lanes: c = 0 and a finite B; nothing of theirs is stored
  const double ct0 = chan_live ? ctau[fi] : 0.0;
  const double hk0 = chan_live ? hnu_k[fi] : hk_ref;
  const double dnu = nu_f0 - ln.nu_ref, dh = hk0 - hk_ref;

#pragma unroll
  for (int j = 0; j < NZP; ++j) {
    s_I[j * kRB + tid] = 0.0;
    s_Th[j * kRB + tid] = 1.0;
    s_D[j * kRB + tid] = 0.0;
  }
  if (tid < ZT) s_hot[tid] = 0;

  if constexpr (CEN) wave_channel_range(ch, nu_f0, s_rng);
  __syncthreads();

  const PoleTop ptop = pole_top();
  const int cy = tid / ZT, cz = tid % ZT;       // this thread's cell in the slab (phase 1)

  int ya, ye;
  tile_y_range<ZT>(f.ylo, f.yhi, x, z0, nz, ny, ya, ye);

  const FormalFields<T> ff{f.nd, f.xi, f.temp, f.pf, f.ts, nullptr, nullptr, nullptr, nullptr};
  // (a scalar: the path code must reach the branches below as a wave-uniform value)
  const int wave = (CEN && LF > RJP_WAVE) ? __builtin_amdgcn_readfirstlane(fl / RJP_WAVE) : 0;

  for (int yb = ya; yb < ye; yb += YC) {
    // ---- phase 1: per-cell constants ---------------------------------------------------------
    if (NC == kRB || tid < NC) {
      const int yy = yb + cy, zz = z0 + cz;
      CellLine cl;
      double bb = 0.0, g0 = 0.0, te = 0.0;
      bool pexp = false;
      if (yy < ye && zz < nz) {
        const int64_t o = ((int64_t)x * ny + yy) * nz + zz;
        const double Tk = (double)f.temp[o];
        if (Tk > 0.0) s_hot[cz] = 1;                  // (every writer stores the same value)
        cl = cell_line<T, BURSTS, CEN>(f, o, b, time_s, ln);
        bb = formal_b<T, LAY_WIDE, BURSTS>(ff, o, mode, b, time_s, Tk);
        if (cl.C != 0.0 || bb != 0.0) {
          te = Tk * cl.E0;                            // E0 = exp(-x0), x0 = (h / kT) nu_ref
          g0 = -Tk * expm1(-cl.a * ln.nu_ref);
          // the per-lane layout (K3: 1e-11 per evaluation) keeps the second order of the expansion:
          // the dropped term is d^3 / 6, held below 1e-11 of expm1(x0) ~ 1 - E0
          const double ad = cl.a * ln.dnu_max;
          pexp = (CEN ? band_needs_exp(cl.a, cl.E0, ln.dnu_max)
                      : !(ad * ad * ad < 6e-11 * (1.0 - cl.E0))) ||
                 !(g0 - g0 == 0.0) || !(te - te == 0.0);
        }
      }
      const bool cen_cell = CEN && cl.y < kCenYMax;
      const double gq = cl.q >= 0.0 ? 2.0 * cl.q * exp(cl.y * cl.y) : 0.0;
      s_C[tid] = CEN ? cl.A : cl.C; s_nu0[tid] = CEN ? cl.c1 : cl.nu0; s_is2[tid] = cl.is2;
      s_y[tid] = cl.y; s_E0[tid] = CEN ? cl.B : cl.E0;
      s_q[tid] = cen_cell ? gq / (1.0 + cl.q) : cl.q;
      s_cq[tid] = (CEN && !cen_cell) ? gq : cl.cq;
      s_ky[tid] = CEN ? cl.y * (kHW / 3.14159265358979323846) : cl.a;
      s_b[tid] = bb; s_g0[tid] = g0; s_te[tid] = te;
      if constexpr (CEN) {
#pragma unroll
        for (int w = 0; w < NWC; ++w) {
          const double rg[4] = {s_rng[w][0], s_rng[w][1], s_rng[w][2], s_rng[w][3]};
          int code = path_code(cl, rg, ln.dnu_max);
          if (bb != 0.0) code |= kCodeCont;
          if (code != 0 && pexp) code |= kPathExpFlag;
          s_cb[(w * ZT + cz) * YC + cy] = (uint8_t)code;
        }
      } else {
        s_cb[tid] = pexp ? (uint8_t)kPathExpFlag : (uint8_t)0;
        s_it[tid] = 1.0 / (g0 + te);
      }
    }
    __syncthreads();

    // ---- phase 2: lanes over channels, rows front to back ------------------------------------
#pragma unroll 1
    for (int j = 0; j < NZP; ++j) {
      double I = s_I[j * kRB + tid], Th = s_Th[j * kRB + tid], D = s_D[j * kRB + tid];
      if constexpr (CEN) {
        CodeStream codes(s_cb + (wave * ZT + g * NZP + j) * YC);
#pragma unroll 1
        for (int r = 0; r < YC; ++r) {
          const int ci = r * ZT + g * NZP + j;
          const int pc = codes.next(r);
          if (pc == 0) continue;                // dead in both opacities
          const int path = pc & 7;
          double om_l = 0.0;                    // C == 0: the continuum's update alone
          if (path == kPathGeneric) {
            const int64_t o = ((int64_t)x * ny + (yb + r)) * nz + (z0 + g * NZP + j);
            const double term = line_term_generic<T, BURSTS>(f, o, b, time_s, ln, nu_f0, dnu);
            om_l = one_minus_exp_neg(term == term ? term : 0.0);     // nansum drops NaN terms
          } else if (path != kPathSkip) {
            const double yv = s_y[ci];
            const double xs = __builtin_fma(nu_f0, s_is2[ci], s_nu0[ci]);            // s_nu0 holds c1
            const double V = voigt_wave_path(path, xs, fabs(xs), yv, &s_ky[ci], &s_q[ci],
                                             &s_cq[ci], s_tab[tid / RJP_WAVE], ptop);
            double l;
            if (pc & kPathExpFlag) {
              const double a = ln.h_over_k / (s_g0[ci] + s_te[ci]);
              const double ce0 = s_E0[ci] / a;                  // C E0
              l = V * ((s_C[ci] + ce0) - ce0 * exp(-a * dnu));
            } else {
              l = V * __builtin_fma(s_E0[ci], dnu, s_C[ci]);    // V (A + B dnu)
            }
            om_l = one_minus_exp_neg(l);
          }
          double Bp;
          if (pc & kPathExpFlag) Bp = 1.0 / expm1(hk0 / (s_g0[ci] + s_te[ci]));
          else Bp = s_te[ci] * rcp_fast(s_g0[ci] + dh);
          formal_line_update(Bp, ct0 * s_b[ci], om_l, I, Th, D);
        }
      } else {
#pragma unroll 1
        for (int r = 0; r < YC; ++r) {
          const int ci = r * ZT + g * NZP + j;
          const double C = s_C[ci], bb = s_b[ci];
          if (C == 0.0 && bb == 0.0) continue;
          double om_l = 0.0;
          if (C != 0.0) {
            CellLine cl;
            cl.C = C; cl.nu0 = s_nu0[ci]; cl.is2 = s_is2[ci]; cl.y = s_y[ci]; cl.a = s_ky[ci];
            cl.E0 = s_E0[ci]; cl.q = s_q[ci]; cl.cq = s_cq[ci];
            const double term = line_term<false>(cl, nu_f0, dnu, ln.dnu_max, nullptr);
            om_l = one_minus_exp_neg(term == term ? term : 0.0);
          }
          double Bp;
          if (s_cb[ci] & kPathExpFlag) Bp = 1.0 / expm1(hk0 / (s_g0[ci] + s_te[ci]));
          else Bp = s_te[ci] * rcp_fast(__builtin_fma(dh, __builtin_fma(0.5 * dh, s_it[ci], 1.0), s_g0[ci]));
          formal_line_update(Bp, ct0 * bb, om_l, I, Th, D);
        }
      }
      s_I[j * kRB + tid] = I; s_Th[j * kRB + tid] = Th; s_D[j * kRB + tid] = D;
    }
    __syncthreads();
  }

  if (chan_live) {
    const double cs = csrc[fi];
    const int64_t base = (int64_t)fi * nx * nz + (int64_t)x * nz + z0 + g * NZP;
#pragma unroll
    for (int j = 0; j < NZP; ++j)
      if (z0 + g * NZP + j < nz) {
        double v = formal_out(s_hot[g * NZP + j], cs, s_I[j * kRB + tid]);
        if (add) v += add[base + j];
        out[base + j] = v;
      }
  }
}

template <typename T, int LF>
static hipError_t rrl_formal_launch_t(const rjp_fields* fl, int mode, const BurstsDev& b,
                                      bool bursts, double time_s, const LineDev& ln,
                                      const double* d_nu, const double* d_ctau,
                                      const double* d_csrc, const double* d_hnu_k, int nchan,
                                      const double* d_add, double* out, hipStream_t st) {
  RrlFields<T> f{(const T*)fl->d_nd, (const T*)fl->d_xi, (const T*)fl->d_temp,
                 (const T*)fl->d_pf, (const T*)fl->d_ts, (const T*)fl->d_vy, fl->d_ylo, fl->d_yhi};
  const int ntz = (fl->nz + RrlFormalTile<LF>::ZT - 1) / RrlFormalTile<LF>::ZT;
  const dim3 grid((unsigned)((int64_t)fl->nx * ntz), (unsigned)((nchan + LF - 1) / LF));
  if (bursts)
    hipLaunchKernelGGL((rrl_formal_kernel<T, LF, true>), grid, dim3(kRB), 0, st, f, fl->nx,
                       fl->ny, fl->nz, mode, b, time_s, ln, d_nu, d_ctau, d_csrc, d_hnu_k, nchan,
                       d_add, out);
  else
    hipLaunchKernelGGL((rrl_formal_kernel<T, LF, false>), grid, dim3(kRB), 0, st, f, fl->nx,
                       fl->ny, fl->nz, mode, b, time_s, ln, d_nu, d_ctau, d_csrc, d_hnu_k, nchan,
                       d_add, out);
  return hipGetLastError();
}

// channel lanes as K3: up to 16 channels the per-lane layout, blocks of 64 lanes up to 128
// channels, of 256 beyond
template <typename T>
static hipError_t rrl_formal_launch_lf(const rjp_fields* fl, int mode, const BurstsDev& b,
                                       bool bursts, double time_s, const LineDev& ln,
                                       const double* d_nu, const double* d_ctau,
                                       const double* d_csrc, const double* d_hnu_k, int nchan,
                                       const double* d_add, double* out, hipStream_t st) {
  if (nchan > 128)
    return rrl_formal_launch_t<T, 256>(fl, mode, b, bursts, time_s, ln, d_nu, d_ctau, d_csrc,
                                       d_hnu_k, nchan, d_add, out, st);
  if (nchan > 16)
    return rrl_formal_launch_t<T, 64>(fl, mode, b, bursts, time_s, ln, d_nu, d_ctau, d_csrc,
                                      d_hnu_k, nchan, d_add, out, st);
  return rrl_formal_launch_t<T, 16>(fl, mode, b, bursts, time_s, ln, d_nu, d_ctau, d_csrc,
                                    d_hnu_k, nchan, d_add, out, st);
}

hipError_t rrl_formal_launch(const rjp_fields* fl, const rjp_bursts* hb, const double* d_ext,
                             double time_s, int mode, const rjp_line* line, const double* h_nu,
                             const double* d_nu, const double* d_ctau, const double* d_csrc,
                             const double* d_hnu_k, int nchan, const double* d_add, double* out,
                             hipStream_t st) {
  BurstsDev b;
  const bool bursts = bursts_to_dev(hb, b, d_ext);
  if (bursts && !fl->d_ts) return hipErrorInvalidValue;
  LineDev ln;
  fill_line(fl, line, h_nu, nchan, ln);
  if (fl->dtype == RJP_F64)
    return rrl_formal_launch_lf<double>(fl, mode, b, bursts, time_s, ln, d_nu, d_ctau, d_csrc,
                                        d_hnu_k, nchan, d_add, out, st);
  return rrl_formal_launch_lf<float>(fl, mode, b, bursts, time_s, ln, d_nu, d_ctau, d_csrc,
                                     d_hnu_k, nchan, d_add, out, st);
}

}  // namespace rjp
