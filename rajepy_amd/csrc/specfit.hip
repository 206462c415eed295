// K21 (rjp_cube_moments, rjp_specfit): moment maps of a line cube and one Levenberg-Marquardt fit
// of n_comp Gaussians plus a linear baseline per sightline -- what radio astronomers get from CASA
// immoments and specfit.  CASA is not at hand: the header comment (include/rjprt.h) IS the
// definition, parity is not claimed.
//
// Shape.  Both kernels run ONE LANE PER PIXEL, workgroups of one wave (64 pixels), and walk the
// channels in ascending order: for channel c a wave reads the 64 consecutive doubles
// cube[c * n_pix + p0 .. p0 + 63] (one 512-byte request), and the channel tables x, dx / w are the
// same for every lane (uniform addresses: scalar loads).  Every sum is a chain in channel order in
// the lane's own registers: no atomics, no cross-lane reduction, no LDS, no workspace, and the
// bits of a pixel's outputs are a function of its spectrum and the tables alone.
//
// Moments: pass 1 (m0, s1, peak, count), m1, then pass 2 (s2) over the same counted channels in
// the same launch and lane; the second pass re-reads the spectrum.
//
// Fit: the whole fit of a pixel in one launch.  A lane keeps theta_cur, the trial, chi^2, N and g
// of theta_cur and the trial's sums in registers, re-reads its spectrum once per trial, and takes
// lm_common.h's decision for itself after every trial, in its own loop: feasible = every width
// finite and > 0; the step scales (max(|A|, 1e-300), s, s) per line, s = max(sigma, 1e-300), and
// max(|b|, 1e-300) for a free baseline parameter; enough = count >= the number of free parameters.
// lm_tri, lm_solve and lm_step_converged are the header's; the take-over of a trial's sums and the
// breakdown loop are lm_take_sums and lm_damped_solve WRITTEN OUT here: through the calls the
// same arithmetic is allocated 4 to 16 VGPRs more (162 / 118 / 288 / 212 against 158 / 112 / 272 /
// 200 for <1, true>, <1, false>, <2, true>, <2, false>).  A finished lane idles; the wave leaves
// when its last lane is finished.  The kernel is templated on n_comp and on whether a baseline
// parameter is free (BL): with both held, the sums and the Cholesky run on the 3 n_comp line
// parameters alone (the identity's rows of the baseline would change no bit of the others:
// they come last, their L entries and steps are exact zeros), the baseline still enters the model.
#include "lm_common.h"

namespace rjp {

constexpr int kSfB = 64;           // pixels per workgroup: one wave

int64_t specfit_workgroups(int64_t n_pix) { return (n_pix + kSfB - 1) / kSfB; }

__global__ __launch_bounds__(kSfB) void cube_moments_kernel(
    const double* __restrict__ cube, int64_t n_pix, int n_chan, const double* __restrict__ x,
    const double* __restrict__ dx, double x_ref, double clip, const uint8_t* __restrict__ mask,
    double* __restrict__ mom, int* __restrict__ ipeak, int* __restrict__ count) {
  const int64_t p = (int64_t)blockIdx.x * kSfB + threadIdx.x;
  if (p >= n_pix) return;
  const double nan = __builtin_nan("");
  double m0 = 0.0, s1 = 0.0, peak = -__builtin_inf();
  int ip = -1, cnt = 0;
  const bool live = !mask || mask[p] != 0;
  if (live) {
    const double* __restrict__ col = cube + p;
#pragma unroll 4
    for (int c = 0; c < n_chan; ++c) {
      const double y = col[(int64_t)c * n_pix];
      if (!(finite_d(y) && __builtin_fabs(y) >= clip)) continue;
      const double yd = y * dx[c];
      m0 = __builtin_fma(y, dx[c], m0);
      s1 = __builtin_fma(yd, x[c] - x_ref, s1);
      if (y > peak) {
        peak = y;
        ip = c;
      }
      ++cnt;
    }
  }
  double m1 = nan, m2 = nan;
  if (cnt == 0 || m0 == 0.0) {
    m0 = 0.0;
    peak = nan;
    ip = -1;
  } else {
    m1 = x_ref + s1 / m0;
    double s2 = 0.0;
    const double* __restrict__ col = cube + p;
#pragma unroll 4
    for (int c = 0; c < n_chan; ++c) {
      const double y = col[(int64_t)c * n_pix];
      if (!(finite_d(y) && __builtin_fabs(y) >= clip)) continue;
      const double d = x[c] - m1;
      s2 = __builtin_fma(y * dx[c], d * d, s2);
    }
    const double q = s2 / m0;
    m2 = q < 0.0 ? nan : __builtin_sqrt(q);
  }
  mom[p] = m0;
  mom[n_pix + p] = m1;
  mom[2 * n_pix + p] = m2;
  mom[3 * n_pix + p] = peak;
  if (ipeak) ipeak[p] = ip;
  if (count) count[p] = cnt;
}

hipError_t cube_moments_launch(const double* cube, int64_t n_pix, int n_chan, const double* d_x,
                               const double* d_dx, double x_ref, double clip, const uint8_t* mask,
                               double* mom, int32_t* ipeak, int32_t* count, hipStream_t st) {
  hipLaunchKernelGGL(cube_moments_kernel, dim3((unsigned)specfit_workgroups(n_pix)), dim3(kSfB), 0,
                     st, cube, n_pix, n_chan, d_x, d_dx, x_ref, clip, mask, mom, ipeak, count);
  return hipGetLastError();
}

template <int NC, bool BL>
__global__ __launch_bounds__(kSfB) void specfit_kernel(
    const double* __restrict__ cube, int64_t n_pix, int n_chan, const double* __restrict__ x,
    const double* __restrict__ w, double x_ref, const uint8_t* __restrict__ mask,
    unsigned free_bits, double* __restrict__ theta, double lambda0, double xtol, int n_iter,
    double* __restrict__ chi2, double* __restrict__ cov, int* __restrict__ o_nchan,
    int* __restrict__ o_niter, int* __restrict__ o_status, double* __restrict__ trace) {
  constexpr int P = 3 * NC + 2;                      // the parameters of a pixel
  constexpr int PA = BL ? P : 3 * NC;                // those that enter N and g
  constexpr int TA = PA * (PA + 1) / 2;
  const int64_t p = (int64_t)blockIdx.x * kSfB + threadIdx.x;
  if (p >= n_pix) return;
  if (mask && mask[p] == 0) {
    o_status[p] = 3;
    return;
  }
  double th_c[P], th_t[P];
  bool good = true;
#pragma unroll
  for (int i = 0; i < P; ++i) {
    th_c[i] = th_t[i] = theta[(int64_t)i * n_pix + p];
    good = good && finite_d(th_c[i]);
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) good = good && th_c[3 * c + 2] > 0.0;
  if (!good) {
    o_status[p] = 3;
    return;
  }
  const int n_free = __builtin_popcount(free_bits);
  const double* __restrict__ col = cube + p;
  double* __restrict__ row = trace ? trace + p * n_iter * (3 + P) : nullptr;
  double Nc[TA], gc[PA];
#pragma unroll
  for (int i = 0; i < TA; ++i) Nc[i] = 0.0;
#pragma unroll
  for (int i = 0; i < PA; ++i) gc[i] = 0.0;
  double chi_c = __builtin_inf(), lam = lambda0, lam_used = lambda0;
  int cnt = 0, status = 0, it = 1;
  for (;; ++it) {
    // one trial: chi^2, N, g of th_t over the counted channels, ascending
    double chi_t = 0.0, Nt[TA], gt[PA], rs[NC];
#pragma unroll
    for (int i = 0; i < TA; ++i) Nt[i] = 0.0;
#pragma unroll
    for (int i = 0; i < PA; ++i) gt[i] = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) rs[c] = 1.0 / th_t[3 * c + 2];
    int n = 0;
#pragma unroll 1
    for (int c = 0; c < n_chan; ++c) {
      const double y = col[(int64_t)c * n_pix];
      const double wc = w ? w[c] : 1.0;
      if (!(finite_d(y) && wc > 0.0)) continue;
      const double xc = x[c], xr = xc - x_ref;
      double J[PA], m = 0.0;
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        const double d = xc - th_t[3 * k + 1];
        const double z = d / th_t[3 * k + 2];
        const double e = -0.5 * (z * z);
        // (NaN compares false -> exp_any -> NaN: such a trial is rejected)
        const double E = e < -700.0 ? 0.0 : exp_any(e);
        const double ae = th_t[3 * k] * E;
        const double jx = (ae * z) * rs[k];
        J[3 * k] = E;
        J[3 * k + 1] = jx;
        J[3 * k + 2] = jx * z;
        m = k == 0 ? ae : m + ae;
      }
      m += __builtin_fma(th_t[P - 1], xr, th_t[P - 2]);
      if (BL) {
        J[PA - 2] = 1.0;
        J[PA - 1] = xr;
      }
      const double r = y - m;
      chi_t = __builtin_fma(wc * r, r, chi_t);
#pragma unroll
      for (int i = 0; i < PA; ++i) {
        const double wj = wc * J[i];
#pragma unroll
        for (int j = i; j < PA; ++j)
          Nt[lm_tri<PA>(i, j)] = __builtin_fma(wj, J[j], Nt[lm_tri<PA>(i, j)]);
        gt[i] = __builtin_fma(wj, r, gt[i]);
      }
      ++n;
    }
    if (it == 1) {
      cnt = n;
      if (cnt < n_free || !finite_d(chi_t)) {
        o_status[p] = 3;
        return;
      }
    }
    // the decision (lm_common.h)
    bool feas = true;
#pragma unroll
    for (int c = 0; c < NC; ++c) feas = feas && finite_d(th_t[3 * c + 2]) && th_t[3 * c + 2] > 0.0;
    const bool acc = feas && finite_d(chi_t) && chi_t < chi_c;
    if (row) {
      double* __restrict__ t = row + (int64_t)(it - 1) * (3 + P);
      t[0] = chi_t;
      t[1] = lam_used;
      t[2] = acc ? 1.0 : 0.0;
#pragma unroll
      for (int i = 0; i < P; ++i) t[3 + i] = th_t[i];
    }
    if (acc) {
#pragma unroll
      for (int i = 0; i < P; ++i) th_c[i] = th_t[i];
      // (lm_take_sums)
#pragma unroll
      for (int i = 0; i < PA; ++i) {
        const bool fi = (free_bits >> i) & 1u;
#pragma unroll
        for (int j = i; j < PA; ++j)
          Nc[lm_tri<PA>(i, j)] =
              (fi && ((free_bits >> j) & 1u)) ? Nt[lm_tri<PA>(i, j)] : (i == j ? 1.0 : 0.0);
        gc[i] = fi ? gt[i] : 0.0;
      }
      chi_c = chi_t;
      if (it > 1) lam = __builtin_fmax(lam / 10.0, 1e-12);
    } else {
      lam *= 10.0;
    }
    if (chi_c == 0.0) {
      status = 1;
      break;
    }
    double delta[PA], scale[PA];
    bool ok = false;
    // (lm_damped_solve)
    while (true) {
      if (lam > 1e12) break;
      if (lm_solve<PA>(Nc, gc, lam, delta)) {
        ok = true;
        break;
      }
      lam *= 10.0;
    }
    if (!ok) {
      status = 2;
      break;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      scale[3 * c] = __builtin_fmax(__builtin_fabs(th_c[3 * c]), 1e-300);
      scale[3 * c + 1] = scale[3 * c + 2] = __builtin_fmax(th_c[3 * c + 2], 1e-300);
    }
#pragma unroll
    for (int i = 3 * NC; i < PA; ++i) scale[i] = __builtin_fmax(__builtin_fabs(th_c[i]), 1e-300);
    if (lm_step_converged<PA>(delta, scale, xtol)) {
      status = 1;
      break;
    }
    if (it == n_iter) {
      status = 0;
      break;
    }
#pragma unroll
    for (int i = 0; i < PA; ++i) th_t[i] = th_c[i] + delta[i];
#pragma unroll
    for (int i = PA; i < P; ++i) th_t[i] = th_c[i];
    lam_used = lam;
  }
#pragma unroll
  for (int i = 0; i < P; ++i) theta[(int64_t)i * n_pix + p] = th_c[i];
  chi2[p] = chi_c;
  // the packed upper triangle of the P x P matrix: N of the active parameters, the identity's rows
  // of a baseline held by the template
  {
    int q = 0;
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
      for (int j = i; j < P; ++j, ++q)
        cov[(int64_t)q * n_pix + p] =
            (i < PA && j < PA) ? Nc[lm_tri<PA>(i < PA ? i : 0, j < PA ? j : 0)] : (i == j ? 1.0 : 0.0);
  }
  o_nchan[p] = cnt;
  o_niter[p] = it;
  o_status[p] = status;
}

hipError_t specfit_launch(const double* cube, int64_t n_pix, int n_chan, const double* d_x,
                          const double* d_w, double x_ref, const uint8_t* mask, int n_comp,
                          unsigned free_bits, double* theta, double lambda0, double xtol,
                          int n_iter, double* chi2, double* cov, int32_t* nchan, int32_t* niter,
                          int32_t* status, double* trace, hipStream_t st) {
  const dim3 grid((unsigned)specfit_workgroups(n_pix)), block(kSfB);
  const bool bl = ((free_bits >> (3 * n_comp)) & 3u) != 0;
#define RJP_SF(NC, B)                                                                             \
  hipLaunchKernelGGL((specfit_kernel<NC, B>), grid, block, 0, st, cube, n_pix, n_chan, d_x, d_w,  \
                     x_ref, mask, free_bits, theta, lambda0, xtol, n_iter, chi2, cov, nchan,      \
                     niter, status, trace)
  if (n_comp == 1) {
    if (bl) RJP_SF(1, true); else RJP_SF(1, false);
  } else {
    if (bl) RJP_SF(2, true); else RJP_SF(2, false);
  }
#undef RJP_SF
  return hipGetLastError();
}

}  // namespace rjp
