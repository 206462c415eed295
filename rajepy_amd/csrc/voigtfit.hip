// K24 (rjp_voigtfit): one Levenberg-Marquardt fit of n_comp area-normalised Voigt profiles plus a
// linear baseline per sightline of a line cube -- K21's fit (specfit.hip) with the profile the
// model's own lines have (K3, K6: a thermal Doppler core with pressure-broadened Lorentz wings), so
// that the fitted widths can be held against the physics.  The header comment (include/rjprt.h) IS
// the definition.
//
// Shape: K21's.  ONE LANE PER PIXEL, workgroups of one wave (64 pixels), channels ascending, the
// channel tables x and w through uniform loads, every sum a chain in channel order in the lane's
// own registers: no atomics, no cross-lane reduction, no workspace, and the bits of a pixel's
// outputs are a function of its spectrum and the tables alone.  The whole fit of a pixel in one
// launch: a lane keeps theta_cur, the trial, chi^2, N and g of theta_cur and the trial's sums,
// re-reads its spectrum once per trial and takes lm_common.h's decision for itself: feasible =
// every s finite and > 0 and every g finite and >= 0; the step scales max(|F|, 1e-300) for F and
// max(s, g, 1e-300) for x0, s and g per component, max(|b|, 1e-300) for a free baseline parameter;
// enough = count >= the number of free parameters.  lm_tri, lm_solve and lm_step_converged are the
// header's; the take-over of a trial's sums and the breakdown loop are written out as in K21.
//
// w(u + i a) is voigt_w.h's, per lane: a lane takes the lattice or the continued fraction by its
// own (u, a), so a wave pays for both where its lanes differ.  Templated on n_comp and on whether a
// baseline parameter is free (BL) as K21 is: with both held the sums and the Cholesky run on the
// 4 n_comp line parameters alone.
//
// Where N and g of theta_cur live.  At two components P = 10: N_cur and N_trial are 2 x 55 doubles,
// the triangle of the Cholesky 55 more.  N and g of theta_cur are touched on an accept and in the
// solve only, so the kernel keeps them in LDS, each lane its own column ([entry][lane], so a wave's
// access to one entry is 64 consecutive doubles: no bank conflict, and no barrier, because no lane
// reads another's column): 64 x 65 doubles = 33 KiB at <2, true>.  This is the one departure
// from K21's "no LDS"; the channel loop itself touches registers only.
#include "lm_common.h"
#include "voigt_w.h"

namespace rjp {

constexpr int kVfB = 64;           // pixels per workgroup: one wave

// a lane's column of an LDS array [n][kVfB]
struct VfCol {
  double* p;
  __device__ __forceinline__ double& operator[](int i) const { return p[i * kVfB]; }
};

template <int NC, bool BL>
__global__ __launch_bounds__(kVfB) void voigtfit_kernel(
    const double* __restrict__ cube, int64_t n_pix, int n_chan, const double* __restrict__ x,
    const double* __restrict__ w, double x_ref, const uint8_t* __restrict__ mask,
    unsigned free_bits, double* __restrict__ theta, double lambda0, double xtol, int n_iter,
    double* __restrict__ chi2, double* __restrict__ cov, int* __restrict__ o_nchan,
    int* __restrict__ o_niter, int* __restrict__ o_status, double* __restrict__ trace) {
  constexpr int P = 4 * NC + 2;                      // the parameters of a pixel
  constexpr int PA = BL ? P : 4 * NC;                // those that enter N and g
  constexpr int TA = PA * (PA + 1) / 2;
  __shared__ double lds[(TA + PA) * kVfB];
  const VfCol Nc{lds + threadIdx.x}, gc{lds + TA * kVfB + threadIdx.x};
  const int64_t p = (int64_t)blockIdx.x * kVfB + threadIdx.x;
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
  for (int c = 0; c < NC; ++c) good = good && th_c[4 * c + 2] > 0.0 && th_c[4 * c + 3] >= 0.0;
  if (!good) {
    o_status[p] = 3;
    return;
  }
  const int n_free = __builtin_popcount(free_bits);
  const double* __restrict__ col = cube + p;
  double* __restrict__ row = trace ? trace + p * n_iter * (3 + P) : nullptr;
#pragma unroll
  for (int i = 0; i < TA; ++i) Nc[i] = 0.0;
#pragma unroll
  for (int i = 0; i < PA; ++i) gc[i] = 0.0;
  double chi_c = __builtin_inf(), lam = lambda0, lam_used = lambda0;
  int cnt = 0, status = 0, it = 1;
  for (;; ++it) {
    // one trial: chi^2, N, g of th_t over the counted channels, ascending
    double chi_t = 0.0, Nt[TA], gt[PA], rs[NC], q[NC], av[NC], cn[NC];
#pragma unroll
    for (int i = 0; i < TA; ++i) Nt[i] = 0.0;
#pragma unroll
    for (int i = 0; i < PA; ++i) gt[i] = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      rs[c] = 1.0 / th_t[4 * c + 2];
      q[c] = rs[c] * 0.70710678118654752440;
      av[c] = th_t[4 * c + 3] * q[c];
      cn[c] = rs[c] * 0.39894228040143267794;
    }
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
        const double u = (xc - th_t[4 * k + 1]) * q[k];
        const double a = av[k];
        double K, L;
        // (a NaN or infinite u gives NaN: such a trial is rejected)
        voigt_w(u, a, K, L);
        const double Rw = -2.0 * __builtin_fma(u, K, -(a * L));
        const double Iw = __builtin_fma(-2.0, __builtin_fma(u, L, a * K), 1.1283791670955125739);
        const double cF = th_t[4 * k] * cn[k];
        const double cq = cF * q[k];
        const double ck = cF * K;
        J[4 * k] = K * cn[k];
        J[4 * k + 1] = -(cq * Rw);
        J[4 * k + 2] = -(cF * rs[k]) * __builtin_fma(-a, Iw, __builtin_fma(u, Rw, K));
        J[4 * k + 3] = -(cq * Iw);
        m = k == 0 ? ck : m + ck;
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
    for (int c = 0; c < NC; ++c)
      feas = feas && finite_d(th_t[4 * c + 2]) && th_t[4 * c + 2] > 0.0 &&
             finite_d(th_t[4 * c + 3]) && th_t[4 * c + 3] >= 0.0;
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
      scale[4 * c] = __builtin_fmax(__builtin_fabs(th_c[4 * c]), 1e-300);
      scale[4 * c + 1] = scale[4 * c + 2] = scale[4 * c + 3] =
          __builtin_fmax(__builtin_fmax(th_c[4 * c + 2], th_c[4 * c + 3]), 1e-300);
    }
#pragma unroll
    for (int i = 4 * NC; i < PA; ++i) scale[i] = __builtin_fmax(__builtin_fabs(th_c[i]), 1e-300);
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
    int k = 0;
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
      for (int j = i; j < P; ++j, ++k)
        cov[(int64_t)k * n_pix + p] =
            (i < PA && j < PA) ? Nc[lm_tri<PA>(i < PA ? i : 0, j < PA ? j : 0)] : (i == j ? 1.0 : 0.0);
  }
  o_nchan[p] = cnt;
  o_niter[p] = it;
  o_status[p] = status;
}

hipError_t voigtfit_launch(const double* cube, int64_t n_pix, int n_chan, const double* d_x,
                           const double* d_w, double x_ref, const uint8_t* mask, int n_comp,
                           unsigned free_bits, double* theta, double lambda0, double xtol,
                           int n_iter, double* chi2, double* cov, int32_t* nchan, int32_t* niter,
                           int32_t* status, double* trace, hipStream_t st) {
  const dim3 grid((unsigned)specfit_workgroups(n_pix)), block(kVfB);
  const bool bl = ((free_bits >> (4 * n_comp)) & 3u) != 0;
#define RJP_VF(NC, B)                                                                             \
  hipLaunchKernelGGL((voigtfit_kernel<NC, B>), grid, block, 0, st, cube, n_pix, n_chan, d_x, d_w, \
                     x_ref, mask, free_bits, theta, lambda0, xtol, n_iter, chi2, cov, nchan,      \
                     niter, status, trace)
  if (n_comp == 1) {
    if (bl) RJP_VF(1, true); else RJP_VF(1, false);
  } else {
    if (bl) RJP_VF(2, true); else RJP_VF(2, false);
  }
#undef RJP_VF
  return hipGetLastError();
}

}  // namespace rjp
