// K20 (rjp_uvfit): a Levenberg-Marquardt fit of n_comp point / elliptical-Gaussian components per
// map to a stack of visibility sets -- what radio astronomers get from CASA uvmodelfit or difmap
// modelfit.  CASA is not at hand: this comment IS the definition, parity is not claimed.
//
// Model.  For map m and visibility k, a = su[m] * u[k], b = sv[m] * v[k] (one product each, cycles
// per cell, K10's convention), and per component c with theta_c = (F, x, z, sxx, sxz, szz):
//   ph = fma(a, x, b * z)                           the phase in turns; (sn, cs) = sincos_2pi(ph)
//   q  = fma(sxx, a * a, fma(2 sxz, a * b, szz * (b * b)))
//   e  = q * -19.739208802178716 (= -2 pi^2)        E = e < -700 ? 0 : exp_any(e)
//   A  = F * E,   M_c = (A * cs, -(A * sn))         M = sum_c M_c, added in component order
// A point source is sxx = sxz = szz = 0: q = 0, E = 1 exactly.  With ka = 6.283185307179586 * a,
// kb likewise, pa = -19.739208802178716 * (a * a), pab = -39.478417604357432 * (a * b), pb = the
// same as pa with b, the Jacobian columns (re, im) of component c are
//   dF   (E * cs, -(E * sn))          dx   (Im M_c * ka, -(Re M_c * ka))     dz   the same with kb
//   dsxx (Re M_c * pa, Im M_c * pa)   dsxz (... * pab)                       dszz (... * pb)
// Visibility k of map m counts when Re V, Im V, u, v and w are finite and w > 0 (w = 1 without
// weights).  With r = V - M:
//   chi^2 = sum w |r|^2,  N = Re(J^H W J) (packed upper triangle, T = P (P + 1) / 2),  g = Re(J^H W r)
// accumulated per visibility as fma(w * Re, Re, .) then fma(w * Im, Im, .), the weight on the left
// factor (for N: the column with the lower index).  P = 6 n_comp.
//
// The launches, the block sum (four passes for two components) and the decision are lm_common.h's;
// a tile is 1024 consecutive visibilities, and the partial sums of a thread live in registers (92
// doubles for two components).  The policy: feasible = every component's Sigma is positive
// SEMI-definite (sxx >= 0, szz >= 0, sxx szz >= sxz^2); the step scales s = (max(|F|, 1e-300), 1,
// 1, t, t, t), t = max(sxx + szz, 1) per component; enough = 2 count >= the number of free
// parameters; `free_bits` is the caller's.
#include "lm_common.h"

namespace rjp {

constexpr double kUfM2Pi2 = -19.739208802178716;   // -2 pi^2
constexpr double kUfM4Pi2 = -39.478417604357432;   // -4 pi^2
constexpr double kUf2Pi = 6.283185307179586;

template <int NC>
struct UfPolicy {
  static constexpr int P = 6 * NC;
  static __device__ __forceinline__ bool feasible(const double* th) {
    bool psd = true;
    for (int c = 0; c < NC; ++c) {
      const double sxx = th[6 * c + 3], sxz = th[6 * c + 4], szz = th[6 * c + 5];
      psd = psd && sxx >= 0.0 && szz >= 0.0 && sxx * szz >= sxz * sxz;
    }
    return psd;
  }
  // (|F| = 0 would make 0 / 0, which fmax drops: the floor keeps F in the test)
  static __device__ __forceinline__ void scales(const double* th, double (&s)[P]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      s[6 * c] = __builtin_fmax(__builtin_fabs(th[6 * c]), 1e-300);
      s[6 * c + 1] = s[6 * c + 2] = 1.0;
      s[6 * c + 3] = s[6 * c + 4] = s[6 * c + 5] = __builtin_fmax(th[6 * c + 3] + th[6 * c + 5], 1.0);
    }
  }
  static __device__ __forceinline__ bool enough(double count, unsigned free_bits) {
    return 2.0 * count >= (double)__builtin_popcount(free_bits);
  }
};

LmTiling uvfit_tiling(int n_maps, int64_t n_vis) { return lm_tiling(n_maps, n_vis); }

size_t uvfit_workspace_bytes(int n_maps, int64_t n_vis, int n_comp) {
  return lm_workspace_bytes(lm_tiling(n_maps, n_vis), n_maps,
                            n_comp == 1 ? LmState<6>::Q : LmState<12>::Q,
                            n_comp == 1 ? LmState<6>::S : LmState<12>::S);
}

template <int NC>
__global__ __launch_bounds__(kLmB) void uvfit_step_kernel(
    const double* __restrict__ vis, const double* __restrict__ u, const double* __restrict__ v,
    const double* __restrict__ w, int64_t w_stride, const double* __restrict__ su,
    const double* __restrict__ sv, int n_vis, unsigned free_bits, LmLaunch lm,
    const double* __restrict__ p_in, double* __restrict__ p_out, const double* __restrict__ s_in,
    double* __restrict__ s_out) {
  using U = LmState<6 * NC>;
  constexpr int P = U::P, T = U::T, Q = U::Q;
  __shared__ LmLds<P> l;
  __shared__ LmCur<P> cur;
  const int tid = threadIdx.x;
  const int tile = (int)(blockIdx.x % (unsigned)lm.tiles), m = (int)(blockIdx.x / (unsigned)lm.tiles);
  if (!lm_begin<UfPolicy<NC>>(lm, p_in, s_in, s_out, tile, m, free_bits, l, cur)) return;
  double th[P];
#pragma unroll
  for (int i = 0; i < P; ++i) th[i] = l.dec[i];
  const double sum = su[m], svm = sv[m];
  const double* __restrict__ vm = vis + (int64_t)m * n_vis * 2;
  const double* __restrict__ wm = w ? w + (int64_t)m * w_stride : nullptr;
  double acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = 0.0;
#pragma unroll 1
  for (int j = 0; j < 4; ++j) {
    // (64-bit: tile * 1024 + 1023 may pass 2^31 for n_vis near it)
    const int64_t k = (int64_t)tile * kLmT + (tid + kLmB * j);
    if (k >= n_vis) continue;
    const double uk = u[k], vk = v[k], wk = wm ? wm[k] : 1.0;
    const double vr = vm[2 * k], vi = vm[2 * k + 1];
    if (!(finite_d(uk) && finite_d(vk) && finite_d(wk) && wk > 0.0 && finite_d(vr) && finite_d(vi)))
      continue;
    const double a = sum * uk, b = svm * vk;
    const double aa = a * a, ab = a * b, bb = b * b;
    const double ka = kUf2Pi * a, kb = kUf2Pi * b;
    const double pa = kUfM2Pi2 * aa, pab = kUfM4Pi2 * ab, pb = kUfM2Pi2 * bb;
    double Jr[P], Ji[P];
    double mr = 0.0, mi = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const double F = th[6 * c], x = th[6 * c + 1], z = th[6 * c + 2];
      const double sxx = th[6 * c + 3], sxz2 = 2.0 * th[6 * c + 4], szz = th[6 * c + 5];
      double sn, cs;
      sincos_2pi(__builtin_fma(a, x, b * z), sn, cs);
      const double q = __builtin_fma(sxx, aa, __builtin_fma(sxz2, ab, szz * bb));
      const double e = q * kUfM2Pi2;
      // (NaN compares false -> exp_any -> NaN: such a trial is rejected)
      const double E = e < -700.0 ? 0.0 : exp_any(e);
      const double A = F * E;
      const double cr = A * cs, ci = -(A * sn);
      Jr[6 * c] = E * cs;
      Ji[6 * c] = -(E * sn);
      Jr[6 * c + 1] = ci * ka;
      Ji[6 * c + 1] = -(cr * ka);
      Jr[6 * c + 2] = ci * kb;
      Ji[6 * c + 2] = -(cr * kb);
      Jr[6 * c + 3] = cr * pa;
      Ji[6 * c + 3] = ci * pa;
      Jr[6 * c + 4] = cr * pab;
      Ji[6 * c + 4] = ci * pab;
      Jr[6 * c + 5] = cr * pb;
      Ji[6 * c + 5] = ci * pb;
      mr += cr;
      mi += ci;
    }
    const double rr = vr - mr, ri = vi - mi;
    acc[0] = __builtin_fma(wk * rr, rr, acc[0]);
    acc[0] = __builtin_fma(wk * ri, ri, acc[0]);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const double wr = wk * Jr[p], wi = wk * Ji[p];
#pragma unroll
      for (int c = p; c < P; ++c) {
        double s = acc[1 + lm_tri<P>(p, c)];
        s = __builtin_fma(wr, Jr[c], s);
        acc[1 + lm_tri<P>(p, c)] = __builtin_fma(wi, Ji[c], s);
      }
      double s = acc[1 + T + p];
      s = __builtin_fma(wr, rr, s);
      acc[1 + T + p] = __builtin_fma(wi, ri, s);
    }
    acc[Q - 1] += 1.0;
  }
  lm_store_partials<Q>(acc, p_out, lm.tiles, tile, m, l);
}

template <int NC>
static hipError_t uvfit_launch_n(const double* vis, int n_maps, int n_vis, const double* d_su,
                                 const double* d_sv, const double* u, const double* v,
                                 const double* w, int64_t w_stride, unsigned free_bits,
                                 const LmTiling& t, double* theta, double lambda0, double xtol,
                                 int n_iter, double* chi2, double* cov, int32_t* nvis, int32_t* niter,
                                 int32_t* status, double* trace, void* work, hipStream_t st) {
  using U = LmState<6 * NC>;
  return lm_launch_loop(
      t, n_maps, U::Q, U::S, lambda0, xtol, n_iter, theta, chi2, cov, nvis, niter, status, trace, work,
      [&](const LmLaunch& a, const double* p_in, double* p_out, const double* s_in, double* s_out) {
        hipLaunchKernelGGL(uvfit_step_kernel<NC>, dim3((unsigned)t.workgroups), dim3(kLmB), 0, st, vis,
                           u, v, w, w_stride, d_su, d_sv, n_vis, free_bits, a, p_in, p_out, s_in, s_out);
      });
}

hipError_t uvfit_launch(const double* vis, int n_maps, int n_vis, const double* d_su,
                        const double* d_sv, const double* u, const double* v, const double* w,
                        int w_maps, int n_comp, unsigned free_bits, double* theta, double lambda0,
                        double xtol, int n_iter, double* chi2, double* cov, int32_t* nvis,
                        int32_t* niter, int32_t* status, double* trace, void* work,
                        hipStream_t st) {
  const LmTiling t = lm_tiling(n_maps, n_vis);
  const int64_t w_stride = w && w_maps == n_maps && n_maps > 1 ? n_vis : 0;
  if (n_comp == 1)
    return uvfit_launch_n<1>(vis, n_maps, n_vis, d_su, d_sv, u, v, w, w_stride, free_bits, t, theta,
                             lambda0, xtol, n_iter, chi2, cov, nvis, niter, status, trace, work, st);
  return uvfit_launch_n<2>(vis, n_maps, n_vis, d_su, d_sv, u, v, w, w_stride, free_bits, t, theta,
                           lambda0, xtol, n_iter, chi2, cov, nvis, niter, status, trace, work, st);
}

}  // namespace rjp
