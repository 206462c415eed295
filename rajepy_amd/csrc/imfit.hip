// K14 (rjp_gaussfit): a Levenberg-Marquardt fit of one elliptical Gaussian per map to a stack of
// images -- what the reference gets from CASA imfit on the restored image (classes.py:2790-2840).
//
// Model, pixel order p = ix nz + iz as K10-K13:
//   G(ix, iz) = S exp(-(A dx^2 + 2 B dx dz + C dz^2)),  dx = ix - x0, dz = iz - z0,
// theta = (S, x0, z0, A, B, C), (A, B, C) the quadratic form of beam_quadratic in cells^-2; no angle,
// so a circular source is not degenerate; no offset.  exp_any, an exact 0 below an exponent of -700
// (K13's rule).  A pixel counts when it lies in the box (i0, i1, j0, j1), is non-zero in the mask
// (if any) and is finite in the image.  r = I - G, J = dG / dtheta,
//   chi^2 = sum r^2,  N = J^T J (packed upper triangle, 21),  g = J^T r (6).
//
// The launches, the block sum and the decision are lm_common.h's; a tile is 1024 consecutive pixels
// of the box in the box's own row-major order; thread 0 keeps theta_cur, N and g in registers
// while it decides (in LDS the decision cost 4 % at 4096 workgroups).  The policy: feasible = (A, B, C) positive definite;
// the step scales s = (max(|S|, 1e-300), 1, 1, A + C, A + C, A + C); enough = 6 counting pixels;
// every parameter is free.
#include "lm_common.h"

namespace rjp {

__device__ __forceinline__ bool gf_posdef(double A, double B, double C) {
  return A > 0.0 && C > 0.0 && A * C > B * B;
}

struct GfPolicy {
  static constexpr int P = 6;
  static __device__ __forceinline__ bool feasible(const double* th) {
    return gf_posdef(th[3], th[4], th[5]);
  }
  // (|S| = 0 would make 0 / 0, which fmax drops: the floor keeps S in the test)
  static __device__ __forceinline__ void scales(const double* th, double (&s)[6]) {
    s[0] = __builtin_fmax(__builtin_fabs(th[0]), 1e-300);
    s[1] = s[2] = 1.0;
    s[3] = s[4] = s[5] = th[3] + th[5];
  }
  static __device__ __forceinline__ bool enough(double count, unsigned) { return count >= 6.0; }
};
using GfState = LmState<6>;        // 29 sums per tile, 48 doubles of state per map

LmTiling gaussfit_tiling(int n_maps, int64_t box_pixels) { return lm_tiling(n_maps, box_pixels); }

size_t gaussfit_workspace_bytes(int n_maps, int64_t box_pixels) {
  return lm_workspace_bytes(lm_tiling(n_maps, box_pixels), n_maps, GfState::Q, GfState::S);
}

__global__ __launch_bounds__(kLmB) void gaussfit_step_kernel(
    const double* __restrict__ img, int64_t npix, int nz, int i0, int j0, int bw, int64_t nbox,
    const uint8_t* __restrict__ mask, LmLaunch lm,
    const double* __restrict__ p_in, double* __restrict__ p_out, const double* __restrict__ s_in,
    double* __restrict__ s_out) {
  constexpr int Q = GfState::Q;
  __shared__ LmLds<6> l;
  LmCur<6> cur;                                      // (thread 0's registers)
  const int tid = threadIdx.x;
  const int tile = (int)(blockIdx.x % (unsigned)lm.tiles), m = (int)(blockIdx.x / (unsigned)lm.tiles);
  if (!lm_begin<GfPolicy>(lm, p_in, s_in, s_out, tile, m, 0x3fu, l, cur)) return;
  const double S = l.dec[0], x0 = l.dec[1], z0 = l.dec[2];
  const double A = l.dec[3], B2 = 2.0 * l.dec[4], C = l.dec[5];
  const double* __restrict__ im = img + (int64_t)m * npix;
  double v[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) v[q] = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // (32-bit: an index of the box, a tile's tail beyond it included, is below 2^31 + 1024)
    const unsigned b = (unsigned)tile * (unsigned)kLmT + (unsigned)(tid + kLmB * j);
    if ((int64_t)b >= nbox) continue;
    const unsigned bx = b / (unsigned)bw, bz = b - bx * (unsigned)bw;
    const int ix = i0 + (int)bx, iz = j0 + (int)bz;
    const int64_t p = (int64_t)ix * nz + iz;
    if (mask && mask[p] == 0) continue;
    const double I = im[p];
    if (!finite_d(I)) continue;
    const double dx = (double)ix - x0, dz = (double)iz - z0;
    const double xx = dx * dx, xz = dx * dz, zz = dz * dz;
    const double e = -(A * xx + B2 * xz + C * zz);
    // (NaN compares false -> exp_any -> NaN: such a trial is rejected)
    const double ex = e < -700.0 ? 0.0 : exp_any(e);
    const double G = S * ex, r = I - G;
    double J[6];
    J[0] = ex;
    J[1] = G * (2.0 * A * dx + B2 * dz);
    J[2] = G * (B2 * dx + 2.0 * C * dz);
    J[3] = -G * xx;
    J[4] = -2.0 * G * xz;
    J[5] = -G * zz;
    v[0] = __builtin_fma(r, r, v[0]);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
      for (int c = i; c < 6; ++c)
        v[1 + lm_tri<6>(i, c)] = __builtin_fma(J[i], J[c], v[1 + lm_tri<6>(i, c)]);
      v[22 + i] = __builtin_fma(J[i], r, v[22 + i]);
    }
    v[28] += 1.0;
  }
  lm_store_partials<Q>(v, p_out, lm.tiles, tile, m, l);
}

hipError_t gaussfit_launch(const double* img, int n_maps, int nx, int nz, const int32_t* box,
                           const uint8_t* mask, double* theta, double lambda0, double xtol,
                           int n_iter, double* chi2, double* cov, int32_t* npix, int32_t* niter,
                           int32_t* status, double* trace, void* work, hipStream_t st) {
  const int bw = box[3] - box[2] + 1;
  const int64_t nbox = (int64_t)(box[1] - box[0] + 1) * bw;
  const LmTiling t = lm_tiling(n_maps, nbox);
  return lm_launch_loop(
      t, n_maps, GfState::Q, GfState::S, lambda0, xtol, n_iter, theta, chi2, cov, npix, niter, status,
      trace, work,
      [&](const LmLaunch& a, const double* p_in, double* p_out, const double* s_in, double* s_out) {
        hipLaunchKernelGGL(gaussfit_step_kernel, dim3((unsigned)t.workgroups), dim3(kLmB), 0, st,
                           img, (int64_t)nx * nz, nz, box[0], box[2], bw, nbox, mask, a, p_in, p_out,
                           s_in, s_out);
      });
}

}  // namespace rjp
