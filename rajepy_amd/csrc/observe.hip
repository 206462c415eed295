// K16 (rjp_uv_tracks, rjp_vis_noise): the two device halves of a synthetic observation -- what the
// reference leaves to CASA simobserve (classes.py:2490-2650): the (u, v, w) tracks of an array under
// earth rotation, and thermal noise on the visibilities.
//
// uv_tracks_kernel   one thread per (integration t, baseline p), workgroup b = tile b % tb of 256
//                    baselines of integration b / tb.  The pair (i < j) of p in i-major order is
//                    decoded with one double sqrt and an integer fix-up (a float decode fails past
//                    2^15 pairs); the hour angle is reduced EXACTLY to |g| <= 1/2 turn (g - rint(g))
//                    and goes through sincos_2pi; three baseline differences and eleven
//                    products / FMAs give (u, v, w).  The elevation flag of an antenna is one dot
//                    product of its vertical with the source direction.  24 bytes written per
//                    (t, p), 48 + 48 bytes of tables read (cached: 3 n_ant + n_t doubles in all).
// vis_noise_kernel   one thread per (map m, visibility k): ONE Philox4x32-10 block, keyed by the
//                    seed, counted by (k0 + k, m0 + m) -- a pure function of (seed, map, visibility),
//                    whatever the launch shape -- gives the two uniforms of one Box-Muller pair, the
//                    real and the imaginary part.  16 bytes read, 16 written (+ 8 with d_s); ~100
//                    integer and ~120 FP64 operations: memory bound only on paper, the log and the
//                    two polynomials decide.  No atomics, no LDS, no cross-lane traffic.
#include "rjp_host.h"

namespace rjp {

constexpr int kObB = 256;          // threads per workgroup

int64_t uv_tracks_workgroups(int n_ant, int n_t) {
  const int64_t n_bl = (int64_t)n_ant * (n_ant - 1) / 2;
  return (int64_t)n_t * ((n_bl + kObB - 1) / kObB);
}

int64_t vis_noise_workgroups(int n_maps, int n_vis) {
  return (int64_t)n_maps * (((int64_t)n_vis + kObB - 1) / kObB);
}

// pairs before row i of the i-major list of (i < j) pairs of n antennas
__device__ __forceinline__ int64_t ob_row_start(int64_t i, int64_t n) {
  return i * (2 * n - i - 1) / 2;
}

__global__ __launch_bounds__(kObB) void uv_tracks_kernel(
    const double* __restrict__ xyz, const double* __restrict__ gha, const double* __restrict__ up,
    int n_ant, int64_t n_bl, int tb, double sd, double cd, double sin_min_el,
    double* __restrict__ u, double* __restrict__ v, double* __restrict__ w) {
  const int t = (int)(blockIdx.x / (unsigned)tb);
  const int64_t p = (int64_t)(blockIdx.x % (unsigned)tb) * kObB + threadIdx.x;
  if (p >= n_bl) return;
  // p -> (i, j): the root of i (2 n - i - 1) / 2 = p, then at most a step either way
  const int64_t n = n_ant;
  const double a = (double)(2 * n - 1);
  int64_t i = (int64_t)((a - __builtin_sqrt(__builtin_fma(a, a, -8.0 * (double)p))) * 0.5);
  i = i < 0 ? 0 : (i > n - 2 ? n - 2 : i);
  while (i > 0 && ob_row_start(i, n) > p) --i;
  while (i < n - 2 && ob_row_start(i + 1, n) <= p) ++i;
  const int64_t j = p - ob_row_start(i, n) + i + 1;
  const double nan = __builtin_nan("");
  double uo = nan, vo = nan, wo = nan;
  const double g0 = gha[t];
  if (finite_d(g0)) {
    double sG, cG;
    sincos_2pi(g0 - __builtin_rint(g0), sG, cG);
    bool ok = true;
    if (up) {
      const double sx = cd * cG, sy = -(cd * sG);
      const double ei = __builtin_fma(up[3 * i + 2], sd, __builtin_fma(up[3 * i + 1], sy, up[3 * i] * sx));
      const double ej = __builtin_fma(up[3 * j + 2], sd, __builtin_fma(up[3 * j + 1], sy, up[3 * j] * sx));
      ok = !(ei < sin_min_el) && !(ej < sin_min_el);
    }
    if (ok) {
      const double bx = xyz[3 * j] - xyz[3 * i];
      const double by = xyz[3 * j + 1] - xyz[3 * i + 1];
      const double bz = xyz[3 * j + 2] - xyz[3 * i + 2];
      uo = __builtin_fma(sG, bx, cG * by);
      vo = __builtin_fma(cd, bz, sd * __builtin_fma(sG, by, -(cG * bx)));
      wo = __builtin_fma(sd, bz, cd * __builtin_fma(-sG, by, cG * bx));
    }
  }
  const int64_t o = (int64_t)t * n_bl + p;
  u[o] = uo;
  v[o] = vo;
  if (w) w[o] = wo;
}

hipError_t uv_tracks_launch(const double* d_xyz, int n_ant, const double* d_gha, int n_t,
                            double sin_dec, double cos_dec, const double* d_up, double sin_min_el,
                            double* u, double* v, double* w, hipStream_t st) {
  const int64_t n_bl = (int64_t)n_ant * (n_ant - 1) / 2;
  const int tb = (int)((n_bl + kObB - 1) / kObB);
  hipLaunchKernelGGL(uv_tracks_kernel, dim3((unsigned)((int64_t)n_t * tb)), dim3(kObB), 0, st, d_xyz,
                     d_gha, d_up, n_ant, n_bl, tb, sin_dec, cos_dec, sin_min_el, u, v, w);
  return hipGetLastError();
}

// ---- Philox4x32-10 (Salmon et al. 2011) -------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t (&x)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// (2 n + 1) 2^-53 with n the 52 bits (hi << 20) | (lo >> 12): exact, strictly inside (0, 1)
__device__ __forceinline__ double ob_unit(uint32_t hi, uint32_t lo) {
  const uint64_t n = ((uint64_t)hi << 20) | (uint64_t)(lo >> 12);
  return (double)(2 * n + 1) * 1.1102230246251565404e-16;
}

__global__ __launch_bounds__(kObB) void vis_noise_kernel(
    const double2* vis, int n_vis, int kb, const double* __restrict__ sigma,
    const double* __restrict__ s, uint32_t key0, uint32_t key1, uint64_t k0, uint32_t m0,
    double2* out) {            // (out may be vis: neither is __restrict__)
  const int m = (int)(blockIdx.x / (unsigned)kb);
  const int64_t k = (int64_t)(blockIdx.x % (unsigned)kb) * kObB + threadIdx.x;
  if (k >= n_vis) return;
  const int64_t o = (int64_t)m * n_vis + k;
  double2 val = vis[o];           // (read before the store: d_out may be d_vis)
  const double sk = s ? s[k] : 1.0;
  const double sg = sigma[m];
  if (!finite_d(sk)) {
    val.x = val.y = __builtin_nan("");
  } else if (sg != 0.0) {         // sigma = 0: the bits of the input, -0.0 included
    const uint64_t kk = k0 + (uint64_t)k;
    uint32_t x[4];
    philox4x32_10((uint32_t)kk, (uint32_t)(kk >> 32), m0 + (uint32_t)m, 0u, key0, key1, x);
    const double u1 = ob_unit(x[0], x[1]), u2 = ob_unit(x[2], x[3]);
    const double r = __builtin_sqrt(-2.0 * log(u1));
    double sn, cs;
    sincos_2pi(u2, sn, cs);
    const double ar = (sg * sk) * r;
    val.x = __builtin_fma(ar, cs, val.x);
    val.y = __builtin_fma(ar, sn, val.y);
  }
  out[o] = val;
}

hipError_t vis_noise_launch(const double* vis, int n_maps, int n_vis, const double* d_sigma,
                            const double* s, uint64_t seed, int64_t k0, int m0, double* out,
                            hipStream_t st) {
  const int kb = (int)(((int64_t)n_vis + kObB - 1) / kObB);
  hipLaunchKernelGGL(vis_noise_kernel, dim3((unsigned)((int64_t)n_maps * kb)), dim3(kObB), 0, st,
                     (const double2*)vis, n_vis, kb, d_sigma, s, (uint32_t)seed,
                     (uint32_t)(seed >> 32), (uint64_t)k0, (uint32_t)m0, (double2*)out);
  return hipGetLastError();
}

}  // namespace rjp
