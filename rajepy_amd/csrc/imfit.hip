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
// One launch per iteration for the whole stack, grid = tiles x maps; a tile is kGfT = 1024
// consecutive pixels of the box in the box's own row-major order, thread tid owns the pixels
// t0 + tid + 256 j, j < 4.  Launch k = 0 .. n_iter; a workgroup of launch k >= 1
//   1. reduces the 29 partial sums (chi^2, N, g, count) that launch k - 1 left per tile of its map
//      for the trial point theta_t -- every workgroup redundantly and in the same order, thread i the
//      tiles i, i + 256, ..., then the block sum below;
//   2. thread 0 decides the iteration (gf_decide) and broadcasts the next trial through LDS;
//   3. every thread evaluates that trial on its pixels; the block sum goes to the other half of the
//      double-buffered partials;
//   4. (tile 0 only) writes the map's state to the other half of the double-buffered state, the
//      trace row, and in launch n_iter the outputs.
// Launch 0 only takes the start from d_theta as the first trial.  Workgroups of one launch exchange
// nothing; the kernel boundary makes launch k's writes visible to launch k + 1, as in K12.  A
// finished map's workgroups skip 1-3; tile 0 carries the state over.  No atomics; every sum in a
// fixed order: the same bits on every call.
//
// The block sum of 29 values per thread goes through LDS, not through 29 x 6 cross-lane steps: each
// thread stores its values in rows of 8 x 33 doubles (the pad keeps the eight 32-term partial sums of
// a row on different banks), 232 threads add 32 consecutive entries each, 29 threads add the 8
// partial sums.
//
// The decision, in this order (trial theta_t with sums chi_t, N_t, g_t):
//   accept iff theta_t is positive definite, chi_t is finite and chi_t < chi_cur (+inf before the
//   first trial).  accept: (theta, chi, N, g)_cur <- trial, lambda <- max(lambda / 10, 1e-12) (the
//   start's own acceptance leaves lambda0); reject: lambda <- 10 lambda.
//   chi_cur == 0 -> status 1.  Else solve (N + lambda diag N) delta = g by a 6 x 6 Cholesky; a
//   breakdown (a pivot not > 0) counts as a reject: lambda <- 10 lambda and again; lambda > 1e12 ->
//   status 2.  max_i |delta_i| / s_i <= xtol, s = (max(|S|, 1e-300), 1, 1, A + C, A + C, A + C)
//   -> status 1 (tested on every proposed step).  Launch n_iter -> status 0.  Else theta_t = theta_cur + delta.
//   First trial: fewer than 6 counting pixels or a chi^2 that is not finite -> status 3, as a start
//   that is not finite and positive definite in launch 0.
#include "rjp_host.h"

namespace rjp {

constexpr int kGfB = 256;          // threads per workgroup
constexpr int kGfT = 1024;         // pixels of the box per tile: four per thread
constexpr int kGfQ = 29;           // sums per tile: chi^2, N[21], g[6], count
constexpr int kGfS = 48;           // doubles of state per map (45 used)
constexpr int kGfRow = 8 * 33;     // LDS row of the block sum: 8 parts of 32 + 1 pad
// state: theta_cur 0..5, chi_cur 6, lambda 7, lambda of the trial 8, status 9, trials 10, pixels 11,
// theta_t 12..17, N 18..38, g 39..44
constexpr int kGfRun = -1;         // status while the fit goes on

GaussfitTiling gaussfit_tiling(int n_maps, int64_t box_pixels) {
  GaussfitTiling t;
  t.tiles = (box_pixels + kGfT - 1) / kGfT;
  t.workgroups = t.tiles * n_maps;
  return t;
}

// two halves of (29 sums per tile, 48 doubles of state) per map; 0: no size_t holds it
size_t gaussfit_workspace_bytes(int n_maps, int64_t box_pixels) {
  const GaussfitTiling t = gaussfit_tiling(n_maps, box_pixels);
  const unsigned __int128 n =
      ((unsigned __int128)t.workgroups * kGfQ + (unsigned __int128)n_maps * kGfS) * 2u * 8u;
  return n > (unsigned __int128)SIZE_MAX ? 0 : (size_t)n;
}

__device__ __forceinline__ bool gf_posdef(double A, double B, double C) {
  return A > 0.0 && C > 0.0 && A * C > B * B;
}

// index of (i, j), i <= j, in the packed upper triangle, row by row
__device__ __forceinline__ constexpr int gf_tri(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// s_tot[q] = sum over the workgroup of v[q], valid in every thread on return
__device__ __forceinline__ void gf_block_sum(const double (&v)[kGfQ], double* s_a, double* s_b,
                                             double* s_tot) {
  const int tid = threadIdx.x;
  const int slot = (tid >> 5) * 33 + (tid & 31);
  __syncthreads();                                  // earlier readers of s_a / s_b / s_tot are done
#pragma unroll
  for (int q = 0; q < kGfQ; ++q) s_a[q * kGfRow + slot] = v[q];
  __syncthreads();
  if (tid < kGfQ * 8) {
    const double* p = s_a + (tid >> 3) * kGfRow + (tid & 7) * 33;
    double a = p[0];
    for (int i = 1; i < 32; ++i) a += p[i];
    s_b[tid] = a;
  }
  __syncthreads();
  if (tid < kGfQ) {
    double a = s_b[tid * 8];
#pragma unroll
    for (int i = 1; i < 8; ++i) a += s_b[tid * 8 + i];
    s_tot[tid] = a;
  }
  __syncthreads();
}

// (N + lam diag N) delta = g by Cholesky, everything at compile-time indices (registers, no
// scratch); false: a pivot is not > 0
__device__ __forceinline__ bool gf_solve(const double (&N)[21], const double (&g)[6], double lam,
                                         double (&delta)[6]) {
  double L[21];                                      // L^T, packed like N: L[gf_tri(k, i)] = l_ik
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = __builtin_fma(lam, N[gf_tri(j, j)], N[gf_tri(j, j)]);
#pragma unroll
    for (int k = 0; k < j; ++k) d = __builtin_fma(-L[gf_tri(k, j)], L[gf_tri(k, j)], d);
    ok = ok && d > 0.0;
    const double l = __builtin_sqrt(d);
    L[gf_tri(j, j)] = l;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = N[gf_tri(j, i)];
#pragma unroll
      for (int k = 0; k < j; ++k) s = __builtin_fma(-L[gf_tri(k, i)], L[gf_tri(k, j)], s);
      L[gf_tri(j, i)] = s / l;
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = __builtin_fma(-L[gf_tri(k, i)], y[k], s);
    y[i] = s / L[gf_tri(i, i)];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s = __builtin_fma(-L[gf_tri(i, k)], delta[k], s);
    delta[i] = s / L[gf_tri(i, i)];
  }
  return ok;
}

// the outputs of a map from its final state (status 3: the status alone)
__device__ __forceinline__ void gf_outputs(const double* __restrict__ s, int m,
                                           double* __restrict__ theta, double* __restrict__ chi2,
                                           double* __restrict__ cov, int* __restrict__ npix,
                                           int* __restrict__ niter, int* __restrict__ status) {
  const int st = (int)s[9];
  status[m] = st == kGfRun ? 0 : st;
  if (st == 3) return;
  for (int i = 0; i < 6; ++i) theta[6 * m + i] = s[i];
  chi2[m] = s[6];
  for (int i = 0; i < 21; ++i) cov[21 * m + i] = s[18 + i];
  npix[m] = (int)s[11];
  niter[m] = (int)s[10];
}

// Step 2 of launch `it` >= 1 in thread 0: the state `si` and the trial's sums `tot` -> the state
// `so` (tile 0 stores it), the trace row, and the next trial in dec[0..5]; true: evaluate it.
__device__ __forceinline__ bool gf_decide(const double* __restrict__ si, const double* tot,
                                          double* __restrict__ so, bool store, int it, int n_iter,
                                          double xtol, double* __restrict__ trace_row, double* dec) {
  const bool first = it == 1;
  const double chi_t = tot[0], lam_used = si[8];
  double th[6], N[21], g[6];
  double lam = si[7], chi_cur = si[6];
  const double npix = first ? tot[28] : si[11];
  int status = kGfRun;
  bool eval = false;
  if (first && (!(tot[28] >= 6.0) || !finite_d(chi_t))) {
    if (store) {
      for (int i = 0; i < kGfS; ++i) so[i] = si[i];
      so[9] = 3.0;
    }
    return false;
  }
  const bool acc = gf_posdef(si[15], si[16], si[17]) && finite_d(chi_t) && chi_t < chi_cur;
  if (acc) {
#pragma unroll
    for (int i = 0; i < 6; ++i) th[i] = si[12 + i];
#pragma unroll
    for (int i = 0; i < 21; ++i) N[i] = tot[1 + i];
#pragma unroll
    for (int i = 0; i < 6; ++i) g[i] = tot[22 + i];
    chi_cur = chi_t;
    if (!first) lam = __builtin_fmax(lam / 10.0, 1e-12);
  } else {
#pragma unroll
    for (int i = 0; i < 6; ++i) th[i] = si[i];
#pragma unroll
    for (int i = 0; i < 21; ++i) N[i] = si[18 + i];
#pragma unroll
    for (int i = 0; i < 6; ++i) g[i] = si[39 + i];
    lam *= 10.0;
  }
  if (store && trace_row) {
    trace_row[0] = chi_t;
    trace_row[1] = lam_used;
    trace_row[2] = acc ? 1.0 : 0.0;
    for (int i = 0; i < 6; ++i) trace_row[3 + i] = si[12 + i];
  }
  double tn[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) tn[i] = si[12 + i];
  if (chi_cur == 0.0) {
    status = 1;
  } else {
    double delta[6];
    bool ok = false;
    // (at most 25 rounds: lambda >= 1e-12 grows tenfold per breakdown)
    while (true) {
      if (lam > 1e12) {
        status = 2;
        break;
      }
      if (gf_solve(N, g, lam, delta)) {
        ok = true;
        break;
      }
      lam *= 10.0;
    }
    if (ok) {
      const double sh = th[3] + th[5];
      // (|S| = 0 would make 0 / 0, which fmax drops: the floor keeps S in the test)
      double worst = __builtin_fabs(delta[0]) / __builtin_fmax(__builtin_fabs(th[0]), 1e-300);
      worst = __builtin_fmax(worst, __builtin_fmax(__builtin_fabs(delta[1]), __builtin_fabs(delta[2])));
#pragma unroll
      for (int i = 3; i < 6; ++i) worst = __builtin_fmax(worst, __builtin_fabs(delta[i]) / sh);
      bool nan = false;
#pragma unroll
      for (int i = 0; i < 6; ++i) nan = nan || delta[i] != delta[i];
      if (!nan && worst <= xtol) {
        status = 1;
      } else if (it == n_iter) {
        status = 0;
      } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) tn[i] = th[i] + delta[i];
        eval = true;
      }
    }
  }
  if (store) {
#pragma unroll
    for (int i = 0; i < 6; ++i) so[i] = th[i];
    so[6] = chi_cur;
    so[7] = lam;
    so[8] = eval ? lam : lam_used;
    so[9] = (double)status;
    so[10] = (double)it;
    so[11] = npix;
#pragma unroll
    for (int i = 0; i < 6; ++i) so[12 + i] = tn[i];
#pragma unroll
    for (int i = 0; i < 21; ++i) so[18 + i] = N[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) so[39 + i] = g[i];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) dec[i] = tn[i];
  return eval;
}

// launch `it` of n_iter + 1: partials p_in -> p_out ([n_maps][29][tiles]), state s_in -> s_out
__global__ __launch_bounds__(kGfB) void gaussfit_step_kernel(
    const double* __restrict__ img, int64_t npix, int nz, int i0, int j0, int bw, int64_t nbox,
    int tiles, const uint8_t* __restrict__ mask, double lambda0, double xtol, int it, int n_iter,
    const double* __restrict__ p_in, double* __restrict__ p_out, const double* __restrict__ s_in,
    double* __restrict__ s_out, double* __restrict__ theta, double* __restrict__ chi2,
    double* __restrict__ cov, int* __restrict__ o_npix, int* __restrict__ o_niter,
    int* __restrict__ o_status, double* __restrict__ trace) {
  __shared__ double s_a[kGfQ * kGfRow];
  __shared__ double s_b[kGfQ * 8];
  __shared__ double s_tot[32];
  __shared__ double s_dec[8];
  const int tid = threadIdx.x;
  const int tile = (int)(blockIdx.x % (unsigned)tiles), m = (int)(blockIdx.x / (unsigned)tiles);
  const double* __restrict__ si = s_in + (int64_t)m * kGfS;
  double* __restrict__ so = s_out + (int64_t)m * kGfS;
  const bool store = tile == 0;
  if (it == 0) {
    if (tid == 0) {
      double t0[6];
      bool good = true;
      for (int i = 0; i < 6; ++i) {
        t0[i] = theta[6 * m + i];
        good = good && finite_d(t0[i]);
        s_dec[i] = t0[i];
      }
      good = good && gf_posdef(t0[3], t0[4], t0[5]);
      s_dec[6] = good ? 1.0 : 0.0;
      if (store) {
        for (int i = 0; i < kGfS; ++i) so[i] = 0.0;
        for (int i = 0; i < 6; ++i) so[i] = so[12 + i] = t0[i];
        so[6] = __builtin_inf();
        so[7] = so[8] = lambda0;
        so[9] = good ? (double)kGfRun : 3.0;
      }
    }
  } else if ((int)si[9] != kGfRun) {
    // a finished map: nothing but the carry (the status is workgroup-uniform)
    if (store && tid == 0) {
      for (int i = 0; i < kGfS; ++i) so[i] = si[i];
      if (it == n_iter) gf_outputs(so, m, theta, chi2, cov, o_npix, o_niter, o_status);
    }
    return;
  } else {
    double v[kGfQ];
#pragma unroll
    for (int q = 0; q < kGfQ; ++q) v[q] = 0.0;
    const double* __restrict__ pm = p_in + (int64_t)m * kGfQ * tiles;
    for (int i = tid; i < tiles; i += kGfB) {
#pragma unroll
      for (int q = 0; q < kGfQ; ++q) v[q] += pm[(int64_t)q * tiles + i];
    }
    gf_block_sum(v, s_a, s_b, s_tot);
    if (tid == 0) {
      double* row = trace ? trace + ((int64_t)m * n_iter + (it - 1)) * 9 : nullptr;
      const bool eval = gf_decide(si, s_tot, so, store, it, n_iter, xtol, row, s_dec);
      s_dec[6] = eval ? 1.0 : 0.0;
      if (store && it == n_iter) gf_outputs(so, m, theta, chi2, cov, o_npix, o_niter, o_status);
    }
  }
  __syncthreads();
  if (s_dec[6] == 0.0) return;                       // (workgroup-uniform)
  const double S = s_dec[0], x0 = s_dec[1], z0 = s_dec[2];
  const double A = s_dec[3], B2 = 2.0 * s_dec[4], C = s_dec[5];
  const double* __restrict__ im = img + (int64_t)m * npix;
  double v[kGfQ];
#pragma unroll
  for (int q = 0; q < kGfQ; ++q) v[q] = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // (32-bit: an index of the box, a tile's tail beyond it included, is below 2^31 + 1024)
    const unsigned b = (unsigned)tile * (unsigned)kGfT + (unsigned)(tid + kGfB * j);
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
    for (int a = 0; a < 6; ++a) {
#pragma unroll
      for (int c = a; c < 6; ++c) v[1 + gf_tri(a, c)] = __builtin_fma(J[a], J[c], v[1 + gf_tri(a, c)]);
      v[22 + a] = __builtin_fma(J[a], r, v[22 + a]);
    }
    v[28] += 1.0;
  }
  gf_block_sum(v, s_a, s_b, s_tot);
  if (tid < kGfQ) p_out[((int64_t)m * kGfQ + tid) * tiles + tile] = s_tot[tid];
}

hipError_t gaussfit_launch(const double* img, int n_maps, int nx, int nz, const int32_t* box,
                           const uint8_t* mask, double* theta, double lambda0, double xtol,
                           int n_iter, double* chi2, double* cov, int32_t* npix, int32_t* niter,
                           int32_t* status, double* trace, void* work, hipStream_t st) {
  const int bw = box[3] - box[2] + 1;
  const int64_t nbox = (int64_t)(box[1] - box[0] + 1) * bw;
  const GaussfitTiling t = gaussfit_tiling(n_maps, nbox);
  const int tiles = (int)t.tiles;
  const unsigned nb = (unsigned)t.workgroups;
  // workspace: sums [2][n_maps][29][tiles], then state [2][n_maps][48]
  const int64_t ph = t.workgroups * kGfQ, sh = (int64_t)n_maps * kGfS;
  double* pv = (double*)work;
  double* sv = pv + 2 * ph;
  hipError_t err = hipSuccess;
  for (int it = 0; it <= n_iter && err == hipSuccess; ++it) {
    const int in = (it + 1) & 1, out = it & 1;
    hipLaunchKernelGGL(gaussfit_step_kernel, dim3(nb), dim3(kGfB), 0, st, img, (int64_t)nx * nz, nz,
                       box[0], box[2], bw, nbox, tiles, mask, lambda0, xtol, it, n_iter,
                       pv + in * ph, pv + out * ph, sv + in * sh, sv + out * sh, theta, chi2, cov,
                       npix, niter, status, trace);
    err = hipGetLastError();
  }
  return err;
}

}  // namespace rjp
