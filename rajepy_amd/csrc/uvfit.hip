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
// Structure: K14's (imfit.hip).  One launch per iteration for the whole stack, grid = tiles x maps;
// a tile is kUfT = 1024 consecutive visibilities, thread tid owns t0 + tid + 256 j, j < 4.  Launch
// k = 0 .. n_iter; a workgroup of launch k >= 1
//   1. reduces the Q = 1 + T + P + 1 partial sums (chi^2, N, g, count) that launch k - 1 left per
//      tile of its map -- every workgroup redundantly and in the same order, thread i the tiles
//      i, i + 256, ..., then the block sum;
//   2. thread 0 decides the iteration (uf_decide) and broadcasts the next trial through LDS;
//   3. every thread evaluates that trial on its visibilities; the block sum goes to the other half
//      of the double-buffered partials;
//   4. (tile 0 only) writes the map's state to the other half of the double-buffered state, the
//      trace row, and in launch n_iter the outputs.
// No atomics; every sum in a fixed order: the same bits on every call.  The block sum goes through
// LDS in chunks of 29 sums (K14's rows of 8 x 33 doubles), four chunks for two components.  The
// partial sums of a thread live in registers (92 doubles for two components); thread 0 factorises
// with L in registers and N, g in LDS, everything at compile-time indices: no scratch.
//
// The decision is K14's, word for word, with: "positive definite" -> every component's Sigma is
// positive SEMI-definite (sxx >= 0, szz >= 0, sxx szz >= sxz^2); the step scale s = (max(|F|,
// 1e-300), 1, 1, t, t, t), t = max(sxx + szz, 1) per component; status 3 for a start that is not
// finite or not PSD, a first chi^2 that is not finite, or 2 count < the number of free parameters;
// a P x P Cholesky.  A fixed parameter (bit i of `free_bits` clear) has its row and column of N
// replaced by the identity's and g_i by 0 when a trial's sums are taken over: delta_i = 0 exactly.
#include "rjp_host.h"

namespace rjp {

constexpr int kUfB = 256;          // threads per workgroup
constexpr int kUfT = 1024;         // visibilities per tile: four per thread
constexpr int kUfC = 29;           // sums per pass of the block sum
constexpr int kUfRow = 8 * 33;     // LDS row of the block sum: 8 parts of 32 + 1 pad
constexpr int kUfRun = -1;         // status while the fit goes on
constexpr double kUfM2Pi2 = -19.739208802178716;   // -2 pi^2
constexpr double kUfM4Pi2 = -39.478417604357432;   // -4 pi^2
constexpr double kUf2Pi = 6.283185307179586;

// sizes and the layout of a map's state for NC components:
// theta_cur 0..P-1, chi_cur, lambda, lambda of the trial, status, trials, count, theta_t, N, g
template <int NC>
struct Uf {
  static constexpr int P = 6 * NC, T = P * (P + 1) / 2, Q = 1 + T + P + 1;
  static constexpr int oChi = P, oLam = P + 1, oLamT = P + 2, oStat = P + 3, oIt = P + 4,
                       oCnt = P + 5, oTt = P + 6, oN = 2 * P + 6, oG = 2 * P + 6 + T;
  static constexpr int S = (oG + P + 7) / 8 * 8;    // doubles of state per map: 48, 120
};

static int uf_sums(int n_comp) { return n_comp == 1 ? Uf<1>::Q : Uf<2>::Q; }
static int uf_state(int n_comp) { return n_comp == 1 ? Uf<1>::S : Uf<2>::S; }

UvfitTiling uvfit_tiling(int n_maps, int64_t n_vis) {
  UvfitTiling t;
  t.tiles = (n_vis + kUfT - 1) / kUfT;
  t.workgroups = t.tiles * n_maps;
  return t;
}

// two halves of (Q sums per tile, S doubles of state per map); 0: no size_t holds it
size_t uvfit_workspace_bytes(int n_maps, int64_t n_vis, int n_comp) {
  const UvfitTiling t = uvfit_tiling(n_maps, n_vis);
  const unsigned __int128 n = ((unsigned __int128)t.workgroups * (unsigned)uf_sums(n_comp) +
                               (unsigned __int128)n_maps * (unsigned)uf_state(n_comp)) * 2u * 8u;
  return n > (unsigned __int128)SIZE_MAX ? 0 : (size_t)n;
}

__device__ __forceinline__ bool uf_psd(double sxx, double sxz, double szz) {
  return sxx >= 0.0 && szz >= 0.0 && sxx * szz >= sxz * sxz;
}

// index of (i, j), i <= j, in the packed upper triangle of a P x P matrix, row by row
template <int P>
__device__ __forceinline__ constexpr int uf_tri(int i, int j) {
  return i * P - i * (i - 1) / 2 + (j - i);
}

// s_tot[q] = sum over the workgroup of v[q], valid in every thread on return
template <int Q>
__device__ __forceinline__ void uf_block_sum(const double (&v)[Q], double* s_a, double* s_b,
                                             double* s_tot) {
  const int tid = threadIdx.x;
  const int slot = (tid >> 5) * 33 + (tid & 31);
#pragma unroll
  for (int c0 = 0; c0 < Q; c0 += kUfC) {
    const int n = Q - c0 < kUfC ? Q - c0 : kUfC;
    __syncthreads();                                // earlier readers of s_a / s_tot are done
#pragma unroll
    for (int q = 0; q < kUfC; ++q)
      if (c0 + q < Q) s_a[q * kUfRow + slot] = v[c0 + q < Q ? c0 + q : 0];
    __syncthreads();
    if (tid < n * 8) {
      const double* p = s_a + (tid >> 3) * kUfRow + (tid & 7) * 33;
      double a = p[0];
      for (int i = 1; i < 32; ++i) a += p[i];
      s_b[tid] = a;
    }
    __syncthreads();
    if (tid < n) {
      double a = s_b[tid * 8];
#pragma unroll
      for (int i = 1; i < 8; ++i) a += s_b[tid * 8 + i];
      s_tot[c0 + tid] = a;
    }
  }
  __syncthreads();
}

// (N + lam diag N) delta = g by Cholesky; N, g in LDS, L in registers, everything at compile-time
// indices; false: a pivot is not > 0
template <int P>
__device__ __forceinline__ bool uf_solve(const double* N, const double* g, double lam,
                                         double (&delta)[P]) {
  double L[P * (P + 1) / 2];                         // L^T, packed like N: L[tri(k, i)] = l_ik
  bool ok = true;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const double njj = N[uf_tri<P>(j, j)];
    double d = __builtin_fma(lam, njj, njj);
#pragma unroll
    for (int k = 0; k < j; ++k) d = __builtin_fma(-L[uf_tri<P>(k, j)], L[uf_tri<P>(k, j)], d);
    ok = ok && d > 0.0;
    const double l = __builtin_sqrt(d);
    L[uf_tri<P>(j, j)] = l;
#pragma unroll
    for (int i = j + 1; i < P; ++i) {
      double s = N[uf_tri<P>(j, i)];
#pragma unroll
      for (int k = 0; k < j; ++k) s = __builtin_fma(-L[uf_tri<P>(k, i)], L[uf_tri<P>(k, j)], s);
      L[uf_tri<P>(j, i)] = s / l;
    }
  }
  double y[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    double s = g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = __builtin_fma(-L[uf_tri<P>(k, i)], y[k], s);
    y[i] = s / L[uf_tri<P>(i, i)];
  }
#pragma unroll
  for (int i = P - 1; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < P; ++k) s = __builtin_fma(-L[uf_tri<P>(i, k)], delta[k], s);
    delta[i] = s / L[uf_tri<P>(i, i)];
  }
  return ok;
}

// the outputs of a map from its final state (status 3: the status alone)
template <int NC>
__device__ __forceinline__ void uf_outputs(const double* __restrict__ s, int m,
                                           double* __restrict__ theta, double* __restrict__ chi2,
                                           double* __restrict__ cov, int* __restrict__ nvis,
                                           int* __restrict__ niter, int* __restrict__ status) {
  using U = Uf<NC>;
  const int st = (int)s[U::oStat];
  status[m] = st == kUfRun ? 0 : st;
  if (st == 3) return;
  for (int i = 0; i < U::P; ++i) theta[U::P * m + i] = s[i];
  chi2[m] = s[U::oChi];
  for (int i = 0; i < U::T; ++i) cov[(int64_t)U::T * m + i] = s[U::oN + i];
  nvis[m] = (int)s[U::oCnt];
  niter[m] = (int)s[U::oIt];
}

// Step 2 of launch `it` >= 1 in thread 0: the state `si` and the trial's sums `tot` -> the state
// `so` (tile 0 stores it), the trace row, and the next trial in dec[0..P-1]; true: evaluate it.
// s_th [P], s_N [T], s_g [P]: LDS of thread 0's own.
template <int NC>
__device__ __forceinline__ bool uf_decide(const double* __restrict__ si, const double* tot,
                                          double* __restrict__ so, bool store, int it, int n_iter,
                                          double xtol, unsigned free_bits,
                                          double* __restrict__ trace_row, double* dec, double* s_th,
                                          double* s_N, double* s_g) {
  using U = Uf<NC>;
  constexpr int P = U::P, T = U::T;
  const bool first = it == 1;
  const double chi_t = tot[0], lam_used = si[U::oLamT];
  double lam = si[U::oLam], chi_cur = si[U::oChi];
  const double cnt = first ? tot[U::Q - 1] : si[U::oCnt];
  int status = kUfRun;
  bool eval = false;
  if (first && (!(2.0 * cnt >= (double)__builtin_popcount(free_bits)) || !finite_d(chi_t))) {
    if (store) {
      for (int i = 0; i < U::S; ++i) so[i] = si[i];
      so[U::oStat] = 3.0;
    }
    return false;
  }
  bool psd = true;
  for (int c = 0; c < NC; ++c)
    psd = psd && uf_psd(si[U::oTt + 6 * c + 3], si[U::oTt + 6 * c + 4], si[U::oTt + 6 * c + 5]);
  const bool acc = psd && finite_d(chi_t) && chi_t < chi_cur;
  if (acc) {
    for (int i = 0; i < P; ++i) s_th[i] = si[U::oTt + i];
    int q = 0;
    for (int i = 0; i < P; ++i) {
      const bool fi = (free_bits >> i) & 1u;
      for (int j = i; j < P; ++j, ++q)
        s_N[q] = (fi && ((free_bits >> j) & 1u)) ? tot[1 + q] : (i == j ? 1.0 : 0.0);
      s_g[i] = fi ? tot[1 + T + i] : 0.0;
    }
    chi_cur = chi_t;
    if (!first) lam = __builtin_fmax(lam / 10.0, 1e-12);
  } else {
    for (int i = 0; i < P; ++i) s_th[i] = si[i];
    for (int i = 0; i < T; ++i) s_N[i] = si[U::oN + i];
    for (int i = 0; i < P; ++i) s_g[i] = si[U::oG + i];
    lam *= 10.0;
  }
  if (store && trace_row) {
    trace_row[0] = chi_t;
    trace_row[1] = lam_used;
    trace_row[2] = acc ? 1.0 : 0.0;
    for (int i = 0; i < P; ++i) trace_row[3 + i] = si[U::oTt + i];
  }
  for (int i = 0; i < P; ++i) dec[i] = si[U::oTt + i];
  if (chi_cur == 0.0) {
    status = 1;
  } else {
    double delta[P];
    bool ok = false;
    // (at most 25 rounds: lambda >= 1e-12 grows tenfold per breakdown)
    while (true) {
      if (lam > 1e12) {
        status = 2;
        break;
      }
      if (uf_solve<P>(s_N, s_g, lam, delta)) {
        ok = true;
        break;
      }
      lam *= 10.0;
    }
    if (ok) {
      double worst = 0.0;
      bool nan = false;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const double t = __builtin_fmax(s_th[6 * c + 3] + s_th[6 * c + 5], 1.0);
        // (|F| = 0 would make 0 / 0, which fmax drops: the floor keeps F in the test)
        worst = __builtin_fmax(worst, __builtin_fabs(delta[6 * c]) /
                                          __builtin_fmax(__builtin_fabs(s_th[6 * c]), 1e-300));
        worst = __builtin_fmax(worst, __builtin_fmax(__builtin_fabs(delta[6 * c + 1]),
                                                     __builtin_fabs(delta[6 * c + 2])));
#pragma unroll
        for (int i = 3; i < 6; ++i)
          worst = __builtin_fmax(worst, __builtin_fabs(delta[6 * c + i]) / t);
      }
#pragma unroll
      for (int i = 0; i < P; ++i) nan = nan || delta[i] != delta[i];
      if (!nan && worst <= xtol) {
        status = 1;
      } else if (it == n_iter) {
        status = 0;
      } else {
#pragma unroll
        for (int i = 0; i < P; ++i) dec[i] = s_th[i] + delta[i];
        eval = true;
      }
    }
  }
  if (store) {
    for (int i = 0; i < P; ++i) so[i] = s_th[i];
    so[U::oChi] = chi_cur;
    so[U::oLam] = lam;
    so[U::oLamT] = eval ? lam : lam_used;
    so[U::oStat] = (double)status;
    so[U::oIt] = (double)it;
    so[U::oCnt] = cnt;
    for (int i = 0; i < P; ++i) so[U::oTt + i] = dec[i];
    for (int i = 0; i < T; ++i) so[U::oN + i] = s_N[i];
    for (int i = 0; i < P; ++i) so[U::oG + i] = s_g[i];
    for (int i = U::oG + P; i < U::S; ++i) so[i] = 0.0;
  }
  return eval;
}

// launch `it` of n_iter + 1: partials p_in -> p_out ([n_maps][Q][tiles]), state s_in -> s_out
template <int NC>
__global__ __launch_bounds__(kUfB) void uvfit_step_kernel(
    const double* __restrict__ vis, const double* __restrict__ u, const double* __restrict__ v,
    const double* __restrict__ w, int64_t w_stride, const double* __restrict__ su,
    const double* __restrict__ sv, int n_vis, int tiles, unsigned free_bits, double lambda0,
    double xtol, int it, int n_iter, const double* __restrict__ p_in, double* __restrict__ p_out,
    const double* __restrict__ s_in, double* __restrict__ s_out, double* __restrict__ theta,
    double* __restrict__ chi2, double* __restrict__ cov, int* __restrict__ o_nvis,
    int* __restrict__ o_niter, int* __restrict__ o_status, double* __restrict__ trace) {
  using U = Uf<NC>;
  constexpr int P = U::P, T = U::T, Q = U::Q;
  __shared__ double s_a[kUfC * kUfRow];
  __shared__ double s_b[kUfC * 8];
  __shared__ double s_tot[Q];
  __shared__ double s_dec[P + 1];
  __shared__ double s_th[P];
  __shared__ double s_N[T];
  __shared__ double s_g[P];
  const int tid = threadIdx.x;
  const int tile = (int)(blockIdx.x % (unsigned)tiles), m = (int)(blockIdx.x / (unsigned)tiles);
  const double* __restrict__ si = s_in + (int64_t)m * U::S;
  double* __restrict__ so = s_out + (int64_t)m * U::S;
  const bool store = tile == 0;
  if (it == 0) {
    if (tid == 0) {
      bool good = true;
      for (int i = 0; i < P; ++i) {
        const double t = theta[P * m + i];
        good = good && finite_d(t);
        s_dec[i] = t;
      }
      for (int c = 0; c < NC; ++c)
        good = good && uf_psd(s_dec[6 * c + 3], s_dec[6 * c + 4], s_dec[6 * c + 5]);
      s_dec[P] = good ? 1.0 : 0.0;
      if (store) {
        for (int i = 0; i < U::S; ++i) so[i] = 0.0;
        for (int i = 0; i < P; ++i) so[i] = so[U::oTt + i] = s_dec[i];
        so[U::oChi] = __builtin_inf();
        so[U::oLam] = so[U::oLamT] = lambda0;
        so[U::oStat] = good ? (double)kUfRun : 3.0;
      }
    }
  } else if ((int)si[U::oStat] != kUfRun) {
    // a finished map: nothing but the carry (the status is workgroup-uniform)
    if (store && tid == 0) {
      for (int i = 0; i < U::S; ++i) so[i] = si[i];
      if (it == n_iter) uf_outputs<NC>(so, m, theta, chi2, cov, o_nvis, o_niter, o_status);
    }
    return;
  } else {
    double acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0;
    const double* __restrict__ pm = p_in + (int64_t)m * Q * tiles;
    for (int i = tid; i < tiles; i += kUfB) {
#pragma unroll
      for (int q = 0; q < Q; ++q) acc[q] += pm[(int64_t)q * tiles + i];
    }
    uf_block_sum<Q>(acc, s_a, s_b, s_tot);
    if (tid == 0) {
      double* row = trace ? trace + ((int64_t)m * n_iter + (it - 1)) * (3 + P) : nullptr;
      const bool eval = uf_decide<NC>(si, s_tot, so, store, it, n_iter, xtol, free_bits, row, s_dec,
                                      s_th, s_N, s_g);
      s_dec[P] = eval ? 1.0 : 0.0;
      if (store && it == n_iter) uf_outputs<NC>(so, m, theta, chi2, cov, o_nvis, o_niter, o_status);
    }
  }
  __syncthreads();
  if (s_dec[P] == 0.0) return;                       // (workgroup-uniform)
  double th[P];
#pragma unroll
  for (int i = 0; i < P; ++i) th[i] = s_dec[i];
  const double sum = su[m], svm = sv[m];
  const double* __restrict__ vm = vis + (int64_t)m * n_vis * 2;
  const double* __restrict__ wm = w ? w + (int64_t)m * w_stride : nullptr;
  double acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = 0.0;
#pragma unroll 1
  for (int j = 0; j < 4; ++j) {
    // (64-bit: tile * 1024 + 1023 may pass 2^31 for n_vis near it)
    const int64_t k = (int64_t)tile * kUfT + (tid + kUfB * j);
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
        double s = acc[1 + uf_tri<P>(p, c)];
        s = __builtin_fma(wr, Jr[c], s);
        acc[1 + uf_tri<P>(p, c)] = __builtin_fma(wi, Ji[c], s);
      }
      double s = acc[1 + T + p];
      s = __builtin_fma(wr, rr, s);
      acc[1 + T + p] = __builtin_fma(wi, ri, s);
    }
    acc[Q - 1] += 1.0;
  }
  uf_block_sum<Q>(acc, s_a, s_b, s_tot);
  for (int q = tid; q < Q; q += kUfB) p_out[((int64_t)m * Q + q) * tiles + tile] = s_tot[q];
}

template <int NC>
static hipError_t uvfit_launch_n(const double* vis, int n_maps, int n_vis, const double* d_su,
                                 const double* d_sv, const double* u, const double* v,
                                 const double* w, int w_maps, unsigned free_bits, double* theta,
                                 double lambda0, double xtol, int n_iter, double* chi2, double* cov,
                                 int32_t* nvis, int32_t* niter, int32_t* status, double* trace,
                                 void* work, hipStream_t st) {
  using U = Uf<NC>;
  const UvfitTiling t = uvfit_tiling(n_maps, n_vis);
  const int tiles = (int)t.tiles;
  const unsigned nb = (unsigned)t.workgroups;
  // workspace: sums [2][n_maps][Q][tiles], then state [2][n_maps][S]
  const int64_t ph = t.workgroups * U::Q, sh = (int64_t)n_maps * U::S;
  double* pv = (double*)work;
  double* sv = pv + 2 * ph;
  const int64_t w_stride = w && w_maps == n_maps && n_maps > 1 ? n_vis : 0;
  hipError_t err = hipSuccess;
  for (int it = 0; it <= n_iter && err == hipSuccess; ++it) {
    const int in = (it + 1) & 1, out = it & 1;
    hipLaunchKernelGGL(uvfit_step_kernel<NC>, dim3(nb), dim3(kUfB), 0, st, vis, u, v, w, w_stride,
                       d_su, d_sv, n_vis, tiles, free_bits, lambda0, xtol, it, n_iter, pv + in * ph,
                       pv + out * ph, sv + in * sh, sv + out * sh, theta, chi2, cov, nvis, niter,
                       status, trace);
    err = hipGetLastError();
  }
  return err;
}

hipError_t uvfit_launch(const double* vis, int n_maps, int n_vis, const double* d_su,
                        const double* d_sv, const double* u, const double* v, const double* w,
                        int w_maps, int n_comp, unsigned free_bits, double* theta, double lambda0,
                        double xtol, int n_iter, double* chi2, double* cov, int32_t* nvis,
                        int32_t* niter, int32_t* status, double* trace, void* work,
                        hipStream_t st) {
  if (n_comp == 1)
    return uvfit_launch_n<1>(vis, n_maps, n_vis, d_su, d_sv, u, v, w, w_maps, free_bits, theta,
                             lambda0, xtol, n_iter, chi2, cov, nvis, niter, status, trace, work, st);
  return uvfit_launch_n<2>(vis, n_maps, n_vis, d_su, d_sv, u, v, w, w_maps, free_bits, theta,
                           lambda0, xtol, n_iter, chi2, cov, nvis, niter, status, trace, work, st);
}

}  // namespace rjp
