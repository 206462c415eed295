// What the Levenberg-Marquardt fits share (imfit.hip: K14; uvfit.hip: K20; specfit.hip: K21): the
// packed triangle, the damped Cholesky solve with its breakdown loop, taking over a trial's sums,
// the step test -- and, for the two tiled fits K14 and K20, the block sum, the state of a map, the
// decision of an iteration and the host's loop of launches.
//
// The decision, in this order (trial theta_t with sums chi_t, N_t, g_t):
//   accept iff theta_t is FEASIBLE, chi_t is finite and chi_t < chi_cur (+inf before the first
//   trial).  accept: (theta, chi, N, g)_cur <- trial, lambda <- max(lambda / 10, 1e-12) (the
//   start's own acceptance leaves lambda0); reject: lambda <- 10 lambda.  A fixed parameter (bit i
//   of `free_bits` clear) has its row and column of N replaced by the identity's and g_i by 0 when
//   a trial's sums are taken over: delta_i = 0 exactly.
//   chi_cur == 0 -> status 1.  Else solve (N + lambda diag N) delta = g by a P x P Cholesky; a
//   breakdown (a pivot not > 0) counts as a reject: lambda <- 10 lambda and again; lambda > 1e12 ->
//   status 2.  max_i |delta_i| / s_i <= xtol with the step SCALES s -> status 1 (tested on every
//   proposed step).  Launch n_iter -> status 0.  Else theta_t = theta_cur + delta.
//   First trial: NOT ENOUGH counting items or a chi^2 that is not finite -> status 3, as a start
//   that is not finite and feasible in launch 0.
// A kernel supplies the three points in capitals, K14 and K20 as a Policy -- a struct of
//   static constexpr int P                              the number of parameters
//   static bool feasible(const double* theta)
//   static void scales(const double* theta, double (&s)[P])
//   static bool enough(double count, unsigned free_bits)
// -- and K21, whose state lives in a lane's registers, in its own loop around lm_tri, lm_solve and
// lm_step_converged below.  specfit.hip carries lm_take_sums and lm_damped_solve WRITTEN OUT (the
// calls cost it registers, see there): a change to either is made in both files.
//
// The tiled fits: one launch per iteration for the whole stack, grid = tiles x maps; a tile is
// kLmT = 1024 consecutive items (pixels of the box, visibilities), thread tid owns the items
// t0 + tid + 256 j, j < 4.  Launch k = 0 .. n_iter; a workgroup of launch k >= 1
//   1. reduces the Q = 1 + T + P + 1 partial sums (chi^2, N, g, count) that launch k - 1 left per
//      tile of its map for the trial theta_t -- every workgroup redundantly and in the same order,
//      thread i the tiles i, i + 256, ..., then the block sum;
//   2. thread 0 decides the iteration (lm_decide; L in registers, theta, N, g where the kernel
//      keeps its LmCur, everything at compile-time indices: no scratch) and broadcasts the next
//      trial through LDS;
//   3. every thread evaluates that trial on its items (the kernel's own part); the block sum goes
//      to the other half of the double-buffered partials (lm_store_partials);
//   4. (tile 0 only) writes the map's state to the other half of the double-buffered state, the
//      trace row, and in launch n_iter the outputs.
// Launch 0 only takes the start from d_theta as the first trial.  Workgroups of one launch exchange
// nothing; the kernel boundary makes launch k's writes visible to launch k + 1, as in K12.  A
// finished map's workgroups skip 1-3; tile 0 carries the state over.  No atomics; every sum in a
// fixed order: the same bits on every call.
//
// The block sum goes through LDS, not through Q x 6 cross-lane steps, in passes of 29 sums: each
// thread stores its values in rows of 8 x 33 doubles (the pad keeps the eight 32-term partial sums
// of a row on different banks), 232 threads add 32 consecutive entries each, 29 threads add the 8
// partial sums.
#pragma once
#include "rjp_host.h"

namespace rjp {

constexpr int kLmB = 256;          // threads per workgroup
constexpr int kLmT = 1024;         // items per tile: four per thread
constexpr int kLmC = 29;           // sums per pass of the block sum
constexpr int kLmRow = 8 * 33;     // LDS row of the block sum: 8 parts of 32 + 1 pad
constexpr int kLmRun = -1;         // status while the fit goes on

// index of (i, j), i <= j, in the packed upper triangle of a P x P matrix, row by row
template <int P>
__device__ __forceinline__ constexpr int lm_tri(int i, int j) {
  return i * P - i * (i - 1) / 2 + (j - i);
}

// (N + lam diag N) delta = g by Cholesky; N, g register arrays or LDS pointers, L in registers,
// everything at compile-time indices; false: a pivot is not > 0
template <int P, class TN, class TG>
__device__ __forceinline__ bool lm_solve(const TN& N, const TG& g, double lam, double (&delta)[P]) {
  double L[P * (P + 1) / 2];                         // L^T, packed like N: L[tri(k, i)] = l_ik
  bool ok = true;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const double njj = N[lm_tri<P>(j, j)];
    double d = __builtin_fma(lam, njj, njj);
#pragma unroll
    for (int k = 0; k < j; ++k) d = __builtin_fma(-L[lm_tri<P>(k, j)], L[lm_tri<P>(k, j)], d);
    ok = ok && d > 0.0;
    const double l = __builtin_sqrt(d);
    L[lm_tri<P>(j, j)] = l;
#pragma unroll
    for (int i = j + 1; i < P; ++i) {
      double s = N[lm_tri<P>(j, i)];
#pragma unroll
      for (int k = 0; k < j; ++k) s = __builtin_fma(-L[lm_tri<P>(k, i)], L[lm_tri<P>(k, j)], s);
      L[lm_tri<P>(j, i)] = s / l;
    }
  }
  double y[P];
#pragma unroll
  for (int i = 0; i < P; ++i) {
    double s = g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = __builtin_fma(-L[lm_tri<P>(k, i)], y[k], s);
    y[i] = s / L[lm_tri<P>(i, i)];
  }
#pragma unroll
  for (int i = P - 1; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < P; ++k) s = __builtin_fma(-L[lm_tri<P>(i, k)], delta[k], s);
    delta[i] = s / L[lm_tri<P>(i, i)];
  }
  return ok;
}

// the breakdown loop: lam grows tenfold per failed pivot (at most 25 rounds from 1e-12); false:
// lam > 1e12, status 2
template <int P, class TN, class TG>
__device__ __forceinline__ bool lm_damped_solve(const TN& N, const TG& g, double& lam,
                                                double (&delta)[P]) {
  for (;; lam *= 10.0) {
    if (lam > 1e12) return false;
    if (lm_solve<P>(N, g, lam, delta)) return true;
  }
}

// (N, g) <- an accepted trial's sums, the identity's rows and g_i = 0 for a fixed parameter
template <int P, class SN, class SG, class TN, class TG>
__device__ __forceinline__ void lm_take_sums(unsigned free_bits, const SN& tot_N, const SG& tot_g,
                                             TN& N, TG& g) {
#pragma unroll
  for (int i = 0; i < P; ++i) {
    const bool fi = (free_bits >> i) & 1u;
#pragma unroll
    for (int j = i; j < P; ++j)
      N[lm_tri<P>(i, j)] =
          (fi && ((free_bits >> j) & 1u)) ? tot_N[lm_tri<P>(i, j)] : (i == j ? 1.0 : 0.0);
    g[i] = fi ? tot_g[i] : 0.0;
  }
}

// no NaN in the step and max_i |delta_i| / scale_i <= xtol.  (The maximum starts from 0: fmax is
// exact and drops a NaN, which the NaN test catches anyway, so neither the order of the terms nor
// a scale of exactly 1 -- |d| / 1.0 is |d| -- changes the value or the branch.)
template <int P>
__device__ __forceinline__ bool lm_step_converged(const double (&delta)[P], const double (&scale)[P],
                                                  double xtol) {
  double worst = 0.0;
  bool nan = false;
#pragma unroll
  for (int i = 0; i < P; ++i) worst = __builtin_fmax(worst, __builtin_fabs(delta[i]) / scale[i]);
#pragma unroll
  for (int i = 0; i < P; ++i) nan = nan || delta[i] != delta[i];
  return !nan && worst <= xtol;
}

// ---- the tiled fits (K14, K20) -------------------------------------------------------------------
// sizes and the layout of a map's state for P parameters:
// theta_cur 0..P-1, chi_cur, lambda, lambda of the trial, status, trials, count, theta_t, N, g
template <int P_>
struct LmState {
  static constexpr int P = P_, T = P * (P + 1) / 2, Q = 1 + T + P + 1;
  static constexpr int oChi = P, oLam = P + 1, oLamT = P + 2, oStat = P + 3, oIt = P + 4,
                       oCnt = P + 5, oTt = P + 6, oN = 2 * P + 6, oG = 2 * P + 6 + T;
  static constexpr int S = (oG + P + 7) / 8 * 8;    // doubles of state per map: 48, 120
};

// the LDS of a workgroup: the block sum's rows and partial sums, the totals, and the broadcast
// trial (dec[P]: evaluate it or not)
template <int P>
struct LmLds {
  double a[kLmC * kLmRow], b[kLmC * 8], tot[LmState<P>::Q], dec[P + 1];
};

// theta_cur, N and g of the map while thread 0 decides.  The kernel says where they live: a local
// (thread 0's registers: K14) or __shared__ (K20, whose 102 doubles at two components beside the
// 78 of L would not fit).
template <int P>
struct LmCur {
  double th[P], N[LmState<P>::T], g[P];
};

// What launch `it` of n_iter + 1 gets besides its halves of the workspace, which stay kernel
// arguments of their own for their __restrict__: partials p_in -> p_out ([n_maps][Q][tiles]), state
// s_in -> s_out ([n_maps][S]).
struct LmLaunch {
  int tiles, it, n_iter;
  double lambda0, xtol;
  double *theta, *chi2, *cov;
  int *count, *niter, *status;
  double* trace;
};

// l.tot[q] = sum over the workgroup of v[q], valid in every thread on return
template <int Q, int P>
__device__ __forceinline__ void lm_block_sum(const double (&v)[Q], LmLds<P>& l) {
  const int tid = threadIdx.x;
  const int slot = (tid >> 5) * 33 + (tid & 31);
#pragma unroll
  for (int c0 = 0; c0 < Q; c0 += kLmC) {
    const int n = Q - c0 < kLmC ? Q - c0 : kLmC;
    __syncthreads();                                // earlier readers of l.a / l.tot are done
#pragma unroll
    for (int q = 0; q < kLmC; ++q)
      if (c0 + q < Q) l.a[q * kLmRow + slot] = v[c0 + q < Q ? c0 + q : 0];
    __syncthreads();
    if (tid < n * 8) {
      const double* p = l.a + (tid >> 3) * kLmRow + (tid & 7) * 33;
      double a = p[0];
      for (int i = 1; i < 32; ++i) a += p[i];
      l.b[tid] = a;
    }
    __syncthreads();
    if (tid < n) {
      double a = l.b[tid * 8];
#pragma unroll
      for (int i = 1; i < 8; ++i) a += l.b[tid * 8 + i];
      l.tot[c0 + tid] = a;
    }
  }
  __syncthreads();
}

// the outputs of map m from its final state (status 3: the status alone)
template <int P>
__device__ __forceinline__ void lm_outputs(const double* __restrict__ s, int m, const LmLaunch& a) {
  using U = LmState<P>;
  const int st = (int)s[U::oStat];
  a.status[m] = st == kLmRun ? 0 : st;
  if (st == 3) return;
  for (int i = 0; i < P; ++i) a.theta[P * m + i] = s[i];
  a.chi2[m] = s[U::oChi];
  for (int i = 0; i < U::T; ++i) a.cov[(int64_t)U::T * m + i] = s[U::oN + i];
  a.count[m] = (int)s[U::oCnt];
  a.niter[m] = (int)s[U::oIt];
}

// Step 2 of launch a.it >= 1 in thread 0: the state `si` and the trial's sums l.tot -> the state
// `so` (tile 0 stores it), the trace row, and the next trial in l.dec[0..P-1]; true: evaluate it.
template <class Pol>
__device__ __forceinline__ bool lm_decide(const double* __restrict__ si, double* __restrict__ so,
                                          bool store, const LmLaunch& a, unsigned free_bits,
                                          double* __restrict__ trace_row, LmLds<Pol::P>& l,
                                          LmCur<Pol::P>& c) {
  using U = LmState<Pol::P>;
  constexpr int P = U::P, T = U::T;
  const bool first = a.it == 1;
  const double chi_t = l.tot[0], lam_used = si[U::oLamT];
  double lam = si[U::oLam], chi_cur = si[U::oChi];
  const double cnt = first ? l.tot[U::Q - 1] : si[U::oCnt];
  int status = kLmRun;
  bool eval = false;
  if (first && (!Pol::enough(cnt, free_bits) || !finite_d(chi_t))) {
    if (store) {
      for (int i = 0; i < U::S; ++i) so[i] = si[i];
      so[U::oStat] = 3.0;
    }
    return false;
  }
  const bool acc = Pol::feasible(si + U::oTt) && finite_d(chi_t) && chi_t < chi_cur;
  if (acc) {
#pragma unroll
    for (int i = 0; i < P; ++i) c.th[i] = si[U::oTt + i];
    lm_take_sums<P>(free_bits, l.tot + 1, l.tot + 1 + T, c.N, c.g);
    chi_cur = chi_t;
    if (!first) lam = __builtin_fmax(lam / 10.0, 1e-12);
  } else {
#pragma unroll
    for (int i = 0; i < P; ++i) c.th[i] = si[i];
#pragma unroll
    for (int i = 0; i < T; ++i) c.N[i] = si[U::oN + i];
#pragma unroll
    for (int i = 0; i < P; ++i) c.g[i] = si[U::oG + i];
    lam *= 10.0;
  }
  if (store && trace_row) {
    trace_row[0] = chi_t;
    trace_row[1] = lam_used;
    trace_row[2] = acc ? 1.0 : 0.0;
    for (int i = 0; i < P; ++i) trace_row[3 + i] = si[U::oTt + i];
  }
  // (the next trial stays in registers to the end: parked in l.dec and read back for the state it
  // cost K14 4 % at 4096 workgroups)
  double tn[P];
#pragma unroll
  for (int i = 0; i < P; ++i) tn[i] = si[U::oTt + i];
  if (chi_cur == 0.0) {
    status = 1;
  } else {
    double delta[P], scale[P];
    if (!lm_damped_solve<P>(c.N, c.g, lam, delta)) {
      status = 2;
    } else {
      Pol::scales(c.th, scale);
      if (lm_step_converged<P>(delta, scale, a.xtol)) {
        status = 1;
      } else if (a.it == a.n_iter) {
        status = 0;
      } else {
#pragma unroll
        for (int i = 0; i < P; ++i) tn[i] = c.th[i] + delta[i];
        eval = true;
      }
    }
  }
  if (store) {
#pragma unroll
    for (int i = 0; i < P; ++i) so[i] = c.th[i];
    so[U::oChi] = chi_cur;
    so[U::oLam] = lam;
    so[U::oLamT] = eval ? lam : lam_used;
    so[U::oStat] = (double)status;
    so[U::oIt] = (double)a.it;
    so[U::oCnt] = cnt;
#pragma unroll
    for (int i = 0; i < P; ++i) so[U::oTt + i] = tn[i];
#pragma unroll
    for (int i = 0; i < T; ++i) so[U::oN + i] = c.N[i];
#pragma unroll
    for (int i = 0; i < P; ++i) so[U::oG + i] = c.g[i];
    for (int i = U::oG + P; i < U::S; ++i) so[i] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < P; ++i) l.dec[i] = tn[i];
  return eval;
}

// Steps 1, 2 and 4 of a launch for the workgroup of (tile, map m); true, in every thread: evaluate
// the trial l.dec[0..P-1] and hand the sums to lm_store_partials.
template <class Pol>
__device__ __forceinline__ bool lm_begin(const LmLaunch& a, const double* __restrict__ p_in,
                                         const double* __restrict__ s_in,
                                         double* __restrict__ s_out, int tile, int m,
                                         unsigned free_bits, LmLds<Pol::P>& l, LmCur<Pol::P>& c) {
  using U = LmState<Pol::P>;
  constexpr int P = U::P, Q = U::Q;
  const int tid = threadIdx.x;
  const double* __restrict__ si = s_in + (int64_t)m * U::S;
  double* __restrict__ so = s_out + (int64_t)m * U::S;
  const bool store = tile == 0;
  if (a.it == 0) {
    if (tid == 0) {
      bool good = true;
      for (int i = 0; i < P; ++i) {
        const double t = a.theta[P * m + i];
        good = good && finite_d(t);
        l.dec[i] = t;
      }
      good = good && Pol::feasible(l.dec);
      l.dec[P] = good ? 1.0 : 0.0;
      if (store) {
        for (int i = 0; i < U::S; ++i) so[i] = 0.0;
        for (int i = 0; i < P; ++i) so[i] = so[U::oTt + i] = l.dec[i];
        so[U::oChi] = __builtin_inf();
        so[U::oLam] = so[U::oLamT] = a.lambda0;
        so[U::oStat] = good ? (double)kLmRun : 3.0;
      }
    }
  } else if ((int)si[U::oStat] != kLmRun) {
    // a finished map: nothing but the carry (the status is workgroup-uniform)
    if (store && tid == 0) {
      for (int i = 0; i < U::S; ++i) so[i] = si[i];
      if (a.it == a.n_iter) lm_outputs<P>(so, m, a);
    }
    return false;
  } else {
    double acc[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) acc[q] = 0.0;
    const double* __restrict__ pm = p_in + (int64_t)m * Q * a.tiles;
    for (int i = tid; i < a.tiles; i += kLmB) {
#pragma unroll
      for (int q = 0; q < Q; ++q) acc[q] += pm[(int64_t)q * a.tiles + i];
    }
    lm_block_sum<Q>(acc, l);
    if (tid == 0) {
      double* row = a.trace ? a.trace + ((int64_t)m * a.n_iter + (a.it - 1)) * (3 + P) : nullptr;
      l.dec[P] = lm_decide<Pol>(si, so, store, a, free_bits, row, l, c) ? 1.0 : 0.0;
      if (store && a.it == a.n_iter) lm_outputs<P>(so, m, a);
    }
  }
  __syncthreads();
  return l.dec[P] != 0.0;                             // (workgroup-uniform)
}

// step 3's end: the block sum of the trial's sums to the tile's place in the partials
template <int Q, int P>
__device__ __forceinline__ void lm_store_partials(const double (&v)[Q], double* __restrict__ p_out,
                                                  int tiles, int tile, int m, LmLds<P>& l) {
  lm_block_sum<Q>(v, l);
  for (int q = threadIdx.x; q < Q; q += kLmB) p_out[((int64_t)m * Q + q) * tiles + tile] = l.tot[q];
}

// ---- the host half -------------------------------------------------------------------------------
inline LmTiling lm_tiling(int n_maps, int64_t items) {
  LmTiling t;
  t.tiles = (items + kLmT - 1) / kLmT;
  t.workgroups = t.tiles * n_maps;
  return t;
}

// two halves of (Q sums per tile, S doubles of state per map); 0: no size_t holds it
inline size_t lm_workspace_bytes(const LmTiling& t, int n_maps, int Q, int S) {
  const unsigned __int128 n =
      ((unsigned __int128)t.workgroups * (unsigned)Q + (unsigned __int128)n_maps * (unsigned)S) * 2u * 8u;
  return n > (unsigned __int128)SIZE_MAX ? 0 : (size_t)n;
}

// The n_iter + 1 launches over the workspace: sums [2][n_maps][Q][tiles], then state [2][n_maps][S];
// launch(a, p_in, p_out, s_in, s_out) starts launch a.it with its halves.  No host synchronisation.
template <class F>
hipError_t lm_launch_loop(const LmTiling& t, int n_maps, int Q, int S, double lambda0, double xtol,
                          int n_iter, double* theta, double* chi2, double* cov, int32_t* count,
                          int32_t* niter, int32_t* status, double* trace, void* work, F launch) {
  LmLaunch a{(int)t.tiles, 0, n_iter, lambda0, xtol, theta, chi2, cov, count, niter, status, trace};
  const int64_t ph = t.workgroups * Q, sh = (int64_t)n_maps * S;
  double* pv = (double*)work;
  double* sv = pv + 2 * ph;
  hipError_t err = hipSuccess;
  for (a.it = 0; a.it <= a.n_iter && err == hipSuccess; ++a.it) {
    const int in = (a.it + 1) & 1, out = a.it & 1;
    launch(a, pv + in * ph, pv + out * ph, sv + in * sh, sv + out * sh);
    err = hipGetLastError();
  }
  return err;
}

}  // namespace rjp
