// K22 (rjp_gain_apply, rjp_gaincal): antenna-based complex gains -- what radio astronomers get
// from CASA simobserve's `corrupt`, gaincal and applycal.  CASA is not at hand: the header comment
// (include/rjprt.h) IS the definition, parity is not claimed.
//
// gain_apply_kernel        one thread per visibility (m, t, pq) of a flat index whose 64-bit
//                          divisions are made once per workgroup (gc_split); the pair (p < q)
//                          decoded with one float sqrt and an integer fix-up (exact: at most 2016
//                          pairs), the interval of t from a staged table, two gains (cached: n_sol
//                          n_ant of them), 16 B read and 16 B written per visibility.  No atomics,
//                          no LDS.
// gaincal_accumulate_kernel  kernel 1, the pass over the data: one thread per (m, s, pq), a chain
//                          over the interval's integrations in ascending t.  Consecutive lanes hold
//                          consecutive pq, so an integration's row is read in whole lines: 16 B of
//                          data, 16 B of model, 8 B of weight per visibility (40 B, the model and
//                          the weights shared between maps stay in cache for the later maps).
//                          Writes A (2 planes), B (1 plane) and the count of its pair.
// gaincal_solve_kernel     kernel 2: one workgroup of ONE WAVE per (m, s), ONE LANE PER ANTENNA,
//                          the triangle of A and B (24 B a pair) and the gains in LDS, the whole
//                          iteration in one launch.  Why one lane per antenna: a call holds
//                          thousands of (m, s) problems, so the device is filled by problems, not
//                          by lanes of one problem; sharing an antenna's sum between lanes would
//                          buy a shorter chain at the price of a cross-lane exchange per step and of
//                          an order of summation that depends on the split.  The latency of the
//                          chain is taken from inside the lane instead: the sum over q runs as FOUR
//                          independent chains (q mod 4), combined (c0 + c1) + (c2 + c3), so that
//                          four LDS reads and four fma chains are in flight per lane, and the other
//                          waves of the CU cover the rest.  LDS decides how many: the kernel is
//                          built for 16, 32 and 64 antennas (2.9, 11.9 and 48 KiB of triangle), so
//                          a 27-antenna array runs 13 problems per CU and not the 3 that the cap's
//                          triangle would leave.  A barrier of a one-wave workgroup costs nothing.
// gaincal_residual_kernel  kernel 3: one workgroup per (m, s), lane l takes the pairs pq = l, l +
//                          256, ... and for each the interval's integrations in ascending t as one
//                          running chain, for the start gains and for the solution at once; the
//                          256 partials are folded by halves (128, 64, ... 1).  Reads the data a
//                          second time: chi^2 from A, B and sum w |D|^2 would cancel.
// No atomics anywhere; every sum has one order, a function of n_ant and the interval alone.
#include "rjp_host.h"

namespace rjp {

constexpr int kGcB = 256;          // threads per workgroup of apply, accumulate and residual
constexpr int kGcW = 64;           // solve: one wave, one lane per antenna

static int64_t gc_tri(int n_ant) { return (int64_t)n_ant * (n_ant - 1) / 2; }

int64_t gain_apply_workgroups(int n_maps, int n_t, int n_ant) {
  return ((int64_t)n_maps * n_t * gc_tri(n_ant) + kGcB - 1) / kGcB;
}

static int64_t gc_acc_workgroups(int n_maps, int n_sol, int n_ant) {
  return ((int64_t)n_maps * n_sol * gc_tri(n_ant) + kGcB - 1) / kGcB;
}

int64_t gaincal_workgroups(int n_maps, int n_sol, int n_ant) {
  return gc_acc_workgroups(n_maps, n_sol, n_ant) + 2 * (int64_t)n_maps * n_sol;
}

// [n_ms][3][n_tri] doubles (Re A, Im A, B), [n_ms][n_ant][2] doubles (the start gains),
// [n_ms][n_tri] int32 (the counts), rounded up to 8 bytes
size_t gaincal_workspace_bytes(int n_maps, int n_sol, int n_ant) {
  const size_t ms = (size_t)n_maps * n_sol, tri = (size_t)gc_tri(n_ant);
  return 8 * ms * (3 * tri + 2 * (size_t)n_ant) + ((4 * ms * tri + 7) / 8) * 8;
}

// pairs before row p of the p-major list of (p < q) pairs of n antennas
__device__ __forceinline__ int gc_row_start(int p, int n) { return p * (2 * n - p - 1) / 2; }

// pq -> p (n <= 64: every integer below is exact in a float)
__device__ __forceinline__ int gc_row(int pq, int n) {
  const int a = 2 * n - 1;
  int p = (int)(((float)a - __builtin_sqrtf((float)(a * a - 8 * pq))) * 0.5f);
  p = p < 0 ? 0 : (p > n - 2 ? n - 2 : p);
  while (p > 0 && gc_row_start(p, n) > pq) --p;
  while (p < n - 2 && gc_row_start(p + 1, n) <= pq) ++p;
  return p;
}

// Lane `tid` of a workgroup whose first flat index is `base`, over rows of n_in entries and groups of
// n_out rows -> (group, row in group, entry in row).  The 64-bit divisions are of workgroup-uniform
// numbers (once per wave, on the scalar unit); a lane divides 32-bit numbers only.
__device__ __forceinline__ void gc_split(int64_t base, unsigned tid, unsigned n_in, unsigned n_out,
                                         int64_t& group, int& row, int& col) {
  const int64_t row0 = base / n_in;
  const int64_t group0 = row0 / n_out;
  const unsigned x = (unsigned)(base - row0 * n_in) + tid;
  const unsigned ax = x / n_in;
  const unsigned y = (unsigned)(row0 - group0 * n_out) + ax;
  const unsigned ay = y / n_out;
  col = (int)(x - ax * n_in);
  row = (int)(y - ay * n_out);
  group = group0 + ay;
}

__global__ __launch_bounds__(kGcB) void gain_apply_kernel(
    const double* __restrict__ vis, int64_t total, int n_t, int n_ant, int n_bl,
    const double* __restrict__ gains, int g_maps, int n_sol, const double* __restrict__ sol,
    int mode, double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * kGcB + threadIdx.x;
  if (idx >= total) return;
  int64_t m;
  int t, pq;
  gc_split((int64_t)blockIdx.x * kGcB, threadIdx.x, (unsigned)n_bl, (unsigned)n_t, m, t, pq);
  const int s = (int)sol[t];
  const int p = gc_row(pq, n_ant), q = pq - gc_row_start(p, n_ant) + p + 1;
  const double* __restrict__ g = gains + ((g_maps == 1 ? 0 : m) * n_sol + s) * n_ant * 2;
  const double pr = g[2 * p], pi = g[2 * p + 1], qr = g[2 * q], qi = g[2 * q + 1];
  const double vr = vis[2 * idx], vi = vis[2 * idx + 1];
  const double cr = __builtin_fma(pr, qr, pi * qi);
  const double ci = __builtin_fma(pi, qr, -(pr * qi));
  double o_r, o_i;
  if (mode == 0) {
    o_r = __builtin_fma(cr, vr, -(ci * vi));
    o_i = __builtin_fma(cr, vi, ci * vr);
  } else {
    const double n2 = __builtin_fma(cr, cr, ci * ci);
    o_r = __builtin_fma(vr, cr, vi * ci) / n2;
    o_i = __builtin_fma(vi, cr, -(vr * ci)) / n2;
  }
  out[2 * idx] = o_r;
  out[2 * idx + 1] = o_i;
}

hipError_t gain_apply_launch(const double* vis, int n_maps, int n_t, int n_ant, const double* gains,
                             int g_maps, int n_sol, const double* d_sol, int mode, double* out,
                             hipStream_t st) {
  const int64_t total = (int64_t)n_maps * n_t * gc_tri(n_ant);
  hipLaunchKernelGGL(gain_apply_kernel, dim3((unsigned)gain_apply_workgroups(n_maps, n_t, n_ant)),
                     dim3(kGcB), 0, st, vis, total, n_t, n_ant, (int)gc_tri(n_ant), gains, g_maps,
                     n_sol, d_sol, mode, out);
  return hipGetLastError();
}

// the counting rule, and the visibility's terms
__device__ __forceinline__ bool gc_counts(double dr, double di, double mr, double mi, double w,
                                          double& m2) {
  m2 = __builtin_fma(mr, mr, mi * mi);
  return finite_d(dr) && finite_d(di) && finite_d(mr) && finite_d(mi) && finite_d(w) && w > 0.0 &&
         m2 > 0.0;
}

__global__ __launch_bounds__(kGcB) void gaincal_accumulate_kernel(
    const double* __restrict__ vis, const double* __restrict__ model, const double* __restrict__ w,
    int64_t total, int n_t, int n_sol, int n_bl, int model_maps, int w_maps,
    const double* __restrict__ t0, double* __restrict__ AB, int* __restrict__ cnt) {
  const int64_t idx = (int64_t)blockIdx.x * kGcB + threadIdx.x;
  if (idx >= total) return;
  int64_t m;
  int s, pq;
  gc_split((int64_t)blockIdx.x * kGcB, threadIdx.x, (unsigned)n_bl, (unsigned)n_sol, m, s, pq);
  const int64_t ms = m * n_sol + s;
  const int ta = (int)t0[s], tb = (int)t0[s + 1];
  const double* __restrict__ D = vis + (m * n_t * n_bl + pq) * 2;
  const double* __restrict__ M = model + ((model_maps == 1 ? 0 : m) * n_t * n_bl + pq) * 2;
  const double* __restrict__ W = w ? w + (w_maps == 1 ? 0 : m) * n_t * n_bl + pq : nullptr;
  double ar = 0.0, ai = 0.0, b = 0.0;
  int n = 0;
  for (int t = ta; t < tb; ++t) {
    const int64_t o = (int64_t)t * n_bl;
    const double dr = D[2 * o], di = D[2 * o + 1], mr = M[2 * o], mi = M[2 * o + 1];
    const double wt = W ? W[o] : 1.0;
    double m2;
    if (!gc_counts(dr, di, mr, mi, wt, m2)) continue;
    ar = __builtin_fma(wt, __builtin_fma(dr, mr, di * mi), ar);
    ai = __builtin_fma(wt, __builtin_fma(di, mr, -(dr * mi)), ai);
    b = __builtin_fma(wt, m2, b);
    ++n;
  }
  double* __restrict__ o = AB + ms * 3 * n_bl;
  o[pq] = ar;
  o[n_bl + pq] = ai;
  o[2 * n_bl + pq] = b;
  cnt[idx] = n;
}

__device__ __forceinline__ double gc_wave_max(double x) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) x = __builtin_fmax(x, __shfl_xor(x, d, kGcW));
  return x;
}

template <int CAP>
__global__ __launch_bounds__(kGcW) void gaincal_solve_kernel(
    const double* __restrict__ AB, const int* __restrict__ cnt, int n_ant, int n_tri, int mode,
    int refant, int min_bl, double tol, int n_iter, double* __restrict__ gains,
    double* __restrict__ g0, int* __restrict__ o_nvis, int* __restrict__ o_niter,
    int* __restrict__ o_status, uint8_t* __restrict__ o_live, double* __restrict__ trace) {
  constexpr int TRI = CAP * (CAP - 1) / 2;
  __shared__ double sAr[TRI], sAi[TRI], sB[TRI];
  __shared__ double sgr[CAP], sgi[CAP], sg2[CAP];
  __shared__ int slive[CAP];
  const int64_t ms = blockIdx.x;
  const int p = threadIdx.x;
  const bool ant = p < n_ant;
  const double nan = __builtin_nan("");
  int nv = 0;
  {
    const double* __restrict__ a = AB + ms * 3 * n_tri;
    const int* __restrict__ c = cnt + ms * n_tri;
    for (int i = p; i < n_tri; i += kGcW) {
      sAr[i] = a[i];
      sAi[i] = a[n_tri + i];
      sB[i] = a[2 * n_tri + i];
      nv += c[i];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nv += __shfl_xor(nv, d, kGcW);
  }
  if (ant) slive[p] = 1;
  __syncthreads();
  // the live set: sweeps in which every antenna counts its partners by the flags of the sweep
  // before, and all that fall short leave together
  bool live = ant;
  while (true) {
    int c = 0;
    if (live)
      for (int q = 0; q < n_ant; ++q) {
        if (q == p || !slive[q]) continue;
        const int lo = q < p ? q : p, hi = q < p ? p : q;
        c += sB[gc_row_start(lo, n_ant) + hi - lo - 1] > 0.0 ? 1 : 0;
      }
    const bool drop = live && c < min_bl;
    __syncthreads();
    if (drop) {
      slive[p] = 0;
      live = false;
    }
    __syncthreads();
    if (!__any(drop)) break;
  }
  const unsigned long long lmask = __ballot(live);
  const int n_live = __popcll(lmask);
  double gr = 0.0, gi = 0.0;
  if (ant) {
    gr = gains[(ms * n_ant + p) * 2];
    gi = gains[(ms * n_ant + p) * 2 + 1];
  }
  const bool bad = live && !(finite_d(gr) && finite_d(gi) && (gr != 0.0 || gi != 0.0));
  if (__any(bad) || n_live < (mode == 0 ? 3 : 2)) {
    if (ant) {
      gains[(ms * n_ant + p) * 2] = nan;
      gains[(ms * n_ant + p) * 2 + 1] = nan;
    }
    if (p == 0) {
      o_nvis[ms] = nv;
      o_status[ms] = 3;
    }
    return;
  }
  if (ant) {
    g0[(ms * n_ant + p) * 2] = gr;
    g0[(ms * n_ant + p) * 2 + 1] = gi;
    o_live[ms * n_ant + p] = live ? 1 : 0;
  }
  int status = 0, it = 0;
  for (int k = 1;; ++k) {
    if (ant) {
      sgr[p] = gr;
      sgi[p] = gi;
      sg2[p] = __builtin_fma(gr, gr, gi * gi);
    }
    __syncthreads();
    double nr[4] = {0.0, 0.0, 0.0, 0.0}, ni[4] = {0.0, 0.0, 0.0, 0.0}, dn[4] = {0.0, 0.0, 0.0, 0.0};
    if (live) {
      for (int q0 = 0; q0 < n_ant; q0 += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int q = q0 + j;
          if (q >= n_ant || !slive[q] || q == p) continue;
          const int lo = q < p ? q : p, hi = q < p ? p : q;
          const int i = gc_row_start(lo, n_ant) + hi - lo - 1;
          const double a_r = sAr[i], a_i = q < p ? -sAi[i] : sAi[i];
          const double qr = sgr[q], qi = sgi[q];
          nr[j] = __builtin_fma(qr, a_r, nr[j]);
          nr[j] = __builtin_fma(-qi, a_i, nr[j]);
          ni[j] = __builtin_fma(qr, a_i, ni[j]);
          ni[j] = __builtin_fma(qi, a_r, ni[j]);
          if (mode == 0) dn[j] = __builtin_fma(sg2[q], sB[i], dn[j]);
        }
      }
    }
    const double numr = (nr[0] + nr[1]) + (nr[2] + nr[3]);
    const double numi = (ni[0] + ni[1]) + (ni[2] + ni[3]);
    const double div = mode == 0 ? (dn[0] + dn[1]) + (dn[2] + dn[3])
                                 : __builtin_sqrt(__builtin_fma(numr, numr, numi * numi));
    const double hr = numr / div, hi = numi / div;
    const bool ok = !live || (finite_d(div) && div > 0.0 && finite_d(hr) && finite_d(hi));
    if (!__all(ok)) {
      status = 2;
      it = k - 1;
      break;
    }
    double d = 0.0, a = 0.0;
    if (live) {
      const double xr = (k & 1) ? hr : 0.5 * (hr + gr), xi = (k & 1) ? hi : 0.5 * (hi + gi);
      const double er = xr - gr, ei = xi - gi;
      d = __builtin_sqrt(__builtin_fma(er, er, ei * ei));
      a = __builtin_sqrt(__builtin_fma(xr, xr, xi * xi));
      gr = xr;
      gi = xi;
    }
    if (trace && ant) {
      double* __restrict__ row = trace + ((ms * n_iter + (k - 1)) * n_ant + p) * 2;
      row[0] = live ? gr : nan;
      row[1] = live ? gi : nan;
    }
    const double dmax = gc_wave_max(d), gmax = gc_wave_max(a);
    __syncthreads();                       // every lane has read the gains of step k - 1
    it = k;
    if (dmax <= tol * gmax) {
      status = 1;
      break;
    }
    if (k == n_iter) break;
  }
  // the reference antenna
  if (ant) {
    sgr[p] = gr;
    sgi[p] = gi;
  }
  __syncthreads();
  const int r = ((lmask >> refant) & 1ull) ? refant : __ffsll((long long)lmask) - 1;
  const double rr = sgr[r], ri = sgi[r];
  const double ra = __builtin_sqrt(__builtin_fma(rr, rr, ri * ri));
  const double cr = rr / ra, ci = -(ri / ra);
  if (ant) {
    double xr = nan, xi = nan;
    if (live) {
      xr = __builtin_fma(gr, cr, -(gi * ci));
      xi = p == r ? 0.0 : __builtin_fma(gr, ci, gi * cr);
    }
    gains[(ms * n_ant + p) * 2] = xr;
    gains[(ms * n_ant + p) * 2 + 1] = xi;
  }
  if (p == 0) {
    o_nvis[ms] = nv;
    o_niter[ms] = it;
    o_status[ms] = status;
  }
}

__global__ __launch_bounds__(kGcB) void gaincal_residual_kernel(
    const double* __restrict__ vis, const double* __restrict__ model, const double* __restrict__ w,
    int n_t, int n_sol, int n_ant, int n_bl, int model_maps, int w_maps,
    const double* __restrict__ t0, const double* __restrict__ gains, const double* __restrict__ g0,
    const uint8_t* __restrict__ o_live, const int* __restrict__ o_status,
    double* __restrict__ chi2) {
  __shared__ double s0[kGcB], s1[kGcB];
  const int64_t ms = blockIdx.x;
  if (o_status[ms] == 3) return;
  const int64_t m = ms / n_sol;
  const int s = (int)(ms - m * n_sol);
  const int ta = (int)t0[s], tb = (int)t0[s + 1];
  const double* __restrict__ ga = g0 + ms * n_ant * 2;
  const double* __restrict__ gb = gains + ms * n_ant * 2;
  const uint8_t* __restrict__ lv = o_live + ms * n_ant;
  double x0 = 0.0, x1 = 0.0;
  for (int pq = threadIdx.x; pq < n_bl; pq += kGcB) {
    const int p = gc_row(pq, n_ant), q = pq - gc_row_start(p, n_ant) + p + 1;
    if (!(lv[p] && lv[q])) continue;
    const double ar = __builtin_fma(ga[2 * p], ga[2 * q], ga[2 * p + 1] * ga[2 * q + 1]);
    const double ai = __builtin_fma(ga[2 * p + 1], ga[2 * q], -(ga[2 * p] * ga[2 * q + 1]));
    const double br = __builtin_fma(gb[2 * p], gb[2 * q], gb[2 * p + 1] * gb[2 * q + 1]);
    const double bi = __builtin_fma(gb[2 * p + 1], gb[2 * q], -(gb[2 * p] * gb[2 * q + 1]));
    const double* __restrict__ D = vis + (m * n_t * n_bl + pq) * 2;
    const double* __restrict__ M = model + ((model_maps == 1 ? 0 : m) * n_t * n_bl + pq) * 2;
    const double* __restrict__ W = w ? w + (w_maps == 1 ? 0 : m) * n_t * n_bl + pq : nullptr;
    for (int t = ta; t < tb; ++t) {
      const int64_t o = (int64_t)t * n_bl;
      const double dr = D[2 * o], di = D[2 * o + 1], mr = M[2 * o], mi = M[2 * o + 1];
      const double wt = W ? W[o] : 1.0;
      double m2;
      if (!gc_counts(dr, di, mr, mi, wt, m2)) continue;
      double er = dr - __builtin_fma(ar, mr, -(ai * mi));
      double ei = di - __builtin_fma(ar, mi, ai * mr);
      x0 = __builtin_fma(wt * er, er, x0);
      x0 = __builtin_fma(wt * ei, ei, x0);
      er = dr - __builtin_fma(br, mr, -(bi * mi));
      ei = di - __builtin_fma(br, mi, bi * mr);
      x1 = __builtin_fma(wt * er, er, x1);
      x1 = __builtin_fma(wt * ei, ei, x1);
    }
  }
  s0[threadIdx.x] = x0;
  s1[threadIdx.x] = x1;
  __syncthreads();
  for (int h = kGcB / 2; h >= 1; h >>= 1) {
    if ((int)threadIdx.x < h) {
      s0[threadIdx.x] += s0[threadIdx.x + h];
      s1[threadIdx.x] += s1[threadIdx.x + h];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    chi2[2 * ms] = s0[0];
    chi2[2 * ms + 1] = s1[0];
  }
}

hipError_t gaincal_launch(const double* vis, const double* model, int model_maps, const double* w,
                          int w_maps, int n_maps, int n_t, int n_ant, int n_sol, const double* d_t0,
                          int mode, int refant, int min_bl, double tol, int n_iter, double* gains,
                          double* chi2, int32_t* nvis, int32_t* niter, int32_t* status,
                          uint8_t* live, double* trace, void* work, hipStream_t st) {
  const int n_tri = (int)gc_tri(n_ant);
  const int64_t n_ms = (int64_t)n_maps * n_sol;
  double* AB = (double*)work;
  double* g0 = AB + n_ms * 3 * n_tri;
  int* cnt = (int*)(g0 + n_ms * 2 * n_ant);
  hipLaunchKernelGGL(gaincal_accumulate_kernel,
                     dim3((unsigned)gc_acc_workgroups(n_maps, n_sol, n_ant)), dim3(kGcB), 0, st, vis,
                     model, w, n_ms * n_tri, n_t, n_sol, n_tri, model_maps, w_maps, d_t0, AB, cnt);
  if (hipError_t e = hipGetLastError()) return e;
#define RJP_GC(CAP)                                                                               \
  hipLaunchKernelGGL((gaincal_solve_kernel<CAP>), dim3((unsigned)n_ms), dim3(kGcW), 0, st, AB,    \
                     cnt, n_ant, n_tri, mode, refant, min_bl, tol, n_iter, gains, g0, nvis, niter, \
                     status, live, trace)
  if (n_ant <= 16) RJP_GC(16);
  else if (n_ant <= 32) RJP_GC(32);
  else RJP_GC(64);
#undef RJP_GC
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(gaincal_residual_kernel, dim3((unsigned)n_ms), dim3(kGcB), 0, st, vis, model,
                     w, n_t, n_sol, n_ant, n_tri, model_maps, w_maps, d_t0, gains, g0, live, status,
                     chi2);
  return hipGetLastError();
}

}  // namespace rjp
