// Field layout kernels: upload packing, K4 (geometry -> fields on the device) and the
// synthetic dense-field generator of the measurement harness.
#include <algorithm>
#include <cmath>
#include <string>

#include "rjp_host.h"

namespace rjp {

constexpr int kFB = 256;

__device__ __forceinline__ double with_sign(double mag, bool neg) {
  long long bits = __double_as_longlong(mag) & 0x7FFFFFFFFFFFFFFFll;
  if (neg) bits |= (long long)0x8000000000000000ull;
  return __longlong_as_double(bits);
}

// ---- upload packing ---------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kFB) void pack_field_kernel(const double* __restrict__ src,
                                                         const double* __restrict__ den,
                                                         const uint8_t* __restrict__ red,
                                                         T* __restrict__ dst, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * kFB + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kFB;
  for (; i < n; i += step) {
    double v = src[i];
    if (den) v = v / den[i];
    if (red) v = with_sign(v, red[i] != 0);
    dst[i] = (T)v;     // a float cast keeps the sign bit, NaN stays NaN
  }
}

hipError_t pack_field_launch(const double* src, const double* den, const uint8_t* red,
                             void* dst, int64_t n, int dtype, hipStream_t st) {
  const unsigned blocks = (unsigned)std::min<int64_t>((n + kFB - 1) / kFB, 256 * 16);
  if (dtype == RJP_F64)
    hipLaunchKernelGGL(pack_field_kernel<double>, dim3(blocks), dim3(kFB), 0, st, src, den,
                       red, (double*)dst, n);
  else
    hipLaunchKernelGGL(pack_field_kernel<float>, dim3(blocks), dim3(kFB), 0, st, src, den,
                       red, (float*)dst, n);
  return hipGetLastError();
}

// ---- compact scan layout ------------------------------------------------------------------
// One field for K1 instead of three (rjp_fields.d_em0): (|nd| xi)^2 pf, evaluated in the very
// order K1 uses on the wide layout (so both layouts give bit-identical maps), with the
// red-jet flag in the sign bit.
template <typename T>
__global__ __launch_bounds__(kFB) void compact_fields_kernel(
    const T* __restrict__ nd, const T* __restrict__ xi, const T* __restrict__ pf,
    T* __restrict__ em0, int64_t n, unsigned long long* __restrict__ n_bad) {
  int64_t i = (int64_t)blockIdx.x * kFB + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kFB;
  unsigned bad = 0;
  for (; i < n; i += step) {
    const double d = (double)nd[i], p = (double)pf[i];
    const double n0 = fabs(d) * (double)xi[i];
    const double g = n0 * n0 * p;
    if (p < 0.0) bad++;                    // the sign bit is taken: such a field stays wide
    const T out = (T)g;
    if (sizeof(T) == 4) {
      // float storage must hold the product: no overflow, no flush of a non-zero term
      const double back = fabs((double)out);
      if (g == g && fabs(g) <= 1.7e308 && (back > 3.4e38 || (g != 0.0 && back < 1.2e-38))) bad++;
    }
    // NaN keeps its payload; only the sign bit changes
    if (sizeof(T) == 8) {
      em0[i] = (T)with_sign(g, signbit_d(d));
    } else {
      unsigned u = __float_as_uint((float)out) & 0x7FFFFFFFu;
      if (signbit_d(d)) u |= 0x80000000u;
      em0[i] = (T)__uint_as_float(u);
    }
  }
  if (bad) atomicAdd(n_bad, (unsigned long long)bad);
}

hipError_t compact_fields_launch(const rjp_fields* fl, void* d_em0, int64_t* d_n_bad,
                                 hipStream_t st) {
  const int64_t n = (int64_t)fl->nx * fl->ny * fl->nz;
  hipError_t e = hipMemsetAsync(d_n_bad, 0, sizeof(int64_t), st);
  if (e != hipSuccess) return e;
  const unsigned blocks = (unsigned)std::min<int64_t>((n + kFB - 1) / kFB, 256 * 32);
  if (fl->dtype == RJP_F64)
    hipLaunchKernelGGL(compact_fields_kernel<double>, dim3(blocks), dim3(kFB), 0, st,
                       (const double*)fl->d_nd, (const double*)fl->d_xi, (const double*)fl->d_pf,
                       (double*)d_em0, n, (unsigned long long*)d_n_bad);
  else
    hipLaunchKernelGGL(compact_fields_kernel<float>, dim3(blocks), dim3(kFB), 0, st,
                       (const float*)fl->d_nd, (const float*)fl->d_xi, (const float*)fl->d_pf,
                       (float*)d_em0, n, (unsigned long long*)d_n_bad);
  return hipGetLastError();
}

// ---- tau scan layout ------------------------------------------------------------------------
// a0 = em0 * T^-1.5 (scalar Gaunt factor) or em0 * T^-1.35 (power law): every factor of a
// cell's free-free optical depth that depends on neither frequency nor epoch
// (classes.py:1395-1397), formed exactly as K1 forms it on the compact layout (fabs(em0) *
// tpow), red-jet flag in the sign bit.  f64 storage.
__global__ __launch_bounds__(kFB) void tau_field_kernel(const double* __restrict__ em0,
                                                        const double* __restrict__ temp,
                                                        int gff_mode, double* __restrict__ a0,
                                                        int64_t n) {
  int64_t i = (int64_t)blockIdx.x * kFB + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kFB;
  for (; i < n; i += step) {
    const double g = em0[i];
    a0[i] = with_sign(fabs(g) * tau_weight(temp[i], gff_mode), signbit_d(g));
  }
}

hipError_t tau_field_launch(const rjp_fields* fl, int gff_mode, void* d_a0, hipStream_t st) {
  const int64_t n = (int64_t)fl->nx * fl->ny * fl->nz;
  const unsigned blocks = (unsigned)std::min<int64_t>((n + kFB - 1) / kFB, 256 * 32);
  hipLaunchKernelGGL(tau_field_kernel, dim3(blocks), dim3(kFB), 0, st, (const double*)fl->d_em0,
                     (const double*)fl->d_temp, gff_mode, (double*)d_a0, n);
  return hipGetLastError();
}

// ---- launch times of a jet without bursts -----------------------------------------------------
// The reference's burst Gaussians carry a NaN launch time into the cell's density (dropped by
// nansum) -- but a jet WITHOUT any registered burst has the constant steady-state mass-loss
// rate whatever the launch time (classes.py:232-233, 442-448): its cells keep chi = 1.  The
// free-free scan masks every cell with a NaN launch time as soon as the model has a burst, so
// a model with bursts in ONE jet only scans a copy of `ts` in which the NaNs of the other
// jet's cells are replaced by fields.ts_lo (any finite value gives chi = 1 there).  `flag`: a field that
// carries the red-jet flag in its sign bit (a0, em0 or nd).
template <typename T>
__global__ __launch_bounds__(kFB) void unmask_ts_kernel(const T* __restrict__ ts,
                                                        const T* __restrict__ flag, int jet,
                                                        T fill, T* __restrict__ out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * kFB + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kFB;
  for (; i < n; i += step) {
    const double t = (double)ts[i];
    const bool red = signbit_d((double)flag[i]);
    const bool mine = red == (jet == 0);
    out[i] = (!(t == t) && mine) ? fill : ts[i];
  }
}

hipError_t unmask_ts_launch(const rjp_fields* fl, int jet, void* d_out, hipStream_t st) {
  const int64_t n = (int64_t)fl->nx * fl->ny * fl->nz;
  const unsigned blocks = (unsigned)std::min<int64_t>((n + kFB - 1) / kFB, 256 * 32);
  const void* flag = fl->d_a0 ? fl->d_a0 : fl->d_em0 ? fl->d_em0 : fl->d_nd;
  // the replacement value lies INSIDE the declared launch-time range (its lower end; 0 when no
  // range is given): the copy is scanned under the same range, and the range guard watches it
  const double fill = fl->ts_lo;
  if (fl->dtype == RJP_F64)
    hipLaunchKernelGGL(unmask_ts_kernel<double>, dim3(blocks), dim3(kFB), 0, st,
                       (const double*)fl->d_ts, (const double*)flag, jet, fill, (double*)d_out, n);
  else
    hipLaunchKernelGGL(unmask_ts_kernel<float>, dim3(blocks), dim3(kFB), 0, st,
                       (const float*)fl->d_ts, (const float*)flag, jet, (float)fill, (float*)d_out, n);
  return hipGetLastError();
}

// ---- synthetic dense fields --------------------------------------------
// No FMA contraction from here to the end of K4: the generator must be bit-identical to its
// host restatement, and K4's inside test must follow NumPy's operation order.
#pragma clang fp contract(off)
template <typename T>
__global__ __launch_bounds__(kFB) void synth_kernel(uint64_t seed, int temp_mode, int nz,
                                                    int64_t cell0, int64_t n, T* nd, T* xi,
                                                    T* temp, T* pf, T* ts, T* vy, T* em0,
                                                    T* a0, int a0_mode) {
  int64_t i = (int64_t)blockIdx.x * kFB + threadIdx.x;
  const int64_t step = (int64_t)gridDim.x * kFB;
  for (; i < n; i += step) {
    const uint64_t cell = (uint64_t)(cell0 + i);
    const int iz = (int)(cell % (uint64_t)nz);
    const bool red = iz < nz / 2;
    const double un = hash_u01(seed, 1, cell), ux = hash_u01(seed, 2, cell),
                 ut = hash_u01(seed, 3, cell), up = hash_u01(seed, 4, cell),
                 us = hash_u01(seed, 5, cell), uv = hash_u01(seed, 6, cell);
    const double n0 = exp10(5.0 + 2.5 * un);
    if (nd) nd[i] = (T)with_sign(n0, red);
    if (xi) xi[i] = (T)(0.05 + 0.45 * ux);
    const double tk = temp_mode == 0 ? 1e4 : 5e3 + 1.5e4 * ut;
    if (temp) temp[i] = (T)tk;
    if (pf) pf[i] = (T)(up < 0.25 ? 0.5 : 1.0);
    if (em0 || a0) {   // the derived scan fields straight from the generator (f64): as
                       // compact_fields_kernel / tau_field_kernel
      const double e0 = n0 * (0.05 + 0.45 * ux);
      const double g = e0 * e0 * (up < 0.25 ? 0.5 : 1.0);
      if (em0) em0[i] = (T)with_sign(g, red);
      if (a0) a0[i] = (T)with_sign(g * tau_weight(tk, a0_mode), red);
    }
    if (ts) ts[i] = (T)(5.0 * us * 31536000.0);
    if (vy) vy[i] = (T)(6.2 + 60.0 * (uv - 0.5));
  }
}

hipError_t synth_launch(uint64_t seed, int temp_mode, int nz, int64_t cell0, int64_t n,
                        int dtype, void* nd, void* xi, void* temp, void* pf, void* ts, void* vy,
                        void* em0, void* a0, int a0_mode, hipStream_t st) {
  const unsigned blocks = (unsigned)std::min<int64_t>((n + kFB - 1) / kFB, 256 * 32);
  if (dtype == RJP_F64)
    hipLaunchKernelGGL(synth_kernel<double>, dim3(blocks), dim3(kFB), 0, st, seed, temp_mode, nz,
                       cell0, n, (double*)nd, (double*)xi, (double*)temp, (double*)pf,
                       (double*)ts, (double*)vy, (double*)em0, (double*)a0, a0_mode);
  else
    hipLaunchKernelGGL(synth_kernel<float>, dim3(blocks), dim3(kFB), 0, st, seed, temp_mode, nz,
                       cell0, n, (float*)nd, (float*)xi, (float*)temp, (float*)pf, (float*)ts,
                       (float*)vy, (float*)em0, (float*)nullptr, a0_mode);
  return hipGetLastError();
}

// ---- K4: geometry -> fields ---------------------------------------------------------------
// One thread per cell.  Follows the reference's floating-point ORDER (no FMA contraction)
// for everything that feeds a comparison (the 8-vertex inside test, classes.py:657-669), so
// that the jet mask comes out identical; the rotation sines/cosines are computed on the host
// (NumPy) and passed in, as the reference does (maths/geometry.py:249-253).

// x^p for a finite normal x > 0 and |p log2 x| < 1000, relative error < 1e-14 (|p log2 x| up
// to ~100): log2 x = e + 2 atanh((m-1)/(m+1)) log2(e) with m in [sqrt(1/2), sqrt 2) (degree-9
// series in s^2, s^2 <= 0.0295), then 2^t by exp2_any.  ~45 instructions against ~130 of
// libm's pow; anything else (0, negative, inf, NaN, denormal) goes to pow().
__device__ __forceinline__ double pow_pos(double x, double p) {
  if (!(x >= 2.3e-308 && x <= 1.7e308)) return pow(x, p);
  double m = __builtin_amdgcn_frexp_mant(x);               // [0.5, 1)
  int e = __builtin_amdgcn_frexp_exp(x);
  const bool low = m < 0.70710678118654752440;
  m = low ? 2.0 * m : m;
  e = low ? e - 1 : e;
  const double sv = (m - 1.0) * rcp_newton(m + 1.0);
  const double s2 = sv * sv;
  double q = 2.0 / 19.0;
  q = __builtin_fma(q, s2, 2.0 / 17.0);
  q = __builtin_fma(q, s2, 2.0 / 15.0);
  q = __builtin_fma(q, s2, 2.0 / 13.0);
  q = __builtin_fma(q, s2, 2.0 / 11.0);
  q = __builtin_fma(q, s2, 2.0 / 9.0);
  q = __builtin_fma(q, s2, 2.0 / 7.0);
  q = __builtin_fma(q, s2, 2.0 / 5.0);
  q = __builtin_fma(q, s2, 2.0 / 3.0);
  q = __builtin_fma(q, s2, 2.0);
  const double l2m = (sv * q) * 1.4426950408889634074;     // log2 m, |.| <= 1/2
  const double t = __builtin_fma(p, (double)e, p * l2m);
  if (!(fabs(t) < 1000.0)) return pow(x, p);
  return exp2_any(t);
}

__device__ __forceinline__ void xyz_to_rw(const GeomDev& g, double x, double y, double z,
                                          double& r, double& w, double& x2, double& y2) {
  // geometry.py:206 xyz_rotate(order='yx'): y-rotation first, then x-rotation
  const double x1 = g.cb * x + g.sb * z;
  const double y1 = y;
  const double z1 = g.cb * z - g.sb * x;
  x2 = x1;
  y2 = g.ca * y1 - g.sa * z1;
  r = g.sa * y1 + g.ca * z1;
  w = sqrt(x2 * x2 + y2 * y2);      // x ** 2. is an exact square in NumPy too
}

__device__ __forceinline__ double rho_mod(const GeomDev& g, double r) {
  return (fabs(r) + g.mr0 - g.r_0) / g.mr0;          // geometry.py:58-59
}

__device__ __forceinline__ double powerlaw(double zero, double rho_, double reff, double r1,
                                           double q, double qd) {
  // geometry.py:92; x ** 0. == 1 in NumPy, pow() agrees
  double v = zero * pow(rho_, q) * pow(reff / r1, qd);
  if (v == 0.0 || isinf(v)) v = __builtin_nan("");  // classes.py:892, 897
  return v;
}

// S(a, beta, s) = 2F1(a, 1; beta + 1; s) = sum_k (a)_k / (beta + 1)_k s^k for 0 <= s < 1.  A term
// below kHypStop of the sum ends the series -- but only once the denominators beta + 1 + k are
// positive and the term ratio is below 1: with beta = a - b < 0 (the connection formula) the terms
// first fall, far below kHypStop for large b, and rise again to order one around
// k = (b - a)(1 + 1/A); a series cut in the dip is wrong by that hump.  hyp_plan (below) keeps
// every series the kernel meets within kHypMaxTerms.
__device__ __forceinline__ double hyp_series(double a, double beta, double s) {
  double term = 1.0, sum = 1.0;
  for (int k = 0; k < kHypMaxTerms; ++k) {
    const double den = beta + 1.0 + k;
    const double ratio = (a + k) / den * s;
    term *= ratio;
    sum += term;
    if (fabs(term) <= kHypStop * fabs(sum) && den > 0.0 && fabs(ratio) < 1.0) break;
  }
  return sum;
}

// A^a * 2F1(a, b; b+1; -A) for A > 0: the product p2*p3*p4 of maths/geometry.py:159-171
// (p2 p3 = (1 + 1/A)^-a (A + 1)^a = A^a).  Pfaff's transformation for A <= hy_switch, the 1/z
// connection formula (DLMF 15.8.2 with c = b + 1) followed by Pfaff above it.  hy_switch is 1
// where the connection formula is sound from there on; for large b, or a - b close to a
// non-positive integer, it cancels (or needs hundreds of terms) near A = 1 and the host moves the
// switch up.
__device__ __forceinline__ double hyp_flow_factor(const GeomDev& g, double A) {
  const double a = g.hy_a, b = g.hy_b;
  const double s = A / (1.0 + A);
  const double sa = pow(s, a);                     // A^a (1 + A)^-a
  if (A <= g.hy_switch) return sa * hyp_series(a, b, s);
  return sa * g.hy_k1 * hyp_series(a, a - b, 1.0 / (1.0 + A)) + g.hy_k2 * pow(A, a - b);
}

// indefinite integral of geometry.py:150-173 at (r_ [m], w_ [m])
__device__ __forceinline__ double flow_time_antiderivative(const GeomDev& g, double r_m,
                                                           double w_m) {
  const double rad = r_m + g.mr0_m - g.r0_m;
  const double lead = g.ts_const * pow(rad, g.ts_pow);
  if (w_m == 0.0) return lead * g.hy_axis;          // p2 = p3 = 1, p4 = 1 + q^d_v/(1 - q_v)
  const double A = (g.r1_m * g.w0_m * pow(rad, g.eps)) /
                   (w_m * pow(g.mr0_m, g.eps) * (g.r2_m - g.r1_m));
  return lead * hyp_flow_factor(g, A);
}

template <typename T>
__global__ __launch_bounds__(kFB) void build_fields_kernel(GeomDev g, T* nd, T* xi, T* temp,
                                                           T* pf, T* ts, T* vy,
                                                           double* ff_raw, double* areas_raw,
                                                           double* vx_raw, double* vz_raw,
                                                           T* em0, T* a0, int a0_mode) {
  const int64_t n = (int64_t)g.nx * g.ny * g.nz;
  const int64_t i = (int64_t)blockIdx.x * kFB + threadIdx.x;
  if (i >= n) return;
  const int iz = (int)(i % g.nz);
  const int iy = (int)((i / g.nz) % g.ny);
  const int ix = (int)(i / ((int64_t)g.nz * g.ny));
  // classes.py:497-499: bottom-left-front corner
  const double x0 = g.cs * (g.ix0 + ix - g.nx_total / 2), y0 = g.cs * (iy - g.ny / 2),
               z0 = g.cs * (iz - g.nz / 2);

  // centroid coordinates (classes.py:521-525)
  const double h = g.cs / 2.0;
  double rr, ww, xa, ya;
  xyz_to_rw(g, x0 + h, y0 + h, z0 + h, rr, ww, xa, ya);
  const double ar_ = fabs(rr);

  // Most cells of a jet model lie far outside the jet (99.6 % of the example's grid), and the
  // vertex test below costs eight pow().  The rotation preserves lengths, so every vertex has
  // |r| <= |r_c| + d and w >= w_c - d with d = half the cell diagonal; for eps >= 0 and
  // mod_r_0 > 0 the jet width w_0 rho(r)^eps does not decrease with |r|, so a cell whose
  // centroid is further out than the width at |r_c| + d (or wholly inside |r| < r_0) has no
  // vertex inside -- decided with an f32 estimate of that width and a 1e-4 margin that dwarfs
  // its error and the rounding of either side.  Cells that pass, and every other geometry, take the reference's test.
  bool may_touch = true;
  if (g.eps >= 0.0 && g.mr0 > 0.0) {
    const double d = g.cs * 0.86602540378443865 * (1.0 + 1e-9);
    if (ar_ + d < g.r_0) may_touch = false;
    else {
      // (the bound only has to be safe: the hardware f32 log2 / exp2 with a 1e-4 margin)
      const float lr = __builtin_amdgcn_logf((float)rho_mod(g, ar_ + d));
      const double wmax = g.w_0 * (double)__builtin_amdgcn_exp2f((float)g.eps * lr);
      if (wmax * (1.0 + 1e-4) < ww - d) may_touch = false;      // false for NaN: keeps the test
    }
  }
  int n_in = 0;
  if (may_touch) {
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      const double dx = (v & 1) ? g.cs : 0.0, dy = (v & 2) ? g.cs : 0.0,
                   dz = (v & 4) ? g.cs : 0.0;
      double r, w, xv, yv;
      xyz_to_rw(g, x0 + dx, y0 + dy, z0 + dz, r, w, xv, yv);
      const double wr = g.w_0 * pow(rho_mod(g, r), g.eps);            // geometry.py:118
      if (wr >= w && fabs(r) >= g.r_0) ++n_in;                       // classes.py:665
    }
  }
  const double nan = __builtin_nan("");
  const double ff = n_in == 8 ? 1.0 : (n_in > 0 ? 0.5 : nan);
  const double ar = n_in > 0 ? 1.0 : nan;
  if (ff_raw) ff_raw[i] = ff;
  if (areas_raw) areas_raw[i] = ar;
  const bool jet = n_in > 0;
  // classes.py:884-886 (same clamp in ion_fraction / vel / ts)
  const double rc = (ar_ < g.r_0 && (ar_ + h) >= g.r_0) ? (g.r_0 + ar_ + h) / 2.0 : ar_;
  // classes.py:549-555: r_eff uses |rr| (unclamped)
  const double reff = g.R_1 + ((g.R_2 - g.R_1) * ww) / (g.w_0 * pow(rho_mod(g, ar_), g.eps));
  const double rho_c = rho_mod(g, rc);

  double tk = nan;
  if (temp || a0) {
    // classes.py:957-962: r converted to cm BEFORE the r_0 [au] comparison and rho()
    const double rcm = ar_ * 149597870700.0 * 1e2;
    const double rt = (rcm < g.r_0 && (rcm + h) >= g.r_0) ? (g.r_0 + rcm + h) / 2.0 : rcm;
    tk = jet ? powerlaw(g.T_0, rho_mod(g, rt), reff, g.R_1, g.q_T, g.qd_T) : nan;
    if (temp) temp[i] = (T)tk;
  }
  if (nd || em0 || a0) {
    double v = jet ? powerlaw(g.n_0, rho_c, reff, g.R_1, g.q_n, g.qd_n) : nan;
    if (rr < 0) v = v * g.rb_frac;                                 // classes.py:895
    if (nd) nd[i] = (T)with_sign(v, rr < 0);
    if (em0 || a0) {   // the derived scan fields straight from the builder (f64): as
                       // compact_fields_kernel / tau_field_kernel
      const double n0 = fabs(v) * (jet ? powerlaw(g.x_0, rho_c, reff, g.R_1, g.q_x, g.qd_x) : nan);
      const double gg = n0 * n0 * (ff / ar);
      if (em0) em0[i] = (T)with_sign(gg, rr < 0);
      if (a0) a0[i] = (T)with_sign(fabs(gg) * tau_weight(tk, a0_mode), rr < 0);
    }
  }
  if (xi) xi[i] = (T)(jet ? powerlaw(g.x_0, rho_c, reff, g.R_1, g.q_x, g.qd_x) : nan);
  if (pf) pf[i] = (T)(ff / ar);
  if (ts && g.ts_mode == 2) {
    const double au = 149597870700.0;
    const double t_yr = (flow_time_antiderivative(g, rc * au, ww * au) -
                         flow_time_antiderivative(g, g.r0_m, ww * au)) / 31536000.0;
    ts[i] = (T)(t_yr * 31536000.0);
  }
  if (ts && g.ts_mode == 1) {
    // geometry.py:150-178 with q^d_v == 0 (p2 = p3 = p4 = 1), in seconds
    const double au = 149597870700.0;
    const double rad = rc * au + g.mr0 * au - g.r_0 * au;
    const double t_yr = (g.ts_const * pow_pos(rad, g.ts_pow) - g.ts_base) / 31536000.0;
    ts[i] = (T)(t_yr * 31536000.0);
  }
  if (vy || vx_raw || vz_raw) {
    double out = nan, outx = nan, outz = nan;
    if (jet) {
      // classes.py:1056-1093
      double vz = powerlaw(g.v_0, rho_c, reff, g.R_1, g.q_v, g.qd_v);
      vz = vz * (rr > 0 ? 1.0 : (rr < 0 ? -1.0 : 0.0));
      // physics.py:90 with rho(self.rr) (unclamped)
      const double vr = sqrt(g.gm / (reff * 149597870700.0)) * pow(rho_mod(g, rr), -g.eps) / 1e3;
      // geometry.py:292-296: phi = arcsin(y/rho), mirrored for x < 0
      double phi = asin(ya / ww);
      if (xa < 0) phi = -phi + 3.141592653589793;
      const double sgn = g.ccw ? 1.0 : -1.0;
      const double vx0 = -vr * sin(phi) * sgn;
      const double vy0 = vr * cos(phi) * sgn;
      // xyz_rotate(order='xy') with (90 - inc, -pa): x-rotation then y-rotation; the
      // y-component after both is the x-rotated one
      const double y1 = g.ca2 * vy0 - g.sa2 * vz, z1 = g.sa2 * vy0 + g.ca2 * vz;
      out = y1 + g.v_lsr;
      outx = g.cb2 * vx0 + g.sb2 * z1;
      outz = g.cb2 * z1 - g.sb2 * vx0;
    }
    if (vy) vy[i] = (T)out;
    if (vx_raw) vx_raw[i] = outx;
    if (vz_raw) vz_raw[i] = outz;
  }
}
#pragma clang fp contract(fast)

hipError_t build_fields_launch(const GeomDev& g, int dtype, void* nd, void* xi, void* temp,
                               void* pf, void* ts, void* vy, double* ff_raw, double* areas_raw,
                               double* vx_raw, double* vz_raw, void* em0, void* a0, int a0_mode,
                               hipStream_t st) {
  const int64_t n = (int64_t)g.nx * g.ny * g.nz;
  const unsigned blocks = (unsigned)((n + kFB - 1) / kFB);
  if (dtype == RJP_F64)
    hipLaunchKernelGGL(build_fields_kernel<double>, dim3(blocks), dim3(kFB), 0, st, g, (double*)nd,
                       (double*)xi, (double*)temp, (double*)pf, (double*)ts, (double*)vy, ff_raw,
                       areas_raw, vx_raw, vz_raw, (double*)em0, (double*)a0, a0_mode);
  else
    hipLaunchKernelGGL(build_fields_kernel<float>, dim3(blocks), dim3(kFB), 0, st, g, (float*)nd,
                       (float*)xi, (float*)temp, (float*)pf, (float*)ts, (float*)vy, ff_raw,
                       areas_raw, vx_raw, vz_raw, (float*)nullptr, (float*)nullptr, 0);
  return hipGetLastError();
}

// ---- K4's 2F1: which series where ---------------------------------------------------------------
// hyp_series (above) on the host, also returning the largest |term| (the leading 1 included)
// and the number of terms taken (kHypMaxTerms + 1: the series did not end).
struct HypSum { double sum, big; int taken; };

static HypSum hyp_series_host(double a, double beta, double s) {
  HypSum r = {1.0, 1.0, kHypMaxTerms + 1};
  double term = 1.0;
  for (int k = 0; k < kHypMaxTerms; ++k) {
    const double den = beta + 1.0 + k;
    const double ratio = (a + k) / den * s;
    term *= ratio;
    r.sum += term;
    r.big = std::max(r.big, fabs(term));
    if (fabs(term) <= kHypStop * fabs(r.sum) && den > 0.0 && fabs(ratio) < 1.0) {
      r.taken = k + 1;
      break;
    }
  }
  return r;
}

// Gamma(b + 1) Gamma(a - b) / Gamma(a); through lgamma where a factor leaves the double range
// (b + 1 > 171: inf * 0)
static double hyp_gamma_ratio(double b, double amb, double a) {
  const double v = tgamma(b + 1.) * tgamma(amb) / tgamma(a);
  if (std::isfinite(v) && v != 0.0) return v;
  int s1 = 1, s2 = 1, s3 = 1;
  const double lg = lgamma_r(b + 1., &s1) + lgamma_r(amb, &s2) - lgamma_r(a, &s3);
  return (double)(s1 * s2 * s3) * exp(lg);
}

// The launch-time integral A^a 2F1(a, b; b + 1; -A) is summed by the Pfaff series for A <= switch
// and by the 1/z connection formula above it (hyp_flow_factor).  The connection
// formula is sound from A = 1 on for b of a few units.  For large b (narrow jets: b ~ 1/eps) its
// series first falls and then comes back to order one around k = (b - a)(1 + 1/A): hundreds of
// terms near A = 1.  For a - b within ~1e-4 of a non-positive integer its two parts cancel like
// 1/(distance A).  So the switch is the smallest of kHypSwitch at which (probed at five A from the
// switch upwards) the connection formula ends within kHypConnTerms terms and loses at most
// kHypMaxLoss to cancellation, while the Pfaff series ends within kHypMaxTerms at the switch; +inf
// (the Pfaff series for every A) serves large b.  No such switch: refused (false).
static bool hyp_plan(double a, double b, double* k1, double* k2, double* a_switch) {
  constexpr double kHypSwitch[] = {1.0, 1.25, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 16.0, 64.0, HUGE_VAL};
  constexpr double kHypProbe[] = {1.0, 1.5, 2.0, 4.0, 16.0};
  constexpr int kHypConnTerms = 100;
  constexpr double kHypMaxLoss = 4096.0;
  const double amb = a - b;
  auto nonpos_int = [](double v, double tol) { return v < 0.5 && fabs(v - nearbyint(v)) < tol; };
  if (nonpos_int(amb, 1e-9) || nonpos_int(b, 1e-6) || nonpos_int(b + 1., 1e-6) || b == a)
    return false;
  *k1 = b / (b - a);
  *k2 = (a <= 0.0 && a == nearbyint(a)) ? 0.0 : hyp_gamma_ratio(b, amb, a);
  if (!std::isfinite(*k1) || !std::isfinite(*k2)) return false;
  for (double sw : kHypSwitch) {
    const bool all = !std::isfinite(sw);
    if (hyp_series_host(a, b, all ? 1.0 : sw / (1.0 + sw)).taken > kHypMaxTerms)
      return false;                                   // a larger switch needs still more terms
    bool ok = true;
    for (int i = 0; ok && !all && i < 5; ++i) {
      const double A = sw * kHypProbe[i];
      const double sa = pow(A / (1.0 + A), a);
      const HypSum c = hyp_series_host(a, amb, 1.0 / (1.0 + A));
      const double t2 = *k2 * pow(A, amb);
      const double tot = sa * *k1 * c.sum + t2;
      const double loss = std::max(fabs(sa * *k1) * c.big, fabs(t2)) / fabs(tot);
      ok = c.taken <= kHypConnTerms && loss <= kHypMaxLoss;      // (false for NaN)
    }
    if (ok) {
      *a_switch = sw;
      return true;
    }
  }
  return false;
}

// K4's host half: rjp_geometry -> the kernel's GeomDev (rotations, SI lengths, the launch-time
// constants and, with `want_ts`, the plan of the 2F1).  Returns RJP_OK, or the status and message
// rjp_build_fields refuses the model with (an x-slab outside the grid; RJP_ERR_DEGENERATE).
int geometry_to_dev(const rjp_geometry* gm, bool want_ts, GeomDev& g, std::string& err) {
  auto refuse = [&](int code, const char* what) {
    err = what;
    return code;
  };
  const double au = 149597870700.0, d2r = M_PI / 180.0;
  g.nx = gm->nx; g.ny = gm->ny; g.nz = gm->nz; g.ccw = gm->rotation_ccw;
  g.nx_total = gm->nx_total > 0 ? gm->nx_total : gm->nx;
  g.ix0 = gm->ix0;
  if (g.ix0 < 0 || g.ix0 + g.nx > g.nx_total)
    return refuse(RJP_ERR_ARG, "rjp_build_fields: x-slab [ix0, ix0+nx) outside [0, nx_total)");
  g.cs = gm->csize;
  // numpy.radians(x) = x * (pi/180); cos/sin in libm double, as maths/geometry.py:249-253
  const double a = (gm->inc - 90.) * d2r, b = gm->pa * d2r;
  g.ca = cos(a); g.sa = sin(a); g.cb = cos(b); g.sb = sin(b);
  const double a2 = (90. - gm->inc) * d2r, b2 = -gm->pa * d2r;
  g.ca2 = cos(a2); g.sa2 = sin(a2); g.cb2 = cos(b2); g.sb2 = sin(b2);
  g.w_0 = gm->w_0; g.r_0 = gm->r_0; g.mr0 = gm->mod_r_0; g.eps = gm->epsilon;
  g.R_1 = gm->R_1; g.R_2 = gm->R_2;
  g.gm = 6.6743e-11 * gm->M_star * 1.98847e30;
  g.v_lsr = gm->v_lsr;
  g.n_0 = gm->n_0; g.x_0 = gm->x_0; g.T_0 = gm->T_0; g.v_0 = gm->v_0;
  g.q_n = gm->q_n; g.q_x = gm->q_x; g.q_T = gm->q_T; g.q_v = gm->q_v;
  g.qd_n = gm->qd_n; g.qd_x = gm->qd_x; g.qd_T = gm->qd_T; g.qd_v = gm->qd_v;
  g.rb_frac = gm->rb_frac;
  {
    // maths/geometry.py:150-156
    const double mr0 = gm->mod_r_0 * au, r0 = gm->r_0 * au, v0 = gm->v_0 * 1e3;
    const double a = gm->qd_v, b = (1. - gm->q_v + gm->epsilon * gm->qd_v) / gm->epsilon;
    g.ts_pow = 1. - gm->q_v;
    g.ts_const = pow(mr0, gm->q_v) / (v0 * (1. - gm->q_v + gm->epsilon * gm->qd_v));
    g.ts_base = g.ts_const * pow(r0 + mr0 - r0, g.ts_pow);
    g.mr0_m = mr0; g.r0_m = r0;
    g.r1_m = gm->R_1 * au; g.r2_m = gm->R_2 * au; g.w0_m = gm->w_0 * au;
    g.hy_a = a; g.hy_b = b;
    g.hy_axis = 1. + gm->qd_v / (1. - gm->q_v);
    g.hy_k1 = g.hy_k2 = 0.0;
    g.ts_mode = want_ts ? 1 : 0;
    g.hy_switch = 1.0;
    if (want_ts && a != 0.0) {
      // the connection formula needs Gamma(a-b) and 1/Gamma(a): logarithmic cases when a - b or
      // b is an integer <= 0.  hyp_plan refuses those and every model whose series would cancel
      // or not end -> the caller evaluates ts itself
      if (!hyp_plan(a, b, &g.hy_k1, &g.hy_k2, &g.hy_switch))
        return refuse(RJP_ERR_DEGENERATE,
                      "rjp_build_fields: degenerate 2F1 parameters (a-b or b at or too close to a "
                      "non-positive integer for the device series); pass d_ts = NULL and upload "
                      "host-computed launch times");
      g.ts_mode = 2;
    }
  }
  return RJP_OK;
}

}  // namespace rjp
