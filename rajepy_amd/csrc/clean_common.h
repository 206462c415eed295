// What the CLEAN kernels share (clean.hip: K12 / K13; msclean.hip: K17; mtmfs.hip: K19): the tile of 1024
// consecutive pixels of a flat image with two pairs of neighbours per thread, the 16-byte pair
// loads and stores, and the (value, pixel) partial maxima with their fixed-order reductions.
#pragma once
#include "rjp_host.h"

namespace rjp {

constexpr int kClB = 256;          // threads per workgroup
constexpr int kClT = 1024;         // pixels per tile: two pairs per thread

// a partial maximum: the value at the pixel and the pixel; pix < 0: no pixel qualifies
struct ClPeak {
  double v;
  int pix;
};

// the larger |v|, on a tie the lower pixel; "none" loses against anything
__device__ __forceinline__ ClPeak cl_better(ClPeak a, ClPeak b) {
  const double aa = __builtin_fabs(a.v), ab = __builtin_fabs(b.v);
  const bool take_b = b.pix >= 0 && (a.pix < 0 || ab > aa || (ab == aa && b.pix < a.pix));
  return take_b ? b : a;
}

// The workgroup's best candidate, in every thread.  (`s_v`, `s_p`: 4 entries each; the order of
// the combination is fixed and cl_better is a total order on distinct pixels, so the result does
// not depend on it anyway.)
__device__ __forceinline__ ClPeak cl_block_best(ClPeak x, double* s_v, int* s_p) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ClPeak y;
    y.v = __shfl_xor(x.v, off);
    y.pix = __shfl_xor(x.pix, off);
    x = cl_better(x, y);
  }
  const int wave = threadIdx.x >> 6;
  __syncthreads();                                  // earlier readers of s_v / s_p are done
  if ((threadIdx.x & 63) == 0) {
    s_v[wave] = x.v;
    s_p[wave] = x.pix;
  }
  __syncthreads();
  ClPeak r;
  r.v = s_v[0];
  r.pix = s_p[0];
#pragma unroll
  for (int w = 1; w < kClB / 64; ++w) {
    ClPeak y;
    y.v = s_v[w];
    y.pix = s_p[w];
    r = cl_better(r, y);
  }
  return r;
}

// a map's peak from its tiles' partials
__device__ __forceinline__ ClPeak cl_map_peak(const double* __restrict__ pv,
                                              const int* __restrict__ pp, int tiles, double* s_v,
                                              int* s_p) {
  ClPeak x;
  x.v = 0.0;
  x.pix = -1;
  for (int i = threadIdx.x; i < tiles; i += kClB) {
    ClPeak y;
    y.v = pv[i];
    y.pix = pp[i];
    x = cl_better(x, y);
  }
  return cl_block_best(x, s_v, s_p);
}

// the pair (p, p + 1) of one map: 16 bytes when `vec` (the map's base is 16-byte aligned; p is
// even) and both lie inside the image
__device__ __forceinline__ void cl_load_pair(const double* __restrict__ r, int64_t p, int64_t npix,
                                             bool vec, double& a, double& b) {
  a = b = 0.0;
  if (vec && p + 1 < npix) {
    const rjp_d2 t = *(const rjp_d2*)(r + p);
    a = t.x;
    b = t.y;
  } else {
    if (p < npix) a = r[p];
    if (p + 1 < npix) b = r[p + 1];
  }
}

__device__ __forceinline__ void cl_store_pair(double* __restrict__ r, int64_t p, int64_t npix,
                                              bool vec, double a, double b) {
  if (vec && p + 1 < npix) {
    rjp_d2 t;
    t.x = a;
    t.y = b;
    *(rjp_d2*)(r + p) = t;
  } else {
    if (p < npix) r[p] = a;
    if (p + 1 < npix) r[p + 1] = b;
  }
}

// the tile's candidate among a thread's four pixels, in pixel order (lower pixels first, so a
// strict > keeps the lowest on a tie)
__device__ __forceinline__ ClPeak cl_thread_best(const double (&r)[4], const int64_t (&p)[4],
                                                 int64_t npix, const uint8_t* __restrict__ mask) {
  ClPeak x;
  x.v = 0.0;
  x.pix = -1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p[j] >= npix || !finite_d(r[j])) continue;
    if (mask && mask[p[j]] == 0) continue;
    if (x.pix < 0 || __builtin_fabs(r[j]) > __builtin_fabs(x.v)) {
      x.v = r[j];
      x.pix = (int)p[j];
    }
  }
  return x;
}

__device__ __forceinline__ void cl_pixels(int tile, int64_t (&p)[4]) {
  const int64_t t0 = (int64_t)tile * kClT + 2 * threadIdx.x;
  p[0] = t0;
  p[1] = t0 + 1;
  p[2] = t0 + kClT / 2;
  p[3] = t0 + kClT / 2 + 1;
}

__device__ __forceinline__ bool cl_vec_ok(const double* rm) { return ((uintptr_t)rm & 15u) == 0; }

}  // namespace rjp
