// K19 (rjp_mtmfs): multi-term multi-frequency-synthesis CLEAN minor cycles on a stack of maps --
// K12 (clean.hip) generalised from one residual plane per map to n_t Taylor planes R_0 .. R_{n_t-1}
// that are coupled through a small Hessian, with the spectral beams B_0 .. B_{2 n_t - 2}.
//
// Iteration i of map m: among the pixels that are unmasked and finite in ALL n_t planes, with
//   a_q(p) = Hinv[q][0] R_0[p], then a_q = fma(Hinv[q][t], R_t[p], a_q) for t = 1 .. n_t - 1,
// p* is the pixel with the largest |a_0(p)| (ties: the lowest p); stop when there is none or
// |a_0(p*)| <= thresh[m]; else c_q = gain a_q(p*) (one product), the component (p*, c_0 .. c_{n_t-1})
// goes to slot i, model[m][t][p*] += c_t and for every plane t
//   R_t[x] = fma(-c_q, B_{t+q}[x - p* + centre], R_t[x])   for q = 0 .. n_t - 1 ascending,
// for every x inside the beam window that is finite in plane t.
// K12's launch shape: one launch per iteration for the whole stack, grid = tiles x maps, a tile =
// kClT = 1024 consecutive pixels (clean_common.h); ONE workgroup holds all n_t planes of its tile in
// registers (a_0 needs every plane at a pixel), the kernels are templated on NT = 1 .. 4.  A tile's
// partial is (pixel, R_0[pixel] .. R_{NT-1}[pixel]): the coefficients need every plane's value at
// p*, and reading those from d_res inside the step launch would race with the workgroup that owns
// p* and is updating it.  Every workgroup of launch i + 1 recomputes a_0 of every partial and a_q
// of the winner with the same chain: the same bits everywhere.  Workgroups of one launch exchange
// nothing (the kernel boundary makes the previous launch's partials visible: see clean.hip), no
// atomics, every reduction in a fixed order: the same bits on every call.
// Plane bases are npix doubles apart: with an odd npix every other plane is 8 bytes off a 16-byte
// boundary, so the 16-byte path is decided per plane.  With NT = 1, Hinv = 1.0 and a beam of
// centre 1.0, a_0 = R and c_0 = gain R exactly: every output equals rjp_clean's bit for bit.
#include "clean_common.h"

namespace rjp {

MtmfsTiling mtmfs_tiling(int n_maps, int nx, int nz) {
  MtmfsTiling t;
  const int64_t npix = (int64_t)nx * nz;
  t.tiles = (npix + kClT - 1) / kClT;
  t.workgroups = t.tiles * n_maps;
  return t;
}

// two halves of (n_t values f64, pixel i32) per map and tile, rounded up to 16 bytes; 0: no size_t
// holds it
size_t mtmfs_workspace_bytes(int n_maps, int n_t, int nx, int nz) {
  const MtmfsTiling t = mtmfs_tiling(n_maps, nx, nz);
  const unsigned __int128 n =
      (unsigned __int128)t.workgroups * 2u * (8u * (unsigned)n_t + 4u) + 15u;
  return n > (unsigned __int128)SIZE_MAX ? 0 : (size_t)(n / 16u * 16u);
}

// a_q from row q of Hinv and the planes' values at one pixel: one product, then NT - 1 fmas
template <int NT>
__device__ __forceinline__ double mt_solve(const double (&h)[NT], const double (&r)[NT]) {
  double a = h[0] * r[0];
#pragma unroll
  for (int t = 1; t < NT; ++t) a = __builtin_fma(h[t], r[t], a);
  return a;
}

// a map's peak (a_0, pixel) from its tiles' partials (pv: [tiles][NT], pp: [tiles])
template <int NT>
__device__ __forceinline__ ClPeak mt_map_peak(const double* __restrict__ pv,
                                              const int* __restrict__ pp, int tiles,
                                              const double (&h0)[NT], double* s_v, int* s_p) {
  ClPeak x;
  x.v = 0.0;
  x.pix = -1;
  for (int i = threadIdx.x; i < tiles; i += kClB) {
    double r[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) r[t] = pv[(int64_t)i * NT + t];
    ClPeak y;
    y.v = mt_solve<NT>(h0, r);
    y.pix = pp[i];
    x = cl_better(x, y);
  }
  return cl_block_best(x, s_v, s_p);
}

// The tile's candidate among a thread's four pixels, in pixel order (a strict > keeps the lowest
// on a tie), then the workgroup's; the owner of the winner writes the partial from its registers.
template <int NT>
__device__ __forceinline__ void mt_tile_partial(const double (&r)[NT][4], const int64_t (&p)[4],
                                                int64_t npix, const uint8_t* __restrict__ mask,
                                                const double (&h0)[NT], double* s_v, int* s_p,
                                                double* __restrict__ pv_slot,
                                                int* __restrict__ pp_slot) {
  ClPeak x;
  x.v = 0.0;
  x.pix = -1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p[j] >= npix) continue;
    bool fin = true;
    double rj[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      rj[t] = r[t][j];
      fin = fin && finite_d(rj[t]);
    }
    if (!fin) continue;
    if (mask && mask[p[j]] == 0) continue;
    const double a0 = mt_solve<NT>(h0, rj);
    if (x.pix < 0 || __builtin_fabs(a0) > __builtin_fabs(x.v)) {
      x.v = a0;
      x.pix = (int)p[j];
    }
  }
  const ClPeak best = cl_block_best(x, s_v, s_p);
  if (best.pix < 0) {
    if (threadIdx.x == 0) {
      *pp_slot = -1;
#pragma unroll
      for (int t = 0; t < NT; ++t) pv_slot[t] = 0.0;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p[j] == (int64_t)best.pix) {
      *pp_slot = best.pix;
#pragma unroll
      for (int t = 0; t < NT; ++t) pv_slot[t] = r[t][j];
    }
  }
}

template <int NT>
__device__ __forceinline__ void mt_load(const double* __restrict__ rm, int64_t npix,
                                        const int64_t (&p)[4], double (&r)[NT][4]) {
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const double* __restrict__ rt = rm + (int64_t)t * npix;
    const bool vec = cl_vec_ok(rt);
    cl_load_pair(rt, p[0], npix, vec, r[t][0], r[t][1]);
    cl_load_pair(rt, p[2], npix, vec, r[t][2], r[t][3]);
  }
}

// the partials of the planes on entry -> half 0 of the workspace; the counts start at 0
template <int NT>
__global__ __launch_bounds__(kClB) void mtmfs_init_kernel(const double* __restrict__ res,
                                                          int64_t npix, int tiles,
                                                          const double* __restrict__ hinv,
                                                          const uint8_t* __restrict__ mask,
                                                          double* __restrict__ pv,
                                                          int* __restrict__ pp,
                                                          int* __restrict__ ncomp) {
  __shared__ double s_v[kClB / 64];
  __shared__ int s_p[kClB / 64];
  const int tile = (int)(blockIdx.x % (unsigned)tiles), m = (int)(blockIdx.x / (unsigned)tiles);
  const int64_t slot = (int64_t)m * tiles + tile;
  double h0[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) h0[t] = hinv[(int64_t)m * NT * NT + t];
  int64_t p[4];
  cl_pixels(tile, p);
  double r[NT][4];
  mt_load<NT>(res + (int64_t)m * NT * npix, npix, p, r);
  mt_tile_partial<NT>(r, p, npix, mask, h0, s_v, s_p, pv + slot * NT, pp + slot);
  if (tile == 0 && threadIdx.x == 0) ncomp[m] = 0;
}

// iteration `it`: partials (pv_in, pp_in) -> (pv_out, pp_out)
template <int NT>
__global__ __launch_bounds__(kClB) void mtmfs_step_kernel(
    double* __restrict__ res, int64_t npix, int nz, int tiles, const double* __restrict__ spsf,
    int64_t psf_stride, int px, int pz, const double* __restrict__ hinv,
    const uint8_t* __restrict__ mask, const double* __restrict__ thresh, double gain, int it,
    int n_iter, const double* __restrict__ pv_in, const int* __restrict__ pp_in,
    double* __restrict__ pv_out, int* __restrict__ pp_out, int* __restrict__ cpix,
    double* __restrict__ ccoef, int* __restrict__ ncomp, double* __restrict__ model) {
  __shared__ double s_v[kClB / 64];
  __shared__ int s_p[kClB / 64];
  const int tile = (int)(blockIdx.x % (unsigned)tiles), m = (int)(blockIdx.x / (unsigned)tiles);
  const int64_t map0 = (int64_t)m * tiles, slot = map0 + tile;
  const double* __restrict__ hm = hinv + (int64_t)m * NT * NT;
  double h0[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) h0[t] = hm[t];
  const ClPeak peak = mt_map_peak<NT>(pv_in + map0 * NT, pp_in + map0, tiles, h0, s_v, s_p);
  // the window's rows against the tile's (the peak, hence every branch below, is workgroup-uniform)
  const bool live = peak.pix >= 0 && __builtin_fabs(peak.v) > thresh[m];
  const int cx = (px - 1) / 2, cz = (pz - 1) / 2;
  const int ixs = live ? peak.pix / nz : 0, izs = live ? peak.pix - ixs * nz : 0;
  const int64_t t0 = (int64_t)tile * kClT, t1 = min(npix, t0 + kClT) - 1;
  // (32-bit divisions: every pixel index here, a tile's tail beyond the image included, is below
  // 2^31 + 1024)
  const bool reached = live && (int)((unsigned)t1 / (unsigned)nz) >= ixs - cx &&
                       (int)((unsigned)t0 / (unsigned)nz) <= ixs + cx;
  // the coefficients, from the winning tile's partial: the planes' values at p* as the previous
  // launch left them (c[0] = gain peak.v to the bit: the same chain on the same values)
  double c[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) c[q] = 0.0;
  if (live) {
    const int64_t win = map0 + peak.pix / kClT;
    double rp[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) rp[t] = pv_in[win * NT + t];
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      double hq[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) hq[t] = hm[q * NT + t];
      c[q] = gain * mt_solve<NT>(hq, rp);
    }
  }
  if (!reached) {
    if (threadIdx.x == 0) {
      pp_out[slot] = pp_in[slot];
#pragma unroll
      for (int t = 0; t < NT; ++t) pv_out[slot * NT + t] = pv_in[slot * NT + t];
    }
  } else {
    double* __restrict__ rm = res + (int64_t)m * NT * npix;
    const double* __restrict__ bm = spsf + (int64_t)m * psf_stride;
    const int64_t bpix = (int64_t)px * pz;
    int64_t p[4];
    cl_pixels(tile, p);
    double r[NT][4];
    mt_load<NT>(rm, npix, p, r);
    bool hit = false;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int ix = (int)((unsigned)p[2 * h] / (unsigned)nz);
      int iz = (int)((unsigned)p[2 * h] - (unsigned)ix * (unsigned)nz);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        // (64-bit: an index plus half a beam of up to 2^31 - 1 rows passes 2^31)
        const int64_t bx = (int64_t)ix - ixs + cx, bz = (int64_t)iz - izs + cz;
        if (p[2 * h + j] < npix && bx >= 0 && bx < px && bz >= 0 && bz < pz) {
          double b[2 * NT - 1];
#pragma unroll
          for (int s = 0; s < 2 * NT - 1; ++s) b[s] = bm[s * bpix + bx * pz + bz];
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            if (finite_d(r[t][2 * h + j])) {
#pragma unroll
              for (int q = 0; q < NT; ++q)
                r[t][2 * h + j] = __builtin_fma(-c[q], b[t + q], r[t][2 * h + j]);
              hit = true;
            }
          }
        }
        if (++iz == nz) {
          iz = 0;
          ++ix;
        }
      }
    }
    // (a thread that changed nothing writes nothing back)
    if (hit) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        double* __restrict__ rt = rm + (int64_t)t * npix;
        const bool vec = cl_vec_ok(rt);
        cl_store_pair(rt, p[0], npix, vec, r[t][0], r[t][1]);
        cl_store_pair(rt, p[2], npix, vec, r[t][2], r[t][3]);
      }
    }
    mt_tile_partial<NT>(r, p, npix, mask, h0, s_v, s_p, pv_out + slot * NT, pp_out + slot);
  }
  if (live && tile == 0 && threadIdx.x == 0) {
    cpix[(int64_t)m * n_iter + it] = peak.pix;
    ncomp[m] = it + 1;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      ccoef[((int64_t)m * n_iter + it) * NT + t] = c[t];
      if (model) model[((int64_t)m * NT + t) * npix + peak.pix] += c[t];
    }
  }
}

// d_peak[m] = the final masked max |a_0|, 0 when no pixel qualifies
template <int NT>
__global__ __launch_bounds__(kClB) void mtmfs_peak_kernel(const double* __restrict__ pv,
                                                          const int* __restrict__ pp, int tiles,
                                                          const double* __restrict__ hinv,
                                                          double* __restrict__ peak) {
  __shared__ double s_v[kClB / 64];
  __shared__ int s_p[kClB / 64];
  const int m = blockIdx.x;
  double h0[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) h0[t] = hinv[(int64_t)m * NT * NT + t];
  const ClPeak x =
      mt_map_peak<NT>(pv + (int64_t)m * tiles * NT, pp + (int64_t)m * tiles, tiles, h0, s_v, s_p);
  if (threadIdx.x == 0) peak[m] = x.pix >= 0 ? __builtin_fabs(x.v) : 0.0;
}

template <int NT>
static hipError_t mtmfs_launch_nt(double* res, int n_maps, int nx, int nz, const double* spsf,
                                  int n_psf, int px, int pz, const double* d_hinv,
                                  const uint8_t* mask, const double* d_thresh, double gain,
                                  int n_iter, int32_t* cpix, double* ccoef, int32_t* ncomp,
                                  double* model, double* peak, void* work, hipStream_t st) {
  const MtmfsTiling t = mtmfs_tiling(n_maps, nx, nz);
  const int tiles = (int)t.tiles;
  const unsigned nb = (unsigned)t.workgroups;
  const int64_t npix = (int64_t)nx * nz, half = t.workgroups;
  // workspace: values [2][n_maps][tiles][NT] f64, then pixels [2][n_maps][tiles] i32
  double* pv = (double*)work;
  int* pp = (int*)(pv + 2 * half * NT);
  const int64_t psf_stride = n_psf == 1 ? 0 : (int64_t)px * pz * (2 * NT - 1);
  hipLaunchKernelGGL(mtmfs_init_kernel<NT>, dim3(nb), dim3(kClB), 0, st, res, npix, tiles, d_hinv,
                     mask, pv, pp, ncomp);
  hipError_t err = hipGetLastError();
  for (int it = 0; it < n_iter && err == hipSuccess; ++it) {
    const int64_t in = (it & 1) * half, out = ((it + 1) & 1) * half;
    hipLaunchKernelGGL(mtmfs_step_kernel<NT>, dim3(nb), dim3(kClB), 0, st, res, npix, nz, tiles,
                       spsf, psf_stride, px, pz, d_hinv, mask, d_thresh, gain, it, n_iter,
                       pv + in * NT, pp + in, pv + out * NT, pp + out, cpix, ccoef, ncomp, model);
    err = hipGetLastError();
  }
  if (err != hipSuccess || !peak) return err;
  const int64_t last = (n_iter & 1) * half;
  hipLaunchKernelGGL(mtmfs_peak_kernel<NT>, dim3((unsigned)n_maps), dim3(kClB), 0, st,
                     pv + last * NT, pp + last, tiles, d_hinv, peak);
  return hipGetLastError();
}

hipError_t mtmfs_launch(double* res, int n_maps, int n_t, int nx, int nz, const double* spsf,
                        int n_psf, int px, int pz, const double* d_hinv, const uint8_t* mask,
                        const double* d_thresh, double gain, int n_iter, int32_t* cpix,
                        double* ccoef, int32_t* ncomp, double* model, double* peak, void* work,
                        hipStream_t st) {
#define RJP_MTMFS_CASE(NT)                                                                       \
  case NT:                                                                                       \
    return mtmfs_launch_nt<NT>(res, n_maps, nx, nz, spsf, n_psf, px, pz, d_hinv, mask, d_thresh, \
                               gain, n_iter, cpix, ccoef, ncomp, model, peak, work, st)
  switch (n_t) {
    RJP_MTMFS_CASE(1);
    RJP_MTMFS_CASE(2);
    RJP_MTMFS_CASE(3);
    RJP_MTMFS_CASE(4);
  }
#undef RJP_MTMFS_CASE
  return hipErrorInvalidValue;                      // (rjp_mtmfs refused it before)
}

}  // namespace rjp
