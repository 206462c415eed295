// K12 (rjp_clean): Hogbom CLEAN minor cycles on a stack of images, and K13 (rjp_restore): the clean
// components convolved with the clean beam, plus the residual.
//
// K12.  Iteration t of map m: among the pixels that are unmasked and hold a finite residual take
// p* with the largest |R[p]| (ties: the lowest p); stop when there is none or |R[p*]| <= thresh[m];
// else f = gain R[p*], the component (p*, f) goes to slot t, model[p*] += f and
//   R[q] = fma(-f, B[q - p* + centre], R[q])        for every q whose beam index lies inside the beam.
// One launch per iteration for the whole stack, grid = tiles x maps; a tile is kClT = 1024
// consecutive pixels of the flat image (p = ix nz + iz), a thread owns two pairs of neighbours,
// (t0 + 2 tid, +1) and (t0 + 512 + 2 tid, +1): a wave's 16-byte access is 1 KiB of consecutive
// memory.  A workgroup of launch t
//   1. reduces the partial maxima (value, pixel) that the previous launch left per tile of its map
//      to the map's peak -- every workgroup redundantly, a few hundred entries from L2, 256 per pass;
//   2. decides "finished" from that peak alone (no flag: a finished map's partials are carried
//      over unchanged, so the next launch decides the same);
//   3. subtracts inside its tile and forms the tile's new partial from the registers it just
//      updated; a tile whose rows the beam window does not reach only carries its partial over;
//   4. writes the partial to the other half of the double-buffered workspace;
//   5. (tile 0 of the map only) records the component, the model pixel and the count.
// clean_init_kernel forms the partials of the dirty image and zeroes the counts; clean_peak_kernel
// reduces the last partials to d_peak.  Workgroups of one launch exchange nothing: what launch t + 1
// reads was written by launch t, and the kernel boundary in the stream is what makes it visible
// (the XCDs' L2s are not coherent inside a launch).  No atomics, every reduction in a fixed order:
// the same bits on every call.
// Residual accesses are 16 bytes where the map's base is 16-byte aligned and the pair lies inside
// the image, else two 8-byte accesses.  The beam is read 8 bytes at a time: pz is odd, so
// successive beam rows alternate between 16-byte aligned and not whatever the component, and a
// 16-byte path would serve half the rows of a wave and diverge on the others; the 64 lanes' 8-byte
// loads are consecutive and still fetch whole lines.
//
// K13.  out[m][q] = add[m][q] + sum_{c < ncomp[m]} f_c exp(-(A dx^2 + 2 B dx dz + C dz^2)), one pixel
// per thread, the components staged through LDS in chunks of 256 as (ix, iz, f) and read by broadcast,
// the sum in list order, exp_any for the Gaussian; a term whose exponent is below -700 is an exact 0.
#include "clean_common.h"

namespace rjp {

constexpr int kRsC = 256;          // components per LDS chunk of K13

// The tile rule (tests restate it on the host): tiles of 1024 consecutive pixels of one map.
CleanTiling clean_tiling(int n_maps, int nx, int nz) {
  CleanTiling t;
  const int64_t npix = (int64_t)nx * nz;
  t.tiles = (npix + kClT - 1) / kClT;
  t.workgroups = t.tiles * n_maps;
  return t;
}

// two halves of (value f64, pixel i32) per map and tile, rounded up to 16 bytes; 0: no size_t holds it
size_t clean_workspace_bytes(int n_maps, int nx, int nz) {
  const CleanTiling t = clean_tiling(n_maps, nx, nz);
  const unsigned __int128 n = (unsigned __int128)t.workgroups * 2u * 12u + 15u;
  return n > (unsigned __int128)SIZE_MAX ? 0 : (size_t)(n / 16u * 16u);
}

// the partials of the dirty image -> half 0 of the workspace; the counts start at 0
__global__ __launch_bounds__(kClB) void clean_init_kernel(const double* __restrict__ res,
                                                          int64_t npix, int tiles,
                                                          const uint8_t* __restrict__ mask,
                                                          double* __restrict__ pv,
                                                          int* __restrict__ pp,
                                                          int* __restrict__ ncomp) {
  __shared__ double s_v[kClB / 64];
  __shared__ int s_p[kClB / 64];
  const int tile = (int)(blockIdx.x % (unsigned)tiles), m = (int)(blockIdx.x / (unsigned)tiles);
  const double* __restrict__ rm = res + (int64_t)m * npix;
  const bool vec = cl_vec_ok(rm);
  int64_t p[4];
  cl_pixels(tile, p);
  double r[4];
  cl_load_pair(rm, p[0], npix, vec, r[0], r[1]);
  cl_load_pair(rm, p[2], npix, vec, r[2], r[3]);
  const ClPeak best = cl_block_best(cl_thread_best(r, p, npix, mask), s_v, s_p);
  if (threadIdx.x == 0) {
    pv[(int64_t)m * tiles + tile] = best.v;
    pp[(int64_t)m * tiles + tile] = best.pix;
    if (tile == 0) ncomp[m] = 0;
  }
}

// iteration `it`: partials (pv_in, pp_in) -> (pv_out, pp_out)
__global__ __launch_bounds__(kClB) void clean_step_kernel(
    double* __restrict__ res, int64_t npix, int nz, int tiles, const double* __restrict__ psf,
    int64_t psf_stride, int px, int pz, const uint8_t* __restrict__ mask,
    const double* __restrict__ thresh, double gain, int it, int n_iter,
    const double* __restrict__ pv_in, const int* __restrict__ pp_in, double* __restrict__ pv_out,
    int* __restrict__ pp_out, int* __restrict__ cpix, double* __restrict__ cflux,
    int* __restrict__ ncomp, double* __restrict__ model) {
  __shared__ double s_v[kClB / 64];
  __shared__ int s_p[kClB / 64];
  const int tile = (int)(blockIdx.x % (unsigned)tiles), m = (int)(blockIdx.x / (unsigned)tiles);
  const int64_t slot = (int64_t)m * tiles + tile;
  const ClPeak peak = cl_map_peak(pv_in + (int64_t)m * tiles, pp_in + (int64_t)m * tiles, tiles,
                                  s_v, s_p);
  // the window's rows against the tile's (the peak, hence every branch below, is workgroup-uniform)
  const bool live = peak.pix >= 0 && __builtin_fabs(peak.v) > thresh[m];
  const int cx = (px - 1) / 2, cz = (pz - 1) / 2;
  const int ixs = live ? peak.pix / nz : 0, izs = live ? peak.pix - ixs * nz : 0;
  const int64_t t0 = (int64_t)tile * kClT, t1 = min(npix, t0 + kClT) - 1;
  // (32-bit divisions: every pixel index here, a tile's tail beyond the image included, is below
  // 2^31 + 1024)
  const bool reached = live && (int)((unsigned)t1 / (unsigned)nz) >= ixs - cx &&
                       (int)((unsigned)t0 / (unsigned)nz) <= ixs + cx;
  if (!reached) {
    if (threadIdx.x == 0) {
      pv_out[slot] = pv_in[slot];
      pp_out[slot] = pp_in[slot];
    }
  } else {
    const double f = gain * peak.v;
    double* __restrict__ rm = res + (int64_t)m * npix;
    const double* __restrict__ bm = psf + (int64_t)m * psf_stride;
    const bool vec = cl_vec_ok(rm);
    int64_t p[4];
    cl_pixels(tile, p);
    double r[4];
    cl_load_pair(rm, p[0], npix, vec, r[0], r[1]);
    cl_load_pair(rm, p[2], npix, vec, r[2], r[3]);
    bool hit = false;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int ix = (int)((unsigned)p[2 * h] / (unsigned)nz);
      int iz = (int)((unsigned)p[2 * h] - (unsigned)ix * (unsigned)nz);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        // (64-bit: an index plus half a beam of up to 2^31 - 1 rows passes 2^31)
        const int64_t bx = (int64_t)ix - ixs + cx, bz = (int64_t)iz - izs + cz;
        if (p[2 * h + j] < npix && bx >= 0 && bx < px && bz >= 0 && bz < pz &&
            finite_d(r[2 * h + j])) {
          r[2 * h + j] = __builtin_fma(-f, bm[bx * pz + bz], r[2 * h + j]);
          hit = true;
        }
        if (++iz == nz) {
          iz = 0;
          ++ix;
        }
      }
    }
    // (a pair nobody of it changed is not written back)
    if (hit) {
      cl_store_pair(rm, p[0], npix, vec, r[0], r[1]);
      cl_store_pair(rm, p[2], npix, vec, r[2], r[3]);
    }
    const ClPeak best = cl_block_best(cl_thread_best(r, p, npix, mask), s_v, s_p);
    if (threadIdx.x == 0) {
      pv_out[slot] = best.v;
      pp_out[slot] = best.pix;
    }
  }
  if (live && tile == 0 && threadIdx.x == 0) {
    const double f = gain * peak.v;
    cpix[(int64_t)m * n_iter + it] = peak.pix;
    cflux[(int64_t)m * n_iter + it] = f;
    ncomp[m] = it + 1;
    if (model) model[(int64_t)m * npix + peak.pix] += f;
  }
}

// d_peak[m] = the final masked max |R|, 0 when no pixel qualifies
__global__ __launch_bounds__(kClB) void clean_peak_kernel(const double* __restrict__ pv,
                                                          const int* __restrict__ pp, int tiles,
                                                          double* __restrict__ peak) {
  __shared__ double s_v[kClB / 64];
  __shared__ int s_p[kClB / 64];
  const int m = blockIdx.x;
  const ClPeak x = cl_map_peak(pv + (int64_t)m * tiles, pp + (int64_t)m * tiles, tiles, s_v, s_p);
  if (threadIdx.x == 0) peak[m] = x.pix >= 0 ? __builtin_fabs(x.v) : 0.0;
}

hipError_t clean_launch(double* res, int n_maps, int nx, int nz, const double* psf, int n_psf,
                        int px, int pz, const uint8_t* mask, const double* d_thresh, double gain,
                        int n_iter, int32_t* cpix, double* cflux, int32_t* ncomp, double* model,
                        double* peak, void* work, hipStream_t st) {
  const CleanTiling t = clean_tiling(n_maps, nx, nz);
  const int tiles = (int)t.tiles;
  const unsigned nb = (unsigned)t.workgroups;
  const int64_t npix = (int64_t)nx * nz, half = t.workgroups;
  // workspace: values [2][n_maps][tiles] f64, then pixels [2][n_maps][tiles] i32
  double* pv = (double*)work;
  int* pp = (int*)(pv + 2 * half);
  const int64_t psf_stride = n_psf == 1 ? 0 : (int64_t)px * pz;
  hipLaunchKernelGGL(clean_init_kernel, dim3(nb), dim3(kClB), 0, st, res, npix, tiles, mask, pv, pp,
                     ncomp);
  hipError_t err = hipGetLastError();
  for (int it = 0; it < n_iter && err == hipSuccess; ++it) {
    const int64_t in = (it & 1) * half, out = ((it + 1) & 1) * half;
    hipLaunchKernelGGL(clean_step_kernel, dim3(nb), dim3(kClB), 0, st, res, npix, nz, tiles, psf,
                       psf_stride, px, pz, mask, d_thresh, gain, it, n_iter, pv + in, pp + in,
                       pv + out, pp + out, cpix, cflux, ncomp, model);
    err = hipGetLastError();
  }
  if (err != hipSuccess || !peak) return err;
  const int64_t last = (n_iter & 1) * half;
  hipLaunchKernelGGL(clean_peak_kernel, dim3((unsigned)n_maps), dim3(kClB), 0, st, pv + last,
                     pp + last, tiles, peak);
  return hipGetLastError();
}

// ---- K13 ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kClB) void restore_kernel(
    const int* __restrict__ cpix, const double* __restrict__ cflux, const int* __restrict__ ncomp,
    int comp_stride, const double* __restrict__ beam, const double* __restrict__ add, int nz,
    int64_t npix, int tiles, double* __restrict__ out) {
  __shared__ int s_x[kRsC], s_z[kRsC];
  __shared__ double s_f[kRsC];
  const int tile = (int)(blockIdx.x % (unsigned)tiles), m = (int)(blockIdx.x / (unsigned)tiles);
  const int64_t q = (int64_t)tile * kClB + threadIdx.x;
  // (32-bit: q < 2^31 + 256)
  const int qx = (int)((unsigned)q / (unsigned)nz), qz = (int)((unsigned)q - (unsigned)qx * (unsigned)nz);
  const double A = beam[3 * m], B2 = 2.0 * beam[3 * m + 1], Cq = beam[3 * m + 2];
  const int n = min(max(ncomp[m], 0), comp_stride);
  const int* __restrict__ cp = cpix + (int64_t)m * comp_stride;
  const double* __restrict__ cf = cflux + (int64_t)m * comp_stride;
  double acc = 0.0;
  for (int c0 = 0; c0 < n; c0 += kRsC) {
    __syncthreads();                                // the previous chunk's readers are done
    const int c = c0 + threadIdx.x;
    if (c < n) {
      const int p = cp[c];
      s_x[threadIdx.x] = p / nz;
      s_z[threadIdx.x] = p - (p / nz) * nz;
      s_f[threadIdx.x] = cf[c];
    }
    __syncthreads();
    const int nc = min(kRsC, n - c0);
    for (int k = 0; k < nc; ++k) {
      const double dx = (double)(qx - s_x[k]), dz = (double)(qz - s_z[k]);
      const double e = -(A * (dx * dx) + B2 * (dx * dz) + Cq * (dz * dz));
      // (e is never positive: the form is positive definite; NaN compares false -> exp_any)
      const double g = e < -700.0 ? 0.0 : exp_any(e);
      acc = __builtin_fma(s_f[k], g, acc);
    }
  }
  if (q < npix) out[(int64_t)m * npix + q] = add ? add[(int64_t)m * npix + q] + acc : acc;
}

int64_t restore_workgroups(int n_maps, int nx, int nz) {
  return (((int64_t)nx * nz + kClB - 1) / kClB) * n_maps;
}

hipError_t restore_launch(const int32_t* cpix, const double* cflux, const int32_t* ncomp,
                          int n_maps, int comp_stride, const double* d_beam, const double* add,
                          int nx, int nz, double* out, hipStream_t st) {
  const int64_t npix = (int64_t)nx * nz;
  const int tiles = (int)((npix + kClB - 1) / kClB);
  hipLaunchKernelGGL(restore_kernel, dim3((unsigned)restore_workgroups(n_maps, nx, nz)), dim3(kClB),
                     0, st, cpix, cflux, ncomp, comp_stride, d_beam, add, nz, npix, tiles, out);
  return hipGetLastError();
}

}  // namespace rjp
