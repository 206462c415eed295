// K17 (rjp_msclean): multi-scale CLEAN minor cycles on a stack of maps -- K12 (clean.hip) generalised
// from one residual plane per map to n_s planes R_0 .. R_{n_s - 1} (the dirty image convolved with
// each scale kernel) and the cross beams X[k][l] (the beam convolved with scale k and scale l),
// k <= l, as a packed upper triangle: plane t(k, l) = k n_s - k (k - 1) / 2 + (l - k).
//
// Iteration t of map m: among the planes with weight > 0 and the pixels that are unmasked and hold
// a finite R_k[p], the score is s = weight[k] |R_k[p]| (one rounding); the largest s wins, on a tie
// the lower k, then the lower p; stop when there is none or s* <= thresh[m]; else
//   f = (gain R_k*[p*]) / X[k*][k*][centre],
// the component (p*, k*, f) goes to slot t, model[m][k*][p*] += f and for EVERY plane l
//   R_l[q] = fma(-f, X[k*][l][q - p* + centre], R_l[q])     for q inside the beam window.
// K12's launch shape: one launch per iteration for the whole stack, grid = tiles x planes x maps,
// a tile = kClT = 1024 consecutive pixels of one plane (clean_common.h).  A workgroup of launch t
// reduces the n_s x tiles partials (value, pixel) that the previous launch left for its map --
// every workgroup redundantly, 256 per pass, scores recomputed from the values -- decides
// "finished" from that peak alone, subtracts inside its tile of its plane, forms the tile's new
// partial BY SCORE from the registers it just updated and writes it to the other half of the
// double-buffered workspace; tile 0 of plane 0 records the component.  A plane of weight 0 is
// updated but its partials are "none".  A map whose X[k][k][centre] is zero or not finite for some
// k of weight > 0 gets "none" partials from msclean_init_kernel: finished from the start, ncomp 0.
// Workgroups of one launch exchange nothing (the kernel boundary makes the previous launch's
// partials visible: see clean.hip), no atomics, every reduction in a fixed order: the same bits on
// every call.  With n_s = 1, weight 1 and a beam of centre 1.0, s = |R| and f = gain R exactly:
// every output equals rjp_clean's bit for bit.
#include "clean_common.h"

namespace rjp {

MsCleanTiling msclean_tiling(int n_maps, int n_s, int nx, int nz) {
  MsCleanTiling t;
  const int64_t npix = (int64_t)nx * nz;
  t.tiles = (npix + kClT - 1) / kClT;
  const unsigned __int128 wg = (unsigned __int128)t.tiles * (unsigned)n_s * (unsigned)n_maps;
  t.workgroups = wg > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)wg;
  return t;
}

// two halves of (value f64, pixel i32) per map, plane and tile, rounded up to 16 bytes; 0: no
// size_t holds it
size_t msclean_workspace_bytes(int n_maps, int n_s, int nx, int nz) {
  const MsCleanTiling t = msclean_tiling(n_maps, n_s, nx, nz);
  if (t.workgroups == INT64_MAX) return 0;
  const unsigned __int128 n = (unsigned __int128)t.workgroups * 2u * 12u + 15u;
  return n > (unsigned __int128)SIZE_MAX ? 0 : (size_t)(n / 16u * 16u);
}

// a candidate: the score, the value at the pixel, the pixel and the plane; pix < 0: none
struct MsPeak {
  double s, v;
  int pix, k;
};

// the larger score, on a tie the lower plane, then the lower pixel; "none" loses against anything
__device__ __forceinline__ MsPeak ms_better(MsPeak a, MsPeak b) {
  const bool take_b =
      b.pix >= 0 && (a.pix < 0 || b.s > a.s ||
                     (b.s == a.s && (b.k < a.k || (b.k == a.k && b.pix < a.pix))));
  // (field by field: a select of the whole struct goes through scratch memory)
  MsPeak r;
  r.s = take_b ? b.s : a.s;
  r.v = take_b ? b.v : a.v;
  r.pix = take_b ? b.pix : a.pix;
  r.k = take_b ? b.k : a.k;
  return r;
}

// The workgroup's best candidate, in every thread (`s_d`: 8 doubles, `s_i`: 8 ints; ms_better is a
// total order on distinct (plane, pixel), so the result does not depend on the combination's order,
// which is fixed anyway).
__device__ __forceinline__ MsPeak ms_block_best(MsPeak x, double* s_d, int* s_i) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    MsPeak y;
    y.s = __shfl_xor(x.s, off);
    y.v = __shfl_xor(x.v, off);
    y.pix = __shfl_xor(x.pix, off);
    y.k = __shfl_xor(x.k, off);
    x = ms_better(x, y);
  }
  const int wave = threadIdx.x >> 6;
  __syncthreads();                                  // earlier readers of s_d / s_i are done
  if ((threadIdx.x & 63) == 0) {
    s_d[2 * wave] = x.s;
    s_d[2 * wave + 1] = x.v;
    s_i[2 * wave] = x.pix;
    s_i[2 * wave + 1] = x.k;
  }
  __syncthreads();
  MsPeak r;
  r.s = s_d[0], r.v = s_d[1], r.pix = s_i[0], r.k = s_i[1];
#pragma unroll
  for (int w = 1; w < kClB / 64; ++w) {
    MsPeak y;
    y.s = s_d[2 * w], y.v = s_d[2 * w + 1], y.pix = s_i[2 * w], y.k = s_i[2 * w + 1];
    r = ms_better(r, y);
  }
  return r;
}

__device__ __forceinline__ MsPeak ms_none() {
  MsPeak x;
  x.s = 0.0, x.v = 0.0, x.pix = -1, x.k = 0;
  return x;
}

// a map's peak from the partials of its n_s x tiles tiles (pv / pp: the map's rows)
__device__ __forceinline__ MsPeak ms_map_peak(const double* __restrict__ pv,
                                              const int* __restrict__ pp, int n_s, int tiles,
                                              const double* __restrict__ wm, double* s_d,
                                              int* s_i) {
  MsPeak x = ms_none();
  int k = (int)(threadIdx.x / (unsigned)tiles), i = (int)(threadIdx.x % (unsigned)tiles);
  const int dk = kClB / tiles, di = kClB % tiles;
  // (entry e = k tiles + i, e = tid, tid + 256, ...; k and i advance without a division per pass)
  for (int64_t e = threadIdx.x; e < (int64_t)n_s * tiles; e += kClB) {
    MsPeak y;
    y.v = pv[e];
    y.pix = pp[e];
    y.k = k;
    y.s = wm[k] * __builtin_fabs(y.v);
    x = ms_better(x, y);
    k += dk;
    i += di;
    if (i >= tiles) {
      i -= tiles;
      ++k;
    }
  }
  return ms_block_best(x, s_d, s_i);
}

// the tile's candidate of plane k (weight w > 0) among a thread's four pixels, in pixel order: a
// strict > keeps the lowest pixel on a tie of the SCORE
__device__ __forceinline__ MsPeak ms_thread_best(const double (&r)[4], const int64_t (&p)[4],
                                                 int64_t npix, const uint8_t* __restrict__ mask,
                                                 double w, int k) {
  MsPeak x = ms_none();
  x.k = k;
  if (!(w > 0.0)) return x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (p[j] >= npix || !finite_d(r[j])) continue;
    if (mask && mask[p[j]] == 0) continue;
    const double s = w * __builtin_fabs(r[j]);
    if (x.pix < 0 || s > x.s) {
      x.s = s;
      x.v = r[j];
      x.pix = (int)p[j];
    }
  }
  return x;
}

__device__ __forceinline__ int64_t ms_tri(int k, int l, int n_s) {
  const int a = min(k, l), b = max(k, l);
  return (int64_t)a * n_s - (int64_t)a * (a - 1) / 2 + (b - a);
}

// blockIdx.x -> (tile, plane, map)
__device__ __forceinline__ void ms_ids(int tiles, int n_s, int& tile, int& l, int& m) {
  const unsigned id = blockIdx.x;
  tile = (int)(id % (unsigned)tiles);
  const unsigned r = id / (unsigned)tiles;
  l = (int)(r % (unsigned)n_s);
  m = (int)(r / (unsigned)n_s);
}

// the partials of the planes on entry -> half 0 of the workspace; the counts start at 0
__global__ __launch_bounds__(kClB) void msclean_init_kernel(
    const double* __restrict__ res, int64_t npix, int n_s, int tiles,
    const double* __restrict__ xpsf, int64_t psf_stride, int64_t bpix, int64_t centre,
    const double* __restrict__ weight, const uint8_t* __restrict__ mask, double* __restrict__ pv,
    int* __restrict__ pp, int* __restrict__ ncomp) {
  __shared__ double s_d[2 * kClB / 64];
  __shared__ int s_i[2 * kClB / 64];
  int tile, l, m;
  ms_ids(tiles, n_s, tile, l, m);
  const double* __restrict__ wm = weight + (int64_t)m * n_s;
  const double* __restrict__ xm = xpsf + (int64_t)m * psf_stride;
  bool dead = false;                                // (workgroup-uniform)
  for (int k = 0; k < n_s; ++k) {
    const double d = xm[ms_tri(k, k, n_s) * bpix + centre];
    dead = dead || (wm[k] > 0.0 && (d == 0.0 || !finite_d(d)));
  }
  const double* __restrict__ rm = res + ((int64_t)m * n_s + l) * npix;
  const bool vec = cl_vec_ok(rm);
  int64_t p[4];
  cl_pixels(tile, p);
  double r[4];
  cl_load_pair(rm, p[0], npix, vec, r[0], r[1]);
  cl_load_pair(rm, p[2], npix, vec, r[2], r[3]);
  const MsPeak best =
      ms_block_best(ms_thread_best(r, p, npix, mask, dead ? 0.0 : wm[l], l), s_d, s_i);
  if (threadIdx.x == 0) {
    const int64_t slot = ((int64_t)m * n_s + l) * tiles + tile;
    pv[slot] = best.v;
    pp[slot] = best.pix;
    if (tile == 0 && l == 0) ncomp[m] = 0;
  }
}

// iteration `it`: partials (pv_in, pp_in) -> (pv_out, pp_out)
__global__ __launch_bounds__(kClB) void msclean_step_kernel(
    double* __restrict__ res, int64_t npix, int nz, int n_s, int tiles,
    const double* __restrict__ xpsf, int64_t psf_stride, int px, int pz,
    const double* __restrict__ weight, const uint8_t* __restrict__ mask,
    const double* __restrict__ thresh, double gain, int it, int n_iter,
    const double* __restrict__ pv_in, const int* __restrict__ pp_in, double* __restrict__ pv_out,
    int* __restrict__ pp_out, int* __restrict__ cpix, int* __restrict__ cscale,
    double* __restrict__ cflux, int* __restrict__ ncomp, double* __restrict__ model) {
  __shared__ double s_d[2 * kClB / 64];
  __shared__ int s_i[2 * kClB / 64];
  int tile, l, m;
  ms_ids(tiles, n_s, tile, l, m);
  const int64_t map0 = (int64_t)m * n_s * tiles, slot = map0 + (int64_t)l * tiles + tile;
  const double* __restrict__ wm = weight + (int64_t)m * n_s;
  const MsPeak peak = ms_map_peak(pv_in + map0, pp_in + map0, n_s, tiles, wm, s_d, s_i);
  // the window's rows against the tile's (the peak, hence every branch below, is workgroup-uniform)
  const bool live = peak.pix >= 0 && peak.s > thresh[m];
  const int cx = (px - 1) / 2, cz = (pz - 1) / 2;
  const int64_t bpix = (int64_t)px * pz;
  const int ixs = live ? peak.pix / nz : 0, izs = live ? peak.pix - ixs * nz : 0;
  const int64_t t0 = (int64_t)tile * kClT, t1 = min(npix, t0 + kClT) - 1;
  const bool reached = live && (int)((unsigned)t1 / (unsigned)nz) >= ixs - cx &&
                       (int)((unsigned)t0 / (unsigned)nz) <= ixs + cx;
  const double* __restrict__ xm = xpsf + (int64_t)m * psf_stride;
  // (one product and one division, both correctly rounded; the diagonal's centre is finite and not
  // zero: msclean_init_kernel left no candidate otherwise)
  const double f =
      live ? (gain * peak.v) / xm[ms_tri(peak.k, peak.k, n_s) * bpix + (int64_t)cx * pz + cz] : 0.0;
  if (!reached) {
    if (threadIdx.x == 0) {
      pv_out[slot] = pv_in[slot];
      pp_out[slot] = pp_in[slot];
    }
  } else {
    double* __restrict__ rm = res + ((int64_t)m * n_s + l) * npix;
    const double* __restrict__ bm = xm + ms_tri(peak.k, l, n_s) * bpix;
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
    const MsPeak best = ms_block_best(ms_thread_best(r, p, npix, mask, wm[l], l), s_d, s_i);
    if (threadIdx.x == 0) {
      pv_out[slot] = best.v;
      pp_out[slot] = best.pix;
    }
  }
  if (live && tile == 0 && l == 0 && threadIdx.x == 0) {
    cpix[(int64_t)m * n_iter + it] = peak.pix;
    cscale[(int64_t)m * n_iter + it] = peak.k;
    cflux[(int64_t)m * n_iter + it] = f;
    ncomp[m] = it + 1;
    if (model) model[((int64_t)m * n_s + peak.k) * npix + peak.pix] += f;
  }
}

// d_peak[m] = the final best score, 0 when no pixel qualifies
__global__ __launch_bounds__(kClB) void msclean_peak_kernel(const double* __restrict__ pv,
                                                            const int* __restrict__ pp, int n_s,
                                                            int tiles,
                                                            const double* __restrict__ weight,
                                                            double* __restrict__ peak) {
  __shared__ double s_d[2 * kClB / 64];
  __shared__ int s_i[2 * kClB / 64];
  const int m = blockIdx.x;
  const int64_t map0 = (int64_t)m * n_s * tiles;
  const MsPeak x = ms_map_peak(pv + map0, pp + map0, n_s, tiles, weight + (int64_t)m * n_s, s_d, s_i);
  if (threadIdx.x == 0) peak[m] = x.pix >= 0 ? x.s : 0.0;
}

hipError_t msclean_launch(double* res, int n_maps, int n_s, int nx, int nz, const double* xpsf,
                          int n_psf, int px, int pz, const double* d_weight, const uint8_t* mask,
                          const double* d_thresh, double gain, int n_iter, int32_t* cpix,
                          int32_t* cscale, double* cflux, int32_t* ncomp, double* model,
                          double* peak, void* work, hipStream_t st) {
  const MsCleanTiling t = msclean_tiling(n_maps, n_s, nx, nz);
  const int tiles = (int)t.tiles;
  const unsigned nb = (unsigned)t.workgroups;
  const int64_t npix = (int64_t)nx * nz, half = t.workgroups, bpix = (int64_t)px * pz;
  // workspace: values [2][n_maps][n_s][tiles] f64, then pixels [2][n_maps][n_s][tiles] i32
  double* pv = (double*)work;
  int* pp = (int*)(pv + 2 * half);
  const int64_t psf_stride = n_psf == 1 ? 0 : bpix * ((int64_t)n_s * (n_s + 1) / 2);
  const int64_t centre = (int64_t)((px - 1) / 2) * pz + (pz - 1) / 2;
  hipLaunchKernelGGL(msclean_init_kernel, dim3(nb), dim3(kClB), 0, st, res, npix, n_s, tiles, xpsf,
                     psf_stride, bpix, centre, d_weight, mask, pv, pp, ncomp);
  hipError_t err = hipGetLastError();
  for (int it = 0; it < n_iter && err == hipSuccess; ++it) {
    const int64_t in = (it & 1) * half, out = ((it + 1) & 1) * half;
    hipLaunchKernelGGL(msclean_step_kernel, dim3(nb), dim3(kClB), 0, st, res, npix, nz, n_s, tiles,
                       xpsf, psf_stride, px, pz, d_weight, mask, d_thresh, gain, it, n_iter, pv + in,
                       pp + in, pv + out, pp + out, cpix, cscale, cflux, ncomp, model);
    err = hipGetLastError();
  }
  if (err != hipSuccess || !peak) return err;
  const int64_t last = (n_iter & 1) * half;
  hipLaunchKernelGGL(msclean_peak_kernel, dim3((unsigned)n_maps), dim3(kClB), 0, st, pv + last,
                     pp + last, n_s, tiles, d_weight, peak);
  return hipGetLastError();
}

}  // namespace rjp
