// K18 (rjp_vis_components): the visibilities of a list of clean components, added to or taken from a
// stack of visibility sets -- the cheap forward step of a CLEAN major cycle -- and
// rjp_components_image: the delta model image of the same list.
//
// K18.  out[m,k] = in[m,k] + sign sum_s G[m,s,k] sum_{c < ncomp[m], cscale[m,c] = s}
//                  f_c exp(-2 pi i (a (ix_c - (nx-1)/2) + b (iz_c - (nz-1)/2))),
//       a = su[m] u[k], b = sv[m] v[k], p_c = ix_c nz + iz_c.
// n_comp x n_vis phasors, where K10 on the dense model image would take nx nz x n_vis multiply-adds
// (and nx + nz phasors) per visibility.  A workgroup of 256 threads owns 64 visibilities of one map:
// lane l of every wave is visibility k0 + l, and the four waves take four SLICES of the list.  The
// list goes through LDS in chunks of kVcC = 256 components as (jx, jz, f, s) -- jx = ix - (nx-1)/2 and
// jz likewise (half-integers: exact), f = sign x flux (exact), s the scale, -1 for a component that
// adds nothing -- and wave w reads entries [64 w, 64 w + 64) of every chunk by broadcast: slice w is
// the components c with (c mod 256) / 64 = w.  The order of every sum, per (map, visibility):
//   for s = 0 .. n_s - 1:                                       (the outer loop: the list is staged
//     for w = 0 .. 3:  P[w] = sum over slice w's components      once per scale; `s_c == s` is uniform
//                      of scale s, in list order:                over the wave, so there is no
//        (sx, cx) = sincos_2pi(a jx), (sz, cz) = sincos_2pi(b jz) divergence and no gather)
//        cr = fma(cx, cz, -(sx sz)), si = fma(sx, cz, cx sz)
//        P.re = fma(f, cr, P.re), P.im = fma(-f, si, P.im)
//     T[w] += G[m,s,k] P[w]:  T.re = fma(-G.im, P.im, fma(G.re, P.re, T.re)),
//                             T.im = fma(G.im, P.re, fma(G.re, P.im, T.im))   (G NULL: T[w] += P[w])
//   out = in + (((T[0] + T[1]) + T[2]) + T[3])                  (the slices meet in LDS, in slice order)
// Phase arguments are ONE double product per factor, a jx and b jz, reduced and evaluated by
// sincos_2pi, exactly as K10 forms them; no recurrence, no float.  No atomics: the same bits on every
// call.  A map with ncomp = 0 copies `in` bit for bit; a non-finite u[k] or v[k] makes visibility k
// NaN in every map; a non-finite in[m,k] stays non-finite through the last add.
//
// rjp_components_image.  out[m][s][q] = sum_{c: p_c = q, s_c = s} f_c in list order from +0.0: K13
// with a delta beam.  One pixel per thread, 256 pixels per workgroup, grid = tiles x planes x maps;
// the list staged through LDS in chunks of 256 as (p, f, s) and read by broadcast.  What rjp_clean
// and rjp_msclean add into a zeroed d_model, to the bit, as a function of the list alone.
#include "rjp_host.h"

namespace rjp {

constexpr int kVcB = 256;          // threads per workgroup: 4 waves = 4 slices
constexpr int kVcV = 64;           // visibilities per workgroup: one per lane
constexpr int kVcC = 256;          // components per LDS chunk: 64 per slice

int64_t vis_components_workgroups(int n_maps, int n_vis) {
  return (((int64_t)n_vis + kVcV - 1) / kVcV) * n_maps;
}

int64_t components_image_workgroups(int n_maps, int n_s, int nx, int nz) {
  return (((int64_t)nx * nz + kVcB - 1) / kVcB) * n_s * n_maps;
}

__global__ __launch_bounds__(kVcB) void vis_components_kernel(
    const int* __restrict__ cpix, const int* __restrict__ cscale, const double* __restrict__ cflux,
    const int* __restrict__ ncomp, int comp_stride, int n_s, int nx, int nz,
    const double* __restrict__ su, const double* __restrict__ sv, const double* __restrict__ u,
    const double* __restrict__ v, int n_vis, int nvt, const double* __restrict__ gvis,
    const double* in, double sign, double* out) {
  __shared__ double s_jx[kVcC], s_jz[kVcC], s_f[kVcC];
  __shared__ int s_s[kVcC];
  __shared__ double s_t[kVcB / 64][kVcV][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int vt = (int)(blockIdx.x % (unsigned)nvt), m = (int)(blockIdx.x / (unsigned)nvt);
  const int k = vt * kVcV + lane;
  const bool have = k < n_vis;
  const double uk = have ? u[k] : 0.0, vk = have ? v[k] : 0.0;
  const double a = su[m] * uk, b = sv[m] * vk;
  const int64_t npix = (int64_t)nx * nz;
  const double cx = 0.5 * (double)(nx - 1), cz = 0.5 * (double)(nz - 1);
  const int n = min(max(ncomp[m], 0), comp_stride);
  const int* __restrict__ cp = cpix + (int64_t)m * comp_stride;
  const int* __restrict__ cs = cscale ? cscale + (int64_t)m * comp_stride : nullptr;
  const double* __restrict__ cf = cflux + (int64_t)m * comp_stride;

  double tr = 0.0, ti = 0.0;
  for (int s = 0; s < n_s; ++s) {
    double pr = 0.0, pi = 0.0;
    for (int c0 = 0; c0 < n; c0 += kVcC) {
      __syncthreads();                              // the previous chunk's readers are done
      const int c = c0 + tid;
      if (c < n) {
        const int p = cp[c], sc = cs ? cs[c] : 0;
        const double f = cf[c];
        const bool ok = finite_d(f) && p >= 0 && (int64_t)p < npix && sc >= 0 && sc < n_s;
        // (32-bit division: 0 <= p < 2^31 where it counts)
        const int ix = ok ? (int)((unsigned)p / (unsigned)nz) : 0;
        const int iz = ok ? p - ix * nz : 0;
        s_jx[tid] = (double)ix - cx;
        s_jz[tid] = (double)iz - cz;
        s_f[tid] = ok ? sign * f : 0.0;
        s_s[tid] = ok ? sc : -1;
      }
      __syncthreads();
      const int j1 = min(kVcC, n - c0);
      for (int j = wave * 64; j < min(wave * 64 + 64, j1); ++j) {
        if (s_s[j] != s) continue;                  // (an LDS broadcast: uniform over the wave)
        double sx, cxx, sz, czz;
        sincos_2pi(a * s_jx[j], sx, cxx);
        sincos_2pi(b * s_jz[j], sz, czz);
        const double cr = __builtin_fma(cxx, czz, -(sx * sz));
        const double si = __builtin_fma(sx, czz, cxx * sz);
        const double f = s_f[j];
        pr = __builtin_fma(f, cr, pr);
        pi = __builtin_fma(-f, si, pi);
      }
    }
    if (gvis) {
      const double* g = gvis + (((int64_t)m * n_s + s) * n_vis + (have ? k : 0)) * 2;
      const double gr = g[0], gi = g[1];
      tr = __builtin_fma(-gi, pi, __builtin_fma(gr, pr, tr));
      ti = __builtin_fma(gi, pr, __builtin_fma(gr, pi, ti));
    } else {
      tr += pr;
      ti += pi;
    }
  }
  s_t[wave][lane][0] = tr;
  s_t[wave][lane][1] = ti;
  __syncthreads();
  if (wave == 0 && have) {
    const int64_t o = ((int64_t)m * n_vis + k) * 2;
    double re = in ? in[o] : 0.0, im = in ? in[o + 1] : 0.0;
    if (!finite_d(uk) || !finite_d(vk)) {
      re = im = __builtin_nan("");
    } else if (n > 0) {
      double sr = s_t[0][lane][0], sm = s_t[0][lane][1];
#pragma unroll
      for (int w = 1; w < kVcB / 64; ++w) {
        sr += s_t[w][lane][0];
        sm += s_t[w][lane][1];
      }
      re += sr;
      im += sm;
    }
    out[o] = re;
    out[o + 1] = im;
  }
}

hipError_t vis_components_launch(const int32_t* cpix, const int32_t* cscale, const double* cflux,
                                 const int32_t* ncomp, int n_maps, int comp_stride, int n_s, int nx,
                                 int nz, const double* d_su, const double* d_sv, const double* u,
                                 const double* v, int n_vis, const double* gvis, const double* in,
                                 int sign, double* out, hipStream_t st) {
  const int nvt = (n_vis + kVcV - 1) / kVcV;
  hipLaunchKernelGGL(vis_components_kernel, dim3((unsigned)vis_components_workgroups(n_maps, n_vis)),
                     dim3(kVcB), 0, st, cpix, cscale, cflux, ncomp, comp_stride, n_s, nx, nz, d_su,
                     d_sv, u, v, n_vis, nvt, gvis, in, (double)sign, out);
  return hipGetLastError();
}

__global__ __launch_bounds__(kVcB) void components_image_kernel(
    const int* __restrict__ cpix, const int* __restrict__ cscale, const double* __restrict__ cflux,
    const int* __restrict__ ncomp, int comp_stride, int n_s, int64_t npix, int tiles,
    double* __restrict__ out) {
  __shared__ int s_p[kVcC], s_s[kVcC];
  __shared__ double s_f[kVcC];
  const int tid = threadIdx.x;
  const int tile = (int)(blockIdx.x % (unsigned)tiles);
  const unsigned rest = blockIdx.x / (unsigned)tiles;
  const int s = (int)(rest % (unsigned)n_s), m = (int)(rest / (unsigned)n_s);
  const int64_t q = (int64_t)tile * kVcB + tid;
  const int n = min(max(ncomp[m], 0), comp_stride);
  const int* __restrict__ cp = cpix + (int64_t)m * comp_stride;
  const int* __restrict__ cs = cscale ? cscale + (int64_t)m * comp_stride : nullptr;
  const double* __restrict__ cf = cflux + (int64_t)m * comp_stride;
  double acc = 0.0;
  for (int c0 = 0; c0 < n; c0 += kVcC) {
    __syncthreads();                                // the previous chunk's readers are done
    const int c = c0 + tid;
    if (c < n) {
      const double f = cf[c];
      // (a pixel outside [0, nx nz) meets no q; a non-finite flux gets a scale no plane has)
      s_p[tid] = cp[c];
      s_f[tid] = f;
      s_s[tid] = finite_d(f) ? (cs ? cs[c] : 0) : -1;
    }
    __syncthreads();
    const int nc = min(kVcC, n - c0);
    for (int j = 0; j < nc; ++j)
      if (s_s[j] == s && (int64_t)s_p[j] == q) acc += s_f[j];
  }
  if (q < npix) out[((int64_t)m * n_s + s) * npix + q] = acc;
}

hipError_t components_image_launch(const int32_t* cpix, const int32_t* cscale, const double* cflux,
                                   const int32_t* ncomp, int n_maps, int comp_stride, int n_s,
                                   int nx, int nz, double* out, hipStream_t st) {
  const int64_t npix = (int64_t)nx * nz;
  const int tiles = (int)((npix + kVcB - 1) / kVcB);
  hipLaunchKernelGGL(components_image_kernel,
                     dim3((unsigned)components_image_workgroups(n_maps, n_s, nx, nz)), dim3(kVcB), 0,
                     st, cpix, cscale, cflux, ncomp, comp_stride, n_s, npix, tiles, out);
  return hipGetLastError();
}

}  // namespace rjp
