// K15 (rjp_uv_weights): uniform and Briggs imaging weights from the density of the (u, v) points on
// the Fourier grid of an image -- what tclean(weighting='briggs', robust=0.5) applies before it
// transforms (reference classes.py:2775-2776).  Per map m on an nx x nz image, hx = nx / 2, hz = nz / 2:
//   gu = rint((su[m] u[k]) nx), gv = rint((sv[m] v[k]) nz)     two double products each, in this order
//   counted: u, v, w finite, w >= 0, |gu| <= hx and |gv| <= hz (compared in double)
//   S(c) = sum of the counted q_k in cell c,  q_k = rint(w_k 2^s)  (int64: the sum has no order)
//   W(c) = (S(c) + S(-c)) 2^-s                                  Hermitian gridding, the origin twice
//   uniform w'_k = w_k / W(c_k);  Briggs w'_k = w_k / fma(f2, W(c_k), 1),
//   f2 = (5 10^-R)^2 (2 sum_k w_k) / sum_c W(c)^2.
// The cells are stored at (gu + hx)(2 hz + 1) + (gv + hz), so the mirror of cell i is cell
// ncell - 1 - i: every visibility adds ONCE, to its own cell, and W is folded when it is read --
// half the atomics of adding to both cells, and integers, so the fold is exact.
// A uniform weight whose cell holds nothing (weights below 2^-s all of them) is 0, not w / 0.
// One memset and five launches for the whole stack, stream-ordered, no host synchronisation:
//   (memset)            the scale word, the per-map counters and S: the workspace is laid out so
//                       that one memset covers them, whatever the ratio of cells to visibilities
//   uvw_scale_kernel    max of the counted weights over the call (integer atomicMax on the bits of
//                       the non-negative double, one per wave)
//   uvw_scatter_kernel  one thread per (map, visibility): one 64-bit integer atomicAdd to S; the
//                       map's sum of q and its two counts are reduced per wave first, one atomic
//                       per wave and counter
//   uvw_square_kernel   tiles of 1024 cells: W (written to d_density when asked) and the tile's
//                       sum of W^2 in a fixed order
//   uvw_norm_kernel     one wave per map: the tiles' sums in a fixed order, f2, the statistics
//   uvw_apply_kernel    the cell again by the identical expression, two loads of S, w'
// The atomics are device scope (HIP's default; they execute at the memory side) and every consumer
// is a later launch, so no fence or scope is needed beyond the kernel boundaries.  No
// floating-point atomics anywhere: a repeated call gives the same bits, a permutation of the
// visibilities permutes the weights, and (u, v) -> (-u, -v) changes nothing.
#include "rjp_host.h"

namespace rjp {

constexpr int kUwB = 256;          // threads per workgroup, one visibility (or four cells) each
constexpr int kUwTile = 1024;      // cells per tile of the sum of W^2
constexpr size_t kUwHead = 256;    // bytes in front of the counters: the scale word

struct UvwLayout {
  int64_t ncell;                   // (2 hx + 1)(2 hz + 1), per map
  int64_t tiles;                   // of 1024 cells, per map
  int64_t vis_blocks;              // workgroups of 256 visibilities, per map
  size_t off_cnt, off_part, off_S, bytes;   // bytes == 0: does not fit
};

static UvwLayout uvw_layout(int n_maps, int nx, int nz, int n_vis) {
  UvwLayout l;
  const unsigned __int128 nc = (unsigned __int128)(2 * (int64_t)(nx / 2) + 1) *
                               (unsigned __int128)(2 * (int64_t)(nz / 2) + 1);
  l.ncell = nc > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)nc;
  l.tiles = l.ncell / kUwTile + (l.ncell % kUwTile != 0);
  l.vis_blocks = ((int64_t)n_vis + kUwB - 1) / kUwB;
  // the scale word, the counters and S come first, so that ONE memset zeroes them; the tiles'
  // sums, which are all written, follow.  More than 2^31 - 1 cells per map: no size (refused)
  l.off_cnt = kUwHead;
  l.off_S = l.off_cnt + (size_t)n_maps * 32;
  const unsigned __int128 part = (unsigned __int128)n_maps * (unsigned __int128)l.tiles * 8u;
  const unsigned __int128 dens = (unsigned __int128)n_maps * nc * 8u;
  const unsigned __int128 tot = (unsigned __int128)l.off_S + dens + part;
  const bool fits = nc <= (unsigned __int128)INT32_MAX && tot <= (unsigned __int128)SIZE_MAX;
  l.off_part = fits ? (size_t)((unsigned __int128)l.off_S + dens) : 0;
  l.bytes = fits ? (size_t)tot : 0;
  return l;
}

UvWeightTiling uv_weights_tiling(int n_maps, int nx, int nz, int n_vis) {
  const UvwLayout l = uvw_layout(n_maps, nx, nz, n_vis);
  UvWeightTiling t;
  t.cells = l.ncell;
  t.workgroups = (int64_t)n_maps * l.vis_blocks;
  t.square_workgroups = l.ncell > (int64_t)INT32_MAX ? INT64_MAX : (int64_t)n_maps * l.tiles;
  return t;
}

size_t uv_weights_workspace_bytes(int n_maps, int nx, int nz, int n_vis) {
  return uvw_layout(n_maps, nx, nz, n_vis).bytes;
}

// per map: [0] sum of q (int64), [1] counted, [2] out of range, [3] the bits of f2
struct UvwCnt {
  unsigned long long v[4];
};

// s = 62 - e - L with w_max < 2^e (frexp) and L = ceil(log2(2 n_vis)), the smallest L with
// 2^L >= 2 n_vis; a w_max of 0 has no scale: s = 0 and every q is 0
__device__ __forceinline__ int uvw_shift(unsigned long long wmax_bits, int n_vis) {
  const double wmax = __longlong_as_double((long long)wmax_bits);
  if (!(wmax > 0.0)) return 0;
  int e;
  (void)frexp(wmax, &e);
  const int L = n_vis > 1 ? 33 - __builtin_clz((unsigned)(n_vis - 1)) : 1;
  return 62 - e - L;
}

// The cell of visibility (u, v) of a map with the scales (su, sv): -1 = out of range.  The ONE
// expression the scale pass, the scatter and the apply pass share.
__device__ __forceinline__ int64_t uvw_cell(double su, double sv, double u, double v, int nx, int nz) {
  const int hx = nx / 2, hz = nz / 2;
  const double gu = __builtin_rint((su * u) * (double)nx);
  const double gv = __builtin_rint((sv * v) * (double)nz);
  if (!(__builtin_fabs(gu) <= (double)hx) || !(__builtin_fabs(gv) <= (double)hz)) return -1;
  return ((int64_t)gu + hx) * (2 * (int64_t)hz + 1) + ((int64_t)gv + hz);
}

__device__ __forceinline__ bool uvw_flagged(double u, double v, double w) {
  return !finite_d(u) || !finite_d(v) || !finite_d(w) || !(w >= 0.0);
}

__device__ __forceinline__ unsigned long long uvw_wave_sum(unsigned long long x) {
#pragma unroll
  for (int d = 1; d < RJP_WAVE; d <<= 1) x += __shfl_xor(x, d, RJP_WAVE);
  return x;
}

__device__ __forceinline__ unsigned long long uvw_wave_max(unsigned long long x) {
#pragma unroll
  for (int d = 1; d < RJP_WAVE; d <<= 1) {
    const unsigned long long y = __shfl_xor(x, d, RJP_WAVE);
    x = y > x ? y : x;
  }
  return x;
}

// workgroup b serves visibilities (b % vb) 256 ... of map b / vb
__global__ __launch_bounds__(kUwB) void uvw_scale_kernel(
    const double* __restrict__ su, const double* __restrict__ sv, const double* __restrict__ u,
    const double* __restrict__ v, const double* __restrict__ w, int n_vis, int vb, int nx, int nz,
    unsigned long long* __restrict__ wmax) {
  const int m = (int)(blockIdx.x / (unsigned)vb);
  const int64_t k = (int64_t)(blockIdx.x % (unsigned)vb) * kUwB + threadIdx.x;
  unsigned long long bits = 0;
  if (k < n_vis) {
    const double uk = u[k], vk = v[k], wk = w ? w[k] : 1.0;
    if (!uvw_flagged(uk, vk, wk) && uvw_cell(su[m], sv[m], uk, vk, nx, nz) >= 0)
      bits = (unsigned long long)__double_as_longlong(wk + 0.0);     // (-0 -> +0)
  }
  bits = uvw_wave_max(bits);
  if ((threadIdx.x & (RJP_WAVE - 1)) == 0 && bits != 0) atomicMax(wmax, bits);
}

__global__ __launch_bounds__(kUwB) void uvw_scatter_kernel(
    const double* __restrict__ su, const double* __restrict__ sv, const double* __restrict__ u,
    const double* __restrict__ v, const double* __restrict__ w, int n_vis, int vb, int nx, int nz,
    int64_t ncell, const unsigned long long* __restrict__ wmax, UvwCnt* __restrict__ cnt,
    long long* __restrict__ S) {
  const int m = (int)(blockIdx.x / (unsigned)vb);
  const int64_t k = (int64_t)(blockIdx.x % (unsigned)vb) * kUwB + threadIdx.x;
  const int s = uvw_shift(*wmax, n_vis);
  unsigned long long q = 0, counted = 0, outside = 0;
  if (k < n_vis) {
    const double uk = u[k], vk = v[k], wk = w ? w[k] : 1.0;
    if (!uvw_flagged(uk, vk, wk)) {
      const int64_t c = uvw_cell(su[m], sv[m], uk, vk, nx, nz);
      if (c >= 0) {
        counted = 1;
        q = (unsigned long long)(long long)__builtin_rint(ldexp(wk, s));
        if (q) atomicAdd((unsigned long long*)(S + (int64_t)m * ncell + c), q);
      } else {
        outside = 1;
      }
    }
  }
  q = uvw_wave_sum(q);
  counted = uvw_wave_sum(counted);
  outside = uvw_wave_sum(outside);
  if ((threadIdx.x & (RJP_WAVE - 1)) == 0) {
    if (q) atomicAdd(&cnt[m].v[0], q);
    if (counted) atomicAdd(&cnt[m].v[1], counted);
    if (outside) atomicAdd(&cnt[m].v[2], outside);
  }
}

// W of cell i of a map whose S starts at Sm: the cell and its mirror, one correctly rounded
// int64 -> double conversion, an exact scaling
__device__ __forceinline__ double uvw_density(const long long* __restrict__ Sm, int64_t ncell,
                                              int64_t i, int s) {
  return ldexp((double)(Sm[i] + Sm[ncell - 1 - i]), -s);
}

// workgroup b: tile b % tiles of map b / tiles.  Thread t takes cells t, t + 256, t + 512, t + 768
// of the tile in this order; lanes by xor butterfly, the four waves in wave order.
__global__ __launch_bounds__(kUwB) void uvw_square_kernel(
    const long long* __restrict__ S, int64_t ncell, int tiles, int n_vis,
    const unsigned long long* __restrict__ wmax, double* __restrict__ part,
    double* __restrict__ density) {
  __shared__ double s_w[kUwB / RJP_WAVE];
  const int m = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
  const int s = uvw_shift(*wmax, n_vis);
  const long long* __restrict__ Sm = S + (int64_t)m * ncell;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < kUwTile / kUwB; ++j) {
    const int64_t i = (int64_t)tile * kUwTile + j * kUwB + threadIdx.x;
    if (i < ncell) {
      const double W = uvw_density(Sm, ncell, i, s);
      if (density) density[(int64_t)m * ncell + i] = W;
      acc = __builtin_fma(W, W, acc);
    }
  }
#pragma unroll
  for (int d = 1; d < RJP_WAVE; d <<= 1) acc += __shfl_xor(acc, d, RJP_WAVE);
  if ((threadIdx.x & (RJP_WAVE - 1)) == 0) s_w[threadIdx.x / RJP_WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = s_w[0];
#pragma unroll
    for (int i = 1; i < kUwB / RJP_WAVE; ++i) t += s_w[i];
    part[(int64_t)m * tiles + tile] = t;
  }
}

// one wave per map: lane l adds tiles l, l + 64, ... in this order, then the xor butterfly
__global__ __launch_bounds__(RJP_WAVE) void uvw_norm_kernel(
    const double* __restrict__ part, int tiles, int n_vis, int mode, double c2,
    const unsigned long long* __restrict__ wmax, UvwCnt* __restrict__ cnt,
    double* __restrict__ stats) {
  const int m = blockIdx.x;
  double acc = 0.0;
  for (int t = threadIdx.x; t < tiles; t += RJP_WAVE) acc += part[(int64_t)m * tiles + t];
#pragma unroll
  for (int d = 1; d < RJP_WAVE; d <<= 1) acc += __shfl_xor(acc, d, RJP_WAVE);
  if (threadIdx.x != 0) return;
  const int s = uvw_shift(*wmax, n_vis);
  const double sumw = ldexp((double)(long long)cnt[m].v[0], -s);
  double f2 = 0.0;
  if (mode == 2 && acc > 0.0) f2 = (c2 * (2.0 * sumw)) / acc;
  cnt[m].v[3] = (unsigned long long)__double_as_longlong(f2);
  if (stats) {
    double* __restrict__ o = stats + (int64_t)m * 6;
    o[0] = sumw;
    o[1] = acc;
    o[2] = f2;
    o[3] = (double)cnt[m].v[1];
    o[4] = (double)cnt[m].v[2];
    o[5] = (double)s;
  }
}

__global__ __launch_bounds__(kUwB) void uvw_apply_kernel(
    const double* __restrict__ su, const double* __restrict__ sv, const double* __restrict__ u,
    const double* __restrict__ v, const double* __restrict__ w, int n_vis, int vb, int nx, int nz,
    int64_t ncell, int mode, const unsigned long long* __restrict__ wmax,
    const UvwCnt* __restrict__ cnt, const long long* __restrict__ S, double* __restrict__ wout) {
  const int m = (int)(blockIdx.x / (unsigned)vb);
  const int64_t k = (int64_t)(blockIdx.x % (unsigned)vb) * kUwB + threadIdx.x;
  if (k >= n_vis) return;
  const int s = uvw_shift(*wmax, n_vis);
  const double uk = u[k], vk = v[k], wk = w ? w[k] : 1.0;
  double r = 0.0;
  if (!uvw_flagged(uk, vk, wk)) {
    const int64_t c = uvw_cell(su[m], sv[m], uk, vk, nx, nz);
    if (c >= 0) {
      const double W = uvw_density(S + (int64_t)m * ncell, ncell, c, s);
      if (mode == 2) {
        const double f2 = __longlong_as_double((long long)cnt[m].v[3]);
        r = (wk + 0.0) / __builtin_fma(f2, W, 1.0);
      } else if (W > 0.0) {                         // (a cell of weights too small to count: 0)
        r = (wk + 0.0) / W;
      }
    }
  }
  wout[(int64_t)m * n_vis + k] = r;
}

hipError_t uv_weights_launch(int n_maps, int n_vis, const double* d_su, const double* d_sv,
                             const double* u, const double* v, const double* w, int nx, int nz,
                             int mode, double c2, double* wout, double* stats, double* density,
                             void* work, hipStream_t st) {
  const UvwLayout l = uvw_layout(n_maps, nx, nz, n_vis);
  char* base = (char*)work;
  unsigned long long* wmax = (unsigned long long*)base;
  UvwCnt* cnt = (UvwCnt*)(base + l.off_cnt);
  double* part = (double*)(base + l.off_part);
  long long* S = (long long*)(base + l.off_S);
  const unsigned nb = (unsigned)((int64_t)n_maps * l.vis_blocks);
  const int vb = (int)l.vis_blocks, tiles = (int)l.tiles;
  hipError_t err = hipMemsetAsync(base, 0, l.off_part, st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(uvw_scale_kernel, dim3(nb), dim3(kUwB), 0, st, d_su, d_sv, u, v, w, n_vis, vb,
                     nx, nz, wmax);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  hipLaunchKernelGGL(uvw_scatter_kernel, dim3(nb), dim3(kUwB), 0, st, d_su, d_sv, u, v, w, n_vis,
                     vb, nx, nz, l.ncell, wmax, cnt, S);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  hipLaunchKernelGGL(uvw_square_kernel, dim3((unsigned)((int64_t)n_maps * l.tiles)), dim3(kUwB), 0,
                     st, S, l.ncell, tiles, n_vis, wmax, part, density);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  hipLaunchKernelGGL(uvw_norm_kernel, dim3((unsigned)n_maps), dim3(RJP_WAVE), 0, st, part, tiles,
                     n_vis, mode, c2, wmax, cnt, stats);
  if ((err = hipGetLastError()) != hipSuccess) return err;
  hipLaunchKernelGGL(uvw_apply_kernel, dim3(nb), dim3(kUwB), 0, st, d_su, d_sv, u, v, w, n_vis, vb,
                     nx, nz, l.ncell, mode, wmax, cnt, S, wout);
  return hipGetLastError();
}

}  // namespace rjp
