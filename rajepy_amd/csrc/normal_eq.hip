// K23 (rjp_normal_eq): the normal equations of a least-squares fit from stacks of data, model and
// model derivatives that are already on the device -- a tall-skinny Gram matrix with a tiny output
// and a huge reduction axis.  include/rjprt.h holds the definition; this comment holds the order of
// every sum, which is part of it.
//
// The real operand.  Sample s = row * n_vis + k has n_part real parts (re, im).  With C = P + 1
// columns -- the P selected derivative planes in the order of h_sel, then the residual r = y - m --
// every part of every counting sample is one real row a[0 .. C) of a tall matrix, and
//   G = sum over rows of a^T (w a)                       (upper triangle, p <= q)
// holds everything: N_pq = G[p][q], g_p = G[p][P], chi^2 = G[P][P].
//
// The order.  A tile is kNeTile = 512 consecutive flattened samples.  Inside a tile, sample i (0 ..
// 511) belongs to slice i mod 16.  A slice starts every entry at +0 and takes its samples in
// increasing i, per sample part 0 then part 1, each as ONE fused multiply-add
//   G[p][q] <- fma(a_p, w * a_q, G[p][q])       (w * a_q rounded once; the weight on the column with
//                                                the higher index, for g and chi^2 on r)
// A non-counting sample enters as a row of zeros with w = 0 (fma(0, 0, x) = x for every x a slice
// can hold: none is ever -0).  The 16 slices of a tile are then added in slice order, ((s0 + s1) +
// s2) + ..., and the tiles in tile order by the second launch, starting from tile 0's partial.  The
// order does not depend on P, on the instantiation or on the launch geometry.
//
// The shape.  512 threads per tile.  Thread t first classifies sample t of the tile (w_eff, r) into
// LDS.  Then 32 sub-tiles of 16 samples (one per slice): all threads fetch the sub-tile's P x 16 x
// n_part derivative values into registers one sub-tile ahead, store them to LDS as a and w a, and
// NB (NB + 1) / 2 x 16 threads -- one per (BS x BS block of the upper triangle, slice) -- multiply
// from LDS with BS^2 accumulators in registers: 2 BS LDS doubles per BS^2 FMAs.  Thread t works
// on slice t / blocks, block t % blocks: a wave of 64 spans 3 (28 blocks) to 7 (10 blocks) slices,
// i.e. as many LDS rows, and up to NB column offsets in each; the rows lie CP + 2 doubles apart
// so that consecutive rows start 4 to 52 banks apart instead of on the same ones.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rjp_host.h"

namespace rjp {

constexpr int kNeTile = 512;      // samples per tile = threads per workgroup
constexpr int kNeSlices = 16;     // interleaved slices of a tile = samples per sub-tile
constexpr int kNeSumB = 256;      // threads per workgroup of the second launch

struct NeSel {
  int32_t plane[RJP_NORMAL_EQ_MAX_SEL];
};

int64_t normal_eq_tiles(int64_t n_rows, int n_vis) {
  return (n_rows * (int64_t)n_vis + kNeTile - 1) / kNeTile;
}

static size_t ne_outputs(int n_sel) { return 1 + (size_t)n_sel + (size_t)n_sel * (n_sel + 1) / 2; }

size_t normal_eq_workspace_bytes(int64_t n_rows, int n_vis, int n_sel) {
  return (size_t)normal_eq_tiles(n_rows, n_vis) * (ne_outputs(n_sel) + 1) * 8;
}

// index of (p, q), p <= q < P, in the packed upper triangle, row by row
static __device__ __forceinline__ int ne_tri(int p, int q, int P) {
  return p * P - p * (p - 1) / 2 + (q - p);
}

template <int BS, int NB>
__global__ __launch_bounds__(kNeTile) void normal_eq_tile_kernel(
    const double* __restrict__ data, const double* __restrict__ model,
    const double* __restrict__ dmodel, const double* __restrict__ w, int w_shared, int64_t n_samples,
    int n_vis, int n_part, int n_par, int P, NeSel sel, double* __restrict__ part,
    int64_t* __restrict__ part_count) {
  constexpr int CP = BS * NB;                      // padded columns, >= P + 1
  constexpr int NBLK = NB * (NB + 1) / 2;          // blocks of the upper triangle
  constexpr int ROWS = 2 * kNeSlices;              // real rows of a sub-tile at n_part = 2
  constexpr int STR = CP + 2;                      // row stride of a and w a: off the 64-byte multiples
  constexpr int NBUF = 2 * ROWS * STR > CP * CP ? 2 * ROWS * STR : CP * CP;
  constexpr int NIT = (ROWS * CP + kNeTile - 1) / kNeTile;   // staged values per thread
  __shared__ double buf[NBUF];                     // a | w a of a sub-tile; at the end G[CP][CP]
  __shared__ double wl[kNeTile];                   // w of a counting sample, else 0
  __shared__ double rl[kNeTile][2];                // r of a counting sample, else 0
  __shared__ int32_t sl[RJP_NORMAL_EQ_MAX_SEL];    // the selected planes (indexed per lane)
  double* __restrict__ A = buf;
  double* __restrict__ WA = buf + ROWS * STR;

  const int tid = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kNeTile;
  const int C = P + 1;

  // ---- classify sample `tid` of the tile
  bool counts = false;
  {
    const int64_t s = base + tid;
    double wt = 0.0, r0 = 0.0, r1 = 0.0;
    if (s < n_samples) {
      const int64_t k = s % n_vis;
      wt = w ? w[w_shared ? k : s] : 1.0;
      const double y0 = data[s * n_part], y1 = n_part == 2 ? data[s * n_part + 1] : 0.0;
      counts = __builtin_isfinite(y0) && __builtin_isfinite(y1) && __builtin_isfinite(wt) && wt > 0.0;
      if (counts) {
        r0 = y0 - model[s * n_part];
        if (n_part == 2) r1 = y1 - model[s * n_part + 1];
      }
    }
    wl[tid] = counts ? wt : 0.0;
    rl[tid][0] = counts ? r0 : 0.0;
    rl[tid][1] = counts ? r1 : 0.0;
  }
  for (int i = tid; i < 2 * ROWS * STR; i += kNeTile) buf[i] = 0.0;   // the padding stays zero
  if (tid < P) sl[tid] = sel.plane[tid];
  const int n_count = __syncthreads_count(counts);

  // ---- what this thread stages: value e = tid + i * 512 of a sub-tile is (column e / rpt, real
  // row e % rpt), rpt = 16 n_part real rows; 512 is a multiple of rpt, so the row is the thread's
  const int rpt = kNeSlices * n_part;
  const int my_row = tid % rpt;                    // = sample-in-sub-tile * n_part + part
  const int my_smp = my_row / n_part, my_part = my_row - my_smp * n_part;
  const int col0 = tid / rpt, dcol = kNeTile / rpt;
  const int64_t plane = (int64_t)n_vis * n_part;   // doubles per derivative plane
  double stage[NIT];
  auto fetch = [&](int sub) {
    const int i_s = sub * kNeSlices + my_smp;
    const int64_t s = base + i_s;
    const bool live = s < n_samples && wl[i_s] > 0.0;
    const int64_t row = live ? s / n_vis : 0;
    const int64_t off = row * n_par * plane + (s - row * n_vis) * n_part + my_part;
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
      const int c = col0 + i * dcol;
      double v = 0.0;
      if (live && c < P) v = dmodel[off + (int64_t)sl[c] * plane];
      else if (c == P) v = rl[i_s][my_part];
      stage[i] = v;
    }
  };

  // ---- this thread's block and slice
  const bool worker = tid < NBLK * kNeSlices;
  const int slice = tid / NBLK;
  int bi = 0, bj = 0;
  {
    int b = tid - slice * NBLK;
    while (b >= NB - bi) {
      b -= NB - bi;
      ++bi;
    }
    bj = bi + b;
  }
  double acc[BS][BS];
#pragma unroll
  for (int x = 0; x < BS; ++x)
#pragma unroll
    for (int y = 0; y < BS; ++y) acc[x][y] = 0.0;

  fetch(0);
  for (int sub = 0; sub < kNeTile / kNeSlices; ++sub) {
    __syncthreads();                               // the previous sub-tile has been consumed
    {
      const double wt = wl[sub * kNeSlices + my_smp];
#pragma unroll
      for (int i = 0; i < NIT; ++i) {
        const int c = col0 + i * dcol;
        if (c < C) {
          A[my_row * STR + c] = stage[i];
          WA[my_row * STR + c] = wt > 0.0 ? wt * stage[i] : 0.0;
        }
      }
    }
    __syncthreads();
    if (sub + 1 < kNeTile / kNeSlices) fetch(sub + 1);
    if (worker) {
      for (int part_i = 0; part_i < n_part; ++part_i) {
        const double* __restrict__ ra = A + (slice * n_part + part_i) * STR + bi * BS;
        const double* __restrict__ rb = WA + (slice * n_part + part_i) * STR + bj * BS;
        double a[BS], b[BS];
#pragma unroll
        for (int x = 0; x < BS; ++x) {
          a[x] = ra[x];
          b[x] = rb[x];
        }
#pragma unroll
        for (int x = 0; x < BS; ++x)
#pragma unroll
          for (int y = 0; y < BS; ++y) acc[x][y] = __builtin_fma(a[x], b[y], acc[x][y]);
      }
    }
  }

  // ---- the slices, in slice order, into G (over the staging buffers)
  double* __restrict__ G = buf;
  for (int j = 0; j < kNeSlices; ++j) {
    __syncthreads();
    if (worker && slice == j) {
#pragma unroll
      for (int x = 0; x < BS; ++x)
#pragma unroll
        for (int y = 0; y < BS; ++y) {
          double* g = G + (bi * BS + x) * CP + bj * BS + y;
          *g = j == 0 ? acc[x][y] : *g + acc[x][y];
        }
    }
  }
  __syncthreads();

  // ---- the tile's partial: chi^2, g, the packed upper triangle of N
  double* __restrict__ out = part + (int64_t)blockIdx.x * (1 + P + P * (P + 1) / 2);
  if (tid == 0) {
    out[0] = G[P * CP + P];
    part_count[blockIdx.x] = n_count;
  }
  for (int p = tid; p < P; p += kNeTile) out[1 + p] = G[p * CP + P];
  for (int e = tid; e < P * P; e += kNeTile) {
    const int p = e / P, q = e - p * P;
    if (q >= p) out[1 + P + ne_tri(p, q, P)] = G[p * CP + q];
  }
}

// The second launch: output o is the sum of its partials in tile order.
__global__ __launch_bounds__(kNeSumB) void normal_eq_sum_kernel(
    const double* __restrict__ part, const int64_t* __restrict__ part_count, int64_t n_tiles,
    int n_out, double* __restrict__ out, int64_t* __restrict__ count) {
  const int o = blockIdx.x * kNeSumB + threadIdx.x;
  if (o < n_out) {
    double s = part[o];
    for (int64_t t = 1; t < n_tiles; ++t) s += part[t * n_out + o];
    out[o] = s;
  }
  if (o == 0) {
    int64_t n = 0;
    for (int64_t t = 0; t < n_tiles; ++t) n += part_count[t];
    *count = n;
  }
}

hipError_t normal_eq_launch(const double* data, const double* model, const double* dmodel,
                            int64_t n_rows, int n_vis, int n_part, int n_par, const int32_t* h_sel,
                            int n_sel, const double* w, int64_t w_rows, double* out, int64_t* count,
                            void* work, hipStream_t st) {
  const int64_t n_tiles = normal_eq_tiles(n_rows, n_vis);
  const int n_out = (int)ne_outputs(n_sel);
  double* part = (double*)work;
  int64_t* part_count = (int64_t*)(part + n_tiles * n_out);
  NeSel sel = {};
  for (int i = 0; i < n_sel; ++i) sel.plane[i] = h_sel[i];
  const int w_shared = w_rows == 1 && n_rows != 1 ? 1 : 0;
#define RJP_NE(BS, NB)                                                                          \
  hipLaunchKernelGGL((normal_eq_tile_kernel<BS, NB>), dim3((unsigned)n_tiles), dim3(kNeTile), 0, \
                     st, data, model, dmodel, w, w_shared, n_rows * (int64_t)n_vis, n_vis, n_part, \
                     n_par, n_sel, sel, part, part_count)
  if (n_sel < 8) RJP_NE(2, 4);              // P + 1 <= 8
  else if (n_sel < 16) RJP_NE(4, 4);        // <= 16
  else if (n_sel < 32) RJP_NE(8, 4);        // <= 32
  else RJP_NE(8, 7);                        // <= 56: RJP_NORMAL_EQ_MAX_SEL + 1 = 49
#undef RJP_NE
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(normal_eq_sum_kernel, dim3((unsigned)((n_out + kNeSumB - 1) / kNeSumB)),
                     dim3(kNeSumB), 0, st, part, part_count, n_tiles, n_out, out, count);
  return hipGetLastError();
}

}  // namespace rjp
