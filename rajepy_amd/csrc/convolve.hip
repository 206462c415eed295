// rjp_convolve2d: a direct 2-D convolution of a stack of images with small kernels,
//   out[m][i, j] = add[m][i, j] + sum_{a, b} ker[kappa][a, b] in[m][i - (a - ca), j - (b - cb)],
// (ca, cb) = ((kx - 1) / 2, (kz - 1) / 2), `in` zero outside the image, f64, one fma per term, the
// terms in kernel order (a outer, b inner, both ascending), `add` the accumulator's start: the bits
// are a function of the inputs alone.
//
// The tile rule (tests restate it on the host): a workgroup of 256 threads owns kCvX x kCvZ = 16 x 64
// output pixels (z is the contiguous axis); the grid is n_maps x ceil(nx / 16) x ceil(nz / 64), the
// z tiles running fastest.  Thread t owns column t % 64 of the rows t / 64 + {0, 4, 8, 12} and keeps
// their four accumulators in registers from the first term to the last.
// LDS: kCvLds = 8192 doubles (64 KiB: two workgroups fit a CU's 160 KiB).  The kernel is taken in
// chunks of `ka` rows, ka = conv_chunk_rows(kx, kz) the most for which
//   (16 + ka - 1)(64 + kz - 1)      the input tile plus halo of those rows
//   + ka kz                         the kernel rows themselves
// fits; ka >= 1 for every kz <= RJP_CONV_MAX_K = 255 (16 x 318 + 255 = 5343), and kz = 129 gives
// ka = 16, nine chunks for 129 rows.  Per chunk: stage (zeros outside the image), barrier, then per
// kernel element one LDS broadcast of the kernel value and four conflict-free 8-byte reads (a wave's
// 64 lanes read 64 consecutive doubles of one staged row), four fmas.  Whatever the image size the
// LDS use is the same: a 1 x 1 image is one workgroup with one live lane.
#include "rjp_host.h"

namespace rjp {

constexpr int kCvB = 256;
constexpr int kCvX = 16, kCvZ = 64;
constexpr int kCvR = kCvX / (kCvB / kCvZ);     // 4 rows per thread
constexpr int kCvLds = 8192;                   // doubles
static_assert(kCvX == RJP_CONV_TILE_X && kCvZ == RJP_CONV_TILE_Z, "the tile rule of rjprt.h");
static_assert((kCvLds - (kCvX - 1) * (kCvZ + RJP_CONV_MAX_K - 1)) / (kCvZ + 2 * RJP_CONV_MAX_K - 1) >= 1,
              "one kernel row of RJP_CONV_MAX_K fits");

int conv_chunk_rows(int kx, int kz) {
  const int w = kCvZ + kz - 1;
  const int ka = (kCvLds - (kCvX - 1) * w) / (w + kz);
  return ka < kx ? ka : kx;
}

ConvTiling conv_tiling(int n_maps, int nx, int nz) {
  ConvTiling t;
  t.tiles_x = ((int64_t)nx + kCvX - 1) / kCvX;
  t.tiles_z = ((int64_t)nz + kCvZ - 1) / kCvZ;
  t.workgroups = t.tiles_x * t.tiles_z * n_maps;
  return t;
}

__global__ __launch_bounds__(kCvB) void convolve2d_kernel(
    const double* __restrict__ in, int nx, int nz, const double* __restrict__ ker,
    int64_t ker_stride, int kx, int kz, int ka_max, const double* __restrict__ add,
    double* __restrict__ out, int tiles_x, int tiles_z) {
  __shared__ double s[kCvLds];
  const unsigned id = blockIdx.x;
  const int tz = (int)(id % (unsigned)tiles_z);
  const int tx = (int)((id / (unsigned)tiles_z) % (unsigned)tiles_x);
  const int m = (int)(id / ((unsigned)tiles_z * (unsigned)tiles_x));
  const int64_t npix = (int64_t)nx * nz;
  const double* __restrict__ im = in + (int64_t)m * npix;
  const double* __restrict__ km = ker + (int64_t)m * ker_stride;
  const int x0 = tx * kCvX, z0 = tz * kCvZ;
  const int ca = (kx - 1) / 2, cb = (kz - 1) / 2;
  const int w = kCvZ + kz - 1;                  // staged columns: z0 - cb ... z0 + 63 + cb
  const int c0 = z0 - cb;
  const int lj = threadIdx.x % kCvZ, li = threadIdx.x / kCvZ;
  double acc[kCvR];
#pragma unroll
  for (int r = 0; r < kCvR; ++r) {
    const int i = x0 + li + r * (kCvB / kCvZ), j = z0 + lj;
    acc[r] = (add && i < nx && j < nz) ? add[(int64_t)m * npix + (int64_t)i * nz + j] : 0.0;
  }
  for (int a0 = 0; a0 < kx; a0 += ka_max) {
    const int ka = min(ka_max, kx - a0);
    const int rows = kCvX + ka - 1;
    // staged rows: output row i and kernel row a read input row i - a + ca, so the chunk needs
    // x0 - (a0 + ka - 1 - ca) ... x0 + 15 - (a0 - ca)
    const int r0 = x0 - (a0 + ka - 1 - ca);
    double* __restrict__ sk = s + rows * w;     // the chunk's kernel rows, behind the tile
    __syncthreads();                            // the previous chunk's readers are done
    for (int e = threadIdx.x; e < rows * w; e += kCvB) {
      const int r = e / w, c = e - r * w;
      const int gx = r0 + r, gz = c0 + c;
      s[e] = (gx >= 0 && gx < nx && gz >= 0 && gz < nz) ? im[(int64_t)gx * nz + gz] : 0.0;
    }
    for (int e = threadIdx.x; e < ka * kz; e += kCvB) sk[e] = km[(int64_t)a0 * kz + e];
    __syncthreads();
    for (int a = 0; a < ka; ++a) {
      // local row of (li + 4 r, kernel row a0 + a): li + 4 r + (ka - 1 - a); column lj + kz - 1 - b
      const double* __restrict__ row = s + (li + ka - 1 - a) * w + lj + kz - 1;
      const double* __restrict__ kr = sk + a * kz;
      for (int b = 0; b < kz; ++b) {
        const double kv = kr[b];
#pragma unroll
        for (int r = 0; r < kCvR; ++r)
          acc[r] = __builtin_fma(kv, row[r * (kCvB / kCvZ) * w - b], acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kCvR; ++r) {
    const int i = x0 + li + r * (kCvB / kCvZ), j = z0 + lj;
    if (i < nx && j < nz) out[(int64_t)m * npix + (int64_t)i * nz + j] = acc[r];
  }
}

hipError_t convolve2d_launch(const double* in, int n_maps, int nx, int nz, const double* ker,
                             int n_ker, int kx, int kz, const double* add, double* out,
                             hipStream_t st) {
  const ConvTiling t = conv_tiling(n_maps, nx, nz);
  const int64_t ker_stride = n_ker == 1 ? 0 : (int64_t)kx * kz;
  hipLaunchKernelGGL(convolve2d_kernel, dim3((unsigned)t.workgroups), dim3(kCvB), 0, st, in, nx, nz,
                     ker, ker_stride, kx, kz, conv_chunk_rows(kx, kz), add, out, (int)t.tiles_x,
                     (int)t.tiles_z);
  return hipGetLastError();
}

}  // namespace rjp
