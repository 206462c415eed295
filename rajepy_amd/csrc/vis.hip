// K10 (rjp_vis): model visibilities of a stack of maps at arbitrary (u, v) points -- the direct
// Fourier sum, no gridding:
//   V[m, k] = sum_{ix, iz} I[m, ix nz + iz] exp(-2 pi i (a (ix - (nx-1)/2) + b (iz - (nz-1)/2))),
//   a = su[m] u[k], b = sv[m] v[k]   (cycles per cell; a NaN pixel adds nothing).
// The phasor factorises, e^{-2 pi i (a jx + b jz)} = Ex[ix] Ez[iz], so per (map, visibility)
//   W[ix] = sum_iz I[ix, iz] Ez[iz]      real x complex: 2 FMAs per (visibility, pixel), the hot loop
//   V     = sum_ix Ex[ix] W[ix]          nx complex multiply-adds
// and only nx + nz phasors exist per (map, visibility), none of them in memory.
//
// The first stage is a GEMM, [nx x nz] real times [nz x 2 n_vis] with the second operand generated on
// the fly.  A workgroup of 256 threads owns TR = 16 JR x-rows x 64 visibilities of one map and walks
// z in chunks of 16 cells: the chunk of I goes to LDS transposed ([iz][row], NaN -> 0 there), the
// chunk's 16 x 64 phasors Ez are evaluated once (four sincos_2pi per thread) into LDS, and every
// thread keeps JR rows x 4 visibilities x (re, im) accumulators in registers.  Per z-cell a thread
// reads JR / 2 pairs of adjacent rows and 4 phasors (JR / 2 + 4 ds_read_b128) for 8 JR FMAs:
//   JR = 8 (nx > 64): R = 128 rows, 64 accumulators = 128 VGPRs (250 in all), two workgroups per
//           CU; 32 of the 256 LDS-array cycles the four SIMDs' FMAs take; a phasor (~50 VALU) is
//           amortised over 128 rows x 2 FMAs: 0.2 of the hot loop (counted: 2.47 VALU per
//           multiply-add in all, 2.00 of them the FMAs);
//   JR = 4 (nx <= 64): 64 rows, for maps that would leave more than half of a 128-row tile empty.
// LDS images: the 16 lanes a ds_read_b128 serves together differ in their row group and read 256
// contiguous bytes of I (conflict-free; the other lanes read the same addresses: broadcast) or two
// phasor groups 64 bytes apart; rows of I are TR + 2 doubles long (pairs stay 16-byte aligned, the
// 16 z-cells a staging store writes for one row fall into 8 bank groups).  The next chunk's I is
// loaded into registers before this chunk's FMAs (unconditional loads, clamped into the map).
// Second stage, in the same kernel: every (row, visibility) pair of the tile belongs to exactly one
// thread, which evaluates Ex for its pairs in registers and forms its partial sum over its JR rows;
// the 16 row groups of a visibility are 16 adjacent lanes and are combined by a butterfly of
// shuffles.  With one row tile the result is V; with more, the tiles' partials go through the
// workspace and partial_combine_kernel adds them in tile order.  Every sum runs in a fixed order: no
// atomics, the same bits on every call.
// Phase arguments are ONE double product a * (index - centre) (the centre is a half-integer: exact),
// reduced and evaluated by sincos_2pi; no recurrence, no float.
#include "rjp_host.h"

namespace rjp {

constexpr int kVisB = 256;     // threads per workgroup: 16 row groups x 16 visibility groups
constexpr int kVisV = 64;      // visibilities per workgroup (4 per thread)
constexpr int kVisZ = 16;      // z-cells per LDS chunk

static int64_t vis_row_tiles(int nx) {
  const int tr = 16 * vis_rows_per_thread(nx);
  return ((int64_t)nx + tr - 1) / tr;
}

size_t vis_workspace_bytes(int n_maps, int nx, int nz, int n_vis) {
  (void)nz;
  // one complex partial per (map, row tile, visibility); 0 where that does not fit a size_t
  const unsigned __int128 n = (unsigned __int128)n_maps * (unsigned __int128)vis_row_tiles(nx) *
                              (unsigned __int128)n_vis * 16u;
  return n > (unsigned __int128)SIZE_MAX ? 0 : (size_t)n;
}

template <int JR>
__global__ __launch_bounds__(kVisB, 2) void vis_kernel(const double* __restrict__ maps, int nx,
                                                       int nz, const double* __restrict__ su,
                                                       const double* __restrict__ sv,
                                                       const double* __restrict__ u,
                                                       const double* __restrict__ v, int n_vis,
                                                       int nvt, int nrt, double* __restrict__ out) {
  constexpr int TR = 16 * JR;
  constexpr int SI = TR + 2;                       // row stride of the I image (see the head)
  __shared__ rjp_d2 s_I2[kVisZ * SI / 2];          // [iz][row], read as pairs of rows
  double* s_I = reinterpret_cast<double*>(s_I2);
  __shared__ rjp_d2 s_E[kVisZ * kVisV];            // [iz][visibility] = (cos, -sin)
  const int tid = threadIdx.x;
  const int rg = tid & 15, vg = tid >> 4;
  const int vt = (int)(blockIdx.x % (unsigned)nvt);
  const unsigned rest = blockIdx.x / (unsigned)nvt;
  const int rt = (int)(rest % (unsigned)nrt), m = (int)(rest / (unsigned)nrt);
  const int row0 = rt * TR, k0 = vt * kVisV;
  const double cx = 0.5 * (double)(nx - 1), cz = 0.5 * (double)(nz - 1);
  const double* __restrict__ mp = maps + (int64_t)m * nx * nz;
  // this thread's share of a chunk's phasors: visibility k0 + pv at z-cells pz, pz + 4, pz + 8, pz + 12
  const int pv = tid & (kVisV - 1), pz = tid >> 6;
  const double bk = k0 + pv < n_vis ? sv[m] * v[k0 + pv] : 0.0;

  double acc[JR][4][2];
#pragma unroll
  for (int j = 0; j < JR; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[j][q][0] = acc[j][q][1] = 0.0;

  // I: element e = tid + 256 q of a chunk -> (row e / 16, z-cell e % 16): 128 contiguous bytes per
  // row.  The loads of the NEXT chunk are issued before this chunk's FMAs and land in registers
  // meanwhile; addresses are clamped into the map so that they are unconditional (and batched),
  // what lies outside is replaced by 0 when the chunk goes to LDS
  double stage[JR];
  auto fetch = [&](int z0) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < JR; ++q) {
      const int e = tid + kVisB * q;
      const int z = z0 + (e & (kVisZ - 1)), row = row0 + (e >> 4);
      stage[q] = mp[(int64_t)min(row, nx - 1) * nz + min(z, nz - 1)];
    }
  };
  fetch(0);
  for (int z0 = 0; z0 < nz; z0 += kVisZ) {
    __syncthreads();                               // the previous chunk's readers are done
#pragma unroll
    for (int q = 0; q < JR; ++q) {
      const int e = tid + kVisB * q;
      const int iz = e & (kVisZ - 1), r = e >> 4;
      const double val = stage[q];                 // (first touched here: the loads fly until now)
      // nansum: a NaN pixel adds nothing; neither does what lies outside the map
      s_I[iz * SI + r] = (row0 + r < nx && z0 + iz < nz && val == val) ? val : 0.0;
    }
#pragma unroll
    for (int q = 0; q < kVisZ / 4; ++q) {
      // (past the map's last z-cell I is 0 and the phasor too: the inner loop has one trip count)
      const int iz = pz + 4 * q;
      double sn, cs;
      sincos_2pi(bk * ((double)(z0 + iz) - cz), sn, cs);
      rjp_d2 e;
      e.x = z0 + iz < nz ? cs : 0.0;
      e.y = z0 + iz < nz ? -sn : 0.0;
      s_E[iz * kVisV + pv] = e;
    }
    if (z0 + kVisZ < nz) fetch(z0 + kVisZ);
    __syncthreads();
#pragma unroll 2
    for (int iz = 0; iz < kVisZ; ++iz) {
      double iv[JR];
      rjp_d2 ez[4];
#pragma unroll
      for (int j = 0; j < JR; j += 2) {
        const rjp_d2 t = s_I2[(iz * SI + 2 * rg + 16 * j) / 2];
        iv[j] = t.x; iv[j + 1] = t.y;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) ez[q] = s_E[iz * kVisV + vg * 4 + q];
#pragma unroll
      for (int j = 0; j < JR; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc[j][q][0] = __builtin_fma(iv[j], ez[q].x, acc[j][q][0]);
          acc[j][q][1] = __builtin_fma(iv[j], ez[q].y, acc[j][q][1]);
        }
    }
  }

  // V = sum_ix Ex[ix] W[ix] over this thread's rows, then over the 16 row groups (adjacent lanes)
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int k = k0 + vg * 4 + q;
    const double ak = k < n_vis ? su[m] * u[k] : 0.0;
    double pr = 0.0, pi = 0.0;
#pragma unroll
    for (int j = 0; j < JR; ++j) {
      // (a row past nx holds W = 0 and adds an exact zero)
      double sn, cs;
      sincos_2pi(ak * ((double)(row0 + 2 * rg + 32 * (j >> 1) + (j & 1)) - cx), sn, cs);
      const double wr = acc[j][q][0], wi = acc[j][q][1];
      pr = __builtin_fma(cs, wr, pr);
      pr = __builtin_fma(sn, wi, pr);              // Ex = cs - i sn
      pi = __builtin_fma(cs, wi, pi);
      pi = __builtin_fma(-sn, wr, pi);
    }
#pragma unroll
    for (int d = 8; d > 0; d >>= 1) {
      pr += __shfl_xor(pr, d, 16);
      pi += __shfl_xor(pi, d, 16);
    }
    if (rg == 0 && k < n_vis) {
      double* o = out + (((int64_t)m * nrt + rt) * n_vis + k) * 2;
      o[0] = pr;
      o[1] = pi;
    }
  }
}

// out[m][c] = sum over r < n, in that order, of part[(m n + r) per + c]: K10's row tiles of
// complex visibilities (per = 2 n_vis) and K11's k-splits of images (per = nx nz)
__global__ __launch_bounds__(kVisB) void partial_combine_kernel(const double* __restrict__ part,
                                                                int64_t n_maps, int n, int64_t per,
                                                                double* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * kVisB + threadIdx.x; i < n_maps * per;
       i += (int64_t)gridDim.x * kVisB) {
    const int64_t m = i / per, c = i - m * per;
    double s = 0.0;
    for (int r = 0; r < n; ++r) s += part[(m * n + r) * per + c];
    out[i] = s;
  }
}

hipError_t partial_combine_launch(const double* part, int n_maps, int n, int64_t per, double* out,
                                  hipStream_t st) {
  const int64_t nb = ((int64_t)n_maps * per + kVisB - 1) / kVisB;
  hipLaunchKernelGGL(partial_combine_kernel, dim3((unsigned)(nb < 65536 ? nb : 65536)),
                     dim3(kVisB), 0, st, part, (int64_t)n_maps, n, per, out);
  return hipGetLastError();
}

bool vis_grid_ok(int n_maps, int nx, int n_vis) {
  const int64_t nvt = ((int64_t)n_vis + kVisV - 1) / kVisV;
  const unsigned __int128 nb = (unsigned __int128)n_maps * (unsigned __int128)vis_row_tiles(nx) *
                               (unsigned __int128)nvt;
  return nb <= (unsigned __int128)INT32_MAX;
}

hipError_t vis_launch(const double* maps, int n_maps, int nx, int nz, const double* d_su,
                      const double* d_sv, const double* u, const double* v, int n_vis, double* vis,
                      double* part, hipStream_t st) {
  const int nvt = (n_vis + kVisV - 1) / kVisV;
  const int nrt = (int)vis_row_tiles(nx);
  const unsigned nb = (unsigned)((int64_t)n_maps * nrt * nvt);
  double* out = nrt > 1 ? part : vis;
  if (vis_rows_per_thread(nx) == 8)
    hipLaunchKernelGGL(vis_kernel<8>, dim3(nb), dim3(kVisB), 0, st, maps, nx, nz, d_su, d_sv, u, v,
                       n_vis, nvt, nrt, out);
  else
    hipLaunchKernelGGL(vis_kernel<4>, dim3(nb), dim3(kVisB), 0, st, maps, nx, nz, d_su, d_sv, u, v,
                       n_vis, nvt, nrt, out);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess || nrt == 1) return err;
  return partial_combine_launch(part, n_maps, nrt, (int64_t)n_vis * 2, vis, st);
}

}  // namespace rjp
