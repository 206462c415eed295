// K11 (rjp_vis_adjoint): dirty images from visibilities -- the real transpose of K10's direct
// Fourier sum (vis.hip), no gridding:
//   D[m, ix nz + iz] = sum_k w[k] Re( V[m, k] exp(+2 pi i (a (ix - (nx-1)/2) + b (iz - (nz-1)/2))) ),
//   a = su[m] u[k], b = sv[m] v[k]   (cycles per cell; a flagged visibility adds nothing).
// The phasor factorises, e^{+2 pi i (a jx + b jz)} = Ex[k, ix] Ez[k, iz], so per map
//   P[ix, k] = w_k V[m, k] Ex[k, ix]                          one complex product per (row, visibility)
//   D[ix, iz] = sum_k (P_re cos t_kz - P_im sin t_kz)          2 FMAs per (pixel, visibility), real
// a real GEMM [nx x 2K] x [2K x nz] with BOTH operands generated on the fly; nx + nz phasors exist
// per (map, visibility), none of them in memory.
//
// A workgroup of 256 threads (16 row groups x 16 column groups) owns R = 16 JR rows x 128 columns
// of one map's image and one range of visibilities, which it walks in chunks of 16: the chunk's P
// ([k][row]) and Ez ([k][column], stored as (cos, -sin)) go to LDS, every thread keeps JR x 8 real
// accumulators in registers and per visibility reads JR rows of P and 8 columns of Ez (JR + 8
// ds_read_b128) for 16 JR FMAs:
//   JR = 8 (nx > 64): 128 x 128 pixels, 64 accumulators = 128 VGPRs, two workgroups per CU, 64 KiB of
//           LDS each; 16 phasors per thread and chunk against 2048 FMAs;
//   JR = 4 (nx <= 64): 64 rows, for images that would leave more than half of a 128-row tile empty.
// Staging: a thread fills ONE row (column) of the tile for 256 / R (2) visibilities apart, so the
// visibility is the same for a whole wave and the 64 lanes of a store write 1 KiB of consecutive
// LDS.  Every wave holds the chunk's 16 visibilities in registers, one per lane (mod 16), with the
// flag test and the products su u, sv v, w V done once per chunk; a phasor takes its visibility's
// numbers from that lane by v_readlane.  The next chunk's u, v, w and V are loaded (clamped into
// the set) before this chunk's phasors and land during its FMAs.  A visibility outside the
// workgroup's range, or flagged -- a non-finite Re V, Im V, w, or product su u, sv v (non-finite
// exactly when u or v is) -- is staged as P = 0 with the phases 0, so it adds an exact zero to
// every pixel.
// LDS reads: the 16 lanes a ds_read_b128 serves together hold all 16 column groups and read 256
// contiguous bytes of Ez (conflict-free), and two row groups of P 16 bytes apart (broadcast).
// Few tiles (maps x row tiles x column tiles < 256): the visibilities are split over workgroups,
// at least 64 each, the partial images go to the workspace and partial_combine_kernel (vis.hip) adds
// them in split order.  Every sum runs in a fixed order: no atomics, the same bits on every call.
// Phase arguments are ONE double product a * (index - centre) (the centre is a half-integer: exact),
// reduced and evaluated by sincos_2pi; no recurrence, no float.
#include "rjp_host.h"

namespace rjp {

constexpr int kVaB = 256;        // threads per workgroup: 16 row groups x 16 column groups
constexpr int kVaC = 128;        // columns per tile (8 per thread)
constexpr int kVaK = 16;         // visibilities per LDS chunk
constexpr int kVaMinSplit = 64;  // fewest visibilities a k-split is worth
constexpr int kVaFill = 256;     // workgroups the k-split aims at: one per CU

// The tiling rule (tests restate it on the host): row tiles of 128 (nx > 64) or 64 rows, column
// tiles of 128; with T = n_maps x row tiles x column tiles < 256 the visibilities are split
// min(ceil(256 / T), ceil(n_vis / 64)) ways into ranges of a whole number of 16-chunks, and the
// split count is what those ranges need to cover n_vis.
VisAdjointTiling vis_adjoint_tiling(int n_maps, int nx, int nz, int n_vis) {
  VisAdjointTiling t;
  const int tr = 16 * vis_rows_per_thread(nx);
  t.row_tiles = (int)(((int64_t)nx + tr - 1) / tr);
  t.col_tiles = (int)(((int64_t)nz + kVaC - 1) / kVaC);
  const unsigned __int128 all = (unsigned __int128)n_maps * (unsigned __int128)t.row_tiles *
                                (unsigned __int128)t.col_tiles;
  if (all > (unsigned __int128)INT32_MAX) {        // more than one launch takes: refused upstream
    t.k_per_split = ((int64_t)n_vis + kVaK - 1) / kVaK * kVaK;
    t.k_splits = 1;
    t.workgroups = INT64_MAX;
    return t;
  }
  const int64_t tiles = (int64_t)all;
  int64_t ns = 1;
  if (tiles < kVaFill) {
    ns = (kVaFill + tiles - 1) / tiles;
    const int64_t most = ((int64_t)n_vis + kVaMinSplit - 1) / kVaMinSplit;
    if (ns > most) ns = most;
  }
  const int64_t per = ((int64_t)n_vis + ns - 1) / ns;
  t.k_per_split = (per + kVaK - 1) / kVaK * kVaK;
  t.k_splits = (int)(((int64_t)n_vis + t.k_per_split - 1) / t.k_per_split);
  t.workgroups = tiles * t.k_splits;
  return t;
}

size_t vis_adjoint_workspace_bytes(int n_maps, int nx, int nz, int n_vis) {
  const VisAdjointTiling t = vis_adjoint_tiling(n_maps, nx, nz, n_vis);
  // one partial image per (map, k-split); never empty, so that 0 says "does not fit a size_t"
  if (t.k_splits == 1) return 16;
  const unsigned __int128 n = (unsigned __int128)n_maps * (unsigned __int128)t.k_splits *
                              (unsigned __int128)nx * (unsigned __int128)nz * 8u;
  return n > (unsigned __int128)SIZE_MAX ? 0 : (size_t)n;
}

template <int JR>
__global__ __launch_bounds__(kVaB, 2) void vis_adjoint_kernel(
    const double* __restrict__ vis, const double* __restrict__ su, const double* __restrict__ sv,
    const double* __restrict__ u, const double* __restrict__ v, const double* __restrict__ w,
    int n_vis, int64_t kper, int ns, int nx, int nz, int nrt, int nct, double* __restrict__ out) {
  constexpr int R = 16 * JR;
  constexpr int PS = kVaB / R;                     // visibilities of a chunk one pass of P fills
  constexpr int ES = kVaB / kVaC;
  __shared__ rjp_d2 s_P[kVaK * R];                 // [k][row] = w V Ex
  __shared__ rjp_d2 s_E[kVaK * kVaC];              // [k][column] = (cos, -sin)
  const int tid = threadIdx.x;
  const int cg = tid & 15, rg = tid >> 4;
  unsigned rest = blockIdx.x;
  const int ct = (int)(rest % (unsigned)nct);
  rest /= (unsigned)nct;
  const int rt = (int)(rest % (unsigned)nrt);
  rest /= (unsigned)nrt;
  const int sp = (int)(rest % (unsigned)ns), m = (int)(rest / (unsigned)ns);
  const int row0 = rt * R, col0 = ct * kVaC;
  // (64-bit: a range's end and the chunk after the last may lie beyond 2^31)
  const int64_t kbeg = sp * kper, kend = min((int64_t)n_vis, kbeg + kper);
  const double sum = su[m], svm = sv[m];
  const double* __restrict__ vm = vis + (int64_t)m * n_vis * 2;
  // staging: row prow of P and column ecol of Ez, for the visibilities pk0 + PS q and ek0 + ES q of
  // a chunk -- the same ones for every lane of a wave
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int prow = tid & (R - 1), pk0 = wave * 64 / R;
  const int ecol = tid & (kVaC - 1), ek0 = wave * 64 / kVaC;
  const double jx = (double)(row0 + prow) - 0.5 * (double)(nx - 1);
  const double jz = (double)(col0 + ecol) - 0.5 * (double)(nz - 1);

  double acc[JR][8];
#pragma unroll
  for (int j = 0; j < JR; ++j)
#pragma unroll
    for (int c = 0; c < 8; ++c) acc[j][c] = 0.0;

  // Every wave keeps the chunk's 16 visibilities in registers, lane l (mod 16) visibility k0 + l as it
  // is staged -- (a, b, w Re V, w Im V), all 0 when it is flagged or out of range -- and staging
  // takes visibility kl's four numbers from lane kl (v_readlane: kl is the same for the wave).
  // The next chunk's five values are loaded (unconditionally, clamped into the set) before this
  // chunk's phasors and turned into the table after its FMAs.
  const int lk = tid & (kVaK - 1);
  double raw_u, raw_v, raw_w, raw_r, raw_i;
  auto fetch = [&](int64_t k) __attribute__((always_inline)) {
    const int64_t kc = min(k, (int64_t)n_vis - 1);
    raw_u = u[kc];
    raw_v = v[kc];
    raw_w = w ? w[kc] : 1.0;
    raw_r = vm[2 * kc];
    raw_i = vm[2 * kc + 1];
  };
  double ta, tb, tr, ti;
  auto table = [&](int64_t k) __attribute__((always_inline)) {
    const double a = sum * raw_u, b = svm * raw_v;
    const bool ok = k < kend && finite_d(a) && finite_d(b) && finite_d(raw_w) &&
                    finite_d(raw_r) && finite_d(raw_i);
    ta = ok ? a : 0.0;
    tb = ok ? b : 0.0;
    tr = ok ? raw_w * raw_r : 0.0;
    ti = ok ? raw_w * raw_i : 0.0;
  };
  auto lane_of = [](double x, int lane) __attribute__((always_inline)) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), lane),
                            __builtin_amdgcn_readlane(__double2loint(x), lane));
  };
  fetch(kbeg + lk);
  table(kbeg + lk);

  for (int64_t k0 = kbeg; k0 < kend; k0 += kVaK) {
    __syncthreads();                               // the previous chunk's readers are done
    fetch(k0 + kVaK + lk);
#pragma unroll
    for (int q = 0; q < kVaK / PS; ++q) {
      const int kl = pk0 + PS * q;
      const double a = lane_of(ta, kl), pr = lane_of(tr, kl), pi = lane_of(ti, kl);
      double sn, cs;
      sincos_2pi(a * jx, sn, cs);
      rjp_d2 p;                                    // (pr + i pi) (cs + i sn)
      p.x = __builtin_fma(-pi, sn, pr * cs);
      p.y = __builtin_fma(pi, cs, pr * sn);
      s_P[kl * R + prow] = p;
    }
#pragma unroll
    for (int q = 0; q < kVaK / ES; ++q) {
      const int kl = ek0 + ES * q;
      double sn, cs;
      sincos_2pi(lane_of(tb, kl) * jz, sn, cs);
      rjp_d2 e;
      e.x = cs;
      e.y = -sn;
      s_E[kl * kVaC + ecol] = e;
    }
    __syncthreads();
#pragma unroll 2
    for (int kl = 0; kl < kVaK; ++kl) {
      rjp_d2 p[JR], e[8];
#pragma unroll
      for (int j = 0; j < JR; ++j) p[j] = s_P[kl * R + rg + 16 * j];
#pragma unroll
      for (int c = 0; c < 8; ++c) e[c] = s_E[kl * kVaC + cg + 16 * c];
#pragma unroll
      for (int j = 0; j < JR; ++j)
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          acc[j][c] = __builtin_fma(p[j].x, e[c].x, acc[j][c]);
          acc[j][c] = __builtin_fma(p[j].y, e[c].y, acc[j][c]);
        }
    }
    table(k0 + kVaK + lk);
  }

  double* __restrict__ o = out + ((int64_t)m * ns + sp) * nx * nz;
#pragma unroll
  for (int j = 0; j < JR; ++j) {
    const int ix = row0 + rg + 16 * j;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int iz = col0 + cg + 16 * c;
      if (ix < nx && iz < nz) o[(int64_t)ix * nz + iz] = acc[j][c];
    }
  }
}

hipError_t vis_adjoint_launch(const double* vis, int n_maps, int n_vis, const double* d_su,
                              const double* d_sv, const double* u, const double* v, const double* w,
                              int nx, int nz, double* img, double* part, hipStream_t st) {
  const VisAdjointTiling t = vis_adjoint_tiling(n_maps, nx, nz, n_vis);
  const unsigned nb = (unsigned)t.workgroups;
  double* out = t.k_splits > 1 ? part : img;
  if (vis_rows_per_thread(nx) == 8)
    hipLaunchKernelGGL(vis_adjoint_kernel<8>, dim3(nb), dim3(kVaB), 0, st, vis, d_su, d_sv, u, v, w,
                       n_vis, t.k_per_split, t.k_splits, nx, nz, t.row_tiles, t.col_tiles, out);
  else
    hipLaunchKernelGGL(vis_adjoint_kernel<4>, dim3(nb), dim3(kVaB), 0, st, vis, d_su, d_sv, u, v, w,
                       n_vis, t.k_per_split, t.k_splits, nx, nz, t.row_tiles, t.col_tiles, out);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess || t.k_splits == 1) return err;
  // img[m][p] = sum over the k-splits, in split order, of part[m][split][p]
  return partial_combine_launch(part, n_maps, t.k_splits, (int64_t)nx * nz, img, st);
}

}  // namespace rjp
