// K25 (rjp_image_stats, rjp_label_regions, rjp_mask_grow): the three primitives of an automatic
// clean mask -- robust statistics of an image, connected components of a mask, constrained growth
// of a mask -- as integer and order-statistic work on stacks that stay on the device.
// include/rjprt.h holds the definitions; this comment holds the shapes.
//
// Statistics.  A tile is kStTile = 2048 consecutive pixels of a map, one workgroup of 256 threads.
//   launch 1   per tile: count, non-finite count, the smallest and largest key, sum, sum of squares.
//              Thread t takes pixels t, t + 256, ... of the tile in that order (from +0; the squares
//              as fma(x, x, .)); the 256 lane values are folded by halving, s[t] += s[t + h], h =
//              128 .. 1.  That is the fixed order of include/rjprt.h.
//   launch 2   one workgroup per map adds the tiles in tile order, writes everything but the median
//              and the MAD, and sets the select state (rank (count - 1) / 2, empty prefix).
//   12 x 2     radix select on the order-preserving key, the median then the MAD: six digits of 11,
//              11, 11, 11, 11 and 9 bits from the top.  Per digit one launch in which every tile
//              counts, in an LDS histogram with integer atomics, the digit of its counting pixels
//              whose higher bits equal the prefix, and adds the non-empty bins to the map's
//              histogram in global memory with integer atomics; then one workgroup per map picks
//              the bin that holds the rank, extends the prefix, reduces the rank and clears the
//              histogram.  After the sixth digit the prefix IS the key of the answer.  The MAD's
//              passes form fabs(x - median) on the fly from the median in d_stats.
// Workgroups talk to each other only through integer atomics and launch boundaries.
//
// Labels.  A tile is 16 x 64 pixels (x by z), 256 threads with 4 pixels each.
//   launch 1   union-find of the tile in LDS: parent[l] = l on a set pixel, each pixel united with
//              its left, upper (and, eight neighbours, both upper diagonal) neighbours in the tile;
//              then every pixel stores the global index of its local root.  Local and global
//              indices order the pixels of a tile alike, so a root is its set's smallest index.
//   launch 2   one thread per pixel unites it with those of the same four backward neighbours that
//              lie in another tile, on the parents in global memory: atomicMin on a root.
//   launch 3   flatten: label = 1 + root, +1 on the root's counter, the roots counted into d_nreg.
//   launch 4   area = the counter of the pixel's root.
// Parents only ever decrease and stay inside their set, so the smallest index of a region is its
// only possible final root whatever the order of the merges.  Every loop is capped (see rg_find,
// rg_union) and raises the flag word of the workspace instead of spinning.
//
// Growth.  n_iter > 0: a 16 x 64 tile with a halo of kRgHalo = 8 pixels is staged in LDS (seed and
// constraint, 32 x 80 bytes each) and advanced up to 8 steps per launch between two LDS planes; what
// the edge of the staged region gets wrong moves inward one pixel per step and never reaches the
// tile.  The launches ping-pong between d_seed and a plane of the workspace, ending in d_seed.
// n_iter < 0: the constraint is labelled as above, a region is flagged at its root when one of its
// pixels is a seed or next to one, and the flagged regions are added to the seed: two short launches
// after the four of the labelling, no loop of launches.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rjp_host.h"

namespace rjp {

constexpr int kRgThreads = 256;
constexpr int kStTile = 2048;           // pixels per statistics tile
constexpr int kStBins = 2048;           // bins of the widest digit
constexpr int kStPasses = 6;            // digits of 11, 11, 11, 11, 11, 9 bits
constexpr int kRgTX = 16, kRgTZ = 64;   // tile of the labelling and of the growth
constexpr int kRgTile = kRgTX * kRgTZ;
constexpr int kRgHalo = RJP_GROW_HALO;
constexpr int kRgSX = kRgTX + 2 * kRgHalo, kRgSZ = kRgTZ + 2 * kRgHalo;
constexpr size_t kRgHeader = 256;       // the flag word lives in the first bytes of a workspace

struct StPart {                         // one tile's partial
  int64_t count, nonfinite;
  uint64_t kmin, kmax;
  double sum, sumsq;
};
struct StState {                        // the select state of a map
  uint64_t prefix;
  int64_t rank, count, pad_;
};

static int64_t st_tiles(int nx, int nz) { return ((int64_t)nx * nz + kStTile - 1) / kStTile; }
static int64_t rg_tiles(int nx, int nz) {
  return (int64_t)((nx + kRgTX - 1) / kRgTX) * ((nz + kRgTZ - 1) / kRgTZ);
}

int64_t image_stats_workgroups(int n_maps, int nx, int nz) { return st_tiles(nx, nz) * n_maps; }
int64_t regions_workgroups(int n_maps, int nx, int nz) { return rg_tiles(nx, nz) * n_maps; }

size_t image_stats_workspace_bytes(int n_maps, int nx, int nz) {
  return (size_t)n_maps * (sizeof(StState) + kStBins * sizeof(uint32_t) +
                           (size_t)st_tiles(nx, nz) * sizeof(StPart));
}
static size_t rg_plane4(int n_maps, int nx, int nz) { return (size_t)n_maps * nx * nz * 4; }
static size_t rg_plane1(int n_maps, int nx, int nz) {
  return ((size_t)n_maps * nx * nz + 7) / 8 * 8;
}
size_t label_regions_workspace_bytes(int n_maps, int nx, int nz) {
  return kRgHeader + 2 * rg_plane4(n_maps, nx, nz);
}
size_t mask_grow_workspace_bytes(int n_maps, int nx, int nz) {
  return kRgHeader + rg_plane1(n_maps, nx, nz) + 3 * rg_plane4(n_maps, nx, nz);
}

// ---- statistics ---------------------------------------------------------------------------------
// IEEE total order on the finite doubles (and +-inf) as unsigned order: -0.0 < +0.0
static __device__ __forceinline__ uint64_t st_key(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
static __device__ __forceinline__ double st_val(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

__global__ __launch_bounds__(kRgThreads) void stats_tile_kernel(
    const double* __restrict__ img, const uint8_t* __restrict__ mask, int mask_per_map, int sense,
    int64_t npix, StPart* __restrict__ part) {
  __shared__ double ss[kRgThreads], qq[kRgThreads];
  __shared__ uint64_t mn[kRgThreads], mx[kRgThreads];
  __shared__ int cn[kRgThreads], nn[kRgThreads];
  const int tid = threadIdx.x, m = blockIdx.y;
  const double* __restrict__ x = img + (int64_t)m * npix;
  const uint8_t* __restrict__ mk = mask ? mask + (mask_per_map ? (int64_t)m * npix : 0) : nullptr;
  double s = 0.0, q = 0.0;
  uint64_t kmin = ~0ull, kmax = 0ull;
  int cnt = 0, nf = 0;
  for (int i = 0; i < kStTile / kRgThreads; ++i) {
    const int64_t p = (int64_t)blockIdx.x * kStTile + i * kRgThreads + tid;
    if (p >= npix) break;
    if (mk && ((mk[p] != 0) != (sense != 0))) continue;
    const double v = x[p];
    if (__builtin_isfinite(v)) {
      ++cnt;
      s += v;
      q = __builtin_fma(v, v, q);
      const uint64_t k = st_key(v);
      kmin = k < kmin ? k : kmin;
      kmax = k > kmax ? k : kmax;
    } else {
      ++nf;
    }
  }
  ss[tid] = s, qq[tid] = q, mn[tid] = kmin, mx[tid] = kmax, cn[tid] = cnt, nn[tid] = nf;
  for (int h = kRgThreads / 2; h >= 1; h >>= 1) {
    __syncthreads();
    if (tid < h) {
      ss[tid] += ss[tid + h];
      qq[tid] += qq[tid + h];
      mn[tid] = mn[tid + h] < mn[tid] ? mn[tid + h] : mn[tid];
      mx[tid] = mx[tid + h] > mx[tid] ? mx[tid + h] : mx[tid];
      cn[tid] += cn[tid + h];
      nn[tid] += nn[tid + h];
    }
  }
  if (tid == 0) {
    StPart o;
    o.count = cn[0], o.nonfinite = nn[0], o.kmin = mn[0], o.kmax = mx[0], o.sum = ss[0],
    o.sumsq = qq[0];
    part[(int64_t)m * gridDim.x + blockIdx.x] = o;
  }
}

// one workgroup per map: the tiles in tile order, the select state, a cleared histogram
__global__ __launch_bounds__(kRgThreads) void stats_final_kernel(
    const StPart* __restrict__ part, int64_t n_tiles, double* __restrict__ stats,
    StState* __restrict__ state, uint32_t* __restrict__ hist) {
  const int m = blockIdx.x;
  for (int b = threadIdx.x; b < kStBins; b += kRgThreads) hist[(int64_t)m * kStBins + b] = 0u;
  if (threadIdx.x != 0) return;
  const StPart* __restrict__ p = part + (int64_t)m * n_tiles;
  int64_t count = 0, nf = 0;
  uint64_t kmin = ~0ull, kmax = 0ull;
  double s = 0.0, q = 0.0;
  for (int64_t t = 0; t < n_tiles; ++t) {
    count += p[t].count;
    nf += p[t].nonfinite;
    kmin = p[t].kmin < kmin ? p[t].kmin : kmin;
    kmax = p[t].kmax > kmax ? p[t].kmax : kmax;
    s = t == 0 ? p[t].sum : s + p[t].sum;
    q = t == 0 ? p[t].sumsq : q + p[t].sumsq;
  }
  const double nan = __builtin_nan("");
  double* __restrict__ o = stats + (int64_t)m * 8;
  o[0] = (double)count;
  o[1] = (double)nf;
  o[2] = count ? st_val(kmin) : nan;
  o[3] = count ? st_val(kmax) : nan;
  o[4] = nan;
  o[5] = nan;
  o[6] = count ? s : 0.0;
  o[7] = count ? q : 0.0;
  StState st;
  st.prefix = 0ull, st.rank = count ? (count - 1) / 2 : 0, st.count = count, st.pad_ = 0;
  state[m] = st;
}

static __device__ __forceinline__ int st_shift(int pass) { return pass < 5 ? 53 - 11 * pass : 0; }
static __device__ __forceinline__ int st_bits(int pass) { return pass < 5 ? 11 : 9; }

// `stage` 0: the values themselves; 1: fabs(x - median), the median read from d_stats
__global__ __launch_bounds__(kRgThreads) void stats_hist_kernel(
    const double* __restrict__ img, const uint8_t* __restrict__ mask, int mask_per_map, int sense,
    int64_t npix, const double* __restrict__ stats, const StState* __restrict__ state,
    uint32_t* __restrict__ hist, int pass, int stage) {
  __shared__ uint32_t h[kStBins];
  const int tid = threadIdx.x, m = blockIdx.y;
  const StState st = state[m];
  if (st.count == 0) return;                       // (the whole workgroup)
  for (int b = tid; b < kStBins; b += kRgThreads) h[b] = 0u;
  __syncthreads();
  const double* __restrict__ x = img + (int64_t)m * npix;
  const uint8_t* __restrict__ mk = mask ? mask + (mask_per_map ? (int64_t)m * npix : 0) : nullptr;
  const double med = stage ? stats[(int64_t)m * 8 + 4] : 0.0;
  const int shift = st_shift(pass), bits = st_bits(pass);
  for (int i = 0; i < kStTile / kRgThreads; ++i) {
    const int64_t p = (int64_t)blockIdx.x * kStTile + i * kRgThreads + tid;
    if (p >= npix) break;
    if (mk && ((mk[p] != 0) != (sense != 0))) continue;
    double v = x[p];
    if (!__builtin_isfinite(v)) continue;
    if (stage) v = __builtin_fabs(v - med);
    const uint64_t k = st_key(v);
    if (pass == 0 || (k >> (shift + bits)) == st.prefix)
      atomicAdd(&h[(uint32_t)(k >> shift) & ((1u << bits) - 1u)], 1u);
  }
  __syncthreads();
  uint32_t* __restrict__ g = hist + (int64_t)m * kStBins;
  for (int b = tid; b < kStBins; b += kRgThreads)
    if (h[b]) atomicAdd(&g[b], h[b]);
}

// one workgroup per map: the bin that holds the rank
__global__ __launch_bounds__(kRgThreads) void stats_pick_kernel(
    double* __restrict__ stats, StState* __restrict__ state, uint32_t* __restrict__ hist, int pass,
    int stage) {
  __shared__ uint32_t h[kStBins];
  __shared__ uint64_t part[kRgThreads];
  constexpr int PER = kStBins / kRgThreads;
  const int tid = threadIdx.x, m = blockIdx.x;
  uint32_t* __restrict__ g = hist + (int64_t)m * kStBins;
  for (int b = tid; b < kStBins; b += kRgThreads) {
    h[b] = g[b];
    g[b] = 0u;
  }
  __syncthreads();
  uint64_t s = 0;
  for (int j = 0; j < PER; ++j) s += h[tid * PER + j];
  part[tid] = s;
  __syncthreads();
  if (tid != 0) return;
  StState st = state[m];
  if (st.count == 0) return;
  const uint64_t r = (uint64_t)st.rank;
  uint64_t c = 0;
  int chunk = 0;
  while (chunk < kRgThreads - 1 && c + part[chunk] <= r) c += part[chunk++];
  int d = chunk * PER;
  while (d < chunk * PER + PER - 1 && c + h[d] <= r) c += h[d++];
  st.prefix = (st.prefix << st_bits(pass)) | (uint64_t)d;
  st.rank = (int64_t)(r - c);
  if (pass == kStPasses - 1) {
    stats[(int64_t)m * 8 + 4 + stage] = st_val(st.prefix);
    st.prefix = 0ull;
    st.rank = (st.count - 1) / 2;
  }
  state[m] = st;
}

hipError_t image_stats_launch(const double* img, int n_maps, int nx, int nz, const uint8_t* mask,
                              int n_mask, int sense, double* stats, void* work, hipStream_t st) {
  const int64_t npix = (int64_t)nx * nz, n_tiles = st_tiles(nx, nz);
  StState* state = (StState*)work;
  uint32_t* hist = (uint32_t*)(state + n_maps);
  StPart* part = (StPart*)(hist + (size_t)n_maps * kStBins);
  const int per_map = n_mask == n_maps && n_maps > 1 ? 1 : 0;
  const dim3 grid((unsigned)n_tiles, (unsigned)n_maps), blk(kRgThreads);
  hipLaunchKernelGGL(stats_tile_kernel, grid, blk, 0, st, img, mask, per_map, sense, npix, part);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(stats_final_kernel, dim3((unsigned)n_maps), blk, 0, st, part, n_tiles, stats,
                     state, hist);
  if (hipError_t e = hipGetLastError()) return e;
  for (int stage = 0; stage < 2; ++stage)
    for (int pass = 0; pass < kStPasses; ++pass) {
      hipLaunchKernelGGL(stats_hist_kernel, grid, blk, 0, st, img, mask, per_map, sense, npix,
                         stats, state, hist, pass, stage);
      if (hipError_t e = hipGetLastError()) return e;
      hipLaunchKernelGGL(stats_pick_kernel, dim3((unsigned)n_maps), blk, 0, st, stats, state, hist,
                         pass, stage);
      if (hipError_t e = hipGetLastError()) return e;
    }
  return hipSuccess;
}

// ---- labels -------------------------------------------------------------------------------------
// The parents live in LDS (SCOPE = workgroup) or in global memory (SCOPE = agent); every access to
// them is an integer atomic of that scope, so no thread works on a value the compiler kept.
template <int SCOPE>
static __device__ __forceinline__ int rg_load(int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE);
}

// The root of i.  Terminates: par[j] <= j for every set pixel at all times (a parent is set once
// to j and afterwards only lowered by atomic minima with indices >= 0), so the indices visited
// decrease strictly until par[j] == j: at most `cap` = nx nz steps.  The cap is a second line of
// defence: when it is hit the flag is raised and the walk ends where it stands.
template <int SCOPE>
static __device__ int rg_find(int* par, int i, int64_t cap, int* flag) {
  for (int64_t n = 0; n <= cap; ++n) {
    const int p = rg_load<SCOPE>(par + i);
    if (p == i) return i;
    i = p;
  }
  atomicOr(flag, 1);
  return i;
}

// Unites the sets of a and b.  Terminates: a retry happens only when the atomic minimum met a
// parent that another thread had lowered below a in the meantime; the retry goes on from that
// lower index (and b), so the larger of the two roots decreases strictly from retry to retry and
// is bounded below by 0: at most `cap` retries.  Capped all the same, with the flag.
template <int SCOPE>
static __device__ void rg_union(int* par, int a, int b, int64_t cap, int* flag) {
  for (int64_t n = 0; n <= cap; ++n) {
    a = rg_find<SCOPE>(par, a, cap, flag);
    b = rg_find<SCOPE>(par, b, cap, flag);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(par + a, b, __ATOMIC_RELAXED, SCOPE);
    if (old == a) return;            // a was still a root and now hangs under b
    a = old;                         // a had been hung under `old` < a: unite that set with b's
  }
  atomicOr(flag, 1);
}

__global__ __launch_bounds__(kRgThreads) void label_tile_kernel(
    const uint8_t* __restrict__ mask, int mask_per_map, int nx, int nz, int conn,
    int32_t* __restrict__ L, int64_t cap, int* flag) {
  __shared__ int par[kRgTile];
  const int tid = threadIdx.x, m = blockIdx.z;
  const int x0 = blockIdx.y * kRgTX, z0 = blockIdx.x * kRgTZ;
  const int64_t npix = (int64_t)nx * nz;
  const uint8_t* __restrict__ mk = mask + (mask_per_map ? (int64_t)m * npix : 0);
  int32_t* __restrict__ Lm = L + (int64_t)m * npix;
  constexpr int PER = kRgTile / kRgThreads;
  bool fg[PER];
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int l = i * kRgThreads + tid, gx = x0 + l / kRgTZ, gz = z0 + l % kRgTZ;
    fg[i] = gx < nx && gz < nz && mk[(int64_t)gx * nz + gz] != 0;
    par[l] = fg[i] ? l : -1;
  }
  __syncthreads();
  constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    if (!fg[i]) continue;
    const int l = i * kRgThreads + tid, lx = l / kRgTZ, lz = l % kRgTZ;
    // (a background pixel keeps -1 for good: minima are only ever taken on set pixels)
    if (lz > 0 && rg_load<WG>(par + l - 1) >= 0) rg_union<WG>(par, l, l - 1, cap, flag);
    if (lx > 0 && rg_load<WG>(par + l - kRgTZ) >= 0) rg_union<WG>(par, l, l - kRgTZ, cap, flag);
    if (conn == 2 && lx > 0) {
      if (lz > 0 && rg_load<WG>(par + l - kRgTZ - 1) >= 0)
        rg_union<WG>(par, l, l - kRgTZ - 1, cap, flag);
      if (lz < kRgTZ - 1 && rg_load<WG>(par + l - kRgTZ + 1) >= 0)
        rg_union<WG>(par, l, l - kRgTZ + 1, cap, flag);
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const int l = i * kRgThreads + tid, gx = x0 + l / kRgTZ, gz = z0 + l % kRgTZ;
    if (gx >= nx || gz >= nz) continue;
    int32_t out = -1;
    if (fg[i]) {
      const int r = rg_find<WG>(par, l, cap, flag);
      out = (int32_t)((int64_t)(x0 + r / kRgTZ) * nz + z0 + r % kRgTZ);
    }
    Lm[(int64_t)gx * nz + gz] = out;
  }
}

// one thread per pixel: its backward neighbours in OTHER tiles
__global__ __launch_bounds__(kRgThreads) void label_merge_kernel(int32_t* __restrict__ L, int nx,
                                                                 int nz, int conn, int64_t cap,
                                                                 int* flag) {
  const int64_t npix = (int64_t)nx * nz;
  const int64_t p = (int64_t)blockIdx.x * kRgThreads + threadIdx.x;
  if (p >= npix) return;
  int* Lm = L + (int64_t)blockIdx.y * npix;
  constexpr int AG = __HIP_MEMORY_SCOPE_AGENT;
  if (rg_load<AG>(Lm + p) < 0) return;
  const int ix = (int)(p / nz), iz = (int)(p - (int64_t)ix * nz);
  const int lx = ix % kRgTX, lz = iz % kRgTZ;
  if (iz > 0 && lz == 0 && rg_load<AG>(Lm + p - 1) >= 0)
    rg_union<AG>(Lm, (int)p, (int)(p - 1), cap, flag);
  if (ix > 0 && lx == 0 && rg_load<AG>(Lm + p - nz) >= 0)
    rg_union<AG>(Lm, (int)p, (int)(p - nz), cap, flag);
  if (conn == 2 && ix > 0) {
    if (iz > 0 && (lx == 0 || lz == 0) && rg_load<AG>(Lm + p - nz - 1) >= 0)
      rg_union<AG>(Lm, (int)p, (int)(p - nz - 1), cap, flag);
    if (iz < nz - 1 && (lx == 0 || lz == kRgTZ - 1) && rg_load<AG>(Lm + p - nz + 1) >= 0)
      rg_union<AG>(Lm, (int)p, (int)(p - nz + 1), cap, flag);
  }
}

// L is only read here: label = 1 + root; `cnt` (or nullptr) +1 at the root; `nreg` (or nullptr)
__global__ __launch_bounds__(kRgThreads) void label_flatten_kernel(
    int32_t* __restrict__ L, int64_t npix, int32_t* __restrict__ label, int32_t* __restrict__ cnt,
    int32_t* __restrict__ nreg, int64_t cap, int* flag) {
  const int64_t p = (int64_t)blockIdx.x * kRgThreads + threadIdx.x;
  const int64_t base = (int64_t)blockIdx.y * npix;
  bool root = false;
  if (p < npix) {
    int32_t out = 0;
    if (L[base + p] >= 0) {
      const int r = rg_find<__HIP_MEMORY_SCOPE_AGENT>(L + base, (int)p, cap, flag);
      out = r + 1;
      root = r == (int)p;
      if (cnt) atomicAdd(cnt + base + r, 1);
    }
    label[base + p] = out;
  }
  const int n = __syncthreads_count(root);
  if (nreg && threadIdx.x == 0 && n) atomicAdd(nreg + blockIdx.y, n);
}

__global__ __launch_bounds__(kRgThreads) void label_area_kernel(const int32_t* __restrict__ label,
                                                                const int32_t* __restrict__ cnt,
                                                                int64_t npix,
                                                                int32_t* __restrict__ area) {
  const int64_t p = (int64_t)blockIdx.x * kRgThreads + threadIdx.x;
  if (p >= npix) return;
  const int64_t base = (int64_t)blockIdx.y * npix;
  const int32_t l = label[base + p];
  area[base + p] = l ? cnt[base + l - 1] : 0;
}

// the four launches; `cnt` is needed with `area`, `area` and `nreg` may be nullptr
static hipError_t label_core(const uint8_t* mask, int per_map, int n_maps, int nx, int nz, int conn,
                             int32_t* L, int32_t* label, int32_t* cnt, int32_t* area,
                             int32_t* nreg, int* flag, hipStream_t st) {
  const int64_t npix = (int64_t)nx * nz;
  const dim3 blk(kRgThreads);
  const dim3 tiles((unsigned)((nz + kRgTZ - 1) / kRgTZ), (unsigned)((nx + kRgTX - 1) / kRgTX),
                   (unsigned)n_maps);
  const dim3 pix((unsigned)((npix + kRgThreads - 1) / kRgThreads), (unsigned)n_maps);
  hipLaunchKernelGGL(label_tile_kernel, tiles, blk, 0, st, mask, per_map, nx, nz, conn, L, npix,
                     flag);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(label_merge_kernel, pix, blk, 0, st, L, nx, nz, conn, npix, flag);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(label_flatten_kernel, pix, blk, 0, st, L, npix, label, area ? cnt : nullptr,
                     nreg, npix, flag);
  if (hipError_t e = hipGetLastError()) return e;
  if (area) {
    hipLaunchKernelGGL(label_area_kernel, pix, blk, 0, st, label, cnt, npix, area);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

hipError_t label_regions_launch(const uint8_t* mask, int n_mask, int n_maps, int nx, int nz,
                                int conn, int32_t* label, int32_t* area, int32_t* nreg, void* work,
                                hipStream_t st) {
  const size_t plane = rg_plane4(n_maps, nx, nz);
  int* flag = (int*)work;
  int32_t* L = (int32_t*)((char*)work + kRgHeader);
  int32_t* cnt = (int32_t*)((char*)work + kRgHeader + plane);
  if (hipError_t e = hipMemsetAsync(work, 0, kRgHeader, st)) return e;
  if (area)
    if (hipError_t e = hipMemsetAsync(cnt, 0, plane, st)) return e;
  if (hipError_t e = hipMemsetAsync(nreg, 0, (size_t)n_maps * 4, st)) return e;
  return label_core(mask, n_mask == n_maps && n_maps > 1, n_maps, nx, nz, conn, L, label, cnt, area,
                    nreg, flag, st);
}

// ---- growth -------------------------------------------------------------------------------------
static __device__ __forceinline__ bool rg_near(const uint8_t* a, int sx, int sz, int SX, int SZ,
                                               int conn) {
  bool v = (sz > 0 && a[sx * SZ + sz - 1]) || (sz < SZ - 1 && a[sx * SZ + sz + 1]) ||
           (sx > 0 && a[(sx - 1) * SZ + sz]) || (sx < SX - 1 && a[(sx + 1) * SZ + sz]);
  if (conn == 2 && !v)
    v = (sx > 0 && sz > 0 && a[(sx - 1) * SZ + sz - 1]) ||
        (sx > 0 && sz < SZ - 1 && a[(sx - 1) * SZ + sz + 1]) ||
        (sx < SX - 1 && sz > 0 && a[(sx + 1) * SZ + sz - 1]) ||
        (sx < SX - 1 && sz < SZ - 1 && a[(sx + 1) * SZ + sz + 1]);
  return v;
}

// `steps` (1 .. kRgHalo) steps of src -> dst; both are [n_maps][nx nz], src is only read
__global__ __launch_bounds__(kRgThreads) void grow_steps_kernel(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const uint8_t* __restrict__ con,
    int con_per_map, int nx, int nz, int steps, int conn) {
  constexpr int N = kRgSX * kRgSZ;
  __shared__ uint8_t a[2][N], c[N];
  const int tid = threadIdx.x, m = blockIdx.z;
  const int x0 = blockIdx.y * kRgTX, z0 = blockIdx.x * kRgTZ;
  const int64_t npix = (int64_t)nx * nz;
  const uint8_t* __restrict__ s = src + (int64_t)m * npix;
  const uint8_t* __restrict__ k = con + (con_per_map ? (int64_t)m * npix : 0);
  for (int i = tid; i < N; i += kRgThreads) {
    const int gx = x0 - kRgHalo + i / kRgSZ, gz = z0 - kRgHalo + i % kRgSZ;
    const bool in = gx >= 0 && gx < nx && gz >= 0 && gz < nz;
    const int64_t g = (int64_t)gx * nz + gz;
    a[0][i] = in && s[g] != 0;
    c[i] = in && k[g] != 0;
  }
  __syncthreads();
  int cur = 0;
  for (int step = 0; step < steps; ++step) {
    for (int i = tid; i < N; i += kRgThreads) {
      uint8_t v = a[cur][i];
      if (!v && c[i]) v = rg_near(a[cur], i / kRgSZ, i % kRgSZ, kRgSX, kRgSZ, conn);
      a[cur ^ 1][i] = v;
    }
    __syncthreads();
    cur ^= 1;
  }
  for (int l = tid; l < kRgTile; l += kRgThreads) {
    const int lx = l / kRgTZ, lz = l % kRgTZ, gx = x0 + lx, gz = z0 + lz;
    if (gx < nx && gz < nz)
      dst[(int64_t)m * npix + (int64_t)gx * nz + gz] = a[cur][(lx + kRgHalo) * kRgSZ + lz + kRgHalo];
  }
}

// a constraint pixel that is a seed or next to one flags its region at the root
// (`label_per_map` 0: one plane of labels, of a constraint all maps share)
__global__ __launch_bounds__(kRgThreads) void grow_mark_kernel(
    const uint8_t* __restrict__ seed, const int32_t* __restrict__ label, int label_per_map, int nx,
    int nz, int conn, int32_t* __restrict__ hit) {
  const int64_t npix = (int64_t)nx * nz;
  const int64_t p = (int64_t)blockIdx.x * kRgThreads + threadIdx.x;
  if (p >= npix) return;
  const int64_t base = (int64_t)blockIdx.y * npix;
  const int32_t l = label[(label_per_map ? base : 0) + p];
  if (!l) return;
  const uint8_t* __restrict__ s = seed + base;
  const int ix = (int)(p / nz), iz = (int)(p - (int64_t)ix * nz);
  bool v = s[p] || (iz > 0 && s[p - 1]) || (iz < nz - 1 && s[p + 1]) || (ix > 0 && s[p - nz]) ||
           (ix < nx - 1 && s[p + nz]);
  if (conn == 2 && !v)
    v = (ix > 0 && iz > 0 && s[p - nz - 1]) || (ix > 0 && iz < nz - 1 && s[p - nz + 1]) ||
        (ix < nx - 1 && iz > 0 && s[p + nz - 1]) || (ix < nx - 1 && iz < nz - 1 && s[p + nz + 1]);
  if (v) atomicOr(hit + base + l - 1, 1);
}

__global__ __launch_bounds__(kRgThreads) void grow_apply_kernel(uint8_t* __restrict__ seed,
                                                                const int32_t* __restrict__ label,
                                                                int label_per_map,
                                                                const int32_t* __restrict__ hit,
                                                                int64_t npix) {
  const int64_t p = (int64_t)blockIdx.x * kRgThreads + threadIdx.x;
  if (p >= npix) return;
  const int64_t base = (int64_t)blockIdx.y * npix;
  const int32_t l = label[(label_per_map ? base : 0) + p];
  if (l && hit[base + l - 1]) seed[base + p] = 1;
}

hipError_t mask_grow_launch(uint8_t* seed, const uint8_t* con, int n_mask, int n_maps, int nx,
                            int nz, int n_iter, int conn, void* work, hipStream_t st) {
  const int64_t npix = (int64_t)nx * nz;
  const size_t p1 = rg_plane1(n_maps, nx, nz), p4 = rg_plane4(n_maps, nx, nz);
  const int per_map = n_mask == n_maps && n_maps > 1 ? 1 : 0;
  int* flag = (int*)work;
  uint8_t* other = (uint8_t*)work + kRgHeader;
  if (hipError_t e = hipMemsetAsync(work, 0, kRgHeader, st)) return e;
  if (n_iter == 0) return hipSuccess;
  const dim3 blk(kRgThreads);
  if (n_iter > 0) {
    const dim3 tiles((unsigned)((nz + kRgTZ - 1) / kRgTZ), (unsigned)((nx + kRgTX - 1) / kRgTX),
                     (unsigned)n_maps);
    const int launches = (n_iter + kRgHalo - 1) / kRgHalo;
    uint8_t *src = seed, *dst = other;
    if (launches & 1) {          // an odd number of hops has to start from the workspace's plane
      if (hipError_t e = hipMemcpyAsync(other, seed, (size_t)n_maps * npix,
                                        hipMemcpyDeviceToDevice, st))
        return e;
      src = other, dst = seed;
    }
    for (int i = 0, left = n_iter; i < launches; ++i, left -= kRgHalo) {
      hipLaunchKernelGGL(grow_steps_kernel, tiles, blk, 0, st, src, dst, con, per_map, nx, nz,
                         left < kRgHalo ? left : kRgHalo, conn);
      if (hipError_t e = hipGetLastError()) return e;
      uint8_t* t = src;
      src = dst, dst = t;
    }
    return hipSuccess;
  }
  // a constraint that all maps share is labelled once; the flags are per map either way
  const int n_lab = per_map ? n_maps : 1;
  int32_t* L = (int32_t*)((char*)work + kRgHeader + p1);
  int32_t* label = (int32_t*)((char*)L + p4);
  int32_t* hit = (int32_t*)((char*)label + p4);
  if (hipError_t e = hipMemsetAsync(hit, 0, p4, st)) return e;
  if (hipError_t e = label_core(con, per_map, n_lab, nx, nz, conn, L, label, nullptr, nullptr,
                                nullptr, flag, st))
    return e;
  const dim3 pix((unsigned)((npix + kRgThreads - 1) / kRgThreads), (unsigned)n_maps);
  hipLaunchKernelGGL(grow_mark_kernel, pix, blk, 0, st, seed, label, per_map, nx, nz, conn,
                     hit);
  if (hipError_t e = hipGetLastError()) return e;
  hipLaunchKernelGGL(grow_apply_kernel, pix, blk, 0, st, seed, label, per_map, hit, npix);
  return hipGetLastError();
}

}  // namespace rjp
