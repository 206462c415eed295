// What the formal-solution kernels share: K5 (ff_formal.hip), K6 (rrl_formal.hip) and K8
// (ff_formal_sweep.hip) count and weigh a cell's continuum opacity with the code below, and K5 and
// K8 take their tile, their recurrence, their dead-cell and output rules and their host dispatch
// from here -- a sweep's maps are K5's bit for bit because both run these statements.
#pragma once
#include <type_traits>

#include "rjp_host.h"

namespace rjp {

constexpr int kFB = 256;     // threads per workgroup
#ifndef RJP_FORMAL_WAVES
#define RJP_FORMAL_WAVES 4      /* 128-VGPR budget */
#endif

template <int LF> struct FormalTile {
  static constexpr int ZT = LF == 256 ? 8 : 16;   // sightlines per workgroup
  static constexpr int YC = kFB / ZT;             // y-rows per slab
  static constexpr int G = kFB / LF;              // sightline groups
  static constexpr int NZP = ZT / G;              // sightlines per thread
};

// A thread's places in the tile of workgroup blockIdx.x: the ZT sightlines from z0 of row x; LF =
// lanes along the kernel's lane axis (K5: channels, K8: epochs)
template <int LF> struct FormalPlace {
  int x, z0;
  int cy, cz;      // this thread's cell in a slab (phase 1)
  int cb;          // first sightline of this thread (phase 2)
  __device__ __forceinline__ explicit FormalPlace(int nz) {
    constexpr int ZT = FormalTile<LF>::ZT;
    const int ntz = (nz + ZT - 1) / ZT;
    const int tid = threadIdx.x;
    x = (int)blockIdx.x / ntz;
    z0 = ((int)blockIdx.x - x * ntz) * ZT;
    cy = tid / ZT;
    cz = tid % ZT;
    cb = tid / LF * FormalTile<LF>::NZP;
  }
};

template <typename T>
struct FormalFields {
  using value_type = T;
  const T* nd;
  const T* xi;
  const T* temp;
  const T* pf;
  const T* ts;
  const T* em0;
  const double* a0;
  const int32_t* ylo;      // optional occupied y-range per sightline
  const int32_t* yhi;
};

// |a0| of one cell as the scans of the layout form it (ff_scan_kernels.h load_rows / compute_rows):
// the stored tau field, |em0| T^-1.5|-1.35, or (|nd| xi)^2 pf T^-1.5|-1.35; `red` = the cell lies
// in the red jet (the sign of the layout's signed field).
template <typename T, int LAY>
__device__ __forceinline__ double formal_a(const FormalFields<T>& f, int64_t o, int mode, double Tk,
                                           bool& red) {
  if constexpr (LAY == LAY_TAU) {
    const double v = f.a0[o];
    red = signbit_d(v);
    return fabs(v);
  } else if constexpr (LAY == LAY_CMP) {
    const double g = (double)f.em0[o];
    red = signbit_d(g);
    return fabs(g) * tau_weight(Tk, mode);
  } else {
    const double nd = (double)f.nd[o];
    const double n0 = fabs(nd) * (double)f.xi[o];
    red = signbit_d(nd);
    return n0 * n0 * (double)f.pf[o] * tau_weight(Tk, mode);
  }
}

// |a0| chi^2, and the rule for a cell that contributes nothing (NaN: the term is dropped, as
// nansum drops it).  K5 and K8 (ff_formal_sweep.hip) form b through these two, so that a sweep's
// maps are K5's bit for bit.
__device__ __forceinline__ double formal_weigh(double a, double c) { return a * (c * c); }
__device__ __forceinline__ double formal_live(double b) { return b == b ? b : 0.0; }

// b = |a0| chi^2 of one cell, 0 when it contributes nothing.  chi exactly from the bursts (K3's
// cell_line) -- a NaN launch time gives NaN where the cell's jet has bursts (the term is dropped)
// and chi = 1 where it has none (classes.py:232-233).
template <typename T, int LAY, bool BURSTS>
__device__ __forceinline__ double formal_b(const FormalFields<T>& f, int64_t o, int mode,
                                           const BurstsDev& bd, double time_s, double Tk) {
  bool red;
  const double a = formal_a<T, LAY>(f, o, mode, Tk, red);
  double b = a;
  if (BURSTS) b = formal_weigh(a, chi_cell(bd, red, time_s - (double)f.ts[o]));
  return formal_live(b);
}

// The walk, front to back: one cell of optical depth dtau = ctau b and temperature T, with
// om = 1 - e^-dtau.  A dead cell (b == 0) adds T * 0 = 0, not NaN; a sightline without a cell of
// T > 0 (`hot` false) is NaN, as T_avg is.
__device__ __forceinline__ double formal_temp(double b, double Tk) { return b != 0.0 ? Tk : 0.0; }
__device__ __forceinline__ void formal_update(double tk, double om, double& I, double& Th) {
  I = __builtin_fma(tk * om, Th, I);
  Th = __builtin_fma(-Th, om, Th);
}
__device__ __forceinline__ double formal_out(bool hot, double cs, double I) {
  return hot ? cs * I : __builtin_nan("");
}

// ---- what the epoch-lane kernels (K8, K9 = ff_formal_grad.hip) share ---------------------------
// Phase 1 of a slab: the thread's cell (row yy, sightline zz of row x) -> what does not depend on
// the epoch: the signed a (|a0| as formal_a forms it, jet flag in the sign), T and ts; marks the
// sightline hot where T > 0.  A cell outside the tile or the y-range is (0, 0, 0): dead.
template <typename T, int LAY>
__device__ __forceinline__ void formal_stage_cell(const FormalFields<T>& f, int x, int yy, int zz,
                                                  int ye, int ny, int nz, int mode, int* s_hot_cz,
                                                  rjp_d2& at, double& ts) {
  double sa = 0.0, tk = 0.0;
  ts = 0.0;
  if (yy < ye && zz < nz) {
    const int64_t o = ((int64_t)x * ny + yy) * nz + zz;
    tk = (double)f.temp[o];
    if (tk > 0.0) *s_hot_cz = 1;                      // (every writer stores the same value)
    bool red;
    const double a = formal_a<T, LAY>(f, o, mode, tk, red);
    sa = red ? -a : a;
    if (f.ts) ts = (double)f.ts[o];                   // (null without bursts: chi = 1 whatever ts)
  }
  at.x = sa;
  at.y = tk;
}

// One plane of the tile, s_x[epoch lane * 16 + sightline] (a barrier lies between its writes and
// this call): the map rows of the `ne` live epochs, 128-byte runs along z, to row[e * estride +
// sightline], and the epoch's 16 values added in a fixed order (NaN pixels add nothing, as
// nansum) to prow[e * pstride].  Either pointer may be null.  Ends with a barrier.
__device__ __forceinline__ void formal_tile_emit(const double* s_x, int ne, int z0, int nz,
                                                 double* row, int64_t estride, double* prow,
                                                 int64_t pstride) {
  constexpr int ZT = 16;
  const int tid = threadIdx.x;
  if (row) {
    for (int i = tid; i < ne * ZT; i += kFB) {
      const int zz = z0 + i % ZT;
      if (zz < nz) row[(int64_t)(i / ZT) * estride + i % ZT] = s_x[i];
    }
  }
  if (prow && tid < ne) {
    double tot = 0.0;
    for (int zz = 0; zz < ZT; ++zz) {
      const double v = s_x[tid * ZT + zz];
      tot += v == v ? v : 0.0;
    }
    prow[(int64_t)tid * pstride] = tot;
  }
  __syncthreads();
}

// Host: epochs [0, n64) go to blocks of 64 lanes, the tail to blocks of 16 unless it fills more
// than three of them -- the only dead lanes are the last block's.
inline int formal_epochs64(int n_epochs) {
  const int n64 = n_epochs / RJP_WAVE * RJP_WAVE;
  return n_epochs - n64 > 48 ? n_epochs : n64;
}

// Host: the fields as FormalFields<T> and the layout the scans of this model stream, handed to
// go(fields, std::integral_constant<int, LAY>) -- tau layout (f64 only), compact, else wide.  `ts`:
// the launch times the kernel is to see (K8 passes null without bursts).
template <typename T>
FormalFields<T> formal_fields(const rjp_fields* fl, const void* ts) {
  return {(const T*)fl->d_nd, (const T*)fl->d_xi, (const T*)fl->d_temp, (const T*)fl->d_pf,
          (const T*)ts, (const T*)fl->d_em0,
          std::is_same<T, double>::value ? (const double*)fl->d_a0 : nullptr, fl->d_ylo, fl->d_yhi};
}
template <typename Go>
hipError_t formal_dispatch(const rjp_fields* fl, int mode, const void* ts, Go&& go) {
  auto lay = [&](auto f, bool tau) {
    if constexpr (std::is_same<decltype(f), FormalFields<double>>::value)
      if (tau) return go(f, std::integral_constant<int, LAY_TAU>{});
    if (fl->d_em0) return go(f, std::integral_constant<int, LAY_CMP>{});
    return go(f, std::integral_constant<int, LAY_WIDE>{});
  };
  if (fl->dtype == RJP_F64)
    return lay(formal_fields<double>(fl, ts), fl->d_a0 && fl->a0_mode == mode);
  return lay(formal_fields<float>(fl, ts), false);
}

}  // namespace rjp
