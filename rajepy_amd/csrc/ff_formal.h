// The tile of the formal-solution kernels and a cell's free-free optical-depth factor b: K5
// (ff_formal.hip), K6 (rrl_formal.hip) and K8 (ff_formal_sweep.hip) include this header, so that
// all three count and weigh a cell's continuum opacity with the same code.
#pragma once
#include "rjp_host.h"

namespace rjp {

constexpr int kFB = 256;     // threads per workgroup

template <int LF> struct FormalTile {
  static constexpr int ZT = LF == 256 ? 8 : 16;   // sightlines per workgroup
  static constexpr int YC = kFB / ZT;             // y-rows per slab
  static constexpr int G = kFB / LF;              // sightline groups
  static constexpr int NZP = ZT / G;              // sightlines per thread
};

template <typename T>
struct FormalFields {
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

}  // namespace rjp
