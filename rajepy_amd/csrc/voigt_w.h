// The complex Faddeeva function w(z) = exp(-z^2) erfc(-i z) for the device, z = u + i a, a >= 0,
// any finite u: (K, L) = (Re w, Im w) to
//   |w_dev - w| <= kVoigtWEps |w|,  kVoigtWEps = 2.0e-15
// -- against the MODULUS, neither part on its own (Re w in a Lorentz wing is a / u times smaller
// than |w|; the Voigt fit of K24 needs both parts against |w| only).  kVoigtWEps is twice the worst
// error of the float64 restatement of this file (tests/voigtfit_ref.py: w_dev, with this header's
// exp_any and sincos_2pi restated too) against mpmath at 50 digits over the grid of
// tools/voigt_w_design.py (worst 9.83e-16; far 8.0e-17, fraction 8.3e-16, the two lattices 9.8e-16
// and 8.5e-16): every a of {0, 1e-300, 1e-12, 1e-6, 1e-3, 0.03, 0.5, 1, 6 and 6 -+ 1e-9, 2 pi -+
// 1e-9, 10, 1e3, 1e6}, > 2000 u in [0, 1e8] each with every
// node and half-node -+ 1 ulp, the lattice switch points -+ 1 ulp and the path boundaries.  The
// factor 2 covers the fma contraction of the device, which NumPy does not share.
//
// It stands beside rrl_voigt.h (Re w alone to 4e-9 for K3 and K6, whose paths and bits do not
// change), per-lane code: no wave-uniform assumption, no LDS, no table in memory.  Three paths by
// d = u^2 + a^2:
//   far      d not < 1e200 (an overflowing or NaN d included): w = (i / sqrt(pi)) / z with z scaled
//            by 1 / max(|u|, a), relative error 1 / (2 d).
//   fraction d >= 49 or a >= 6: the Laplace continued fraction, twelve levels from the bottom,
//            r <- z - (k / 2) / r for k = 12 .. 1 from r = z, w = (i / sqrt(pi)) / r: thirteen
//            divisions.  Worst on the real axis at |z| = 7 (8.6e-16 measured on the circle).
//   lattice  else: the trapezoidal sum of (i / pi) int exp(-t^2) / (z - t) dt with step h = 1/2 plus
//            the pole term of the residue at t = z (Matta and Reichel 1971; Hunter and Regan 1972),
//              w = (i h / pi) sum_n exp(-t_n^2) / (z - t_n) + 2 exp(-z^2) / (1 -+ exp(-2 pi i z / h)),
//            on ONE OF TWO lattices, t_n = n h ("-") or t_n = (n + 1/2) h ("+"): the one whose nodes
//            lie at least h / 4 from u (f = 2 u - rint(2 u), exact; |f| <= 1/4 takes the half-node
//            lattice), so that neither the sum nor the pole term grows near a node and a = 0 works:
//            there the sum is purely imaginary and the pole term's real part is exp(-u^2).  Nodes
//            in pairs +-t_n, 2 z exp(-t_n^2) / (z^2 - t_n^2), fourteen of them (t <= 7:
//            exp(-t^2) < 6e-22 beyond), one division each, and 1 / z for the node 0.  a < 6 < pi / h
//            here, so the pole term is always present (truncation 2 exp(-pi^2 / h^2) = 1.4e-17).
//            exp(-z^2) = exp(-(u - a)(u + a)) (cos 2ua - i sin 2ua); the phases through sincos_2pi
//            (of f, exactly reduced, and of 2ua / 2 pi with |2ua| < 84).
// The operations, in this order, are restated by tests/voigtfit_ref.py: w_dev.
#pragma once
#include "rjp_device.h"

namespace rjp {

constexpr double kVoigtWEps = 2.0e-15;

// exp(-t^2) at the fourteen node pairs of the two lattices: t = (n + 1) / 2 and t = (n + 1/2) / 2
#define RJP_VW_NODES(X)                                                                           \
  X(0.25, 0.7788007830714049, 0.0625, 0.9394130628134758)                                         \
  X(1.0, 0.36787944117144233, 0.5625, 0.569782824730923)                                          \
  X(2.25, 0.10539922456186433, 1.5625, 0.2096113871510978)                                        \
  X(4.0, 0.01831563888873418, 3.0625, 0.04677062238395898)                                        \
  X(6.25, 0.0019304541362277093, 5.0625, 0.006329715427485747)                                    \
  X(9.0, 0.00012340980408667956, 7.5625, 0.0005195746821548384)                                   \
  X(12.25, 4.785117392129009e-06, 10.5625, 2.586810022265412e-05)                                 \
  X(16.0, 1.1253517471925912e-07, 14.0625, 7.811489408304491e-07)                                 \
  X(20.25, 1.6052280551856116e-09, 18.0625, 1.4307241918567688e-08)                               \
  X(25.0, 1.3887943864964021e-11, 22.5625, 1.5893910094516368e-10)                                \
  X(30.25, 7.287724095819692e-14, 27.5625, 1.0709232382508077e-12)                                \
  X(36.0, 2.3195228302435696e-16, 33.0625, 4.37661850287085e-15)                                  \
  X(42.25, 4.4777324417183015e-19, 39.0625, 1.0848552640429378e-17)                               \
  X(49.0, 5.242885663363464e-22, 45.5625, 1.6310139226701858e-20)

__device__ __forceinline__ void voigt_w(double u, double a, double& K, double& L) {
  const double kInvSqrtPi = 0.56418958354775628695;
  const double d = __builtin_fma(u, u, a * a);
  if (!(d < 49.0 && a < 6.0)) {
    if (!(d < 1e200)) {
      const double s = 1.0 / __builtin_fmax(__builtin_fabs(u), a);
      const double us = u * s, as = a * s;
      const double inv = (kInvSqrtPi * s) / __builtin_fma(us, us, as * as);
      K = as * inv;
      L = us * inv;
      return;
    }
    double rr = u, ri = a;
#pragma unroll
    for (int k = 12; k >= 1; --k) {
      const double inv = (0.5 * k) / __builtin_fma(rr, rr, ri * ri);
      rr = __builtin_fma(-rr, inv, u);
      ri = __builtin_fma(ri, inv, a);
    }
    const double inv = kInvSqrtPi / __builtin_fma(rr, rr, ri * ri);
    K = ri * inv;
    L = rr * inv;
    return;
  }
  const double t = 2.0 * u;
  const double f = t - __builtin_rint(t);
  const bool mid = __builtin_fabs(f) <= 0.25;
  const double z2r = (u - a) * (u + a), z2i = 2.0 * (u * a);
  const double z2i2 = z2i * z2i;
  double sr = 0.0, sv = 0.0;
#define RJP_VW_PAIR(T2I, EI, T2M, EM)                                                             \
  {                                                                                               \
    const double dr = z2r - (mid ? T2M : T2I);                                                    \
    const double inv = (mid ? EM : EI) / __builtin_fma(dr, dr, z2i2);                             \
    sr = __builtin_fma(dr, inv, sr);                                                              \
    sv += inv;                                                                                    \
  }
  RJP_VW_NODES(RJP_VW_PAIR)
#undef RJP_VW_PAIR
  const double si = -(z2i * sv);
  double zr = 2.0 * __builtin_fma(u, sr, -(a * si));
  double zi = 2.0 * __builtin_fma(u, si, a * sr);
  if (!mid) {
    const double id = 1.0 / d;
    zr = __builtin_fma(u, id, zr);
    zi = __builtin_fma(-a, id, zi);
  }
  const double kHPi = 0.15915494309189533577;       // h / pi
  const double tr = -(kHPi * zi), ti = kHPi * zr;
  // the pole term 2 exp(-z^2) / (1 -+ E), E = exp(4 pi a) (cos 2 pi f - i sin 2 pi f)
  double sn, cs, sa, ca;
  sincos_2pi(f, sn, cs);
  sincos_2pi(z2i * 0.15915494309189533577, sa, ca);
  const double mag = exp_any(12.566370614359172954 * a);
  const double sm = mid ? mag : -mag;
  const double qr = __builtin_fma(sm, cs, 1.0), qi = -(sm * sn);
  const double g = 2.0 * exp_any(-z2r);
  const double gr = g * ca, gi = -(g * sa);
  const double iq = 1.0 / __builtin_fma(qr, qr, qi * qi);
  K = tr + __builtin_fma(gr, qr, gi * qi) * iq;
  L = ti + __builtin_fma(gi, qr, -(gr * qi)) * iq;
}

}  // namespace rjp
