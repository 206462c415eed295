// check_convolve2d and check_msclean of rajepy_amd/csrc/rjp_args.h -- the pure argument checks of
// rjp_convolve2d and rjp_msclean -- driven from a plain C++ program (no HIP): one line
// "case<TAB>status<TAB>message" per case, in the order the checks refuse;
// tests/test_msclean_reference_cpu.py holds the lines to the messages that tests/test_gpu_msclean.py
// sees from the library.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>

#include "rjp_args.h"

namespace A = rjp_args;

static double* const kD = (double*)0x1000;      // stand for device pointers: never dereferenced
static int32_t* const kI = (int32_t*)0x2000;

struct Conv {
  const double *in = kD, *ker = kD, *out = kD;
  int n_maps = 2, nx = 5, nz = 3, n_ker = 1, kx = 3, kz = 5;
};

static void put(const char* name, const Conv& a) {
  std::string m;
  const int r = A::check_convolve2d(a.in, a.n_maps, a.nx, a.nz, a.ker, a.n_ker, a.kx, a.kz, a.out, m);
  std::printf("%s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

struct Ms {
  const double *res = kD, *xpsf = kD, *cflux = kD;
  const int32_t *cpix = kI, *cscale = kI, *ncomp = kI;
  int n_maps = 2, n_s = 3, nx = 5, nz = 3, n_psf = 1, px = 9, pz = 5, n_iter = 4;
  double weight[6] = {1.0, 0.5, 0.0, 2.0, 0.0, 0.25}, thresh[2] = {0.0, 1e-3}, gain = 0.1;
  bool null_weight = false, null_thresh = false;
};

static void put(const char* name, const Ms& a) {
  std::string m;
  const int r = A::check_msclean(a.res, a.n_maps, a.n_s, a.nx, a.nz, a.xpsf, a.n_psf, a.px, a.pz,
                                 a.null_weight ? nullptr : a.weight,
                                 a.null_thresh ? nullptr : a.thresh, a.gain, a.n_iter, a.cpix,
                                 a.cscale, a.cflux, a.ncomp, m);
  std::printf("%s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  {
    Conv a;
    put("conv valid", a);
    a = Conv(); a.n_ker = 2; put("conv valid per-map kernels", a);
    a = Conv(); a.kx = a.kz = 255; put("conv valid 255", a);
    a = Conv(); a.nx = a.nz = a.kx = a.kz = a.n_maps = 1; put("conv valid 1x1", a);
    a = Conv(); a.in = nullptr; put("conv NULL d_in", a);
    a = Conv(); a.ker = nullptr; put("conv NULL d_ker", a);
    a = Conv(); a.out = nullptr; put("conv NULL d_out", a);
    a = Conv(); a.n_maps = 0; put("conv n_maps 0", a);
    a = Conv(); a.nx = 0; put("conv nx 0", a);
    a = Conv(); a.nz = -1; put("conv nz -1", a);
    a = Conv(); a.kx = 0; put("conv kx 0", a);
    a = Conv(); a.kz = -3; put("conv kz -3", a);
    a = Conv(); a.kx = 4; put("conv kx even", a);
    a = Conv(); a.kz = 2; put("conv kz even", a);
    a = Conv(); a.kx = 257; put("conv kx 257", a);
    a = Conv(); a.kz = 257; put("conv kz 257", a);
    a = Conv(); a.n_ker = 0; put("conv n_ker 0", a);
    a = Conv(); a.n_ker = 3; put("conv n_ker 3", a);
    a = Conv(); a.nx = 46341; a.nz = 46341; put("conv nx nz 2^31", a);
    a = Conv(); a.nx = 46340; a.nz = 46340; a.n_maps = a.n_ker = 2000; put("conv workgroups", a);
    a = Conv(); a.in = nullptr; a.nx = 0; put("conv NULL beats sizes", a);
    a = Conv(); a.nx = 0; a.kx = 4; put("conv sizes beat even", a);
    a = Conv(); a.kx = 256; put("conv even beats max", a);
    a = Conv(); a.kx = 257; a.n_ker = 3; put("conv max beats n_ker", a);
    a = Conv(); a.n_ker = 3; a.nx = a.nz = 46341; put("conv n_ker beats the image size", a);
  }
  Ms a;
  put("valid", a);
  a = Ms(); a.gain = 1.0; a.n_psf = 2; put("valid gain 1 per-map beams", a);
  a = Ms(); a.res = nullptr; put("NULL d_res", a);
  a = Ms(); a.xpsf = nullptr; put("NULL d_xpsf", a);
  a = Ms(); a.null_weight = true; put("NULL h_weight", a);
  a = Ms(); a.null_thresh = true; put("NULL h_thresh", a);
  a = Ms(); a.cpix = nullptr; put("NULL d_cpix", a);
  a = Ms(); a.cscale = nullptr; put("NULL d_cscale", a);
  a = Ms(); a.cflux = nullptr; put("NULL d_cflux", a);
  a = Ms(); a.ncomp = nullptr; put("NULL d_ncomp", a);
  a = Ms(); a.n_maps = 0; put("n_maps 0", a);
  a = Ms(); a.n_s = 0; put("n_s 0", a);
  a = Ms(); a.nx = 0; put("nx 0", a);
  a = Ms(); a.nz = -1; put("nz -1", a);
  a = Ms(); a.px = 0; put("px 0", a);
  a = Ms(); a.pz = 0; put("pz 0", a);
  a = Ms(); a.px = 8; put("px even", a);
  a = Ms(); a.pz = 4; put("pz even", a);
  a = Ms(); a.n_psf = 0; put("n_psf 0", a);
  a = Ms(); a.n_psf = 3; put("n_psf 3", a);
  a = Ms(); a.nx = 46341; a.nz = 46341; put("nx nz 2^31", a);
  a = Ms(); a.gain = 0.0; put("gain 0", a);
  a = Ms(); a.gain = 1.5; put("gain 1.5", a);
  a = Ms(); a.gain = nan; put("gain nan", a);
  a = Ms(); a.n_iter = 0; put("n_iter 0", a);
  a = Ms(); a.thresh[1] = -1.0; put("thresh negative", a);
  a = Ms(); a.thresh[0] = inf; put("thresh inf", a);
  a = Ms(); a.weight[4] = -0.5; put("weight negative", a);
  a = Ms(); a.weight[5] = inf; put("weight inf", a);
  a = Ms(); a.weight[0] = nan; put("weight nan", a);
  // which one wins
  a = Ms(); a.cscale = nullptr; a.n_s = 0; put("NULL beats sizes", a);
  a = Ms(); a.n_s = 0; a.px = 8; put("sizes beat even", a);
  a = Ms(); a.px = 8; a.n_psf = 3; put("even beats n_psf", a);
  a = Ms(); a.n_psf = 3; a.gain = 0.0; put("n_psf beats gain", a);
  a = Ms(); a.gain = 0.0; a.n_iter = 0; put("gain beats n_iter", a);
  a = Ms(); a.n_iter = 0; a.thresh[0] = nan; put("n_iter beats thresh", a);
  a = Ms(); a.thresh[0] = nan; a.weight[0] = nan; put("thresh beats weight", a);
  return 0;
}
