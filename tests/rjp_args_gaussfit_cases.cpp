// check_gaussfit of rajepy_amd/csrc/rjp_args.h -- the pure argument check of rjp_gaussfit -- driven
// from a plain C++ program (no HIP): one line "case<TAB>status<TAB>message" per case, in the order
// the check refuses; tests/test_gaussfit_reference_cpu.py holds the lines to the messages that
// tests/test_gpu_gaussfit.py sees from the library.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "rjp_args.h"

namespace A = rjp_args;

static double* const kD = (double*)0x1000;      // stand for device pointers: never dereferenced
static int32_t* const kI = (int32_t*)0x2000;

struct Args {
  const double* img = kD;
  int n_maps = 2, nx = 5, nz = 3;
  int32_t box[4] = {0, 4, 0, 2};
  bool null_box = false;
  const double* theta = kD;
  double lambda0 = 1e-3, xtol = 1e-12;
  int n_iter = 4;
  const double *chi2 = kD, *cov = kD;
  const int32_t *npix = kI, *niter = kI, *status = kI;
};

static void put(const char* name, const Args& a) {
  std::string m;
  const int r = A::check_gaussfit(a.img, a.n_maps, a.nx, a.nz, a.null_box ? nullptr : a.box, a.theta,
                                  a.lambda0, a.xtol, a.n_iter, a.chi2, a.cov, a.npix, a.niter,
                                  a.status, m);
  std::printf("%s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  Args a;
  put("valid", a);
  a = Args(); a.box[0] = a.box[1] = 4; a.box[2] = a.box[3] = 2; put("valid one pixel", a);
  a = Args(); a.img = nullptr; put("NULL d_img", a);
  a = Args(); a.null_box = true; put("NULL h_box", a);
  a = Args(); a.theta = nullptr; put("NULL d_theta", a);
  a = Args(); a.chi2 = nullptr; put("NULL d_chi2", a);
  a = Args(); a.cov = nullptr; put("NULL d_cov", a);
  a = Args(); a.npix = nullptr; put("NULL d_npix", a);
  a = Args(); a.niter = nullptr; put("NULL d_niter", a);
  a = Args(); a.status = nullptr; put("NULL d_status", a);
  a = Args(); a.n_maps = 0; put("n_maps 0", a);
  a = Args(); a.nx = 0; put("nx 0", a);
  a = Args(); a.nz = -1; put("nz -1", a);
  a = Args(); a.nx = 1 << 16; a.nz = 1 << 15; put("nx nz 2^31", a);
  a = Args(); a.nx = 46341; a.nz = 46340; a.box[1] = 46340; a.box[3] = 46339; put("valid nx nz below 2^31", a);
  a = Args(); a.box[0] = -1; put("i0 < 0", a);
  a = Args(); a.box[1] = 5; put("i1 = nx", a);
  a = Args(); a.box[0] = 3; a.box[1] = 2; put("i1 < i0", a);
  a = Args(); a.box[2] = -1; put("j0 < 0", a);
  a = Args(); a.box[3] = 3; put("j1 = nz", a);
  a = Args(); a.box[2] = 2; a.box[3] = 1; put("j1 < j0", a);
  a = Args(); a.lambda0 = 0.0; put("lambda0 0", a);
  a = Args(); a.lambda0 = inf; put("lambda0 inf", a);
  a = Args(); a.lambda0 = nan; put("lambda0 nan", a);
  a = Args(); a.xtol = -1.0; put("xtol -1", a);
  a = Args(); a.xtol = inf; put("xtol inf", a);
  a = Args(); a.xtol = nan; put("xtol nan", a);
  a = Args(); a.n_iter = 0; put("n_iter 0", a);
  // which one wins
  a = Args(); a.img = nullptr; a.nx = 0; put("NULL beats sizes", a);
  a = Args(); a.nx = 0; a.box[0] = 3; a.box[1] = 2; put("sizes beat the box", a);
  a = Args(); a.nx = 1 << 16; a.nz = 1 << 15; a.box[0] = -1; put("npix beats the box", a);
  a = Args(); a.box[0] = 3; a.box[1] = 2; a.lambda0 = 0.0; put("box beats lambda0", a);
  a = Args(); a.lambda0 = 0.0; a.n_iter = 0; put("lambda0 beats n_iter", a);
  return 0;
}
