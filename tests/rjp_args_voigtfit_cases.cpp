// check_voigtfit of rajepy_amd/csrc/rjp_args.h -- the pure argument check of rjp_voigtfit -- driven from
// a plain C++ program (no HIP): one line "case<TAB>status<TAB>message" per case, in the order the
// check refuses; tests/test_voigtfit_reference_cpu.py holds the lines to the messages that
// tests/test_gpu_voigtfit.py sees from the library.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "rjp_args.h"

namespace A = rjp_args;

static double* const kD = (double*)0x1000;      // stand for device pointers: never dereferenced
static int32_t* const kI = (int32_t*)0x2000;

struct Fit {
  const double* cube = kD;
  int64_t n_pix = 70;
  int n_chan = 3;
  std::vector<double> x = {3.0, 1.0, 2.0}, w = {1.0, 0.0, 2.0};
  bool null_x = false, null_w = false;
  double x_ref = 1.0;
  int n_comp = 2;
  std::vector<uint8_t> free_ = {1, 1, 1, 0, 0, 0, 0, 1, 1, 1};
  bool null_free = false;
  const double* theta = kD;
  double lambda0 = 1e-3, xtol = 1e-10;
  int n_iter = 4;
  const double *chi2 = kD, *cov = kD;
  const int32_t *nchan = kI, *niter = kI, *status = kI;
};

static void put(const char* name, const Fit& a) {
  std::string m;
  const int r = A::check_voigtfit(a.cube, a.n_pix, a.n_chan, a.null_x ? nullptr : a.x.data(), a.x_ref,
                                  a.null_w ? nullptr : a.w.data(), a.n_comp,
                                  a.null_free ? nullptr : a.free_.data(), a.theta, a.lambda0, a.xtol,
                                  a.n_iter, a.chi2, a.cov, a.nchan, a.niter, a.status, m);
  std::printf("%s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  const int64_t many = (int64_t)64 * 2147483647;          // 2^31 - 1 workgroups: the most
  Fit a;
  put("valid", a);
  a = Fit(); a.null_w = true; a.null_free = true; put("valid without weights and flags", a);
  a = Fit(); a.n_comp = 1; a.free_ = {0, 0, 0, 0, 0, 1}; put("valid one component, b1 alone", a);
  a = Fit(); a.n_comp = 1; a.free_ = {1, 1, 1, 0, 0, 0}; put("valid g held", a);
  a = Fit(); a.n_pix = many; put("valid 2^31 - 1 workgroups", a);
  a = Fit(); a.n_chan = 4096; a.x.assign(4096, 1.0); a.w.assign(4096, 1.0); put("valid 4096 channels", a);
  a = Fit(); a.cube = nullptr; put("NULL d_cube", a);
  a = Fit(); a.null_x = true; put("NULL h_x", a);
  a = Fit(); a.theta = nullptr; put("NULL d_theta", a);
  a = Fit(); a.chi2 = nullptr; put("NULL d_chi2", a);
  a = Fit(); a.cov = nullptr; put("NULL d_cov", a);
  a = Fit(); a.nchan = nullptr; put("NULL d_nchan", a);
  a = Fit(); a.niter = nullptr; put("NULL d_niter", a);
  a = Fit(); a.status = nullptr; put("NULL d_status", a);
  a = Fit(); a.n_pix = 0; put("n_pix 0", a);
  a = Fit(); a.n_pix = -3; put("n_pix -3", a);
  a = Fit(); a.n_chan = 0; put("n_chan 0", a);
  a = Fit(); a.n_chan = 4097; a.x.assign(4097, 1.0); a.w.assign(4097, 1.0); put("n_chan 4097", a);
  a = Fit(); a.n_comp = 0; put("n_comp 0", a);
  a = Fit(); a.n_comp = 3; put("n_comp 3", a);
  a = Fit(); a.x[1] = nan; put("x nan", a);
  a = Fit(); a.x[2] = inf; put("x inf", a);
  a = Fit(); a.x_ref = nan; put("x_ref nan", a);
  a = Fit(); a.x_ref = -inf; put("x_ref -inf", a);
  a = Fit(); a.w[0] = -1.0; put("w negative", a);
  a = Fit(); a.w[1] = inf; put("w inf", a);
  a = Fit(); a.w[2] = nan; put("w nan", a);
  a = Fit(); a.free_.assign(10, 0); put("no free parameter", a);
  a = Fit(); a.n_comp = 1; a.free_ = {0, 0, 0, 0, 0, 0, 1, 1, 1, 1}; put("no free parameter among the first six", a);
  a = Fit(); a.lambda0 = 0.0; put("lambda0 0", a);
  a = Fit(); a.lambda0 = inf; put("lambda0 inf", a);
  a = Fit(); a.lambda0 = nan; put("lambda0 nan", a);
  a = Fit(); a.xtol = -1.0; put("xtol -1", a);
  a = Fit(); a.xtol = inf; put("xtol inf", a);
  a = Fit(); a.xtol = nan; put("xtol nan", a);
  a = Fit(); a.n_iter = 0; put("n_iter 0", a);
  a = Fit(); a.n_pix = many + 1; put("2^31 workgroups", a);
  // which one wins
  a = Fit(); a.cube = nullptr; a.n_pix = 0; put("NULL beats sizes", a);
  a = Fit(); a.n_chan = 0; a.n_comp = 3; put("sizes beat the limit and n_comp", a);
  a = Fit(); a.n_chan = 4097; a.x.assign(4097, 1.0); a.w.assign(4097, 1.0); a.n_comp = 3;
  put("the limit beats n_comp", a);
  a = Fit(); a.n_comp = 3; a.x[0] = nan; put("n_comp beats x", a);
  a = Fit(); a.x[0] = nan; a.x_ref = nan; put("x beats x_ref", a);
  a = Fit(); a.x_ref = nan; a.w[0] = -1.0; put("x_ref beats w", a);
  a = Fit(); a.w[0] = -1.0; a.free_.assign(10, 0); put("w beats free", a);
  a = Fit(); a.free_.assign(10, 0); a.lambda0 = 0.0; put("free beats lambda0", a);
  a = Fit(); a.lambda0 = 0.0; a.n_iter = 0; put("lambda0 beats n_iter", a);
  a = Fit(); a.n_iter = 0; a.n_pix = many + 1; put("n_iter beats the workgroups", a);
  return 0;
}
