// check_uvfit of rajepy_amd/csrc/rjp_args.h -- the pure argument check of rjp_uvfit -- driven from a
// plain C++ program (no HIP): one line "case<TAB>status<TAB>message" per case, in the order the
// check refuses; tests/test_uvfit_reference_cpu.py holds the lines to the messages that
// tests/test_gpu_uvfit.py sees from the library.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "rjp_args.h"

namespace A = rjp_args;

static double* const kD = (double*)0x1000;      // stand for device pointers: never dereferenced
static int32_t* const kI = (int32_t*)0x2000;

struct Args {
  const double* vis = kD;
  int n_maps = 2, n_vis = 7;
  std::vector<double> su = {1.0, -1.0}, sv = {1.0, 1.0};
  bool null_su = false, null_sv = false;
  const double *u = kD, *v = kD, *w = kD;
  int w_maps = 2, n_comp = 2;
  std::vector<uint8_t> free_ = {1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 1, 1};
  bool null_free = false;
  const double* theta = kD;
  double lambda0 = 1e-3, xtol = 1e-10;
  int n_iter = 4;
  const double *chi2 = kD, *cov = kD;
  const int32_t *nvis = kI, *niter = kI, *status = kI;
};

static void put(const char* name, const Args& a) {
  std::string m;
  const int r = A::check_uvfit(a.vis, a.n_maps, a.n_vis, a.null_su ? nullptr : a.su.data(),
                               a.null_sv ? nullptr : a.sv.data(), a.u, a.v, a.w, a.w_maps, a.n_comp,
                               a.null_free ? nullptr : a.free_.data(), a.theta, a.lambda0, a.xtol,
                               a.n_iter, a.chi2, a.cov, a.nvis, a.niter, a.status, m);
  std::printf("%s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  Args a;
  put("valid", a);
  a = Args(); a.null_free = true; a.w = nullptr; a.w_maps = 9; put("valid without weights and flags", a);
  a = Args(); a.n_comp = 1; a.w_maps = 1; put("valid one component, shared weights", a);
  a = Args(); a.n_maps = 1023; a.n_vis = 2147483647; a.su.assign(1023, 1.0); a.sv.assign(1023, 1.0);
  a.w_maps = 1; put("valid 1023 x 2^21 workgroups", a);
  a = Args(); a.vis = nullptr; put("NULL d_vis", a);
  a = Args(); a.null_su = true; put("NULL h_su", a);
  a = Args(); a.null_sv = true; put("NULL h_sv", a);
  a = Args(); a.u = nullptr; put("NULL d_u", a);
  a = Args(); a.v = nullptr; put("NULL d_v", a);
  a = Args(); a.theta = nullptr; put("NULL d_theta", a);
  a = Args(); a.chi2 = nullptr; put("NULL d_chi2", a);
  a = Args(); a.cov = nullptr; put("NULL d_cov", a);
  a = Args(); a.nvis = nullptr; put("NULL d_nvis", a);
  a = Args(); a.niter = nullptr; put("NULL d_niter", a);
  a = Args(); a.status = nullptr; put("NULL d_status", a);
  a = Args(); a.n_maps = 0; put("n_maps 0", a);
  a = Args(); a.n_vis = 0; put("n_vis 0", a);
  a = Args(); a.n_vis = -1; put("n_vis -1", a);
  a = Args(); a.n_comp = 0; put("n_comp 0", a);
  a = Args(); a.n_comp = 3; put("n_comp 3", a);
  a = Args(); a.w_maps = 0; put("w_maps 0", a);
  a = Args(); a.w_maps = 3; put("w_maps 3", a);
  a = Args(); a.su[1] = nan; put("su nan", a);
  a = Args(); a.sv[0] = inf; put("sv inf", a);
  a = Args(); a.free_.assign(12, 0); put("no free parameter", a);
  a = Args(); a.n_comp = 1; a.free_ = {0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1};
  put("no free parameter among the first six", a);
  a = Args(); a.lambda0 = 0.0; put("lambda0 0", a);
  a = Args(); a.lambda0 = inf; put("lambda0 inf", a);
  a = Args(); a.lambda0 = nan; put("lambda0 nan", a);
  a = Args(); a.xtol = -1.0; put("xtol -1", a);
  a = Args(); a.xtol = inf; put("xtol inf", a);
  a = Args(); a.xtol = nan; put("xtol nan", a);
  a = Args(); a.n_iter = 0; put("n_iter 0", a);
  a = Args(); a.n_maps = 1025; a.n_vis = 2147483647; a.su.assign(1025, 1.0); a.sv.assign(1025, 1.0);
  a.w_maps = 1; put("1025 x 2^21 workgroups", a);
  // which one wins
  a = Args(); a.vis = nullptr; a.n_vis = 0; put("NULL beats sizes", a);
  a = Args(); a.n_maps = 0; a.n_comp = 3; put("sizes beat n_comp", a);
  a = Args(); a.n_comp = 3; a.w_maps = 5; put("n_comp beats w_maps", a);
  a = Args(); a.w_maps = 5; a.su[0] = nan; put("w_maps beats the scales", a);
  a = Args(); a.su[0] = nan; a.free_.assign(12, 0); put("scales beat free", a);
  a = Args(); a.free_.assign(12, 0); a.lambda0 = 0.0; put("free beats lambda0", a);
  a = Args(); a.lambda0 = 0.0; a.n_iter = 0; put("lambda0 beats n_iter", a);
  a = Args(); a.n_maps = 1025; a.n_vis = 2147483647; a.su.assign(1025, 1.0); a.sv.assign(1025, 1.0);
  a.w_maps = 1; a.n_iter = 0; put("n_iter beats the workgroups", a);
  return 0;
}
