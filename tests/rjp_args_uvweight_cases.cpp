// check_uv_weights of rajepy_amd/csrc/rjp_args.h -- the pure argument check of rjp_uv_weights --
// driven from a plain C++ program (no HIP): one line "case<TAB>status<TAB>message" per case, in the
// order the check refuses; tests/test_uvweight_reference_cpu.py holds the lines to the messages
// that tests/test_gpu_uvweight.py sees from the library.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>

#include "rjp_args.h"

namespace A = rjp_args;

static double* const kD = (double*)0x1000;      // stand for device pointers: never dereferenced

struct Args {
  int n_maps = 2, n_vis = 7;
  double su[2] = {1.0, -0.5}, sv[2] = {-1.0, 0.25};
  bool null_su = false, null_sv = false;
  const double *u = kD, *v = kD;
  int nx = 5, nz = 3, mode = 2;
  double robust = 0.5;
  const double* wout = kD;
};

static void put(const char* name, const Args& a) {
  std::string m;
  const int r = A::check_uv_weights(a.n_maps, a.n_vis, a.null_su ? nullptr : a.su,
                                    a.null_sv ? nullptr : a.sv, a.u, a.v, a.nx, a.nz, a.mode,
                                    a.robust, a.wout, m);
  std::printf("%s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  Args a;
  put("valid", a);
  a = Args(); a.mode = 1; a.robust = nan; put("valid uniform ignores robust", a);
  a = Args(); a.robust = -2.0; put("valid robust -2", a);
  a = Args(); a.robust = 2.0; put("valid robust 2", a);
  a = Args(); a.null_su = true; put("NULL h_su", a);
  a = Args(); a.null_sv = true; put("NULL h_sv", a);
  a = Args(); a.u = nullptr; put("NULL d_u", a);
  a = Args(); a.v = nullptr; put("NULL d_v", a);
  a = Args(); a.wout = nullptr; put("NULL d_wout", a);
  a = Args(); a.n_maps = 0; put("n_maps 0", a);
  a = Args(); a.n_vis = 0; put("n_vis 0", a);
  a = Args(); a.nx = 0; put("nx 0", a);
  a = Args(); a.nz = -1; put("nz -1", a);
  a = Args(); a.su[1] = inf; put("su inf", a);
  a = Args(); a.sv[0] = nan; put("sv nan", a);
  a = Args(); a.mode = 0; put("mode 0", a);
  a = Args(); a.mode = 3; put("mode 3", a);
  a = Args(); a.robust = 2.5; put("robust 2.5", a);
  a = Args(); a.robust = -2.0000001; put("robust below -2", a);
  a = Args(); a.robust = nan; put("robust nan", a);
  a = Args(); a.robust = inf; put("robust inf", a);
  // which one wins
  a = Args(); a.u = nullptr; a.nx = 0; put("NULL beats sizes", a);
  a = Args(); a.nx = 0; a.su[0] = nan; put("sizes beat the scale", a);
  a = Args(); a.su[0] = nan; a.mode = 7; put("scale beats the mode", a);
  a = Args(); a.mode = 7; a.robust = nan; put("mode beats robust", a);
  return 0;
}
