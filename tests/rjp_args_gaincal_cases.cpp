// check_gain_apply and check_gaincal of rajepy_amd/csrc/rjp_args.h -- the pure argument checks of
// rjp_gain_apply and rjp_gaincal -- driven from a plain C++ program (no HIP): one line
// "case<TAB>status<TAB>message" per case, in the order the checks refuse;
// tests/test_gaincal_reference_cpu.py holds the lines to the messages that
// tests/test_gpu_gaincal.py sees from the library.  Cases of the apply begin with "a ", those of
// the solve with "g ".
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "rjp_args.h"

namespace A = rjp_args;

static double* const kD = (double*)0x1000;      // stand for device pointers: never dereferenced
static int32_t* const kI = (int32_t*)0x2000;
static uint8_t* const kB = (uint8_t*)0x3000;

struct App {
  const double* vis = kD;
  int n_maps = 2, n_t = 4, n_ant = 5;
  const double* gains = kD;
  int g_maps = 1;
  std::vector<int32_t> sol = {0, 0, 1, 2};
  bool null_sol = false;
  int n_sol = 3, mode = 0;
  const double* out = kD;
};

static void put(const char* name, const App& a) {
  std::string m;
  const int r = A::check_gain_apply(a.vis, a.n_maps, a.n_t, a.n_ant, a.gains, a.g_maps,
                                    a.null_sol ? nullptr : a.sol.data(), a.n_sol, a.mode, a.out, m);
  std::printf("a %s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

struct Cal {
  const double* vis = kD;
  int n_maps = 2, n_t = 4, n_ant = 5;
  const double* model = kD;
  int model_maps = 1;
  const double* w = nullptr;
  int w_maps = 7;                                // (not looked at without weights)
  std::vector<int32_t> sol = {0, 0, 1, 2};
  bool null_sol = false;
  int n_sol = 3, mode = 1, refant = 4, min_bl = 1;
  double tol = 1e-10;
  int n_iter = 3;
  const double *gains = kD, *chi2 = kD;
  const int32_t *nvis = kI, *niter = kI, *status = kI;
  const uint8_t* live = kB;
};

static void put(const char* name, const Cal& a) {
  std::string m;
  const int r = A::check_gaincal(a.vis, a.n_maps, a.n_t, a.n_ant, a.model, a.model_maps, a.w, a.w_maps,
                                 a.null_sol ? nullptr : a.sol.data(), a.n_sol, a.mode, a.refant, a.min_bl,
                                 a.tol, a.n_iter, a.gains, a.chi2, a.nvis, a.niter, a.status, a.live, m);
  std::printf("g %s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  {
    App a;
    put("valid", a);
    { App b = a; b.g_maps = 2; b.mode = 1; put("valid per map", b); }
    { App b = a; b.n_ant = 64; b.sol = {0}; b.n_t = 1; b.n_sol = 1; put("valid at the cap", b); }
    { App b = a; b.vis = nullptr; put("NULL d_vis", b); }
    { App b = a; b.gains = nullptr; put("NULL d_gains", b); }
    { App b = a; b.null_sol = true; put("NULL h_sol", b); }
    { App b = a; b.out = nullptr; put("NULL d_out", b); }
    { App b = a; b.out = nullptr; b.n_t = 0; put("NULL beats sizes", b); }
    { App b = a; b.n_maps = 0; put("n_maps 0", b); }
    { App b = a; b.n_t = -1; put("n_t -1", b); }
    { App b = a; b.n_sol = 0; put("n_sol 0", b); }
    { App b = a; b.n_sol = 0; b.n_ant = 1; put("sizes beat n_ant", b); }
    { App b = a; b.n_ant = 1; put("n_ant 1", b); }
    { App b = a; b.n_ant = 65; put("n_ant 65", b); }
    { App b = a; b.n_ant = 65; b.sol[0] = 1; put("n_ant beats h_sol", b); }
    { App b = a; b.sol = {1, 1, 2, 3}; b.n_sol = 4; put("h_sol starts at 1", b); }
    { App b = a; b.sol = {0, 2, 2, 2}; put("h_sol skips", b); }
    { App b = a; b.sol = {0, 1, 0, 1}; b.n_sol = 2; put("h_sol falls", b); }
    { App b = a; b.n_sol = 4; put("n_sol too large", b); }
    { App b = a; b.n_sol = 2; put("n_sol too small", b); }
    { App b = a; b.n_sol = 2; b.g_maps = 3; put("h_sol beats g_maps", b); }
    { App b = a; b.g_maps = 0; put("g_maps 0", b); }
    { App b = a; b.g_maps = 3; put("g_maps 3", b); }
    { App b = a; b.g_maps = 3; b.mode = 2; put("g_maps beats mode", b); }
    { App b = a; b.mode = 2; put("mode 2", b); }
    { App b = a; b.mode = -1; put("mode -1", b); }
    { App b = a; b.mode = 2; b.n_maps = 1 << 28; b.n_ant = 64; put("mode beats the workgroups", b); }
    { App b = a; b.n_maps = 1 << 28; b.n_ant = 64; put("2^31 workgroups", b); }
  }
  {
    Cal a;
    put("valid", a);
    { Cal b = a; b.w = kD; b.w_maps = 2; b.model_maps = 2; b.mode = 0; put("valid with weights", b); }
    { Cal b = a; b.n_ant = 2; b.refant = 1; put("valid two antennas", b); }
    { Cal b = a; b.vis = nullptr; put("NULL d_vis", b); }
    { Cal b = a; b.model = nullptr; put("NULL d_model", b); }
    { Cal b = a; b.null_sol = true; put("NULL h_sol", b); }
    { Cal b = a; b.gains = nullptr; put("NULL d_gains", b); }
    { Cal b = a; b.chi2 = nullptr; put("NULL d_chi2", b); }
    { Cal b = a; b.nvis = nullptr; put("NULL d_nvis", b); }
    { Cal b = a; b.niter = nullptr; put("NULL d_niter", b); }
    { Cal b = a; b.status = nullptr; put("NULL d_status", b); }
    { Cal b = a; b.live = nullptr; put("NULL d_live", b); }
    { Cal b = a; b.live = nullptr; b.n_maps = 0; put("NULL beats sizes", b); }
    { Cal b = a; b.n_maps = 0; put("n_maps 0", b); }
    { Cal b = a; b.n_t = 0; put("n_t 0", b); }
    { Cal b = a; b.n_sol = -3; put("n_sol -3", b); }
    { Cal b = a; b.n_sol = 0; b.n_ant = 70; put("sizes beat n_ant", b); }
    { Cal b = a; b.n_ant = 1; put("n_ant 1", b); }
    { Cal b = a; b.n_ant = 65; put("n_ant 65", b); }
    { Cal b = a; b.n_ant = 0; b.n_sol = 2; put("n_ant beats h_sol", b); }
    { Cal b = a; b.sol = {0, 0, 2, 2}; put("h_sol skips", b); }
    { Cal b = a; b.n_sol = 2; put("n_sol too small", b); }
    { Cal b = a; b.n_sol = 2; b.model_maps = 0; put("h_sol beats model_maps", b); }
    { Cal b = a; b.model_maps = 0; put("model_maps 0", b); }
    { Cal b = a; b.model_maps = 3; put("model_maps 3", b); }
    { Cal b = a; b.model_maps = 3; b.w = kD; b.w_maps = 3; put("model_maps beats w_maps", b); }
    { Cal b = a; b.w = kD; b.w_maps = 0; put("w_maps 0", b); }
    { Cal b = a; b.w = kD; b.w_maps = 3; put("w_maps 3", b); }
    { Cal b = a; b.w = kD; b.w_maps = 3; b.mode = 2; put("w_maps beats mode", b); }
    { Cal b = a; b.mode = 2; put("mode 2", b); }
    { Cal b = a; b.mode = 2; b.refant = 5; put("mode beats refant", b); }
    { Cal b = a; b.refant = -1; put("refant -1", b); }
    { Cal b = a; b.refant = 5; put("refant 5", b); }
    { Cal b = a; b.refant = 5; b.min_bl = 0; put("refant beats min_bl", b); }
    { Cal b = a; b.min_bl = 0; put("min_bl 0", b); }
    { Cal b = a; b.min_bl = 0; b.tol = 0.0; put("min_bl beats tol", b); }
    { Cal b = a; b.tol = 0.0; put("tol 0", b); }
    { Cal b = a; b.tol = -1e-3; put("tol negative", b); }
    { Cal b = a; b.tol = inf; put("tol inf", b); }
    { Cal b = a; b.tol = nan; put("tol nan", b); }
    { Cal b = a; b.tol = nan; b.n_iter = 0; put("tol beats n_iter", b); }
    { Cal b = a; b.n_iter = 0; put("n_iter 0", b); }
    { Cal b = a; b.n_iter = 0; b.n_maps = 1 << 29; put("n_iter beats the workgroups", b); }
    { Cal b = a; b.n_maps = 1 << 29; put("2^31 workgroups", b); }
  }
  return 0;
}
