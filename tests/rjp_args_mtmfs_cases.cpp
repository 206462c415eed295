// check_mtmfs of rajepy_amd/csrc/rjp_args.h -- the pure argument checks of rjp_mtmfs -- driven from a
// plain C++ program (no HIP): one line "case<TAB>status<TAB>message" per case, in the order the checks
// refuse; tests/test_mtmfs_reference_cpu.py holds the lines to the messages that
// tests/test_gpu_mtmfs.py sees from the library.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>

#include "rjp_args.h"

namespace A = rjp_args;

static double* const kD = (double*)0x1000;      // stand for device pointers: never dereferenced
static int32_t* const kI = (int32_t*)0x2000;

struct Mt {
  const double *res = kD, *spsf = kD, *ccoef = kD;
  const int32_t *cpix = kI, *ncomp = kI;
  int n_maps = 2, n_t = 2, nx = 5, nz = 3, n_psf = 1, px = 9, pz = 5, n_iter = 4;
  double hinv[32] = {1.0, -0.5, -0.5, 80.0, 1.0, 0.25, 0.25, 75.0}, thresh[2] = {0.0, 1e-3}, gain = 0.1;
  bool null_hinv = false, null_thresh = false;
};

static void put(const char* name, const Mt& a) {
  std::string m;
  const int r = A::check_mtmfs(a.res, a.n_maps, a.n_t, a.nx, a.nz, a.spsf, a.n_psf, a.px, a.pz,
                               a.null_hinv ? nullptr : a.hinv, a.null_thresh ? nullptr : a.thresh,
                               a.gain, a.n_iter, a.cpix, a.ccoef, a.ncomp, m);
  std::printf("%s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  Mt a;
  put("valid", a);
  a = Mt(); a.gain = 1.0; a.n_psf = 2; put("valid gain 1 per-map beams", a);
  a = Mt(); a.n_t = 4; put("valid four terms", a);
  a = Mt(); a.n_t = 1; a.n_maps = 1; put("valid one term", a);
  a = Mt(); a.res = nullptr; put("NULL d_res", a);
  a = Mt(); a.spsf = nullptr; put("NULL d_spsf", a);
  a = Mt(); a.null_hinv = true; put("NULL h_hinv", a);
  a = Mt(); a.null_thresh = true; put("NULL h_thresh", a);
  a = Mt(); a.cpix = nullptr; put("NULL d_cpix", a);
  a = Mt(); a.ccoef = nullptr; put("NULL d_ccoef", a);
  a = Mt(); a.ncomp = nullptr; put("NULL d_ncomp", a);
  a = Mt(); a.n_maps = 0; put("n_maps 0", a);
  a = Mt(); a.n_t = 0; put("n_t 0", a);
  a = Mt(); a.n_t = -1; put("n_t -1", a);
  a = Mt(); a.nx = 0; put("nx 0", a);
  a = Mt(); a.nz = -1; put("nz -1", a);
  a = Mt(); a.px = 0; put("px 0", a);
  a = Mt(); a.pz = 0; put("pz 0", a);
  a = Mt(); a.n_t = 5; put("n_t 5", a);
  a = Mt(); a.n_t = 2147483647; put("n_t 2^31 - 1", a);
  a = Mt(); a.px = 8; put("px even", a);
  a = Mt(); a.pz = 4; put("pz even", a);
  a = Mt(); a.n_psf = 0; put("n_psf 0", a);
  a = Mt(); a.n_psf = 3; put("n_psf 3", a);
  a = Mt(); a.nx = 46341; a.nz = 46341; put("nx nz 2^31", a);
  a = Mt(); a.gain = 0.0; put("gain 0", a);
  a = Mt(); a.gain = 1.5; put("gain 1.5", a);
  a = Mt(); a.gain = nan; put("gain nan", a);
  a = Mt(); a.n_iter = 0; put("n_iter 0", a);
  a = Mt(); a.thresh[1] = -1.0; put("thresh negative", a);
  a = Mt(); a.thresh[0] = inf; put("thresh inf", a);
  a = Mt(); a.hinv[0] = nan; put("hinv nan", a);
  a = Mt(); a.hinv[7] = inf; put("hinv inf in the last map", a);
  a = Mt(); a.hinv[2] = -inf; put("hinv -inf off the diagonal", a);
  // which one wins
  a = Mt(); a.ccoef = nullptr; a.n_t = 0; put("NULL beats sizes", a);
  a = Mt(); a.nx = 0; a.n_t = 5; put("sizes beat n_t", a);
  a = Mt(); a.n_t = 5; a.px = 8; put("n_t beats even", a);
  a = Mt(); a.px = 8; a.n_psf = 3; put("even beats n_psf", a);
  a = Mt(); a.n_psf = 3; a.gain = 0.0; put("n_psf beats gain", a);
  a = Mt(); a.gain = 0.0; a.n_iter = 0; put("gain beats n_iter", a);
  a = Mt(); a.n_iter = 0; a.thresh[0] = nan; put("n_iter beats thresh", a);
  a = Mt(); a.thresh[0] = nan; a.hinv[0] = nan; put("thresh beats hinv", a);
  return 0;
}
