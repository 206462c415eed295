// check_normal_eq of rajepy_amd/csrc/rjp_args.h -- the pure argument check of rjp_normal_eq --
// driven from a plain C++ program (no HIP): one line "case<TAB>status<TAB>message" per case, in the
// order the check refuses; tests/test_normal_eq_reference_cpu.py holds the lines to the messages
// that tests/test_gpu_normal_eq.py sees from the library.
#include <cstdio>
#include <string>
#include <vector>

#include "rjp_args.h"

namespace A = rjp_args;

static double* const kD = (double*)0x1000;      // stand for device pointers: never dereferenced
static int64_t* const kL = (int64_t*)0x2000;

struct Ne {
  const double *data = kD, *model = kD, *dmodel = kD;
  int64_t n_rows = 3;
  int n_vis = 5, n_part = 2, n_par = 6;
  std::vector<int32_t> sel = {4, 0, 5};
  bool null_sel = false;
  int n_sel = 3;
  const double* w = nullptr;
  int64_t w_rows = 7;                            // (not looked at without weights)
  const double* out = kD;
  const int64_t* count = kL;
};

static void put(const char* name, const Ne& a) {
  std::string m;
  const int r = A::check_normal_eq(a.data, a.model, a.dmodel, a.n_rows, a.n_vis, a.n_part, a.n_par,
                                   a.null_sel ? nullptr : a.sel.data(), a.n_sel, a.w, a.w_rows, a.out,
                                   a.count, m);
  std::printf("%s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

int main() {
  Ne a;
  put("valid", a);
  a = Ne(); a.n_sel = 0; a.dmodel = nullptr; a.null_sel = true; a.n_par = 0; put("valid n_sel 0", a);
  a = Ne(); a.w = kD; a.w_rows = 1; put("valid shared weights", a);
  a = Ne(); a.w = kD; a.w_rows = 3; a.n_part = 1; put("valid weights per row", a);
  a = Ne(); a.n_rows = (int64_t)INT32_MAX * 512; a.n_vis = 1; put("valid 2^31 - 1 workgroups", a);
  a = Ne(); a.sel.resize(48); for (int i = 0; i < 48; ++i) a.sel[i] = 47 - i;
  a.n_sel = 48; a.n_par = 48; put("valid n_sel 48", a);

  a = Ne(); a.data = nullptr; put("NULL d_data", a);
  a = Ne(); a.model = nullptr; put("NULL d_model", a);
  a = Ne(); a.out = nullptr; put("NULL d_out", a);
  a = Ne(); a.count = nullptr; put("NULL d_count", a);
  a = Ne(); a.out = nullptr; a.n_rows = 0; put("NULL beats sizes", a);

  a = Ne(); a.n_rows = 0; put("n_rows 0", a);
  a = Ne(); a.n_vis = -1; put("n_vis -1", a);
  a = Ne(); a.n_vis = 0; a.n_part = 3; put("sizes beat n_part", a);

  a = Ne(); a.n_part = 0; put("n_part 0", a);
  a = Ne(); a.n_part = 3; put("n_part 3", a);
  a = Ne(); a.n_part = 3; a.n_sel = 49; put("n_part beats n_sel", a);

  a = Ne(); a.n_sel = -1; put("n_sel -1", a);
  a = Ne(); a.n_sel = 49; a.n_par = 60; put("n_sel 49", a);
  a = Ne(); a.n_sel = 49; a.dmodel = nullptr; put("n_sel beats the NULLs", a);

  a = Ne(); a.dmodel = nullptr; put("NULL d_dmodel", a);
  a = Ne(); a.null_sel = true; put("NULL h_sel", a);
  a = Ne(); a.null_sel = true; a.n_par = 2; put("the NULLs beat n_par", a);

  a = Ne(); a.n_par = 2; put("n_par 2", a);
  a = Ne(); a.n_par = 2; a.sel = {0, 0, 9}; put("n_par beats the indices", a);

  a = Ne(); a.sel = {4, -1, 5}; put("index -1", a);
  a = Ne(); a.sel = {4, 6, 5}; put("index n_par", a);
  a = Ne(); a.sel = {4, 6, 4}; put("range beats repeat", a);

  a = Ne(); a.sel = {4, 0, 4}; put("repeat", a);
  a = Ne(); a.sel = {4, 4, 5}; a.w = kD; a.w_rows = 2; put("repeat beats w_rows", a);

  a = Ne(); a.w = kD; a.w_rows = 0; put("w_rows 0", a);
  a = Ne(); a.w = kD; a.w_rows = 2; put("w_rows 2", a);
  a = Ne(); a.w = kD; a.w_rows = 2; a.n_rows = (int64_t)1 << 40; a.n_vis = 1 << 20;
  put("w_rows beats the workgroups", a);

  a = Ne(); a.n_rows = (int64_t)INT32_MAX * 512 + 1; a.n_vis = 1; put("2^31 workgroups", a);
  a = Ne(); a.n_rows = (int64_t)1 << 40; a.n_vis = 1 << 20; put("2^60 samples", a);
  return 0;
}
