// check_srt_codes of rajepy_amd/csrc/rjp_args.h -- the pure argument check of rjp_srt_codes -- driven
// from a plain C++ program (no HIP): one line "case<TAB>status<TAB>message" per case, in the order the
// check refuses; tests/test_srt_codes_cpu.py holds the lines to the messages that
// tests/test_gpu_srt_codes.py sees from the library.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>

#include "rjp_args.h"

namespace A = rjp_args;

static void* const kD = (void*)0x1000;          // stand for device pointers: never dereferenced

struct Codes {
  rjp_fields f{};
  bool null_fields = false;
  int K = 32;
  const void *start = kD, *rowbase = kD, *cells = kD, *pc = kD;
  Codes() {
    f.dtype = RJP_F64;
    f.d_a0 = kD;
    f.d_ts = kD;
    f.nx = 128; f.ny = 320; f.nz = 256;
    f.ts_lo = 0.0;
    f.ts_hi = 1.5e8;
  }
};

static void put(const char* name, const Codes& a) {
  std::string m;
  const int r = A::check_srt_codes(a.null_fields ? nullptr : &a.f, a.K, 32, a.start, a.rowbase,
                                   a.cells, a.pc, m);
  std::printf("%s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  Codes a;
  put("valid", a);
  a = Codes(); a.K = 1; put("valid K 1", a);
  a = Codes(); a.f.ts_lo = a.f.ts_hi = 7.0; put("valid empty range", a);
  a = Codes(); a.f.ts_lo = -3e7; a.f.ts_hi = 0.0; put("valid range ending at 0", a);
  a = Codes(); a.pc = (void*)0x1010; a.cells = (void*)0x2020; put("valid 16-byte aligned", a);
  a = Codes(); a.null_fields = true; put("NULL fields", a);
  a = Codes(); a.f.dtype = RJP_F32; put("f32", a);
  a = Codes(); a.f.d_a0 = nullptr; put("no a0", a);
  a = Codes(); a.f.d_ts = nullptr; put("no ts", a);
  a = Codes(); a.f.ny = 0; put("n_y 0", a);
  a = Codes(); a.K = 0; put("K 0", a);
  a = Codes(); a.K = 33; put("K 33", a);
  a = Codes(); a.f.ts_lo = a.f.ts_hi = 0.0; put("no range", a);
  a = Codes(); a.f.ts_hi = nan; put("range nan", a);
  a = Codes(); a.f.ts_hi = inf; put("range inf", a);
  a = Codes(); a.f.ts_lo = 2.0; a.f.ts_hi = 1.0; put("range reversed", a);
  a = Codes(); a.start = nullptr; put("NULL d_start", a);
  a = Codes(); a.rowbase = nullptr; put("NULL d_rowbase", a);
  a = Codes(); a.cells = nullptr; put("NULL d_cells", a);
  a = Codes(); a.pc = nullptr; put("NULL d_pc", a);
  a = Codes(); a.pc = (void*)0x1004; put("d_pc + 4", a);
  a = Codes(); a.pc = (void*)0x1008; put("d_pc + 8", a);
  a = Codes(); a.cells = (void*)0x1008; put("d_cells + 8", a);
  // which one wins
  a = Codes(); a.null_fields = true; a.K = 0; put("fields beat K", a);
  a = Codes(); a.f.dtype = RJP_F32; a.f.nx = 0; put("storage beats dimensions", a);
  a = Codes(); a.f.nz = -1; a.K = 0; put("dimensions beat K", a);
  a = Codes(); a.K = 0; a.f.ts_lo = a.f.ts_hi = 0.0; put("K beats the range", a);
  a = Codes(); a.f.ts_lo = a.f.ts_hi = 0.0; a.pc = nullptr; put("the range beats NULL", a);
  a = Codes(); a.start = nullptr; a.pc = (void*)0x1004; put("NULL beats alignment", a);
  return 0;
}
