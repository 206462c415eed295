// The pure argument checks of rajepy_amd/csrc/rjp_args.h on hand-built structs, from a plain C++
// program (tests/test_host_logic.py builds it with g++: no HIP, no GPU).  Every line it prints,
//   <entry point> TAB <case> TAB <status> TAB <message>
// names a case of tests/abi_refusal_cases.py that the check alone decides; the test compares it
// with that case's entry of tests/golden/abi_refusals.json.  "scale" lines: the chain-rule table.
#include <cmath>
#include <cstdio>
#include <string>

#include "rjp_args.h"

namespace A = rjp_args;

static void* const kDev = (void*)0x1000;     // stands for a device pointer: never dereferenced
static double g_t0[2][9], g_amp[2][9], g_inv[2][9];

static rjp_fields fields() {
  rjp_fields f = {};
  f.d_nd = f.d_xi = f.d_temp = f.d_pf = f.d_ts = f.d_vy = f.d_em0 = f.d_a0 = kDev;
  f.nx = 8; f.ny = 16; f.nz = 16;
  f.dtype = RJP_F64;
  f.csize_au = 0.5;
  f.a0_mode = RJP_GFF_SCALAR;
  f.ts_lo = 1.0; f.ts_hi = 2.0;
  return f;
}

static rjp_bursts bursts(int red = 1, int blue = 1) {
  rjp_bursts b = {};
  b.n[0] = red; b.n[1] = blue;
  for (int j = 0; j < 2; ++j) {
    for (int i = 0; i < 9; ++i) { g_t0[j][i] = 3e7 * (1 + j); g_amp[j][i] = 2.0 - j; g_inv[j][i] = 1e-14; }
    b.t0[j] = g_t0[j]; b.amp_rel[j] = g_amp[j]; b.inv2s2[j] = g_inv[j];
  }
  return b;
}

static void put(const char* entry, const char* name, int status, const std::string& msg) {
  std::printf("%s\t%s\t%d\t%s\n", entry, name, status, status ? msg.c_str() : "");
}

// check_fields as rjp_compact_fields (wide fields only), rjp_y_bounds (compact layout accepted) and
// rjp_rrl_scan (d_vy needed) call it
static void fields_case(const char* entry, const char* name, const rjp_fields* f) {
  const std::string e(entry);
  std::string m;
  put(entry, name, A::check_fields(f, e == "rjp_rrl_scan", e == "rjp_y_bounds", -1, m), m);
}

static void layout_case(const char* name, const rjp_fields* f, int K_lt = 4, int K_srt = 4) {
  std::string m;
  put("rjp_lt_count", name, A::check_layout(f, K_lt, "launch-time-ordered layout", 80, 65536, m), m);
  put("rjp_srt_count", name, A::check_layout(f, K_srt, "launch-time-bucketed layout", 32, 0, m), m);
}

static void grad_case(const char* name, const rjp_bursts* b, const double* ep, int n_ep,
                      bool show = false) {
  const rjp_fields f = fields();
  for (int lead = 1; lead >= 0; --lead) {
    const char* who = lead ? "rjp_ff_grad" : "rjp_ff_formal_grad";
    double scale[1 + 6 * 8];
    int n = 0;
    std::string m;
    const int r = A::check_grad_bursts(b, &f, ep, n_ep, 8, lead, who, scale, &n, m);
    put(who, name, r, m);
    if (show && r == RJP_OK) {
      std::printf("scale\t%s", who);
      for (int k = 0; k < n; ++k) std::printf("\t%.17g", scale[k]);
      std::printf("\n");
    }
  }
}

int main() {
  rjp_fields f;
  const char* three[] = {"rjp_compact_fields", "rjp_y_bounds", "rjp_rrl_scan"};
  for (const char* e : three) {
    f = fields(); fields_case(e, "valid", &f);
    fields_case(e, "fields NULL", nullptr);
    f = fields(); f.dtype = 3; fields_case(e, "fields.dtype", &f);
    f = fields(); f.nx = 0; fields_case(e, "fields.nx = 0", &f);
    f = fields(); f.nz = -4; fields_case(e, "fields.nz < 0", &f);
    f = fields(); f.a0_mode = 7; fields_case(e, "fields.a0_mode", &f);
    f = fields(); f.csize_au = 0.0; fields_case(e, "fields.csize_au = 0", &f);
    f = fields(); f.d_ylo = (const int32_t*)kDev; fields_case(e, "fields.d_ylo alone", &f);
  }
  f = fields(); f.d_xi = nullptr; fields_case("rjp_compact_fields", "fields.d_xi NULL", &f);
  f = fields(); f.d_xi = nullptr; fields_case("rjp_rrl_scan", "fields.d_xi NULL", &f);
  f = fields(); f.d_vy = nullptr; fields_case("rjp_rrl_scan", "fields.d_vy NULL", &f);
  f = fields(); f.d_a0 = f.d_temp = nullptr; fields_case("rjp_y_bounds", "compact without d_temp", &f);
  f = fields(); f.d_a0 = f.d_em0 = f.d_pf = nullptr; fields_case("rjp_y_bounds", "no complete layout", &f);

  {  // check_grid with the y-range pairing, as rjp_tavg calls it
    std::string m;
    f = fields(); f.dtype = 3; put("rjp_tavg", "fields.dtype", A::check_grid(&f, true, m), m);
    f = fields(); f.nx = 0; put("rjp_tavg", "fields.nx = 0", A::check_grid(&f, true, m), m);
    f = fields(); f.d_ylo = (const int32_t*)kDev;
    put("rjp_tavg", "fields.d_ylo alone", A::check_grid(&f, true, m), m);
  }

  {  // check_bursts, as every entry point with bursts calls it after check_fields
    std::string m;
    rjp_bursts b;
    f = fields();
    b = bursts(); put("rjp_rrl_scan", "valid", A::check_bursts(&b, &f, m), m);
    put("rjp_rrl_scan", "valid", A::check_bursts(nullptr, &f, m), m);
    b = bursts(); b.n[1] = -1; put("rjp_rrl_scan", "bursts.n < 0", A::check_bursts(&b, &f, m), m);
    b = bursts(); b.n[0] = (1 << 20) + 1;
    put("rjp_rrl_scan", "bursts.n too large", A::check_bursts(&b, &f, m), m);
    b = bursts(); b.amp_rel[0] = nullptr;
    put("rjp_rrl_scan", "bursts.amp_rel NULL", A::check_bursts(&b, &f, m), m);
    b = bursts(); f.d_ts = nullptr;
    put("rjp_rrl_scan", "bursts without fields.d_ts", A::check_bursts(&b, &f, m), m);
  }

  const double ep[2] = {3.1e7, 3.9e7}, ep_nan[2] = {3.1e7, NAN};
  {  // check_epochs
    std::string m;
    const char* w = "rjp_ff_formal_sweep";
    put(w, "valid", A::check_epochs(ep, 2, true, w, m), m);
    put(w, "valid", A::check_epochs(ep_nan, 2, false, w, m), m);     // (not asked to be finite)
    put(w, "h_epochs_s NULL", A::check_epochs(nullptr, 2, true, w, m), m);
    put(w, "n_epochs = 0", A::check_epochs(ep, 0, true, w, m), m);
    put(w, "non-finite epoch", A::check_epochs(ep_nan, 2, true, w, m), m);
  }

  {  // check_grad_bursts, with and without the leading entry of the chain-rule table
    rjp_bursts b = bursts();
    grad_case("valid", &b, ep, 2, true);
    b = bursts(8, 8); grad_case("valid", &b, ep, 2, true);           // the table at its fullest
    grad_case("bursts NULL", nullptr, ep, 2);
    b = bursts(0, 0); grad_case("no burst", &b, ep, 2);
    b = bursts(); b.n[1] = -1; grad_case("bursts.n < 0", &b, ep, 2);
    b = bursts(); b.amp_rel[0] = nullptr; grad_case("bursts.amp_rel NULL", &b, ep, 2);
    b = bursts(9, 1); grad_case("nine bursts in a jet", &b, ep, 2);
    b = bursts(); g_inv[1][0] = NAN; grad_case("non-finite burst parameter", &b, ep, 2);
    grad_case("2: non-finite epoch and burst parameter", &b, ep_nan, 2);
    b = bursts(); grad_case("h_epochs_s NULL", &b, nullptr, 2);
    grad_case("n_epochs = 0", &b, ep, 0);
    grad_case("non-finite epoch", &b, ep_nan, 2);
    b = bursts(1, 9); grad_case("2: nine bursts, n_epochs = 0", &b, ep, 0);
  }

  // check_layout for both launch-time layouts
  f = fields(); layout_case("valid", &f);
  layout_case("fields NULL", nullptr);
  f = fields(); f.dtype = RJP_F32; f.d_a0 = nullptr; layout_case("f32 fields", &f);
  layout_case("2: f32 fields, K = 0", &f, 0, 0);
  f = fields(); f.d_a0 = nullptr; layout_case("fields.d_a0 NULL", &f);
  f = fields(); f.d_ts = nullptr; layout_case("fields.d_ts NULL", &f);
  f = fields(); f.ny = 0; layout_case("fields.ny = 0", &f);
  f = fields(); layout_case("K = 0", &f, 0, 0);
  layout_case("K above the limit", &f, 81, 33);
  f.ts_lo = f.ts_hi = 0.0; layout_case("no launch-time range", &f);
  layout_case("2: K = 0, no launch-time range", &f, 0, 0);
  f = fields(); f.ts_lo = 2.0; f.ts_hi = 1.0; layout_case("ts_hi < ts_lo", &f);
  f = fields(); f.ts_hi = INFINITY; layout_case("ts_hi infinite", &f);
  {
    std::string m;
    f = fields(); f.ny = 65536;
    put("rjp_lt_count", "fields.ny = 65536",
        A::check_layout(&f, 4, "launch-time-ordered layout", 80, 65536, m), m);
    put("rjp_srt_count", "valid", A::check_layout(&f, 4, "launch-time-bucketed layout", 32, 0, m), m);
  }
  return 0;
}
