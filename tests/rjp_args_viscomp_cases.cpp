// check_vis_components and check_components_image of rajepy_amd/csrc/rjp_args.h -- the pure argument
// checks of rjp_vis_components and rjp_components_image -- driven from a plain C++ program (no HIP):
// one line "case<TAB>status<TAB>message" per case, in the order the checks refuse;
// tests/test_vis_components_reference_cpu.py holds the lines to the messages that
// tests/test_gpu_vis_components.py sees from the library.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>

#include "rjp_args.h"

namespace A = rjp_args;

static double* const kD = (double*)0x1000;      // stand for device pointers: never dereferenced
static int32_t* const kI = (int32_t*)0x2000;

struct Vc {
  const int32_t *cpix = kI, *ncomp = kI;
  const double *cflux = kD, *u = kD, *v = kD, *gvis = kD, *out = kD;
  int n_maps = 2, stride = 7, n_s = 3, nx = 5, nz = 3, n_vis = 65, sign = -1;
  double su[64], sv[64];                        // (64 maps: what the workgroup limit takes)
  Vc() {
    for (int m = 0; m < 64; ++m) { su[m] = m & 1 ? -0.25 : 0.5; sv[m] = 0.125 * (m + 1); }
  }
  bool null_su = false, null_sv = false;
};

static void put(const char* name, const Vc& a) {
  std::string m;
  const int r = A::check_vis_components(a.cpix, a.cflux, a.ncomp, a.n_maps, a.stride, a.n_s, a.nx,
                                        a.nz, a.null_su ? nullptr : a.su,
                                        a.null_sv ? nullptr : a.sv, a.u, a.v, a.n_vis, a.gvis,
                                        a.sign, a.out, m);
  std::printf("%s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

struct Ci {
  const int32_t *cpix = kI, *ncomp = kI;
  const double *cflux = kD, *out = kD;
  int n_maps = 2, stride = 7, n_s = 3, nx = 5, nz = 3;
};

static void put(const char* name, const Ci& a) {
  std::string m;
  const int r = A::check_components_image(a.cpix, a.cflux, a.ncomp, a.n_maps, a.stride, a.n_s,
                                          a.nx, a.nz, a.out, m);
  std::printf("%s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  Vc a;
  put("valid", a);
  a = Vc(); a.sign = 1; put("valid sign +1", a);
  a = Vc(); a.gvis = nullptr; a.n_s = 1; put("valid hogbom", a);
  a = Vc(); a.n_maps = a.stride = a.n_s = a.nx = a.nz = a.n_vis = 1; put("valid 1", a);
  a = Vc(); a.cpix = nullptr; put("NULL d_cpix", a);
  a = Vc(); a.cflux = nullptr; put("NULL d_cflux", a);
  a = Vc(); a.ncomp = nullptr; put("NULL d_ncomp", a);
  a = Vc(); a.null_su = true; put("NULL h_su", a);
  a = Vc(); a.null_sv = true; put("NULL h_sv", a);
  a = Vc(); a.u = nullptr; put("NULL d_u", a);
  a = Vc(); a.v = nullptr; put("NULL d_v", a);
  a = Vc(); a.out = nullptr; put("NULL d_out", a);
  a = Vc(); a.n_maps = 0; put("n_maps 0", a);
  a = Vc(); a.stride = 0; put("comp_stride 0", a);
  a = Vc(); a.n_s = 0; put("n_s 0", a);
  a = Vc(); a.nx = 0; put("nx 0", a);
  a = Vc(); a.nz = -1; put("nz -1", a);
  a = Vc(); a.n_vis = 0; put("n_vis 0", a);
  a = Vc(); a.sign = 0; put("sign 0", a);
  a = Vc(); a.sign = 2; put("sign 2", a);
  a = Vc(); a.gvis = nullptr; put("NULL d_gvis n_s 3", a);
  a = Vc(); a.su[1] = nan; put("su nan", a);
  a = Vc(); a.sv[0] = -inf; put("sv inf", a);
  a = Vc(); a.nx = 46341; a.nz = 46341; put("nx nz 2^31", a);
  a = Vc(); a.n_maps = 64; a.n_vis = 2147483647; put("workgroups", a);
  a = Vc(); a.n_maps = 63; a.n_vis = 2147483647; put("valid 63 x 2^25 workgroups", a);
  // which one wins
  a = Vc(); a.out = nullptr; a.n_vis = 0; put("NULL beats sizes", a);
  a = Vc(); a.n_vis = 0; a.sign = 0; put("sizes beat sign", a);
  a = Vc(); a.sign = 0; a.gvis = nullptr; put("sign beats gvis", a);
  a = Vc(); a.gvis = nullptr; a.su[0] = nan; put("gvis beats scales", a);
  a = Vc(); a.su[0] = nan; a.nx = a.nz = 46341; put("scales beat the image size", a);
  a = Vc(); a.nx = a.nz = 46341; a.n_maps = 64; a.n_vis = 2147483647; put("image size beats workgroups", a);

  Ci c;
  put("img valid", c);
  c = Ci(); c.n_maps = c.stride = c.n_s = c.nx = c.nz = 1; put("img valid 1", c);
  c = Ci(); c.cpix = nullptr; put("img NULL d_cpix", c);
  c = Ci(); c.cflux = nullptr; put("img NULL d_cflux", c);
  c = Ci(); c.ncomp = nullptr; put("img NULL d_ncomp", c);
  c = Ci(); c.out = nullptr; put("img NULL d_out", c);
  c = Ci(); c.n_maps = 0; put("img n_maps 0", c);
  c = Ci(); c.stride = -2; put("img comp_stride -2", c);
  c = Ci(); c.n_s = 0; put("img n_s 0", c);
  c = Ci(); c.nx = 0; put("img nx 0", c);
  c = Ci(); c.nz = 0; put("img nz 0", c);
  c = Ci(); c.nx = 46341; c.nz = 46341; put("img nx nz 2^31", c);
  c = Ci(); c.nx = 46340; c.nz = 46340; c.n_s = 300; put("img workgroups", c);
  c = Ci(); c.out = nullptr; c.nx = 0; put("img NULL beats sizes", c);
  c = Ci(); c.nx = 0; c.nz = 0; c.n_s = 0; put("img sizes first", c);
  return 0;
}
