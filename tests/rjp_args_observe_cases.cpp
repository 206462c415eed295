// check_uv_tracks and check_vis_noise of rajepy_amd/csrc/rjp_args.h -- the pure argument checks of
// rjp_uv_tracks and rjp_vis_noise -- driven from a plain C++ program (no HIP): one line
// "case<TAB>status<TAB>message" per case, in the order the checks refuse;
// tests/test_observe_reference_cpu.py holds the lines to the messages that tests/test_gpu_observe.py
// sees from the library.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "rjp_args.h"

namespace A = rjp_args;

static double* const kD = (double*)0x1000;      // stand for device pointers: never dereferenced

struct Tracks {
  std::vector<double> xyz = {1.0, 2.0, 3.0, -4.0, 5.0, 6.5, 7.0, -8.0, 9.0};
  int n_ant = 3, n_t = 2;
  double gha[2] = {0.25, -1.5};
  bool null_xyz = false, null_gha = false;
  double sd = 0.6, cd = 0.8;
  const double *u = kD, *v = kD;
};

static void put(const char* name, const Tracks& a) {
  std::string m;
  const int r = A::check_uv_tracks(a.null_xyz ? nullptr : a.xyz.data(), a.n_ant,
                                   a.null_gha ? nullptr : a.gha, a.n_t, a.sd, a.cd, a.u, a.v, m);
  std::printf("tracks %s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

struct Noise {
  const double* vis = kD;
  int n_maps = 2, n_vis = 7;
  double sigma[2] = {0.0, 1.5};
  bool null_sigma = false;
  int64_t k0 = 0;
  int32_t m0 = 0;
  const double* out = kD;
};

static void put(const char* name, const Noise& a) {
  std::string m;
  const int r = A::check_vis_noise(a.vis, a.n_maps, a.n_vis, a.null_sigma ? nullptr : a.sigma, a.k0,
                                   a.m0, a.out, m);
  std::printf("noise %s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  Tracks a;
  put("valid", a);
  a = Tracks(); a.gha[0] = nan; a.gha[1] = inf; put("valid non-finite hour angles flag", a);
  a = Tracks(); a.sd = std::sin(0.3); a.cd = std::cos(0.3); put("valid unit circle", a);
  a = Tracks(); a.sd = 1.0; a.cd = 4e-7; put("valid within 1e-12", a);
  a = Tracks(); a.xyz.assign(3 * 65536, 0.0); a.n_ant = 65536; a.n_t = 1; put("valid 2^31 - 32768 outputs", a);
  a = Tracks(); a.null_xyz = true; put("NULL h_xyz", a);
  a = Tracks(); a.null_gha = true; put("NULL h_gha", a);
  a = Tracks(); a.u = nullptr; put("NULL d_u", a);
  a = Tracks(); a.v = nullptr; put("NULL d_v", a);
  a = Tracks(); a.n_ant = 1; put("n_ant 1", a);
  a = Tracks(); a.n_ant = -3; put("n_ant -3", a);
  a = Tracks(); a.n_t = 0; put("n_t 0", a);
  a = Tracks(); a.xyz[8] = nan; put("xyz nan", a);
  a = Tracks(); a.xyz[0] = -inf; put("xyz inf", a);
  a = Tracks(); a.sd = nan; put("sin_dec nan", a);
  a = Tracks(); a.cd = inf; put("cos_dec inf", a);
  a = Tracks(); a.sd = 0.6; a.cd = 0.8 + 1e-11; put("off the circle", a);
  a = Tracks(); a.sd = 0.0; a.cd = 0.0; put("zero vector", a);
  a = Tracks(); a.xyz.assign(3 * 65536, 0.0); a.n_ant = 65536; a.n_t = 2; put("2^32 outputs", a);
  a = Tracks(); a.xyz.assign(3 * 3, 0.0); a.n_t = 715827883; put("3 x 715827883 outputs", a);
  // which one wins
  a = Tracks(); a.u = nullptr; a.n_ant = 0; put("NULL beats n_ant", a);
  a = Tracks(); a.n_ant = 1; a.n_t = 0; put("n_ant beats n_t", a);
  a = Tracks(); a.n_t = 0; a.xyz[1] = nan; put("n_t beats xyz", a);
  a = Tracks(); a.xyz[1] = nan; a.sd = nan; put("xyz beats the declination", a);
  a = Tracks(); a.sd = inf; a.cd = 0.0; put("non-finite beats the circle", a);

  Noise b;
  put("valid", b);
  b = Noise(); b.k0 = INT64_MAX - 7; b.m0 = INT32_MAX - 2; put("valid largest offsets", b);
  b = Noise(); b.out = b.vis; put("valid in place", b);
  b = Noise(); b.vis = nullptr; put("NULL d_vis", b);
  b = Noise(); b.null_sigma = true; put("NULL h_sigma", b);
  b = Noise(); b.out = nullptr; put("NULL d_out", b);
  b = Noise(); b.n_maps = 0; put("n_maps 0", b);
  b = Noise(); b.n_vis = -1; put("n_vis -1", b);
  b = Noise(); b.sigma[1] = -1e-300; put("sigma negative", b);
  b = Noise(); b.sigma[0] = nan; put("sigma nan", b);
  b = Noise(); b.sigma[1] = inf; put("sigma inf", b);
  b = Noise(); b.k0 = -1; put("k0 -1", b);
  b = Noise(); b.k0 = INT64_MAX - 6; put("k0 + n_vis 2^63", b);
  b = Noise(); b.m0 = -1; put("m0 -1", b);
  b = Noise(); b.m0 = INT32_MAX - 1; put("m0 + n_maps 2^31", b);
  // which one wins
  b = Noise(); b.vis = nullptr; b.n_vis = 0; put("NULL beats sizes", b);
  b = Noise(); b.n_vis = 0; b.sigma[0] = nan; put("sizes beat sigma", b);
  b = Noise(); b.sigma[0] = nan; b.k0 = -1; put("sigma beats k0", b);
  b = Noise(); b.k0 = -1; b.m0 = -1; put("k0 beats m0", b);
  return 0;
}
