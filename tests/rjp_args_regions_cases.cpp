// check_image_stats, check_label_regions and check_mask_grow of rajepy_amd/csrc/rjp_args.h -- the
// pure argument checks of K25 -- driven from a plain C++ program (no HIP): one line
// "case<TAB>status<TAB>message" per case, in the order the checks refuse;
// tests/test_regions_reference_cpu.py holds the lines to the messages that tests/test_gpu_regions.py
// sees from the library.
#include <cstdio>
#include <string>

#include "rjp_args.h"

namespace A = rjp_args;

static double* const kD = (double*)0x1000;      // stand for device pointers: never dereferenced
static uint8_t* const kB = (uint8_t*)0x2000;
static int32_t* const kI = (int32_t*)0x3000;

struct St {
  const double* img = kD;
  int n_maps = 3, nx = 40, nz = 50;
  const uint8_t* mask = nullptr;
  int n_mask = 7;                                // (not looked at without a mask)
  const double* stats = kD;
};
struct Lb {
  const uint8_t* mask = kB;
  int n_mask = 3, n_maps = 3, nx = 40, nz = 50, conn = 1;
  const int32_t *label = kI, *nreg = kI;
};
struct Gr {
  const uint8_t *seed = kB, *con = kB;
  int n_mask = 1, n_maps = 3, nx = 40, nz = 50, conn = 2;
};

static void line(const char* name, int r, const std::string& m) {
  std::printf("%s\t%d\t%s\n", name, r, r ? m.c_str() : "");
}
static void put(const char* name, const St& a) {
  std::string m;
  line(name, A::check_image_stats(a.img, a.n_maps, a.nx, a.nz, a.mask, a.n_mask, a.stats, m), m);
}
static void put(const char* name, const Lb& a) {
  std::string m;
  line(name, A::check_label_regions(a.mask, a.n_mask, a.n_maps, a.nx, a.nz, a.conn, a.label, a.nreg, m), m);
}
static void put(const char* name, const Gr& a) {
  std::string m;
  line(name, A::check_mask_grow(a.seed, a.con, a.n_mask, a.n_maps, a.nx, a.nz, a.conn, m), m);
}

int main() {
  St s;
  put("stats valid", s);
  s = St(); s.mask = kB; s.n_mask = 1; put("stats valid shared mask", s);
  s = St(); s.mask = kB; s.n_mask = 3; put("stats valid mask per map", s);
  s = St(); s.n_maps = 65535; s.nx = 1; s.nz = 1; put("stats valid 65535 maps", s);
  s = St(); s.n_maps = 1; s.nx = 1048560; s.nz = 2048; put("stats valid 2^31 - 2^15 pixels", s);
  s = St(); s.img = nullptr; put("stats NULL d_img", s);
  s = St(); s.stats = nullptr; put("stats NULL d_stats", s);
  s = St(); s.stats = nullptr; s.nx = 0; put("stats NULL beats sizes", s);
  s = St(); s.n_maps = 0; put("stats n_maps 0", s);
  s = St(); s.nx = -1; put("stats nx -1", s);
  s = St(); s.nz = 0; s.mask = kB; s.n_mask = 2; put("stats sizes beat n_mask", s);
  s = St(); s.n_maps = 65536; put("stats n_maps 65536", s);
  s = St(); s.nx = 1048561; s.nz = 1; put("stats nx 1048561", s);
  s = St(); s.nx = 65536; s.nz = 32768; put("stats 2^31 pixels", s);
  s = St(); s.mask = kB; s.n_mask = 2; put("stats n_mask 2", s);
  s = St(); s.mask = kB; s.n_mask = 0; put("stats n_mask 0", s);
  s = St(); s.n_maps = 65535; s.nx = 8192; s.nz = 8200; put("stats 2^31 workgroups", s);

  Lb l;
  put("label valid", l);
  l = Lb(); l.n_mask = 1; l.conn = 2; put("label valid shared mask", l);
  l = Lb(); l.mask = nullptr; put("label NULL d_mask_in", l);
  l = Lb(); l.label = nullptr; put("label NULL d_label", l);
  l = Lb(); l.nreg = nullptr; put("label NULL d_nreg", l);
  l = Lb(); l.nz = 0; put("label nz 0", l);
  l = Lb(); l.n_maps = 65536; l.n_mask = 65536; put("label n_maps 65536", l);
  l = Lb(); l.nx = 1048561; l.nz = 1; put("label nx 1048561", l);
  l = Lb(); l.nx = 65536; l.nz = 32768; l.n_mask = 2; put("label 2^31 pixels beat n_mask", l);
  l = Lb(); l.n_mask = 2; l.conn = 3; put("label n_mask beats connectivity", l);
  l = Lb(); l.n_mask = 4; put("label n_mask 4", l);
  l = Lb(); l.conn = 0; put("label connectivity 0", l);
  l = Lb(); l.conn = 3; put("label connectivity 3", l);

  Gr g;
  put("grow valid", g);
  g = Gr(); g.n_mask = 3; g.conn = 1; put("grow valid constraint per map", g);
  g = Gr(); g.seed = nullptr; put("grow NULL d_seed", g);
  g = Gr(); g.con = nullptr; put("grow NULL d_con", g);
  g = Gr(); g.n_maps = 0; put("grow n_maps 0", g);
  g = Gr(); g.n_maps = 65536; put("grow n_maps 65536", g);
  g = Gr(); g.nx = 1048561; g.nz = 1; put("grow nx 1048561", g);
  g = Gr(); g.nx = 65536; g.nz = 32768; g.conn = 7; put("grow 2^31 pixels beat connectivity", g);
  g = Gr(); g.n_mask = 2; put("grow n_mask 2", g);
  g = Gr(); g.n_mask = 2; g.conn = 4; put("grow n_mask beats connectivity", g);
  g = Gr(); g.conn = 4; put("grow connectivity 4", g);
  return 0;
}
