// Stand-alone driver of uvio_amd/csrc/fast_prop.h and select_imu (imu_math.h) for tests/test_fast_propagate.py:
// reads cases from a text file, runs the queries of each on one cache and prints every output at full precision.
//
// Input, whitespace separated:
//   ncases
//   per case: imu_model dw[6] da[6] tg[9] q_acc[4] q_gyro[4]
//             sigma_w sigma_a sigma_wb sigma_ab gravity_mag
//             t est[16] cov[225] t_off
//             nimu, then nimu x (t wm[3] am[3])
//             nquery, then nquery x t
// Output per query: "ok" state_plus[13] cov[144] cache_t cache_t_off est[16] cov15[225], or "no"; the outputs are
// pre-filled with a sentinel and printed after "no" as well (the call must leave them untouched).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fast_prop.h"

using namespace uvhp;

static double rd(FILE *f) {
  double v = 0;
  if (std::fscanf(f, "%lf", &v) != 1) {
    std::fprintf(stderr, "fast_prop_check: short input\n");
    std::exit(3);
  }
  return v;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int ncases = (int)rd(f);
  for (int c = 0; c < ncases; c++) {
    const int model = (int)rd(f);
    double dw[6], da[6], tg[9], qa[4], qg[4];
    for (double &v : dw) v = rd(f);
    for (double &v : da) v = rd(f);
    for (double &v : tg) v = rd(f);
    for (double &v : qa) v = rd(f);
    for (double &v : qg) v = rd(f);
    fastprop::Noise nz;
    const double sw = rd(f), sa = rd(f), swb = rd(f), sab = rd(f);
    nz.sigma_w_2 = sw * sw, nz.sigma_a_2 = sa * sa, nz.sigma_wb_2 = swb * swb, nz.sigma_ab_2 = sab * sab;
    nz.gravity_mag = rd(f);
    fastprop::Cache cache;
    fastprop::make_calib(model, dw, da, tg, qa, qg, &cache.calib);
    cache.t = rd(f);
    for (double &v : cache.est) v = rd(f);
    for (double &v : cache.cov) v = rd(f);
    cache.t_off = rd(f);
    const int nimu = (int)rd(f);
    std::vector<ImuSample> imu((size_t)nimu);
    for (auto &s : imu) {
      s.t = rd(f);
      for (double &v : s.wm) v = rd(f);
      for (double &v : s.am) v = rd(f);
    }
    const int nq = (int)rd(f);
    for (int q = 0; q < nq; q++) {
      const double t = rd(f);
      double sp[13], cv[144];
      for (double &v : sp) v = -777.0;
      for (double &v : cv) v = -777.0;
      const bool ok = fastprop::query(cache, nz, imu, t, sp, cv);
      std::printf(ok ? "ok" : "no");
      for (double v : sp) std::printf(" %.17g", v);
      for (double v : cv) std::printf(" %.17g", v);
      std::printf(" %.17g %.17g", cache.t, cache.t_off);
      for (double v : cache.est) std::printf(" %.17g", v);
      for (double v : cache.cov) std::printf(" %.17g", v);
      std::printf("\n");
    }
  }
  std::fclose(f);
  return 0;
}
