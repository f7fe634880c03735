// Compile-and-run check of the measurement-update part of include/uvio_hp.hpp on a host without a GPU: the facade
// methods are instantiated, position_fix_jacobian is evaluated at the pose and lever arm given on the command line
// (q x y z w, p, p_SinI: 10 numbers after the config path) and printed with 17 digits for the finite-difference test,
// chi2_95 is read through the library, and Manager construction fails loudly with UVIO_HP_E_DEVICE.
#include <cstdio>
#include <cstdlib>

#include "uvio_hp.hpp"

int main(int argc, char **argv) {
  if (argc < 12) return 2;
  auto f1 = &uvio_amd::Manager::propagate;
  auto f2 = &uvio_amd::Manager::measurement_update;
  auto f3 = &uvio_amd::Manager::position_fix;
  auto f4 = &uvio_amd::Manager::state_meta;
  (void)f1, (void)f2, (void)f3, (void)f4;

  double imu[7];
  for (int k = 0; k < 7; k++) imu[k] = std::atof(argv[2 + k]);
  const std::array<double, 3> s = {std::atof(argv[9]), std::atof(argv[10]), std::atof(argv[11])};
  double h[3], H[18];
  uvio_amd::position_fix_jacobian(imu, s, h, H);
  std::printf("JAC");
  for (int k = 0; k < 3; k++) std::printf(" %.17g", h[k]);
  for (int k = 0; k < 18; k++) std::printf(" %.17g", H[k]);
  std::printf("\n");
  std::printf("CHI2 %.17g %.17g\n", uvio_amd::chi2_95(1), uvio_amd::chi2_95(3));
  try {
    uvio_amd::chi2_95(0);
    return 3;
  } catch (const uvio_amd::Error &e) {
    if (e.code != UVIO_HP_E_ARG) return 3;
  }
  try {
    uvio_amd::Manager m(argv[1], 0);
    m.propagate(1.0);
    const auto out = m.position_fix({0.0, 0.0, 0.0}, s, {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0});
    std::printf("created %d\n", (int)out.applied);
    return 4;
  } catch (const uvio_amd::Error &e) {
    std::printf("code %d: %s\n", e.code, e.what());
    return e.code == UVIO_HP_E_DEVICE ? 0 : 5;
  }
}
