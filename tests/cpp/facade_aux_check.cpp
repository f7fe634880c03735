// Compile-and-run check of the aux-state part of include/uvio_hp.hpp.
//   facade_aux_check <config> jac q(4) p(3) p_AinI(3)   no device needed: position_fix_lever_arm_jacobian at the given
//       pose, printed with 17 digits for the finite-difference test; the facade methods are instantiated and Manager
//       construction fails loudly with UVIO_HP_E_DEVICE on a host without a GPU
//   facade_aux_check <config> gpu                        on the device: add a lever arm to an initialized estimator,
//       read it, run position_fix_lever_arm, remove it, and see the dead handle refused
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "uvio_hp.hpp"

static int run_gpu(const char *cfg) {
  uvio_hp_options_t o;
  if (uvio_hp_options_default(&o) || uvio_hp_options_load(cfg, &o)) return 10;
  o.max_aux_dim = 8;
  uvio_amd::Manager m(o, 0);
  m.initialize_with_gt({0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0});
  const int n0 = m.cov_dim();
  const std::vector<double> arm = {0.2, -0.05, 0.1};
  const int h = m.add_state(arm, {1e-2, 0.0, 0.0, 0.0, 1e-2, 0.0, 0.0, 0.0, 1e-2});
  const uvio_amd::Manager::AuxState a = m.aux_state(h);
  if (a.id != n0 || a.value != arm || m.cov_dim() != n0 + 3) return 11;
  bool kind6 = false;
  for (const auto &v : m.state_meta()) kind6 = kind6 || (v[0] == 6 && v[1] == n0 && v[2] == 3);
  if (!kind6) return 12;
  // identity attitude: the prediction is p + p_AinI; a fix 1 cm off in x
  const auto out = m.position_fix_lever_arm({1.21, 1.95, 3.1}, h, {1e-4, 0.0, 0.0, 0.0, 1e-4, 0.0, 0.0, 0.0, 1e-4});
  if (!out.applied || (int)out.dx.size() != n0 + 3) return 13;
  const uvio_amd::Manager::AuxState b = m.aux_state(h);
  for (int k = 0; k < 3; k++)
    if (b.value[(size_t)k] != arm[(size_t)k] + out.dx[(size_t)(n0 + k)]) return 14;
  std::printf("AUX applied chi2 %.17g dx %.17g %.17g %.17g\n", out.chi2, out.dx[(size_t)n0], out.dx[(size_t)n0 + 1],
              out.dx[(size_t)n0 + 2]);
  m.remove_state(h);
  if (m.cov_dim() != n0) return 15;
  try {
    m.aux_state(h);
    return 16;
  } catch (const uvio_amd::Error &e) {
    if (e.code != UVIO_HP_E_ARG) return 17;
    std::printf("dead handle: code %d: %s\n", e.code, e.what());
  }
  const int h2 = m.add_state_from_measurement({0.0}, {{0, 6}}, {0.0, 0.0, 0.0, 0.0, 0.0, 1.0}, {2.0}, {0.5}, {1e-2}, {0.1});
  if (m.aux_state(h2).value[0] != 0.25) return 18;
  std::printf("AUX ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  auto f1 = &uvio_amd::Manager::add_state;
  auto f2 = &uvio_amd::Manager::add_state_from_measurement;
  auto f3 = &uvio_amd::Manager::aux_state;
  auto f4 = &uvio_amd::Manager::remove_state;
  auto f5 = &uvio_amd::Manager::position_fix_lever_arm;
  (void)f1, (void)f2, (void)f3, (void)f4, (void)f5;
  try {
    if (!std::strcmp(argv[2], "gpu")) return run_gpu(argv[1]);
    if (std::strcmp(argv[2], "jac") || argc < 13) return 2;
    double imu[7];
    for (int k = 0; k < 7; k++) imu[k] = std::atof(argv[3 + k]);
    const std::array<double, 3> s = {std::atof(argv[10]), std::atof(argv[11]), std::atof(argv[12])};
    double h[3], H[27];
    uvio_amd::position_fix_lever_arm_jacobian(imu, s, h, H);
    std::printf("JACL");
    for (int k = 0; k < 3; k++) std::printf(" %.17g", h[k]);
    for (int k = 0; k < 27; k++) std::printf(" %.17g", H[k]);
    std::printf("\n");
    uvio_amd::Manager m(argv[1], 0);
    m.add_state({0.0}, {1.0});
    return 4;
  } catch (const uvio_amd::Error &e) {
    std::printf("code %d: %s\n", e.code, e.what());
    return (e.code == UVIO_HP_E_DEVICE && std::strcmp(argv[2], "gpu")) ? 0 : 5;  // (gpu: every error fails)
  }
}
