// Compile-and-run check of the pose-fix and quaternion-variable part of include/uvio_hp.hpp.
//   facade_pose_check <config> nogpu   no device needed: feed_pose, pose_results and add_quat_state are instantiated and
//       Manager construction fails loudly with UVIO_HP_E_DEVICE on a host without a GPU
//   facade_pose_check <config> gpu     on the device: a quaternion variable is added (normalized on entry, 4 values over
//       3 error columns, kind 7), pose fixes are queued against it and against constants, one queued before
//       initialization or at the state time is not kept, malformed ones are refused with UVIO_HP_E_ARG, and pose_results
//       is empty before any frame
#include <cmath>
#include <cstdio>
#include <cstring>

#include "uvio_hp.hpp"

static int run_gpu(const char *cfg) {
  uvio_hp_options_t o;
  if (uvio_hp_options_default(&o) || uvio_hp_options_load(cfg, &o)) return 10;
  o.max_aux_dim = 8;
  uvio_amd::Manager m(o, 0);
  const std::array<double, 4> zq = {0.0, 0.0, 0.0, 1.0};
  const std::array<double, 3> zp = {1.0, 2.0, 3.0};
  const std::vector<double> R3 = {1e-6, 0.0, 0.0, 0.0, 1e-6, 0.0, 0.0, 0.0, 1e-6};
  std::vector<double> R6(36, 0.0);
  for (size_t k = 0; k < 6; k++) R6[7 * k] = k < 3 ? 1e-6 : 1e-4;
  R6[3] = 1e-6;  // rotation and translation coupled (upper triangle)
  if (m.feed_pose(1.0, zq, zp, R6)) return 11;  // not initialized: not kept
  m.initialize_with_gt({0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0});
  const int n0 = m.cov_dim();
  const std::array<double, 9> prior = {1e-2, 0.0, 0.0, 0.0, 1e-2, 0.0, 0.0, 0.0, 1e-2};
  const int hq = m.add_quat_state({0.0, 0.0, 2.0 * std::sin(0.1), 2.0 * std::cos(0.1)}, prior, {1e-3, 1e-3, 1e-3});
  const uvio_amd::Manager::AuxState a = m.aux_state(hq);
  if (a.id != n0 || a.value.size() != 4 || m.cov_dim() != n0 + 3) return 12;
  if (std::fabs(a.value[2] - std::sin(0.1)) > 1e-15 || std::fabs(a.value[3] - std::cos(0.1)) > 1e-15) return 13;
  bool kind7 = false;
  for (const auto &v : m.state_meta()) kind7 = kind7 || (v[0] == 7 && v[1] == n0 && v[2] == 3);
  if (!kind7) return 14;
  try {
    m.add_quat_state({0.0, 0.0, 0.0, 3.0}, prior);
    return 25;
  } catch (const uvio_amd::Error &e) {
    if (e.code != UVIO_HP_E_ARG) return 26;
  }
  const int ha = m.add_state({0.2, -0.05, 0.1}, {1e-2, 0.0, 0.0, 0.0, 1e-2, 0.0, 0.0, 0.0, 1e-2});
  if (m.aux_state(ha).value.size() != 3) return 15;
  if (m.feed_pose(0.0, zq, zp, R6)) return 16;  // at the state time: not kept
  if (!m.feed_pose(0.01, zq, zp, R3)) return 17;  // orientation only, identity mounting
  if (!m.feed_pose(0.01, zq, zp, R6, {0.0, 0.0, 0.0, 1.0}, hq, {0.0, 0.0, 0.0}, ha)) return 18;
  try {
    m.feed_pose(0.02, {0.0, 0.0, 0.0, 3.0}, zp, R3);  // a norm outside [0.5, 2]
    return 19;
  } catch (const uvio_amd::Error &e) {
    if (e.code != UVIO_HP_E_ARG) return 20;
    std::printf("refused: code %d: %s\n", e.code, e.what());
  }
  try {
    m.feed_pose(0.02, zq, zp, R6, {0.0, 0.0, 0.0, 1.0}, ha);  // the rotation handle names an additive vector
    return 21;
  } catch (const uvio_amd::Error &e) {
    if (e.code != UVIO_HP_E_ARG) return 22;
  }
  try {
    m.feed_pose(0.02, zq, zp, std::vector<double>(16, 1.0));
    return 23;
  } catch (const uvio_amd::Error &e) {
    if (e.code != UVIO_HP_E_ARG) return 24;
  }
  if (!m.pose_results().empty() || !m.position_results().empty()) return 27;
  m.remove_state(hq);
  m.remove_state(ha);
  if (m.cov_dim() != n0) return 28;
  std::printf("POSE ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  auto f1 = &uvio_amd::Manager::feed_pose;
  auto f2 = &uvio_amd::Manager::pose_results;
  auto f3 = &uvio_amd::Manager::add_quat_state;
  (void)f1, (void)f2, (void)f3;
  try {
    if (!std::strcmp(argv[2], "gpu")) return run_gpu(argv[1]);
    if (std::strcmp(argv[2], "nogpu")) return 2;
    uvio_amd::Manager m(argv[1], 0);
    m.feed_pose(1.0, {0.0, 0.0, 0.0, 1.0}, {0.0, 0.0, 0.0}, std::vector<double>(9, 0.0));
    const std::vector<uvio_amd::Manager::PositionResult> res = m.pose_results();
    return res.empty() ? 4 : 3;
  } catch (const uvio_amd::Error &e) {
    std::printf("code %d: %s\n", e.code, e.what());
    return (e.code == UVIO_HP_E_DEVICE && std::strcmp(argv[2], "gpu")) ? 0 : 5;  // (gpu: every error fails)
  }
}
