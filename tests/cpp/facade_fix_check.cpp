// Compile-and-run check of the buffered position-fix part of include/uvio_hp.hpp.
//   facade_fix_check <config> nogpu   no device needed: feed_position and position_results are instantiated and Manager
//       construction fails loudly with UVIO_HP_E_DEVICE on a host without a GPU
//   facade_fix_check <config> gpu     on the device: a fix queued before initialization or at the state time is not
//       kept, a malformed one is refused with UVIO_HP_E_ARG, and position_results is empty before any frame
#include <cstdio>
#include <cstring>

#include "uvio_hp.hpp"

static int run_gpu(const char *cfg) {
  uvio_amd::Manager m(cfg, 0);
  const std::vector<double> I3 = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  const std::vector<double> R3 = {1e-4, 0.0, 0.0, 0.0, 1e-4, 0.0, 0.0, 0.0, 1e-4};
  if (m.feed_position(1.0, {1.0, 2.0, 3.0}, I3, R3)) return 10;  // not initialized: not kept
  m.initialize_with_gt({0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 2.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0});
  if (m.feed_position(0.0, {1.0, 2.0, 3.0}, I3, R3)) return 11;  // at the state time: not kept
  if (!m.feed_position(0.01, {1.0, 2.0, 3.0}, I3, R3, {0.2, -0.05, 0.1})) return 12;
  if (!m.feed_position(0.01, {3.0}, {0.0, 0.0, 1.0}, {1e-2})) return 13;  // an altimeter
  try {
    m.feed_position(0.02, {1.0, 2.0, 3.0}, I3, {1e-4, 0.0, 0.0, 0.0, -1e-4, 0.0, 0.0, 0.0, 1e-4});
    return 14;
  } catch (const uvio_amd::Error &e) {
    if (e.code != UVIO_HP_E_ARG) return 15;
    std::printf("refused: code %d: %s\n", e.code, e.what());
  }
  try {
    m.feed_position(0.02, {1.0, 2.0, 3.0}, I3, R3, {0.0, 0.0, 0.0}, 7);  // no such aux variable
    return 16;
  } catch (const uvio_amd::Error &e) {
    if (e.code != UVIO_HP_E_ARG) return 17;
  }
  if (!m.position_results().empty()) return 18;
  std::printf("FIX ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  auto f1 = &uvio_amd::Manager::feed_position;
  auto f2 = &uvio_amd::Manager::position_results;
  (void)f1, (void)f2;
  try {
    if (!std::strcmp(argv[2], "gpu")) return run_gpu(argv[1]);
    if (std::strcmp(argv[2], "nogpu")) return 2;
    uvio_amd::Manager m(argv[1], 0);
    m.feed_position(1.0, {0.0}, {0.0, 0.0, 1.0}, {1.0});
    const std::vector<uvio_amd::Manager::PositionResult> res = m.position_results();
    return res.empty() ? 4 : 3;
  } catch (const uvio_amd::Error &e) {
    std::printf("code %d: %s\n", e.code, e.what());
    return (e.code == UVIO_HP_E_DEVICE && std::strcmp(argv[2], "gpu")) ? 0 : 5;  // (gpu: every error fails)
  }
}
