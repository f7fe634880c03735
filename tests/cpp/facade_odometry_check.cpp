// Compile-and-run check of the odometry / marginal-covariance part of include/uvio_hp.hpp on a host without a
// GPU: the four facade methods are instantiated, the ROS covariance reordering (ROS1Visualizer.cpp:311-325) is
// checked on a 12 x 12 of distinct integers, and Manager construction fails loudly with UVIO_HP_E_DEVICE.
#include <cstdio>

#include "uvio_hp.hpp"

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  auto f1 = &uvio_amd::Manager::marginal_covariance;
  auto f2 = &uvio_amd::Manager::good_features_MSCKF;
  auto f3 = &uvio_amd::Manager::enable_odometry;
  auto f4 = &uvio_amd::Manager::fast_state_propagate;
  (void)f1, (void)f2, (void)f3, (void)f4;

  // cov(r, c) = 100 r + c: every entry distinct, so each output names the entry it came from
  std::array<double, 144> cov{};
  for (int r = 0; r < 12; r++)
    for (int c = 0; c < 12; c++) cov[(size_t)(12 * r + c)] = 100.0 * r + c;
  std::array<double, 36> pose{}, twist{};
  uvio_amd::odometry_covariance_ros(cov, pose, twist);
  // Phi = [0 I 0; I 0 0; 0 0 I6], cov' = Phi cov Phi^T: row / column k of the pose block is p (k < 3) or theta
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) {
      const int sr = r < 3 ? r + 3 : r - 3, sc = c < 3 ? c + 3 : c - 3;
      if (pose[(size_t)(6 * r + c)] != 100.0 * sr + sc) {
        std::printf("pose(%d, %d) = %g\n", r, c, pose[(size_t)(6 * r + c)]);
        return 6;
      }
      if (twist[(size_t)(6 * r + c)] != 100.0 * (r + 6) + (c + 6)) {
        std::printf("twist(%d, %d) = %g\n", r, c, twist[(size_t)(6 * r + c)]);
        return 7;
      }
    }
  std::printf("reorder ok\n");
  try {
    uvio_amd::Manager m(argv[1], 0);
    uvio_amd::Manager::Odometry od;
    m.enable_odometry(true);
    std::printf("created %d\n", (int)m.fast_state_propagate(0.0, od));
    return 4;
  } catch (const uvio_amd::Error &e) {
    std::printf("code %d: %s\n", e.code, e.what());
    return e.code == UVIO_HP_E_DEVICE ? 0 : 5;
  }
}
