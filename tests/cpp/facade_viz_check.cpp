// Compile-and-run check of the image-product part of include/uvio_hp.hpp on a host without a GPU: the facade
// methods are instantiated, uvio_hp_debug_draw_tracks / uvio_hp_debug_loop_depth refuse bad arguments with
// UVIO_HP_E_ARG before any device call, a size query needs no device, a valid draw fails loudly with
// UVIO_HP_E_DEVICE, the 16-bit depth map (host work) is right without a device, and Manager construction throws
// UVIO_HP_E_DEVICE.
#include <cstdio>

#include "uvio_hp.hpp"

#define EXPECT(cond, code)                       \
  if (!(cond)) {                                 \
    std::printf("failed: %s\n", #cond);          \
    return code;                                 \
  }

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  auto f1 = &uvio_amd::Manager::get_historical_viz_image;
  auto f2 = &uvio_amd::Manager::get_historical_viz_image_device;
  auto f3 = &uvio_amd::Manager::track_history;
  auto f4 = &uvio_amd::Manager::loop_depth;
  (void)f1, (void)f2, (void)f3, (void)f4;

  std::vector<uint8_t> img(40 * 31, 7), out(3 * 31 * 31);
  const uint8_t *imgs[1] = {img.data()};
  int w[1] = {31}, h[1] = {31}, stride[1] = {40}, counts[1] = {1};
  uvio_hp_viz_track_t tr{};
  tr.id = 1, tr.u = 10, tr.v = 10, tr.n_cams = 1, tr.hist_off = 0, tr.hist_n = 2;
  const float uv[4] = {5, 5, 10, 10};
  int cw = 0, ch = 0;
  auto draw = [&](int ncam, const uint8_t *const *im, const int *st, int n_uv, uint8_t *o) {
    return uvio_hp_debug_draw_tracks(ncam, im, w, h, st, nullptr, counts, &tr, uv, n_uv, o, out.size(), &cw, &ch, nullptr);
  };
  EXPECT(draw(0, imgs, stride, 2, out.data()) == UVIO_HP_E_ARG, 10);
  EXPECT(draw(UVIO_HP_MAX_CAMS + 1, imgs, stride, 2, out.data()) == UVIO_HP_E_ARG, 11);
  EXPECT(draw(1, nullptr, stride, 2, out.data()) == UVIO_HP_E_ARG, 12);
  const uint8_t *none[1] = {nullptr};
  EXPECT(draw(1, none, stride, 2, out.data()) == UVIO_HP_E_ARG, 13);
  int narrow[1] = {30};
  EXPECT(draw(1, imgs, narrow, 2, out.data()) == UVIO_HP_E_ARG, 14);
  EXPECT(draw(1, imgs, stride, 1, out.data()) == UVIO_HP_E_ARG, 15);  // the history runs past uv
  EXPECT(draw(1, imgs, stride, 2, nullptr) == UVIO_HP_OK && cw == 31 && ch == 31, 16);  // size query
  EXPECT(draw(1, imgs, stride, 2, out.data()) == UVIO_HP_E_DEVICE, 17);
  std::printf("draw args ok\n");

  // the 16-bit map is host work: (u, v) = (4, 27) sits on two border limits, (3.9, 10) fails the test
  const uint64_t ids[2] = {9, 4};
  const double uvd[6] = {4.0, 27.0, 1.5, 3.9, 10.0, 2.0};
  std::vector<uint16_t> depth(31 * 31, 1);
  EXPECT(uvio_hp_debug_loop_depth(img.data(), 31, 31, 40, 2, ids, uvd, depth.data(), nullptr) == UVIO_HP_OK, 20);
  for (int i = 0; i < 31 * 31; i++) EXPECT(depth[(size_t)i] == (i == 27 * 31 + 4 ? 1500 : 0), 21);
  EXPECT(uvio_hp_debug_loop_depth(img.data(), 31, 31, 30, 2, ids, uvd, depth.data(), nullptr) == UVIO_HP_E_ARG, 22);
  EXPECT(uvio_hp_debug_loop_depth(img.data(), 31, 31, 40, 2, ids, uvd, nullptr, out.data()) == UVIO_HP_E_DEVICE, 23);
  std::printf("depth ok\n");

  try {
    std::vector<uvio_amd::DrawCamera> cams(1);
    cams[0].image.data = img.data();
    cams[0].image.stride = 40;
    cams[0].width = cams[0].height = 31;
    cams[0].tracks.push_back(tr);
    (void)uvio_amd::draw_tracks(cams, std::vector<float>(uv, uv + 4), &cw, &ch);
    return 30;
  } catch (const uvio_amd::Error &e) {
    EXPECT(e.code == UVIO_HP_E_DEVICE, 31);
  }
  try {
    uvio_amd::Manager m(argv[1], 0);
    std::printf("created %d\n", (int)m.get_historical_viz_image().empty());
    return 4;
  } catch (const uvio_amd::Error &e) {
    std::printf("code %d: %s\n", e.code, e.what());
    return e.code == UVIO_HP_E_DEVICE ? 0 : 5;
  }
}
