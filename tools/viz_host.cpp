// The host alternative to uvio_hp_get_track_image ("Image products"): TrackBase::display_history
// drawn on the CPU, a sequential painter's loop over the rules of that section, on the inputs of
// uvio_hp_debug_draw_tracks (images already on the host, i.e. after uvio_hp_get_pyramid).  The yardstick of
// tools/viz_times.py, which loads it as a shared library, checks its canvas against the device's and times it:
//   g++ -O2 -std=c++17 -shared -fPIC -I include tools/viz_host.cpp -o build/libviz_host.so
// Stand-alone (synthetic tracks on two 512 x 512 cameras, median of 100 draws):
//   g++ -O2 -std=c++17 -DVIZ_HOST_MAIN -I include tools/viz_host.cpp -o build/viz_host && build/viz_host
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "uvio_hp.h"

namespace {

constexpr int kSat = 1 << 20;

int cv_round(float v) {
  if (!(v == v)) return -kSat;
  const double r = std::nearbyint((double)v);
  return r < -kSat ? -kSat : r > kSat ? kSat : (int)r;
}

struct View {  // one camera's w x h window of the canvas
  uint8_t *base;
  size_t row;  // canvas row bytes
  int w, h;
  void put(int x, int y, const uint8_t c[3]) const {
    if (x < 0 || y < 0 || x >= w || y >= h) return;
    uint8_t *p = base + (size_t)y * row + 3 * (size_t)x;
    p[0] = c[0], p[1] = c[1], p[2] = c[2];
  }
  void disc(int cx, int cy, int r, const uint8_t c[3]) const {
    for (int dy = -r; dy <= r; dy++) {
      const int half = r == 1 ? (dy == 0 ? 1 : 0) : (std::abs(dy) == 2 ? 1 : 2);
      for (int dx = -half; dx <= half; dx++) put(cx + dx, cy + dy, c);
    }
  }
  void segment(int x0, int y0, int x1, int y1, const uint8_t c[3]) const {
    const int dx = x1 - x0, dy = y1 - y0, ax = std::abs(dx), ay = std::abs(dy), n = std::max(ax, ay);
    const int sx = (dx > 0) - (dx < 0), sy = (dy > 0) - (dy < 0);
    if (n == 0) return put(x0, y0, c);
    // (steps outside the image on the major axis paint nothing: skipped, as any host renderer would)
    const bool xm = ax >= ay;
    const int a0 = xm ? x0 : y0, s = xm ? sx : sy, lim = xm ? w : h;
    const long long lo = s > 0 ? std::max(0, -a0) : std::max(0, a0 - (lim - 1));
    const long long hi = s > 0 ? std::min(n, lim - 1 - a0) : std::min(n, a0);
    for (long long i = lo; i <= hi; i++) {
      if (xm)
        put(x0 + sx * (int)i, y0 + sy * (int)((2 * i * ay + n) / (2ll * n)), c);
      else
        put(x0 + sx * (int)((2 * i * ax + n) / (2ll * n)), y0 + sy * (int)i, c);
    }
  }
  void rectangle(int x0, int y0, int x1, int y1, const uint8_t c[3]) const {
    for (int x = x0; x <= x1; x++) put(x, y0, c), put(x, y1, c);
    for (int y = y0; y <= y1; y++) put(x0, y, c), put(x1, y, c);
  }
};

}  // namespace

// out: 3 * max_h * ncam * max_w bytes.  Arguments as uvio_hp_debug_draw_tracks; returns 0
extern "C" int viz_host_draw(int ncam, const uint8_t *const *imgs, const int *w, const int *h, const int *strides,
                             const uint8_t *const *masks, const int *counts, const uvio_hp_viz_track_t *tracks,
                             const float *uv, uint8_t *out) {
  int cw = 0, ch = 0;
  for (int k = 0; k < ncam; k++) cw = std::max(cw, w[k]), ch = std::max(ch, h[k]);
  const size_t row = 3 * (size_t)ncam * cw;
  std::memset(out, 0, row * ch);
  const bool small = std::min(cw, ch) < 400;
  const int r = small ? 1 : 2;
  const float half = small ? 3.f : 5.f;
  const uvio_hp_viz_track_t *t = tracks;
  for (int k = 0; k < ncam; k++) {
    const View v{out + 3 * (size_t)k * cw, row, w[k], h[k]};
    for (int y = 0; y < h[k]; y++) {
      const uint8_t *src = imgs[k] + (size_t)y * strides[k];
      uint8_t *dst = v.base + (size_t)y * row;
      for (int x = 0; x < w[k]; x++) dst[3 * x] = dst[3 * x + 1] = dst[3 * x + 2] = src[x];
    }
    for (int i = 0; i < counts[k]; i++, t++) {
      if (t->highlighted) {
        const uint8_t green[3] = {0, 255, 0};
        v.rectangle(cv_round(t->u - half), cv_round(t->v - half), cv_round(t->u + half), cv_round(t->v + half), green);
        v.disc(cv_round(t->u), cv_round(t->v), r, green);
      }
      if (t->hist_n <= 0 || t->to_delete) continue;
      const size_t size = (size_t)t->hist_n;
      const float *p = uv + 2 * (size_t)t->hist_off;
      const bool stereo = t->n_cams > 1;
      for (size_t z = size - 1; z > 0; z--) {
        if (size - z > 50) break;
        const int fade = std::min(255, std::max(0, 255 - (int)(1.0 * 255 / size * z)));
        const uint8_t f = (uint8_t)fade;
        const uint8_t mono[3] = {f, f, 255}, ster[3] = {255, f, f};
        const uint8_t *c = stereo ? ster : mono;
        const int x = cv_round(p[2 * z]), y = cv_round(p[2 * z + 1]);
        v.disc(x, y, r, c);
        if (z + 1 < size) v.segment(x, y, cv_round(p[2 * z + 2]), cv_round(p[2 * z + 3]), c);
      }
    }
    if (masks && masks[k])
      for (int y = 0; y < h[k]; y++) {
        const uint8_t *m = masks[k] + (size_t)y * strides[k];
        uint8_t *dst = v.base + (size_t)y * row;
        for (int x = 0; x < w[k]; x++)
          if (m[x] > 127) {
            const int q = dst[3 * x + 2];
            dst[3 * x + 2] = (uint8_t)std::min(255, q + 25 + ((q & 1) ? 0 : 1));
          }
      }
  }
  return 0;
}

#ifdef VIZ_HOST_MAIN
int main() {
  const int ncam = 2, W = 512, H = 512, ntr = 400, steps = 51;
  std::srand(3);
  auto rnd = []() { return std::rand() / (double)RAND_MAX; };
  std::vector<std::vector<uint8_t>> img(ncam, std::vector<uint8_t>((size_t)W * H));
  std::vector<uvio_hp_viz_track_t> tracks;
  std::vector<float> uv;
  for (int k = 0; k < ncam; k++) {
    for (auto &b : img[k]) b = (uint8_t)(std::rand() & 255);
    for (int i = 0; i < ntr; i++) {
      uvio_hp_viz_track_t t{};
      t.id = (uint64_t)i, t.highlighted = i % 10 == 0, t.n_cams = ncam, t.hist_off = (int)(uv.size() / 2), t.hist_n = steps;
      double x = 20 + rnd() * (W - 40), y = 20 + rnd() * (H - 40);
      for (int s = 0; s < steps; s++) {
        uv.push_back((float)x), uv.push_back((float)y);
        x += 6 * (rnd() - 0.5), y += 6 * (rnd() - 0.5);
      }
      t.u = uv[uv.size() - 2], t.v = uv[uv.size() - 1];
      tracks.push_back(t);
    }
  }
  const uint8_t *imgs[2] = {img[0].data(), img[1].data()};
  const int w[2] = {W, W}, h[2] = {H, H}, st[2] = {W, W}, counts[2] = {ntr, ntr};
  std::vector<uint8_t> out((size_t)3 * ncam * W * H);
  std::vector<double> ms;
  for (int it = 0; it < 110; it++) {
    const auto t0 = std::chrono::steady_clock::now();
    viz_host_draw(ncam, imgs, w, h, st, nullptr, counts, tracks.data(), uv.data(), out.data());
    const double d = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (it >= 10) ms.push_back(d);
  }
  std::sort(ms.begin(), ms.end());
  std::printf("host draw, 2 x 512 x 512, 400 tracks x 50 steps per camera: median %.3f ms (min %.3f max %.3f)\n",
              ms[ms.size() / 2], ms.front(), ms.back());
  return 0;
}
#endif
