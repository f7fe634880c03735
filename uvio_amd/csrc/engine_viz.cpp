// Engine: the image products a ROS node publishes besides the state ("Image products"):
// VioManager::get_historical_viz_image (VioManagerHelper.cpp:389-415, TrackBase::display_history,
// TrackBase.cpp:119-228) and the two depth images of ROS1Visualizer::publish_loopclosure_information
// (ROS1Visualizer.cpp:950-996), drawn on the device over level 0 of the tracker's last pyramids.
//
// The host walks the last tracks and the feature database once and writes the reference's primitives, in the
// reference's order, into one table (build_tracks / build_depth); the kernels of kernels_viz.hip draw them all at once
// and resolve the order per pixel.  The table goes up in one copy from a pinned buffer of the renderer's own: the
// update staging ring is sized for one update batch (a cfg3 table is several times that) and a getter must not move
// the ring under the feeds.  Nothing is allocated, copied or recorded by a feed for any of this.
#include <cmath>
#include <cstring>
#include <numeric>

#include "engine.h"

namespace uvhp {

namespace {

constexpr int kVizSat = 1 << 20;  // rounded coordinates saturate here (cvRound's result is undefined beyond int)
constexpr int kVizMaxSide = 16384;

// cvRound: round half to even; NaN and anything beyond +-2^20 saturate
int viz_round(float v) {
  if (!(v == v)) return -kVizSat;
  const double r = std::nearbyint((double)v);
  return r < -kVizSat ? -kVizSat : r > kVizSat ? kVizSat : (int)r;
}

unsigned viz_colour(int c0, int c1, int c2) {
  auto sat = [](int c) { return (unsigned)std::min(255, std::max(0, c)); };
  return sat(c0) | sat(c1) << 8 | sat(c2) << 16;
}

struct PrimWriter {
  std::vector<DVizPrim> &prims;
  long long npix = 0;
  void put(int kind, int cam, int x0, int y0, int x1, int y1, unsigned colour, int i0, long long count) {
    if (count <= 0) return;
    DVizPrim p;
    p.first = (int)std::min<long long>(npix, INT32_MAX);
    p.kind_cam = kind | cam << 8;
    p.x0 = x0, p.y0 = y0, p.x1 = x1, p.y1 = y1;
    p.colour = colour;
    p.i0 = i0;
    prims.push_back(p);
    npix += count;
  }
  void disc(int cam, bool small, int x, int y, unsigned colour) {
    const int kind = small ? VIZ_DISC1 : VIZ_DISC2;
    put(kind, cam, x, y, x, y, colour, 0, kVizDiscPixels[kind]);
  }
  // only the steps whose major coordinate lies inside the camera's image become pixels
  void segment(int cam, int w, int h, int x0, int y0, int x1, int y1, unsigned colour) {
    const int dx = x1 - x0, dy = y1 - y0, ax = std::abs(dx), ay = std::abs(dy), n = std::max(ax, ay);
    const bool xmajor = ax >= ay;
    const int a0 = xmajor ? x0 : y0, d = xmajor ? dx : dy, lim = xmajor ? w : h;
    int lo = 0, hi = n;
    if (d > 0) {
      lo = std::max(0, -a0), hi = std::min(n, lim - 1 - a0);
    } else if (d < 0) {
      lo = std::max(0, a0 - (lim - 1)), hi = std::min(n, a0);
    } else if (a0 < 0 || a0 >= lim) {
      return;
    }
    put(VIZ_SEG, cam, x0, y0, x1, y1, colour, lo, (long long)hi - lo + 1);
  }
  void rect(int cam, int x0, int y0, int x1, int y1, unsigned colour) {
    put(VIZ_RECT, cam, x0, y0, x1, y1, colour, 0, 2ll * (x1 - x0 + 1) + 2ll * (y1 - y0 + 1));
  }
  void fill(int cam, int x0, int y0, int x1, int y1, unsigned colour) {
    put(VIZ_FILL, cam, x0, y0, x1, y1, colour, 0, (long long)(x1 - x0 + 1) * (y1 - y0 + 1));
  }
};

}  // namespace

void VizRenderer::cell(int ncam, const VizCamIn *cams, int *cw, int *ch) {
  *cw = *ch = 0;
  for (int k = 0; k < ncam; k++) *cw = std::max(*cw, cams[k].w), *ch = std::max(*ch, cams[k].h);
}

// TrackBase::display_history's drawing loop (TrackBase.cpp:164-211) with r1 g1 b1 = 255 255 0, r2 g2 b2 = 255 255 255
long long VizRenderer::build_tracks(int ncam, const VizCamIn *cams, const int *counts, const uvio_hp_viz_track_t *tracks,
                                    const float *uv, std::vector<DVizPrim> &prims) {
  int cw, ch;
  cell(ncam, cams, &cw, &ch);
  const bool small = std::min(cw, ch) < 400;
  const int half = small ? 3 : 5;
  const size_t maxtracks = 50;
  prims.clear();
  PrimWriter out{prims};
  const uvio_hp_viz_track_t *tr = tracks;
  for (int c = 0; c < ncam; c++) {
    const int w = cams[c].w, h = cams[c].h;
    for (int i = 0; i < counts[c]; i++, tr++) {
      if (tr->highlighted) {
        const unsigned green = viz_colour(0, 255, 0);
        out.rect(c, viz_round(tr->u - (float)half), viz_round(tr->v - (float)half), viz_round(tr->u + (float)half),
                 viz_round(tr->v + (float)half), green);
        out.disc(c, small, viz_round(tr->u), viz_round(tr->v), green);
      }
      if (tr->hist_n <= 0 || tr->to_delete) continue;
      const size_t size = (size_t)tr->hist_n;
      const float *p = uv + 2 * (size_t)tr->hist_off;
      const bool is_stereo = tr->n_cams > 1;
      for (size_t z = size - 1; z > 0; z--) {
        if (size - z > maxtracks) break;
        const int fade = 255 - (int)(1.0 * 255 / size * z), keep = 255 - (int)(1.0 * 0 / size * z);
        const unsigned col = is_stereo ? viz_colour(keep, fade, fade) : viz_colour(fade, fade, keep);
        const int x = viz_round(p[2 * z]), y = viz_round(p[2 * z + 1]);
        out.disc(c, small, x, y, col);
        if (z + 1 < size) out.segment(c, w, h, x, y, viz_round(p[2 * z + 2]), viz_round(p[2 * z + 3]), col);
      }
    }
  }
  return out.npix > INT32_MAX ? -1 : out.npix;
}

// ROS1Visualizer.cpp:957-996 over the tracks in ascending feature id
long long VizRenderer::build_depth(int w, int h, int n, const uint64_t *ids, const double *uvd,
                                   std::vector<DVizPrim> &prims, uint16_t *depth) {
  prims.clear();
  PrimWriter out{prims};
  if (depth) std::memset(depth, 0, sizeof(uint16_t) * (size_t)w * h);
  std::vector<int> order((size_t)n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ids[a] < ids[b]; });
  const double dw = 4;
  for (int k : order) {
    const double u = uvd[3 * k], v = uvd[3 * k + 1], d = uvd[3 * k + 2];
    // (written so that a NaN is skipped, where the reference's test would let it through to an undefined cast)
    if (!(u >= dw && u <= w - dw && v >= dw && v <= h - dw)) continue;
    if (depth) {
      const double m = 1000 * d;
      const long long q = (m == m && std::fabs(m) < 9.0e18) ? (long long)m : 0;
      depth[(size_t)(int)v * w + (int)u] = (uint16_t)q;
    }
    const float id = 1.0f / (float)d;
    float r = (0.0f - id) * 255 / 1.0f, g = (1.0f - id) * 255 / 1.0f, b = (2.0f - id) * 255 / 1.0f;
    if (r < 0) r = -r;
    if (g < 0) g = -g;
    if (b < 0) b = -b;
    auto uc = [](float x) { return !(x == x) ? 0 : x < 0 ? 0 : (x > 255 ? 255 : (int)(unsigned char)x); };
    out.fill(0, (int)(u - dw), (int)(v - dw), (int)(u + dw), (int)(v + dw),
             viz_colour(255 - uc(r), 255 - uc(g), 255 - uc(b)));
  }
  return out.npix > INT32_MAX ? -1 : out.npix;
}

void VizRenderer::render(hipStream_t s, int ncam, const VizCamIn *cams, const std::vector<DVizPrim> &prims,
                         long long npix, uint8_t *out_host, uint8_t *out_dev) {
  VizJob job{};
  cell(ncam, cams, &job.cw, &job.ch);
  job.ncam = ncam;
  const size_t npx = (size_t)ncam * job.cw * job.ch;
  if (npx == 0) return;
  // (an old block is freed before its replacement is made; the last call has completed)
  if (plane_.size() < npx) {
    plane_.reset();
    plane_ = DevBuf<unsigned long long>(npx);
  }
  if (!out_dev && canvas_.size() < 3 * npx) {
    canvas_.reset();
    canvas_ = DevBuf<uint8_t>(3 * npx);
  }
  if (out_host && h_out_.size() < 3 * npx) {
    h_out_.reset();
    h_out_ = PinBuf<uint8_t>(3 * npx);
  }
  if (d_prims_.size() < prims.size()) {
    const size_t cap = prims.size() + prims.size() / 2;
    d_prims_.reset();
    h_prims_.reset();
    d_prims_ = DevBuf<DVizPrim>(cap);
    h_prims_ = PinBuf<DVizPrim>(cap);
  }
  size_t mask_bytes = 0;
  for (int k = 0; k < ncam; k++)
    if (cams[k].mask) mask_bytes += (size_t)cams[k].w * cams[k].h;
  if (d_mask_.size() < mask_bytes) {
    d_mask_.reset();
    h_mask_.reset();
    d_mask_ = DevBuf<uint8_t>(mask_bytes);
    h_mask_ = PinBuf<uint8_t>(mask_bytes);
  }
  if (timing)
    for (auto &e : ev_)
      if (!e) e = TimedEvent::create();
  auto mark = [&](int k) {
    if (timing) HP_HIP(hipEventRecord(ev_[k], s));
  };
  job.canvas = out_dev ? out_dev : canvas_.get();
  job.plane = plane_;
  job.prims = d_prims_;
  job.nprim = (int)prims.size();
  job.npix = (int)npix;
  // the host packing (table and mask rows into the pinned mirrors) comes first: the "uploads" stage, from event 0
  // on, then holds the two transfers only
  if (!prims.empty()) std::memcpy(h_prims_, prims.data(), sizeof(DVizPrim) * prims.size());
  size_t off = 0;
  for (int k = 0; k < ncam; k++) {
    job.img[k] = cams[k].img;
    job.w[k] = cams[k].w, job.h[k] = cams[k].h, job.stride[k] = cams[k].stride;
    job.mask[k] = nullptr;
    if (!cams[k].mask) continue;
    for (int y = 0; y < cams[k].h; y++)
      std::memcpy(h_mask_ + off + (size_t)y * cams[k].w, cams[k].mask + (size_t)y * cams[k].mask_stride, cams[k].w);
    job.mask[k] = d_mask_ + off;
    off += (size_t)cams[k].w * cams[k].h;
  }
  mark(0);
  if (!prims.empty())
    HP_HIP(hipMemcpyAsync(d_prims_, h_prims_, sizeof(DVizPrim) * prims.size(), hipMemcpyHostToDevice, s));
  if (mask_bytes) HP_HIP(hipMemcpyAsync(d_mask_, h_mask_, mask_bytes, hipMemcpyHostToDevice, s));
  mark(1);
  launch_viz_base(s, job);
  mark(2);
  launch_viz_prims(s, job);
  mark(3);
  launch_viz_compose(s, job);
  HP_HIP(hipGetLastError());
  mark(4);
  if (out_host) HP_HIP(hipMemcpyAsync(h_out_, job.canvas, 3 * npx, hipMemcpyDeviceToHost, s));
  mark(5);
  spin_sync(s);
  if (out_host) std::memcpy(out_host, h_out_, 3 * npx);
  if (timing)
    for (int k = 0; k < 5; k++) {
      float t = 0;
      HP_HIP(hipEventElapsedTime(&t, ev_[k], ev_[k + 1]));
      ms[k] = t;
    }
}

int Engine::track_image_times(int on, double *ms) {
  if (!viz_) viz_.reset(new VizRenderer());
  if (ms) std::memcpy(ms, viz_->ms, sizeof(viz_->ms));
  viz_->timing = on != 0;
  return 0;
}

int Engine::track_history(int cam, uint64_t id, float *uv, int cap, int *n, int *n_cams, int *to_delete) const {
  *n = 0;
  if (n_cams) *n_cams = 0;
  if (to_delete) *to_delete = 0;
  auto it = db_.find((size_t)id);
  if (it == db_.end()) return 0;
  const Feature &f = *it->second;
  if (n_cams) *n_cams = (int)f.tracks.size();
  if (to_delete) *to_delete = f.to_delete ? 1 : 0;
  const CamTrack *ct = cam >= 0 ? f.find((size_t)cam) : nullptr;
  if (!ct) return 0;
  *n = (int)ct->m.size();
  for (int i = 0; i < *n && i < cap && uv; i++) uv[2 * i] = ct->m[(size_t)i].u, uv[2 * i + 1] = ct->m[(size_t)i].v;
  return *n <= cap ? 0 : UVIO_HP_E_CAPACITY;
}

int Engine::track_image(uint8_t *out, size_t cap, int *width, int *height, int *overlay, bool device_out) {
  stage_ = "get_historical_viz_image";
  // VioManagerHelper.cpp:402-403
  if (overlay) *overlay = !is_initialized_ ? 1 : (did_zupt_update_ ? 2 : 0);
  *width = *height = 0;
  Tracker::VizCam vc[kMaxCams];
  const int nc = tracker_ ? tracker_->viz_cams(vc) : 0;
  if (nc == 0) return 0;
  VizCamIn cams[kMaxCams];
  for (int k = 0; k < nc; k++)
    cams[k] = VizCamIn{vc[k].img, vc[k].w, vc[k].h, vc[k].w, vc[k].mask->empty() ? nullptr : vc[k].mask->data(), vc[k].w};
  int cw, ch;
  VizRenderer::cell(nc, cams, &cw, &ch);
  *width = nc * cw;
  *height = ch;
  if (!out) return 0;
  if (cap < (size_t)3 * *width * *height) return UVIO_HP_E_CAPACITY;
  // what display_history reads: ids_last / pts_last, the highlighted ids (the state's SLAM landmarks) and a
  // clone of each feature (its uvs of this camera, how many cameras hold it, to_delete)
  int counts[kMaxCams];
  std::vector<uvio_hp_viz_track_t> tracks;
  std::vector<float> uv;
  for (int k = 0; k < nc; k++) {
    counts[k] = (int)vc[k].ids->size();
    for (size_t i = 0; i < vc[k].ids->size(); i++) {
      uvio_hp_viz_track_t t{};
      t.id = (*vc[k].ids)[i];
      t.u = (*vc[k].pts)[i].x;
      t.v = (*vc[k].pts)[i].y;
      t.highlighted = slam_.count((size_t)t.id) ? 1 : 0;
      t.hist_off = (int)(uv.size() / 2);
      auto it = db_.find((size_t)t.id);
      if (it != db_.end()) {
        const Feature &f = *it->second;
        t.n_cams = (int)f.tracks.size();
        t.to_delete = f.to_delete ? 1 : 0;
        if (const CamTrack *ct = f.find((size_t)vc[k].cam)) {
          t.hist_n = (int)ct->m.size();
          for (const FeatMeas &m : ct->m) uv.push_back(m.u), uv.push_back(m.v);
        }
      }
      tracks.push_back(t);
    }
  }
  std::vector<DVizPrim> prims;
  const long long npix = VizRenderer::build_tracks(nc, cams, counts, tracks.data(), uv.data(), prims);
  if (npix < 0) throw HpError(UVIO_HP_E_CAPACITY, "track image: more than 2^31 - 1 primitive pixels");
  if (!viz_) viz_.reset(new VizRenderer());
  viz_->render(d_.stream, nc, cams, prims, npix, device_out ? nullptr : out, device_out ? out : nullptr);
  return 0;
}

int Engine::loop_depth(uint16_t *depth, uint8_t *viz, size_t cap, int *width, int *height, double *t) {
  stage_ = "publish_loopclosure_information";
  *width = *height = 0;
  double tt = -1;
  int n = get_active_tracks(&tt, nullptr, nullptr, nullptr, nullptr, 0);
  if (t) *t = tt;
  if (tt == -1) return 0;  // ROS1Visualizer.cpp:850
  Tracker::VizCam vc[kMaxCams];
  const int nc = tracker_ ? tracker_->viz_cams(vc) : 0;
  const Tracker::VizCam *c0 = nullptr;
  for (int k = 0; k < nc; k++)
    if (vc[k].cam == 0) c0 = &vc[k];
  if (!c0) return 0;  // no camera-0 image (the reference's active_image is empty)
  *width = c0->w;
  *height = c0->h;
  if (!depth && !viz) return 0;
  if (cap < (size_t)c0->w * c0->h) return UVIO_HP_E_CAPACITY;
  std::vector<uint64_t> ids((size_t)n);
  std::vector<double> pos(3 * (size_t)n), uvd(3 * (size_t)n);
  std::vector<int> ok((size_t)n);
  if (n > 0) n = std::min(n, get_active_tracks(&tt, ids.data(), pos.data(), uvd.data(), ok.data(), n));
  // active_tracks_uvd holds only the tracks with a camera-0 projection
  int m = 0;
  for (int i = 0; i < n; i++)
    if (ok[(size_t)i]) {
      ids[(size_t)m] = ids[(size_t)i];
      for (int j = 0; j < 3; j++) uvd[3 * (size_t)m + j] = uvd[3 * (size_t)i + j];
      m++;
    }
  std::vector<DVizPrim> prims;
  const long long npix = VizRenderer::build_depth(c0->w, c0->h, m, ids.data(), uvd.data(), prims, depth);
  if (!viz) return 0;
  if (npix < 0) throw HpError(UVIO_HP_E_CAPACITY, "loop depth: more than 2^31 - 1 primitive pixels");
  const VizCamIn cam{c0->img, c0->w, c0->h, c0->w, nullptr, 0};
  if (!viz_) viz_.reset(new VizRenderer());
  viz_->render(d_.stream, 1, &cam, prims, npix, viz, nullptr);
  return 0;
}

// ---- the same paths on caller-given inputs ----
static bool have_device() {
  int ndev = 0;
  return hipGetDeviceCount(&ndev) == hipSuccess && ndev >= 1;
}

int Engine::draw_tracks_standalone(int ncam, const uint8_t *const *imgs, const int *w, const int *h, const int *strides,
                                   const uint8_t *const *masks, const int *counts, const uvio_hp_viz_track_t *tracks,
                                   const float *uv, int n_uv, uint8_t *out, size_t cap, int *width, int *height,
                                   double *stage_ms) {
  if (ncam < 1 || ncam > UVIO_HP_MAX_CAMS || !imgs || !w || !h || !strides || !counts || !width || !height || n_uv < 0)
    return UVIO_HP_E_ARG;
  long long ntr = 0;
  for (int k = 0; k < ncam; k++) {
    if (!imgs[k] || w[k] < 1 || h[k] < 1 || strides[k] < w[k] || counts[k] < 0) return UVIO_HP_E_ARG;
    ntr += counts[k];
  }
  if (ntr > 0 && !tracks) return UVIO_HP_E_ARG;
  for (long long i = 0; i < ntr; i++) {
    const uvio_hp_viz_track_t &t = tracks[i];
    if (t.hist_n < 0 || t.hist_off < 0 || (long long)t.hist_off + t.hist_n > n_uv || (t.hist_n > 0 && !uv))
      return UVIO_HP_E_ARG;
  }
  VizCamIn cams[kMaxCams];
  for (int k = 0; k < ncam; k++) {
    if (w[k] > kVizMaxSide || h[k] > kVizMaxSide) return UVIO_HP_E_CAPACITY;
    cams[k] = VizCamIn{nullptr, w[k], h[k], w[k], masks ? masks[k] : nullptr, strides[k]};
  }
  int cw, ch;
  VizRenderer::cell(ncam, cams, &cw, &ch);
  *width = ncam * cw;
  *height = ch;
  if (!out) return 0;
  if (cap < (size_t)3 * *width * *height) return UVIO_HP_E_CAPACITY;
  std::vector<DVizPrim> prims;
  const long long npix = VizRenderer::build_tracks(ncam, cams, counts, tracks, uv, prims);
  if (npix < 0) return UVIO_HP_E_CAPACITY;
  if (!have_device()) return UVIO_HP_E_DEVICE;
  Stream s = Stream::create();
  DevBuf<uint8_t> d_img[kMaxCams];
  for (int k = 0; k < ncam; k++) {
    d_img[k] = DevBuf<uint8_t>((size_t)w[k] * h[k]);
    HP_HIP(hipMemcpy2DAsync(d_img[k], w[k], imgs[k], strides[k], w[k], h[k], hipMemcpyHostToDevice, s));
    cams[k].img = d_img[k];
  }
  VizRenderer r;
  r.timing = stage_ms != nullptr;
  r.render(s, ncam, cams, prims, npix, out, nullptr);  // (waits for s: nothing in flight when the buffers go)
  if (stage_ms) std::memcpy(stage_ms, r.ms, sizeof(r.ms));
  return 0;
}

int Engine::loop_depth_standalone(const uint8_t *img, int w, int h, int stride, int n, const uint64_t *ids,
                                  const double *uvd, uint16_t *depth, uint8_t *viz) {
  if (!img || w < 1 || h < 1 || stride < w || n < 0 || (n > 0 && (!ids || !uvd))) return UVIO_HP_E_ARG;
  if (w > kVizMaxSide || h > kVizMaxSide) return UVIO_HP_E_CAPACITY;
  std::vector<DVizPrim> prims;
  const long long npix = VizRenderer::build_depth(w, h, n, ids, uvd, prims, depth);
  if (!viz) return 0;
  if (npix < 0) return UVIO_HP_E_CAPACITY;
  if (!have_device()) return UVIO_HP_E_DEVICE;
  Stream s = Stream::create();
  DevBuf<uint8_t> d_img((size_t)w * h);
  HP_HIP(hipMemcpy2DAsync(d_img, w, img, stride, w, h, hipMemcpyHostToDevice, s));
  const VizCamIn cam{d_img, w, h, w, nullptr, 0};
  VizRenderer r;
  r.render(s, 1, &cam, prims, npix, viz, nullptr);
  return 0;
}

}  // namespace uvhp
