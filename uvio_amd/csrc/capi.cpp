// extern "C" boundary of libuvio_hp.so (declared in include/uvio_hp.h).  Every entry converts
// exceptions into status codes: the library never exits the process.
#include <cstring>
#include <string>

#include "engine.h"

using namespace uvhp;

struct uvio_hp {
  Engine *e = nullptr;
  std::string err;
  // set by a fatal error of a state-changing call (the reference std::exit's on these: negative covariance
  // diagonal, StateHelper.cpp:112,181; a device or internal error likewise leaves the frame half applied, e.g.
  // measurements already trimmed from the feature database): every later state-changing call is refused
  std::string fatal;
};

// an exception that is not an HpError is a host-side logic error (e.g. std::out_of_range from a map
// lookup): reported as UVIO_HP_E_INTERNAL with the reference routine the engine was in
static std::string internal_error(const uvio_hp *h, const std::exception &ex) {
  std::string m = std::string("internal error: ") + ex.what();
  if (h && h->e && h->e->stage()[0]) m += std::string(" (in ") + h->e->stage() + ")";
  return m;
}

#define HP_GUARD(h, body)                                    \
  try {                                                      \
    if ((h) && (h)->e) HP_HIP(hipSetDevice((h)->e->device())); \
    body                                                     \
  } catch (const HpError &ex) {                              \
    if (h) (h)->err = ex.what();                             \
    return ex.code;                                          \
  } catch (const std::exception &ex) {                       \
    if (h) (h)->err = internal_error(h, ex);                 \
    return UVIO_HP_E_INTERNAL;                               \
  }

// a state-changing entry: refused after a fatal error; a fatal result stops the estimator
static bool is_fatal(int rc) { return rc == UVIO_HP_E_NUMERIC || rc == UVIO_HP_E_DEVICE || rc == UVIO_HP_E_INTERNAL; }
#define HP_FEED(h, call)                                                                         \
  if (!(h)->fatal.empty()) {                                                                     \
    (h)->err = "estimator stopped by an earlier fatal error (" + (h)->fatal + ")";             \
    return UVIO_HP_E_STATE;                                                                      \
  }                                                                                              \
  {                                                                                              \
    const int rc_ = [&]() -> int { HP_GUARD(h, return (call);) }();                              \
    if (is_fatal(rc_)) (h)->fatal = (h)->err;                                                    \
    return rc_;                                                                                  \
  }

extern "C" {

int uvio_hp_options_default(uvio_hp_options_t *opts) {
  if (!opts) return UVIO_HP_E_ARG;
  options_default(opts);
  return 0;
}

int uvio_hp_options_load(const char *path, uvio_hp_options_t *opts) {
  if (!path || !opts) return UVIO_HP_E_ARG;
  std::string err;
  return options_load(path, opts, &err);
}

static thread_local std::string g_create_err = "";  // why the last uvio_hp_create on this thread failed

int uvio_hp_create(const uvio_hp_options_t *opts, int device, uvio_hp_t **out) {
  if (!opts || !out) return UVIO_HP_E_ARG;
  *out = nullptr;
  uvio_hp_t *h = new uvio_hp_t();
  try {
    h->e = new Engine(*opts, device);
  } catch (const HpError &ex) {
    int c = ex.code;
    g_create_err = ex.what();
    delete h;
    return c;
  } catch (const std::exception &ex) {
    g_create_err = ex.what();
    delete h;
    return UVIO_HP_E_DEVICE;
  }
  *out = h;
  return 0;
}

int uvio_hp_destroy(uvio_hp_t *h) {
  if (!h) return UVIO_HP_E_ARG;
  delete h->e;
  delete h;
  return 0;
}

const char *uvio_hp_last_error(const uvio_hp_t *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int uvio_hp_initialize_with_gt(uvio_hp_t *h, const double x[17]) {
  if (!h || !x) return UVIO_HP_E_ARG;
  HP_GUARD(h, h->e->initialize_with_gt(x); return 0;)
}

int uvio_hp_feed_imu(uvio_hp_t *h, double t, const double wm[3], const double am[3]) {
  if (!h || !wm || !am) return UVIO_HP_E_ARG;
  HP_GUARD(h, h->e->feed_imu(t, wm, am); return 0;)
}

int uvio_hp_feed_imu_batch(uvio_hp_t *h, int n, const double *t, const double *wm, const double *am) {
  if (!h || n < 0 || (n > 0 && (!t || !wm || !am))) return UVIO_HP_E_ARG;
  HP_GUARD(h, for (int i = 0; i < n; i++) h->e->feed_imu(t[i], wm + 3 * i, am + 3 * i); return 0;)
}

int uvio_hp_feed_simulation(uvio_hp_t *h, double t, int ncam, const int *cam_ids, const int *counts, const uint64_t *ids,
                            const float *uv) {
  if (!h || ncam <= 0 || !cam_ids || !counts) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->feed_simulation(t, ncam, cam_ids, counts, ids, uv))
}

int uvio_hp_feed_camera(uvio_hp_t *h, double t, int ncam, const int *cam_ids, const uint8_t *const *imgs,
                        const int *strides, const uint8_t *const *masks) {
  if (!h || ncam <= 0 || !cam_ids || !imgs || !strides) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->feed_camera(t, ncam, cam_ids, imgs, strides, masks, false))
}

int uvio_hp_feed_camera_device(uvio_hp_t *h, double t, int ncam, const int *cam_ids, const uint8_t *const *imgs,
                               const int *strides, const uint8_t *const *masks) {
  if (!h || ncam <= 0 || !cam_ids || !imgs || !strides) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->feed_camera(t, ncam, cam_ids, imgs, strides, masks, true))
}

int uvio_hp_get_tracks(uvio_hp_t *h, int cam, uint64_t *ids, float *uv, int cap, int *n) {
  if (!h || !n) return UVIO_HP_E_ARG;
  HP_GUARD(h, {
    std::vector<uvhp::KeyPt> pts;
    std::vector<size_t> id;
    if (h->e->tracker()) h->e->tracker()->last_tracks(cam, pts, id);
    *n = (int)pts.size();
    if ((int)pts.size() > cap) return UVIO_HP_E_CAPACITY;
    for (size_t i = 0; i < pts.size(); i++) {
      if (ids) ids[i] = (uint64_t)id[i];
      if (uv) {
        uv[2 * i] = pts[i].x;
        uv[2 * i + 1] = pts[i].y;
      }
    }
    return 0;
  })
}

int uvio_hp_get_pyramid(uvio_hp_t *h, int cam, int level, int *w, int *hgt, uint8_t *img, int16_t *der, size_t cap) {
  if (!h || !w || !hgt) return UVIO_HP_E_ARG;
  HP_GUARD(h, {
    std::vector<uint8_t> im;
    std::vector<int16_t> d;
    if (!h->e->tracker() || !h->e->tracker()->last_pyramid(cam, level, w, hgt, img ? &im : nullptr, der ? &d : nullptr))
      return UVIO_HP_E_STATE;
    size_t px = (size_t)*w * *hgt;
    if ((img || der) && px > cap) return UVIO_HP_E_CAPACITY;
    if (img) std::memcpy(img, im.data(), px);
    if (der) std::memcpy(der, d.data(), px * 2 * sizeof(int16_t));
    return 0;
  })
}

int uvio_hp_feed_uwb(uvio_hp_t *h, double t, int n, const uint64_t *ids, const double *ranges) {
  if (!h || n < 0) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->feed_uwb(t, n, ids, ranges))
}

int uvio_hp_init_anchors(uvio_hp_t *h, int n, const uvio_hp_anchor_t *a) {
  if (!h || n < 0) return UVIO_HP_E_ARG;
  HP_GUARD(h, return h->e->init_anchors(n, a);)
}

int uvio_hp_initialized(const uvio_hp_t *h, int *out) {
  if (!h || !out) return UVIO_HP_E_ARG;
  *out = h->e->initialized() ? 1 : 0;
  return 0;
}

int uvio_hp_get_imu_state(uvio_hp_t *h, double *t, double out[16]) {
  if (!h || !t || !out) return UVIO_HP_E_ARG;
  *t = h->e->timestamp();
  std::memcpy(out, h->e->imu().val, sizeof(double) * 16);
  return 0;
}

int uvio_hp_get_cov_dim(uvio_hp_t *h, int *n) {
  if (!h || !n) return UVIO_HP_E_ARG;
  *n = h->e->cov_dim();
  return 0;
}

int uvio_hp_get_cov(uvio_hp_t *h, double *out, int ld) {
  if (!h || !out || ld < h->e->cov_dim()) return UVIO_HP_E_ARG;
  HP_GUARD(h, h->e->get_cov(out, ld); return 0;)
}

int uvio_hp_get_state_vector(uvio_hp_t *h, double *out, int cap, int *len, int *meta, int meta_cap, int *nvars) {
  if (!h || !out || !len) return UVIO_HP_E_ARG;
  int k = h->e->state_vector(out, cap, meta, meta_cap, nvars);
  *len = k;
  return k <= cap ? 0 : UVIO_HP_E_CAPACITY;
}

int uvio_hp_get_fej_vector(uvio_hp_t *h, double *out, int cap, int *len) {
  if (!h || !out || !len) return UVIO_HP_E_ARG;
  int k = h->e->state_vector(out, cap, nullptr, 0, nullptr, true);
  *len = k;
  return k <= cap ? 0 : UVIO_HP_E_CAPACITY;
}

int uvio_hp_get_timing(uvio_hp_t *h, uvio_hp_timing_t *out) {
  if (!h || !out) return UVIO_HP_E_ARG;
  *out = h->e->timing();
  return 0;
}

int uvio_hp_get_active_tracks(uvio_hp_t *h, double *t, uint64_t *ids, double *posinG, double *uvd, int *uvd_valid,
                              int cap, int *n) {
  if (!h || !t || !n || (cap > 0 && (!ids || !posinG || !uvd || !uvd_valid))) return UVIO_HP_E_ARG;
  HP_GUARD(h, {
    *n = h->e->get_active_tracks(t, ids, posinG, uvd, uvd_valid, cap);
    return *n <= cap ? 0 : UVIO_HP_E_CAPACITY;
  })
}

int uvio_hp_get_features_slam(uvio_hp_t *h, uint64_t *ids, double *xyz_inG, int cap, int *n) {
  if (!h || !n || cap < 0 || (cap > 0 && (!ids || !xyz_inG))) return UVIO_HP_E_ARG;
  HP_GUARD(h, {
    *n = h->e->get_features_slam(ids, xyz_inG, cap);
    return *n <= cap ? 0 : UVIO_HP_E_CAPACITY;
  })
}

int uvio_hp_set_kernel_timing(uvio_hp_t *h, int on) {
  if (!h) return UVIO_HP_E_ARG;
  if (on < 0) return UVIO_HP_E_ARG;
  h->e->set_kernel_timing(on);
  return 0;
}

int uvio_hp_get_kernel_stats(uvio_hp_t *h, int flush, uvio_hp_kstat_t *out, int cap, int *n) {
  if (!h || !n || (cap > 0 && !out)) return UVIO_HP_E_ARG;
  HP_GUARD(h, h->e->kernel_stats(flush != 0, out, cap, n); return 0;)
}

int uvio_hp_get_clone_times(uvio_hp_t *h, double *out, int cap, int *n) {
  if (!h || !n) return UVIO_HP_E_ARG;
  auto t = h->e->clone_times();
  for (int i = 0; i < (int)t.size() && i < cap; i++) out[i] = t[i];
  *n = (int)t.size();
  return 0;
}

int uvio_hp_get_marginal_cov(uvio_hp_t *h, int nvar, const int *ids, const int *sizes, double *out, int ld) {
  if (!h) return UVIO_HP_E_ARG;
  HP_GUARD(h, return h->e->marginal_cov(nvar, ids, sizes, out, ld);)
}

int uvio_hp_get_good_features_msckf(uvio_hp_t *h, double *xyz_inG, int cap, int *n) {
  if (!h || !n || cap < 0 || (cap > 0 && !xyz_inG)) return UVIO_HP_E_ARG;
  *n = h->e->good_features_msckf(xyz_inG, cap);
  return *n <= cap ? 0 : UVIO_HP_E_CAPACITY;
}

int uvio_hp_odometry_enable(uvio_hp_t *h, int on) {
  if (!h) return UVIO_HP_E_ARG;
  HP_GUARD(h, h->e->odometry_enable(on != 0); return 0;)
}

// Runs beside every other call on the handle: it does not touch the handle's error message (the feed thread's)
int uvio_hp_fast_state_propagate(uvio_hp_t *h, double t, double state_plus[13], double cov[144], int *ok) {
  if (!h || !state_plus || !cov || !ok) return UVIO_HP_E_ARG;
  try {
    HP_HIP(hipSetDevice(h->e->device()));
    return h->e->fast_state_propagate(t, state_plus, cov, ok);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (const std::exception &) {
    return UVIO_HP_E_INTERNAL;
  }
}

// ---- image products (engine_viz.cpp) ----
int uvio_hp_get_track_image(uvio_hp_t *h, uint8_t *out, size_t cap, int *width, int *height, int *overlay) {
  if (!h || !width || !height) return UVIO_HP_E_ARG;
  HP_GUARD(h, return h->e->track_image(out, cap, width, height, overlay, false);)
}

int uvio_hp_get_track_image_device(uvio_hp_t *h, uint8_t *out, size_t cap, int *width, int *height, int *overlay) {
  if (!h || !width || !height) return UVIO_HP_E_ARG;
  HP_GUARD(h, return h->e->track_image(out, cap, width, height, overlay, true);)
}

int uvio_hp_get_track_history(uvio_hp_t *h, int cam, uint64_t id, float *uv, int cap, int *n, int *n_cams,
                              int *to_delete) {
  if (!h || !n || cap < 0 || (cap > 0 && !uv)) return UVIO_HP_E_ARG;
  HP_GUARD(h, return h->e->track_history(cam, id, uv, cap, n, n_cams, to_delete);)
}

int uvio_hp_get_loop_depth(uvio_hp_t *h, uint16_t *depth, uint8_t *viz, size_t cap, int *width, int *height, double *t) {
  if (!h || !width || !height) return UVIO_HP_E_ARG;
  HP_GUARD(h, return h->e->loop_depth(depth, viz, cap, width, height, t);)
}

int uvio_hp_debug_track_image_times(uvio_hp_t *h, int on, double ms[5]) {
  if (!h) return UVIO_HP_E_ARG;
  HP_GUARD(h, return h->e->track_image_times(on, ms);)
}

int uvio_hp_debug_draw_tracks(int ncam, const uint8_t *const *imgs, const int *w, const int *h, const int *strides,
                              const uint8_t *const *masks, const int *counts, const uvio_hp_viz_track_t *tracks,
                              const float *uv, int n_uv, uint8_t *out, size_t cap, int *width, int *height,
                              double *stage_ms) {
  try {
    return Engine::draw_tracks_standalone(ncam, imgs, w, h, strides, masks, counts, tracks, uv, n_uv, out, cap, width,
                                          height, stage_ms);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}

int uvio_hp_debug_loop_depth(const uint8_t *img, int w, int h, int stride, int n, const uint64_t *ids,
                             const double *uvd, uint16_t *depth, uint8_t *viz) {
  try {
    return Engine::loop_depth_standalone(img, w, h, stride, n, ids, uvd, depth, viz);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}

// ---- Updater-level boundary (include/uvio_hp.h) ----
int uvio_hp_set_state(uvio_hp_t *h, const double *val, const double *fej, int len, const double *P, int N, int ld) {
  if (!h || !val || !fej || !P || len <= 0 || N <= 0) return UVIO_HP_E_ARG;
  HP_GUARD(h, { return h->e->api_set_state(val, fej, len, P, N, ld); })
}
int uvio_hp_propagate_and_clone(uvio_hp_t *h, double t) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->api_propagate_and_clone(t))
}
int uvio_hp_msckf_update(uvio_hp_t *h, int nfeat, const uint64_t *featids, const int *meas_off,
                         const uvio_hp_feat_meas_t *meas, uvio_hp_feat_result_t *out) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->api_update(Engine::API_MSCKF, nfeat, featids, meas_off, meas, out))
}
int uvio_hp_slam_update(uvio_hp_t *h, int nfeat, const uint64_t *featids, const int *meas_off,
                        const uvio_hp_feat_meas_t *meas, uvio_hp_feat_result_t *out) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->api_update(Engine::API_SLAM, nfeat, featids, meas_off, meas, out))
}
int uvio_hp_slam_delayed_init(uvio_hp_t *h, int nfeat, const uint64_t *featids, const int *meas_off,
                              const uvio_hp_feat_meas_t *meas, uvio_hp_feat_result_t *out) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->api_update(Engine::API_DELAYED, nfeat, featids, meas_off, meas, out))
}
int uvio_hp_slam_change_anchors(uvio_hp_t *h) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->api_change_anchors())
}
int uvio_hp_marginalize_slam(uvio_hp_t *h) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->api_marginalize_slam())
}
int uvio_hp_marginalize_old_clone(uvio_hp_t *h) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->api_marginalize_old_clone())
}
int uvio_hp_uwb_update_single(uvio_hp_t *h, double t, uint64_t anchor_id, double range, int *applied) {
  (void)t;  // the reference's Jacobian does not read the measurement time (UVioUpdaterHelper.cpp:147-241)
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->api_uwb_update_single(anchor_id, range, applied))
}

int uvio_hp_propagate(uvio_hp_t *h, double t) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->api_propagate(t))
}
int uvio_hp_measurement_update(uvio_hp_t *h, int nvar, const int *ids, const int *sizes, const double *H, int ldh, int r,
                               const double *res, const double *R, int ldr, double chi2_thr, double *chi2, int *applied,
                               double *dx) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->api_measurement_update(nvar, ids, sizes, H, ldh, r, res, R, ldr, chi2_thr, chi2, applied, dx))
}

// ---- caller-defined state variables (engine_api.cpp) ----
int uvio_hp_aux_add(uvio_hp_t *h, int dim, const double *val, const double *prior_cov, int ld, const double *walk_sigma,
                    int *handle) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->api_aux_add(dim, val, prior_cov, ld, walk_sigma, handle))
}
int uvio_hp_aux_add_quat(uvio_hp_t *h, const double q[4], const double *prior_cov, int ld, const double walk_sigma[3],
                         int *handle) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->api_aux_add_quat(q, prior_cov, ld, walk_sigma, handle))
}
int uvio_hp_aux_add_from_measurement(uvio_hp_t *h, int dim, const double *val0, int nvar, const int *ids,
                                     const int *sizes, const double *H_x, int ldhx, const double *H_aux, int ldha,
                                     const double *res, const double *R, int ldr, const double *walk_sigma,
                                     int *handle) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->api_aux_add_from_measurement(dim, val0, nvar, ids, sizes, H_x, ldhx, H_aux, ldha, res, R, ldr,
                                                walk_sigma, handle))
}
int uvio_hp_aux_get(uvio_hp_t *h, int handle, int *id, int *dim, double *val) {
  if (!h) return UVIO_HP_E_ARG;
  HP_GUARD(h, return h->e->api_aux_get(handle, id, dim, val);)
}
int uvio_hp_aux_remove(uvio_hp_t *h, int handle) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->api_aux_remove(handle))
}
int uvio_hp_aux_count(uvio_hp_t *h, int *n, int *dims_used) {
  if (!h) return UVIO_HP_E_ARG;
  return h->e->api_aux_count(n, dims_used);
}

int uvio_hp_aux_append_p(double *P, int N, int ld, int dim, const double *prior, int ldp) {
  try {
    return Engine::aux_append_standalone(P, N, ld, dim, prior, ldp);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}
int uvio_hp_aux_init_p(double *P, int N, int ld, int dim, const int *H_index, int n, const double *H_x, int ldhx,
                       const double *H_auxinv, const double *res_unused_or_null, const double *R, int ldr) {
  (void)res_unused_or_null;  // the residual moves the value only (H_aux^-1 res): the covariance does not read it
  try {
    return Engine::aux_init_standalone(P, N, ld, dim, H_index, n, H_x, ldhx, H_auxinv, R, ldr);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}
int uvio_hp_aux_walk_p(double *P, int N, int ld, int ntab, const int *ids, const int *dims, const double *sigma2,
                       double dt) {
  try {
    return Engine::aux_walk_standalone(P, N, ld, ntab, ids, dims, sigma2, dt);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}
int uvio_hp_debug_cov_propagate_p(double *P, int N, int ld, int s0, int p, const int *rows, const int *iold, int q,
                                  const double *Phi, const double *Q, int clone, int src0, int dt_id, const double *dnc,
                                  int path, int *path_ran) {
  try {
    return Engine::cov_propagate_standalone(P, N, ld, s0, p, rows, iold, q, Phi, Q, clone, src0, dt_id, dnc, path,
                                            path_ran);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}
int uvio_hp_debug_cov_gather_p(const double *P, int N, int ld, int op, int m0, int ms, const int *idx, int n,
                               double *out) {
  try {
    return Engine::cov_gather_standalone(P, N, ld, op, m0, ms, idx, n, out);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}

// ---- buffered position fixes (engine_update.cpp) ----
int uvio_hp_feed_position(uvio_hp_t *h, double t, int r, const double *C, const double *z, const double *R, int ldr,
                          const double *p_SinI, int aux_handle, double chi2_mult, int *queued) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->feed_position(t, r, C, z, R, ldr, p_SinI, aux_handle, chi2_mult, queued))
}
int uvio_hp_get_position_results(uvio_hp_t *h, double *t, double *chi2, int *status, int cap, int *n) {
  if (!h || !n) return UVIO_HP_E_ARG;
  const auto &v = h->e->position_results();
  *n = (int)v.size();
  if (*n > cap) return UVIO_HP_E_CAPACITY;
  for (int k = 0; k < *n; k++) {
    if (t) t[k] = v[(size_t)k].t;
    if (chi2) chi2[k] = v[(size_t)k].chi2;
    if (status) status[k] = v[(size_t)k].status;
  }
  return 0;
}
int uvio_hp_debug_position_update_p(double *P, int N, int ld, int imu_id, const double *q, const double *p, int aux_id,
                                    const double *s, int r, const double *C, const double *z, const double *R, int ldr,
                                    double chi2_thr, double *dx, double *chi2, int *applied) {
  try {
    return Engine::position_update_standalone(P, N, ld, imu_id, q, p, aux_id, s, r, C, z, R, ldr, chi2_thr, dx, chi2,
                                              applied);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}

// ---- buffered pose fixes (engine_update.cpp) ----
int uvio_hp_feed_pose(uvio_hp_t *h, double t, int mode, const double z_q[4], const double *z_p, const double *R, int ldr,
                      const double q_ItoS[4], int rot_handle, const double *p_SinI, int arm_handle, double chi2_mult,
                      int *queued) {
  if (!h) return UVIO_HP_E_ARG;
  HP_FEED(h, h->e->feed_pose(t, mode, z_q, z_p, R, ldr, q_ItoS, rot_handle, p_SinI, arm_handle, chi2_mult, queued))
}
int uvio_hp_get_pose_results(uvio_hp_t *h, double *t, double *chi2, int *status, int cap, int *n) {
  if (!h || !n) return UVIO_HP_E_ARG;
  const auto &v = h->e->pose_results();
  *n = (int)v.size();
  if (*n > cap) return UVIO_HP_E_CAPACITY;
  for (int k = 0; k < *n; k++) {
    if (t) t[k] = v[(size_t)k].t;
    if (chi2) chi2[k] = v[(size_t)k].chi2;
    if (status) status[k] = v[(size_t)k].status;
  }
  return 0;
}
int uvio_hp_debug_pose_update_p(double *P, int N, int ld, int imu_id, const double *q, const double *p, int arm_id,
                                const double *s, int rot_id, const double *q_ItoS, int mode, const double *z_q,
                                const double *z_p, const double *R, int ldr, double chi2_thr, double *dx, double *chi2,
                                int *applied) {
  try {
    return Engine::pose_update_standalone(P, N, ld, imu_id, q, p, arm_id, s, rot_id, q_ItoS, mode, z_q, z_p, R, ldr,
                                          chi2_thr, dx, chi2, applied);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}

int uvio_hp_debug_last_msckf(uvio_hp_t *h, uint64_t *ids, double *pG, int *status, double *chi2, int cap, int *n) {
  if (!h || !n) return UVIO_HP_E_ARG;
  const auto &v = h->e->last_msckf_;
  int k = 0;
  for (const auto &d : v) {
    if (k < cap) {
      ids[k] = d.id;
      for (int j = 0; j < 3; j++) pG[3 * k + j] = d.p_FinG[j];
      status[k] = Engine::debug_status(d.status);
      chi2[k] = d.chi2;
    }
    k++;
  }
  *n = k;
  return 0;
}

int uvio_hp_debug_last_msckf_dx(uvio_hp_t *h, double *dx, int cap, int *n) {
  if (!h || !n) return UVIO_HP_E_ARG;
  const auto &v = h->e->last_msckf_dx_;
  *n = (int)v.size();
  if ((int)v.size() > cap || (!dx && !v.empty())) return UVIO_HP_E_CAPACITY;
  std::copy(v.begin(), v.end(), dx);
  return 0;
}

int uvio_hp_debug_frame_feats(uvio_hp_t *h, int *kind, uint64_t *ids, double *pG, int *status, double *chi2, int cap,
                              int *n) {
  if (!h || !n) return UVIO_HP_E_ARG;
  int k = 0;
  for (const auto &kd : h->e->frame_feats_) {
    if (k < cap) {
      kind[k] = kd.first;
      ids[k] = kd.second.id;
      for (int j = 0; j < 3; j++) pG[3 * k + j] = kd.second.p_FinG[j];
      status[k] = Engine::debug_status(kd.second.status);
      chi2[k] = kd.second.chi2;
    }
    k++;
  }
  *n = k;
  return 0;
}

int uvio_hp_shard_unique_id(uint8_t id[128]) {
  if (!id) return UVIO_HP_E_ARG;
  std::string err;
  int rc = rccl_unique_id(id, &err);
  if (rc) g_create_err = err;
  return rc;
}

int uvio_hp_shard_init_rccl(uvio_hp_t *h, int rank, int world, const uint8_t id[128], int min_features) {
  if (!h || !id) return UVIO_HP_E_ARG;
  HP_GUARD(h, h->e->shard_init_rccl(rank, world, id, min_features); return 0;)
}

int uvio_hp_shard_init_host(uvio_hp_t *h, int rank, int world, uvio_hp_allreduce_fn fn, void *user,
                            int min_features) {
  if (!h || !fn) return UVIO_HP_E_ARG;
  HP_GUARD(h, h->e->shard_init_host(rank, world, fn, user, min_features); return 0;)
}

int uvio_hp_shard_partition(const int *rows, int n, int world, int *bounds) {
  if (!rows || !bounds || n < 0 || world < 1) return UVIO_HP_E_ARG;
  shard_partition(rows, n, world, bounds);
  return 0;
}

int uvio_hp_ekf_update(double *P, int N, const int *H_index, int n, const double *H, int r, const double *res,
                       double sigma2, double *dx_out) {
  try {
    return Engine::ekf_update_standalone(P, N, H_index, n, H, r, res, sigma2, dx_out);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}

int uvio_hp_ekf_update_r(double *P, int N, const int *H_index, int n, const double *H, int r, const double *res,
                         const double *R, int ldr, double chi2_thr, double *dx_out, double *chi2, int *applied) {
  try {
    return Engine::ekf_update_R_standalone(P, N, H_index, n, H, r, res, R, ldr, chi2_thr, dx_out, chi2, applied);
  } catch (const HpError &ex) {
    g_create_err = ex.what();  // (no handle: uvio_hp_last_error(NULL) on this thread)
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}

int uvio_hp_chi2_95(int dof, double *thr) {
  if (!thr || dof < 1 || dof > 999) return UVIO_HP_E_ARG;
  *thr = chi2_quantile95(dof);
  return 0;
}

int uvio_hp_msckf_compressed_update(double *P, int N, const int *H_index, int n, const double *H, int m,
                                    const double *res, double sigma2, double *dx_out) {
  try {
    return Engine::ekf_update_standalone(P, N, H_index, n, H, m, res, sigma2, dx_out, true);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}

int uvio_hp_compress(const double *A, int m, int n, double *R_out) {
  try {
    return Engine::compress_standalone(A, m, n, R_out);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}

int uvio_hp_undistort(int model, const double cam[8], int n, const float *uv, float *uvn, uint8_t *ambiguous) {
  try {
    return Engine::undistort_standalone(model, cam, n, uv, uvn, ambiguous);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}

int uvio_hp_debug_grid_order(const uint8_t *resp, const int *off, int ncell, int kmax, int depth, int *arrangement,
                             int *top) {
  try {
    return Engine::grid_order_standalone(resp, off, ncell, kmax, depth, arrangement, top);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}

int uvio_hp_debug_clahe(const uint8_t *img, int w, int h, int stride, uint8_t *out) {
  try {
    return Engine::clahe_standalone(img, w, h, stride, out);
  } catch (const HpError &ex) {
    return ex.code;
  } catch (...) {
    return UVIO_HP_E_DEVICE;
  }
}

int uvio_hp_debug_grid_stats(uvio_hp_t *h, uint64_t *cells, uint64_t *introsort_cells) {
  if (!h) return UVIO_HP_E_ARG;
  unsigned long long c = 0;
  unsigned long long i = 0;
  HP_GUARD(h, if (h->e->tracker()) h->e->tracker()->grid_stats(&c, &i);)
  if (cells) *cells = c;
  if (introsort_cells) *introsort_cells = i;
  return 0;
}

}  // extern "C"
