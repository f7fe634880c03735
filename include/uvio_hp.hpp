/*
 * uvio_hp.hpp — header-only C++ facade over the C ABI (uvio_hp.h) with the reference's method names, for
 * a maintainer who swaps ov_msckf::VioManager / uvio::UVioManager and the Updater classes for the MI355X
 * path.  Plain standard-library types only (no Eigen / OpenCV / ROS): the ROS adapter converts its
 * cv::Mat / Eigen values at the call site.  Errors become uvio_amd::Error exceptions
 * carrying the status code and the library's message; the library itself never exits the process.
 *
 *   Manager                        <- VioManager (VioManager.h:75-114) + UVioManager (UVioManager.h:48-73)
 *   Manager::msckf_update          <- UpdaterMSCKF::update (UpdaterMSCKF.h:68)
 *   Manager::slam_update           <- UpdaterSLAM::update (UpdaterSLAM.h:70)
 *   Manager::slam_delayed_init     <- UpdaterSLAM::delayed_init (UpdaterSLAM.h:77)
 *   Manager::slam_change_anchors   <- UpdaterSLAM::change_anchors (UpdaterSLAM.h:87)
 *   Manager::uwb_update_single     <- UpdaterUWB::update_single (UpdaterUWB.h:55)
 *   Manager::propagate_and_clone   <- Propagator::propagate_and_clone (Propagator.h:110)
 *   Manager::propagate             <- UVioPropagator::propagate (UVioPropagator.cpp:27)
 *   Manager::measurement_update    <- StateHelper::EKFUpdate (StateHelper.h:88) behind UpdaterUWB.cpp:67-79's gate
 *   Manager::add_state             <- StateHelper::set_initial_covariance (StateHelper.cpp:199) for a variable of the caller's
 *   Manager::add_state_from_measurement <- StateHelper::initialize_invertible (StateHelper.cpp:484)
 *   Manager::feed_position         <- the UWB buffer-and-replay of UVioManager.cpp:178-188 for a position fix
 *   Manager::feed_pose             <- the same for a pose fix (orientation rows, then position rows)
 *   Manager::add_quat_state        <- set_initial_covariance for a JPL quaternion of the caller's (ov_type::JPLQuat)
 */
#ifndef UVIO_HP_HPP
#define UVIO_HP_HPP

#include <array>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "uvio_hp.h"

namespace uvio_amd {

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

// One 8-bit camera image (CV_8UC1 data pointer and row stride); mask optional (nullptr)
struct Image {
  const uint8_t *data = nullptr;
  int stride = 0;
  const uint8_t *mask = nullptr;
};

// ov_core::Feature as plain data: measurements in observation order
struct Feature {
  uint64_t featid = 0;
  std::vector<uvio_hp_feat_meas_t> meas;
};

// JPL quaternion (x, y, z, w) -> rotation matrix, row-major (ov_core quat_ops.h quat_2_Rot)
inline std::array<double, 9> quat_2_Rot(const double q[4]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3], c = 2.0 * w * w - 1.0;
  return {c + 2.0 * x * x,         2.0 * (x * y + w * z),   2.0 * (x * z - w * y),
          2.0 * (x * y - w * z),   c + 2.0 * y * y,         2.0 * (y * z + w * x),
          2.0 * (x * z + w * y),   2.0 * (y * z - w * x),   c + 2.0 * z * z};
}

// A position sensor S mounted at p_SinI in the IMU frame that measures its own position in the global frame:
// h(x) = p_IinG + R_GtoI^T p_SinI.  Over the IMU pose's error state [dtheta, dp] (JPL left error,
// R(dtheta (x) q) ~ (I - [dtheta]x) R): H_theta = -R_GtoI^T [p_SinI]x, H_p = I.  imu: Manager::imu_value's first
// 7 numbers; h (3) and H (3 x 6, row-major) are written.
inline void position_fix_jacobian(const double imu[7], const std::array<double, 3> &p_SinI, double h[3], double H[18]) {
  const std::array<double, 9> R = quat_2_Rot(imu);
  const double s[3] = {p_SinI[0], p_SinI[1], p_SinI[2]};
  const double S[9] = {0.0, -s[2], s[1], s[2], 0.0, -s[0], -s[1], s[0], 0.0};
  for (int i = 0; i < 3; i++) {
    h[i] = imu[4 + i];
    for (int k = 0; k < 3; k++) h[i] += R[(size_t)(3 * k + i)] * s[k];
    for (int j = 0; j < 3; j++) {
      double a = 0.0;
      for (int k = 0; k < 3; k++) a += R[(size_t)(3 * k + i)] * S[3 * k + j];
      H[6 * i + j] = -a;
      H[6 * i + 3 + j] = i == j ? 1.0 : 0.0;
    }
  }
}

// position_fix_jacobian with the lever arm a state variable of the caller's (Manager::add_state): the antenna A at
// p_AinI measures z = p_IinG + R_ItoG p_AinI (R_ItoG = R_GtoI^T).  H (3 x 9, row-major) over [dtheta, dp, dp_AinI]:
// [-R_ItoG [p_AinI]x, I, R_ItoG]; h (3) is the prediction.
inline void position_fix_lever_arm_jacobian(const double imu[7], const std::array<double, 3> &p_AinI, double h[3],
                                            double H[27]) {
  double H6[18];
  position_fix_jacobian(imu, p_AinI, h, H6);
  const std::array<double, 9> R = quat_2_Rot(imu);
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 6; j++) H[9 * i + j] = H6[6 * i + j];
    for (int j = 0; j < 3; j++) H[9 * i + 6 + j] = R[(size_t)(3 * j + i)];
  }
}

// the reference's 95 % chi-squared table (chi2_multipler's factor), dof 1 .. 999
inline double chi2_95(int dof) {
  double v = 0.0;
  const int rc = uvio_hp_chi2_95(dof, &v);
  if (rc) throw Error(rc, "uvio_hp_chi2_95: dof outside 1 .. 999");
  return v;
}

class Manager {
 public:
  explicit Manager(const std::string &estimator_config_yaml, int device = 0) {
    uvio_hp_options_t o;
    check_static(uvio_hp_options_default(&o), "options_default");  // the load overlays the YAML's keys on these
    check_static(uvio_hp_options_load(estimator_config_yaml.c_str(), &o), "options_load " + estimator_config_yaml);
    create(o, device);
  }
  Manager(const uvio_hp_options_t &o, int device) { create(o, device); }
  ~Manager() {
    if (h_) uvio_hp_destroy(h_);
  }
  Manager(const Manager &) = delete;
  Manager &operator=(const Manager &) = delete;

  // ---- VioManager / UVioManager feeds ----
  void initialize_with_gt(const std::array<double, 17> &x) { check(uvio_hp_initialize_with_gt(h_, x.data())); }
  void feed_measurement_imu(double t, const std::array<double, 3> &wm, const std::array<double, 3> &am) {
    check(uvio_hp_feed_imu(h_, t, wm.data(), am.data()));
  }
  // a burst of samples (t[i], wm[i], am[i]) in one call
  void feed_measurement_imu(const std::vector<double> &t, const std::vector<std::array<double, 3>> &wm,
                            const std::vector<std::array<double, 3>> &am) {
    if (wm.size() != t.size() || am.size() != t.size()) throw Error(UVIO_HP_E_ARG, "feed_measurement_imu: size mismatch");
    check(uvio_hp_feed_imu_batch(h_, (int)t.size(), t.data(), wm.empty() ? nullptr : wm[0].data(),
                                 am.empty() ? nullptr : am[0].data()));
  }
  // TrackSIM input: per camera (feature id, raw uv); false before initialization (the reference returns silently)
  bool feed_measurement_simulation(double t, const std::vector<int> &camids,
                                   const std::vector<std::vector<std::pair<uint64_t, std::array<float, 2>>>> &feats) {
    std::vector<int> counts;
    std::vector<uint64_t> ids;
    std::vector<float> uv;
    for (const auto &fc : feats) {
      counts.push_back((int)fc.size());
      for (const auto &f : fc) {
        ids.push_back(f.first);
        uv.push_back(f.second[0]);
        uv.push_back(f.second[1]);
      }
    }
    return soft(uvio_hp_feed_simulation(h_, t, (int)camids.size(), camids.data(), counts.data(), ids.data(), uv.data()));
  }
  // CameraData: images (host memory, or device memory with on_device) per sensor id
  bool feed_measurement_camera(double t, const std::vector<int> &camids, const std::vector<Image> &images,
                               bool on_device = false) {
    std::vector<const uint8_t *> imgs, masks;
    std::vector<int> strides;
    bool any_mask = false;
    for (const auto &im : images) {
      imgs.push_back(im.data);
      strides.push_back(im.stride);
      masks.push_back(im.mask);
      any_mask |= im.mask != nullptr;
    }
    const uint8_t *const *mp = any_mask ? masks.data() : nullptr;
    const int rc = on_device ? uvio_hp_feed_camera_device(h_, t, (int)camids.size(), camids.data(), imgs.data(),
                                                          strides.data(), mp)
                             : uvio_hp_feed_camera(h_, t, (int)camids.size(), camids.data(), imgs.data(),
                                                   strides.data(), mp);
    return soft(rc);
  }
  void feed_measurement_uwb(double t, const std::vector<uint64_t> &anchor_ids, const std::vector<double> &ranges) {
    if (anchor_ids.size() != ranges.size()) throw Error(UVIO_HP_E_ARG, "feed_measurement_uwb: size mismatch");
    check(uvio_hp_feed_uwb(h_, t, (int)anchor_ids.size(), anchor_ids.data(), ranges.data()));
  }
  void try_to_initialize_uwb_anchors(const std::vector<uvio_hp_anchor_t> &anchors) {
    check(uvio_hp_init_anchors(h_, (int)anchors.size(), anchors.data()));
  }

  // ---- getters ----
  bool initialized() const {
    int v = 0;
    check(uvio_hp_initialized(h_, &v));
    return v != 0;
  }
  // [q_GtoI(4) p_IinG(3) v_IinG(3) bg(3) ba(3)] and the state time
  std::array<double, 16> imu_value(double *t = nullptr) const {
    std::array<double, 16> x{};
    double tt = 0;
    check(uvio_hp_get_imu_state(h_, &tt, x.data()));
    if (t) *t = tt;
    return x;
  }
  int cov_dim() const {
    int n = 0;
    check(uvio_hp_get_cov_dim(h_, &n));
    return n;
  }
  std::vector<double> covariance() const {  // row-major N x N
    const int n = cov_dim();
    std::vector<double> P((size_t)n * n);
    check(uvio_hp_get_cov(h_, P.data(), n));
    return P;
  }
  std::vector<double> state_vector() const {
    std::vector<double> x(8192);
    int len = 0, nv = 0;
    check(uvio_hp_get_state_vector(h_, x.data(), (int)x.size(), &len, nullptr, 0, &nv));
    x.resize(len);
    return x;
  }
  // VioManager::get_features_SLAM: the SLAM landmarks as global points (3 per landmark) and, optionally, their ids
  std::vector<double> features_slam(std::vector<uint64_t> *ids = nullptr) const {
    int n = 0;
    const int rc = uvio_hp_get_features_slam(h_, nullptr, nullptr, 0, &n);
    if (rc != UVIO_HP_E_CAPACITY) check(rc);
    std::vector<uint64_t> id((size_t)n);
    std::vector<double> p((size_t)3 * n);
    if (n > 0) check(uvio_hp_get_features_slam(h_, id.data(), p.data(), n, &n));
    if (ids) *ids = id;
    return p;
  }
  uvio_hp_timing_t timing() const {
    uvio_hp_timing_t t{};
    check(uvio_hp_get_timing(h_, &t));
    return t;
  }
  // StateHelper::get_marginal_covariance: blocks = (covariance id, size) per variable, any order, repeats allowed;
  // row-major m x m, m = the sum of the sizes (the pose covariance of publish_state: {{imu id, 6}})
  std::vector<double> marginal_covariance(const std::vector<std::pair<int, int>> &blocks) const {
    std::vector<int> ids, sizes;
    size_t m = 0;
    for (const auto &b : blocks) {
      ids.push_back(b.first);
      sizes.push_back(b.second);
      if (b.second > 0) m += (size_t)b.second;
    }
    std::vector<double> out(m * m);
    check(uvio_hp_get_marginal_cov(h_, (int)blocks.size(), ids.data(), sizes.data(), out.data(), (int)m));
    return out;
  }
  // VioManager::get_good_features_MSCKF: p_FinG, 3 per feature
  std::vector<double> good_features_MSCKF() const {
    int n = 0;
    const int rc = uvio_hp_get_good_features_msckf(h_, nullptr, 0, &n);
    if (rc != UVIO_HP_E_CAPACITY) check(rc);
    std::vector<double> p((size_t)3 * n);
    if (n > 0) check(uvio_hp_get_good_features_msckf(h_, p.data(), n, &n));
    return p;
  }

  // ---- IMU-rate odometry (Propagator::fast_state_propagate, ROS1Visualizer::visualize_odometry) ----
  struct Odometry {
    std::array<double, 13> state_plus{};   // q_GtoI(4) p_IinG(3) v_IinI(3) w_IinI(3)
    std::array<double, 144> covariance{};  // row-major 12 x 12: theta, p, v (local), w
  };
  void enable_odometry(bool on = true) { check(uvio_hp_odometry_enable(h_, on ? 1 : 0)); }
  // false where the reference returns false, and before initialization or with the cache off, where
  // visualize_odometry returns without publishing (ROS1Visualizer.cpp:247-256); out is then untouched.  Callable
  // from any thread beside every other call on the manager (the IMU callback); an error carries the code only
  // (the message belongs to the feed thread).
  bool fast_state_propagate(double t, Odometry &out) const {
    int ok = 0;
    Odometry o;
    const int rc = uvio_hp_fast_state_propagate(h_, t, o.state_plus.data(), o.covariance.data(), &ok);
    if (rc == UVIO_HP_E_STATE) return false;
    if (rc) throw Error(rc, "uvio_hp_fast_state_propagate");
    if (ok) out = o;
    return ok != 0;
  }

  // ---- image products (ROS1Visualizer's trackhist and loop-closure depth images) ----
  // CV_8UC3 data, packed: cv::Mat(height, width, CV_8UC3, data.data()).  overlay: the text display_history would
  // draw on each camera's image and this library does not (0 "CAM:k", 1 "init", 2 "zvupt"; uvio_hp.h)
  struct TrackImage {
    int width = 0, height = 0, overlay = 0;
    std::vector<uint8_t> data;
    bool empty() const { return data.empty(); }
  };
  // VioManager::get_historical_viz_image; empty before the first camera feed
  TrackImage get_historical_viz_image() const {
    TrackImage im;
    check(uvio_hp_get_track_image(h_, nullptr, 0, &im.width, &im.height, &im.overlay));
    im.data.resize((size_t)3 * (size_t)im.width * (size_t)im.height);
    if (!im.data.empty())
      check(uvio_hp_get_track_image(h_, im.data.data(), im.data.size(), &im.width, &im.height, &im.overlay));
    return im;
  }
  // the same into device memory (cap bytes at out_dev); returns {width, height, overlay} with data left empty
  TrackImage get_historical_viz_image_device(uint8_t *out_dev, size_t cap) const {
    TrackImage im;
    check(uvio_hp_get_track_image_device(h_, out_dev, cap, &im.width, &im.height, &im.overlay));
    return im;
  }
  // Feature::uvs[cam] of one feature, oldest first, with Feature::uvs.size() and Feature::to_delete
  struct TrackHistory {
    std::vector<std::array<float, 2>> uv;
    int n_cams = 0;
    bool to_delete = false;
  };
  TrackHistory track_history(int cam, uint64_t featid) const {
    TrackHistory th;
    int n = 0, td = 0;
    const int rc = uvio_hp_get_track_history(h_, cam, featid, nullptr, 0, &n, &th.n_cams, &td);
    if (rc != UVIO_HP_E_CAPACITY) check(rc);
    th.uv.resize((size_t)n);
    if (n > 0) check(uvio_hp_get_track_history(h_, cam, featid, th.uv[0].data(), n, &n, &th.n_cams, &td));
    th.to_delete = td != 0;
    return th;
  }
  // the two images of ROS1Visualizer::publish_loopclosure_information for camera 0: depth CV_16UC1, viz CV_8UC3
  struct LoopDepth {
    int width = 0, height = 0;
    double time = -1;
    std::vector<uint16_t> depth;
    std::vector<uint8_t> viz;
  };
  LoopDepth loop_depth() const {
    LoopDepth ld;
    check(uvio_hp_get_loop_depth(h_, nullptr, nullptr, 0, &ld.width, &ld.height, &ld.time));
    const size_t px = (size_t)ld.width * (size_t)ld.height;
    ld.depth.resize(px);
    ld.viz.resize(3 * px);
    if (px > 0) check(uvio_hp_get_loop_depth(h_, ld.depth.data(), ld.viz.data(), px, &ld.width, &ld.height, &ld.time));
    return ld;
  }

  // ---- updater-level calls (uvio_hp.h "Updater-level boundary") ----
  void set_state(const std::vector<double> &val, const std::vector<double> &fej, const std::vector<double> &P) {
    const int n = cov_dim();
    if (val.size() != fej.size() || P.size() != (size_t)n * n) throw Error(UVIO_HP_E_ARG, "set_state: size mismatch");
    check(uvio_hp_set_state(h_, val.data(), fej.data(), (int)val.size(), P.data(), n, n));
  }
  void propagate_and_clone(double t) { check(uvio_hp_propagate_and_clone(h_, t)); }
  std::vector<uvio_hp_feat_result_t> msckf_update(const std::vector<Feature> &fv) {
    return updater(uvio_hp_msckf_update, fv);
  }
  std::vector<uvio_hp_feat_result_t> slam_update(const std::vector<Feature> &fv) {
    return updater(uvio_hp_slam_update, fv);
  }
  std::vector<uvio_hp_feat_result_t> slam_delayed_init(const std::vector<Feature> &fv) {
    return updater(uvio_hp_slam_delayed_init, fv);
  }
  void slam_change_anchors() { check(uvio_hp_slam_change_anchors(h_)); }
  void marginalize_slam() { check(uvio_hp_marginalize_slam(h_)); }
  void marginalize_old_clone() { check(uvio_hp_marginalize_old_clone(h_)); }
  bool uwb_update_single(double t, uint64_t anchor_id, double range) {
    int applied = 0;
    check(uvio_hp_uwb_update_single(h_, t, anchor_id, range, &applied));
    return applied != 0;
  }


  // ---- a measurement of the caller's own: propagate -> read the state -> build H -> update ----
  // UVioPropagator::propagate: the state to time t (IMU clock) without a clone
  void propagate(double t) { check(uvio_hp_propagate(h_, t)); }
  // (kind, covariance id, size) of every state variable, in state_vector()'s order
  std::vector<std::array<int, 3>> state_meta() const {
    std::vector<double> x(8192);
    std::vector<int> meta(3 * 2048);
    int len = 0, nv = 0;
    check(uvio_hp_get_state_vector(h_, x.data(), (int)x.size(), &len, meta.data(), (int)meta.size(), &nv));
    std::vector<std::array<int, 3>> out;
    for (int k = 0; k < nv && 3 * k + 2 < (int)meta.size(); k++)
      out.push_back({meta[(size_t)3 * k], meta[(size_t)3 * k + 1], meta[(size_t)3 * k + 2]});
    return out;
  }
  struct MeasurementResult {
    bool applied = false;
    double chi2 = 0.0;
    std::vector<double> dx;  // cov_dim() numbers, zeros when the update was gated
  };
  // StateHelper::EKFUpdate(state, H_order, H, res, R) behind a chi2 gate: blocks = (covariance id, size) of H's column
  // blocks (state_meta), H row-major res.size() x (sum of the sizes) over the error state, R row-major
  // res.size() x res.size() of which the upper triangle is read; chi2_thr = INFINITY: no gate
  MeasurementResult measurement_update(const std::vector<std::pair<int, int>> &blocks, const std::vector<double> &H,
                                       const std::vector<double> &res, const std::vector<double> &R,
                                       double chi2_thr = INFINITY) {
    std::vector<int> ids, sizes;
    size_t n = 0;
    for (const auto &b : blocks) {
      ids.push_back(b.first);
      sizes.push_back(b.second);
      if (b.second > 0) n += (size_t)b.second;
    }
    const size_t r = res.size();
    if (H.size() != r * n || R.size() != r * r) throw Error(UVIO_HP_E_ARG, "measurement_update: size mismatch");
    MeasurementResult out;
    out.dx.assign((size_t)cov_dim(), 0.0);
    int applied = 0;
    check(uvio_hp_measurement_update(h_, (int)blocks.size(), ids.data(), sizes.data(), H.data(), (int)n, (int)r,
                                     res.data(), R.data(), (int)r, chi2_thr, &out.chi2, &applied, out.dx.data()));
    out.applied = applied != 0;
    return out;
  }
  // one worked measurement: a global position fix p_meas of a sensor at p_SinI (position_fix_jacobian), noise R
  // (3 x 3 row-major), linearized at the current values and gated at chi2_mult * chi2_95(3)
  MeasurementResult position_fix(const std::array<double, 3> &p_meas, const std::array<double, 3> &p_SinI,
                                 const std::array<double, 9> &R, double chi2_mult = 1.0) {
    const std::array<double, 16> x = imu_value();
    double h[3], H[18];
    position_fix_jacobian(x.data(), p_SinI, h, H);
    int imu_id = 0;
    for (const auto &m : state_meta())
      if (m[0] == 0) imu_id = m[1];  // kind 0: the IMU; its pose is its first 6 columns
    return measurement_update({{imu_id, 6}}, std::vector<double>(H, H + 18),
                              {p_meas[0] - h[0], p_meas[1] - h[1], p_meas[2] - h[2]},
                              std::vector<double>(R.begin(), R.end()), chi2_mult * chi2_95(3));
  }

  // ---- state variables of the caller's own (uvio_hp_aux_*): a lever arm, a sensor bias, a frame offset, a scale ----
  // A new additive variable of val.size() scalars (1 .. 8) with the prior covariance prior_cov (row-major, upper
  // triangle read), uncorrelated with the rest; walk_sigma (empty: a constant): random-walk density per component
  // in unit / sqrt(s).  Needs max_aux_dim in the options.  Returns the handle.
  int add_state(const std::vector<double> &val, const std::vector<double> &prior_cov,
                const std::vector<double> &walk_sigma = {}) {
    const size_t d = val.size();
    if (prior_cov.size() != d * d || (!walk_sigma.empty() && walk_sigma.size() != d))
      throw Error(UVIO_HP_E_ARG, "add_state: size mismatch");
    int handle = 0;
    check(uvio_hp_aux_add(h_, (int)d, val.data(), prior_cov.data(), (int)d, walk_sigma.empty() ? nullptr : walk_sigma.data(),
                          &handle));
    return handle;
  }
  // StateHelper::initialize_invertible for a caller's variable: val0.size() rows res = H_x dx + H_aux dx_aux + noise(R),
  // H_x row-major over the blocks (as measurement_update's), H_aux square and invertible; the value becomes
  // val0 + H_aux^-1 res.  Returns the handle.
  int add_state_from_measurement(const std::vector<double> &val0, const std::vector<std::pair<int, int>> &blocks,
                                 const std::vector<double> &H_x, const std::vector<double> &H_aux,
                                 const std::vector<double> &res, const std::vector<double> &R,
                                 const std::vector<double> &walk_sigma = {}) {
    std::vector<int> ids, sizes;
    size_t n = 0;
    for (const auto &b : blocks) {
      ids.push_back(b.first);
      sizes.push_back(b.second);
      if (b.second > 0) n += (size_t)b.second;
    }
    const size_t d = val0.size();
    if (H_x.size() != d * n || H_aux.size() != d * d || res.size() != d || R.size() != d * d ||
        (!walk_sigma.empty() && walk_sigma.size() != d))
      throw Error(UVIO_HP_E_ARG, "add_state_from_measurement: size mismatch");
    int handle = 0;
    check(uvio_hp_aux_add_from_measurement(h_, (int)d, val0.data(), (int)blocks.size(), ids.data(), sizes.data(),
                                           H_x.data(), (int)n, H_aux.data(), (int)d, res.data(), R.data(), (int)d,
                                           walk_sigma.empty() ? nullptr : walk_sigma.data(), &handle));
    return handle;
  }
  // A JPL unit quaternion [x y z w] of the caller's own (a mounting rotation): 3 error dimensions, updated as
  // q <- dq(dtheta) (x) q; prior_cov 3 x 3 row-major over dtheta, walk_sigma in rad / sqrt(s) (empty: a constant).
  // q is normalized on entry.  Returns the handle; aux_state(handle).value then holds 4 doubles.
  int add_quat_state(const std::array<double, 4> &q, const std::array<double, 9> &prior_cov,
                     const std::vector<double> &walk_sigma = {}) {
    if (!walk_sigma.empty() && walk_sigma.size() != 3) throw Error(UVIO_HP_E_ARG, "add_quat_state: size mismatch");
    int handle = 0;
    check(uvio_hp_aux_add_quat(h_, q.data(), prior_cov.data(), 3, walk_sigma.empty() ? nullptr : walk_sigma.data(),
                               &handle));
    return handle;
  }
  struct AuxState {
    int id = 0;  // the covariance offset NOW: it moves when clones / landmarks in front are marginalized
    std::vector<double> value;  // a quaternion variable: 4 values over 3 error dimensions
  };
  AuxState aux_state(int handle) const {
    AuxState a;
    int dim = 0;
    double v[UVIO_HP_AUX_MAX_DIM];
    for (double &x : v) x = std::numeric_limits<double>::quiet_NaN();
    check(uvio_hp_aux_get(h_, handle, &a.id, &dim, v));
    // a quaternion variable reports dim = 3 and writes 4 doubles (values are always finite)
    a.value.assign(v, v + ((dim == 3 && v[3] == v[3]) ? 4 : dim));
    return a;
  }
  // marginalizes the variable; the handle is dead afterwards
  void remove_state(int handle) { check(uvio_hp_aux_remove(h_, handle)); }
  // position_fix with the lever arm p_AinI the aux variable `handle` (3 scalars, add_state): H over
  // [IMU pose | p_AinI] (position_fix_lever_arm_jacobian), the aux offset read at the call
  MeasurementResult position_fix_lever_arm(const std::array<double, 3> &p_meas, int handle, const std::array<double, 9> &R,
                                           double chi2_mult = 1.0) {
    const std::array<double, 16> x = imu_value();
    const AuxState a = aux_state(handle);
    if (a.value.size() != 3) throw Error(UVIO_HP_E_ARG, "position_fix_lever_arm: the variable is not a 3-vector");
    double h[3], H[27];
    position_fix_lever_arm_jacobian(x.data(), {a.value[0], a.value[1], a.value[2]}, h, H);
    int imu_id = 0;
    for (const auto &m : state_meta())
      if (m[0] == 0) imu_id = m[1];
    return measurement_update({{imu_id, 6}, {a.id, 3}}, std::vector<double>(H, H + 27),
                              {p_meas[0] - h[0], p_meas[1] - h[1], p_meas[2] - h[2]},
                              std::vector<double>(R.begin(), R.end()), chi2_mult * chi2_95(3));
  }

  // ---- buffered position fixes (uvio_hp_feed_position): replayed in time order inside the next frame ----
  // z = C (p_IinG + R_GtoI^T s) + noise(R): z.size() = r rows (1 .. 3), C row-major r x 3, R row-major r x r (upper
  // triangle read), s the constant lever arm p_SinI or, with aux_handle > 0, a 3-scalar variable of add_state; gated at
  // chi2_mult * chi2_95(r) (INFINITY: no gate).  True when queued; false when the filter is not initialized or t is
  // not after the state time
  bool feed_position(double t, const std::vector<double> &z, const std::vector<double> &C, const std::vector<double> &R,
                     const std::array<double, 3> &p_SinI = {0.0, 0.0, 0.0}, int aux_handle = 0, double chi2_mult = 1.0) {
    const size_t r = z.size();
    if (C.size() != 3 * r || R.size() != r * r) throw Error(UVIO_HP_E_ARG, "feed_position: size mismatch");
    int queued = 0;
    check(uvio_hp_feed_position(h_, t, (int)r, C.data(), z.data(), R.data(), (int)r, p_SinI.data(), aux_handle, chi2_mult,
                                &queued));
    return queued != 0;
  }
  struct PositionResult {
    double t = 0.0, chi2 = 0.0;
    int status = 0;  // 0 applied, 1 gated, 2 dropped, 3 refused
  };
  // the fixes the last camera / simulation feed consumed, in processing order
  std::vector<PositionResult> position_results() const {
    int n = 0;
    const int rc = uvio_hp_get_position_results(h_, nullptr, nullptr, nullptr, 0, &n);
    if (rc != UVIO_HP_E_CAPACITY) check(rc);
    std::vector<double> t((size_t)n), c((size_t)n);
    std::vector<int> s((size_t)n);
    if (n > 0) check(uvio_hp_get_position_results(h_, t.data(), c.data(), s.data(), n, &n));
    std::vector<PositionResult> out((size_t)n);
    for (size_t k = 0; k < out.size(); k++) out[k].t = t[k], out[k].chi2 = c[k], out[k].status = s[k];
    return out;
  }

  // ---- buffered pose fixes (uvio_hp_feed_pose): the sensor frame S's pose in G, z_q = q_GtoS and z_p = p_SinG ----
  // R row-major r x r (r = 3: orientation only, z_p unused; r = 6: orientation rows, then position rows), the mounting
  // rotation q_ItoS constant or, with rot_handle > 0, a variable of add_quat_state; the lever arm p_SinI constant or,
  // with arm_handle > 0, a 3-scalar variable of add_state.  True when queued.
  bool feed_pose(double t, const std::array<double, 4> &z_q, const std::array<double, 3> &z_p, const std::vector<double> &R,
                 const std::array<double, 4> &q_ItoS = {0.0, 0.0, 0.0, 1.0}, int rot_handle = 0,
                 const std::array<double, 3> &p_SinI = {0.0, 0.0, 0.0}, int arm_handle = 0, double chi2_mult = 1.0) {
    if (R.size() != 9 && R.size() != 36) throw Error(UVIO_HP_E_ARG, "feed_pose: R is neither 3 x 3 nor 6 x 6");
    const bool full = R.size() == 36;
    int queued = 0;
    check(uvio_hp_feed_pose(h_, t, full ? UVIO_HP_POSE_FULL : UVIO_HP_POSE_ORIENTATION, z_q.data(), z_p.data(), R.data(),
                            full ? 6 : 3, q_ItoS.data(), rot_handle, p_SinI.data(), arm_handle, chi2_mult, &queued));
    return queued != 0;
  }
  // the pose fixes the last camera / simulation feed consumed, in processing order
  std::vector<PositionResult> pose_results() const {
    int n = 0;
    const int rc = uvio_hp_get_pose_results(h_, nullptr, nullptr, nullptr, 0, &n);
    if (rc != UVIO_HP_E_CAPACITY) check(rc);
    std::vector<double> t((size_t)n), c((size_t)n);
    std::vector<int> s((size_t)n);
    if (n > 0) check(uvio_hp_get_pose_results(h_, t.data(), c.data(), s.data(), n, &n));
    std::vector<PositionResult> out((size_t)n);
    for (size_t k = 0; k < out.size(); k++) out[k].t = t[k], out[k].chi2 = c[k], out[k].status = s[k];
    return out;
  }

  uvio_hp_t *handle() { return h_; }

 private:
  uvio_hp_t *h_ = nullptr;

  void create(const uvio_hp_options_t &o, int device) {
    const int rc = uvio_hp_create(&o, device, &h_);
    if (rc) {
      const char *m = uvio_hp_last_error(nullptr);
      throw Error(rc, std::string("uvio_hp_create: ") + (m ? m : ""));
    }
  }
  static void check_static(int rc, const std::string &what) {
    if (rc) throw Error(rc, what);
  }
  void check(int rc) const {
    if (rc) {
      const char *m = uvio_hp_last_error(h_);
      throw Error(rc, m ? m : "uvio_hp");
    }
  }
  // E_STATE before initialization: the reference's feeds return without doing anything
  bool soft(int rc) const {
    if (rc == UVIO_HP_E_STATE) return false;
    check(rc);
    return true;
  }
  template <class Fn>
  std::vector<uvio_hp_feat_result_t> updater(Fn fn, const std::vector<Feature> &fv) {
    std::vector<uint64_t> ids;
    std::vector<int> off{0};
    std::vector<uvio_hp_feat_meas_t> meas;
    for (const auto &f : fv) {
      ids.push_back(f.featid);
      meas.insert(meas.end(), f.meas.begin(), f.meas.end());
      off.push_back((int)meas.size());
    }
    std::vector<uvio_hp_feat_result_t> out(fv.size());
    check(fn(h_, (int)fv.size(), ids.data(), off.data(), meas.data(), out.data()));
    return out;
  }
};

// nav_msgs::Odometry's two 6 x 6 covariances from fast_state_propagate's 12 x 12 (ROS1Visualizer.cpp:311-325):
// ROS orders a pose as position, then orientation, so the (theta, p) blocks swap; the twist (v local, w) is kept
inline void odometry_covariance_ros(const std::array<double, 144> &cov, std::array<double, 36> &pose,
                                    std::array<double, 36> &twist) {
  static const int perm[12] = {3, 4, 5, 0, 1, 2, 6, 7, 8, 9, 10, 11};
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) {
      pose[(size_t)(6 * r + c)] = cov[(size_t)(12 * perm[r] + perm[c])];
      twist[(size_t)(6 * r + c)] = cov[(size_t)(12 * perm[r + 6] + perm[c + 6])];
    }
}

// histogram_method CLAHE (cv::createCLAHE(10.0, Size(8, 8))->apply) of one 8-bit image with the tracker's own
// kernels (uvio_hp_debug_clahe): w x h pixels, rows `stride` bytes apart, both sides >= 9; returns w * h packed
inline std::vector<uint8_t> clahe(const uint8_t *img, int w, int h, int stride) {
  std::vector<uint8_t> out(w > 0 && h > 0 ? (size_t)w * (size_t)h : 0);
  const int rc = uvio_hp_debug_clahe(img, w, h, stride, out.data());
  if (rc) throw Error(rc, "uvio_hp_debug_clahe");
  return out;
}

// get_historical_viz_image's renderer on caller-given inputs (uvio_hp_debug_draw_tracks): per camera an image (its
// mask, if any, at the image's stride), its size and its tracks in draw order, whose histories lie in uv ((u, v)
// pairs); returns the packed CV_8UC3 canvas and its size
struct DrawCamera {
  Image image;
  int width = 0, height = 0;
  std::vector<uvio_hp_viz_track_t> tracks;
};
inline std::vector<uint8_t> draw_tracks(const std::vector<DrawCamera> &cams, const std::vector<float> &uv, int *width,
                                        int *height) {
  std::vector<const uint8_t *> imgs, masks;
  std::vector<int> w, h, strides, counts;
  std::vector<uvio_hp_viz_track_t> tracks;
  for (const auto &c : cams) {
    imgs.push_back(c.image.data);
    masks.push_back(c.image.mask);
    strides.push_back(c.image.stride);
    w.push_back(c.width);
    h.push_back(c.height);
    counts.push_back((int)c.tracks.size());
    tracks.insert(tracks.end(), c.tracks.begin(), c.tracks.end());
  }
  int cw = 0, ch = 0;
  int rc = uvio_hp_debug_draw_tracks((int)cams.size(), imgs.data(), w.data(), h.data(), strides.data(), masks.data(),
                                     counts.data(), tracks.data(), uv.data(), (int)(uv.size() / 2), nullptr, 0, &cw, &ch,
                                     nullptr);
  if (rc) throw Error(rc, "uvio_hp_debug_draw_tracks");
  std::vector<uint8_t> out((size_t)3 * (size_t)cw * (size_t)ch);
  rc = uvio_hp_debug_draw_tracks((int)cams.size(), imgs.data(), w.data(), h.data(), strides.data(), masks.data(),
                                 counts.data(), tracks.data(), uv.data(), (int)(uv.size() / 2), out.data(), out.size(),
                                 &cw, &ch, nullptr);
  if (rc) throw Error(rc, "uvio_hp_debug_draw_tracks");
  if (width) *width = cw;
  if (height) *height = ch;
  return out;
}

}  // namespace uvio_amd

#endif  // UVIO_HP_HPP
