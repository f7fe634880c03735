// Engine: per-frame manager logic (VioManager.cpp:166-651, UVioManager.cpp:61-344), feature database
// (FeatureDatabase.cpp:59-263) and the update orchestration (UpdaterMSCKF.cpp:58-295,
// UpdaterSLAM.cpp:61-647, UpdaterUWB.cpp:53-90) over the device kernels.
#include <exception>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unordered_set>

#include "engine.h"

namespace uvhp {

using clk = std::chrono::steady_clock;
static double secs(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// ---- chi-squared 0.95 quantile (boost::math::quantile(chi_squared(dof), 0.95), UpdaterMSCKF.cpp:52-55) ----
static double gamma_p(double a, double x) {
  if (x <= 0) return 0.0;
  double gln = std::lgamma(a);
  if (x < a + 1.0) {
    double ap = a, sum = 1.0 / a, del = sum;
    for (int n = 0; n < 100000; n++) {
      ap += 1;
      del *= x / ap;
      sum += del;
      if (std::fabs(del) < std::fabs(sum) * 1e-17) break;
    }
    return sum * std::exp(-x + a * std::log(x) - gln);
  }
  double b = x + 1.0 - a, c = 1e300, d = 1.0 / b, h = d;
  for (int i = 1; i < 100000; i++) {
    double an = -i * (i - a);
    b += 2.0;
    d = an * d + b;
    if (std::fabs(d) < 1e-300) d = 1e-300;
    c = b + an / c;
    if (std::fabs(c) < 1e-300) c = 1e-300;
    d = 1.0 / d;
    double del = d * c;
    h *= del;
    if (std::fabs(del - 1.0) < 1e-17) break;
  }
  return 1.0 - std::exp(-x + a * std::log(x) - gln) * h;
}
double chi2_quantile95(int dof) {
  double a = 0.5 * dof, lo = 0, hi = std::max(10.0, 4.0 * dof + 50);
  for (int it = 0; it < 200; it++) {
    double mid = 0.5 * (lo + hi);
    if (gamma_p(a, 0.5 * mid) < 0.95)
      lo = mid;
    else
      hi = mid;
    if (hi - lo < 1e-14 * std::max(1.0, hi)) break;
  }
  return 0.5 * (lo + hi);
}

// ---------------------------------------------------------------------------------------------------
// VioManagerHelper.cpp:40-76
void Engine::initialize_with_gt(const double x[17]) {
  for (int k = 0; k < 16; k++) imu_->val[k] = imu_->fej[k] = x[1 + k];
  std::vector<double> cov(15 * 15, 0.0);
  for (int k = 0; k < 15; k++) cov[k * 15 + k] = 0.02 * 0.02;
  for (int k = 0; k < 3; k++) {
    cov[k * 15 + k] = 0.017 * 0.017;
    cov[(3 + k) * 15 + 3 + k] = 0.05 * 0.05;
    cov[(6 + k) * 15 + 6 + k] = 0.01 * 0.01;
  }
  set_initial_covariance(cov, {imu_});
  timestamp_ = x[0];
  startup_time_ = x[0];
  is_initialized_ = true;
  db_cleanup_measurements(timestamp_);
  {
    std::lock_guard<std::mutex> lk(imu_mtx_);
    init_imu_.clear();
  }
  odom_invalidate();
  odom_flush();
}

// VioManager.cpp:166-189 + Propagator::feed_imu (Propagator.h:65-91)
void Engine::feed_imu(double t, const double wm[3], const double am[3]) {
  double oldest = margtimestep();
  if (oldest > timestamp_) oldest = -1;
  if (!is_initialized_) oldest = t - o_.init_window_time + calib_dt_->val[0] - 0.10;
  ImuSample s;
  s.t = t;
  for (int k = 0; k < 3; k++) s.wm[k] = wm[k], s.am[k] = am[k];
  std::lock_guard<std::mutex> lk(imu_mtx_);
  imu_data_.push_back(s);
  // InertialInitializer::feed_imu (InertialInitializer.cpp:49-71): its age test reads the new message's
  // time, so the buffer is emptied only by a message older than oldest (never, in time order); the
  // window is trimmed in InertialInitializer::initialize
  if (!is_initialized_ && !init_success_) {
    init_imu_.push_back(s);
    if (oldest != -1 && t < oldest) init_imu_.clear();
  }
  double cut = oldest - 0.10;
  // UpdaterZeroVelocity::feed_imu (VioManager.cpp:186-188; UpdaterZeroVelocity.h:77-107)
  if (is_initialized_ && o_.try_zupt && (!o_.zupt_only_at_beginning || !has_moved_since_zupt_)) {
    zupt_imu_.push_back(s);
    if (cut >= 0)
      zupt_imu_.erase(std::remove_if(zupt_imu_.begin(), zupt_imu_.end(), [&](const ImuSample &a) { return a.t < cut; }),
                      zupt_imu_.end());
  }
  if (cut >= 0) {
    auto it = imu_data_.begin();
    while (it != imu_data_.end() && it->t < cut) it++;
    // measurements arrive in time order: erase the prefix (same result as the reference's scan)
    bool sorted = true;
    for (auto jt = it; jt != imu_data_.end(); ++jt)
      if (jt->t < cut) sorted = false;
    if (sorted)
      imu_data_.erase(imu_data_.begin(), it);
    else
      imu_data_.erase(std::remove_if(imu_data_.begin(), imu_data_.end(), [&](const ImuSample &a) { return a.t < cut; }),
                      imu_data_.end());
  }
}

// FeatureDatabase::update_feature (FeatureDatabase.cpp:59-85)
void Engine::db_update(size_t id, double t, size_t cam, float u, float v, float un, float vn) {
  auto it = db_.find(id);
  Feature *f;  // no shared_ptr copy (two atomic reference-count updates per observation)
  if (it != db_.end()) {
    f = it->second.get();
  } else {
    FeatP nf = new_feature(id);
    f = nf.get();
    db_insert(id, std::move(nf));
  }
  f->track(cam).m.push_back(FeatMeas{u, v, un, vn, t});
}

// UVioManager.cpp:61-79
int Engine::feed_uwb(double t, int n, const uint64_t *ids, const double *ranges) {
  stage_ = "feed_uwb";
  if (!(is_initialized_ && anchors_initialized_ && distance_ > o_.min_dist_to_use_uwb)) return 0;
  if (timestamp_ >= t) return 0;
  auto &m = past_uwb_[t];
  for (int i = 0; i < n; i++) m[(size_t)ids[i]] = ranges[i];
  return 0;
}

// A position fix z = C (p_IinG + R_GtoI^T s) + noise(R) for the next frame's replay (after_tracking), buffered the
// way feed_uwb buffers a message.  Every refusal comes before anything is stored.
int Engine::feed_position(double t, int r, const double *C, const double *z, const double *R, int ldr,
                          const double *p_SinI, int aux_handle, double chi2_mult, int *queued) {
  stage_ = "feed_position";
  const char *who = "feed_position: ";
  if (!C || !z || !R || !queued || (aux_handle <= 0 && !p_SinI)) throw HpError(UVIO_HP_E_ARG, std::string(who) + "null pointer");
  *queued = 0;
  if (r < 1 || r > 3) throw HpError(UVIO_HP_E_ARG, std::string(who) + "r outside 1 .. 3");
  if (ldr < r) throw HpError(UVIO_HP_E_ARG, std::string(who) + "leading dimension below the row length");
  if (!(chi2_mult > 0.0)) throw HpError(UVIO_HP_E_ARG, std::string(who) + "chi2_mult must be positive");
  FixMeas m{};
  bool finite = std::isfinite(t);
  for (int i = 0; i < r; i++) {
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(m.C[3 * i + k] = C[3 * i + k]);
    finite = finite && std::isfinite(m.z[i] = z[i]);
    for (int j = i; j < r; j++) finite = finite && std::isfinite(m.R[3 * i + j] = m.R[3 * j + i] = R[(size_t)i * ldr + j]);
  }
  if (aux_handle <= 0)
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(m.s[k] = p_SinI[k]);
  if (!finite)
    throw HpError(UVIO_HP_E_ARG, std::string(who) + "t, C, z, the upper triangle of R or p_SinI is not finite");
  for (int i = 0; i < r; i++)
    if (!(m.R[4 * i] > 0.0)) throw HpError(UVIO_HP_E_ARG, std::string(who) + "the diagonal of R must be positive");
  // feed_uwb's behaviour (UVioManager.cpp:61-79): nothing is kept before initialization or at a time the state has passed
  if (!is_initialized_ || timestamp_ >= t) return 0;
  if (aux_handle > 0) {
    auto it = aux_.find(aux_handle);
    if (it == aux_.end()) throw HpError(UVIO_HP_E_ARG, std::string(who) + "no live aux variable has this handle");
    if (it->second.v->kind != V_AUX || it->second.v->size != 3)
      throw HpError(UVIO_HP_E_ARG, std::string(who) + "the aux variable is not a 3-vector");
  }
  if (fix_queued_ >= kFixQueueMax)
    throw HpError(UVIO_HP_E_CAPACITY, std::string(who) + "more than " + std::to_string(kFixQueueMax) + " fixes queued");
  m.r = r;
  m.aux = aux_handle > 0 ? aux_handle : 0;
  m.thr = chi2_mult * chi2_table_[r];
  past_fix_[t].push_back(m);
  fix_queued_++;
  *queued = 1;
  return 0;
}

// a finite quaternion whose norm lies in [0.5, 2], normalized into out (uvio_hp_aux_add_quat, uvio_hp_feed_pose)
bool unit_quat_ok(const double *q, double *out) {
  double n2 = 0.0;
  for (int k = 0; k < 4; k++) {
    if (!std::isfinite(q[k])) return false;
    n2 += q[k] * q[k];
  }
  const double n = std::sqrt(n2);
  if (!(n >= 0.5 && n <= 2.0)) return false;
  for (int k = 0; k < 4; k++) out[k] = q[k] / n;
  return true;
}

// A pose fix (kernels.h DPoseState) for the next frame's replay, into feed_position's queue.  Every refusal comes
// before anything is stored.
int Engine::feed_pose(double t, int mode, const double *z_q, const double *z_p, const double *R, int ldr,
                      const double *q_ItoS, int rot_handle, const double *p_SinI, int arm_handle, double chi2_mult,
                      int *queued) {
  stage_ = "feed_pose";
  const std::string who = "feed_pose: ";
  if (!queued) throw HpError(UVIO_HP_E_ARG, who + "null pointer");
  *queued = 0;
  if (mode != UVIO_HP_POSE_ORIENTATION && mode != UVIO_HP_POSE_FULL)
    throw HpError(UVIO_HP_E_ARG, who + "mode is neither UVIO_HP_POSE_ORIENTATION nor UVIO_HP_POSE_FULL");
  const bool full = mode == UVIO_HP_POSE_FULL;
  const int r = full ? 6 : 3;
  if (!z_q || !R || (full && !z_p) || (rot_handle <= 0 && !q_ItoS) || (full && arm_handle <= 0 && !p_SinI))
    throw HpError(UVIO_HP_E_ARG, who + "null pointer");
  if (ldr < r) throw HpError(UVIO_HP_E_ARG, who + "leading dimension below the row length");
  if (!(chi2_mult > 0.0)) throw HpError(UVIO_HP_E_ARG, who + "chi2_mult must be positive");
  FixMeas m{};
  bool finite = std::isfinite(t);
  constexpr int ldm = kChainMaxRows;
  for (int i = 0; i < r; i++)
    for (int j = i; j < r; j++)
      finite = finite && std::isfinite(m.Rp[ldm * i + j] = m.Rp[ldm * j + i] = R[(size_t)i * ldr + j]);
  if (full)
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(m.z[k] = z_p[k]);
  if (full && arm_handle <= 0)
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(m.s[k] = p_SinI[k]);
  if (!finite) throw HpError(UVIO_HP_E_ARG, who + "t, z_p, the upper triangle of R or p_SinI is not finite");
  if (!unit_quat_ok(z_q, m.zq)) throw HpError(UVIO_HP_E_ARG, who + "z_q is not finite or its norm is outside [0.5, 2]");
  m.qS[3] = 1.0;
  if (rot_handle <= 0 && !unit_quat_ok(q_ItoS, m.qS))
    throw HpError(UVIO_HP_E_ARG, who + "q_ItoS is not finite or its norm is outside [0.5, 2]");
  for (int i = 0; i < r; i++)
    if (!(m.Rp[(ldm + 1) * i] > 0.0)) throw HpError(UVIO_HP_E_ARG, who + "the diagonal of R must be positive");
  if (!is_initialized_ || timestamp_ >= t) return 0;  // feed_uwb's behaviour, as in feed_position
  if (rot_handle > 0) {
    auto it = aux_.find(rot_handle);
    if (it == aux_.end()) throw HpError(UVIO_HP_E_ARG, who + "no live aux variable has the rotation handle");
    if (it->second.v->kind != V_AUX_QUAT)
      throw HpError(UVIO_HP_E_ARG, who + "the rotation handle is not a quaternion variable");
  }
  if (arm_handle > 0) {
    auto it = aux_.find(arm_handle);
    if (it == aux_.end()) throw HpError(UVIO_HP_E_ARG, who + "no live aux variable has the lever-arm handle");
    if (it->second.v->kind != V_AUX || it->second.v->size != 3)
      throw HpError(UVIO_HP_E_ARG, who + "the lever-arm handle is not a 3-vector");
  }
  if (fix_queued_ >= kFixQueueMax)
    throw HpError(UVIO_HP_E_CAPACITY, who + "more than " + std::to_string(kFixQueueMax) + " fixes queued");
  m.pose_r = r;
  m.rot = rot_handle > 0 ? rot_handle : 0;
  m.aux = arm_handle > 0 ? arm_handle : 0;
  m.thr = chi2_mult * chi2_table_[r];
  past_fix_[t].push_back(m);
  fix_queued_++;
  *queued = 1;
  return 0;
}

// UVioManager.cpp:81-113 / 207-266
int Engine::init_anchors(int n, const uvio_hp_anchor_t *a) {
  if (n <= 0) return 0;
  for (int i = 0; i < n; i++) {
    if (anchors_.find(a[i].id) != anchors_.end()) continue;
    VarP v = std::make_shared<Var>(V_ANCHOR, 5, 5);
    v->anchor_id = a[i].id;
    v->fixed = a[i].fix != 0;
    double x[5] = {a[i].p_AinG[0], a[i].p_AinG[1], a[i].p_AinG[2], a[i].const_bias, a[i].dist_bias};
    for (int k = 0; k < 5; k++) v->val[k] = v->fej[k] = x[k];
    anchors_.insert({(size_t)a[i].id, v});
    if (!a[i].fix) {
      std::vector<double> HR(15, 0.0), HL(25, 0.0), R(25, 0.0), res(5, 0.0);
      for (int k = 0; k < 5; k++) HL[6 * k] = 1.0, R[6 * k] = 1.0;
      initialize_invertible_host(v, {{imu_->id, 3}}, HR, HL, R, res);
      std::vector<double> cov(25, 0.0);
      for (int k = 0; k < 5; k++) cov[6 * k] = a[i].cov_diag[k];
      set_initial_covariance(cov, {v});
    }
  }
  anchors_initialized_ = true;
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// VioManager.cpp:191-254 + TrackSIM.cpp:30-79 (+ the UVIO range loop of UVioManager.cpp:178-188)
int Engine::feed_simulation(double t, int ncam, const int *cam_ids, const int *counts, const uint64_t *ids,
                            const float *uv) {
  stage_ = "feed_simulation";
  auto rT1 = clk::now();
  early_prop_s_ = 0.0;
  frame_begin();
  retri_flush();  // the previous frame's retriangulation reads frame_obs_, which this feed refills
  std::vector<int> camids, cam_of;
  for (int i = 0; i < ncam; i++) {
    int cid = cam_ids[i];
    if (cid < 0 || cid >= o_.num_cameras || counts[i] < 0) return UVIO_HP_E_ARG;
    camids.push_back(cid);
    cam_of.insert(cam_of.end(), counts[i], cid);
  }
  // FeatureDatabase::update_feature for every observation, in order, in three passes with the same
  // result: (a) undistort every observation, record it for the retriangulation and look up the known
  // features (independent per observation, read-only on db_, one pool job), (b) insert the new ids into db_
  // sequentially in observation order (db_'s iteration order depends on it), (c) append each observation
  // to its feature; features are split across workers by pointer, and every worker walks the observations
  // in order, so each feature's appends keep the sequential order.
  const size_t nobs = cam_of.size();
  std::vector<float> uvn(2 * nobs);
  std::vector<Feature *> fp(nobs, nullptr);
  frame_obs_.resize(nobs);
  {
    HPROF("feed.undistort_lookup");
    pool_.parallel_for(nobs, 2048, [&](size_t b, size_t e) {
      for (size_t k = b; k < e; k++) {
        const size_t id = (size_t)ids[k] + currid_;
        cam_undistort_f(cams_[cam_of[k]], uv[2 * k], uv[2 * k + 1], uvn[2 * k], uvn[2 * k + 1]);
        DRetriObs &o = frame_obs_[k];
        o.featid = (unsigned long long)id;
        o.u = uv[2 * k];
        o.v = uv[2 * k + 1];
        o.un = uvn[2 * k];
        o.vn = uvn[2 * k + 1];
        o.cam = cam_of[k];
        o.pad = 0;
        auto it = db_.find(id);
        if (it != db_.end()) fp[k] = it->second.get();
      }
    });
  }
  // (b) and (c) as one pool job: its first task inserts the new ids in observation order while the other
  // tasks append the observations of the features db_ already held (they touch neither db_ nor a new
  // feature); then the new features' observations are appended.  Every feature's observations are all in
  // one of the two groups, so its appends keep the sequential order.
  {
    HPROF("feed.db");
    // 4 buckets per thread: the known features' buckets share the threads with the insert task and are
    // taken dynamically (one bucket per thread left one thread with two while the others waited)
    const uint32_t nw = 4 * (uint32_t)pool_.threads();
    std::vector<uint32_t> known, fresh;
    known.reserve(nobs);
    for (size_t k = 0; k < nobs; k++) (fp[k] ? known : fresh).push_back((uint32_t)k);
    // bucket a list of observations by owning worker (a counting sort that keeps observation order inside a
    // bucket); a worker appends its bucket with the feature objects prefetched a few entries ahead -- the
    // appends are cache-miss bound (feature, its track array, the measurement storage)
    struct Buckets {
      std::vector<uint32_t> start, order;
    };
    auto bucket = [&](const std::vector<uint32_t> &obs, Buckets &bk) {
      bk.start.assign(nw + 1, 0);
      bk.order.resize(obs.size());
      std::vector<uint16_t> owner(obs.size());
      for (size_t i = 0; i < obs.size(); i++) {
        const uint64_t h = (uint64_t)((uintptr_t)fp[obs[i]] >> 6) * 0x9E3779B97F4A7C15ull;
        owner[i] = (uint16_t)(((h >> 32) * nw) >> 32);
        bk.start[owner[i] + 1]++;
      }
      for (uint32_t w = 0; w < nw; w++) bk.start[w + 1] += bk.start[w];
      std::vector<uint32_t> pos(bk.start.begin(), bk.start.end() - 1);
      for (size_t i = 0; i < obs.size(); i++) bk.order[pos[owner[i]]++] = obs[i];
    };
    auto append = [&](const Buckets &bk, uint32_t w) {
      const uint32_t i0 = bk.start[w], i1 = bk.start[w + 1];
      for (uint32_t i = i0; i < i1; i++) {
        // two-stage software prefetch: the feature object's first three lines (its tracks) 32 ahead, then
        // the append slot of the observation's camera track 16 ahead
        if (i + 32 < i1) {
          const char *p = (const char *)fp[bk.order[i + 32]];
          __builtin_prefetch(p, 1);
          __builtin_prefetch(p + 64, 1);
          __builtin_prefetch(p + 128, 1);
        }
        if (i + 16 < i1) {
          const size_t k2 = bk.order[i + 16];
          for (const CamTrack &c : fp[k2]->tracks)
            if ((int)c.cam == cam_of[k2]) __builtin_prefetch(c.m.v.data() + c.m.v.size(), 1);
        }
        const size_t k = bk.order[i];
        fp[k]->track((size_t)cam_of[k]).m.push_back(FeatMeas{uv[2 * k], uv[2 * k + 1], uvn[2 * k], uvn[2 * k + 1], t});
      }
    };
    Buckets bk_known, bk_fresh;
    {
      HPROF("feed.db.bucket");
      bucket(known, bk_known);
    }
    const size_t db0 = db_.size();
    auto tj0 = clk::now();
    pool_.parallel_for((size_t)nw + 1, 1, [&](size_t b, size_t e) {
      for (size_t w = b; w < e; w++) {
        if (w > 0) {
          append(bk_known, (uint32_t)w - 1);
          continue;
        }
        HPROF("feed.insert");  // on whichever thread takes task 0; no other task touches the profile
        for (uint32_t k : fresh) {
          const size_t id = (size_t)ids[k] + currid_;
          auto it = db_.find(id);  // a new id seen by an earlier camera of this frame
          if (it == db_.end()) it = db_insert(id, new_feature(id));
          fp[k] = it->second.get();
        }
      }
    });
    if (hprof_.on) {
      auto &a = hprof_.acc["feed.db.job"];
      a.first += secs(tj0, clk::now());
      a.second++;
    }
    stock_target_ = std::min<size_t>(3 * (db_.size() - db0) / 2 + 16, 16384);
    hprof_.count("feed.new_features", (double)(db_.size() - db0));
    hprof_.count("feed.obs", (double)nobs);
    hprof_.count("feed.db_size", (double)db_.size());
    if (!fresh.empty()) {
      HPROF("feed.db.fresh");
      bucket(fresh, bk_fresh);
      pool_.parallel_for((size_t)nw, 1, [&](size_t b, size_t e) {
        for (size_t w = b; w < e; w++) append(bk_fresh, (uint32_t)w);
      });
    }
  }
  return after_tracking(t, camids, rT1);
}

// VioManager::feed_measurement_camera -> TrackKLT::feed_new_camera (TrackKLT.cpp:34-94), then the
// same propagate / update sequence as the simulated feed
int Engine::feed_camera(double t, int ncam, const int *cam_ids, const uint8_t *const *imgs, const int *strides,
                        const uint8_t *const *masks, bool device_imgs) {
  auto rT1 = clk::now();
  frame_begin();
  std::vector<int> camids;
  for (int i = 0; i < ncam; i++) {
    int cid = cam_ids[i];
    if (cid < 0 || cid >= o_.num_cameras || !imgs[i]) return UVIO_HP_E_ARG;
    camids.push_back(cid);
  }
  if (!tracker_) {
    tracker_.reset(new Tracker(o_, cams_, d_.stream, &kprof_));
    tracker_->set_host_prof(&hprof_);
  }
  // Propagator::propagate_and_clone reads nothing the tracker produces.  When nothing can run between the
  // tracking and the propagation (no zero-velocity check, no UWB range before t), the host computes it
  // while the frame's LK + RANSAC are on the device and enqueues its launches behind them: the same
  // launches in the same stream order, the host's share hidden under the tracker's wait.
  // An exception of the early propagation is held until the tracker has finished its frame (results
  // consumed, buffers flipped) and rethrown then; its host time is booked as propagation, not tracking.
  bool early = false;
  int early_rc = 0;
  std::exception_ptr early_exc;
  std::function<void()> in_flight;
  early_prop_s_ = 0.0;
  if (propagation_can_precede_tracking(t))
    in_flight = [&, t]() {
      HPROF("prop");
      early = true;
      auto p0 = clk::now();
      try {
        early_rc = propagate_and_clone(t);
      } catch (...) {
        early_exc = std::current_exception();
      }
      early_prop_s_ = secs(p0, clk::now());
    };
  {
    HPROF("track.feed");
    tracker_->feed(
        t, ncam, cam_ids, imgs, strides, masks, device_imgs,
        [this](size_t id, double tt, int cam, float u, float v, float un, float vn) {
          db_update(id, tt, (size_t)cam, u, v, un, vn);
        },
        std::move(in_flight));
  }
  if (early_exc) std::rethrow_exception(early_exc);
  if (early && early_rc) return early_rc;
  struct FrameFlag {
    bool &f;
    explicit FrameFlag(bool &x) : f(x) { f = true; }
    ~FrameFlag() { f = false; }
  } in_camera_frame(camera_frame_);
  return after_tracking(t, camids, rT1, tracker_->device_syncs, tracker_->sync_wait, true);
}

// the conditions under which after_tracking's first state change is propagate_and_clone(t)
bool Engine::propagation_can_precede_tracking(double t) const {
  if (!is_initialized_ || timestamp_ >= t) return false;
  if (o_.try_zupt && (!o_.zupt_only_at_beginning || !has_moved_since_zupt_)) return false;
  for (auto it = past_uwb_.begin(); it != past_uwb_.end() && it->first < t; it++)
    if (it->first > timestamp_) return false;
  for (auto it = past_fix_.begin(); it != past_fix_.end() && it->first < t; it++)
    if (it->first > timestamp_) return false;
  return true;
}

int Engine::after_tracking(double t, const std::vector<int> &camids, clk::time_point rT1, int track_syncs,
                           double track_wait, bool try_init) {
  HPROF("after_tracking");
  auto rT2 = clk::now();
  timing_ = uvio_hp_timing_t{};
  frame_feats_.clear();
  fix_results_.clear();
  pose_results_.clear();
  timing_.tracking = secs(rT1, rT2) - early_prop_s_;
  timing_.device_syncs = track_syncs;
  timing_.sync_wait = track_wait;
  // VioManager.cpp:308-317: a camera frame before initialization tries the initializer (the simulated
  // feed requires an initialized filter, VioManager.cpp:236-240)
  // The initializer runs single-threaded (use_multi_threading_subs off): on success it sets the state and
  // returns false, so that frame ends uninitialized and the next camera frame finds thread_init_success
  // (VioManagerHelper.cpp:91-93, 187).  The zero-velocity check of that next frame is skipped: it precedes
  // the initialization check and reads is_initialized_vio (VioManager.cpp:294, UVioManager.cpp:152).
  const bool was_initialized = is_initialized_;
  if (!is_initialized_) {
    if (!try_init || !init_success_) {
      if (try_init) try_to_initialize();
      return UVIO_HP_E_STATE;
    }
    is_initialized_ = true;
    odom_invalidate();  // the odometry cache starts from the initializer's state, published at this frame's end
  }
  // zero-velocity update (UVioManager.cpp:147-162, VioManager.cpp:291-307): on success the frame ends here
  if (was_initialized && o_.try_zupt && (!o_.zupt_only_at_beginning || !has_moved_since_zupt_)) {
    if (timestamp_ != t) did_zupt_update_ = zupt_try_update(t) == 1;
    if (did_zupt_update_) {
      // Propagator / UpdaterZeroVelocity::clean_old_imu_measurements(t + dt - 0.10)
      const double cut = t + calib_dt_->val[0] - 0.10;
      std::lock_guard<std::mutex> lk(imu_mtx_);
      if (cut >= 0) {
        auto old = [&](const ImuSample &a) { return a.t < cut; };
        imu_data_.erase(std::remove_if(imu_data_.begin(), imu_data_.end(), old), imu_data_.end());
        zupt_imu_.erase(std::remove_if(zupt_imu_.begin(), zupt_imu_.end(), old), zupt_imu_.end());
      }
      timing_.zupt = 1;
      timing_.timestamp = t;
      timing_.n_clones = (int)clones_.size();
      timing_.cov_dim = N_;
      timing_.total = secs(rT1, clk::now());
      odom_invalidate();  // VioManager.cpp:230, 303, UVioManager.cpp:161
      odom_flush();
      return 0;
    }
  }
  // The buffered UWB messages (UVioManager.cpp:178-188) and position fixes of (timestamp_, t) in ONE pass in
  // ascending time: propagate to each distinct time, then that time's chain; at equal times the UWB message goes
  // first, then the fixes in feed order.  A fix at the frame time is dropped (the UWB loop's it->first < t), and so is
  // one the state has already passed (a caller's uvio_hp_propagate overtook it).
  if (!past_uwb_.empty() || !past_fix_.empty()) {
    HPROF("uwb");
    auto u = past_uwb_.begin();
    const auto ue = past_uwb_.lower_bound(t);
    auto f = past_fix_.begin();
    const auto fe = past_fix_.upper_bound(t);
    double reached = -INFINITY;  // the time this pass has propagated the state to
    while (u != ue || f != fe) {
      if (u != ue && (f == fe || u->first <= f->first)) {
        const auto it = u++;
        if (it->first < t && it->first > timestamp_) {
          bool valid = false;
          for (auto &r : it->second)
            if (anchors_.count(r.first)) valid = true;
          if (!valid) continue;
          {
            HPROF("uwb.prop");
            if (propagate_uwb(it->first) != 0) continue;
          }
          reached = it->first;
          HPROF("uwb.chain");
          std::vector<std::pair<size_t, double>> rs;
          for (auto &r : it->second)
            if (anchors_.count(r.first)) rs.emplace_back(r.first, r.second);
          uwb_update_message(rs);
        }
        continue;
      }
      const auto it = f++;
      const double tf = it->first;
      bool run = tf < t && (tf > timestamp_ || (tf == timestamp_ && tf == reached));
      if (run && tf > timestamp_) {
        HPROF("fix.prop");
        run = propagate_uwb(tf) == 0;
        if (run) reached = tf;
      }
      const std::vector<FixMeas> &fx = it->second;
      if (!run) {
        for (const FixMeas &m : fx) (m.pose_r ? pose_results_ : fix_results_).push_back(FixResult{tf, 0.0, 2});
        continue;
      }
      HPROF("fix.chain");
      // feed order; each run of one kind is its own device chain (a change of kind ends a chain)
      for (size_t a = 0, b; a < fx.size(); a = b) {
        for (b = a + 1; b < fx.size() && (fx[b].pose_r != 0) == (fx[a].pose_r != 0); b++) {}
        if (fx[a].pose_r)
          pose_update_chain(tf, fx.data() + a, b - a);
        else
          fix_update_chain(tf, fx.data() + a, b - a);
      }
    }
    past_uwb_.erase(past_uwb_.begin(), past_uwb_.upper_bound(t));
    for (auto it = past_fix_.begin(); it != fe; it++) fix_queued_ -= (int)it->second.size();
    past_fix_.erase(past_fix_.begin(), fe);
  }
  int rc = do_feature_propagate_update(t, camids, rT2);
  if (rc == 0) odom_flush();  // the frame's snapshot for the IMU-rate odometry, if its update stage ran
  timing_.total = secs(rT1, clk::now());
  // VioManager.cpp:631-644: one row per frame that ran the whole update, times in the reference's columns
  // (the UWB ranges processed before the propagation land in "propagation", as in UVioManager.cpp:147-188)
  if (rc == 0 && timing_csv_ && timing_.n_clones >= std::min(o_.max_clone_size, 5)) {
    std::fprintf(timing_csv_, "%.15f,%.5f,%.5f,%.5f,", timestamp_ + calib_dt_->val[0], timing_.tracking,
                 timing_.propagation, timing_.msckf_update);
    if (o_.max_slam_features > 0) std::fprintf(timing_csv_, "%.5f,%.5f,", timing_.slam_update, timing_.slam_delayed);
    std::fprintf(timing_csv_, "%.5f,%.5f\n", timing_.marg, timing_.total);
    std::fflush(timing_csv_);
  }
  return rc;
}

// VioManager.cpp:323-651 (rT2: the end of tracking, UVioManager.cpp:147)
int Engine::do_feature_propagate_update(double t, const std::vector<int> &camids, clk::time_point rT2) {
  stage_ = "feature selection";
  if (timestamp_ > t) return UVIO_HP_E_ORDER;
  if (timestamp_ != t) {
    HPROF("prop");
    int rc = propagate_and_clone(t);
    if (rc) return rc;
  }
  // the device queue is in order: propagation runs on while the host builds the update batches
  // (record_timing >= 2 waits here so the stage timings are attributable)
  if (o_.record_timing >= 2) dev_sync();
  auto rT3 = clk::now();
  timing_.timestamp = t;
  timing_.propagation = secs(rT2, rT3) + early_prop_s_;  // + the propagation run during the tracking wait
  early_prop_s_ = 0.0;
  timing_.n_clones = (int)clones_.size();
  timing_.cov_dim = N_;
  if ((int)clones_.size() < std::min(o_.max_clone_size, 5)) return 0;
  if (timestamp_ != t) return 0;
  has_moved_since_zupt_ = true;

  std::vector<FeatP> feats_lost, feats_marg, feats_slam;
  auto t_sel = clk::now();
  // FeatureDatabase::features_not_containing_newer(t, false, true) and features_containing(margtimestep), then
  // VioManager.cpp:377-392's filter of the lost list (a track in one of this frame's cameras, not in the marg
  // list): per-feature flags on the pool, lists built in db_ order
  {
    const bool do_marg = (int)clones_.size() > o_.max_clone_size || (int)clones_.size() > 5;
    const double mt = do_marg ? margtimestep() : 0.0, ts = timestamp_;
    // pointers to the map's values (no shared_ptr copies: a reference-count round trip per feature
    // costs more than the scan at cfg4's database sizes); nothing inserts into db_ during the scan
    std::vector<const FeatP *> all;  // the map's values in db_ order
    std::vector<const Feature *> fs;  // the features themselves (the scan reads no map node)
    all.reserve(db_.size());
    fs.reserve(db_.size());
    {
      HPROF("select.walk");
      for (auto &kv : db_) {
        all.push_back(&kv.second);
        fs.push_back(kv.second.get());
      }
    }
    HPROF("select.flags");
    // each chunk's lost / marg lists built by the thread that flagged it (the reference-count increments
    // then hit lines that thread has just read), joined in chunk order = db_ order
    constexpr size_t kChunk = 1024;
    const size_t nchunk = (all.size() + kChunk - 1) / kChunk;
    std::vector<std::vector<FeatP>> lost_c(nchunk), marg_c(nchunk);
    pool_.parallel_for(all.size(), kChunk, [&](size_t b, size_t e) {
      std::vector<FeatP> &lo = lost_c[b / kChunk], &ma = marg_c[b / kChunk];
      for (size_t i = b; i < e; i++) {
        if (i + 8 < e) __builtin_prefetch(fs[i + 8]);
        const Feature &f = *fs[i];
        if (f.to_delete) continue;
        bool newer = false, has = false;
        for (auto &p : f.tracks) {
          newer = (!p.m.empty() && p.m.last_t() >= ts);
          if (newer) break;
        }
        if (do_marg)
          for (auto &p : f.tracks) {
            has = p.m.contains(mt);  // binary search on an in-order track
            if (has) break;
          }
        bool lost = !newer && !has;
        if (lost) {
          bool found = false;
          for (auto &p : f.tracks)
            if (std::find(camids.begin(), camids.end(), (int)p.cam) != camids.end()) {
              found = true;
              break;
            }
          lost = found;
        }
        if (lost) lo.push_back(*all[i]);
        if (has) ma.push_back(*all[i]);
      }
    });
    HPROF("select.lists");
    size_t nl = 0, nm = 0;
    for (size_t c = 0; c < nchunk; c++) nl += lost_c[c].size(), nm += marg_c[c].size();
    feats_lost.reserve(nl);
    feats_marg.reserve(nm);
    for (size_t c = 0; c < nchunk; c++) {
      std::move(lost_c[c].begin(), lost_c[c].end(), std::back_inserter(feats_lost));
      std::move(marg_c[c].begin(), marg_c[c].end(), std::back_inserter(feats_marg));
    }
    hprof_.count("select.db_size", (double)all.size());
    hprof_.count("select.lost", (double)feats_lost.size());
    hprof_.count("select.marg", (double)feats_marg.size());
  }
  std::vector<FeatP> feats_maxtracks;
  {
    HPROF("select.maxtracks");
    std::vector<FeatP> keep;
    for (auto &f : feats_marg) {
      bool reached = false;
      for (auto &p : f->tracks)
        if ((int)p.m.size() > o_.max_clone_size) {
          reached = true;
          break;
        }
      (reached ? feats_maxtracks : keep).push_back(std::move(f));  // (moves: no reference-count traffic)
    }
    feats_marg = std::move(keep);
  }
  int curr_aruco = 0;
  for (auto &l : slam_)
    if ((int)l.second->featid <= 4 * o_.max_aruco_features) curr_aruco++;
  if (o_.max_slam_features > 0 && t - startup_time_ >= o_.dt_slam_delay &&
      (int)slam_.size() < o_.max_slam_features + curr_aruco) {
    int amount = (o_.max_slam_features + curr_aruco) - (int)slam_.size();
    int valid = std::min(amount, (int)feats_maxtracks.size());
    if (valid > 0) {
      feats_slam.insert(feats_slam.end(), std::make_move_iterator(feats_maxtracks.end() - valid),
                        std::make_move_iterator(feats_maxtracks.end()));
      feats_maxtracks.erase(feats_maxtracks.end() - valid, feats_maxtracks.end());
    }
  }
  for (auto &lm : slam_) {
    auto it = db_.find(lm.second->featid);
    FeatP f2 = (it == db_.end()) ? nullptr : it->second;
    if (f2) feats_slam.push_back(f2);
    bool cur = std::find(camids.begin(), camids.end(), lm.second->unique_cam) != camids.end();
    if (!f2 && cur) lm.second->should_marg = true;
    if (lm.second->fail_count > 1) lm.second->should_marg = true;
  }
  {
    HPROF("select.marg_slam");
    marginalize_slam();
  }
  std::vector<FeatP> slam_delayed, slam_upd;
  for (auto &f : feats_slam) {
    if (slam_.find(f->featid) != slam_.end())
      slam_upd.push_back(f);
    else
      slam_delayed.push_back(f);
  }
  std::vector<FeatP> up = std::move(feats_lost);
  up.insert(up.end(), std::make_move_iterator(feats_marg.begin()), std::make_move_iterator(feats_marg.end()));
  up.insert(up.end(), std::make_move_iterator(feats_maxtracks.begin()), std::make_move_iterator(feats_maxtracks.end()));
  // VioManager.cpp:518 std::sort by measurement count (compare_feat), on the counts computed once: std::sort's
  // permutation depends only on the comparison outcomes, which are the same
  {
    HPROF("select.sort");
    std::vector<std::pair<int, FeatP>> keyed(up.size());
    for (size_t i = 0; i < up.size(); i++) keyed[i] = {up[i]->count(), std::move(up[i])};
    std::sort(keyed.begin(), keyed.end(),
              [](const std::pair<int, FeatP> &a, const std::pair<int, FeatP> &b) { return a.first < b.first; });
    for (size_t i = 0; i < up.size(); i++) up[i] = std::move(keyed[i].second);
  }
  if ((int)up.size() > o_.max_msckf_in_update) up.erase(up.begin(), up.end() - o_.max_msckf_in_update);
  // every feature the updaters may flag to_delete (the MSCKF list, SLAM updates, delayed inits); a
  // frame that returns early keeps its entries for the next frame's cleanup
  pending_delete_.insert(pending_delete_.end(), up.begin(), up.end());
  pending_delete_.insert(pending_delete_.end(), feats_slam.begin(), feats_slam.end());
  timing_.n_msckf = (int)up.size();
  if (hprof_.on) {
    auto &a = hprof_.acc["select"];
    a.first += secs(t_sel, clk::now());
    a.second++;
  }
  timing_.n_slam_delayed = (int)slam_delayed.size();
  int rc = 0;
  // FeatureDatabase::cleanup_measurements(margtimestep) of every feature the updaters do not read runs while
  // the device executes the chain: one feature's trimming is independent of the others', nothing between
  // the updates and the cleanup reads the trimmed (older than the marginalized clone) measurements of an
  // unread feature, and erasing a node keeps the other nodes' iteration order.  The held features (every
  // one handed to an updater, pending_delete_) are trimmed at the reference's point, after the chain.
  const bool do_clean = (int)clones_.size() > o_.max_clone_size;
  const double mt_clean = do_clean ? margtimestep() : 0.0;
  bool cleaned_early = false;
  std::vector<FeatP> held;
  // on every exit (a returned error or an exception included): no overlap job left behind, no feature held
  struct HeldGuard {
    Engine &e;
    std::vector<FeatP> &h;
    ~HeldGuard() {
      e.chain_overlap_ = nullptr;
      for (auto &f : h) f->held = false;
    }
  } held_guard{*this, held};
  if (do_clean) {
    held = pending_delete_;
    for (auto &f : held) f->held = true;
    chain_overlap_ = [this, mt_clean, &cleaned_early]() {
      cleanup_measurements(mt_clean, true);
      cleaned_early = true;
    };
  }
  // the three updaters as one device chain with one host wait (engine_chain.cpp); the SLAM list goes in chunks
  // of max_slam_in_update (VioManager.cpp:533-545).  The chain also carries the feature-sharded MSCKF update:
  // over RCCL its all-reduce is enqueued; the host all-reduce (a callback, for ranks that share a GPU) waits for
  // this rank's Gram in the middle of the enqueueing
  odom_invalidate();  // VioManager.cpp:526, 543
  rc = update_frame(up, slam_upd, slam_delayed, (size_t)std::max(o_.max_slam_in_update, 1));
  chain_overlap_ = nullptr;
  if (rc) return rc;
  // VioManager.cpp:555-570: the features the MSCKF update kept, cleared on the base camera's frames only
  if (camids.at(0) == 0) good_feats_.clear();
  for (const auto &d : last_msckf_)
    if (d.status == 0) good_feats_.insert(good_feats_.end(), d.p_FinG, d.p_FinG + 3);
  const auto rT6 = clk::now();
  timing_.msckf_update = chain_times_[0];
  timing_.slam_update = chain_times_[1];
  timing_.slam_delayed = chain_times_[2];
  HPROF("marg.total");
  {
    HPROF("marg.retri");
    retriangulate_active_tracks(t, camids);
  }
  for (auto &f : up) f->to_delete = true;
  // FeatureDatabase::cleanup: only features handed to an updater can carry to_delete, so they are
  // erased by key (erasing a node keeps the others' iteration order, as the reference's scan does)
  for (auto &f : pending_delete_) {
    if (!f->to_delete) continue;
    auto it = db_.find(f->featid);
    if (it != db_.end() && it->second == f) db_erase(it);
  }
  pending_delete_.clear();
  {
    HPROF("marg.anchors");
    rc = slam_change_anchors();
  }
  if (rc) return rc;
  if (do_clean) {
    HPROF("marg.cleanmeas");
    if (!cleaned_early) {
      cleanup_measurements(mt_clean, false);
    } else {
      for (auto &f : held) {  // the chain's features still in the database
        auto it = db_.find(f->featid);
        if (it == db_.end() || it->second != f) continue;
        f->clean_older_measurements(mt_clean);
        if (f->count() < 1) db_erase(it);
      }
    }
  }
  marginalize_old_clone();
  if (o_.record_timing >= 2) dev_sync();
  auto rT7 = clk::now();
  timing_.marg = secs(rT6, rT7);
  timing_.n_slam = (int)slam_.size();
  timing_.cov_dim = N_;
  if (kprof_.on) kprof_.harvest(false);
  if (timelastupdate_ != -1 && clones_.find(timelastupdate_) != clones_.end()) {
    const double *a = imu_->val + 4, *b = clones_.at(timelastupdate_)->val + 4;
    double d[3] = {a[0] - b[0], a[1] - b[1], a[2] - b[2]};
    distance_ += norm3(d);
  }
  timelastupdate_ = t;
  return 0;
}

// FeatureDatabase::cleanup_measurements (FeatureDatabase.cpp:226-243): per-feature trimming on the pool, then
// the emptied features are erased (erasing by key keeps the others' iteration order)
void Engine::cleanup_measurements(double t, bool skip_held) {
  const std::vector<Feature *> all(dense_);  // (a copy: the erasures below reorder dense_)
  std::vector<uint8_t> empty(all.size(), 0);
  pool_.parallel_for(all.size(), 1024, [&](size_t b, size_t e) {
    for (size_t i = b; i < e; i++) {
      if (i + 8 < e) __builtin_prefetch(all[i + 8], 1);
      if (skip_held && all[i]->held) continue;
      all[i]->clean_older_measurements(t);
      empty[i] = all[i]->count() < 1;
    }
  });
  for (size_t i = 0; i < all.size(); i++)
    if (empty[i]) db_erase(db_.find(all[i]->featid));
}

// StateHelper::marginalize_slam (StateHelper.cpp:631-645)
// (the landmarks of one call leave the covariance in one launch, marginalize_many)
void Engine::marginalize_slam() {
  stage_ = "marginalize_slam";
  std::vector<VarP> ms;
  for (auto it = slam_.begin(); it != slam_.end();) {
    if (it->second->should_marg && (int)it->first > 4 * o_.max_aruco_features) {
      ms.push_back(it->second);
      it = slam_.erase(it);
    } else {
      it++;
    }
  }
  marginalize_many(ms);
}

// StateHelper::marginalize_old_clone (StateHelper.cpp:618-629)
void Engine::marginalize_old_clone() {
  stage_ = "marginalize_old_clone";
  if ((int)clones_.size() > o_.max_clone_size) {
    double mt = margtimestep();
    marginalize(clones_.at(mt));
    clones_.erase(mt);
  }
}

// ---------------------------------------------------------------------------------------------------
// Batch tables: clone slots (time order), cameras, canonical columns (calib blocks, clones, landmarks)
void Engine::build_clone_cam_tables(Batch &b, bool include_landmarks) {
  b.clones.clear();
  b.cams.clear();
  b.hidx.clear();
  b.slot_of_time.clear();
  int canon = 0;
  for (int c = 0; c < o_.num_cameras; c++) {
    DCam dc{};
    const VarP &pose = calib_pose_.at(c);
    quat_2_Rot(pose->val, dc.R_ItoC);
    for (int k = 0; k < 3; k++) dc.p_IinC[k] = pose->val[4 + k];
    dc.cam = cams_[c];
    dc.pid_ext = o_.do_calib_camera_pose ? pose->id : -1;
    dc.pid_intr = o_.do_calib_camera_intrinsics ? calib_intr_.at(c)->id : -1;
    dc.canon_ext = dc.canon_intr = -1;
    if (o_.do_calib_camera_pose) {
      dc.canon_ext = canon;
      for (int k = 0; k < 6; k++) b.hidx.push_back(pose->id + k);
      canon += 6;
    }
    if (o_.do_calib_camera_intrinsics) {
      dc.canon_intr = canon;
      for (int k = 0; k < 8; k++) b.hidx.push_back(calib_intr_.at(c)->id + k);
      canon += 8;
    }
    b.cams.push_back(dc);
  }
  for (auto &c : clones_) {
    DClone d{};
    quat_2_Rot(c.second->val, d.R);
    quat_2_Rot(c.second->fej, d.Rf);
    for (int k = 0; k < 3; k++) d.p[k] = c.second->val[4 + k], d.pf[k] = c.second->fej[4 + k];
    d.pid = c.second->id;
    d.canon = canon;
    for (int k = 0; k < 6; k++) b.hidx.push_back(c.second->id + k);
    canon += 6;
    b.slot_of_time.push(c.first);  // slot = index in time order
    b.clones.push_back(d);
  }
  (void)include_landmarks;
  b.n_canon = canon;
}

// Builds the per-feature measurement / variable tables in the reference iteration order
// (get_feature_jacobian_full's x_order, UpdaterHelper.cpp:200-262) and appends them to the batch.
void add_feature(Engine *, const FeatP &f, int mode, int rep, const uvio_hp_options_t &o, const std::vector<DCam> &cams,
                        const SlotTable &slot_of_time, const std::vector<DClone> &clones, std::vector<DFeat> &feats,
                        std::vector<DMeas> &meas, std::vector<DVar> &vars, int &rows, const Var *landmark,
                        int landmark_canon) {
  DFeat F{};
  F.meas_off = (int)meas.size();
  F.var_off = (int)vars.size();
  // the updaters linearize the single inverse depth as the MSCKF inverse depth; in the SLAM updaters (not the MSCKF
  // update, UpdaterMSCKF.cpp:181-183) its two bearing columns are then projected out (DFeat::single)
  F.rep = (rep == REP_ANCHORED_INVERSE_DEPTH_SINGLE) ? REP_ANCHORED_MSCKF_INVERSE_DEPTH : rep;
  F.single = (rep == REP_ANCHORED_INVERSE_DEPTH_SINGLE && mode != 0) ? 1 : 0;
  F.mode = mode;
  // anchor (FeatureInitializer.cpp:35-45): camera with most measurements (first max in map order),
  // anchor time = its last measurement
  size_t anchor_cam = 0, most = 0;
  for (auto &p : f->tracks)
    if (p.m.size() > most) {
      anchor_cam = p.cam;
      most = p.m.size();
    }
  const CamTrack *at = f->find(anchor_cam);
  if (!at || at->m.empty()) throw HpError(UVIO_HP_E_STATE, "feature without measurements in a batch");
  double anchor_time = at->m.back().t;
  if (landmark) {
    anchor_cam = (size_t)landmark->anchor_cam;
    anchor_time = landmark->anchor_time;
  }
  F.anchor_cam = (int)anchor_cam;
  const bool rel = (rep == 2 || rep == 3 || rep == 4 || rep == 5);
  // a global landmark's anchor clone may have been marginalized (change_anchors only re-anchors relative
  // representations, UpdaterSLAM.cpp:481-500) and get_feature_jacobian_full never reads it for a global
  // representation (UpdaterHelper.cpp:226-262): slot 0 is a placeholder the kernel does not use
  const int anc = slot_of_time.find(anchor_time);
  if (anc < 0 && (rel || !landmark)) throw HpError(UVIO_HP_E_STATE, "feature anchor clone is not in the window");
  F.anchor_slot = (anc < 0) ? 0 : anc;
  int loc = 0;
  std::vector<int> clone_loc(clones.size(), -1);  // slot -> local col
  int ext_loc[UVIO_HP_MAX_CAMS], intr_loc[UVIO_HP_MAX_CAMS];
  for (int k = 0; k < UVIO_HP_MAX_CAMS; k++) ext_loc[k] = intr_loc[k] = -1;
  for (auto &p : f->tracks) {
    int c = (int)p.cam;
    if (o.do_calib_camera_pose) {
      vars.push_back(DVar{cams[c].pid_ext, cams[c].canon_ext, 6, loc});
      ext_loc[c] = loc;
      loc += 6;
    }
    if (o.do_calib_camera_intrinsics) {
      vars.push_back(DVar{cams[c].pid_intr, cams[c].canon_intr, 8, loc});
      intr_loc[c] = loc;
      loc += 8;
    }
    for (size_t m = 0; m < p.m.size(); m++) {
      int s = slot_of_time.at(p.m[m].t);
      if (clone_loc[s] < 0) {
        clone_loc[s] = loc;
        vars.push_back(DVar{clones[s].pid, clones[s].canon, 6, loc});
        loc += 6;
      }
    }
  }
  if (rel) {
    if (clone_loc[F.anchor_slot] < 0) {
      clone_loc[F.anchor_slot] = loc;
      vars.push_back(DVar{clones[F.anchor_slot].pid, clones[F.anchor_slot].canon, 6, loc});
      loc += 6;
    }
    if (o.do_calib_camera_pose && ext_loc[F.anchor_cam] < 0) {
      ext_loc[F.anchor_cam] = loc;
      vars.push_back(DVar{cams[F.anchor_cam].pid_ext, cams[F.anchor_cam].canon_ext, 6, loc});
      loc += 6;
    }
    F.lc_anchor_clone = clone_loc[F.anchor_slot];
    F.lc_anchor_ext = ext_loc[F.anchor_cam];
  }
  if (landmark) {
    F.lm_pid = landmark->id;
    F.lm_loc = loc;
    vars.push_back(DVar{landmark->id, landmark_canon, landmark->size, loc});
    loc += landmark->size;
    double p[3], pf[3];
    landmark->xyz(false, p);
    landmark->xyz(true, pf);
    for (int k = 0; k < 3; k++) F.p_in[k] = p[k], F.p_in_fej[k] = pf[k];
    if (landmark->rep == REP_ANCHORED_INVERSE_DEPTH_SINGLE)  // the anchor bearing goes with the feature (kernels.h)
      for (int k = 0; k < 3; k++) F.p_in_fej[k] = landmark->uvn0[k];
  }
  F.nf = loc;
  F.nvar = (int)vars.size() - F.var_off;
  for (auto &p : f->tracks) {
    int c = (int)p.cam;
    for (size_t m = 0; m < p.m.size(); m++) {
      const FeatMeas &fm = p.m[m];
      DMeas d{};
      d.u = fm.u;
      d.v = fm.v;
      d.un = fm.un;
      d.vn = fm.vn;
      d.cam = c;
      d.slot = slot_of_time.at(fm.t);
      d.lc_clone = clone_loc[d.slot];
      d.lc_ext = ext_loc[c];
      d.lc_intr = intr_loc[c];
      meas.push_back(d);
    }
  }
  F.nmeas = (int)meas.size() - F.meas_off;
  F.row_off = rows;
  F.rows = feat_rows_out(F);
  rows += F.rows;
  feats.push_back(F);
}

void Engine::add_feature_to_batch(Batch &b, const FeatP &f, int mode, int rep) {
  if (b.meas_dev) throw HpError(UVIO_HP_E_INTERNAL, "add_feature_to_batch: measurements already staged");
  add_feature(this, f, mode, rep, o_, b.cams, b.slot_of_time, b.clones, b.feats, b.meas, b.vars, b.rows, nullptr, -1);
}

// fv[lo, hi) appended in order.  Large batches (configs 4-5: 800-1500 features x 26-31 clones) are built
// in contiguous chunks on the pool (add_feature only reads the batch's clone / camera tables), then the
// chunks are stitched in order with their offsets shifted: the same tables as the sequential loop.
void Engine::add_features_to_batch(Batch &b, const std::vector<FeatP> &fv, size_t lo, size_t hi, int mode, int rep) {
  const size_t nf = hi - lo;
  if (nf < 256 || pool_.threads() == 1) {
    for (size_t i = lo; i < hi; i++) add_feature_to_batch(b, fv[i], mode, rep);
    return;
  }
  struct Part {
    std::vector<DFeat> feats;
    std::vector<DMeas> meas;
    std::vector<DVar> vars;
    int rows = 0;
  };
  const size_t nparts = std::min(nf / 64, (size_t)pool_.threads() * 4);
  std::vector<Part> parts(nparts);
  pool_.parallel_for(nparts, 1, [&](size_t p0, size_t p1) {
    for (size_t p = p0; p < p1; p++) {
      Part &P = parts[p];
      const size_t a = lo + nf * p / nparts, e = lo + nf * (p + 1) / nparts;
      for (size_t i = a; i < e; i++)
        add_feature(this, fv[i], mode, rep, o_, b.cams, b.slot_of_time, b.clones, P.feats, P.meas, P.vars, P.rows,
                    nullptr, -1);
    }
  });
  // the parts' measurement / variable tables go straight into the upload staging, copied in parallel
  // (no merged host copy); the batch must not hold host tables already
  if (!b.meas.empty() || !b.vars.empty() || b.meas_dev)
    throw HpError(UVIO_HP_E_INTERNAL, "add_features_to_batch: batch already holds measurements");
  std::vector<size_t> mo(nparts + 1, 0), vo(nparts + 1, 0);
  for (size_t p = 0; p < nparts; p++) {
    mo[p + 1] = mo[p] + parts[p].meas.size();
    vo[p + 1] = vo[p] + parts[p].vars.size();
  }
  // ONE reservation for both tables, filled before anything else is staged: a second reservation could
  // flush and recycle the ring while the first one is still unfilled
  const size_t mbytes = (sizeof(DMeas) * mo[nparts] + 255) / 256 * 256;
  void *hm = nullptr;
  char *dm = (char *)stage_reserve(mbytes + sizeof(DVar) * vo[nparts], &hm);
  void *hv = (char *)hm + mbytes;
  b.meas_dev = (const DMeas *)dm;
  b.vars_dev = (const DVar *)(dm + mbytes);
  b.stg_epoch = d_.stg_epoch;
  b.n_meas_dev = mo[nparts];
  b.n_vars_dev = vo[nparts];
  pool_.parallel_for(nparts, 1, [&](size_t p0, size_t p1) {
    for (size_t p = p0; p < p1; p++) {
      if (!parts[p].meas.empty())
        std::memcpy((DMeas *)hm + mo[p], parts[p].meas.data(), sizeof(DMeas) * parts[p].meas.size());
      if (!parts[p].vars.empty())
        std::memcpy((DVar *)hv + vo[p], parts[p].vars.data(), sizeof(DVar) * parts[p].vars.size());
    }
  });
  for (size_t p = 0; p < nparts; p++) {
    const int ro = b.rows;
    for (DFeat F : parts[p].feats) {
      F.meas_off += (int)mo[p];
      F.var_off += (int)vo[p];
      F.row_off += ro;
      b.feats.push_back(F);
    }
    b.rows += parts[p].rows;
  }
}

DBatchParams Engine::batch_params(const Batch &b, double sigma_pix_sq, double chi2_mult) const {
  DBatchParams bp{};
  bp.nfeat = (int)b.feats.size();
  bp.n_canon = b.n_canon;
  bp.ldh = d_.ldh;
  bp.ldp = d_.ldp;
  bp.sigma_pix_sq = sigma_pix_sq;
  bp.chi2_mult = chi2_mult;
  bp.do_fej = o_.do_fej;
  bp.calib_ext = o_.do_calib_camera_pose;
  bp.calib_intr = o_.do_calib_camera_intrinsics;
  bp.fi_max_runs = o_.fi_max_runs;
  bp.fi_refine = o_.fi_refine_features;
  bp.fi_tri1d = o_.fi_triangulate_1d;
  bp.fi_init_lamda = o_.fi_init_lamda;
  bp.fi_max_lamda = o_.fi_max_lamda;
  bp.fi_min_dx = o_.fi_min_dx;
  bp.fi_min_dcost = o_.fi_min_dcost;
  bp.fi_lam_mult = o_.fi_lam_mult;
  bp.fi_min_dist = o_.fi_min_dist;
  bp.fi_max_dist = o_.fi_max_dist;
  bp.fi_max_baseline = o_.fi_max_baseline;
  bp.fi_max_cond = o_.fi_max_cond_number;
  return bp;
}

// per-feature results of a batch whose readback has completed (after a device sync), and the kernel classes'
// FLOP / byte credit
void Engine::finish_batch(Batch &b, int mode, std::vector<DFeatOut> &outs) {
  const int nf = (int)b.feats.size();
  outs.assign(d_.fout_host + b.fout_off, d_.fout_host + b.fout_off + nf);
  if (b.finished) return;
  b.finished = true;
  if (kprof_.on) {
    // algorithmic FP64 FLOPs (SURVEY.md §8(d) F_feat: 3 Householder reflections 12 (2 m_f)(n_f + 4), chi2
    // 2 r n^2 + 2 r^2 n + r^3 / 3 per feature) split by class: reflections -> k_feature, the chi2 terms -> the chi2 group; bytes =
    // the rows each writes (k_feature) / reads with their T rows (chi2) plus the P block gathered
    double fl = 0, fb = 0, cl = 0, cb = 0;
    for (int i = 0; i < nf; i++) {
      const double rows = 2.0 * b.feats[i].nmeas, nfc = b.feats[i].nf;
      fb += 8.0 * (rows * (nfc + 1) + 4.0 * b.feats[i].nmeas);
      if (mode == 2 || outs[i].status == 1 || outs[i].status == 2) continue;
      const double r = (mode == 1) ? rows : rows - 3.0;
      if (mode != 1) fl += 12.0 * rows * (nfc + 4.0);
      if (b.chi2) {
        cl += 2.0 * r * nfc * nfc + 2.0 * r * r * nfc + r * r * r / 3.0;
        cb += 8.0 * (2.0 * r * (nfc + 1) + nfc * nfc);
      }
    }
    kprof_.credit(KC_FEATURE, fl, fb);
    if (b.chi2) kprof_.credit(KC_CHI2, cl, cb);
  }
}

// the Gram [H r]^T [H r] of the m stacked rows in H_all (upper triangle: m ncol (ncol + 1) FLOPs, H read once)
void Engine::gram(int m, int ncol, int *nch) {
  {
    KScope ks(&kprof_, KC_GRAM);
    launch_gram(d_.stream, d_.H, m, ncol, d_.ldh, d_.partials, nch);
  }
  kprof_.credit(KC_GRAM, (double)m * ncol * (ncol + 1), 8.0 * ((double)m * ncol + (double)*nch * ncol * ncol));
}

// UpdaterSLAM::change_anchors / perform_anchor_change (UpdaterSLAM.cpp:481-647)
int Engine::slam_change_anchors() {
  stage_ = "UpdaterSLAM::change_anchors";
  if ((int)clones_.size() <= o_.max_clone_size) return 0;
  double mt = margtimestep();
  // The landmarks' propagations are batched into one EKFPropagation with a block-row Phi: each
  // landmark's rows reference only its own inputs (old/new anchor clone, calibration, itself), so the
  // sequential per-landmark propagations of the reference compose to exactly this single one.
  std::vector<int> b_rows, b_iold;
  std::vector<std::vector<std::pair<int, double>>> b_phi;  // per batched row: (cov id, value)
  auto flush = [&]() {
    if (b_rows.empty()) return;
    std::unordered_map<int, int> col;
    for (size_t k = 0; k < b_iold.size(); k++) col[b_iold[k]] = (int)k;
    const int pr = (int)b_rows.size(), q = (int)b_iold.size();
    std::vector<double> Phi((size_t)pr * q, 0.0), Q((size_t)pr * pr, 0.0);
    for (int x = 0; x < pr; x++)
      for (auto &e : b_phi[x]) Phi[(size_t)x * q + col.at(e.first)] += e.second;
    cov_propagate(0, pr, b_iold, Phi, Q, &b_rows);
    b_rows.clear();
    b_iold.clear();
    b_phi.clear();
  };
  for (auto &kv : slam_) {
    VarP lm = kv.second;
    if (lm->rep == 0 || lm->rep == 1) continue;
    if (lm->anchor_time != mt) continue;
    // old / new anchor camera poses
    auto cam_pose = [&](int cam, const VarP &clone, bool fej, double *R_GtoC, double *p_CinG) {
      double Ric[9], Rgi[9], t[3];
      quat_2_Rot(calib_pose_.at(cam)->val, Ric);
      quat_2_Rot(fej ? clone->fej : clone->val, Rgi);
      m3_mul(Ric, Rgi, R_GtoC);
      m3t_vec(R_GtoC, calib_pose_.at(cam)->val + 4, t);
      const double *p = (fej ? clone->fej : clone->val) + 4;
      for (int k = 0; k < 3; k++) p_CinG[k] = p[k] - t[k];
    };
    VarP iold = clones_.at(lm->anchor_time), inew = clones_.at(timestamp_);
    int cam = lm->anchor_cam;
    double p_old[3], p_old_fej[3];
    lm->xyz(false, p_old);
    lm->xyz(true, p_old_fej);
    auto transfer = [&](bool fej, const double *pin, double *pout) {
      double Ro[9], po[3], Rn[9], pn[3], Ron[9], d[3], t[3];
      cam_pose(cam, iold, fej, Ro, po);
      cam_pose(cam, inew, fej, Rn, pn);
      m3_mul_bt(Rn, Ro, Ron);
      for (int k = 0; k < 3; k++) d[k] = po[k] - pn[k];
      m3_vec(Rn, d, t);
      double a[3];
      m3_vec(Ron, pin, a);
      for (int k = 0; k < 3; k++) pout[k] = a[k] + t[k];
    };
    double p_new[3], p_new_fej[3];
    transfer(false, p_old, p_new);
    transfer(true, p_old_fej, p_new_fej);
    // representation Jacobians (get_feature_jacobian_representation, UpdaterHelper.cpp:90-168)
    auto rep_jac = [&](const VarP &anchor, const double *pFA_in, double *Hf, double *Hanc, double *Hcal) {
      double Ric[9], Rgi[9], pIinC[3], pIinG[3], pFA[3];
      quat_2_Rot(calib_pose_.at(cam)->val, Ric);
      for (int k = 0; k < 3; k++) pIinC[k] = calib_pose_.at(cam)->val[4 + k];
      quat_2_Rot(anchor->val, Rgi);
      for (int k = 0; k < 3; k++) pIinG[k] = anchor->val[4 + k], pFA[k] = pFA_in[k];
      if (o_.do_fej) {
        double d0[3] = {pFA[0] - pIinC[0], pFA[1] - pIinC[1], pFA[2] - pIinC[2]}, t1[3], t2[3], best[3];
        m3t_vec(Ric, d0, t1);
        m3t_vec(Rgi, t1, t2);
        for (int k = 0; k < 3; k++) best[k] = t2[k] + pIinG[k];
        quat_2_Rot(anchor->fej, Rgi);
        for (int k = 0; k < 3; k++) pIinG[k] = anchor->fej[4 + k];
        double d1[3] = {best[0] - pIinG[0], best[1] - pIinG[1], best[2] - pIinG[2]}, u[3];
        m3_vec(Rgi, d1, u);
        m3_vec(Ric, u, t1);
        for (int k = 0; k < 3; k++) pFA[k] = t1[k] + pIinC[k];
      }
      double RIT[9], RCT[9], RCG[9], Sk[9], Tm[9];
      m3_transpose(Rgi, RIT);
      m3_transpose(Ric, RCT);
      m3_mul(RIT, RCT, RCG);
      double dd[3] = {pFA[0] - pIinC[0], pFA[1] - pIinC[1], pFA[2] - pIinC[2]}, w[3];
      m3t_vec(Ric, dd, w);
      skew(w, Sk);
      m3_mul(RIT, Sk, Tm);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
          Hanc[6 * i + j] = -Tm[3 * i + j];
          Hanc[6 * i + 3 + j] = (i == j);
        }
      skew(dd, Sk);
      m3_mul(RCG, Sk, Tm);
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
          Hcal[6 * i + j] = -Tm[3 * i + j];
          Hcal[6 * i + 3 + j] = -RCG[3 * i + j];
        }
      if (lm->rep == 2) {
        std::memcpy(Hf, RCG, sizeof(double) * 9);
      } else if (lm->rep == 3) {  // ANCHORED_FULL_INVERSE_DEPTH (UpdaterHelper.cpp:124-150)
        double a_rho = 1 / norm3(pFA), a_phi = acos(a_rho * pFA[2]), a_theta = atan2(pFA[1], pFA[0]);
        double sth = sin(a_theta), cth = cos(a_theta), sph = sin(a_phi), cph = cos(a_phi), rho = a_rho;
        double d[9] = {-(1.0 / rho) * sth * sph, (1.0 / rho) * cth * cph, -(1.0 / (rho * rho)) * cth * sph,
                       (1.0 / rho) * cth * sph,  (1.0 / rho) * sth * cph, -(1.0 / (rho * rho)) * sth * sph,
                       0.0, -(1.0 / rho) * sph, -(1.0 / (rho * rho)) * cph};
        m3_mul(RCG, d, Hf);
      } else if (lm->rep == 5) {  // ANCHORED_INVERSE_DEPTH_SINGLE: the 3 x 1 Jacobian (UpdaterHelper.cpp:175-186)
        const double rho = 1.0 / pFA[2];
        const double bear[3] = {rho * pFA[0], rho * pFA[1], rho * pFA[2]};
        const double dr[3] = {-(1.0 / (rho * rho)) * bear[0], -(1.0 / (rho * rho)) * bear[1], -(1.0 / (rho * rho)) * bear[2]};
        m3_vec(RCG, dr, Hf);
      } else {
        double alpha = pFA[0] / pFA[2], beta = pFA[1] / pFA[2], rho = 1 / pFA[2];
        double d[9] = {1.0 / rho, 0, -(1.0 / (rho * rho)) * alpha, 0, 1.0 / rho, -(1.0 / (rho * rho)) * beta, 0, 0,
                       -(1.0 / (rho * rho))};
        m3_mul(RCG, d, Hf);
      }
    };
    double Hf_old[9], Ha_old[18], Hc_old[18], Hf_new[9], Ha_new[18], Hc_new[18];
    double pA_old[3], pA_new_tmp[3];
    lm->xyz(false, pA_old);
    rep_jac(iold, pA_old, Hf_old, Ha_old, Hc_old);
    // new representation at the new anchor: the reference passes new_feat with p_FinA = transferred value
    std::memcpy(pA_new_tmp, p_new, sizeof(p_new));
    rep_jac(inew, pA_new_tmp, Hf_new, Ha_new, Hc_new);
    // Phi order: x_order_old (anchor clone, calib), x_order_new (new clone, calib dup), landmark
    std::vector<std::pair<int, int>> order;  // (cov id, size)
    std::vector<int> col_anchor_old, col_cal, col_anchor_new;
    int cur = 0;
    order.push_back({iold->id, 6});
    int c_old = cur;
    cur += 6;
    int c_cal = -1;
    if (o_.do_calib_camera_pose) {
      order.push_back({calib_pose_.at(cam)->id, 6});
      c_cal = cur;
      cur += 6;
    }
    int c_new = cur;
    order.push_back({inew->id, 6});
    cur += 6;
    int c_lm = cur;
    // the landmark's dimension pd: H_f is 3 x pd (row-major), H_f_new^-1 is pd x 3 and Phi has pd rows
    const int pd = lm->size;
    order.push_back({lm->id, pd});
    cur += pd;
    double Hinv[9];
    if (pd == 1) {  // the pseudo-inverse H^T / (H^T H) (UpdaterSLAM.cpp:610-618)
      const double sq = dot3(Hf_new, Hf_new);
      for (int k = 0; k < 3; k++) Hinv[k] = (1.0 / sq) * Hf_new[k];
    } else {
      double *A = Hf_new;
      double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
      Hinv[0] = (A[4] * A[8] - A[5] * A[7]) / det;
      Hinv[1] = (A[2] * A[7] - A[1] * A[8]) / det;
      Hinv[2] = (A[1] * A[5] - A[2] * A[4]) / det;
      Hinv[3] = (A[5] * A[6] - A[3] * A[8]) / det;
      Hinv[4] = (A[0] * A[8] - A[2] * A[6]) / det;
      Hinv[5] = (A[2] * A[3] - A[0] * A[5]) / det;
      Hinv[6] = (A[3] * A[7] - A[4] * A[6]) / det;
      Hinv[7] = (A[1] * A[6] - A[0] * A[7]) / det;
      Hinv[8] = (A[0] * A[4] - A[1] * A[3]) / det;
    }
    std::vector<double> Phi((size_t)pd * cur, 0.0);
    auto addblk = [&](int col, const double *H36, double sgn) {
      for (int i = 0; i < pd; i++)
        for (int j = 0; j < 6; j++) {
          double s = 0;
          for (int k = 0; k < 3; k++) s += Hinv[3 * i + k] * H36[6 * k + j];
          Phi[(size_t)i * cur + col + j] += sgn * s;
        }
    };
    addblk(c_old, Ha_old, 1.0);
    if (c_cal >= 0) addblk(c_cal, Hc_old, 1.0);
    for (int i = 0; i < pd; i++)
      for (int j = 0; j < pd; j++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += Hinv[3 * i + k] * Hf_old[pd * k + j];
        Phi[(size_t)i * cur + c_lm + j] = s;
      }
    addblk(c_new, Ha_new, -1.0);
    if (c_cal >= 0) addblk(c_cal, Hc_new, -1.0);
    std::vector<int> iold_ids;
    for (auto &o : order)
      for (int k = 0; k < o.second; k++) iold_ids.push_back(o.first + k);
    if (b_rows.size() + pd > 63 || b_iold.size() + iold_ids.size() > 256) flush();
    for (int id : iold_ids)
      if (std::find(b_iold.begin(), b_iold.end(), id) == b_iold.end()) b_iold.push_back(id);
    for (int i = 0; i < pd; i++) {
      b_rows.push_back(lm->id + i);
      std::vector<std::pair<int, double>> rowv;
      for (int c = 0; c < cur; c++)
        if (Phi[(size_t)i * cur + c] != 0.0) rowv.push_back({iold_ids[c], Phi[(size_t)i * cur + c]});
      b_phi.push_back(rowv);
    }
    lm->anchor_time = timestamp_;
    timing_.n_anchor_change++;
    lm->set_xyz(p_new, false);
    lm->set_xyz(p_new_fej, true);
  }
  flush();
  return 0;
}

// UpdaterUWB::update_single (UpdaterUWB.cpp:53-90) + UVioUpdaterHelper::get_uwb_jacobian_single
// (UVioUpdaterHelper.cpp:147-241) for one range: a message of one range
int Engine::uwb_update_single(size_t anchor_id, double range) {
  if (anchors_.find(anchor_id) == anchors_.end()) return 0;
  return uwb_update_message({{anchor_id, range}});
}

template <class F>
const double *Engine::run_mchain(int n, F &&enqueue) {
  for (int j = 0; j < n; j++)
    enqueue(j, j ? chain_region(d_.mchain_reg, d_.mchain_stride, j - 1) : nullptr, d_.mchain_row + j,
            chain_region(d_.mchain_reg, d_.mchain_stride, j));
  ++p_epoch_;
  const size_t len = (size_t)(n - 1) * d_.mchain_stride + kChainHeader + N_;
  HP_HIP(hipMemcpyAsync(d_.mchain_host, d_.mchain_reg, sizeof(double) * len, hipMemcpyDeviceToHost, d_.stream));
  dev_sync();
  return d_.mchain_host;
}

// The ranges of one message as ONE device chain (UVioManager.cpp:178-188 runs update_single per range, each
// linearized at the state the previous one left): the linearization state (IMU pose, p_IinU, the message's
// anchors) goes up once; per range k_uwb_row moves it by the previous range's dx when that was accepted (Var::update's
// formulas) and forms the row, k_chain_M forms M = P[:, I] h, k_chain_update gates chi2 = res^2 / S on the device and
// updates P and dx when accepted.  One readback returns every range's [accepted, negative diagonals, chi2, S | dx];
// the host then applies the accepted dx's to its mean in order (the same values the device state moved by), so
// each row is linearized exactly where the per-range path linearized it -- with two host waits per range (S for
// the gate, then dx) instead of one per message.
int Engine::uwb_update_message(const std::vector<std::pair<size_t, double>> &ranges) {
  stage_ = "UpdaterUWB::update_single";
  int applied = 0;
  for (size_t c0 = 0; c0 < ranges.size(); c0 += kUwbMaxRanges) {
    const int nr = (int)std::min(ranges.size() - c0, (size_t)kUwbMaxRanges);
    DUwbState st{};
    std::memcpy(st.q, imu_->val, sizeof(double) * 4);
    std::memcpy(st.p, imu_->val + 4, sizeof(double) * 3);
    std::memcpy(st.pU, p_IinU_->val, sizeof(double) * 3);
    st.s2 = o_.uwb_sigma_range * o_.uwb_sigma_range;
    st.thr = o_.uwb_chi2_multipler * chi2_table_[1];
    st.id_imu = imu_->id;
    st.id_cal = o_.do_calib_uwb_extrinsics ? p_IinU_->id : -1;
    st.nr = nr;
    for (int j = 0; j < nr; j++) {
      const VarP &an = anchors_.at(ranges[c0 + j].first);
      std::memcpy(st.anc[j], an->val, sizeof(double) * 5);
      st.range[j] = ranges[c0 + j].second;
      st.id_anc[j] = an->fixed ? -1 : an->id;
    }
    DUwbState *dst = stage(&st, 1);
    stage_flush();
    const double *host = run_mchain(nr, [&](int j, const DChainRegion *prev, DChainRow *row, DChainRegion *reg) {
      launch_uwb_row(d_.stream, dst, j, prev, row, reg);
      launch_chain_M(d_.stream, d_.P, d_.ldp, N_, row, 1, d_.ekf.M);
      launch_chain_update(d_.stream, d_.P, d_.ldp, N_, d_.ekf.M, row, 1, true, reg);
    });
    for (int j = 0; j < nr; j++) {
      const double *reg = host + (size_t)j * d_.mchain_stride;
      const DChainRegion g = chain_header(reg);
      if (g.accepted == 0.0) continue;
      if (g.neg > 0) throw HpError(UVIO_HP_E_NUMERIC, "UWB EKFUpdate: negative covariance diagonal");
      apply_dx(reg + kChainHeader);
      applied++;
    }
  }
  return applied;
}

// The position fixes of one timestamp as device chains like uwb_update_message's: the linearization state
// (IMU pose, every fix's lever arm) goes up once per chain; per fix k_fix_rows moves it by the previous fix's dx when
// that was accepted and forms H and the residual, k_chain_M forms M = P[:, I] H^T, k_chain_update factors S, gates
// chi2 on the device and updates P and dx when accepted.  One readback returns every fix's
// [accepted, negative diagonals, chi2, refused | dx]; the host then applies the accepted dx's to its mean in order.
// An aux lever arm is looked up here, at replay: its covariance offset moves when clones in front of it are
// marginalized, and a handle removed since the feed refuses its fix (status 3) without touching the state.
void Engine::fix_update_chain(double t, const FixMeas *fixes, size_t nfix) {
  stage_ = "position fix chain";
  std::vector<const FixMeas *> live;
  std::vector<size_t> slot;  // live fix -> its entry of fix_results_
  for (size_t f = 0; f < nfix; f++) {
    const FixMeas &m = fixes[f];
    fix_results_.push_back(FixResult{t, 0.0, 3});
    if (m.aux > 0) {
      auto it = aux_.find(m.aux);
      if (it == aux_.end() || it->second.v->kind != V_AUX || it->second.v->size != 3) continue;
    }
    live.push_back(&m);
    slot.push_back(fix_results_.size() - 1);
  }
  for (size_t c0 = 0; c0 < live.size(); c0 += kFixMaxChain) {
    const int nf = (int)std::min(live.size() - c0, (size_t)kFixMaxChain);
    DFixState st{};
    std::memcpy(st.q, imu_->val, sizeof(double) * 4);
    std::memcpy(st.p, imu_->val + 4, sizeof(double) * 3);
    st.id_imu = imu_->id;
    st.nf = nf;
    for (int j = 0; j < nf; j++) {
      const FixMeas &m = *live[c0 + j];
      const Var *av = m.aux > 0 ? aux_.at(m.aux).v.get() : nullptr;
      std::memcpy(st.s[j], av ? av->val : m.s, sizeof(double) * 3);
      std::memcpy(st.C[j], m.C, sizeof(m.C));
      std::memcpy(st.z[j], m.z, sizeof(m.z));
      std::memcpy(st.R[j], m.R, sizeof(m.R));
      st.thr[j] = m.thr;
      st.r[j] = m.r;
      st.id_aux[j] = av ? av->id : -1;
    }
    DFixState *dst = stage(&st, 1);
    stage_flush();
    const double *host = run_mchain(nf, [&](int j, const DChainRegion *prev, DChainRow *row, DChainRegion *reg) {
      launch_fix_rows(d_.stream, dst, j, prev, row, reg);
      launch_chain_M(d_.stream, d_.P, d_.ldp, N_, row, st.r[j], d_.ekf.M);
      launch_chain_update(d_.stream, d_.P, d_.ldp, N_, d_.ekf.M, row, st.r[j], false, reg);
    });
    bool applied = false;
    for (int j = 0; j < nf; j++) {
      const double *reg = host + (size_t)j * d_.mchain_stride;
      const DChainRegion g = chain_header(reg);
      FixResult &res = fix_results_[slot[c0 + j]];
      res.chi2 = g.chi2;
      if (g.accepted == 0.0) {
        res.status = g.extra != 0.0 ? 3 : 1;
        continue;
      }
      if (g.neg > 0) throw HpError(UVIO_HP_E_NUMERIC, "position fix EKFUpdate: negative covariance diagonal");
      apply_dx(reg + kChainHeader);
      res.status = 0;
      applied = true;
    }
    if (applied) {  // as after an applied uvio_hp_measurement_update
      odom_invalidate();
      odom_flush();
    }
  }
}

// The pose fixes of one timestamp as device chains, fix_update_chain's shape with k_pose_rows as the row kernel: the
// linearization state (IMU pose, every fix's lever arm and mounting rotation) goes up once per chain, each step is
// three launches (orientation only: the R = 3 instances, full: the R = 6 ones), one readback per chain, apply_dx per
// accepted step in order (an aux mounting rotation moves by boxplus there as on the device).  Both handles are looked
// up here, at replay; a dead or retyped one refuses its fix (status 3) without touching the state.
void Engine::pose_update_chain(double t, const FixMeas *fixes, size_t nfix) {
  stage_ = "pose fix chain";
  std::vector<const FixMeas *> live;
  std::vector<size_t> slot;  // live fix -> its entry of pose_results_
  for (size_t f = 0; f < nfix; f++) {
    const FixMeas &m = fixes[f];
    pose_results_.push_back(FixResult{t, 0.0, 3});
    if (m.aux > 0) {
      auto it = aux_.find(m.aux);
      if (it == aux_.end() || it->second.v->kind != V_AUX || it->second.v->size != 3) continue;
    }
    if (m.rot > 0) {
      auto it = aux_.find(m.rot);
      if (it == aux_.end() || it->second.v->kind != V_AUX_QUAT) continue;
    }
    live.push_back(&m);
    slot.push_back(pose_results_.size() - 1);
  }
  for (size_t c0 = 0; c0 < live.size(); c0 += kFixMaxChain) {
    const int nf = (int)std::min(live.size() - c0, (size_t)kFixMaxChain);
    DPoseState st{};
    std::memcpy(st.q, imu_->val, sizeof(double) * 4);
    std::memcpy(st.p, imu_->val + 4, sizeof(double) * 3);
    st.id_imu = imu_->id;
    st.nf = nf;
    for (int j = 0; j < nf; j++) {
      const FixMeas &m = *live[c0 + j];
      const Var *av = m.aux > 0 ? aux_.at(m.aux).v.get() : nullptr;
      const Var *rv = m.rot > 0 ? aux_.at(m.rot).v.get() : nullptr;
      std::memcpy(st.s[j], av ? av->val : m.s, sizeof(double) * 3);
      std::memcpy(st.qS[j], rv ? rv->val : m.qS, sizeof(double) * 4);
      std::memcpy(st.zq[j], m.zq, sizeof(m.zq));
      std::memcpy(st.zp[j], m.z, sizeof(m.z));
      std::memcpy(st.R[j], m.Rp, sizeof(m.Rp));
      st.thr[j] = m.thr;
      st.r[j] = m.pose_r;
      // an orientation-only fix has no lever-arm columns
      st.id_arm[j] = (av && m.pose_r == 6) ? av->id : -1;
      st.id_rot[j] = rv ? rv->id : -1;
    }
    DPoseState *dst = stage(&st, 1);
    stage_flush();
    const double *host = run_mchain(nf, [&](int j, const DChainRegion *prev, DChainRow *row, DChainRegion *reg) {
      launch_pose_rows(d_.stream, dst, j, prev, row, reg);
      launch_chain_M(d_.stream, d_.P, d_.ldp, N_, row, st.r[j], d_.ekf.M);
      launch_chain_update(d_.stream, d_.P, d_.ldp, N_, d_.ekf.M, row, st.r[j], false, reg);
    });
    bool applied = false;
    for (int j = 0; j < nf; j++) {
      const double *reg = host + (size_t)j * d_.mchain_stride;
      const DChainRegion g = chain_header(reg);
      FixResult &res = pose_results_[slot[c0 + j]];
      res.chi2 = g.chi2;
      if (g.accepted == 0.0) {
        res.status = g.extra != 0.0 ? 3 : 1;
        continue;
      }
      if (g.neg > 0) throw HpError(UVIO_HP_E_NUMERIC, "pose fix EKFUpdate: negative covariance diagonal");
      apply_dx(reg + kChainHeader);
      res.status = 0;
      applied = true;
    }
    if (applied) {  // as after an applied uvio_hp_measurement_update
      odom_invalidate();
      odom_flush();
    }
  }
}

}  // namespace uvhp
