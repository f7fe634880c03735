// Engine: what the ROS node reads after every message besides the state itself (ROS1Visualizer.cpp:245-327, 618,
// 687, 805): marginal covariance blocks gathered on the device (StateHelper::get_marginal_covariance,
// StateHelper.cpp:226-254), the frame's MSCKF features (VioManager::get_good_features_MSCKF, VioManager.h:123)
// and the IMU-rate odometry (Propagator::fast_state_propagate, Propagator.cpp:140-267; the math is fast_prop.h).
//
// The odometry cache.  The reference marks its cache invalid after a state change (invalidate_cache(),
// VioManager.cpp:230, 303, 526, 543, UVioManager.cpp:161) and refreshes it from the live state inside the first
// query that follows, a read that races with the update thread.  Here the feed thread publishes the snapshot at
// the end of the invalidating call -- the schedule in which that query follows the frame at once: the host-side
// values are stored under odom_mtx_, the IMU block of P is gathered and copied to a pinned slot on the main
// stream behind the frame's last P write, and an event marks the copy.  The feed call does not wait; a query
// adopts the snapshot first and waits for the event only if the copy is still in flight.
#include <cstring>

#include "engine.h"

namespace uvhp {

int Engine::marginal_cov(int nvar, const int *ids, const int *sizes, double *out, int ld) {
  stage_ = "get_marginal_covariance";
  if (nvar < 0) return UVIO_HP_E_ARG;
  if (nvar == 0) return 0;
  if (!ids || !sizes || !out) return UVIO_HP_E_ARG;
  long long m = 0;
  for (int k = 0; k < nvar; k++) {
    if (sizes[k] < 1 || ids[k] < 0 || (long long)ids[k] + sizes[k] > N_) return UVIO_HP_E_ARG;
    m += sizes[k];
  }
  if (m > d_.ldp) return UVIO_HP_E_CAPACITY;
  if (ld < m) return UVIO_HP_E_ARG;
  const int mi = (int)m;
  std::vector<int> idx;
  idx.reserve((size_t)mi);
  for (int k = 0; k < nvar; k++)
    for (int i = 0; i < sizes[k]; i++) idx.push_back(ids[k] + i);
  const size_t mm = (size_t)mi * mi;
  if (d_.marg.size() < mm) {  // (the old block is freed before the new one is made)
    d_.marg.reset();
    d_.marg = DevBuf<double>(mm);
    d_.marg_host.reset();
    d_.marg_host = PinBuf<double>(mm);
  }
  const int *didx = stage(idx.data(), idx.size());
  stage_flush();
  launch_marginal_gather(d_.stream, d_.P, d_.ldp, didx, mi, d_.marg);
  HP_HIP(hipMemcpyAsync(d_.marg_host, d_.marg, sizeof(double) * mm, hipMemcpyDeviceToHost, d_.stream));
  dev_sync();
  for (int i = 0; i < mi; i++) std::memcpy(out + (size_t)i * ld, d_.marg_host + (size_t)i * mi, sizeof(double) * mi);
  return 0;
}

int Engine::good_features_msckf(double *xyz_inG, int cap) const {
  const int n = (int)(good_feats_.size() / 3);
  if (xyz_inG && cap > 0) std::memcpy(xyz_inG, good_feats_.data(), sizeof(double) * 3 * std::min(n, cap));
  return n;
}

void Engine::odometry_enable(bool on) {
  if (on && !d_.odom_dev) {
    d_.odom_idx = DevBuf<int>(16);
    d_.odom_dev = DevBuf<double>(2 * DeviceBufs::kOdomSlot);
    d_.odom_host = PinBuf<double>(2 * DeviceBufs::kOdomSlot);
    for (auto &e : d_.ev_odom) e = Event::create();
    int idx[16] = {0};
    for (int k = 0; k < 15; k++) idx[k] = imu_->id + k;
    HP_HIP(hipMemcpy(d_.odom_idx, idx, sizeof(idx), hipMemcpyHostToDevice));
  }
  if (!on) {
    odom_on_.store(false);
    std::lock_guard<std::mutex> lk(odom_mtx_);
    odom_pub_.pending = false;
    odom_cache_valid_ = false;
    return;
  }
  odom_on_.store(true);
  odom_invalidate();
  odom_flush();
}

// Publishes the filter state as the cache's next content, if a call has invalidated it (feed thread only)
void Engine::odom_flush() {
  if (!odom_dirty_) return;
  odom_dirty_ = false;
  if (!odom_on_.load(std::memory_order_relaxed) || !is_initialized_) return;
  // the slot a query may be reading is the published one: the copy goes to the other
  const int slot = odom_slot_ ^ 1;
  double *dev = d_.odom_dev + (size_t)slot * DeviceBufs::kOdomSlot;
  launch_marginal_gather(d_.stream, d_.P, d_.ldp, d_.odom_idx, 15, dev);
  HP_HIP(hipMemcpyAsync(d_.odom_host + (size_t)slot * DeviceBufs::kOdomSlot, dev, sizeof(double) * DeviceBufs::kOdomSlot,
                        hipMemcpyDeviceToHost, d_.stream));
  HP_HIP(hipEventRecord(d_.ev_odom[slot], d_.stream));
  OdomSnap s;
  s.pending = true;
  s.slot = slot;
  s.t = timestamp_;
  s.t_off = calib_dt_->val[0];
  std::memcpy(s.est, imu_->val, sizeof(s.est));
  fastprop::make_calib(o_.imu_model, dw_->val, da_->val, tg_->val, qa_->val, qg_->val, &s.calib);
  std::lock_guard<std::mutex> lk(odom_mtx_);
  odom_pub_ = s;
  odom_slot_ = slot;
}

int Engine::fast_state_propagate(double t, double *state_plus, double *cov, int *ok) {
  // (the refusals are plain codes: this call runs beside the feeds and leaves the handle's error message alone)
  if (!odom_on_.load()) return UVIO_HP_E_STATE;  // the cache is off
  std::lock_guard<std::mutex> lk(odom_mtx_);
  if (odom_pub_.pending) {
    HP_HIP(hipEventSynchronize(d_.ev_odom[odom_pub_.slot]));
    odom_cache_.t = odom_pub_.t;
    odom_cache_.t_off = odom_pub_.t_off;
    std::memcpy(odom_cache_.est, odom_pub_.est, sizeof(odom_cache_.est));
    odom_cache_.calib = odom_pub_.calib;
    std::memcpy(odom_cache_.cov, d_.odom_host + (size_t)odom_pub_.slot * DeviceBufs::kOdomSlot,
                sizeof(double) * DeviceBufs::kOdomSlot);
    odom_cache_valid_ = true;
    odom_pub_.pending = false;
  }
  if (!odom_cache_valid_) return UVIO_HP_E_STATE;  // nothing published yet: the filter is not initialized
  std::vector<ImuSample> imu;
  {
    std::lock_guard<std::mutex> lk2(imu_mtx_);
    imu = imu_data_;
  }
  const fastprop::Noise nz = {o_.sigma_w * o_.sigma_w, o_.sigma_a * o_.sigma_a, o_.sigma_wb * o_.sigma_wb,
                              o_.sigma_ab * o_.sigma_ab, o_.gravity_mag};
  double sp[13], cv[144];
  const bool good = fastprop::query(odom_cache_, nz, imu, t, sp, cv);
  *ok = good ? 1 : 0;
  if (good) {
    std::memcpy(state_plus, sp, sizeof(sp));
    std::memcpy(cov, cv, sizeof(cv));
  }
  return 0;
}

}  // namespace uvhp
